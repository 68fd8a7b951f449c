"""Test helper: steer a real rollout's hand-off merge (mppi_merge.h) into a chosen branch with crafted noise.

With param_exploration = 0 a sample's cost depends on its own noise column alone, so permuting the columns of the
noise buffer permutes S: a test can put chosen costs into chosen lanes of chosen workgroups.

  pool       candidate columns, rolled out once on the device and sorted by d = (S - min S) / lambda into tiers:
             *near* d <= 3, *mid* 10 <= d <= 25, *heavy* d >= 80 (gaussian_columns, perturbed_columns, make_pool);
  placement  a Scenario lists (row, slot, kind): build_index copies pool columns there and heavy ones everywhere else;
  model      predict() applies the documented decision rules (kSparseMax, kDirectMax, kDirectRows, kGroup,
             G = threads // ncol, the floor 2^-64 relative to the block, group and global minimum) to the S of the
             steered launch: kept samples and gather per workgroup, weighted rows, path, level-2 rounds, rescale,
             the deferred walk's row list;
  guard      guard_band() asserts that no exponent that decides a claimed branch lies in (30, 50): the floor is at
             64 ln 2 = 44.36, so neither fp64 rounding nor the device's exp can flip it;
  emulate()  the merge's own order of operations (floors, groups, rounds, rescale) in NumPy, for the CPU test that
             bounds the structure's error against the plain sum.

A row is a workgroup: `spr` samples (threads // lanes per sample), sample slot s of row r is sample r * spr + s and
is owned by thread s * lanes_per_sample, so slot 64 / lanes_per_sample is the first one of the second wave.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

K_SPARSE_MAX = 16     # kSparseMax: kept samples per workgroup the epilogue gathers (buckets 1, 2, 4, 8, 16)
K_DIRECT_MAX = 16     # kDirectMax
K_DIRECT_ROWS = 256   # kDirectRows
K_GROUP = 16          # kGroup
FLOOR = 64.0 * np.log(2.0)   # a weight is kept while its exponent (S - min) / lambda is at most this (2^-64)
BAND = (30.0, 50.0)          # no deciding exponent may lie strictly inside
NEAR_MAX, MID_MIN, MID_MAX, HEAVY_MIN = 3.0, 10.0, 25.0, 80.0
# perturbation scales in units of Sigma's standard deviation.  A scale's d grows with the horizon (the fp64 oracle on
# the arm: a median |d| of 1.3 at scale 1e-1 and T = 5, of 8 at scale 1e-4 and T = 128), so the ladder runs further
# both ways than 1e-1 .. 3e-4: the first three scales fill the mid tier at T = 5 .. 8, the last five the near tier
# at T = 64 and 128
LADDER = (3.0, 1.0, 3e-1, 1e-1, 3e-2, 1e-2, 3e-3, 1e-3, 3e-4, 1e-4, 3e-5, 1e-5, 3e-6, 1e-6)
W_TOL = 1e-10   # rtol = atol of w_eps against the plain fp64 sum (test_gpu_obstacles.py's W_TOL)


# ---------------------------------------------------------------- pool

def gaussian_columns(n, T, sigma, seed):
    """n seeded columns (n, T, du) fp32 of N(0, Sigma) noise."""
    rng = np.random.default_rng(seed)
    sigma = np.asarray(sigma, dtype=np.float64)
    L = np.linalg.cholesky(sigma)
    return (rng.normal(size=(n, T, sigma.shape[0])) @ L.T).astype(np.float32)


def perturbed_columns(best, n, sigma, seed, ladder=LADDER):
    """n columns around `best` (T, du): best + scale * N(0, diag Sigma), n // len(ladder) per scale of the ladder
    (the remainder at the last scale).  fp32, as the device reads them."""
    rng = np.random.default_rng(seed)
    sd = np.sqrt(np.diag(np.asarray(sigma, dtype=np.float64)))
    per = n // len(ladder)
    scale = np.concatenate([np.full(per, s) for s in ladder] + [np.full(n - per * len(ladder), ladder[-1])])
    z = rng.normal(size=(n,) + best.shape) * sd
    return (best.astype(np.float64)[None] + scale[:, None, None] * z).astype(np.float32)


@dataclass
class Pool:
    cols: np.ndarray      # (n, T, du) fp32
    S: np.ndarray         # (n,) the device's cost of each column
    lam: float
    best: int             # the column of the pool's minimum
    near: np.ndarray      # column indices, ascending d, distinct costs, without `best`
    mid: np.ndarray
    heavy: np.ndarray

    def d(self, idx):
        return (self.S[idx] - self.S[self.best]) / self.lam


def make_pool(cols, S, lam, centre):
    """Tiers of the candidates by d = (S - min S) / lambda.  Candidates that beat `centre` (the column the
    perturbations were made around) are discarded with the rest, so the centre stays the minimum and the small
    scales of the ladder stay near it; within a tier every cost is distinct."""
    S = np.asarray(S, dtype=np.float64)
    assert np.all(np.isfinite(S))
    d = (S - S[centre]) / lam
    order = np.argsort(d, kind="stable")
    order = order[d[order] > 0.0]
    _, first = np.unique(S[order], return_index=True)
    order = order[np.sort(first)]
    dd = d[order]
    return Pool(cols, S, float(lam), int(centre), order[dd <= NEAR_MAX], order[(dd >= MID_MIN) & (dd <= MID_MAX)],
                order[dd >= HEAVY_MIN])


def spread(pool, tier, n):
    """n distinct members of a tier (ascending d) whose d are spread evenly over the tier's range, so that their
    weights differ visibly: each target value takes the nearest member not taken yet."""
    assert len(tier) >= n, f"tier holds {len(tier)} columns, the scenario needs {n}"
    if n == 0:
        return tier[:0]
    d = pool.d(tier)
    free = np.ones(len(tier), bool)
    out = []
    for p in np.searchsorted(d, np.linspace(d[0], d[-1], n)).clip(0, len(tier) - 1):
        cand = np.flatnonzero(free)
        j = cand[np.argmin(np.abs(cand - p))]
        free[j] = False
        out.append(tier[j])
    return np.array(out)


# ---------------------------------------------------------------- geometry and scenarios

@dataclass(frozen=True)
class Grid:
    """One launch geometry.  ncol = T * du + 1 merged columns in maxch column chunks (arm 1, chain 4)."""
    K: int
    T: int
    du: int
    lps: int
    threads: int = 256
    maxch: int = 1

    @property
    def spr(self):
        return self.threads // self.lps

    @property
    def rows(self):
        return -(-self.K // self.spr)

    @property
    def ncol(self):
        return self.T * self.du + 1

    @property
    def groups(self):
        return -(-self.rows // K_GROUP)

    @property
    def col_groups(self):      # direct_merge's G
        return max(1, self.threads // self.ncol) if self.maxch == 1 else 1

    @property
    def direct_limit(self):
        G = self.col_groups
        return min(64, 2 * K_DIRECT_MAX * G) if G > 1 else K_DIRECT_MAX

    def row_len(self, r):
        return min(self.spr, self.K - r * self.spr)


@dataclass
class Scenario:
    """Light samples as (row, slot, kind): kind "best" (the pool's minimum, at most once unless tied), "near", "mid",
    or "tie" (every "tie" place gets the same near column).  Everything else is heavy.  path / rescale / rounds:
    the intent the model's prediction must equal."""
    name: str
    places: list
    path: str                       # "one-group", "direct-single", "direct-grouped", "two-level"
    rescale: bool = False           # a level-2 round after the first lowers the running minimum
    rounds: dict = field(default_factory=dict)   # hand-off form -> level-2 rounds, where the scenario claims them

    def light_rows(self):
        return sorted({r for r, _, _ in self.places})

    def light_count(self):
        out = {}
        for r, _, _ in self.places:
            out[r] = out.get(r, 0) + 1
        return out


def one_per_row(grid, rows, best_row=None, mid_rows=()):
    """One light sample in each of `rows`, its slot walking through the row (slot = 5 r mod row length)."""
    places = []
    for r in rows:
        kind = "best" if r == best_row else ("mid" if r in mid_rows else "near")
        places.append((r, (5 * r) % grid.row_len(r), kind))
    return places


def build_index(scn, pool, grid):
    """(idx (K,) pool column of every sample, light (K,) bool).  Heavy columns fill what the scenario leaves; light
    ones are drawn without reuse (spread over their tier), except the tied ones."""
    idx = np.resize(pool.heavy, grid.K).copy()
    assert len(pool.heavy) >= 1, "no heavy column in the pool"
    light = np.zeros(grid.K, bool)
    kinds = [k for _, _, k in scn.places]
    assert kinds.count("best") <= 1
    near = iter(spread(pool, pool.near, kinds.count("near") + (1 if "tie" in kinds else 0)))
    mid = iter(spread(pool, pool.mid, kinds.count("mid")))
    tie = next(near) if "tie" in kinds else None
    for r, s, kind in scn.places:
        assert 0 <= r < grid.rows and 0 <= s < grid.row_len(r), (r, s)
        k = r * grid.spr + s
        assert not light[k], f"two places at row {r} slot {s}"
        light[k] = True
        idx[k] = pool.best if kind == "best" else tie if kind == "tie" else next(near if kind == "near" else mid)
    return idx, light


# ---------------------------------------------------------------- the branch model

def _bucket(nl):
    return "dense" if nl > K_SPARSE_MAX else str(next(b for b in (1, 2, 4, 8, 16) if nl <= b))


def predict(S, grid, lam, form="poll"):
    """The merge's decisions for a launch with costs S on `grid` in hand-off form `form` ("poll": granules,
    "counter").  Exponents are (x - min) / lambda >= 0; kept means exponent <= FLOOR."""
    S = np.asarray(S, dtype=np.float64)
    assert S.shape == (grid.K,)
    n, spr = grid.rows, grid.spr
    pad = np.full(n * spr, np.inf)
    pad[:grid.K] = S
    rowsS = pad.reshape(n, spr)
    rho = rowsS.min(1)
    e_sample = (rowsS - rho[:, None]) / lam                     # vs the block minimum
    nl = (e_sample <= FLOOR).sum(1)
    e_row = (rho - rho.min()) / lam                             # vs the global minimum
    nrel = int((e_row <= FLOOR).sum())
    ng = grid.groups
    gpad = np.full(ng * K_GROUP, np.inf)
    gpad[:n] = rho
    rho_g = gpad.reshape(ng, K_GROUP).min(1)
    e_in_group = (rho - np.repeat(rho_g, K_GROUP)[:n]) / lam    # vs the group minimum
    e_group = (rho_g - rho.min()) / lam
    if ng == 1:
        path = "one-group"
    elif n <= K_DIRECT_ROWS and nrel <= grid.direct_limit:
        path = "direct-grouped" if grid.col_groups > 1 else "direct-single"
    else:
        path = "two-level"
    # level 2: the group rows in rounds of 32 (counter form, one column chunk: the eager form) or 16
    R1 = 32 if (form == "counter" and grid.maxch == 1) else 16
    rounds, rescale, run = 0, False, np.inf
    if path in ("one-group", "two-level"):
        rows2 = rho_g if not (path == "one-group" and form == "poll") else rho   # one group, granules: its rows
        for r0 in range(0, len(rows2), R1):
            m = rows2[r0:r0 + R1].min()
            rescale |= bool(m < run and np.isfinite(run))
            run = min(run, m)
            rounds += 1
    # the deferred finish's two-level walk (n <= kDirectRows): the rows kept in their group whose group is kept
    walk = np.flatnonzero((e_in_group <= FLOOR) & (np.repeat(e_group, K_GROUP)[:n] <= FLOOR))
    return dict(nl=nl, gather=[_bucket(int(x)) for x in nl], nrel=nrel, path=path, rounds=rounds, rescale=rescale,
                walk=walk, walk_batches=-(-len(walk) // 32), e_sample=e_sample, e_row=e_row, e_in_group=e_in_group,
                e_group=e_group, rho=rho, rho_g=rho_g)


def guard_band(p, grid, light_rows):
    """Every exponent that decides something a scenario claims lies outside BAND: the samples of the light rows
    against their block minimum, every row against the global minimum, the rows of a group that holds a light row
    against the group minimum, every group against the global minimum.  (Heavy rows among themselves decide nothing
    a scenario claims: whatever they keep is dropped against the global minimum, far beyond the band.)"""
    def clear(e):
        e = np.asarray(e)[np.isfinite(e)]
        return not np.any((e > BAND[0]) & (e < BAND[1]))
    lr = np.asarray(light_rows, dtype=int)
    in_light_group = np.isin(np.arange(grid.rows) // K_GROUP, np.unique(lr // K_GROUP))
    assert clear(p["e_sample"][lr]), "a sample of a light row is within the band of its block minimum"
    assert clear(p["e_row"]), "a row is within the band of the global minimum"
    assert clear(p["e_in_group"][in_light_group]), "a row is within the band of its group's minimum"
    assert clear(p["e_group"]), "a group is within the band of the global minimum"


def check_intent(scn, p, grid, form):
    """The prediction is the scenario's intent: the kept samples of every light row are its light samples, the
    weighted rows are the light rows, the path, and (where claimed) the level-2 rounds and the rescale."""
    want = scn.light_count()
    for r, cnt in want.items():
        assert p["nl"][r] == cnt, f"{scn.name}: row {r} keeps {p['nl'][r]} samples, intended {cnt}"
        assert p["gather"][r] == _bucket(cnt)
    assert p["nrel"] == len(want), f"{scn.name}: {p['nrel']} weighted rows, intended {len(want)}"
    assert sorted(np.flatnonzero(p["e_row"] <= FLOOR)) == sorted(want)
    assert p["path"] == scn.path, f"{scn.name}: path {p['path']}, intended {scn.path}"
    assert p["rescale"] == scn.rescale, f"{scn.name}: rescale {p['rescale']}, intended {scn.rescale}"
    if form in scn.rounds:
        assert p["rounds"] == scn.rounds[form]
    guard_band(p, grid, scn.light_rows())


# ---------------------------------------------------------------- reference and emulation

def plain_sum(S, eps, lam):
    """(rho, eta, N (T, du)) of control.py:112-118 in plain fp64: no floor, no groups, no rounds."""
    S = np.asarray(S, dtype=np.float64)
    rho = S.min()
    e = np.exp(-(S - rho) / lam)
    return rho, e.sum(), np.tensordot(e, np.asarray(eps, dtype=np.float64), axes=(0, 0))


def _merge_rows(rho, eta, N, lam, R1, rescale=True):
    """merge_rows_block: rounds of R1 rows, floor against the running minimum, online rescale (rescale=False: the
    merge as it would be without it, for the CPU test that shows the comparison would notice)."""
    acc, a_eta, run = np.zeros_like(N[0]), 0.0, np.inf
    for r0 in range(0, len(rho), R1):
        rr = rho[r0:r0 + R1]
        rnew = min(run, rr.min())
        s = np.exp((rnew - rr) / lam)
        s = np.where(s >= 2.0 ** -64, s, 0.0)
        if rescale and rnew < run and np.isfinite(run):
            f = np.exp((rnew - run) / lam)
            acc, a_eta = acc * f, a_eta * f
        run = rnew
        for i in np.flatnonzero(s):
            acc = acc + s[i] * N[r0 + i]
            a_eta = a_eta + s[i] * eta[r0 + i]
    return run, a_eta, acc


def emulate(S, eps, grid, lam, form="poll", deferred=False, rescale=True):
    """w_eps (T, du) in the merge's own order: the workgroup rows with the floor against the block minimum, then
    the path predict() names (deferred: the deferred finish's, direct or its two-level walk)."""
    S = np.asarray(S, dtype=np.float64)
    eps = np.asarray(eps, dtype=np.float64)
    n, spr = grid.rows, grid.spr
    rho, eta, N = np.empty(n), np.empty(n), np.empty((n,) + eps.shape[1:])
    for r in range(n):
        s, e = S[r * spr:(r + 1) * spr], eps[r * spr:(r + 1) * spr]
        rho[r] = s.min()
        w = np.exp((rho[r] - s) / lam)
        w = np.where(w >= 2.0 ** -64, w, 0.0)
        eta[r], N[r] = w.sum(), np.tensordot(w, e, axes=(0, 0))
    p = predict(S, grid, lam, form)
    path = p["path"]
    if deferred and path == "one-group":
        path = "two-level"          # deferred_merge takes the direct merge only beyond one group
    if path.startswith("direct"):
        s = np.exp((rho.min() - rho) / lam)
        s = np.where(s >= 2.0 ** -64, s, 0.0)
        k = np.flatnonzero(s)
        G = grid.col_groups          # weighted row j goes to column group j mod G; the groups fold in order
        a_eta = sum(sum(s[i] * eta[i] for i in k[g::G]) for g in range(G))
        acc = sum(sum(s[i] * N[i] for i in k[g::G]) for g in range(G))
        return acc / a_eta
    R1 = 32 if (form == "counter" and grid.maxch == 1) else 16
    if path == "one-group" and form == "poll":
        _, a_eta, acc = _merge_rows(rho, eta, N, lam, R1)
        return acc / a_eta
    g_rho, g_eta, g_N = [], [], []
    for g0 in range(0, n, K_GROUP):
        r, e, a = _merge_rows(rho[g0:g0 + K_GROUP], eta[g0:g0 + K_GROUP], N[g0:g0 + K_GROUP], lam, R1)
        g_rho.append(r), g_eta.append(e), g_N.append(a)
    _, a_eta, acc = _merge_rows(np.array(g_rho), np.array(g_eta), np.array(g_N), lam, 16 if deferred else R1, rescale)
    return acc / a_eta


# ---------------------------------------------------------------- the catalogue: the arm

def _pick(rows, must, n):
    """n rows of range(rows) that include `must`, the others spread evenly."""
    must = sorted(set(must))
    rest = [r for r in range(rows) if r not in must]
    take = n - len(must)
    assert 0 <= take <= len(rest)
    extra = [rest[i] for i in np.linspace(0, len(rest) - 1, take).round().astype(int)] if take else []
    out = sorted(set(must) | set(extra))
    assert len(out) == n, "the spread picked a row twice"
    return out


ARM_GRIDS = {
    # T = 8: 17 columns, G = 15 column groups, limit 64; 70 rows in five groups, the last of 6 rows, the last row partial
    "t8": Grid(K=2230, T=8, du=2, lps=8),
    # T = 64: 129 columns, one column group, limit 16; 40 rows
    "t64": Grid(K=1280, T=64, du=2, lps=8),
    # T = 128: 257 columns force 512 threads; 20 rows, the last partial
    "t128": Grid(K=630, T=128, du=2, lps=16, threads=512),
    "g8": Grid(K=256, T=5, du=2, lps=8),
    "g16": Grid(K=506, T=5, du=2, lps=8),
    # more rows than the direct merge scans: 257 (17 group rows) and 530 (34: the counter form's final merge takes
    # rounds of 32 and 2; 530 * 256 lanes are past the 512-thread threshold, so 32 samples per row)
    "r257": Grid(K=4105, T=5, du=2, lps=16),
    "r530": Grid(K=16950, T=5, du=2, lps=16, threads=512),
    # one lane per sample: 256 samples per row, the dense gather's four passes per lane; 18 rows, the last partial
    "lps1": Grid(K=4500, T=7, du=2, lps=1),
}


def arm_row_scenarios(name):
    """The row-level scenarios of ARM_GRIDS[name]: one light sample per light row."""
    g = ARM_GRIDS[name]
    n = g.rows
    one = lambda rows, **kw: one_per_row(g, rows, **kw)   # noqa: E731
    if name == "t8":
        assert (n, g.groups, g.col_groups, g.direct_limit, g.row_len(69)) == (70, 5, 15, 64, 22)
        edge = [0, 15, 16, 63, 64, 69]     # a group edge, the lane-slot edge of rho_l[j], the partial last row
        return [
            Scenario("w1", one([37], best_row=37), "direct-grouped"),
            Scenario("w2", one([0, 69], best_row=69), "direct-grouped"),
            Scenario("w16", one(_pick(n, edge, 16), best_row=16), "direct-grouped"),
            Scenario("w17", one(_pick(n, edge, 17), best_row=63), "direct-grouped"),
            Scenario("w64", one(_pick(n, edge, 64), best_row=64), "direct-grouped"),
            # the minimum in the last group behind mid-tier rows, direct and through the group rows (five group
            # rows: one level-2 round in either form, so no rescale at this size; r530 has the second round)
            Scenario("w17-min-last", one(_pick(n, edge, 17), best_row=69, mid_rows=(0, 15, 16, 33)), "direct-grouped"),
            Scenario("w65", one(_pick(n, edge, 65), best_row=15), "two-level", rounds={"poll": 1, "counter": 1}),
            Scenario("w65-min-last", one(_pick(n, edge, 65), best_row=69, mid_rows=(0, 15, 16, 33, 63)), "two-level"),
            Scenario("w70", one(range(n), best_row=66, mid_rows=(1, 17, 64)), "two-level"),
            # one light column in three rows (across a group edge) and twice within one row
            Scenario("ties", [(10, 3, "tie"), (15, 31, "tie"), (16, 0, "tie"), (40, 7, "tie"), (40, 8, "tie"),
                              (52, 9, "best")], "direct-grouped"),
        ]
    if name == "t64":
        assert (n, g.groups, g.col_groups, g.direct_limit) == (40, 3, 1, 16)
        return [
            Scenario("w1", one([39], best_row=39), "direct-single"),
            Scenario("w16", one(_pick(n, [0, 15, 16, 39], 16), best_row=16), "direct-single"),
            Scenario("w17", one(_pick(n, [0, 15, 16, 39], 17), best_row=15), "two-level"),
            # the batch edge of deferred_merge's walk (32 row loads in flight)
            Scenario("w32", one(_pick(n, [0, 15, 16, 31, 32, 39], 32), best_row=32), "two-level"),
            Scenario("w33", one(_pick(n, [0, 15, 16, 31, 32, 39], 33), best_row=39, mid_rows=(0, 16)), "two-level"),
        ]
    if name == "t128":
        assert (n, g.groups, g.col_groups, g.direct_limit, g.row_len(19)) == (20, 2, 1, 16, 22)
        return [
            Scenario("w16", one(_pick(n, [0, 15, 16, 19], 16), best_row=19), "direct-single"),
            Scenario("w17", one(_pick(n, [0, 15, 16, 19], 17), best_row=16, mid_rows=(15,)), "two-level"),
        ]
    if name in ("g8", "g16"):
        assert n == (8 if name == "g8" else 16) and g.groups == 1
        return [
            Scenario("w1", one([n - 1], best_row=n - 1), "one-group"),
            Scenario("all", one(range(n), best_row=n - 1, mid_rows=(0, 3)), "one-group"),
        ]
    if name in ("r257", "r530"):
        assert (n, g.groups) == ((257, 17) if name == "r257" else (530, 34))
        last = n - 1
        # r530: the minimum sits in group 33, the second level-2 round of the counter form (rounds of 32 and 2),
        # behind weighted near and mid rows of the first round: the running sums are rescaled
        two = name == "r530"
        rounds = {"counter": 2 if two else 1}
        return [
            Scenario("w1", one([last], best_row=last), "two-level", rescale=two, rounds=rounds),
            Scenario("w17", one(_pick(n, [0, 15, 16, 255, 256, last], 17), best_row=last, mid_rows=(0, 16)),
                     "two-level", rescale=two, rounds=rounds),
            Scenario("all", one(range(n), best_row=last, mid_rows=(0, 16, 255, 256)), "two-level", rescale=two,
                     rounds=rounds),
        ]
    raise KeyError(name)


# light samples per row, and where: the first slot, the last, either side of every wave edge of the workgroup
SAMPLE_COUNTS = (1, 2, 3, 5, 9, 16, 17, 32)


def _slots(g, row, cnt):
    """cnt slots of a row: the first, the last, both sides of each wave edge, then the rest in order."""
    L = g.row_len(row)
    per_wave = 64 // g.lps
    pref = [0, L - 1] + [s for e in range(per_wave, L, per_wave) for s in (e - 1, e)]
    seen, order = set(), []
    for s in pref + list(range(L)):
        if 0 <= s < L and s not in seen:
            seen.add(s)
            order.append(s)
    return sorted(order[:cnt])


def arm_sample_scenarios():
    """grid t8 (8 lanes per sample, 32 samples per row, waves of 8 samples): each count alone in row 16 (the first
    row of the second group; the minimum in it, so it is the one weighted row), then all of them in one launch,
    with every sample of the partial last row."""
    g = ARM_GRIDS["t8"]
    out = []
    for cnt in SAMPLE_COUNTS:
        places = [(16, s, "best" if i == 0 else "near") for i, s in enumerate(_slots(g, 16, cnt))]
        out.append(Scenario(f"s{cnt}", places, "direct-grouped"))
    rows = (2, 9, 15, 16, 30, 47, 63, 64)
    places = [(r, s, "mid" if (i == 1 and cnt > 1) else "near") for r, cnt in zip(rows, SAMPLE_COUNTS)
              for i, s in enumerate(_slots(g, r, cnt))]
    places += [(69, s, "best" if s == 21 else "near") for s in range(g.row_len(69))]
    out.append(Scenario("mixed", places, "direct-grouped"))
    return out


def arm_lps1_scenarios():
    """grid lps1 (256 samples per row): 17 light samples in one row (the first dense count), every sample of
    another, one in the last slot of the partial last row."""
    g = ARM_GRIDS["lps1"]
    assert (g.rows, g.groups, g.row_len(17)) == (18, 2, 148)
    places = [(3, s, "near") for s in _slots(g, 3, 17)] + [(10, s, "near") for s in range(256)]
    places += [(17, 147, "best")]
    return [Scenario("17-and-256", places, "direct-grouped")]


# ---------------------------------------------------------------- the catalogue: the chain

CHAIN_SHAPES = ((3, 5), (7, 37))                               # (links, T): 16 and 260 columns in four chunks
CHAIN_FORMS = (("f32", 1), ("f32", 4), ("f64", 1))             # (precision, lanes per sample)
CHAIN_BLOCKS = (20, 70)


def chain_grid(n, T, lps, blocks):
    """`blocks` workgroups of 256 threads, the last one partial."""
    spr = 256 // lps
    return Grid(K=blocks * spr - spr // 3, T=T, du=n, lps=lps, maxch=4)


def chain_scenarios(g):
    """The chain's direct merge has one column group, limit 16, and no deferred form."""
    n = g.rows
    assert g.col_groups == 1 and g.direct_limit == 16 and g.groups in (2, 5)
    one = lambda rows, **kw: one_per_row(g, rows, **kw)   # noqa: E731
    last = n - 1
    edge = [0, 15, 16, last]
    out = [
        Scenario("w1", one([last], best_row=last), "direct-single"),
        Scenario("w16", one(_pick(n, edge, 16), best_row=16), "direct-single"),
        Scenario("w17", one(_pick(n, edge, 17), best_row=15, mid_rows=(16,)), "two-level"),
        Scenario("all", one(range(n), best_row=last, mid_rows=(0, 16)), "two-level"),
    ]
    if n >= 33:
        out.append(Scenario("w33-min-last", one(_pick(n, edge + [31, 32], 33), best_row=last, mid_rows=(0, 16, 32)),
                            "two-level"))
    # samples per row: 1, 9, 16, 17 and every sample, in one launch
    places = [(r, s, "near") for r, cnt in ((1, 1), (5, 9), (15, 16), (16, 17)) for s in _slots(g, r, cnt)]
    places += [(last, s, "best" if s == 0 else "near") for s in range(g.row_len(last))]
    places += [(8, s, "near") for s in range(g.spr)]
    out.append(Scenario("samples", places, "direct-single"))
    return out
