"""CPU: the steering helper of the merge tests (tests/merge_steer.py) asks for what it means to ask for.

  1. the branch model on hand-written S arrays at each boundary: the floor 2^-64, the gather buckets and the dense
     gather at kSparseMax, kDirectMax and its grouped limit, kDirectRows, one group, the level-2 rounds of either
     hand-off form and the rescale, the deferred walk's batches;
  2. the placement builder on a synthetic pool, for every scenario the GPU files run: the model's prediction on the
     placed costs is the scenario's intent, guard band included, so the GPU files are known to ask for the right
     thing before they run;
  3. a NumPy emulation of the merge's own order (floors against the block, group and global minimum, column groups,
     rounds, rescale) against the plain sum on every scenario's weight pattern: the structure costs below 1e-13
     where the tests allow 1e-10 (merge_steer.W_TOL), three orders left for the device's exp and fma order.
"""
import numpy as np
import pytest

import merge_steer as M

LAM = 100.0


def synthetic_pool(T, du, n_near=700, n_mid=40, n_heavy=300, lam=LAM, seed=0):
    """Random columns with made-up costs in the three tiers (and some in the gaps, which make_pool must discard)."""
    rng = np.random.default_rng(seed)
    d = np.concatenate([[0.0], rng.uniform(0.02, M.NEAR_MAX, n_near), rng.uniform(M.MID_MIN, M.MID_MAX, n_mid),
                        rng.uniform(M.HEAVY_MIN, 3000.0, n_heavy), rng.uniform(3.5, 9.5, 20), rng.uniform(26, 79, 20),
                        -rng.uniform(0.1, 50.0, 10)])
    S = 12345.0 + lam * d
    cols = rng.normal(0, 4.0, (len(S), T, du)).astype(np.float32)
    pool = M.make_pool(cols, S, lam, 0)
    assert (len(pool.near), len(pool.mid), len(pool.heavy)) == (n_near, n_mid, n_heavy)
    assert pool.d(pool.near).max() <= M.NEAR_MAX and pool.d(pool.heavy).min() >= M.HEAVY_MIN
    return pool


def all_cases():
    """(id, grid, scenario, forms) of every scenario of the two GPU files."""
    out = []
    for name, g in M.ARM_GRIDS.items():
        if name == "lps1":
            scns = M.arm_lps1_scenarios()
        else:
            scns = M.arm_row_scenarios(name) + (M.arm_sample_scenarios() if name == "t8" else [])
        forms = ("counter",) if name in ("r257", "r530") else ("poll", "counter")
        out += [(f"arm-{name}-{s.name}", g, s, forms) for s in scns]
    for n, T in M.CHAIN_SHAPES:
        for lps in (1, 4):
            for blocks in M.CHAIN_BLOCKS:
                g = M.chain_grid(n, T, lps, blocks)
                out += [(f"chain-n{n}-lps{lps}-b{blocks}-{s.name}", g, s, ("poll", "counter"))
                        for s in M.chain_scenarios(g)]
    return out


CASES = all_cases()


# ---------------------------------------------------------------- 1: the model at its boundaries

def _S(grid, light, heavy=1.0e6):
    """S with the given {(row, slot): exponent} and everything else far away."""
    S = np.full(grid.K, heavy)
    for (r, s), e in light.items():
        S[r * grid.spr + s] = 1000.0 + LAM * e
    return S


def test_floor_and_buckets():
    g = M.Grid(K=64, T=5, du=2, lps=8)      # two rows of 32
    assert (g.rows, g.spr) == (2, 32)
    assert abs(M.FLOOR - 44.3614195558365) < 1e-12
    for cnt, bucket in ((1, "1"), (2, "2"), (3, "4"), (4, "4"), (5, "8"), (8, "8"), (9, "16"), (16, "16"),
                        (17, "dense"), (32, "dense")):
        p = M.predict(_S(g, {(0, s): 0.1 * s for s in range(cnt)}), g, LAM)
        assert p["nl"][0] == cnt and p["gather"][0] == bucket, cnt
    # the floor is relative to the block's own minimum: 44.3 is kept, 44.4 is not
    p = M.predict(_S(g, {(0, 0): 0.0, (0, 1): 44.3, (0, 2): 44.4, (1, 0): 44.3, (1, 5): 88.0}), g, LAM)
    assert list(p["nl"]) == [2, 2] and p["nrel"] == 2
    p = M.predict(_S(g, {(0, 0): 0.0, (1, 0): 44.4}), g, LAM)
    assert p["nrel"] == 1
    with pytest.raises(AssertionError):
        M.guard_band(p, g, [0])          # 44.4 decides the weighted-row count from inside the band


@pytest.mark.parametrize("name,limit", [("t8", 64), ("t64", 16), ("t128", 16)])
def test_direct_limit_and_path(name, limit):
    g = M.ARM_GRIDS[name]
    assert g.direct_limit == limit
    grouped = g.col_groups > 1
    for nw, path in ((1, "direct"), (limit, "direct"), (limit + 1, "two-level"), (g.rows, "two-level")):
        p = M.predict(_S(g, {(r, 0): 0.01 * r for r in range(nw)}), g, LAM)
        want = path if path == "two-level" else ("direct-grouped" if grouped else "direct-single")
        assert (p["nrel"], p["path"]) == (nw, want)


def test_chain_has_one_column_group():
    g = M.chain_grid(3, 5, 1, 20)     # 16 columns would make 16 column groups on the arm
    assert (g.ncol, g.col_groups, g.direct_limit) == (16, 1, 16)
    assert M.chain_grid(7, 37, 4, 70).ncol == 260


def test_rows_groups_rounds_and_rescale():
    one = M.ARM_GRIDS["g16"]
    assert M.predict(_S(one, {(3, 0): 0.0}), one, LAM)["path"] == "one-group"
    g256 = M.Grid(K=256 * 16, T=5, du=2, lps=16)
    g257 = M.ARM_GRIDS["r257"]
    assert g256.rows == 256 and g257.rows == 257
    assert M.predict(_S(g256, {(255, 0): 0.0}), g256, LAM)["path"] == "direct-grouped"
    assert M.predict(_S(g257, {(256, 0): 0.0}), g257, LAM)["path"] == "two-level"      # past kDirectRows
    # 17 group rows: one eager round of 32 in the counter form, rounds of 16 and 1 as granules
    p_c = M.predict(_S(g257, {(256, 0): 0.0}), g257, LAM, "counter")
    p_p = M.predict(_S(g257, {(256, 0): 0.0}), g257, LAM, "poll")
    assert (p_c["rounds"], p_c["rescale"], p_p["rounds"], p_p["rescale"]) == (1, False, 2, True)
    assert not M.predict(_S(g257, {(0, 0): 0.0}), g257, LAM, "poll")["rescale"]       # the minimum in round one
    g530 = M.ARM_GRIDS["r530"]
    for row, resc in ((0, False), (32 * 16 - 1, False), (32 * 16, True), (529, True)):
        p = M.predict(_S(g530, {(row, 0): 0.0}), g530, LAM, "counter")
        assert (p["rounds"], p["rescale"]) == (2, resc), row
    # the chain's four column chunks merge in rounds of 16 in either form
    c = M.Grid(K=300 * 256, T=5, du=3, lps=1, maxch=4)
    assert M.predict(_S(c, {(299, 0): 0.0}), c, LAM, "counter")["rounds"] == 2


def test_deferred_walk():
    g = M.ARM_GRIDS["t64"]
    for nw, batches in ((17, 1), (32, 1), (33, 2)):
        p = M.predict(_S(g, {(r, 0): 0.01 * r for r in range(nw)}), g, LAM, "counter")
        assert (list(p["walk"]), p["walk_batches"]) == (list(range(nw)), batches)
    # a row kept in its group whose group is dropped, and a row dropped in a kept group, are not walked
    p = M.predict(_S(g, {(0, 0): 0.0, (1, 0): 60.0, (16, 0): 70.0, (17, 0): 71.0}), g, LAM, "counter")
    assert list(p["walk"]) == [0]


# ---------------------------------------------------------------- 2, 3: every scenario on a synthetic pool

@pytest.fixture(scope="module")
def pools():
    return {}


def _placed(pools, g, scn):
    key = (g.T, g.du)
    if key not in pools:
        pools[key] = synthetic_pool(g.T, g.du)
    pool = pools[key]
    idx, light = M.build_index(scn, pool, g)
    return pool, idx, light


@pytest.mark.parametrize("cid,g,scn,forms", CASES, ids=[c[0] for c in CASES])
def test_placement_meets_the_intent(cid, g, scn, forms, pools):
    pool, idx, light = _placed(pools, g, scn)
    S = pool.S[idx]
    assert light.sum() == len(scn.places) and np.all(pool.d(idx[~light]) >= M.HEAVY_MIN)
    lightS = S[light]
    if not any(k == "tie" for _, _, k in scn.places):
        assert len(np.unique(lightS)) == len(lightS)          # distinct weights: a swapped row would show
    else:
        assert len(lightS) - len(np.unique(lightS)) == sum(k == "tie" for _, _, k in scn.places) - 1
    for form in forms:
        M.check_intent(scn, M.predict(S, g, pool.lam, form), g, form)


@pytest.mark.parametrize("cid,g,scn,forms", CASES, ids=[c[0] for c in CASES])
def test_structure_error_is_far_below_the_tolerance(cid, g, scn, forms, pools):
    pool, idx, _ = _placed(pools, g, scn)
    S, eps = pool.S[idx], pool.cols[idx]
    _, eta, N = M.plain_sum(S, eps, pool.lam)
    ref = N / eta
    for form in forms:
        for deferred in ((False, True) if (g.maxch == 1 and g.rows <= M.K_DIRECT_ROWS and form == "counter")
                         else (False,)):
            w = M.emulate(S, eps, g, pool.lam, form, deferred)
            err = np.max(np.abs(w - ref) / (M.W_TOL + M.W_TOL * np.abs(ref)))   # in units of the allowed error
            assert err < 1e-3, (form, deferred, err)


def test_emulation_sees_a_missing_rescale():
    """The comparison is sharp enough to tell: without the level-2 rescale the r530 scenarios miss the tolerance."""
    g = M.ARM_GRIDS["r530"]
    pool = synthetic_pool(g.T, g.du)
    for scn in M.arm_row_scenarios("r530"):
        idx, _ = M.build_index(scn, pool, g)
        S, eps = pool.S[idx], pool.cols[idx]
        _, eta, N = M.plain_sum(S, eps, pool.lam)
        w = M.emulate(S, eps, g, pool.lam, "counter", rescale=False)
        assert not np.allclose(w, N / eta, rtol=M.W_TOL, atol=M.W_TOL), scn.name
