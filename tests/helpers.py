"""What the test files share besides conftest.py's fixtures: the clamp_* / obst_* / asym_* fixture plumbing, run.py's
constants, the asymmetric arm cases and non-uniform chains, the chain tests' uniform chain and Sigma, the cases of the
chain's fused update (UPDATE_*: test_gpu_chain_update.py and test_chain_update_cpu.py) and the GPU tests' helpers (torch
and the package are imported inside the functions, so this module imports without either).

The yardsticks themselves live in ``oracle/``: ``mppi_oracle.py`` (the arm, with torque limits and workspace
obstacles, at rest or moving; the one collision-cost loop and step of either model, ``discs_at``, ``moving_masks``)
and ``chain_oracle.py`` (the chain, with torque limits, the same obstacles through ``chain_collides`` and
self-collision through ``chain_self_collides``; ``chain_segment_test``, ``chain_touch_mask``, ``chain_moving_masks``,
``chain_self_test``), pinned to these fixtures by
test_oracle_golden.py, test_clamp_cpu.py, test_chain_clamp_cpu.py, test_obstacle_cpu.py, test_chain_obstacle_cpu.py,
test_moving_obstacle_cpu.py, test_chain_moving_obstacle_cpu.py and test_chain_oracle.py (the self-collision predicate
by test_chain_self_collision_cpu.py).
"""
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN, ctor_kwargs


def _names(prefix):
    return sorted(os.path.basename(f)[len(prefix):-4] for f in glob.glob(os.path.join(GOLDEN, prefix + "*.npz")))


# the fixtures' names (tests/conftest.py globs step_* / loop_* into the plain tests: these keep clear of both)
CLAMP_STEPS = _names("clamp_step_")
OBST_STEPS = _names("obst_step_")


def load_clamp_step(name):
    return dict(np.load(os.path.join(GOLDEN, f"clamp_step_{name}.npz")))


def load_clamp_loop(name):
    return dict(np.load(os.path.join(GOLDEN, f"clamp_loop_{name}.npz")))


def load_obst_step(name):
    return dict(np.load(os.path.join(GOLDEN, f"obst_step_{name}.npz")))


def load_obst_loop(name):
    return dict(np.load(os.path.join(GOLDEN, f"obst_loop_{name}.npz")))


ASYM_STEPS = _names("asym_step_")


def load_asym_step(name):
    return dict(np.load(os.path.join(GOLDEN, f"asym_step_{name}.npz")))


def load_asym_loop(name):
    return dict(np.load(os.path.join(GOLDEN, f"asym_loop_{name}.npz")))


RUNPY = dict(param_exploration=0.0, param_lambda=100.0, param_alpha=0.98, sigma=np.eye(2) * 20.0,
             stage_cost_weight=np.array([0.5, 0.5, 5.0, 5.0]),
             terminal_cost_weight=np.array([5.0, 5.0, 50.0, 50.0]))
X0 = np.array([1.152198236517471885e00, -1.266101672070702344e00, 0.0, 0.0])


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    """Imported by a GPU test module: skips it without a device, selects device 0."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)


def _urel(a, b):
    return float(np.max(np.abs(a - b)) / max(1.0, float(np.max(np.abs(b)))))


def _inside(u, lo, hi):
    return bool(np.all((u >= lo) & (u <= hi)))


def _window(paths, prev=0):
    return paths["xydq_circle"][prev:prev + 30]


def _engine(K, T, lps=0, K_total=None, k_offset=0, u_min=None, u_max=None, clamp_nominal=True, **over):
    """The arm's engine with run.py's parameters, `over` replacing any of RUNPY's."""
    from mppi_robotarm_amd.engine import RolloutEngine
    from mppi_robotarm_amd.params import ArmParams
    kw = dict(RUNPY)
    kw.update(over)
    return RolloutEngine(K, T, 0.006, kw["param_lambda"], kw["param_alpha"], kw["sigma"],
                         kw["stage_cost_weight"], kw["terminal_cost_weight"], kw["param_exploration"],
                         ArmParams(), K_total=K_total, k_offset=k_offset, device=0, lanes_per_sample=lps,
                         u_min=u_min, u_max=u_max, clamp_nominal=clamp_nominal)


def _chains(n):
    """n uniform slender links of 1 kg and 2 m total reach (config 5's arm at n = 7): the engine's and the oracle's."""
    import chain_oracle as CO
    import mppi_robotarm_amd.chain as chain_mod
    L = 2.0 / n
    kw = dict(m=(1.0,) * n, l=(L,) * n, lc=(L / 2,) * n, I=(L * L / 12.0,) * n, fk=(L,) * n, J=(0.1,) * n, b=(1.0,) * n)
    return chain_mod.ChainParams(**kw), CO.ChainParams(**kw)


def _sigma(n):
    """The chain tests' Sigma: config 5's at n = 7, a diagonal ramp otherwise."""
    from mppi_robotarm_amd.chain import CHAIN7_SIGMA
    return CHAIN7_SIGMA.copy() if n == 7 else np.diag(np.linspace(8.0, 1.0, n))


def _ctrl(g, paths, **kw):
    """The drop-in controller of a step fixture, at the fixture's u_prev and waypoint index, with the fixture's
    trajectory switch, limits and discs where it has them."""
    from mppi_robotarm_amd.controller import MPPIControllerForPathTracking
    opt = ctor_kwargs(g)
    if "visualize_optimal_traj" in g:
        opt["visualize_optimal_traj"] = bool(g["visualize_optimal_traj"])
    if "u_min" in g:
        opt.update(u_min=g["u_min"], u_max=g["u_max"])
    if "obstacles" in g:
        opt.update(obstacles=g["obstacles"], obstacle_cost=float(g["obstacle_cost"]))
    c = MPPIControllerForPathTracking(ref_path=paths[str(g["path"])], verbose=False, **opt, **kw)
    c.prev_waypoints_idx = int(g["prev_idx"])
    c.u_prev = g["u_prev"].copy()
    return c


# ---------------------------------------------------------------- asymmetric parameters (tests/golden/make_golden_asym.py)

ARM_FIELDS = ("m1", "m2", "l1", "l2", "lc1", "lc2", "g", "fk_l1", "fk_l2")
# the arm cases the GPU tests run besides the fixtures themselves: (fixture whose parameter set, pose and window it
# takes, K, T) at the smallest shapes that reach every code path (test_gpu_obstacles.py's)
ASYM_SHAPES = ((1000, 9), (300, 20))
ASYM_CASES = [(name, K, T) for name in ("a_k128_t20", "b_dense_k256_t24", "c_elbowup_k128_t20")
              for K, T in ASYM_SHAPES]
# Set b's alpha = 0.9 at lambda = 3e6 makes gamma = 3e5: the control-cost term, which the device computes in fp64 from
# the noise it is given, is then 99.9 % of S and hides the dynamics and the state cost from any relative tolerance.
# The fixture keeps alpha = 0.9 (through the drop-in); the rollout cases take alpha = 1.
ASYM_OVER = {"b_dense_k256_t24": dict(param_alpha=0.99999)}


def arm_of(g, cls):
    """The ArmParams (oracle's or package's class) stored in an asym_* fixture."""
    return cls(**{f: float(g[f]) for f in ARM_FIELDS})


def asym_cfg(g):
    """The controller constants of an asym_* fixture (either kind)."""
    return dict(delta_t=float(g["delta_t"]), param_lambda=float(g["param_lambda"]), param_alpha=float(g["param_alpha"]),
                param_exploration=float(g["param_exploration"]), sigma=g["sigma"],
                stage_cost_weight=g["stage_cost_weight"], terminal_cost_weight=g["terminal_cost_weight"])


def asym_problem(name, T):
    """Fixture `name`'s constants, start state and window with a nominal of horizon T: the fixture's gravity-holding
    row plus seeded noise.  Returns (g, cfg, x0, prev, u)."""
    g = load_asym_step(name)
    g.update({k: np.float64(v) for k, v in ASYM_OVER.get(name, {}).items()})
    u = np.tile(g["u_prev"][0], (T, 1)) + np.random.default_rng(T).normal(0, 0.5, (T, 2))
    return g, asym_cfg(g), g["x0"], int(g["prev_idx_after"]), u


def asym_engine(g, K, T, lps=0, K_total=None, k_offset=0, u_min=None, u_max=None, **over):
    """The arm's engine at an asym_* fixture's constants, `over` replacing any of asym_cfg's."""
    from mppi_robotarm_amd.engine import RolloutEngine
    from mppi_robotarm_amd.params import ArmParams
    kw = asym_cfg(g)
    kw.update(over)
    return RolloutEngine(K, T, kw["delta_t"], kw["param_lambda"], kw["param_alpha"], kw["sigma"],
                         kw["stage_cost_weight"], kw["terminal_cost_weight"], kw["param_exploration"],
                         arm_of(g, ArmParams), K_total=K_total, k_offset=k_offset, device=0, lanes_per_sample=lps,
                         u_min=u_min, u_max=u_max)


# (n, K, T, lambda) of the non-uniform chains on the GPU (test_gpu_chain_asym.py): test_gpu_chain.LINK_CASES' shapes.
# lambda = 100 at n = 7 too: at LINK_CASES' 1e8 the control-cost term is all of S and no link constant shows.
ASYM_LINK_CASES = [(3, 256, 16, 100.0), (4, 3000, 24, 100.0), (5, 777, 32, 1.0e4), (6, 2048, 20, 100.0),
                   (7, 1000, 9, 100.0), (2, 513, 40, 100.0)]


def asym_chain_kwargs(n):
    """A non-uniform n-link chain, seeded per n: every entry of m, l, lc, I, fk, J, b differs from every other entry
    of its vector (a permuted ramp), total reach 2 m, armature and damping spread over a decade."""
    rng = np.random.default_rng(7000 + n)
    ramp = lambda lo, hi: rng.permutation(np.linspace(lo, hi, n))   # noqa: E731
    l = ramp(0.7, 1.3)
    l = l * 2.0 / l.sum()
    return dict(m=tuple(ramp(0.6, 1.4)), l=tuple(l), lc=tuple(l * ramp(0.35, 0.6)), I=tuple(ramp(0.01, 0.12)),
                fk=tuple(l * ramp(0.75, 1.2)), J=tuple(ramp(0.02, 0.4)), b=tuple(ramp(0.2, 3.0)))


def asym_chain_inputs(n, T, mod):
    """asym_chain_kwargs(n) as `mod`.ChainParams (the oracle's module or the package's), a start state with joint
    rates around 1 rad/s, a random SPD Sigma and a gravity-holding nominal plus noise."""
    import chain_oracle as CO
    rng = np.random.default_rng(n * 100 + T + 7)
    kw = asym_chain_kwargs(n)
    q = np.array([1.4] + [-2.2 / (n - 1)] * (n - 1))
    x0 = np.concatenate([q, rng.uniform(0.6, 1.4, n) * rng.choice([-1.0, 1.0], n)])
    A = rng.normal(0, 1, (n, n))
    sig = A @ A.T / n + np.diag(np.linspace(8.0, 1.0, n))
    u = np.tile(CO.gravity_torque(q, CO.ChainParams(**kw)), (T, 1)) + rng.normal(0, 0.3, (T, n))
    return mod.ChainParams(**kw), x0, sig, u


def asym_rollout(g, cfg, x0, prev, u, eps, paths, **kw):
    """The fp64 yardstick's rollout (details=True) at an asym_* fixture's constants; eps (K, T, 2)."""
    import mppi_oracle as O
    return O.rollout_costs(x0, u, eps, paths["xydq_circle"], prev, cfg["delta_t"], cfg["param_lambda"],
                           cfg["param_alpha"], cfg["sigma"], cfg["stage_cost_weight"], cfg["terminal_cost_weight"],
                           cfg["param_exploration"], arm_of(g, O.ArmParams), details=True, **kw)


def asym_obstacle_problem(g, cfg, x0, prev, u, eps, paths):
    """Discs that tell the cost's two link lengths apart (fk_l1 = 1.1, fk_l2 = 0.9), placed from the yardstick's own
    unobstructed rollout on eps (over a short horizon the arm moves millimetres: a disc anywhere else is never
    touched).  With s the spread of link 1's final angle:
      0. beside link 1's last 5 cm, 2.5 cm short of the elbow on the side away from link 2, radius 4 s: the 30 % of
         the samples whose link 1 turned furthest that way touch it; a link 1 of 0.9 ends 17 cm short of it;
      1. 3 cm past link 2's tip along the link, radius 1.5 cm: never touched, but a link 2 of 1.1 runs through it;
      2. at the elbow, its centre 0.8 r beside link 1's end on that same side (behind link 2's start), radius
         r = 0.4 s: the clipped ends of both links touch it in a band of samples above the 8 % quantile of the other
         tail (the start pose, from which the samples spread, stays outside the band);
      3. behind the base, 4 mm short of link 1's clipped start: never touched.
    Returns dict(free=the rollout, discs=(4, 3))."""
    free = asym_rollout(g, cfg, x0, prev, u, eps, paths)
    a, b = float(g["fk_l1"]), float(g["fk_l2"])
    q1, q12 = free["q"][:, -1, 0], free["q"][:, -1].sum(-1)
    side = 1.0 if float(np.median(free["q"][:, -1, 1])) < 0 else -1.0
    s = float(np.std(q1))
    unit = lambda t: np.array([np.cos(t), np.sin(t)])           # noqa: E731
    normal = lambda t: np.array([-np.sin(t), np.cos(t)])        # noqa: E731
    th = float(np.quantile(q1, 0.7 if side > 0 else 0.3))
    d = a - 0.025
    r0 = max(4.0 * d * s, 1e-4)
    c0 = d * unit(th) + side * r0 * normal(th)
    c1 = a * unit(float(np.median(q1))) + (b + 0.03) * unit(float(np.median(q12)))
    te = float(np.quantile(q1, 0.08 if side > 0 else 0.92))
    r2 = max(0.4 * a * s, 1e-4)
    c2 = a * unit(te) + side * 0.8 * r2 * normal(te)
    discs = np.array([[c0[0], c0[1], r0], [c1[0], c1[1], 0.015], [c2[0], c2[1], r2], [-0.05, -0.02, 0.05]])
    return dict(free=free, discs=discs)


# ---------------------------------------------------------------- the chain's fused update (chain_update_block)
# test_gpu_chain_update.py runs it on the device, test_chain_update_cpu.py proves on the CPU what its cases rely on.

UPDATE_NS = (2, 3, 4, 5, 6, 7)
# 5: the device minimum; below 10 every window reflects at both ends; 6, 7, 11, 13, 125, 127: T % 4 in {1, 2, 3}, a
# tail thread whose last windows lie past T; 127, 128: the full thread map and the tid % MPPI_MAX_T row split
UPDATE_TS = (5, 6, 7, 9, 11, 13, 125, 127, 128)
# (precision, lanes per sample, K): test_gpu_chain_obstacles.FORMS, two workgroups with a ragged second one in each
UPDATE_FORMS = [("f32", 1, 300), ("f32", 4, 100), ("f64", 1, 300)]
UPDATE_FORM_IDS = ["f32-lps1", "f32-lps4", "f64"]
UPDATE_WIN = slice(40, 70)
UPDATE_DT, UPDATE_ALPHA = 0.006, 0.98
UPDATE_W, UPDATE_TW = [0.5, 0.5, 5.0, 5.0], [5.0, 5.0, 50.0, 50.0]
# lambda per n: the smallest power of ten at which the control-cost share of every single joint,
# sum_t a_t[d] v[k, t, d], is a median >= 3e-4 of S over the samples at T = 6 and T = 128 of asym_chain_inputs (the
# last joint carries the least torque and sets it: 2.6e-4 .. 1.1e-3 at these values, a decade less one power below),
# so that a wrong a_t row of any joint moves S by 100 x the fp32 bound of 1e-6 with room to spare
# (test_chain_update_cpu.py asserts the 1e-4).  gamma = lambda (1 - alpha) scales a_t.
UPDATE_LAMBDA = {2: 1.0e3, 3: 1.0e5, 4: 1.0e4, 5: 1.0e4, 6: 1.0e5, 7: 1.0e4}
UPDATE_S_RTOL = {"f32": 1e-6, "f64": 1e-12}   # test_chain_fused_update_matches_host_update's bounds on S


def update_seed(n):
    """The Philox seed of the update tests' draws at n links."""
    return 40 + n


def shift_nominal(un):
    """control.py:148-149: the rows moved up by one, the last one kept."""
    return np.concatenate([un[1:], un[-1:]], 0)


def median10(w):
    """control.py:319-327: scipy's median of 10 with reflected ends, per column."""
    from scipy.ndimage import median_filter
    return np.stack([median_filter(w[:, d], size=10, mode="reflect") for d in range(w.shape[1])], 1)


def reflected_windows(T):
    """(T, 10) indices of the windows t - 5 .. t + 4 reflected into [0, T) ('reflect': -1 -> 0, T -> T - 1), T >= 5."""
    m = np.arange(T)[:, None] + np.arange(-5, 5)[None]
    m = np.mod(m, 2 * T)
    return np.where(m >= T, 2 * T - 1 - m, m)


def sorted_median10(w):
    """The same filter without SciPy: rank 5 of np.sort over the reflected index list."""
    return np.sort(w[reflected_windows(w.shape[0])], axis=1)[:, 5]


def expected_nominal(u, w, lo=None, hi=None):
    """The fused update's nominal from the launch's own weighted noise w: shift(clip(u + median10(w)))."""
    un = u + median10(w)
    return shift_nominal(un if lo is None else np.clip(un, lo, hi))


def update_reference(n, T, paths, K=300, lo=None, hi=None, lam=None):
    """The fp64 oracle's update before its shift and clip, u + median10(w_eps), of asym_chain_inputs(n, T) at
    `lam` (None: UPDATE_LAMBDA[n]) on the host restatement of the device's Philox draw (philox_ref.chain_noise: the
    device's values to ~1e-6), with the sampled controls clipped to lo / hi when given.  Returns (un (T, n), S (K,),
    u, eps)."""
    import chain_oracle as CO
    import philox_ref
    Po, x0, sig, u = asym_chain_inputs(n, T, CO)
    lam = UPDATE_LAMBDA[n] if lam is None else lam
    eps = philox_ref.chain_noise(K, T, n, 0, update_seed(n), 0, sig).transpose(2, 0, 1)
    eps = eps.astype(np.float32).astype(np.float64)
    S = CO.chain_rollout_costs(x0, u, eps, paths["xydq_circle"], UPDATE_WIN.start, UPDATE_DT, lam, UPDATE_ALPHA, sig,
                               UPDATE_W, UPDATE_TW, 0.0, Po, lo=lo, hi=hi)
    wk = np.exp(-(S - S.min()) / lam)
    w = np.einsum("k,ktd->td", wk / wk.sum(), eps)
    return u + median10(w), S, u, eps


_UPDATE_LIMITS = {}


UPDATE_CLAMP_LAMBDA = 1.0e3   # the torque-limit cases' lambda, the same at every n


def update_limits(n, T, paths):
    """Torque limits inside the spread of the updated nominal, distinct per joint and per side: quantiles of the
    columns of update_reference's unlimited u + filt at UPDATE_CLAMP_LAMBDA, from (0.05, 0.95) at joint 0 to
    (0.15, 0.85) at the last.  The limits change the weights (mode 2 clips the sampled controls too), and at T = 9
    every window holds nearly the same values, so a column of the filtered noise moves as a whole: the share that
    the limits clip in the run that has them lies between 0.18 and 0.84 over the cases of test_chain_update_cpu.py,
    which asserts (0.1, 0.9).  Computed once per (n, T) and left unchanged."""
    if (n, T) not in _UPDATE_LIMITS:
        un = update_reference(n, T, paths, lam=UPDATE_CLAMP_LAMBDA)[0]
        lo = np.array([np.quantile(un[:, d], q) for d, q in enumerate(np.linspace(0.05, 0.15, n))])
        hi = np.array([np.quantile(un[:, d], q) for d, q in enumerate(np.linspace(0.95, 0.85, n))])
        lo.setflags(write=False)
        hi.setflags(write=False)
        _UPDATE_LIMITS[(n, T)] = (lo, hi)
    return _UPDATE_LIMITS[(n, T)]


def sparse_steps(T):
    """Every fourth step from 0, at most four: the steps of the structured noise whose every window's median is 0
    (test_chain_update_cpu.py counts them per reflected window)."""
    return np.arange(0, T, 4)[:4]


def dense_steps(T):
    """Six consecutive steps in the middle of the horizon: windows with six non-zero values, a non-zero median."""
    return np.arange((T - 6) // 2, (T - 6) // 2 + 6)


def step_noise(K, T, n, steps, sig, seed):
    """Host noise (K, T, n) fp32, N(0, diag Sigma) at `steps` and +0 everywhere else."""
    eps = np.zeros((K, T, n), dtype=np.float32)
    rng = np.random.default_rng(seed)
    eps[:, steps] = (rng.normal(size=(K, len(steps), n)) * np.sqrt(np.diag(sig))).astype(np.float32)
    return eps


def clipped_share(un, lo, hi):
    """The share of the entries of un that lo / hi clip."""
    return float(np.mean(np.clip(un, lo, hi) != un))
