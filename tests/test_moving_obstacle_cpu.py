"""CPU: moving obstacles (disc velocities predicted along the rollout horizon) on the 2-link arm.

  * oracle/mppi_oracle.py's moving discs, the NumPy yardstick the GPU tests use (O.collision_costs with vel=: the
    oracle's horizon loop with its penalty hook, the discs at c + v (t + 1) dt, O.discs_at), are pinned to every
    move_step_* / move_loop_* fixture captured from the reference itself (make_golden_moving.py: the reference with
    only _c and _phi overridden, the evaluation time from a call counter): S to 1e-12 relative and every collision
    flag equal;
  * zero velocities are the static definition bit for bit, and the chain yardstick at n = 2 is the arm's;
  * the fixtures mean something: the generator's conditions, and the two that make the motion matter;
  * the drop-in's validation of obstacle_velocities and its by-value comparison key;
  * the C ABI: the entry point is declared and exported, and its argument errors need no device.
"""
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import chain_oracle as CO
import mppi_oracle as O
from conftest import GOLDEN, ROOT
from helpers import load_obst_step
from mppi_robotarm_amd.controller import MPPIControllerForPathTracking
from mppi_robotarm_amd.engine import RolloutEngine

HEADER = os.path.join(ROOT, "include", "mppi_rocm.h")
MOVE_STEPS = sorted(os.path.basename(f)[len("move_step_"):-4] for f in glob.glob(os.path.join(GOLDEN, "move_step_*.npz")))


def load_move_step(name):
    return dict(np.load(os.path.join(GOLDEN, f"move_step_{name}.npz")))


def load_move_loop(name):
    return dict(np.load(os.path.join(GOLDEN, f"move_loop_{name}.npz")))


def ref_step(g, path, vel="own", shift=0):
    kw = dict(lo=g.get("u_min"), hi=g.get("u_max"), discs=g["obstacles"],
              vel=g["obstacle_velocities"] if isinstance(vel, str) else vel, obstacle_cost=float(g["obstacle_cost"]))
    args = (g["x0"], g["u_prev"], g["eps"].astype(np.float64), path, int(g["prev_idx_after"]), float(g["delta_t"]),
            float(g["param_lambda"]), float(g["param_alpha"]), g["sigma"], g["stage_cost_weight"],
            g["terminal_cost_weight"], float(g["param_exploration"]))
    if shift:
        return O.rollout_costs(*args, shift=shift, details=True, **kw)
    return O.step(*args, visualize_optimal_traj=bool(g["visualize_optimal_traj"]), **kw)


def test_the_fixtures_are_all_here():
    assert MOVE_STEPS == ["a_k128_t20", "b_dense_k256_t24", "c_expl_k128_t20", "d_clamp_k128_t20"]
    assert os.path.exists(os.path.join(GOLDEN, "move_loop_k64_t20.npz"))
    # tests/conftest.py globs step_* and loop_* into the unobstructed parity tests, helpers.py obst_step_*: none of ours
    assert not [f for f in os.listdir(GOLDEN) if "move" in f and f.startswith(("step_", "loop_", "obst_"))]


@pytest.mark.parametrize("name", MOVE_STEPS)
def test_moving_ref_matches_the_reference(name, paths):
    g = load_move_step(name)
    r = ref_step(g, paths[str(g["path"])])
    assert np.array_equal(r["flag"], g["flag"])
    np.testing.assert_allclose(r["clear"], g["clearance"], rtol=1e-9, atol=1e-13)
    assert int(np.argmin(r["S"])) == int(np.argmin(g["S"]))
    assert float(np.max(np.abs(r["S"] - g["S"]) / np.abs(g["S"]))) < 1e-12
    assert float(np.max(np.abs(r["S_track"] + float(g["obstacle_cost"]) * r["hits"] - g["S"]) / np.abs(g["S"]))) < 1e-12
    if np.count_nonzero(g["w"]) == 1:
        assert np.array_equal(r["w_eps_filt"], g["w_eps_filt"])
        assert np.array_equal(r["u_seq"], g["u_seq"]) and np.array_equal(r["u0"], g["u0"])
    else:
        np.testing.assert_allclose(r["u_seq"], g["u_seq"], rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(r["optimal_traj"], g["optimal_traj"], rtol=1e-10, atol=1e-10)


@pytest.mark.parametrize("name", MOVE_STEPS)
def test_the_fixtures_exercise_the_motion(name, paths):
    g = load_move_step(name)
    path = paths[str(g["path"])]
    r = ref_step(g, path)
    hit = r["dist"] < g["obstacles"][:, 2][None, None, :, None]
    assert 0.10 <= float(np.mean(g["flag"].any(1))) <= 0.90
    assert hit[..., 0].any() and hit[..., 1].any()                       # both links
    assert (hit & r["clipped"]).any() and (hit & ~r["clipped"]).any()    # a clipped and an unclipped foot
    assert float(np.mean(g["clearance"].min(1) >= 1e-4)) >= 0.80
    if bool(g["one_hot"]):
        order = np.argsort(g["S"])
        assert g["clearance"][order[:2]].min() >= 1e-4
        assert (g["S"][order[1]] - g["S"][order[0]]) / abs(g["S"][order[0]]) >= 1e-3
    # the motion matters: against the same discs at rest, and against the off-by-one definition c + v t dt
    rest = ref_step(g, path, vel=np.zeros_like(g["obstacle_velocities"]))
    off = ref_step(g, path, shift=-1)
    assert np.array_equal(rest["hits"], g["hits_rest"]) and np.array_equal(off["hits"], g["hits_off"])
    assert float(np.mean(r["hits"] != rest["hits"])) >= 0.50
    assert float(np.mean(r["hits"] != off["hits"])) >= 0.10


def test_moving_ref_matches_the_reference_closed_loop(paths):
    g = load_move_loop("k64_t20")
    from mppi_robotarm_amd.params import runpy_config
    kw = runpy_config()
    T = int(g["T"])
    u_prev = np.array([[10.0, -2.0]] * T)
    assert g["obstacles"].shape == (int(g["ticks"]),) + g["obstacle_velocities"].shape[:1] + (3,)
    # the generator advanced the discs by v times one plant step (half the controller's delta_t) between ticks
    np.testing.assert_allclose(g["obstacles"][1, :, :2] - g["obstacles"][0, :, :2], g["obstacle_velocities"] * 0.003,
                               rtol=0, atol=1e-15)
    assert not np.allclose(g["u"], g["u_free"])
    for i in range(int(g["ticks"])):
        r = O.step(g["states"][i], u_prev, g["eps"][i].astype(np.float64), paths["xydq_circle"],
                   int(g["prev_idx"][i]), 0.006, kw["param_lambda"], kw["param_alpha"], kw["sigma"],
                   kw["stage_cost_weight"], kw["terminal_cost_weight"], discs=g["obstacles"][i],
                   vel=g["obstacle_velocities"], obstacle_cost=float(g["obstacle_cost"]))
        assert np.array_equal(r["flag"], g["flag"][i]), i
        assert float(np.max(np.abs(r["S"] - g["S"][i]) / np.abs(g["S"][i]))) < 1e-12, i
        np.testing.assert_allclose(r["u_seq"], g["u_seq"][i], rtol=1e-10, atol=1e-10)
        u_prev = g["u_seq"][i].copy()


@pytest.mark.parametrize("vel", [None, "zeros"])
def test_zero_velocity_is_the_static_definition_bit_for_bit(vel, paths):
    g = load_obst_step("a_k128_t20")
    args = (g["x0"], g["u_prev"], g["eps"].astype(np.float64), paths[str(g["path"])], int(g["prev_idx_after"]),
            float(g["delta_t"]), float(g["param_lambda"]), float(g["param_alpha"]), g["sigma"], g["stage_cost_weight"],
            g["terminal_cost_weight"])
    want = O.rollout_costs(*args, discs=g["obstacles"], obstacle_cost=float(g["obstacle_cost"]), details=True)
    got = O.rollout_costs(*args, discs=g["obstacles"], vel=None if vel is None else np.zeros((4, 2)),
                          obstacle_cost=float(g["obstacle_cost"]), details=True)
    for k in ("S", "S_track", "flag", "clear", "hits", "dist", "q"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["S"], g["S"]) or float(np.max(np.abs(got["S"] - g["S"]) / np.abs(g["S"]))) < 1e-12


def test_the_chain_yardstick_at_two_links_is_the_arms(paths):
    g = load_move_step("a_k128_t20")
    args = (g["x0"], g["u_prev"], g["eps"].astype(np.float64), paths[str(g["path"])], int(g["prev_idx_after"]),
            float(g["delta_t"]), float(g["param_lambda"]), float(g["param_alpha"]), g["sigma"], g["stage_cost_weight"],
            g["terminal_cost_weight"])
    kw = dict(discs=g["obstacles"], vel=g["obstacle_velocities"], obstacle_cost=float(g["obstacle_cost"]))
    arm = O.rollout_costs(*args, details=True, **kw)
    chain = CO.chain_rollout_costs(*args, P=CO.ChainParams.from_arm2(), details=True, **kw)
    assert np.array_equal(chain["flag"], arm["flag"]) and np.array_equal(chain["hits"], arm["hits"])
    assert float(np.max(np.abs(chain["S"] - arm["S"]) / np.abs(arm["S"]))) < 1e-12
    # ... and at rest it is the chain's static yardstick, bit for bit
    rest = CO.chain_rollout_costs(*args, P=CO.ChainParams.from_arm2(), discs=g["obstacles"], vel=np.zeros((4, 2)),
                                  obstacle_cost=float(g["obstacle_cost"]), details=True)
    want = CO.chain_rollout_costs(*args, P=CO.ChainParams.from_arm2(), discs=g["obstacles"],
                                  obstacle_cost=float(g["obstacle_cost"]), details=True)
    assert np.array_equal(rest["S"], want["S"]) and np.array_equal(rest["flag"], want["flag"])


def test_moving_masks_agree_with_the_rollout_yardstick(paths):
    """moving_masks (what the GPU tests evaluate on the device's recorded directions) on the yardstick's own."""
    g = load_move_step("d_clamp_k128_t20")
    r = ref_step(g, paths[str(g["path"])])
    q = r["q"]
    dirs = np.stack([np.cos(q[..., 0]), np.sin(q[..., 0]), np.cos(q.sum(-1)), np.sin(q.sum(-1))], -1)
    mask, gap = O.moving_masks(dirs, g["obstacles"], g["obstacle_velocities"], float(g["delta_t"]))
    assert np.array_equal(mask != 0, g["flag"])
    np.testing.assert_allclose(gap.reshape(gap.shape[:2] + (-1,)).min(-1), g["clearance"], rtol=1e-9, atol=1e-13)
    off, _ = O.moving_masks(dirs, g["obstacles"], g["obstacle_velocities"], float(g["delta_t"]), shift=-1)
    assert not np.array_equal(off, mask)


# ---------------------------------------------------------------- the drop-in's key logic

def _ctrl(paths, **kw):
    return MPPIControllerForPathTracking(delta_t=0.006, ref_path=paths["xydq_circle"], horizon_step_T=8,
                                         number_of_samples_K=16, verbose=False, sigma=np.eye(2) * 20.0, **kw)


DISCS = [[1.0, 0.5, 0.1], [0.2, 0.3, 0.0]]


@pytest.mark.parametrize("bad", [
    dict(obstacles=DISCS, obstacle_velocities=[[0.1, 0.0]]),                       # one row for two discs
    dict(obstacles=DISCS, obstacle_velocities=[0.1, 0.0, 0.2, 0.0]),               # flat
    dict(obstacles=DISCS, obstacle_velocities=[[0.1, 0.0, 0.0], [0.0, 0.0, 0.0]]),
    dict(obstacles=DISCS, obstacle_velocities=[[0.1, float("nan")], [0.0, 0.0]]),
    dict(obstacles=DISCS, obstacle_velocities=[[float("inf"), 0.0], [0.0, 0.0]]),
    dict(obstacles=DISCS, obstacle_velocities=[[1e300, 0.0], [0.0, 0.0]]),         # not finite in fp32
    dict(obstacles=DISCS, obstacle_velocities="fast"),
    dict(obstacles=None, obstacle_velocities=[[0.1, 0.0]]),                        # velocities without discs
    dict(obstacles=[], obstacle_velocities=np.zeros((0, 2)))])
def test_validation(paths, bad):
    with pytest.raises(ValueError):
        _ctrl(paths, **bad)
    c = _ctrl(paths)
    for k, v in bad.items():
        setattr(c, k, v)
    state = np.random.get_state()
    with pytest.raises(ValueError):
        c.calc_control_input(np.zeros(4))       # before any RNG draw, and before a GPU is needed
    assert all(np.array_equal(a, b) for a, b in zip(state, np.random.get_state()))
    assert c.prev_waypoints_idx == 0
    if bad["obstacles"]:
        with pytest.raises(ValueError):
            RolloutEngine.check_velocities(bad["obstacle_velocities"], len(bad["obstacles"]))


def test_velocities_are_a_plain_attribute_compared_by_value(paths):
    c = _ctrl(paths, obstacles=DISCS, obstacle_cost=5.0)
    assert c.obstacle_velocities is None
    static = c._obstacle_key()
    assert len(static) == 3                      # None is the static path: the key the static feature had
    v = np.array([[0.1, -0.2], [0.0, 0.0]])
    c.obstacle_velocities = v
    k = c._obstacle_key()
    assert k != static and k[:3] == static and k == c._obstacle_key()
    v[1, 0] = 0.3                                # an in-place edit
    assert c._obstacle_key() != k
    k = c._obstacle_key()
    c.obstacle_velocities = v.tolist()           # a rebind to an equal value
    assert c._obstacle_key() == k
    c.obstacle_velocities = np.zeros((2, 2))     # at rest, given: its own key (the engine takes it as at rest)
    assert c._obstacle_key() not in (k, static)
    c.obstacle_velocities = None
    assert c._obstacle_key() == static
    c.obstacles = None
    assert c._obstacle_key() is None
    a = RolloutEngine.check_velocities([(1, 2)], 1)
    assert a.dtype == np.float64 and a.shape == (1, 2) and a.flags.c_contiguous
    assert RolloutEngine.check_velocities(None, 0) is None and RolloutEngine.check_velocities(None, 3) is None


def test_push_gives_the_engine_the_velocities_once(paths):
    """_push_obstacles against a stand-in engine: the call it makes, and that an engine holding the same discs and
    velocities is left alone."""
    calls = []

    class Eng:
        obstacles, obstacle_cost, obstacle_velocities = np.zeros((0, 3)), 0.0, None

        def set_obstacles(self, discs, cost, velocities=None):
            a, w = RolloutEngine.check_obstacles(discs, cost)
            self.obstacles, self.obstacle_cost = a, w
            self.obstacle_velocities = RolloutEngine.check_velocities(velocities, a.shape[0])
            calls.append(None if velocities is None else np.array(velocities, dtype=np.float64))

    c, eng = _ctrl(paths, obstacles=DISCS, obstacle_cost=5.0), Eng()
    c._push_obstacles(eng, c._obstacle_key())
    c._push_obstacles(eng, c._obstacle_key())
    assert len(calls) == 1 and calls[0] is None
    c.obstacle_velocities = [[0.1, 0.0], [0.0, -0.1]]
    c._push_obstacles(eng, c._obstacle_key())
    c._push_obstacles(eng, c._obstacle_key())
    assert len(calls) == 2 and np.array_equal(calls[1], [[0.1, 0.0], [0.0, -0.1]])
    c.obstacle_velocities[0][0] = 0.2
    c._push_obstacles(eng, c._obstacle_key())
    assert len(calls) == 3 and calls[2][0, 0] == 0.2
    c.obstacle_velocities = None
    c._push_obstacles(eng, c._obstacle_key())
    assert len(calls) == 4 and calls[3] is None and eng.obstacle_velocities is None
    c.obstacles = None
    c._push_obstacles(eng, c._obstacle_key())
    assert eng.obstacles.shape == (0, 3)


def test_the_new_parameter_is_keyword_only():
    import inspect
    params = inspect.signature(MPPIControllerForPathTracking.__init__).parameters
    assert params["obstacle_velocities"].kind is inspect.Parameter.KEYWORD_ONLY
    assert params["obstacle_velocities"].default is None
    assert inspect.signature(RolloutEngine.set_obstacles).parameters["velocities"].default is None


def test_the_entry_point_is_declared_and_exported():
    from mppi_robotarm_amd import _native
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    name = "mppi_set_moving_obstacles"
    assert re.search(rf"\bint {name}\s*\(\s*mppi_ctx \*ctx, int n, const double \*discs, const double \*vel,\s*double cost\)", text)
    assert name in _native.EXPORTS
    if not os.path.exists(_native.LIB_PATH):
        from mppi_robotarm_amd.build import build_native
        build_native()
    lib = _native.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    assert hasattr(lib, name) and getattr(lib, name).argtypes is not None
    assert re.search(rf"\bT {name}\b", nm)
    # no context: an argument error, not a crash
    assert lib.mppi_set_moving_obstacles(None, 0, None, None, 0.0) == _native.MPPI_E_ARG
