"""CPU: moving obstacles for the n-link chain.

  * oracle/chain_oracle.py's moving discs (O.collision_costs on chain_model with vel=) at n = 2 with
    ChainParams.from_arm2() against every move_step_* fixture captured from the reference (S to 1e-12 relative, every
    flag equal) and against the arm's;
  * zero velocities are the static definition (vel=None), bit for bit, at n = 2, 3 and 7;
  * chain_moving_masks (what the GPU tests evaluate on the device's recorded directions) agrees with the rollout's flags;
  * ChainMPPIController's validation of obstacle_velocities and its by-value comparison key;
  * the C ABI: mppi_chain_set_moving_obstacles is declared and exported, and refuses a null context.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import chain_oracle as CO
import mppi_oracle as O
from conftest import GOLDEN, ROOT
from mppi_robotarm_amd.chain import ChainMPPIController, ChainParams

HEADER = os.path.join(ROOT, "include", "mppi_rocm.h")
MOVE_STEPS = ["a_k128_t20", "b_dense_k256_t24", "c_expl_k128_t20", "d_clamp_k128_t20"]


def _load(name):
    return dict(np.load(os.path.join(GOLDEN, f"move_step_{name}.npz")))


def _args(g, path):
    return (g["x0"], g["u_prev"], g["eps"].astype(np.float64), path, int(g["prev_idx_after"]), float(g["delta_t"]),
            float(g["param_lambda"]), float(g["param_alpha"]), g["sigma"], g["stage_cost_weight"],
            g["terminal_cost_weight"], float(g["param_exploration"]))


@pytest.mark.parametrize("name", MOVE_STEPS)
def test_chain_yardstick_at_two_links_matches_the_reference(name, paths):
    g = _load(name)
    kw = dict(lo=g.get("u_min"), hi=g.get("u_max"), discs=g["obstacles"], vel=g["obstacle_velocities"],
              obstacle_cost=float(g["obstacle_cost"]))
    r = CO.step(*_args(g, paths[str(g["path"])]), CO.ChainParams.from_arm2(), **kw)
    assert np.array_equal(r["flag"], g["flag"])
    np.testing.assert_allclose(r["clear"], g["clearance"], rtol=1e-9, atol=1e-13)
    assert float(np.max(np.abs(r["S"] - g["S"]) / np.abs(g["S"]))) < 1e-12
    assert int(np.argmin(r["S"])) == int(np.argmin(g["S"]))
    np.testing.assert_allclose(r["u_seq"], g["u_seq"], rtol=1e-10, atol=1e-10)
    arm = O.rollout_costs(*_args(g, paths[str(g["path"])]), details=True, **kw)
    assert np.array_equal(r["flag"], arm["flag"]) and np.array_equal(r["hits"], arm["hits"])
    assert float(np.max(np.abs(r["S"] - arm["S"]) / np.abs(arm["S"]))) < 1e-12


@pytest.mark.parametrize("n", [2, 3, 7])
def test_zero_velocity_is_the_static_chain_yardstick_bit_for_bit(n, paths):
    rng = np.random.default_rng(n)
    L = 2.0 / n
    P = CO.ChainParams(m=(1.0,) * n, l=(L,) * n, lc=(L / 2,) * n, I=(L * L / 12.0,) * n, fk=(L,) * n, J=(0.1,) * n,
                       b=(1.0,) * n)
    q = np.array([1.4] + [-2.2 / (n - 1)] * (n - 1))
    x0 = np.concatenate([q, rng.normal(0, 0.2, n)])
    T, K = 5, 40
    u = np.tile(CO.gravity_torque(q, P), (T, 1))
    eps = rng.normal(0, 2.0, (K, T, n))
    tip = np.array(CO.chain_fk(q, P))
    discs = np.array([[tip[0] + 0.02, tip[1], 0.03], [0.3, 0.3, 0.1]])
    args = (x0, u, eps, paths["xydq_circle"], 40, 0.03, 100.0, 0.98, np.eye(n) * 4.0, [0.5, 0.5, 5.0, 5.0],
            [5.0, 5.0, 50.0, 50.0], 0.0, P)
    want = CO.chain_rollout_costs(*args, discs=discs, obstacle_cost=7.0, details=True)
    assert want["flag"].any() and not want["flag"].all()
    for vel in (None, np.zeros((2, 2))):
        got = CO.chain_rollout_costs(*args, discs=discs, vel=vel, obstacle_cost=7.0, details=True)
        for k in ("S", "S_track", "flag", "clear", "hits"):
            assert np.array_equal(got[k], want[k]), k
    moved = CO.chain_rollout_costs(*args, discs=discs, vel=np.array([[0.5, 0.0], [0.0, 0.0]]), obstacle_cost=7.0,
                                   details=True)
    assert not np.array_equal(moved["flag"], want["flag"])
    # the masks from recorded directions are the rollout's flags, and a step off they are not
    th = np.cumsum(moved["q"], -1)
    dirs = np.concatenate([np.cos(th), np.sin(th)], -1)
    vel = np.array([[0.5, 0.0], [0.0, 0.0]])
    mask, gap = CO.chain_moving_masks(dirs, discs, vel, 0.03, P.fk)
    assert np.array_equal(mask != 0, moved["flag"])
    np.testing.assert_allclose(gap.reshape(K, T, -1).min(-1), moved["clear"], rtol=1e-9, atol=1e-13)
    assert not np.array_equal(CO.chain_moving_masks(dirs, discs, vel, 0.03, P.fk, shift=-1)[0], mask)


# ---------------------------------------------------------------- the drop-in's key logic

DISCS = [[1.0, 0.5, 0.1], [0.2, 0.3, 0.0]]


def _ctrl(paths, **kw):
    return ChainMPPIController(0.006, paths["xydq_circle"], 8, 16, chain=ChainParams.from_arm2(), **kw)


@pytest.mark.parametrize("bad", [
    dict(obstacles=DISCS, obstacle_velocities=[[0.1, 0.0]]),
    dict(obstacles=DISCS, obstacle_velocities=[[0.1, 0.0, 0.0], [0.0, 0.0, 0.0]]),
    dict(obstacles=DISCS, obstacle_velocities=[[0.1, float("nan")], [0.0, 0.0]]),
    dict(obstacles=DISCS, obstacle_velocities=[[float("inf"), 0.0], [0.0, 0.0]]),
    dict(obstacles=None, obstacle_velocities=[[0.1, 0.0]])])
def test_validation(paths, bad):
    with pytest.raises(ValueError):
        _ctrl(paths, **bad)
    c = _ctrl(paths)
    for k, v in bad.items():
        setattr(c, k, v)
    state, u_before = np.random.get_state(), c.u_prev.copy()
    with pytest.raises(ValueError):
        c.calc_control_input(np.zeros(4))       # before any RNG draw, and before a GPU is needed
    assert all(np.array_equal(a, b) for a, b in zip(state, np.random.get_state()))
    assert np.array_equal(c.u_prev, u_before) and c.prev_waypoints_idx == 0


def test_velocities_are_a_plain_attribute_compared_by_value(paths):
    c = _ctrl(paths, obstacles=DISCS, obstacle_cost=5.0)
    assert c.obstacle_velocities is None
    static = c._obstacle_key()
    assert len(static) == 3                      # None is the static path
    v = np.array([[0.1, -0.2], [0.0, 0.0]])
    c.obstacle_velocities = v
    k = c._obstacle_key()
    assert k != static and k[:3] == static
    v[1, 0] = 0.3                                # an in-place edit
    assert c._obstacle_key() != k
    k = c._obstacle_key()
    c.obstacle_velocities = v.tolist()           # a rebind to an equal value
    assert c._obstacle_key() == k
    c.obstacle_velocities = None
    assert c._obstacle_key() == static


def test_the_entry_point_is_declared_and_exported_under_both_prefixes():
    from mppi_robotarm_amd import _native
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    name = "mppi_chain_set_moving_obstacles"
    assert re.search(rf"\bint {name}\s*\(\s*mppi_chain_ctx \*ctx, int n, const double \*discs,\s*const double \*vel, double cost\)", text)
    assert name in _native.EXPORTS and "mppi_set_moving_obstacles" in _native.EXPORTS
    if not os.path.exists(_native.LIB_PATH):
        from mppi_robotarm_amd.build import build_native
        build_native()
    lib = _native.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    assert getattr(lib, name).argtypes is not None and re.search(rf"\bT {name}\b", nm)
    assert lib.mppi_chain_set_moving_obstacles(None, 0, None, None, 0.0) == _native.MPPI_E_ARG
