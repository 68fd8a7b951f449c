"""GPU: moving obstacles in a sharded run.  Two ranks on one GPU (torch.distributed, gloo) run the arm's and the
chain's drop-in controller on the dense-weight moving fixture (move_step_b: every sample carries weight, so the merge
of the two shards' rows matters) with the discs and their velocities set on every rank, and must leave what the
single-process controller leaves, to 1e-10; and not what the same discs at rest leave.  The structure is
test_gpu_multigpu_dropin.py's: each scenario runs identically in a rank (pg = the process group) and in the parent
(pg = None).
"""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from conftest import GOLDEN, ctor_kwargs, load_paths  # noqa: E402
from helpers import _gpu  # noqa: E402, F401
from test_gpu_multigpu_dropin import _free_port  # noqa: E402

X_TOL = 1e-10


def _g():
    return dict(np.load(os.path.join(GOLDEN, "move_step_b_dense_k256_t24.npz")))


def _arm(pg, moving=True):
    from mppi_robotarm_amd.controller import MPPIControllerForPathTracking
    g, paths = _g(), load_paths()
    c = MPPIControllerForPathTracking(ref_path=paths[str(g["path"])], verbose=False, process_group=pg,
                                      obstacles=g["obstacles"], obstacle_cost=float(g["obstacle_cost"]),
                                      obstacle_velocities=g["obstacle_velocities"] if moving else None,
                                      **ctor_kwargs(g))
    c.prev_waypoints_idx = int(g["prev_idx"])
    c.u_prev = g["u_prev"].copy()
    eps = g["eps"].astype(np.float64)
    c._calc_epsilon = lambda *a, **k: eps
    u0, u_seq, opt, _ = c.calc_control_input(g["x0"])
    v = c._engine.obstacle_velocities
    out = dict(u_seq=u_seq.copy(), u0=np.array(u0), opt=opt, prev=c.prev_waypoints_idx,
               rankonly_vel=np.zeros((0, 2)) if v is None else v)
    c.close()
    return out


def _chain(pg, moving=True):
    from mppi_robotarm_amd.chain import ChainMPPIController, ChainParams
    g, paths = _g(), load_paths()
    c = ChainMPPIController(float(g["delta_t"]), paths[str(g["path"])], int(g["T"]), int(g["K"]),
                            float(g["param_exploration"]), float(g["param_lambda"]), float(g["param_alpha"]),
                            g["sigma"], g["stage_cost_weight"], g["terminal_cost_weight"], chain=ChainParams.from_arm2(),
                            u_init=g["u_prev"], process_group=pg, obstacles=g["obstacles"],
                            obstacle_cost=float(g["obstacle_cost"]),
                            obstacle_velocities=g["obstacle_velocities"] if moving else None)
    c.prev_waypoints_idx = int(g["prev_idx"])
    eps = g["eps"].astype(np.float64)
    c._calc_epsilon = lambda *a, **k: eps
    u0, u_seq, opt, _ = c.calc_control_input(g["x0"])
    v = c._engine.obstacle_velocities
    out = dict(u_seq=u_seq.copy(), u0=np.array(u0), opt=opt, prev=c.prev_waypoints_idx,
               rankonly_vel=np.zeros((0, 2)) if v is None else v)
    c.close()
    return out


SCENARIOS = {"arm": _arm, "chain": _chain}


def _rank(rank, world, port, out):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        res = {}
        for name, fn in SCENARIOS.items():
            for k, v in fn(dist.group.WORLD).items():
                res[f"{name}.{k}"] = np.asarray(v)
        np.savez(f"{out}.{rank}.npz", **res)
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    import torch.multiprocessing as mp
    out = str(tmp_path_factory.mktemp("mgpu_moving") / "r")
    mp.start_processes(_rank, args=(2, _free_port(), out), nprocs=2, join=True, start_method="spawn")
    return [dict(np.load(f"{out}.{r}.npz")) for r in range(2)]


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_two_ranks_match_the_single_process_controller(ranks, name):
    g = _g()
    single, rest = SCENARIOS[name](None), SCENARIOS[name](None, moving=False)
    for r in ranks:
        assert np.array_equal(r[f"{name}.rankonly_vel"], g["obstacle_velocities"])     # set on every rank
        for k in ("u_seq", "u0", "opt"):
            np.testing.assert_allclose(r[f"{name}.{k}"], single[k], rtol=X_TOL, atol=X_TOL, err_msg=f"{name}.{k}")
        assert int(r[f"{name}.prev"]) == single["prev"]
    np.testing.assert_array_equal(ranks[0][f"{name}.u_seq"], ranks[1][f"{name}.u_seq"])
    assert float(np.max(np.abs(single["u_seq"] - rest["u_seq"]))) > 1e-6               # the velocities matter here
