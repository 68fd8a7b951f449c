"""What the test files share besides conftest.py's fixtures: the clamp_* / obst_* fixture plumbing, run.py's
constants, and the GPU tests' helpers (torch and the package are imported inside the functions, so this module
imports without either).

The yardsticks themselves live in ``oracle/``: ``mppi_oracle.py`` (the arm, with torque limits and workspace
obstacles) and ``chain_oracle.py`` (the chain, with torque limits), pinned to these fixtures by
test_oracle_golden.py, test_clamp_cpu.py, test_chain_clamp_cpu.py, test_obstacle_cpu.py and test_chain_oracle.py.
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
