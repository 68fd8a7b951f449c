"""Drop-in ``MPPIControllerForPathTracking`` backed by the MI355X engine.

Same constructor arguments (control.py:21-35, including the ``visualze``
spelling), same ``calc_control_input(observed_x)`` contract (control.py:67-152):

  * host, fp64 NumPy (O(T) work, exactly as the reference):
      nearest-waypoint update + end-of-path ``IndexError`` (control.py:75-78),
      noise draw ``np.random.multivariate_normal`` on the legacy global RNG
      (control.py:154-164, same stream as the reference; its standard-normal
      stream threaded in C with the same values, ``hostrng``),
      ``np.linalg.inv(Sigma)`` (``LinAlgError`` as at control.py:106),
      and the aliasing return (``u0`` is a view of the shifted ``u_prev``;
      ``u_seq is self.u_prev``);
  * device, HIP (O(K*T) work): rollouts, costs, soft-min weights, weighted
    noise sum (control.py:81-118) and the trajectory re-rolls
    (control.py:129-145);
  * the update of control.py:120-149 (median filter, ``u += w_eps``, shift):
    for T >= 5 inside the rollout launch (fused update: the median of 10 is a
    selection and the add is the same fp64 add, so the values equal the host
    path's), then one read-back of the shifted nominal and the optimal
    trajectory; with T < 5, or ``host_update=True``, on the host through
    ``scipy.ndimage.median_filter`` (control.py:319-327) as the reference does.
    With device noise the next step's noise is generated at the end of a call,
    off the next call's critical path.

Extra keyword arguments (all optional): ``device``, ``verbose`` (the three
progress prints of control.py:227-229, on by default like the reference),
``noise`` ("numpy" = reference RNG stream, or "device" = on-device Philox),
``seed`` (device noise), ``lanes_per_sample``, ``arm`` (ArmParams; its
``fk_l1``/``fk_l2`` start ``self.l1``/``self.l2``, which the engine follows
from then on), ``u_min`` / ``u_max`` (torque limits, a scalar or one value per
joint: the reference's clamp hook ``_g``, control.py:166-172, switched on —
the sampled controls are clipped before the dynamics and the control cost, the
weights still multiply the unclamped noise, and with ``visualize_optimal_traj``
the updated nominal is clipped too, exactly as ``_g`` clipping in place would),
``obstacles`` / ``obstacle_cost`` (up to eight discs ``(cx, cy, r)`` that neither
link may touch: every colliding step of a sample, and its final state once more,
adds ``obstacle_cost`` to its cost, the reference with ``_c`` and ``_phi``
returning ``... + obstacle_cost * collides(x)``; plain attributes, re-read on
every call, so they may move between calls), ``obstacle_velocities`` (``(n, 2)``
rows of ``(vx, vy)`` in m/s, one per disc, constant over the horizon of a call,
or ``None`` for discs at rest: ``obstacles`` then holds the positions at the
observed state, and the state rollout step ``t`` produces is tested against the
discs at ``c + v (t + 1) delta_t``; the caller advances ``obstacles`` between
calls; a plain attribute compared by value like ``obstacles``),
``process_group`` (shard the samples over the ranks of a
torch.distributed group), ``exchange`` (with a process group: "auto" = the
in-launch exchange, one launch per rank per step, when its one-step self-check
against the all-gather passes, else one RCCL all-gather of the per-device
partials plus a merge launch per step; "launch" or "rccl" force one) and
``host_update`` (force the host update path).

Multi-GPU: every rank constructs the controller with the same arguments and
calls ``calc_control_input`` with the same ``observed_x`` in the same order
(run.py's loop, replicated); with NumPy noise every rank draws the reference's
full (K, T, 2) stream from the same seed and keeps its slice (checked once,
at the first step).

The noise draw (host and device), the draw queued for the next call, sharding
and the multi-GPU set-up are ``controller_base.MPPIControllerBase``'s, shared
with the 7-link chain's controller (``chain.py``); ``first_min_index``,
``SampledReadback``, ``DeviceDrawn``, ``_noise_check`` and ``_pinned_zbuf``
live there too and are re-exported here.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np
import torch
from scipy.ndimage import median_filter

import dataclasses

from . import _native, hostrng
from .controller_base import (DeviceDrawn, MPPIControllerBase, SampledReadback,  # noqa: F401 (re-exported)
                              _noise_check, _pinned_zbuf, first_min_index)
from .distributed import exchange_partials, same_on_all_ranks, shard_geometry
from .engine import RolloutEngine
from .params import ArmParams

SEARCH_IDX_LEN = 30  # control.py:203


class MPPIControllerForPathTracking(MPPIControllerBase):
    def __init__(
            self,
            delta_t: float = 0.01,
            ref_path: float = 0,
            horizon_step_T: int = 20,
            number_of_samples_K: int = 500,
            param_exploration: float = 0.0,
            param_lambda: float = 50.0,
            param_alpha: float = 1.0,
            sigma: np.ndarray = np.array([[10.0, 10.0], [100.0, 100.0]]),
            stage_cost_weight: np.ndarray = np.array([10.0, 10.0, 10.0, 10.0]),
            terminal_cost_weight: np.ndarray = np.array([10.0, 10.0, 10.0, 10.0]),
            visualize_optimal_traj=True,
            visualze_sampled_trajs=False,
            *,
            device: int | None = None,
            verbose: bool = True,
            noise: str = "numpy",
            seed: int = 0,
            lanes_per_sample: int = 0,
            arm: ArmParams | None = None,
            u_min=None,
            u_max=None,
            obstacles=None,
            obstacle_cost: float = 1.0e10,
            obstacle_velocities=None,
            process_group=None,
            exchange: str = "auto",
            host_update: bool = False,
            numpy_noise_on_device: bool = True,
    ) -> None:
        self.dim_x = 4
        self.dim_u = 2
        self.T = horizon_step_T
        self.K = number_of_samples_K
        self.param_exploration = param_exploration
        self.param_lambda = param_lambda
        self.param_alpha = param_alpha
        self.param_gamma = self.param_lambda * (1.0 - (self.param_alpha))
        self.Sigma = sigma
        self.stage_cost_weight = stage_cost_weight
        self.terminal_cost_weight = terminal_cost_weight
        self.visualize_optimal_traj = visualize_optimal_traj
        self.visualze_sampled_trajs = visualze_sampled_trajs
        self.delta_t = delta_t
        self.ref_path = ref_path
        self.l1 = 1
        self.l2 = 1
        self.u_prev = np.array([[10.0, -2.0] for i in range(self.T)])
        self.prev_waypoints_idx = 0

        super().__init__(device=device, verbose=verbose, noise=noise, seed=seed, process_group=process_group,
                         exchange=exchange, numpy_noise_on_device=numpy_noise_on_device)
        if arm is not None:                # the cost's kinematics lengths (control.py:55-56)
            self.l1, self.l2 = arm.fk_l1, arm.fk_l2
        self.arm = ArmParams(fk_l1=float(self.l1), fk_l2=float(self.l2)) if arm is None else arm
        self._lanes_per_sample = lanes_per_sample
        self.host_update = host_update  # property: forced, or T < 5 (the device median needs T >= 5)
        self.u_min, self.u_max = u_min, u_max   # properties: torque limits of _g, validated
        self._limits()                          # u_min <= u_max
        self.obstacles = obstacles              # (n, 3) array-like of discs (cx, cy, r), n <= 8, or None
        self.obstacle_cost = obstacle_cost      # added to S per colliding step (and once for the final state)
        self.obstacle_velocities = obstacle_velocities   # (n, 2) array-like of (vx, vy) in m/s, or None: at rest
        self._obst_checked = None               # the last (obstacles bytes, cost, velocities) that passed the checks
        self._okey = None                       # this call's key, for _tick (whose signature tests stub)
        self._obstacle_key()
        self._bound = None             # what the engine's drop-in tick is bound to (_bind_key)
        self._fast = None              # what the last bound tick checked (calc_control_input's fast test)

    @property
    def host_update(self) -> bool:
        """The update of control.py:120-149 on the host: asked for, or T < 5 (the
        device median filter needs T >= 5), following self.T if it changes."""
        return self._host_update or self.T < 5

    @host_update.setter
    def host_update(self, value) -> None:
        self._host_update = bool(value)

    # ------------------------------------------------------------ engine
    def _engine_key(self):
        """The shared key plus the kinematics lengths self.l1/l2 (control.py:178-179,205-206), the arm
        constants and the torque limits with their mode."""
        return super()._engine_key() + (float(self.l1), float(self.l2), self.arm, self._clamp_key())

    def _get_engine(self, key=None) -> RolloutEngine:
        key = self._engine_key() if key is None else key
        if self._engine is not None and key != self._engine_built_for:
            self.close()             # an attribute the engine baked in changed: rebuild, as the reference re-reads it
        if self._engine is None:
            world, rank = self._shard()
            K_local, k_offset = shard_geometry(self.K, world, rank)
            device = self._device if self._device is not None else torch.cuda.current_device()
            # gamma is fixed at construction in the reference (control.py:45) while lambda is
            # re-read per call: the engine takes gamma as given; the cost's kinematics follow self.l1/l2
            arm = dataclasses.replace(self.arm, fk_l1=float(self.l1), fk_l2=float(self.l2))
            lo, hi = self._limits() or (None, None)
            self._engine = RolloutEngine(
                K_local, self.T, self.delta_t, self.param_lambda, self.param_alpha, self.Sigma,
                self.stage_cost_weight, self.terminal_cost_weight, self.param_exploration, arm,
                K_total=self.K, k_offset=k_offset, device=device, lanes_per_sample=self._lanes_per_sample,
                param_gamma=self.param_gamma, u_min=lo, u_max=hi, clamp_nominal=bool(self.visualize_optimal_traj))
            self._engine_built_for = key
            self._noise_dev = self._engine.new_noise()
            self._noise_alt = None
            self._partial = self._engine.new_partial()
            self._S_dev = torch.empty(K_local, dtype=torch.float64, device=self._engine.device)
            self._traj_dev = torch.empty((self.T, self.dim_x), dtype=torch.float32, device=self._engine.device)
            if world > 1:
                self._gathered = torch.empty(world * self._engine.partial_len, dtype=torch.float64,
                                             device=self._engine.device)
            self._xmode = None
        return self._engine

    def _multi_rollout(self, eng: RolloutEngine, S_out, fused: bool) -> None:
        """control.py:81-118 over every rank's shard, the rows merged on every rank:
        one launch with the in-launch exchange, or rollout + RCCL all-gather + merge
        launch.  fused: the update of control.py:120-149 too, published for wait_outputs."""
        if self._xmode == "launch":
            eng.rollout(self._noise_dev, S_out=S_out, fused_update=fused, exchange=True, host_out=fused)
            return
        world, _ = self._shard()
        eng.rollout(self._noise_dev, S_out=S_out, partial_out=self._partial)
        exchange_partials(self._partial, self._gathered, self.process_group)
        eng.merge(self._gathered, world, fused_update=fused, host_out=fused)

    # ------------------------------------------------------------ API
    def calc_control_input(self, observed_x: np.ndarray) -> Tuple[float, np.ndarray]:
        """calculate optimal control input (control.py:67-152)"""
        if self.process_group is not None and (self._xmode == "launch" or (
                self._xmode is None and self.exchange != "rccl" and not self._x_failed)):
            # the in-launch exchange can fail on a late rank (ExchangeError on every rank of the step, no update
            # applied anywhere): every rank then restores what the call changed and runs it again over the
            # all-gather, which waits for the late rank, and stays on it.  The first call is covered too (it
            # picks the exchange and then runs its step in-launch).
            saved = (self.prev_waypoints_idx, self._step_count,
                     np.random.get_state() if self.noise_source == "numpy" else None)
            try:
                return self._calc_control_input(observed_x)
            except _native.ExchangeError:
                self.prev_waypoints_idx, self._step_count, rng = saved
                # the ranks re-run the same step: a rank whose verdict differed (it saw the step fail while the
                # others applied it) would pair its retry's all-gather with their next step
                if not same_on_all_ranks(("exchange retry", self._step_count), self.process_group):
                    raise RuntimeError("multi-GPU exchange: the ranks disagree on the failed step; "
                                       "their nominals can no longer be kept in step") from None
                if rng is not None:
                    np.random.set_state(rng)
                self._exchange_failed()
                verbose, self.verbose = self.verbose, False     # the call's three lines are printed already
                try:
                    return self._calc_control_input(observed_x)
                finally:
                    self.verbose = verbose
        return self._calc_control_input(observed_x)

    def _exchange_failed(self) -> None:
        """After an ExchangeError (every rank): the collective exchange from now on, no native tick, and the
        device noise drawn again for the step (the tick queues the next step's draw into the same buffer)."""
        self._xmode = "rccl"
        self._x_failed = True
        self._fast = None
        self._bound = None
        self._noise_ready = None

    def _calc_control_input(self, observed_x: np.ndarray) -> Tuple[float, np.ndarray]:
        okey = self._okey = self._obstacle_key()           # ValueError before anything is drawn or moved
        if self._npre is not None and self.noise_source != "numpy":
            self._settle_predraw()                         # (the NumPy path settles it after its checks)
        f = self._fast
        if (f is not None and f[10] == okey and f[0] is self.ref_path and f[1] is self.u_prev and f[2] is self.Sigma
                and f[3] is self.stage_cost_weight and f[4] is self.terminal_cost_weight and f[5] is self._engine
                and f[6] == self._fast_scalars() and f[7] == self.Sigma.tobytes()
                and f[8] == self.stage_cost_weight.tobytes() and f[9] == self.terminal_cost_weight.tobytes()):
            return self._tick_bound(observed_x)
        if (self.noise_source == "device" and not self.host_update and not self.visualze_sampled_trajs
                and (self.process_group is None or self._xmode == "launch") and self.K >= 1):
            out = self._tick(observed_x)
            if out is not None:
                return out
        u = self.u_prev
        x0 = observed_x
        self._get_nearest_waypoint(x0[0], x0[1], update_prev_idx=True)
        if self.prev_waypoints_idx >= self.ref_path.shape[0] - 1:
            print("[ERROR] Reached the end of the reference path.")
            raise IndexError
        if self.K < 1:
            raise ValueError("zero-size array to reduction operation minimum which has no identity")

        if self.noise_source == "numpy":
            epsilon = self._device_reference_noise()
            if epsilon is None:
                epsilon = self._reference_noise()
        else:
            epsilon = None
            self._check_sigma(self.Sigma, self.dim_u)
        key = self._engine_key()
        if key != self._engine_built_for:
            np.linalg.inv(self.Sigma)                      # LinAlgError exactly as control.py:106
        eng = self._get_engine(key)
        self._push_obstacles(eng, okey)
        if isinstance(epsilon, DeviceDrawn):
            pass                                           # already in self._noise_dev
        elif isinstance(epsilon, hostrng.StdNoise):
            self._zbuf_ev = eng.upload_std_noise(epsilon, self._zbuf, self._noise_dev)
        elif epsilon is not None:
            lo = eng.k_offset
            eng.upload_noise(epsilon[lo:lo + eng.K_local], out=self._noise_dev)
        elif self._noise_ready != (self.seed, self._step_count):
            eng.philox_noise(self.seed, self._step_count, out=self._noise_dev)
        self._step_count += 1

        window = self.ref_path[self.prev_waypoints_idx:(self.prev_waypoints_idx + SEARCH_IDX_LEN)]
        world, _ = self._shard()
        if not self.host_update and world == 1 and not self.visualze_sampled_trajs:
            # (after a device draw, _device_reference_noise has queued the next call's draw beside this step)
            return self._dropin_step(eng, x0, window, u)
        eng.set_step_inputs(np.asarray(x0, dtype=np.float64), window, u)
        if world > 1 and self._xmode is None:
            check = _noise_check(self, epsilon)
            self._multi_setup(eng, check)
        if not self.host_update:
            return self._fused_step(eng, x0, u, world, predraw=isinstance(epsilon, DeviceDrawn) and world == 1)
        S_out = self._S_dev if self.keep_costs else None
        if world == 1:
            eng.rollout(self._noise_dev, S_out=S_out)
        else:
            self._multi_rollout(eng, S_out, fused=False)
        w_epsilon = eng.weighted_noise()
        if self.keep_costs:
            self.last_S = self._S_dev.cpu().numpy()

        w_epsilon = self._moving_median_filter(xx=w_epsilon, window_size=10)
        u += w_epsilon

        optimal_traj = np.zeros((self.T, self.dim_x))
        if self.visualize_optimal_traj:
            self._g(u)                                     # _g(u[t-1]) for every row, in place (control.py:133)
            optimal_traj = eng.optimal_traj_host(x0, u)

        if self.visualze_sampled_trajs:
            tr = eng.trajectories(base_u=None, noise=self._noise_dev)   # pre-update u, v[k, t-1]
            sampled_traj_list = self._sampled_host(tr, world)
        else:
            sampled_traj_list = np.zeros((self.K, self.T, self.dim_x))

        self.u_prev[:-1] = u[1:]
        self.u_prev[-1] = u[-1]
        self._prefetch_noise(eng)
        return u[0], u, optimal_traj, sampled_traj_list

    def _sampled_host(self, tr: torch.Tensor, world: int) -> np.ndarray:
        """sampled_traj_list (K, T, 4) fp64 (control.py:135-145) from the device re-roll: widened to fp64 on
        the device and read back into a host array that is returned as is (no second 134 MB copy into an
        np.zeros; SampledReadback); the ranks' shards gathered into one array with a process group."""
        if world > 1:
            from .distributed import gather_trajectories
            out = np.zeros((self.K, self.T, self.dim_x))
            gather_trajectories(tr, self.K, out, self.process_group)
            return out
        return self._sampled_pool(tr)

    def _tick(self, observed_x):
        """The whole call in one native step (mppi_dropin_tick) when the buffers it
        binds are plain arrays: the fp64 nearest-waypoint update and end-of-path
        check of control.py:70-78 (the same operations as _get_nearest_waypoint),
        then the fused device step of _dropin_step.  None: not applicable, take the
        general path."""
        path, u = self.ref_path, self.u_prev
        if not (isinstance(path, np.ndarray) and path.dtype == np.float64 and path.ndim == 2 and path.shape[1] >= 4
                and path.strides[1] == 8 and path.strides[0] % 8 == 0 and path.strides[0] >= 32
                and isinstance(u, np.ndarray) and u.dtype == np.float64
                and u.shape == (self.T, 2) and u.flags.c_contiguous and u.flags.writeable):
            return None
        sig = self.Sigma
        if not (isinstance(sig, np.ndarray) and sig.shape == (self.dim_u, self.dim_u)):
            return None                                    # the general path raises as the reference does
        key = self._engine_key()
        if self._engine is None or key != self._engine_built_for:
            return None                                    # (re)build on the general path (LinAlgError order kept)
        eng = self._engine
        okey = self._okey                                  # this call's discs (_calc_control_input)
        self._push_obstacles(eng, okey)
        bkey = (eng, path, u, self.keep_costs, self.visualize_optimal_traj, self.seed, self.l1, self.l2,
                self._noise_dev)                           # (a NumPy-noise run swaps the noise buffers)
        if self._bound is None or any(a is not b for a, b in zip(bkey, self._bound)):
            self._x_buf = np.zeros(4)
            self._idx_buf = np.zeros(2, dtype=np.int64)
            self._traj_buf = np.zeros((self.T, self.dim_x)) if self.visualize_optimal_traj else None
            eng.dropin_bind(path, float(self.l1), float(self.l2), self._x_buf, self._idx_buf, u, self._traj_buf,
                            self._noise_dev, self._noise_dev, self._S_dev if self.keep_costs else None, self.seed)
            self._bound = bkey
        if self._noise_ready != (self.seed, self._step_count):
            eng.philox_noise(self.seed, self._step_count, out=self._noise_dev)
        out = self._tick_bound(observed_x)
        # the next call may skip every check above while nothing they read has changed
        # (the same objects, scalars and array contents): calc_control_input's fast test
        if all(isinstance(a, np.ndarray) and a.dtype == np.float64
               for a in (self.Sigma, self.stage_cost_weight, self.terminal_cost_weight)):
            self._fast = (path, u, self.Sigma, self.stage_cost_weight, self.terminal_cost_weight, eng,
                          self._fast_scalars(), self.Sigma.tobytes(), self.stage_cost_weight.tobytes(),
                          self.terminal_cost_weight.tobytes(), okey)
        return out

    def _fast_scalars(self):
        """Every scalar _tick's checks and the engine key read (control.py's per-call reads of
        lambda, gamma, the exploration split, delta_t, l1/l2), plus the controller switches."""
        return (self.noise_source, self.host_update, self.visualze_sampled_trajs, self.process_group, self.K, self.T,
                self.param_lambda, self.param_gamma, self.param_exploration, self.delta_t, self.l1, self.l2,
                self.arm, self.seed, self.keep_costs, self.visualize_optimal_traj, self.verbose,
                self._noise_ready == (self.seed, self._step_count), self._clamp_key())

    def _tick_bound(self, observed_x):
        """The bound drop-in tick (engine built, buffers bound, the noise of this step in
        the buffer): stage x0 and the index, launch, allocate sampled_traj_list, wait."""
        eng = self._engine
        if type(observed_x) is np.ndarray and observed_x.shape == (4,):
            self._x_buf[:] = observed_x
        else:
            self._x_buf[:] = np.asarray(observed_x, dtype=np.float64).ravel()[:4]
        self._idx_buf[0] = self.prev_waypoints_idx
        self._step_count += 1
        rc = eng.dropin_tick_launch(self._step_count)
        self.prev_waypoints_idx = self._idx_buf.item(0)
        if rc != 0:                                        # MPPI_E_PATH_END: nothing was launched
            if self.verbose:
                self._print_update(int(self._idx_buf[1]), self.prev_waypoints_idx)
            self._step_count -= 1
            print("[ERROR] Reached the end of the reference path.")
            raise IndexError
        # the launched step is always consumed (its wait runs whatever is raised in between: a failing
        # print or allocation, KeyboardInterrupt), so the next launch never finds a tick still pending
        try:
            if self.verbose:
                self._print_update(int(self._idx_buf[1]), self.prev_waypoints_idx)
            sampled = self._fresh_sampled()                 # control.py:135, allocated while the launch runs
        finally:
            eng.dropin_tick_wait()
        self._noise_ready = (self.seed, self._step_count)
        if self.keep_costs:
            self.last_S = self._S_dev.cpu().numpy()
        traj = self._traj_buf.copy() if self._traj_buf is not None else np.zeros((self.T, self.dim_x))
        u = self.u_prev
        return u[0], u, traj, sampled

    def _dropin_step(self, eng: RolloutEngine, x0, window, u: np.ndarray):
        """control.py:81-152 on one device in one native call (mppi_step_dropin):
        rollouts + soft-min + weighted noise + median filter + u += w_eps + shift in
        the launch, the result read from host-mapped memory, the optimal trajectory
        in fp64 on the host from the update, then the next step's device noise queued
        behind the rollout.  u is self.u_prev (updated in place)."""
        nxt = self._noise_dev if self.noise_source == "device" else None
        u_new, traj = eng.step_dropin(x0, window, u, self._noise_dev,
                                      S_out=self._S_dev if self.keep_costs else None, next_noise=nxt,
                                      seed=self.seed, next_step=self._step_count,
                                      want_traj=self.visualize_optimal_traj)
        if nxt is not None:
            self._noise_ready = (self.seed, self._step_count)
        if self.keep_costs:
            self.last_S = self._S_dev.cpu().numpy()
        u[:] = u_new                                       # the shifted nominal, in place (aliasing kept)
        optimal_traj = traj if traj is not None else np.zeros((self.T, self.dim_x))
        return u[0], u, optimal_traj, self._fresh_sampled()

    def _fused_step(self, eng: RolloutEngine, x0, u: np.ndarray, world: int, predraw: bool = False):
        """control.py:81-152 with the update inside the launch (the multi-GPU merge
        launch, or the rollout when sampled trajectories are asked for): median filter
        + u += w_eps + shift on device, the result read from host-mapped memory, the
        optimal trajectory in fp64 on the host from the update.  u is self.u_prev
        (updated in place).  predraw: the next call's NumPy draw is queued behind the
        trajectory re-roll, so it runs during the sampled trajectories' read-back."""
        S_out = self._S_dev if self.keep_costs else None
        u_before = u.copy() if self.visualze_sampled_trajs else None
        if world == 1:
            eng.rollout(self._noise_dev, S_out=S_out, fused_update=True, host_out=True)
        else:
            self._multi_rollout(eng, S_out, fused=True)
        tr = None
        if self.visualze_sampled_trajs:
            tr = eng.trajectories(base_u=u_before, noise=self._noise_dev)   # pre-update u, v[k, t-1]
        if predraw:
            self._queue_predraw(eng)
        u_new, traj = eng.wait_outputs(x0 if self.visualize_optimal_traj else None)
        if self.keep_costs:
            self.last_S = self._S_dev.cpu().numpy()
        sampled_traj_list = (self._sampled_host(tr, world) if tr is not None
                             else np.zeros((self.K, self.T, self.dim_x)))
        # next step's noise after the last read-back: the draw overlaps the caller's
        # work between ticks instead of sitting in front of this call's wait
        self._prefetch_noise(eng)
        u[:] = u_new                                       # the shifted nominal, in place (aliasing kept)
        optimal_traj = traj if traj is not None else np.zeros((self.T, self.dim_x))
        return u[0], u, optimal_traj, sampled_traj_list

    # ------------------------------------------------------------ host helpers (reference semantics)
    def _get_nearest_waypoint(self, q1: float, q2: float, update_prev_idx: bool = False):
        """search the closest waypoint (control.py:200-232), host fp64"""
        prev_idx = self.prev_waypoints_idx
        x = self.l1 * np.cos(q1) + self.l2 * np.cos(q1 + q2)
        y = self.l1 * np.sin(q1) + self.l2 * np.sin(q1 + q2)
        win = self.ref_path[prev_idx:(prev_idx + SEARCH_IDX_LEN)]
        d = ((x - win[:, 0]) ** 2 + (y - win[:, 1]) ** 2) * 100
        nearest_idx = first_min_index(d) + prev_idx
        ref_x = self.ref_path[nearest_idx, 0]
        ref_y = self.ref_path[nearest_idx, 1]
        ref_dq1 = self.ref_path[nearest_idx, 2]
        ref_dq2 = self.ref_path[nearest_idx, 3]
        if update_prev_idx:
            if self.verbose:
                self._print_update(prev_idx, nearest_idx)
            self.prev_waypoints_idx = nearest_idx
        return nearest_idx, ref_x, ref_y, ref_dq1, ref_dq2

    @staticmethod
    def _print_update(prev_idx: int, nearest_idx: int) -> None:
        """the three progress lines of control.py:227-229"""
        print(f"0     prev_idx = {prev_idx}")
        print(f"0     nearest_idx = {nearest_idx}")
        print("======================updated=======================")

    def _moving_median_filter(self, xx: np.ndarray, window_size: int) -> np.ndarray:
        """median smoothing per input dimension (control.py:319-327)"""
        out = np.zeros(xx.shape)
        for d in range(xx.shape[1]):
            out[:, d] = median_filter(xx[:, d], size=window_size, mode='reflect')
        return out

    def close(self):
        self._close_noise_draw()
        if self._engine is not None:
            self._engine.close()
            self._engine = None
        self._noise_ready = None      # the next engine's noise buffer is fresh: draw again
        self._engine_built_for = None
        self._bound = None
        self._fast = None
        self._xmode = None
        self._sampled_pool.clear()
