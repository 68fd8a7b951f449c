"""n-link planar chain MPPI (BASELINE config 5: 7-DoF, K=131072 T=128).

The reference has no 7-DoF model; this model is build-defined (equations in
``oracle/chain_oracle.py`` and ``include/mppi_rocm.h``) and reduces to the
reference ``_F`` (control.py:234-263) at n = 2 with inertia := link length.
``ChainMPPIController`` keeps the reference controller's interface
(control.py:21-152) with ``dim_u = n``, ``dim_x = 2n``:
``calc_control_input(observed_x)`` -> (u0, u_seq, optimal_traj (T, 2n),
sampled_traj_list (K, T, 2n)); the cost is control.py:174-232 on the end
effector (x, y) and the first two joint rates (xydq_circle.txt's columns).

Device work runs in ``csrc/mppi_chain.hip`` through ``mppi_chain_*``; the host
keeps the O(T n) work in fp64 (nearest-waypoint update, noise draw, median
filter, update, shift), as ``controller.py`` does for the 2-link arm.  The
engine calls both ABIs have come from ``engine._Engine``, the noise draw and the
multi-GPU set-up from ``controller_base.MPPIControllerBase``.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field

import numpy as np
import torch
from scipy.ndimage import median_filter

from . import _native as N
from . import hostrng
from .controller_base import DeviceDrawn, MPPIControllerBase, _noise_check, first_min_index
from .distributed import exchange_partials, gather_trajectories, same_on_all_ranks, shard_geometry
from .engine import _Engine
from .params import ArmParams

SEARCH_IDX_LEN = 30  # control.py:203


def _tup(v):
    return field(default_factory=lambda: tuple(v))


@dataclass(frozen=True)
class ChainParams:
    """Link constants of the chain ("extended sys_params.py").  Defaults: the
    config-5 arm — 7 uniform slender links of 1 kg, total reach 2 m (the 2-link
    arm's l1 + l2), centre of mass at mid-link, I = m l^2 / 12, and joint drives
    with 0.1 kg m^2 armature and 1 N m s / rad viscous damping (without them the
    undamped 7-link chain collapses from its gravity-held pose and a few percent
    of T = 128 rollouts overflow)."""
    m: tuple = _tup([1.0] * 7)
    l: tuple = _tup([2.0 / 7.0] * 7)
    lc: tuple = _tup([1.0 / 7.0] * 7)
    I: tuple = _tup([(2.0 / 7.0) ** 2 / 12.0] * 7)
    fk: tuple = _tup([2.0 / 7.0] * 7)
    J: tuple = _tup([0.1] * 7)
    b: tuple = _tup([1.0] * 7)
    g: float = 9.81

    @property
    def n(self) -> int:
        return len(self.m)

    @staticmethod
    def from_arm2(arm=None) -> "ChainParams":
        """The reference 2-link model (control.py:11-18, 241-245): inertia := link length."""
        a = ArmParams() if arm is None else arm
        return ChainParams(m=(a.m1, a.m2), l=(a.l1, a.l2), lc=(a.lc1, a.lc2), I=(a.l1, a.l2),
                           fk=(a.fk_l1, a.fk_l2), J=(0.0, 0.0), b=(0.0, 0.0), g=a.g)


# Config-5 start pose: the end effector on xydq_circle.txt's first waypoint
# (least-squares IK with a smooth bend, computed once), at rest.
CHAIN7_X0 = np.array([1.481492] + [-0.320757] * 6 + [0.0] * 7)
# Noise covariance scaled with the gravity load each joint carries.
CHAIN7_SIGMA = np.diag([20.0, 16.0, 12.0, 8.0, 4.0, 2.0, 1.0])


def gravity_torque(q, P: ChainParams = ChainParams()) -> np.ndarray:
    """Joint torques that hold the chain still at q (the nominal's natural start)."""
    m, l, lc = map(np.asarray, (P.m, P.l, P.lc))
    tail = np.array([m[k + 1:].sum() for k in range(P.n)])
    g_th = P.g * (m * lc + l * tail) * np.cos(np.cumsum(q))
    return np.cumsum(g_th[::-1])[::-1]


def chain7_config() -> dict:
    """Constructor kwargs of the config-5 controller: run.py's constants (run.py:25-37) with the 7-link Sigma."""
    return dict(delta_t=0.006, horizon_step_T=128, number_of_samples_K=131072, param_exploration=0.0,
                param_lambda=100.0, param_alpha=0.98, sigma=CHAIN7_SIGMA.copy(),
                stage_cost_weight=np.array([0.5, 0.5, 5.0, 5.0]),
                terminal_cost_weight=np.array([5.0, 5.0, 50.0, 50.0]))


class ChainEngine(_Engine):
    """Owns one ``mppi_chain_ctx`` (one device, one shard of samples); noise layout [T][K_local][n] fp32."""

    WAIT_FOLLOWS_STREAM = True   # wait_outputs follows torch's current stream first (the arm's does not)

    def __init__(self, K_local: int, T: int, delta_t: float, param_lambda: float, param_alpha: float, sigma,
                 stage_cost_weight, terminal_cost_weight, param_exploration: float = 0.0,
                 chain: ChainParams = ChainParams(), K_total: int | None = None, k_offset: int = 0,
                 device: int | torch.device | None = None, precision: str = "f32", lanes_per_sample: int = 0,
                 param_gamma: float | None = None, u_min=None, u_max=None, clamp_nominal: bool = True):
        """u_min / u_max: torque limits per joint (a scalar or n values; None or +-inf: no limit on that side),
        as RolloutEngine's: every sampled control is clipped before the dynamics and the control cost (in the
        rollout's own precision), the re-rolled trajectories clip theirs, and with clamp_nominal (the reference
        with visualize_optimal_traj) the fused update clips the nominal too.  The context rejects NaN limits
        and u_min > u_max (ValueError)."""
        if precision not in ("f32", "f64"):
            raise ValueError("precision must be 'f32' or 'f64'")
        self.precision = precision
        self.n = chain.n
        cfg = N.ChainConfigC()
        self._set_limits(cfg, self.n, u_min, u_max, clamp_nominal)
        cfg.delta_t, cfg.param_lambda = float(delta_t), float(param_lambda)
        cfg.param_alpha, cfg.param_exploration = float(param_alpha), float(param_exploration)
        sig = np.asarray(sigma, dtype=np.float64)
        if sig.shape != (self.n, self.n):
            raise ValueError(f"sigma must be {self.n} x {self.n}")
        for i, v in enumerate(sig.ravel()):
            cfg.sigma[i] = float(v)
        for i in range(4):
            cfg.stage_cost_weight[i] = float(stage_cost_weight[i])
            cfg.terminal_cost_weight[i] = float(terminal_cost_weight[i])
        cfg.chain.n = self.n
        for f in ("m", "l", "lc", "I", "fk", "J", "b"):
            arr = getattr(cfg.chain, f)
            for i, v in enumerate(getattr(chain, f)):
                arr[i] = float(v)
        cfg.chain.g = float(chain.g)
        cfg.precision = 1 if precision == "f64" else 0
        cfg.lanes_per_sample = int(lanes_per_sample)
        # gamma as given (control.py:45 fixes it at construction); None: lambda (1 - alpha)
        cfg.param_gamma = float("nan") if param_gamma is None else float(param_gamma)
        super().__init__("mppi_chain_", self.n, 2 * self.n, cfg, K_local, T, K_total, k_offset, device)
        blocks, threads, poll, lps = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        N.check(self._lib.mppi_chain_ctx_info(self._ctx, C.byref(blocks), C.byref(threads), C.byref(poll),
                                              C.byref(lps)), "mppi_chain_ctx_info")
        self.blocks, self.threads, self.lanes_per_sample = blocks.value, threads.value, lps.value
        self.handoff = "poll" if poll.value else "counter"
        # what set_self_collision last gave the context: the clearance (None: disabled) and the cost
        self.self_clearance, self.self_collision_cost = None, 0.0
        # (resolved leniently, as set_moving_obstacles: the tools build engines on an older build of the library)
        self._c_set_self_collision = getattr(self._lib, "mppi_chain_set_self_collision", None)

    # -- self-collision (mppi_chain_set_self_collision) ------------------------
    @staticmethod
    def check_self_collision(clearance, cost) -> tuple[float | None, float]:
        """(clearance as a float or None for disabled, cost as a float), or ValueError: a clearance that is NaN,
        negative or infinite, a cost that is NaN, negative or infinite (checked with the feature disabled too)."""
        try:
            d = None if clearance is None else float(clearance)
            w = float(cost)
        except (TypeError, ValueError) as e:
            raise ValueError(f"self collision: {e}") from None
        if d is not None and not (d >= 0.0 and math.isfinite(d)):
            raise ValueError("self_clearance must be finite and >= 0 (None disables the self-collision cost)")
        if not (w >= 0.0 and math.isfinite(w)):
            raise ValueError("self_collision_cost must be finite and >= 0")
        return d, w

    def set_self_collision(self, clearance, cost: float = 1.0e10) -> None:
        """The cost on non-adjacent link pairs: two links b >= a + 2 collide when they cross or come within
        `clearance` (m, centre line to centre line; 0: crossings only), and every self-colliding step of a sample
        adds `cost` to its S (the final state once more): mppi_chain_set_self_collision.  In effect from the next
        launch of any kind; `clearance=None` disables it (the kernels launched before).  No device call.  A
        2-link chain has no such pair: accepted, without effect.  ValueError for a bad value."""
        d, w = self.check_self_collision(clearance, cost)
        if self._c_set_self_collision is None:
            raise ValueError("mppi_chain_set_self_collision: this build of the library has no self-collision cost")
        N.check(self._c_set_self_collision(self._ctx, 0 if d is None else 1, 0.0 if d is None else d, w),
                "mppi_chain_set_self_collision")
        self.self_clearance, self.self_collision_cost = d, w

    def self_hits(self, noise: torch.Tensor, K: int | None = None) -> tuple[np.ndarray, np.ndarray]:
        """Tests: the self-collision test of the first K samples per step as this context's rollout evaluates it
        (mppi_chain_debug_self_hits) -> (mask (K, T) uint32: bit i is pair i of the enumeration a ascending, then
        b ascending, over a < b, b >= a + 2; dir (K, T, 2 n) fp32 as obstacle_hits')."""
        self._sync_stream()
        self._check_noise(noise)
        K = self.K_local if K is None else int(K)
        mask = torch.zeros((K, self.T), dtype=torch.int32, device=self.device)
        d = torch.zeros((K, self.T, 2 * self.n), dtype=torch.float32, device=self.device)
        N.check(self._lib.mppi_chain_debug_self_hits(self._ctx, C.c_void_p(noise.data_ptr()), K,
                                                     C.c_void_p(mask.data_ptr()), C.c_void_p(d.data_ptr())),
                "mppi_chain_debug_self_hits")
        self.synchronize()
        return mask.cpu().numpy().view(np.uint32), d.cpu().numpy()

    def last_eta(self) -> float:
        """eta = sum_k exp(-(S_k - min S) / lambda) of the last update (wait_outputs) or weighted noise
        (weighted_noise) read back: 1 for one-hot weights, eta - 1 the weight outside the best sample."""
        v = C.c_double()
        N.check(self._lib.mppi_chain_last_eta(self._ctx, C.byref(v)), "mppi_chain_last_eta")
        return v.value

    def debug_slots(self, noise: torch.Tensor, S_out: torch.Tensor | None = None) -> np.ndarray:
        """Tests: one rollout (as rollout(noise, S_out)) through the slot-recording build of the
        kernel -> the window slot every sample picked at every step, (K_local, T) int32
        (mppi_chain_debug_slots; the 7-link chain only)."""
        self._sync_stream()
        self._check_noise(noise)
        if S_out is not None:
            assert S_out.dtype == torch.float64 and S_out.numel() >= self.K_local and S_out.device == self.device
        slots = torch.full((self.K_local, self.T), -1, dtype=torch.int32, device=self.device)
        N.check(self._lib.mppi_chain_debug_slots(self._ctx, C.c_void_p(noise.data_ptr()),
                                                 C.c_void_p(S_out.data_ptr()) if S_out is not None else None,
                                                 C.c_void_p(slots.data_ptr())), "mppi_chain_debug_slots")
        return slots.cpu().numpy()

    def obstacle_hits(self, noise: torch.Tensor, K: int | None = None) -> tuple[np.ndarray, np.ndarray]:
        """Tests: the collision test of the first K samples per step as this context's rollout evaluates it
        (mppi_chain_debug_obstacle_hits: its precision, its lanes per sample, its step and hit functions) ->
        (mask (K, T) uint64: bit 8 j + a link a touches disc j; dir (K, T, 2 n) fp32: cos th_a at a, sin th_a
        at n + a, the values the test ran on)."""
        self._sync_stream()
        self._check_noise(noise)
        K = self.K_local if K is None else int(K)
        mask = torch.zeros((K, self.T), dtype=torch.int64, device=self.device)
        d = torch.zeros((K, self.T, 2 * self.n), dtype=torch.float32, device=self.device)
        N.check(self._lib.mppi_chain_debug_obstacle_hits(self._ctx, C.c_void_p(noise.data_ptr()), K,
                                                         C.c_void_p(mask.data_ptr()), C.c_void_p(d.data_ptr())),
                "mppi_chain_debug_obstacle_hits")
        self.synchronize()
        return mask.cpu().numpy().view(np.uint64), d.cpu().numpy()


class ChainMPPIController(MPPIControllerBase):
    """control.py:20-152 for the n-link chain (dim_u = n, dim_x = 2n).

    ``precision``: the rollout arithmetic.  "f32" (fastest) or "f64" (ChainStateD, ~2.9x the time), or "auto"
    (the default): fp32 while the weights are one-hot, fp64 where they spread.  In fp32 a nearest-waypoint tie
    of a weighted sample can move its S by a whole stage-cost step, which reaches w_eps only when
    more than one sample carries weight; so after each fp32 step the spread of its weights, eta - 1 =
    sum_k exp(-(S_k - min S) / lambda) - 1 (mppi_chain_last_eta), is checked, and a step whose weights spread
    (eta - 1 > ETA_TOL) is run again in fp64 from the same inputs, as are the steps after it until the weights
    are one-hot again.  run.py's lambda = 100 keeps them one-hot (eta - 1 ~ 0): the fp32 step alone.

    ``u_min`` / ``u_max``: torque limits, a scalar or one value per joint (properties, re-read on every call:
    rebinding either rebuilds the engines before the next step), with the arm controller's meaning — the
    reference's clamp hook ``_g`` (control.py:166-172) switched on: the sampled controls are clipped before the
    dynamics and the control cost, the weights still multiply the unclamped noise, and with
    ``visualize_optimal_traj`` the updated nominal is clipped too.  Both engines of ``precision="auto"`` carry
    them.

    ``obstacles`` / ``obstacle_cost``: up to eight discs ``(cx, cy, r)`` that no link may touch, as on the arm
    controller: every colliding step of a sample, and its final state once more, adds ``obstacle_cost`` to its
    cost (mppi_chain_set_obstacles).  ``obstacle_velocities``: ``(n, 2)`` rows of ``(vx, vy)`` in m/s, one per disc,
    constant over the horizon of a call, or ``None`` for discs at rest (mppi_chain_set_moving_obstacles): ``obstacles``
    then holds the positions at the observed state, rollout step ``t`` tests its new state against the discs at
    ``c + v (t + 1) delta_t``, and the caller advances ``obstacles`` between calls.  Plain attributes, compared by value on every call, so they may be edited in
    place or rebound between calls; a bad value raises ValueError before anything is drawn or moved.  Every
    engine a step runs on (``precision="auto"``'s fp64 one, every rank's of a process group) gets them before its
    launch.

    ``self_clearance`` / ``self_collision_cost``: the cost on non-adjacent link pairs (mppi_chain_set_self_collision):
    links ``a`` and ``b >= a + 2`` collide when they cross or come within ``self_clearance`` metres, centre line to
    centre line (0: crossings only; ``None``, the default: off), and every self-colliding step of a sample, and its
    final state once more, adds ``self_collision_cost``.  Plain attributes too, compared by value on every call and
    pushed to whichever engine runs the step; a bad value raises ValueError before anything is drawn or moved.  A
    2-link chain has no such pair: accepted, without effect."""

    ETA_TOL = 1e-6   # weight outside the best sample above which precision="auto" takes the fp64 rollout

    def __init__(self, delta_t: float = 0.006, ref_path=0, horizon_step_T: int = 128,
                 number_of_samples_K: int = 131072, param_exploration: float = 0.0, param_lambda: float = 100.0,
                 param_alpha: float = 0.98, sigma: np.ndarray = CHAIN7_SIGMA,
                 stage_cost_weight: np.ndarray = np.array([0.5, 0.5, 5.0, 5.0]),
                 terminal_cost_weight: np.ndarray = np.array([5.0, 5.0, 50.0, 50.0]),
                 visualize_optimal_traj=True, visualze_sampled_trajs=False, *, chain: ChainParams = ChainParams(),
                 u_init=None, device: int | None = None, verbose: bool = False, noise: str = "numpy", seed: int = 0,
                 process_group=None, exchange: str = "auto", precision: str = "auto",
                 numpy_noise_on_device: bool = True, u_min=None, u_max=None, obstacles=None,
                 obstacle_cost: float = 1.0e10, obstacle_velocities=None, self_clearance=None,
                 self_collision_cost: float = 1.0e10) -> None:
        self.chain = chain
        if precision not in ("auto", "f32", "f64"):
            raise ValueError("precision must be 'auto', 'f32' or 'f64'")
        self.precision = precision
        self.dim_u, self.dim_x = chain.n, 2 * chain.n
        self.T, self.K = horizon_step_T, number_of_samples_K
        self.param_exploration, self.param_lambda, self.param_alpha = param_exploration, param_lambda, param_alpha
        self.param_gamma = self.param_lambda * (1.0 - self.param_alpha)
        self.Sigma = np.asarray(sigma, dtype=np.float64)
        self.stage_cost_weight, self.terminal_cost_weight = stage_cost_weight, terminal_cost_weight
        self.visualize_optimal_traj, self.visualze_sampled_trajs = visualize_optimal_traj, visualze_sampled_trajs
        self.delta_t, self.ref_path = delta_t, ref_path
        u0 = np.zeros(self.dim_u) if u_init is None else np.asarray(u_init, dtype=np.float64)
        self.u_prev = np.tile(u0, (self.T, 1)) if u0.ndim == 1 else u0.astype(np.float64).copy()
        self.prev_waypoints_idx = 0
        super().__init__(device=device, verbose=verbose, noise=noise, seed=seed, process_group=process_group,
                         exchange=exchange, numpy_noise_on_device=numpy_noise_on_device)
        self.u_min, self.u_max = u_min, u_max   # properties (MPPIControllerBase): torque limits of _g, validated
        self._limits()                          # u_min <= u_max
        self.obstacles = obstacles              # (n, 3) array-like of discs (cx, cy, r), n <= 8, or None
        self.obstacle_cost = obstacle_cost      # added to S per colliding step (and once for the final state)
        self.obstacle_velocities = obstacle_velocities   # (n, 2) array-like of (vx, vy) in m/s, or None: at rest
        self._obst_checked = None               # the last (obstacles bytes, cost, velocities) that passed the checks
        self._okey = None                       # this call's key (_obstacle_key), for _device_step
        self._obstacle_key()
        self.self_clearance = self_clearance            # m between the centre lines of non-adjacent links, or None: off
        self.self_collision_cost = self_collision_cost  # added to S per self-colliding step (and once for the final state)
        self._skey = self._self_key()                   # this call's (clearance, cost), for _device_step
        self._slots = {}               # rollout precision -> the parked state of its engine (_SLOT fields)
        self._active = None            # the precision whose engine the per-engine fields hold
        self._spread = False           # precision="auto": the last step's weights were spread (next step fp64)
        self.last_precision = None     # the rollout precision of the last step's result
        self.last_eta = None           # and the spread of its weights (eta, mppi_chain_last_eta)

    def _self_key(self):
        """self.self_clearance / self.self_collision_cost by value, checked (ValueError): what every engine of this
        call must hold (ChainEngine.self_clearance, self_collision_cost)."""
        return ChainEngine.check_self_collision(self.self_clearance, self.self_collision_cost)

    def _push_self_collision(self, eng, key) -> None:
        """Give the engine this call's self-collision setting unless it holds it already (no device call either
        way): a parked engine may hold an older one."""
        have = (eng.self_clearance, eng.self_collision_cost)
        if key[0] is None and have[0] is None:
            return                                          # off stays off, whatever cost came with it
        if key != have:
            eng.set_self_collision(*key)

    @property
    def host_update(self) -> bool:
        """The update of control.py:120-149 on the host: T < 5 (the device median filter needs T >= 5)."""
        return self.T < 5

    # the per-engine fields: the active engine's live here, the others' are parked in _slots
    _SLOT = ("_engine", "_engine_built_for", "_xmode", "_noise_ready", "_noise_dev", "_noise_alt", "_partial",
             "_S_dev", "_gathered")

    def _activate(self, precision: str) -> None:
        """Make the engine of `precision` (built on first use) the one the fields above refer to."""
        if self._active == precision:
            return
        if self._active is not None:
            self._slots[self._active] = {f: getattr(self, f, None) for f in self._SLOT}
        parked = self._slots.pop(precision, {})
        for f in self._SLOT:
            setattr(self, f, parked.get(f))
        self._active = precision

    def _engine_key(self):
        """The shared key plus the chain, the rollout precision and the torque limits with their mode."""
        return super()._engine_key() + (self.chain, self._active, self._clamp_key())

    def _get_engine(self, key=None) -> ChainEngine:
        key = self._engine_key() if key is None else key
        if self._engine is not None and key != self._engine_built_for:
            self._close_active()
        if self._engine is None:
            world, rank = self._shard()
            K_local, k_offset = shard_geometry(self.K, world, rank)
            device = self._device if self._device is not None else torch.cuda.current_device()
            # gamma is fixed at construction in the reference (control.py:45) while lambda is
            # re-read per call: the engine takes gamma as given, as the 2-link engine does
            lo, hi = self._limits() or (None, None)
            self._engine = ChainEngine(K_local, self.T, self.delta_t, self.param_lambda, self.param_alpha, self.Sigma,
                                       self.stage_cost_weight, self.terminal_cost_weight, self.param_exploration,
                                       self.chain, K_total=self.K, k_offset=k_offset, device=device,
                                       precision=self._active, param_gamma=self.param_gamma, u_min=lo, u_max=hi,
                                       clamp_nominal=bool(self.visualize_optimal_traj))
            self._noise_dev = self._engine.new_noise()
            self._noise_alt = None                         # the queued draw's buffer, made on first use
            self._partial = self._engine.new_partial()
            self._S_dev = torch.empty(K_local, dtype=torch.float64, device=self._engine.device)
            if world > 1:
                self._gathered = torch.empty(world * self._engine.partial_len, dtype=torch.float64,
                                             device=self._engine.device)
            self._xmode = None
            self._engine_built_for = key
        return self._engine

    def _effector(self, q):
        th = np.cumsum(q)
        fk = np.asarray(self.chain.fk)
        return float((fk * np.cos(th)).sum()), float((fk * np.sin(th)).sum())

    def _get_nearest_waypoint(self, x: float, y: float, update_prev_idx: bool = False):
        """control.py:200-232 on the end-effector position, host fp64"""
        prev_idx = self.prev_waypoints_idx
        win = self.ref_path[prev_idx:(prev_idx + SEARCH_IDX_LEN)]
        nearest_idx = first_min_index(((x - win[:, 0]) ** 2 + (y - win[:, 1]) ** 2) * 100) + prev_idx
        if update_prev_idx:
            if self.verbose:
                print(f"0     prev_idx = {prev_idx}")
                print(f"0     nearest_idx = {nearest_idx}")
                print("======================updated=======================")
            self.prev_waypoints_idx = nearest_idx
        return nearest_idx

    def calc_control_input(self, observed_x):
        self._okey = self._obstacle_key()                  # ValueError before anything is drawn or moved
        self._skey = self._self_key()                      # likewise
        if self._npre is not None and self.noise_source != "numpy":
            self._settle_predraw()                         # (the NumPy path settles it after its checks)
        u = self.u_prev
        x0 = np.asarray(observed_x, dtype=np.float64)
        self._get_nearest_waypoint(*self._effector(x0[:self.dim_u]), update_prev_idx=True)
        if self.prev_waypoints_idx >= self.ref_path.shape[0] - 1:
            print("[ERROR] Reached the end of the reference path.")
            raise IndexError
        auto = self.precision == "auto"
        prec = ("f64" if self._spread else "f32") if auto else self.precision
        if self.noise_source == "numpy":
            epsilon = self._device_reference_noise(prec)   # (it also queues the next call's draw beside this step)
            if epsilon is None:
                epsilon = self._reference_noise()
        else:
            epsilon = None
        step = self._step_count
        self._step_count += 1
        window = self.ref_path[self.prev_waypoints_idx:(self.prev_waypoints_idx + SEARCH_IDX_LEN)]
        out = self._device_step_x(prec, x0, window, u, epsilon, step)
        if auto:
            self._spread = self.last_eta - 1.0 > self.ETA_TOL
            if self._spread and prec == "f32":
                # the weights spread: this step again in fp64 from the same inputs (u is not updated yet)
                out = self._device_step_x("f64", x0, window, u, epsilon, step)
                self._spread = self.last_eta - 1.0 > self.ETA_TOL
        u_new, optimal_traj, sampled = out
        u[:] = u_new                                        # the shifted nominal, in place (aliasing kept)
        return u[0], u, optimal_traj, sampled

    def _device_step_x(self, prec: str, x0, window, u, epsilon, step: int):
        """_device_step; after an ExchangeError (raised on every rank of the step, no update applied) the same
        step again over the all-gather, which waits for the late rank, and the all-gather from then on."""
        try:
            return self._device_step(prec, x0, window, u, epsilon, step)
        except N.ExchangeError:
            # every rank re-runs the same step (a rank whose verdict differed would pair its retry with the
            # others' next step)
            if not same_on_all_ranks(("exchange retry", step), self.process_group):
                raise RuntimeError("multi-GPU exchange: the ranks disagree on the failed step; "
                                   "their nominals can no longer be kept in step") from None
            # a late rank is the ranks' property, not one engine's: every engine takes the all-gather from now on
            self._x_failed = True
            self._xmode = "rccl"
            for parked in self._slots.values():
                if parked.get("_xmode") is not None:
                    parked["_xmode"] = "rccl"
            self._noise_ready = None   # the fused step queues the next draw into the buffer: draw this one again
            return self._device_step(prec, x0, window, u, epsilon, step)

    def _device_step(self, prec: str, x0, window, u, epsilon, step: int):
        """control.py:81-149 of one step on the engine of rollout precision `prec`: the shifted updated
        nominal (T, n), the optimal trajectory and sampled_traj_list.  u (self.u_prev) is only read."""
        self._activate(prec)
        key = self._engine_key()
        if key != self._engine_built_for:
            np.linalg.inv(self.Sigma)                      # LinAlgError as control.py:106 (Sigma checked when it changes)
        eng = self._get_engine(key)
        self._push_obstacles(eng, self._okey)              # this call's discs, before any launch of this engine
        self._push_self_collision(eng, self._skey)         # ... and its self-collision setting
        if isinstance(epsilon, DeviceDrawn):               # a device draw, into one engine's buffer
            if epsilon.buf is not self._noise_dev:
                eng._sync_stream()
                self._noise_dev.copy_(epsilon.buf)         # the step re-run in the other precision
        elif isinstance(epsilon, hostrng.StdNoise):
            self._zbuf_ev = eng.upload_std_noise(epsilon, self._zbuf, self._noise_dev)
        elif epsilon is not None:
            eng.upload_noise(epsilon[eng.k_offset:eng.k_offset + eng.K_local], out=self._noise_dev)
        elif self._noise_ready != (self.seed, step):
            eng.philox_noise(self.seed, step, out=self._noise_dev)
        eng.set_step_inputs(x0, window, u)
        world, _ = self._shard()
        S_out = self._S_dev if self.keep_costs else None
        if world > 1 and self._xmode is None:
            self._multi_setup(eng, _noise_check(self, epsilon))
        self.last_precision = prec
        if self.T >= 5 and not self.visualze_sampled_trajs and (world == 1 or self._xmode == "launch"):
            # the update of control.py:120-149 inside the launch (the median of 10 is a selection and the
            # add the same fp64 add: the host path's values), one read-back, the optimal trajectory in fp64
            # on the host, the next step's device noise queued behind the launch; with a process group the
            # same launch trades the ranks' rows first (the in-launch exchange)
            eng.rollout(self._noise_dev, S_out=S_out, fused_update=True, exchange=world > 1, host_out=True)
            # the next step's draw right behind the launch and its read-back (stream order: it starts once
            # the rollout has read the buffer), so it runs under the host trajectory and the caller's work
            self._prefetch_noise(eng)
            sampled = self._fresh_sampled()                     # control.py:135, while the launch runs
            u_new, traj = eng.wait_outputs(x0 if self.visualize_optimal_traj else None)
            self.last_eta = eng.last_eta()
            if self.keep_costs:
                self.last_S = self._S_dev.cpu().numpy()
            return u_new, traj if traj is not None else np.zeros((self.T, self.dim_x)), sampled
        if world == 1:
            eng.rollout(self._noise_dev, S_out=S_out)
        elif self._xmode == "launch":
            eng.rollout(self._noise_dev, S_out=S_out, exchange=True)      # one launch: rows traded in-launch
        else:
            eng.rollout(self._noise_dev, S_out=S_out, partial_out=self._partial)
            exchange_partials(self._partial, self._gathered, self.process_group)
            eng.merge(self._gathered, world)
        w_epsilon = eng.weighted_noise()
        self.last_eta = eng.last_eta()
        if self.keep_costs:
            self.last_S = self._S_dev.cpu().numpy()
        w_epsilon = np.stack([median_filter(w_epsilon[:, d], size=10, mode="reflect")
                              for d in range(self.dim_u)], axis=1)   # control.py:319-327
        un = u + w_epsilon                                            # control.py:126 (u itself untouched here)
        optimal_traj = np.zeros((self.T, self.dim_x))
        if self.visualize_optimal_traj:
            self._g(un)                                    # _g(u[t-1]) for every row, in place (control.py:133)
            optimal_traj = eng.optimal_traj_host(x0, un)
        if self.visualze_sampled_trajs:
            tr = eng.trajectories(base_u=None, noise=self._noise_dev)
            if world > 1:
                sampled = np.zeros((self.K, self.T, self.dim_x))
                gather_trajectories(tr, self.K, sampled, self.process_group)
            else:
                sampled = self._sampled_pool(tr)   # the caller's alone, as a fresh array (SampledReadback)
        else:
            sampled = np.zeros((self.K, self.T, self.dim_x))
        self._prefetch_noise(eng)
        return np.concatenate([un[1:], un[-1:]]), optimal_traj, sampled   # control.py:148-149

    def _close_active(self):
        if self._engine is not None:
            self._engine.close()
            self._engine = None
        self._engine_built_for = None
        self._noise_ready = None       # a new engine's noise buffer is fresh: draw again
        self._xmode = None

    def close(self):
        self._close_noise_draw()
        self._close_active()
        for parked in self._slots.values():
            if parked.get("_engine") is not None:
                parked["_engine"].close()
        self._slots = {}
        self._sampled_pool.clear()
