"""Host logic the two drop-in controllers share (``controller.py``: the reference's 2-link arm,
``chain.py``: the n-link chain): ``MPPIControllerBase`` and its helpers.

What lives here is independent of the model: sharding over a process group and the choice of the multi-GPU
exchange, the reference's noise draw on NumPy's legacy global RNG (control.py:154-164) on the host or, bit for
bit, on the device (engine.NpDeviceStream), the draw queued for the next call beside a step ("predraw") and the
device-noise prefetch.  Each controller keeps its step paths, its engine and the buffers of that engine
(``_noise_dev``, ``_noise_alt``, ``_partial``, ``_S_dev``, ``_gathered``: plain attributes, set by its
``_get_engine``).
"""
from __future__ import annotations

import sys
import warnings
import weakref

import numpy as np
import torch

from . import hostrng
from .distributed import attach_exchange, check_exchange, same_on_all_ranks
from .engine import HostReadback, NpDeviceStream, _Engine


def first_min_index(d: np.ndarray) -> int:
    """``d.index(min(d))`` of control.py:213-215 on a 1-D array: Python's min()
    keeps d[0] and replaces it only on a strict '<', so a NaN at j > 0 is never
    chosen and a NaN at j = 0 is (np.argmin would return the first NaN)."""
    j = int(np.argmin(d))
    if d[j] != d[j]:                                   # a NaN somewhere: Python's rule
        j = 0 if d[0] != d[0] else int(np.nanargmin(d))
    return j


def _pinned_zbuf(buf, ev, n: int):
    """(buffer, None): a float64 host tensor of at least n values, page-locked where the host allows it,
    reused across calls once the event of the last DMA out of it has completed."""
    if ev is not None:
        ev.synchronize()
    if buf is None or buf.numel() < n:
        buf = None   # the old one is released first
        try:
            buf = torch.empty(n, dtype=torch.float64, pin_memory=True)
        except RuntimeError:
            buf = torch.empty(n, dtype=torch.float64)
    return buf, None


class DeviceDrawn:
    """The reference's draw (control.py:84) made on the device straight into an engine's noise buffer `buf`
    (engine.NpDeviceStream)."""

    def __init__(self, buf: torch.Tensor):
        self.buf = buf


def _noise_check(ctrl, epsilon):
    """The value the ranks compare at their first step to agree on the noise stream.  The reference's own draw
    (NumPy's global RNG, control.py:163): the RNG state it left, which the device draw and the host draw leave
    alike, so a rank that fell back to the host draw still agrees with one that drew on the device; a replaced
    _calc_epsilon: eps[0, 0, 0] + eps[-1, -1, -1] of its array; device noise: None (the seed is compared)."""
    if ctrl.noise_source != "numpy" or epsilon is None:
        return None
    if not ctrl._custom_epsilon():
        st = np.random.get_state()
        return (float(np.sum(np.asarray(st[1][:16], dtype=np.float64))), int(st[2]), int(st[3]), float(st[4]))
    if isinstance(epsilon, hostrng.StdNoise):
        K, T, du = epsilon.z.shape
        return epsilon.eps(0, 0, 0) + epsilon.eps(K - 1, T - 1, du - 1)
    return float(epsilon[0, 0, 0] + epsilon[-1, -1, -1])


class SampledReadback:
    """sampled_traj_list's host arrays (control.py:135-145): the device re-roll's fp32 states read back and
    widened to fp64 on the host (engine.HostReadback: chunked DMA of the fp32 bytes, host threads widening
    each landed chunk; fp32 -> fp64 is exact, so the values are the device-side widening's, with half the
    bytes over the host link: 2.5 -> ~1.3 ms at K = 65536, T = 64) into an array of a pool that no caller
    holds any more, returned as is.  An array is reused only when nothing outside the pool refers to it (views
    of it included: their base is that array), so every returned array is the caller's alone, as
    control.py:137's fresh np.zeros is; a reused array's pages are already mapped.

    The pool is bounded: at most MAX arrays and MAX_BYTES in all (a larger array, e.g. the chain's 1.9 GB at
    config 5, is a fresh one per call).  A CPU tensor (tests) is widened by torch."""

    MAX = 3                 # arrays held at most (run.py's loop holds one array across a call: it cycles through two)
    MAX_BYTES = 768 << 20   # bytes held at most (3 x 134 MB at K = 65536, T = 64 fit)

    def __init__(self):
        self._pool = []    # arrays
        self._rb = None    # engine.HostReadback of the device last read from

    def clear(self) -> None:
        self._pool = []    # arrays the caller still holds stay theirs
        if self._rb is not None:
            self._rb.close()
            self._rb = None

    def __len__(self) -> int:
        return len(self._pool)

    def _fill(self, tr: torch.Tensor, out: np.ndarray) -> np.ndarray:
        if not tr.is_cuda:
            np.copyto(out, tr.double().numpy())
            return out
        if self._rb is None or self._rb.device != tr.device:
            if self._rb is not None:
                self._rb.close()
            self._rb = HostReadback(tr.device)
        return self._rb.run(tr.contiguous(), out)

    def __call__(self, tr: torch.Tensor) -> np.ndarray:
        shape = tuple(tr.shape)
        pool = self._pool
        if pool and tuple(pool[0].shape) != shape:
            self._pool = pool = []   # K or T changed
        for arr in pool:
            if sys.getrefcount(arr) == 3:   # the pool list's reference, the loop variable's and the argument's
                return self._fill(tr, arr)
        arr = np.empty(shape)
        if len(pool) < self.MAX and (len(pool) + 1) * arr.nbytes <= self.MAX_BYTES:
            pool.append(arr)
        return self._fill(tr, arr)


class MPPIControllerBase:
    """What MPPIControllerForPathTracking and ChainMPPIController share.  A subclass sets the reference's
    attributes (K, T, dim_u, dim_x, Sigma, the cost weights, visualze_sampled_trajs, ...), has a ``host_update``
    attribute or property (the update of control.py:120-149 runs on the host) and a ``_get_engine(key)`` that
    builds its engine and that engine's buffers.  The torque limits (``u_min`` / ``u_max``, the clamp hook _g)
    are kept here, sized by ``dim_u``: a subclass assigns them after ``dim_u`` and appends ``_clamp_key()`` to
    its engine key."""

    def __init__(self, *, device, verbose: bool, noise: str, seed: int, process_group, exchange: str,
                 numpy_noise_on_device: bool) -> None:
        if noise not in ("numpy", "device"):
            raise ValueError("noise must be 'numpy' or 'device'")
        self.verbose, self.noise_source, self.seed = verbose, noise, int(seed)
        self.process_group = process_group
        if exchange not in ("auto", "launch", "rccl"):
            raise ValueError("exchange must be 'auto', 'launch' or 'rccl'")
        self.exchange = exchange
        self._xmode = None             # multi-GPU exchange in use: "launch" / "rccl" (decided at the first step)
        self._x_failed = False         # an in-launch exchange failed (a late rank): the all-gather for good
        self._device = device
        self._engine = None
        self._engine_built_for = None  # _engine_key() of the live engine
        self._step_count = 0
        self._noise_ready = None       # (seed, step) of the device noise already in the buffer
        self.keep_costs = False        # set True to keep per-sample S (self.last_S)
        self.last_S = None
        self._last_sampled = None      # the previous call's sampled_traj_list (_fresh_sampled)
        self._sampled_pool = SampledReadback()   # sampled_traj_list's read-back arrays
        self.numpy_noise_on_device = numpy_noise_on_device   # noise="numpy": the same stream drawn on the device
        self._npdev = None             # its engine.NpDeviceStream (False: unavailable here)
        self._npre = None              # (start state, spec, buffer) of the next call's draw, queued beside a step
        self._np_spec = None           # (spec, plan) of this call's device draw
        self._np_left = None           # the state this call's draw left np.random in
        self._np_plan = None           # (Sigma bytes, dtype, hostrng.device_plan) of the last draw
        self._npre_used = 0            # calls that used the queued draw
        self._np_recorded = {}         # id -> weakref of the noise buffers already record_stream'ed on the draw stream
        self._noise_alt = None         # the second noise buffer: the queued draw writes it while a step reads the other
        self._np_stream = None         # the stream of the queued draws (concurrent with the step)
        self._np_ev = None

    # ------------------------------------------------------------ torque limits (_g, control.py:166-172)
    def _limit(self, name: str, value):
        """A limit as the controller stores it: None, or a read-only fp64 (dim_u,) array (a scalar is broadcast)."""
        if value is None:
            return None
        n = self.dim_u
        a = np.asarray(value, dtype=np.float64)
        if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != n):
            raise ValueError(f"{name} must be a scalar or have one value per control component ({n})")
        a = np.array(np.broadcast_to(a, (n,)))
        if np.isnan(a).any():
            raise ValueError(f"{name} must not be NaN (use +-inf or None for no limit)")
        a.setflags(write=False)     # rebind to change: the engine key reads the bytes cached at the assignment
        return a

    @property
    def u_min(self):
        """Lower torque limits, fp64 (dim_u,), or None; with u_max the np.clip bounds of _g.  Read on every call like
        the reference's other attributes: rebinding either rebuilds the engine before the next step."""
        return self._u_min

    @u_min.setter
    def u_min(self, value) -> None:
        self._u_min = self._limit("u_min", value)
        self._limits_key = None

    @property
    def u_max(self):
        """Upper torque limits, fp64 (dim_u,), or None."""
        return self._u_max

    @u_max.setter
    def u_max(self, value) -> None:
        self._u_max = self._limit("u_max", value)
        self._limits_key = None

    def _limits(self):
        """(lo, hi) fp64 (dim_u,) with +-inf for an absent side, or None without limits; ValueError if lo > hi."""
        lo, hi = self._u_min, self._u_max
        if lo is None and hi is None:
            return None
        lo = np.full(self.dim_u, -np.inf) if lo is None else lo
        hi = np.full(self.dim_u, np.inf) if hi is None else hi
        if (lo > hi).any():
            raise ValueError(f"u_min {lo.tolist()} exceeds u_max {hi.tolist()}")
        return lo, hi

    def _clamp_key(self):
        """What the engine bakes in of the limits: its clamp mode (2: _g also clips the updated nominal, which
        the reference does in its optimal-trajectory loop, so with visualize_optimal_traj only; control.py:130-133)
        and the limits' bytes; (0,) without limits."""
        if self._limits_key is None:
            lim = self._limits()
            self._limits_key = () if lim is None else (lim[0].tobytes(), lim[1].tobytes())
        if not self._limits_key:
            return (0,)
        return (2 if self.visualize_optimal_traj else 1,) + self._limits_key

    def _g(self, v: np.ndarray) -> float:
        """clamp input (control.py:166-172, whose two np.clip lines are commented out): with u_min / u_max
        set, v (one control, or rows of them) is clipped in place, as those lines would; else the identity"""
        lim = self._limits()
        if lim is not None:
            np.clip(v, lim[0], lim[1], out=v)
        return v

    # ------------------------------------------------------------ obstacles (both drop-ins)
    def _obstacle_key(self):
        """self.obstacles / self.obstacle_cost / self.obstacle_velocities by value: None without discs, else (the
        (n, 3) fp64 bytes, the cost[, the (n, 2) velocity bytes]), checked (ValueError for a bad shape or value,
        and for velocities without discs).  Compared on every call, the bound tick's too, so a rebind and an
        in-place edit are both seen.  A subclass sets the plain attributes and ``_obst_checked = None`` (the
        last key that passed the checks)."""
        vel = getattr(self, "obstacle_velocities", None)   # (a controller without moving obstacles has none)
        a = None
        if self.obstacles is not None:
            try:
                a = np.array(self.obstacles, dtype=np.float64, ndmin=1)
            except (TypeError, ValueError) as e:
                raise ValueError(f"obstacles: {e}") from None
        if a is None or a.size == 0:
            if vel is not None:
                raise ValueError("obstacle_velocities given without obstacles")
            return None
        try:
            key = (a.shape, a.tobytes(), float(self.obstacle_cost))
        except (TypeError, ValueError) as e:
            raise ValueError(f"obstacle_cost: {e}") from None
        if vel is not None:
            # by value, beside the discs: a rebind and an in-place edit are both seen; a key of three entries is
            # the static one, so None and discs at rest given as zeros are told apart only by the call they take
            try:
                v = np.array(vel, dtype=np.float64, ndmin=1)
            except (TypeError, ValueError) as e:
                raise ValueError(f"obstacle_velocities: {e}") from None
            key += (v.shape, v.tobytes())
        if key != self._obst_checked:
            a, _ = _Engine.check_obstacles(a, self.obstacle_cost)
            _Engine.check_velocities(vel, a.shape[0])
            self._obst_checked = key
        return key

    def _push_obstacles(self, eng, key) -> None:
        """Give the engine this call's discs and velocities unless it holds them already (no device call either
        way)."""
        have = eng.obstacles
        have = (have.shape, have.tobytes(), eng.obstacle_cost) if have.shape[0] else None
        hv = getattr(eng, "obstacle_velocities", None)
        if have is not None and hv is not None:
            have += (hv.shape, hv.tobytes())
        if key != have:
            if key is None:
                eng.set_obstacles(None, self.obstacle_cost)
            elif getattr(self, "obstacle_velocities", None) is None:
                eng.set_obstacles(self.obstacles, self.obstacle_cost)
            else:
                eng.set_obstacles(self.obstacles, self.obstacle_cost, velocities=self.obstacle_velocities)

    # ------------------------------------------------------------ engine
    def _shard(self):
        if self.process_group is None:
            return 1, 0
        import torch.distributed as dist
        return dist.get_world_size(self.process_group), dist.get_rank(self.process_group)

    def _engine_key(self):
        """What every engine bakes in at creation that the reference reads on every call (Sigma at
        control.py:84,106; lambda :112; gamma :106; the cost weights :185,198; the exploration split :98;
        delta_t :256-259; the sample count and horizon self.K / self.T of :81-95); a subclass appends its
        model's.  A change rebuilds the engine before the next step."""
        return (int(self.K), int(self.T), np.asarray(self.Sigma, dtype=np.float64).tobytes(), float(self.param_lambda),
                float(self.param_gamma), np.asarray(self.stage_cost_weight, dtype=np.float64).tobytes(),
                np.asarray(self.terminal_cost_weight, dtype=np.float64).tobytes(), float(self.param_exploration),
                float(self.delta_t))

    def _activate(self, precision) -> None:
        """Make the engine of rollout precision `precision` the live one (the chain keeps one per precision;
        the arm has one engine: nothing to do)."""

    def _multi_setup(self, eng, noise_check) -> None:
        """First multi-GPU step of an engine (collective, every rank): check that the
        ranks agree on the noise stream, then pick the exchange — the in-launch one
        (distributed.attach_exchange) if its one-step self-check against the
        all-gather + merge passes (distributed.check_exchange), else RCCL."""
        pg = self.process_group
        if not same_on_all_ranks((self.K, self.T, self.noise_source, self.seed, noise_check), pg):
            raise RuntimeError("ranks disagree on the noise stream: every rank must seed np.random identically "
                               "(and pass the same seed / K / T)")
        mode = "rccl"
        if self.exchange != "rccl" and not self._x_failed:   # after a failed exchange: the all-gather for good
            self.exchange_report = {}                      # why an exchange was (not) picked (distributed.py)
            ok = attach_exchange(eng, pg, report=self.exchange_report)
            ok = ok and check_exchange(eng, self._noise_dev, self._partial, self._gathered, pg,
                                       report=self.exchange_report)
            if not ok and self.exchange == "launch":
                raise RuntimeError("the in-launch exchange failed its self-check (exchange='launch')")
            mode = "launch" if ok else "rccl"
        self._xmode = mode

    def _fresh_sampled(self) -> np.ndarray:
        """A fresh writable zero array for sampled_traj_list (control.py:137: np.zeros each call, 134 MB at
        K = 65536, T = 64; 1.9 GB at config 5, mapped lazily), made while the launch runs.  The controller keeps
        the previous call's array until now, so if the caller has dropped it, its unmapping (~12 us) also happens
        here, under the launch, instead of in the caller after the call returns; an array the caller still holds
        is untouched."""
        out = np.zeros((self.K, self.T, self.dim_x))
        self._last_sampled = out
        return out

    def _prefetch_noise(self, eng) -> None:
        """Device noise: draw the next step's noise now (stream-ordered after every
        reader of this step's), so the next call does not wait for it."""
        if self.noise_source == "device":
            eng.philox_noise(self.seed, self._step_count, out=self._noise_dev)
            self._noise_ready = (self.seed, self._step_count)

    # ------------------------------------------------------------ the reference's noise draw
    @staticmethod
    def _check_sigma(sigma, size_dim_u):
        if sigma.shape[0] != sigma.shape[1] or sigma.shape[0] != size_dim_u or size_dim_u < 1:
            print("[ERROR] sigma must be a square matrix with the size of size_dim_u.")
            raise ValueError

    def _calc_epsilon(self, sigma: np.ndarray, size_sample: int, size_time_step: int, size_dim_u: int) -> np.ndarray:
        """sample epsilon (control.py:154-164) — the reference's RNG stream"""
        self._check_sigma(sigma, size_dim_u)
        mu = np.full((size_dim_u), 0.0)
        return hostrng.multivariate_normal(mu, sigma, (size_sample, size_time_step))   # NumPy's values, threaded

    def _custom_epsilon(self) -> bool:
        """_calc_epsilon replaced on the instance or a subclass: the caller's noise, not the reference's draw."""
        return "_calc_epsilon" in self.__dict__ or type(self)._calc_epsilon is not MPPIControllerBase._calc_epsilon

    def _zbuf_numpy(self, n: int) -> np.ndarray:
        """The page-locked buffer of the standard normals (>= n values), free to be rewritten: the DMA of the
        previous draw out of it has completed."""
        self._zbuf, self._zbuf_ev = _pinned_zbuf(getattr(self, "_zbuf", None), getattr(self, "_zbuf_ev", None), n)
        return self._zbuf.numpy()

    def _reference_noise(self):
        """control.py:84, the reference's draw on the legacy global RNG.  When _calc_epsilon is the reference's
        (not replaced on the instance or a subclass) and Sigma's transform is a scaled column permutation
        (run.py's 20 I, the chain's diagonal Sigma), the draw stops at its standard normals: NumPy's values,
        written into a page-locked buffer that goes to the device in one DMA, where the same fp64 multiply and
        add make the noise (hostrng.multivariate_normal_std, the engine's upload_std_noise) instead of NumPy's
        np.dot and `x += mean` over the 67 MB draw and a pageable copy.  Otherwise _calc_epsilon's array."""
        if self._custom_epsilon():
            return self._calc_epsilon(self.Sigma, self.K, self.T, self.dim_u)
        self._check_sigma(self.Sigma, self.dim_u)
        std = hostrng.multivariate_normal_std(np.full((self.dim_u), 0.0), self.Sigma, (self.K, self.T),
                                              self._zbuf_numpy(self.K * self.T * self.dim_u))
        return std if std is not None else self._calc_epsilon(self.Sigma, self.K, self.T, self.dim_u)

    @staticmethod
    def _same_np_state(a, b) -> bool:
        return (a[0] == b[0] and a[2] == b[2] and a[3] == b[3] and a[4] == b[4]
                and np.array_equal(a[1], b[1]))

    def _drop_predraw(self):
        """Wait for a queued draw this call does not use (its buffer may be rewritten or freed next); None."""
        if self._npre is not None:
            self._settle_predraw()
        return None

    def _settle_predraw(self):
        """Wait for the draw queued by the last call: (the state it started from, its spec, its buffer, the state
        it leaves), or None.  Settled before anything may rewrite or free its buffer."""
        pre, self._npre = self._npre, None
        new = self._npdev.result()
        return None if new is None else (pre[0], pre[1], pre[2], new)

    def _queue_predraw(self, eng) -> None:
        """The next call's draw, queued from the state this call's draw left, into the engine's second noise
        buffer on a stream of its own: it runs beside the step and while the caller works between calls.  Its
        stream first waits for the work already queued on the engine's stream (the last step, which read that
        buffer).  The next call uses it only if NumPy's state is still that one, it runs on the same engine
        (the chain's precision="auto" may switch engines) and nothing the draw depends on has changed
        (_device_reference_noise); otherwise it draws again, so the values and state are NumPy's either way."""
        spec, plan = self._np_spec
        state = self._np_left                              # np.random's state after this call's draw
        eng._sync_stream()
        if self._noise_alt is None:
            self._noise_alt = eng.new_noise()
        if self._np_stream is None:
            self._np_stream = torch.cuda.Stream(device=eng.device)
            self._np_ev = torch.cuda.Event()
        self._np_ev.record(eng.stream)
        self._np_stream.wait_event(self._np_ev)
        rec = self._np_recorded.get(id(self._noise_alt))
        if rec is None or rec() is not self._noise_alt:
            # its block is not reused before the draws on that stream have run (recorded once per tensor: the
            # allocator keeps the stream with the block until it is freed)
            self._noise_alt.record_stream(self._np_stream)
            if len(self._np_recorded) >= 4:
                self._np_recorded.clear()
            self._np_recorded[id(self._noise_alt)] = weakref.ref(self._noise_alt)
        self._npdev.draw(state, (int(self.K), int(self.T), self.dim_u), plan, self._noise_alt,
                         self._np_stream.cuda_stream, eng.k_offset, eng.K_local,
                         (eng.K_local * self.dim_u, self.dim_u, 1))
        self._npre = (state, spec, self._noise_alt)

    def _device_reference_noise(self, prec=None):
        """control.py:84 on the device: the reference's own stream (np.random.multivariate_normal on the legacy
        global RNG, NumPy's values and the state it leaves) drawn straight into the noise buffer of the engine
        the step runs on first (the `prec` one of the chain, which copies it over when it re-runs a step in the
        other precision; engine.NpDeviceStream, include/mppi_rocm.h mppi_np_*), when _calc_epsilon is the
        reference's and Sigma's transform is a scaled column permutation (run.py's 20 I) or, for the 2-link arm,
        any matrix whose np.dot rounding hostrng.dot2_model pins.  None: not applicable here (the host path
        draws then; nothing was drawn).  A singular Sigma takes the host path too, which draws before
        np.linalg.inv raises, as control.py:84,106 do.  The draw the last call queued is waited for only after
        these checks (they run while it does), and used when it started from NumPy's current state on this
        engine.  On one device with the update in the launch and no sampled trajectories, the next call's draw
        is queued here, while the device is idle (the step follows on the engine's own stream)."""
        if not self.numpy_noise_on_device or self._npdev is False:
            return self._drop_predraw()
        if self._custom_epsilon():
            return self._drop_predraw()
        sig = self.Sigma
        if not (isinstance(sig, np.ndarray) and sig.shape == (self.dim_u, self.dim_u)):
            return self._drop_predraw()                    # the host path prints and raises as the reference
        n = int(self.K) * int(self.T) * self.dim_u
        if n < hostrng._MIN_NORMALS or n >= 2 ** 31:
            return self._drop_predraw()
        state = np.random.get_state()
        if state[0] != "MT19937":
            return self._drop_predraw()
        sb = sig.tobytes()
        if self._np_plan is None or self._np_plan[0] != sb or self._np_plan[1] != sig.dtype:
            self._np_plan = (sb, sig.dtype, hostrng.device_plan(np.full((self.dim_u), 0.0), sig))
        plan = self._np_plan[2]
        if plan is None:
            return self._drop_predraw()
        self._activate(prec)
        key = self._engine_key()
        if key != self._engine_built_for:
            self._drop_predraw()                           # the engine and its buffers may be rebuilt below
            try:
                np.linalg.inv(sig)
            except np.linalg.LinAlgError:
                return None
        eng = self._get_engine(key)
        if self._npdev is None:
            try:
                self._npdev = NpDeviceStream(eng.device)
            except (RuntimeError, OSError):
                self._npdev = False
                return None
        if not plan[3]:
            warnings.warn("covariance is not symmetric positive-semidefinite.", RuntimeWarning)   # NumPy's
        spec = (int(self.K), int(self.T), self.dim_u, eng, eng.k_offset, eng.K_local, sb)
        self._np_spec = (spec, plan)
        new = None
        if self._npre is not None:
            pre = self._settle_predraw()
            if (pre is not None and pre[1] == spec and pre[2] is self._noise_alt
                    and self._same_np_state(pre[0], state)):
                new = pre[3]                               # drawn beside the last step: NumPy's values
                self._noise_dev, self._noise_alt = self._noise_alt, self._noise_dev
                self._npre_used += 1
        if new is None:
            eng._sync_stream()
            self._npdev.draw(state, (int(self.K), int(self.T), self.dim_u), plan, self._noise_dev,
                             eng.stream.cuda_stream, eng.k_offset, eng.K_local,
                             (eng.K_local * self.dim_u, self.dim_u, 1))   # [T][K_local][dim_u]
            new = self._npdev.result()
        if new is None:
            return None
        self._np_left = new
        if not self.host_update and not self.visualze_sampled_trajs and self._shard()[0] == 1:
            self._queue_predraw(eng)                       # the next call's draw, beside this call's step
        np.random.set_state(new)
        return DeviceDrawn(self._noise_dev)

    # ------------------------------------------------------------ lifetime
    def __del__(self):  # pragma: no cover - best effort
        try:
            self._drop_predraw()                           # a queued draw still writes _noise_alt
        except Exception:
            pass

    def _close_noise_draw(self) -> None:
        """close(): wait for a queued draw (its buffer outlives it), then release the device draw."""
        self._drop_predraw()
        if self._npdev:
            self._npdev.close()
        self._npdev = None
