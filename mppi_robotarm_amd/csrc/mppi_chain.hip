// mppi_chain.hip — MI355X (gfx950) MPPI engine for an n-link planar chain
// (BASELINE config 5: "7-DoF arm dynamics (extended sys_params.py), K=131072
// T=128, xydq_circle.txt reference").  The reference has no 7-DoF model; the
// model is build-defined (oracle/chain_oracle.py, equations there) and reduces
// to the reference's _F (control.py:234-263) at n = 2 with inertia := length.
//
//  * chain_rollout_kernel<N>: one lane per sample, the whole n-link step in
//    fp32 registers (fully unrolled for N): prefix sums -> cos/sin of the
//    absolute-angle differences from the cached sincos -> D = mu o cos(.) + I,
//    Coriolis/centrifugal and gravity terms -> Cholesky of D (v_rsq) -> two
//    triangular solves -> joint accelerations -> semi-implicit Euler -> new
//    sincos (shared with the next step and the end-effector kinematics) ->
//    the window search of the 2-link engine -> stage + control cost.  Noise is
//    [T][K][N] fp32 (like the 2-link engine's [T][K][2]): a sample's N values of
//    a step contiguous, so a weighted sample's noise is T cache lines.  Same epilogue,
//    in-launch merges and fused update as the 2-link engine (mppi_device.h, mppi_merge.h),
//    with T*N columns per partial row (MAXCH = 4 column chunks).
//  * chain_traj_kernel<N, NOISE>, chain_philox_kernel: trajectory re-roll and
//    counter-based Gaussian noise with an n x n Cholesky factor.
//  * torque limits (mppi_chain_config.clamp_mode; the reference's clamp hook _g, control.py:166-172, switched
//    on, per joint): the CLAMP instantiations of the rollout, merge and trajectory kernels clip every sampled
//    control (v_med3_f32 in the fp32 forms, fp64 compares in the fp64 one) and, in mode 2, the updated nominal
//    in fp64.  The limits travel in ChainClampK, the kernels' last argument, which the other instantiations
//    never read.
//  * workspace obstacles (mppi_chain_set_obstacles): the OBST instantiations of the rollout kernel, in its three forms,
//    test every link against up to eight discs after every step and add cost x (colliding states) to S.  The discs
//    travel in ChainObstK, the last argument after ChainClampK; a context without discs launches the kernels it
//    launched before.
//  * self-collision (mppi_chain_set_self_collision): the SELF instantiations of the CLAMP + OBST rollout kernels test
//    every pair of non-adjacent links after every step (crossing, or closer than the clearance) and add
//    cost x (self-colliding states) to S.  The clearance and cost travel in ChainSelfK, the last argument after
//    ChainObstK; a context with the feature off launches the kernels it launched before.
//
// C ABI: include/mppi_rocm.h (mppi_chain_*).
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "mppi_device.h"
#include "mppi_host.h"
#include "mppi_rocm.h"

namespace {

using namespace mppi;

constexpr int kCMax = MPPI_CHAIN_MAX_DOF;   // links
constexpr int kCDebugN = 7;                  // the link count with slot-recording debug instances (config 5)
constexpr int kCT = 256;                    // threads per workgroup, one lane per sample
constexpr int kCMaxCh = 4;                  // column chunks of a partial row: T N + 1 <= 4 x 256 ... (N <= 7)
constexpr int kCMaxVals = kMaxT * kCMax;    // T N values per row, at most
constexpr int kCPF = 2;                     // noise steps in flight per lane (N rows each)
// the same for a quad per sample (its steps are ~4x shorter); 2 and 4 measured: equal at K = 16384, 4 -2.1 % at
// K = 32768 (profiles/r13/chain_quad_ring_depth_ab.txt)
constexpr int kQPF = 4;
constexpr int kCPU = 2;                     // per-step constant rows in flight

// Device-resident per-step parameter block (ping-pong pair in the context).
struct alignas(16) ChainStep {
    float4 win[kSlots];                    // rx, ry, rdq1, rdq2 of window slot j
    float4 key[kSlots];                    // centred search keys (see Search)
    float4 ctr;                            // window centre (cx, cy), W
    float x0[2 * kCMax];                   // q[n], dq[n]
    double x0d[2 * kCMax];                 // the same in fp64 (fp64 rollout)
    double wind[kSlots][4];                // the window rows in fp64 (fp64 rollout); rows >= W unused
    float ua[kMaxT + kCPU][2 * kCMax];     // u_t[n], a_t[n] (a = (gamma u_t)^T Sigma^-1), fp32; rows >= T zero
    double u[kMaxT][kCMax];                // nominal control sequence, fp64
    double a[kMaxT][kCMax];                // a_t in fp64 (fp64 rollout)
    double u_first[kCMax];                 // fused update: u_new[0], the element the shift drops (optimal_traj)
    double eta;                            // fused update: the merge's eta (read back with u_first)
};

// Launch constants (kernel argument, by value).
constexpr int kCDyn = 72;
struct ChainConst {
    int K_local, T, k_offset, k_exploit, nblocks, acquire, n, cu_off;   // cu_off: per-CU tickets in counters[]
    int fair, pad0;   // fair: > 1 workgroup per CU (fair_priority)
    alignas(8) float dyn[kCDyn];   // packed dynamics / cost constants (layout: kOff* below)
    double lambda, inv_lambda, gamma;
    double sig_inv[kCMax * kCMax];
};

// Torque limits (mppi_chain_config.clamp_mode, u_min, u_max: _g of control.py:166-172 switched on, per joint):
// the fp64 limits (the fp64 rollout, the nominal's clamp) and their nearest fp32 values (the fp32 rollouts and
// re-rolls); entries d >= n are -inf / +inf.  The last argument of every kernel that takes it, read by the
// CLAMP instantiations only: the others keep the instructions they had without it (it is not part of
// ChainConst, whose growth would move the SGPR allocation of kernels that never read the limits).
struct ChainClampK {
    double u_lo[kCMax], u_hi[kCMax];
    float v_lo[kCMax], v_hi[kCMax];
    int mode;   // mppi_chain_config.clamp_mode
};
// the fp32 clip (the fp64 one is clamp_u, mppi_device.h): v_med3_f32 (lo <= hi is guaranteed by mppi_chain_ctx_create), no canonicalising v_max / v_min
__device__ __forceinline__ float clamp_v(float v, float lo, float hi) { return __builtin_amdgcn_fmed3f(v, lo, hi); }
// entry d (a lane value) of a by-value table, as selects over its N compile-time entries (no dynamic index
// into the kernel argument)
template <int N, class T>
__device__ __forceinline__ T pick(const T (&tab)[kCMax], int d) {
    T r = tab[0];
#pragma unroll
    for (int e = 1; e < N; ++e) r = d == e ? tab[e] : r;
    return r;
}

// Workspace obstacles (mppi_chain_set_obstacles): up to MPPI_MAX_OBSTACLES discs, the centres and r^2 in fp32 (the
// fp32 rollouts: ObstR's records, mppi_device.h) and in fp64 (the fp64 rollout), and the cost of one colliding
// state; an unused entry has r2 = -1, which no squared distance is below.  A per-launch input like x0: the last
// argument of the rollout kernel, after ChainClampK, read by the OBST instantiations only.
struct ChainObstK {
    float cx[MPPI_MAX_OBSTACLES], cy[MPPI_MAX_OBSTACLES], r2[MPPI_MAX_OBSTACLES];
    double cxd[MPPI_MAX_OBSTACLES], cyd[MPPI_MAX_OBSTACLES], r2d[MPPI_MAX_OBSTACLES];
    double w;
    int n;
    // moving discs (mppi_chain_set_moving_obstacles), behind everything there was: velocities in m/s, constant over
    // the horizon (0 at rest), in fp32 and fp64 like the centres; the fp64 time step; and whether any velocity is
    // not zero (the host's choice of the MOVE kernels; the kernels do not read it)
    float vx[MPPI_MAX_OBSTACLES], vy[MPPI_MAX_OBSTACLES];
    double vxd[MPPI_MAX_OBSTACLES], vyd[MPPI_MAX_OBSTACLES];
    double dt;
    int moving;
};
// The fp64 rollout's records of one step: cx[8], cy[8], r2[8] (chain_hits_f64)
constexpr int kObstRowD = 3 * MPPI_MAX_OBSTACLES;
// what mppi_chain_debug_obstacle_hits records: bit 8 j + a of a mask is link a against disc j
using ObstMask = unsigned long long;

using CScratch = MergeScratch<kCMaxVals>;

// The dynamics / cost constants, packed (floats, pairs 8-byte aligned).  The
// chain's coupling is separable: mu_ab = l_a nu_b for a < b (chain_oracle.py
// coefficients), so D' and the bias need only the per-link l and nu.  Pairs
// hold links / rows (2p, 2p+1); the pad link of an odd chain has l = nu = fk =
// damping = 0 and D'_aa = 1.  The rollout kernel reads them from a device copy
// through the constant address space every step (scalar loads re-issued after
// each step's scheduling boundary) rather than holding them in SGPRs across the
// loop, where they spill and return as v_readlane (~28 per step at n = 7).
enum : int {
    kOffL = 0,                    // l_a (dynamics link lengths)
    kOffNu = kOffL + kCMax,       // nu_a = m_a lc_a + l_a sum_{b>a} m_b
    kOffDd = kOffNu + kCMax,      // D'_aa = mu_aa + I_a + J_a + J_{a+1}
    kOffJ = kOffDd + kCMax,       // [a]: the pair holding row a+1 of column a: -J_{a+1} at row a+1, 0 beside it
    kOffDamp = kOffJ + 2 * kCMax, // joint viscous damping b_a
    kOffFk = kOffDamp + kCMax,    // cost kinematics lengths
    kOffSw = kOffFk + kCMax,      // stage weights x 10000
    kOffTw = kOffSw + 4,          // terminal weights x 10000
    kOffDt = kOffTw + 4,
    kOffG = kOffDt + 1,
    kDynFloats = kOffG + 7,
};
static_assert(kDynFloats == kCDyn, "dyn layout");
constexpr int kDynF64Off = (kCDyn + 1) & ~1;   // floats before the fp64 copy of the constants (8-B aligned)
// behind the fp64 copy: the fp32 torque limits, v_lo[kCMax] then v_hi[kCMax] (ChainClampK's), for the one-lane-
// per-sample CLAMP rollout, which reads them per step like the constants above (at n = 7 that kernel has no
// registers left to hold them across the horizon: held in VGPRs they spilled 30 to scratch)
constexpr int kDynLimOff = kDynF64Off + 2 * kCDyn;
constexpr int kDynBlockFloats = kDynLimOff + 2 * kCMax;

template <class F>   // F: const float (generic, kernel argument) or cfloat (constant address space)
struct Dyn {
    F* p;
    __device__ __forceinline__ f32x2 pair(int off, int i) const { return f32x2{p[off + 2 * i], p[off + 2 * i + 1]}; }
    __device__ __forceinline__ f32x2 l2(int i) const { return pair(kOffL, i); }
    __device__ __forceinline__ f32x2 nu2(int i) const { return pair(kOffNu, i); }
    __device__ __forceinline__ f32x2 damp2(int i) const { return pair(kOffDamp, i); }
    __device__ __forceinline__ f32x2 fk2(int i) const { return pair(kOffFk, i); }
    __device__ __forceinline__ f32x2 joff2(int a) const { return pair(kOffJ, a); }
    __device__ __forceinline__ float Dd(int a) const { return p[kOffDd + a]; }
    __device__ __forceinline__ float dt() const { return p[kOffDt]; }
    __device__ __forceinline__ float g() const { return p[kOffG]; }
};
using DynMem = Dyn<cfloat>;
using DynArg = Dyn<const float>;

__device__ __forceinline__ f32x2 splat(float x) { return f32x2{x, x}; }
__device__ __forceinline__ f32x2 pfma(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }
template <int P> __device__ __forceinline__ float get(const f32x2 (&v)[P], int i) { return v[i >> 1][i & 1]; }
template <int P> __device__ __forceinline__ void put(f32x2 (&v)[P], int i, float x) { v[i >> 1][i & 1] = x; }

// Chain state of one sample in row pairs: joint angles / rates and the cached
// cos / sin of the absolute angles theta_a = q_1 + ... + q_a.  Pad entries of an
// odd chain stay 0.
template <int N>
struct ChainState {
    static constexpr int P = (N + 1) / 2;
    f32x2 q[P], dq[P], c[P], s[P];

    __device__ __forceinline__ void load(const float* x0) {
#pragma unroll
        for (int p = 0; p < P; ++p) q[p] = dq[p] = c[p] = s[p] = f32x2{0.f, 0.f};
#pragma unroll
        for (int a = 0; a < N; ++a) {
            put(q, a, x0[a]);
            put(dq, a, x0[N + a]);
        }
        angles();
    }
    __device__ __forceinline__ float qa(int a) const { return get(q, a); }
    __device__ __forceinline__ float dqa(int a) const { return get(dq, a); }

    __device__ __forceinline__ void angles() {
        float th = 0.f;
#pragma unroll
        for (int a = 0; a < N; ++a) {
            th += get(q, a);
            float sa, ca;
            sincos_f32(th, &sa, &ca);
            put(s, a, sa);
            put(c, a, ca);
        }
    }

    // One semi-implicit Euler step (oracle/chain_oracle.py chain_forward_dynamics):
    //   D' theta_ddot = tau - bias - g,  tau_a = v'_a - v'_{a+1},  v' = v - b dq,
    //   D'_ab = l_a nu_b cos(th_a - th_b) (a < b; constants I_a + J_a + J_{a+1} on
    //   the diagonal and -J_{a+1} at (a+1, a): the joint armature in absolute
    //   angles), bias_a = sum_b mu_ab sin(th_a - th_b) thdot_b^2,
    //   g_a = g nu_a cos th_a, q_ddot_a = theta_ddot_a - theta_ddot_{a-1},
    //   dq += q_ddot dt, q += dq dt.
    // Packed (v_pk_*) over row pairs; D' is factored in place by a right-looking
    // Cholesky on column-major row pairs; the bias is O(n) through the prefix /
    // suffix sums the separable mu allows:
    //   bias_a = s_a X_a - c_a Y_a,  X_a = l_a C+_a + nu_a C-_a,  Y_a = l_a S+_a + nu_a S-_a,
    //   C+_a = sum_{b>a} nu_b w_b c_b,  C-_a = sum_{b<a} l_b w_b c_b  (S: s_b).
    template <class KC>
    __device__ __forceinline__ void step(const float (&v)[N], const KC& k) {
        f32x2 lc[P], ls[P], vc[P], vs[P], w[P];
        {
            float acc = 0.f;
#pragma unroll
            for (int a = 0; a < N; ++a) {
                acc += get(dq, a);
                put(w, a, acc);
            }
        }
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const f32x2 l = k.l2(p), nu = k.nu2(p);
            w[p] = w[p] * w[p];   // thdot^2
            lc[p] = l * c[p];
            ls[p] = l * s[p];
            vc[p] = nu * c[p];
            vs[p] = nu * s[p];
        }
        // r = tau - g - bias
        f32x2 r[P];
        {
            f32x2 ve[P], vv[P], Cs[P], Ss[P], Cp[P], Sp[P];
#pragma unroll
            for (int a = 0; a < N; ++a) put(vv, a, v[a]);
#pragma unroll
            for (int p = 0; p < P; ++p) ve[p] = pfma(-k.damp2(p), dq[p], vv[p]);
            f32x2 wvc[P], wvs[P], wlc[P], wls[P];
#pragma unroll
            for (int p = 0; p < P; ++p) {
                wvc[p] = w[p] * vc[p];
                wvs[p] = w[p] * vs[p];
                wlc[p] = w[p] * lc[p];
                wls[p] = w[p] * ls[p];
            }
            float cs = 0.f, ss = 0.f, cp = 0.f, sp = 0.f;
#pragma unroll
            for (int a = N - 1; a >= 0; --a) {
                put(Cs, a, cs);
                put(Ss, a, ss);
                cs += get(wvc, a);
                ss += get(wvs, a);
            }
#pragma unroll
            for (int a = 0; a < N; ++a) {
                put(Cp, a, cp);
                put(Sp, a, sp);
                cp += get(wlc, a);
                sp += get(wls, a);
                put(r, a, a + 1 < N ? get(ve, a) - get(ve, a + 1) : get(ve, a));   // tau
            }
            const f32x2 mg = splat(-k.g());
#pragma unroll
            for (int p = 0; p < P; ++p) {
                const f32x2 l = k.l2(p), nu = k.nu2(p);
                const f32x2 X = pfma(l, Cs[p], nu * Cp[p]);
                const f32x2 Y = pfma(l, Ss[p], nu * Sp[p]);
                r[p] = pfma(c[p], Y, pfma(-s[p], X, pfma(mg, vc[p], r[p])));
            }
        }
        // D' lower triangle, column-major row pairs: col[a][p] = rows (2p, 2p+1) of
        // column a; rows < a are don't-cares (kept finite).
        f32x2 col[N][P];
#pragma unroll
        for (int a = 0; a < N; ++a) {
            const f32x2 ca = splat(get(lc, a)), sa = splat(get(ls, a));
#pragma unroll
            for (int p = a / 2; p < P; ++p) {
                if ((a & 1) && p == a / 2) {
                    col[a][p] = splat(k.Dd(a));   // row a - 1: a don't-care
                    continue;
                }
                const f32x2 t = p == (a + 1) / 2 && a + 1 < N ? pfma(sa, vs[p], k.joff2(a)) : sa * vs[p];
                col[a][p] = pfma(ca, vc[p], t);
            }
            if (!(a & 1)) col[a][a / 2].x = k.Dd(a);
        }
        // Cholesky, right-looking: column j scaled by 1 / L_jj, then the trailing
        // columns k > j updated on the rows >= k.
        float inv[N];
#pragma unroll
        for (int j = 0; j < N; ++j) {
            inv[j] = __builtin_amdgcn_rsqf(col[j][j / 2][j & 1]);
            const f32x2 ij = splat(inv[j]);
#pragma unroll
            for (int p = (j + 1) / 2; p < P; ++p) col[j][p] = col[j][p] * ij;
#pragma unroll
            for (int kk = j + 1; kk < N; ++kk) {
                const f32x2 m = splat(-col[j][kk / 2][kk & 1]);
#pragma unroll
                for (int p = kk / 2; p < P; ++p) col[kk][p] = pfma(m, col[j][p], col[kk][p]);
            }
        }
        // L y = r, column-oriented (row j's own pair: only its partner row)
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const float y = r[j / 2][j & 1] * inv[j];
            r[j / 2][j & 1] = y;
            if (!(j & 1) && j + 1 < N) r[j / 2].y = fmaf(-y, col[j][j / 2].y, r[j / 2].y);
#pragma unroll
            for (int p = j / 2 + 1; p < P; ++p) r[p] = pfma(splat(-y), col[j][p], r[p]);
        }
        // L^T x = y, row dots over column i's rows > i (x_i itself is still 0)
        // (full pairs packed; row i's partner and the pad row of an odd chain scalar)
        f32x2 xs[P];
#pragma unroll
        for (int i = N - 1; i >= 0; --i) {
            float e = r[i / 2][i & 1];
            if (!(i & 1) && i + 1 < N) e = fmaf(-col[i][i / 2].y, xs[i / 2].y, e);
            constexpr int PF = N / 2;   // pairs [0, PF) hold two real rows
            const int p0 = i / 2 + 1;
            if (p0 < PF) {
                f32x2 acc = col[i][p0] * xs[p0];
#pragma unroll
                for (int p = p0 + 1; p < PF; ++p) acc = pfma(col[i][p], xs[p], acc);
                e -= acc.x + acc.y;
            }
            if ((N & 1) && i < N - 1 && N / 2 >= p0) e = fmaf(-col[i][N / 2].x, xs[N / 2].x, e);
            xs[i / 2][i & 1] = e * inv[i];
        }
        // q_ddot = diff(theta_ddot); integrate
        f32x2 qdd[P];
#pragma unroll
        for (int a = 0; a < N; ++a) put(qdd, a, a ? get(xs, a) - get(xs, a - 1) : get(xs, 0));
        const f32x2 dt = splat(k.dt());
#pragma unroll
        for (int p = 0; p < P; ++p) {
            dq[p] = pfma(qdd[p], dt, dq[p]);
            q[p] = pfma(dq[p], dt, q[p]);
        }
        angles();
    }

    template <class KC>
    __device__ __forceinline__ void effector(const KC& k, float* px, float* py) const {
        f32x2 x = k.fk2(0) * c[0], y = k.fk2(0) * s[0];
#pragma unroll
        for (int p = 1; p < P; ++p) {
            const f32x2 f = k.fk2(p);
            x = pfma(f, c[p], x);
            y = pfma(f, s[p], y);
        }
        *px = x.x + x.y;
        *py = y.x + y.y;
    }
};
// The chain in fp64 (mppi_chain_config.precision = 1): the same equations as
// ChainState, scalar doubles, sincos from the fp64 library.  Used where the
// weights are spread (lambda comparable to the spread of S): in fp32 the
// end effector sits ~1e-6 m from the fp64 one after 128 steps, so at a near-tie
// of two window slots (slots 6e-5 m apart) the fp32 rollout may take the
// neighbour, and that stage cost moves S by up to ~1e-3 relative — harmless
// while one sample carries the weight, visible in w_eps when tens do.
typedef __attribute__((address_space(4))) const double cdouble;
// 1 / sqrt in fp64 on either side (the device's rsqrt; the host's sqrt and divide)
__host__ __device__ __forceinline__ double rsqrt_hd(double x) {
#ifdef __HIP_DEVICE_COMPILE__
    return rsqrt(x);
#else
    return 1.0 / sqrt(x);
#endif
}

template <int N>
struct ChainStateD {
    double q[N], dq[N], c[N], s[N];

    __host__ __device__ __forceinline__ void load(const double* x0) {
#pragma unroll
        for (int a = 0; a < N; ++a) {
            q[a] = x0[a];
            dq[a] = x0[N + a];
        }
        angles();
    }
    __host__ __device__ __forceinline__ void angles() {
        double th = 0.0;
#pragma unroll
        for (int a = 0; a < N; ++a) {
            th += q[a];
            sincos(th, &s[a], &c[a]);
        }
    }
    // one semi-implicit Euler step (ChainState::step, oracle/chain_oracle.py chain_forward_dynamics);
    // host and device: k is the fp64 constant block (constant memory on the device)
    template <class KP>
    __host__ __device__ __forceinline__ void step(const double (&v)[N], KP k) {
        double w[N], lc[N], ls[N], vc[N], vs[N], r[N];
        double acc = 0.0;
#pragma unroll
        for (int a = 0; a < N; ++a) {
            acc += dq[a];
            w[a] = acc * acc;   // thdot^2
            lc[a] = k[kOffL + a] * c[a];
            ls[a] = k[kOffL + a] * s[a];
            vc[a] = k[kOffNu + a] * c[a];
            vs[a] = k[kOffNu + a] * s[a];
        }
        double ve[N];
#pragma unroll
        for (int a = 0; a < N; ++a) ve[a] = fma(-k[kOffDamp + a], dq[a], v[a]);
        double Cs[N], Ss[N];
        {
            double cs = 0.0, ss = 0.0;
#pragma unroll
            for (int a = N - 1; a >= 0; --a) {
                Cs[a] = cs;
                Ss[a] = ss;
                cs = fma(w[a], vc[a], cs);
                ss = fma(w[a], vs[a], ss);
            }
        }
        {
            double cp = 0.0, sp = 0.0;
            const double g = k[kOffG];
#pragma unroll
            for (int a = 0; a < N; ++a) {
                const double X = fma(k[kOffL + a], Cs[a], k[kOffNu + a] * cp);
                const double Y = fma(k[kOffL + a], Ss[a], k[kOffNu + a] * sp);
                const double tau = a + 1 < N ? ve[a] - ve[a + 1] : ve[a];
                r[a] = fma(c[a], Y, fma(-s[a], X, fma(-g, vc[a], tau)));
                cp = fma(w[a], lc[a], cp);
                sp = fma(w[a], ls[a], sp);
            }
        }
        // D' lower triangle (L[i][a], i >= a), Cholesky in place
        double L[N][N];
#pragma unroll
        for (int a = 0; a < N; ++a) {
            L[a][a] = k[kOffDd + a];
#pragma unroll
            for (int i = a + 1; i < N; ++i) {
                const double t = fma(ls[a], vs[i], lc[a] * vc[i]);
                L[i][a] = i == a + 1 ? t + k[kOffJ + 2 * a + ((a + 1) & 1)] : t;   // -J_{a+1} beside the diagonal
            }
        }
        double inv[N];
#pragma unroll
        for (int j = 0; j < N; ++j) {
            inv[j] = rsqrt_hd(L[j][j]);
#pragma unroll
            for (int i = j + 1; i < N; ++i) L[i][j] *= inv[j];
#pragma unroll
            for (int kk = j + 1; kk < N; ++kk)
#pragma unroll
                for (int i = kk; i < N; ++i) L[i][kk] = fma(-L[i][j], L[kk][j], L[i][kk]);
        }
#pragma unroll
        for (int j = 0; j < N; ++j) {   // L y = r
            r[j] *= inv[j];
#pragma unroll
            for (int i = j + 1; i < N; ++i) r[i] = fma(-L[i][j], r[j], r[i]);
        }
#pragma unroll
        for (int i = N - 1; i >= 0; --i) {   // L^T x = y
            double e = r[i];
#pragma unroll
            for (int kk = i + 1; kk < N; ++kk) e = fma(-L[kk][i], r[kk], e);
            r[i] = e * inv[i];
        }
        const double dt = k[kOffDt];
#pragma unroll
        for (int a = 0; a < N; ++a) {
            const double qdd = a ? r[a] - r[a - 1] : r[0];
            dq[a] = fma(qdd, dt, dq[a]);
            q[a] = fma(dq[a], dt, q[a]);
        }
        angles();
    }
    __device__ __forceinline__ void effector(cdouble* k, double* px, double* py) const {
        double x = 0.0, y = 0.0;
#pragma unroll
        for (int a = 0; a < N; ++a) {
            x = fma(k[kOffFk + a], c[a], x);
            y = fma(k[kOffFk + a], s[a], y);
        }
        *px = x;
        *py = y;
    }
};

// ---- workspace obstacles (mppi_chain_set_obstacles): does a state collide.  Link a is the zero-thickness segment
// from b_{a-1} to b_a = sum_{i <= a} fk_i (cos th_i, sin th_i) (b_{-1} the origin) in the cost's kinematics, the
// one effector() sums; it touches a disc when the centre's distance to it, the projection clipped to [0, fk_a], is
// below r.  The three rollout forms evaluate that on the (cos, sin) their step just produced (no transcendental is
// added), with the arm's seg_hits (mppi_device.h) in fp32 and the same operations in doubles in fp64; each has a
// MASK variant for mppi_chain_debug_obstacle_hits that runs the same operations and keeps every comparison
// (bit 8 j + a: link a against disc j) where the rollout keeps their OR.
//
// One lane per sample: the disc pairs outermost and the links walked inside, so only one pair's centres relative
// to the current link's base are live (4 VGPRs): the base moves along the chain with two v_pk_fma per link, the
// arm's qX, qY repeated.  NP = 0: a scalar branch per pair in use (o.n is wave-uniform), the pairs unrolled; NP < 0:
// the same as a rolled loop; NP > 0: exactly NP pairs without a branch (unused entries are never touched: r2 = -1).
constexpr int kObstNP1 = 0;   // the rollout's NP (DESIGN §3b has the resource report of each variant)
template <int N, int NP, bool MASK, class KC>
__device__ __forceinline__ ObstMask chain_hits(const ObstR& o, const ChainState<N>& x, const KC& k) {
    ObstMask m = 0;
    bool any = false;
    auto pair = [&](int p) {
        const DiscPair d = load_pair(o, p);
        f32x2 qX = d.cX, qY = d.cY;   // the pair's centres relative to link a's base
#pragma unroll
        for (int a = 0; a < N; ++a) {
            const f32x2 cs = {get(x.c, a), get(x.s, a)};
            const float L = k.p[kOffFk + a];
            bool ha, hb;
            seg_hits(qX, qY, cs, L, d.r2, ha, hb);
            if constexpr (MASK) m |= ((ObstMask)ha << (16 * p + a)) | ((ObstMask)hb << (16 * p + 8 + a));
            else any |= ha | hb;
            if (a + 1 < N) {
                qX = pfma(splat(-L), splat(cs.x), qX);
                qY = pfma(splat(-L), splat(cs.y), qY);
            }
        }
    };
    if constexpr (NP < 0) {
#pragma nounroll
        for (int p = 0; 2 * p < o.n; ++p) pair(p);
    } else {
#pragma unroll
        for (int p = 0; p < (NP ? NP : kObstPairs); ++p) {
            if (NP == 0 && 2 * p >= o.n) break;
            pair(p);
        }
    }
    return MASK ? m : (ObstMask)any;
}

// The fp64 rollout: seg_hits' operations in doubles on the fp64 centres and r^2 (rec: cx[8], cy[8], r2[8] in LDS,
// uniform addresses), disc by disc (nd is wave-uniform).
template <int N, bool MASK>
__device__ __forceinline__ ObstMask chain_hits_f64(const double* rec, int nd, const ChainStateD<N>& x, cdouble* k) {
    ObstMask m = 0;
    bool any = false;
    for (int j = 0; j < nd; ++j) {
        double qx = rec[j], qy = rec[MPPI_MAX_OBSTACLES + j];
        const double r2 = rec[2 * MPPI_MAX_OBSTACLES + j];
#pragma unroll
        for (int a = 0; a < N; ++a) {
            const double L = k[kOffFk + a];
            const double s = fma(qy, x.s[a], qx * x.c[a]);
            const double t = s < 0.0 ? 0.0 : (s > L ? L : s);
            const double ox = fma(-t, x.c[a], qx), oy = fma(-t, x.s[a], qy);
            const bool h = fma(oy, oy, ox * ox) < r2;
            if constexpr (MASK) m |= (ObstMask)h << (8 * j + a);
            else any |= h;
            if (a + 1 < N) {
                qx = fma(-L, x.c[a], qx);
                qy = fma(-L, x.s[a], qy);
            }
        }
    }
    return MASK ? m : (ObstMask)any;
}

// What an obstacle-debug instance of the rollout kernel records for the first K samples
// (mppi_chain_debug_obstacle_hits): mask[k][t] and dir[k][t][2 N] = (cos th_a at a, sin th_a at N + a), fp32.
struct ObstDbg {
    ObstMask* mask;
    float* dir;
    int K;
};

// ---- self-collision (mppi_chain_set_self_collision): does a state fold onto itself.  Joint j is b_{j-1} (joint 0
// the origin, joint N the tip), link L the segment from joint L to joint L + 1 along the unit direction
// u_L = (cos th_L, sin th_L), in the cost's kinematics as above.  Links a < b with b >= a + 2 collide when one of
// the four endpoint-to-segment distances is below the clearance d, or when they cross properly.  Per (joint j, link L)
// one test: r = joint j - joint L, the projection s = r . u_L and the perpendicular offset c = u_L x r (a dot and a
// cross product), the projection clipped to [0, fk_L] and the foot point subtracted as seg_hits does it (the squared
// length of r - clip(s) u_L: no term at the magnitude of |r|^2 is cancelled, unlike the expanded |r|^2 - 2 s sigma +
// sigma^2, and the same form as the yardstick's, so directions a rounding off unit length move nothing).  The links
// cross properly when the two offsets of either link's ends from the other's line have strictly opposite signs,
// c c' < 0 for both: the offsets computed beside the distance tests, on the same r.  A joint is tested once per link
// that one of its own links is not adjacent to (self_need): 40 tests and 15 sign pairs at n = 7.  The rollouts keep
// min(distance^2) and min over the pairs of max(c c', c c'), the SMASK variants (mppi_chain_debug_self_hits) the same
// values pair by pair, so both decide on the same numbers; every product-sum is an explicit fma.
struct ChainSelfK {
    double d2d;   // clearance^2 in fp64 (the fp64 rollout)
    double w;     // the cost of one self-colliding state
    float d2;     // clearance^2 rounded once from the fp64 product (the fp32 rollouts)
    int on;       // the host's choice of the SELF kernels; the kernels do not read it
};
using SelfMask = unsigned;
// bit of the pair (a, b), a ascending, then b ascending
constexpr int self_bit(int N, int a, int b) { return a * (N - 2) - a * (a - 1) / 2 + (b - a - 2); }
constexpr bool self_apart(int a, int b) { return a - b >= 2 || b - a >= 2; }
// joint j belongs to links j - 1 and j: tested against link L when one of them is not adjacent to L
constexpr bool self_need(int N, int j, int L) { return (j >= 1 && self_apart(j - 1, L)) || (j < N && self_apart(j, L)); }
// the i-th joint tested against link L (-1 past the last)
constexpr int self_joint(int N, int L, int i) {
    for (int j = 0; j <= N; ++j)
        if (self_need(N, j, L) && i-- == 0) return j;
    return -1;
}
__device__ __forceinline__ float min_raw_f32(float a, float b) {
    float r;
    asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float max_raw_f32(float a, float b) {
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// One lane per sample, fp32: two joints per packed instruction against one link.  Returns the pair mask (SMASK) or
// whether any pair collides.
template <int N, bool SMASK, class KC>
__device__ __forceinline__ SelfMask chain_self_hits(const ChainState<N>& x, const KC& k, float dd) {
    if constexpr (N < 3) return 0;
    float jx[N + 1], jy[N + 1];
    jx[0] = jy[0] = 0.f;
#pragma unroll
    for (int a = 0; a < N; ++a) {
        const float L = k.p[kOffFk + a];
        jx[a + 1] = fmaf(L, get(x.c, a), jx[a]);
        jy[a + 1] = fmaf(L, get(x.s, a), jy[a]);
    }
    float d2[N][N + 1], cr[N][N + 1];   // [link][joint], the tested entries only
    unroll_seq([&](auto L_c) {
        constexpr int L = decltype(L_c)::value;
        const f32x2 ux = splat(get(x.c, L)), uy = splat(get(x.s, L));
        const float len = k.p[kOffFk + L];
        unroll_seq([&](auto i_c) {
            constexpr int i = 2 * decltype(i_c)::value;
            constexpr int ja = self_joint(N, L, i), jn = self_joint(N, L, i + 1);
            if constexpr (ja >= 0) {
                constexpr int jb = jn < 0 ? ja : jn;   // an odd count: the last joint twice
                const f32x2 rx = f32x2{jx[ja], jx[jb]} - splat(jx[L]), ry = f32x2{jy[ja], jy[jb]} - splat(jy[L]);
                const f32x2 s = pfma(ry, uy, rx * ux);
                const f32x2 c = pfma(rx, -uy, ry * ux);
                const f32x2 t = {__builtin_amdgcn_fmed3f(s.x, 0.f, len), __builtin_amdgcn_fmed3f(s.y, 0.f, len)};
                const f32x2 ox = pfma(-t, ux, rx), oy = pfma(-t, uy, ry);
                const f32x2 d = pfma(oy, oy, ox * ox);
                d2[L][ja] = d.x;
                cr[L][ja] = c.x;
                d2[L][jb] = d.y;
                cr[L][jb] = c.y;
            }
        }, std::make_integer_sequence<int, (N + 2) / 2>{});
    }, std::make_integer_sequence<int, N>{});
    SelfMask m = 0;
    float dmin = 0.f, xmin = 0.f;
#pragma unroll
    for (int a = 0; a < N; ++a) {
#pragma unroll
        for (int b = a + 2; b < N; ++b) {
            const float near = min_raw_f32(min_raw_f32(d2[a][b], d2[a][b + 1]), min_raw_f32(d2[b][a], d2[b][a + 1]));
            const float cross = max_raw_f32(cr[a][b] * cr[a][b + 1], cr[b][a] * cr[b][a + 1]);
            if constexpr (SMASK) {
                m |= (SelfMask)(near < dd || cross < 0.f) << self_bit(N, a, b);
            } else {
                const bool first = a == 0 && b == 2;
                dmin = first ? near : min_raw_f32(dmin, near);
                xmin = first ? cross : min_raw_f32(xmin, cross);
            }
        }
    }
    return SMASK ? m : (SelfMask)(dmin < dd || xmin < 0.f);
}

// The fp64 rollout: the same operations in doubles, joint by joint.
template <int N, bool SMASK>
__device__ __forceinline__ SelfMask chain_self_hits_f64(const ChainStateD<N>& x, cdouble* k, double dd) {
    if constexpr (N < 3) return 0;
    double jx[N + 1], jy[N + 1];
    jx[0] = jy[0] = 0.0;
#pragma unroll
    for (int a = 0; a < N; ++a) {
        jx[a + 1] = fma(k[kOffFk + a], x.c[a], jx[a]);
        jy[a + 1] = fma(k[kOffFk + a], x.s[a], jy[a]);
    }
    double d2[N][N + 1], cr[N][N + 1];
#pragma unroll
    for (int L = 0; L < N; ++L) {
        const double len = k[kOffFk + L];
#pragma unroll
        for (int j = 0; j <= N; ++j) {
            if (!self_need(N, j, L)) continue;
            const double rx = jx[j] - jx[L], ry = jy[j] - jy[L];
            const double s = fma(ry, x.s[L], rx * x.c[L]);
            const double c = fma(rx, -x.s[L], ry * x.c[L]);
            const double t = s < 0.0 ? 0.0 : (s > len ? len : s);
            const double ox = fma(-t, x.c[L], rx), oy = fma(-t, x.s[L], ry);
            d2[L][j] = fma(oy, oy, ox * ox);
            cr[L][j] = c;
        }
    }
    SelfMask m = 0;
    double dmin = 0.0, xmin = 0.0;
#pragma unroll
    for (int a = 0; a < N; ++a) {
#pragma unroll
        for (int b = a + 2; b < N; ++b) {
            const double near = min_raw_f64(min_raw_f64(d2[a][b], d2[a][b + 1]), min_raw_f64(d2[b][a], d2[b][a + 1]));
            const double cross = max_raw_f64(cr[a][b] * cr[a][b + 1], cr[b][a] * cr[b][a + 1]);
            if constexpr (SMASK) {
                m |= (SelfMask)(near < dd || cross < 0.0) << self_bit(N, a, b);
            } else {
                const bool first = a == 0 && b == 2;
                dmin = first ? near : min_raw_f64(dmin, near);
                xmin = first ? cross : min_raw_f64(xmin, cross);
            }
        }
    }
    return SMASK ? m : (SelfMask)(dmin < dd || xmin < 0.0);
}

// What a self-collision debug instance of the rollout kernel records for the first K samples
// (mppi_chain_debug_self_hits): mask[k][t] and dir[k][t][2 N] as ObstDbg's.
struct SelfDbg {
    SelfMask* mask;
    float* dir;
    int K;
};

// The fused update's median filter runs over windows of kMedRun consecutive steps per thread: thread
// (q, d) = (tid / N, tid % N) takes the windows of t = kMedRun q .. kMedRun q + 3 of column d.
constexpr int kMedRun = 4;
static_assert(kCMax * ((kMaxT + kMedRun - 1) / kMedRun) <= kCT && 2 * kMaxT <= kCT, "one pass of the workgroup");

// This thread's values of the current nominal (cur->u) for chain_update_block, read at kernel entry so their
// latency is hidden
template <int N>
__device__ __forceinline__ void chain_nominal_prefetch(const ChainStep* s, int T, bool on, double (&u4)[kMedRun]) {
    const int q = threadIdx.x / N, d = threadIdx.x - q * N;
#pragma unroll
    for (int j = 0; j < kMedRun; ++j) {
        const int t = kMedRun * q + j;
        u4[j] = (on && t < T) ? s->u[t][d] : 0.0;
    }
}

// Median filter (control.py:319-327) of the T x N weighted noise, u += w_eps
// (control.py:126), shift (control.py:148-149) and the next launch's fp32
// per-step constants.  u4: chain_nominal_prefetch's values.
//
// The four windows of a thread (t - 5 .. t + 4 for t = t0 .. t0 + 3) share the 7 values t0 - 2 .. t0 + 4:
// those are sorted once (16 comparators), and each window's median — scipy's median of 10, the upper one
// (rank 5, as median10) — is the 6th smallest of that sorted A and the window's 3 other values sorted as B:
// min(A5, max(A4, B0), max(A3, B1), max(A2, B2)) (the k-th smallest of two sorted lists is the least
// max(A_i, B_j) over i + j = k).  80 min / max for the four windows against 4 x 58 with median10, and one
// pass of the workgroup instead of four; the same element is selected, so the same bits.
//
// CLAMP: the kernel was built for torque limits; cl.mode == 2 then clips the updated nominal in fp64 as it is
// written to sm.unew (_g(u[t-1]) over the optimal-trajectory loop, control.py:132-134, clips the whole updated
// u in place), so u_first, the shifted rows, their a_t and the fp32 ua rows all come from clipped values.
template <int N, bool CLAMP>
__device__ __forceinline__ void chain_update_block(ChainStep* nxt, const ChainConst& c, CScratch& sm, const double (&u4)[kMedRun],
                                                   const ChainClampK& cl) {
    const int tid = threadIdx.x, T = c.T;
    const int q = tid / N, d = tid - q * N, t0 = kMedRun * q;
    bool clampu = false;
    double ulo = 0.0, uhi = 0.0;
    if constexpr (CLAMP) {
        clampu = cl.mode == 2;
        ulo = pick<N>(cl.u_lo, d);
        uhi = pick<N>(cl.u_hi, d);
    }
    if (t0 < T) {
        double e[13];   // t0 - 5 .. t0 + 7, reflected at both ends (T >= 5: one reflection)
#pragma unroll
        for (int i = 0; i < 13; ++i) {
            int m = t0 - 5 + i;
            m = m < 0 ? -m - 1 : m;
            m = m >= T ? 2 * T - 1 - m : m;
            m = min(max(m, 0), T - 1);   // only windows past T (never written) read a clamped value
            e[i] = sm.weps[m * N + d];
        }
#define CX(v, i, j) { const double lo = min_raw_f64(v[i], v[j]), hi = max_raw_f64(v[i], v[j]); v[i] = lo; v[j] = hi; }
        double A[7] = {e[3], e[4], e[5], e[6], e[7], e[8], e[9]};
        CX(A, 0, 6) CX(A, 2, 3) CX(A, 4, 5) CX(A, 0, 2) CX(A, 1, 4) CX(A, 3, 6) CX(A, 0, 1) CX(A, 2, 5)
        CX(A, 3, 4) CX(A, 1, 2) CX(A, 4, 6) CX(A, 2, 3) CX(A, 4, 5) CX(A, 1, 2) CX(A, 3, 4) CX(A, 5, 6)
#pragma unroll
        for (int j = 0; j < kMedRun; ++j) {
            // window t0 + j: e[j .. j + 9]; besides A, e[j .. 2] and e[10 .. 9 + j]
            double B[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) B[k] = e[j + k < 3 ? j + k : j + k + 7];
            CX(B, 0, 1) CX(B, 1, 2) CX(B, 0, 1)
            const double med = min_raw_f64(min_raw_f64(A[5], max_raw_f64(A[4], B[0])),
                                           min_raw_f64(max_raw_f64(A[3], B[1]), max_raw_f64(A[2], B[2])));
            double un = u4[j] + med;
            if (clampu) un = clamp_u(un, ulo, uhi);
            if (t0 + j < T) sm.unew[(t0 + j) * N + d] = un;
        }
#undef CX
    }
    __syncthreads();
    if (tid < N) nxt->u_first[tid] = sm.unew[tid];
    if (tid == 0) nxt->eta = sm.eta;
    // row t of the shifted nominal and its a_t = (gamma u_t)^T Sigma^-1: two threads a row, in different waves
    // (h wave-uniform), the first taking d < 4
    const int t = tid % kMaxT;
    if (t < T) {
        const int src = t + 1 < T ? t + 1 : T - 1;
        double u[N];
#pragma unroll
        for (int dd = 0; dd < N; ++dd) u[dd] = sm.unew[src * N + dd];
        auto put = [&](int dd) {   // dd a compile-time constant at every call (sig_inv stays in SGPRs)
            nxt->u[t][dd] = u[dd];
            nxt->ua[t][dd] = (float)u[dd];
            double a = 0.0;
#pragma unroll
            for (int e = 0; e < N; ++e) a += (c.gamma * u[e]) * c.sig_inv[e * N + dd];
            nxt->ua[t][kCMax + dd] = (float)a;
            nxt->a[t][dd] = a;
        };
        if (__builtin_amdgcn_readfirstlane(tid) < kMaxT) {
#pragma unroll
            for (int dd = 0; dd < (N < 4 ? N : 4); ++dd) put(dd);
        } else {
#pragma unroll
            for (int dd = 4; dd < N; ++dd) put(dd);
        }
    }
}

// The horizon loop in fp64 (control.py:95-109 with the chain model): returns S
// of sample k.  Window rows in LDS; the nearest slot by the reference's own
// distance ((x - rx)^2 + (y - ry)^2, first minimum, control.py:205-215).
struct alignas(16) WinRowD {
    double x, y, d1, d2;
};
// CLAMP: every sampled control is clipped in fp64 against the fp64 limits (cl.u_lo, cl.u_hi).
// OBST: every step's new state is tested against the discs (obd: chain_hits_f64's records, nd of them); *hits
// receives the count of colliding states, the final one counted once more.  ODBG: the masks and directions go to od.
// MOVE: obd holds one row of records per step (the discs at c + v (t + 1) dt), and step t reads row t.
// SELF: every step's new state is tested against itself (chain_self_hits_f64, clearance^2 sdd); *shits receives the
// count of self-colliding states, the final one counted once more.  SDBG: the pair masks and directions go to sd.
template <int N, bool CLAMP, bool OBST = false, bool ODBG = false, bool MOVE = false, bool SELF = false, bool SDBG = false>
__device__ __forceinline__ double chain_horizon_f64(const ChainConst& c, const ChainStep* st, cdouble* kd,
                                                    const float* noise, int k, float exf, WinRowD* s_wind,
                                                    int* slots, const ChainClampK& cl, const double* obd = nullptr,
                                                    int nd = 0, int* hits = nullptr, const ObstDbg& od = ObstDbg{},
                                                    double sdd = 0.0, int* shits = nullptr, const SelfDbg& sd = SelfDbg{}) {
    const int tid = threadIdx.x, K = c.K_local, T = c.T;
    if (tid < kSlots) {
        const double* r = st->wind[tid];
        s_wind[tid] = WinRowD{r[0], r[1], r[2], r[3]};
    }
    __syncthreads();
    ChainStateD<N> x;
    x.load(st->x0d);
    cdouble* cu = (cdouble*)&st->u[0][0];
    cdouble* ca = (cdouble*)&st->a[0][0];
    const int W = (int)st->ctr.z;
    double S = 0.0, ex = 0.0, ey = 0.0, e1 = 0.0, e2 = 0.0;
    int nhit = 0;            // colliding states so far (OBST)
    bool hit_last = false;   // the last step's flag: the final state counts once more
    int nself = 0;           // self-colliding states so far (SELF)
    bool self_last = false;
    float nx[N];
#pragma unroll
    for (int d = 0; d < N; ++d) nx[d] = noise[(size_t)k * N + d];
    for (int t = 0; t < T; ++t) {
        double v[N], g = 0.0;
#pragma unroll
        for (int d = 0; d < N; ++d) {
            v[d] = exf != 0.f ? cu[t * kCMax + d] + (double)nx[d] : (double)nx[d];   // control.py:99-101
            if constexpr (CLAMP) v[d] = clamp_u(v[d], cl.u_lo[d], cl.u_hi[d]);         // _g, control.py:104
            g = fma(ca[t * kCMax + d], v[d], g);                                      // control.py:106
        }
        const int tn = t + 1 < T ? t + 1 : t;
#pragma unroll
        for (int d = 0; d < N; ++d) nx[d] = noise[((size_t)tn * K + k) * N + d];
        x.step(v, kd);
        const double* obt = MOVE ? obd + t * kObstRowD : obd;
        if constexpr (ODBG) {
            if (k < od.K) {
                od.mask[(size_t)k * T + t] = chain_hits_f64<N, true>(obt, nd, x, kd);
#pragma unroll
                for (int a = 0; a < N; ++a) {
                    od.dir[((size_t)k * T + t) * 2 * N + a] = (float)x.c[a];
                    od.dir[((size_t)k * T + t) * 2 * N + N + a] = (float)x.s[a];
                }
            }
        } else if constexpr (OBST && !SDBG) {
            hit_last = chain_hits_f64<N, false>(obt, nd, x, kd) != 0;
            nhit += hit_last ? 1 : 0;
        }
        if constexpr (SDBG) {
            if (k < sd.K) {
                sd.mask[(size_t)k * T + t] = chain_self_hits_f64<N, true>(x, kd, sdd);
#pragma unroll
                for (int a = 0; a < N; ++a) {
                    sd.dir[((size_t)k * T + t) * 2 * N + a] = (float)x.c[a];
                    sd.dir[((size_t)k * T + t) * 2 * N + N + a] = (float)x.s[a];
                }
            }
        } else if constexpr (SELF) {
            self_last = chain_self_hits_f64<N, false>(x, kd, sdd) != 0;
            nself += self_last ? 1 : 0;
        }
        double px, py;
        x.effector(kd, &px, &py);
        int best = 0;
        double dmin = INFINITY;
        for (int j = 0; j < W; ++j) {
            const WinRowD r = s_wind[j];
            const double dx = px - r.x, dy = py - r.y;
            const double d = fma(dx, dx, dy * dy);
            if (d < dmin) {
                dmin = d;
                best = j;
            }
        }
        if (slots) slots[(size_t)k * T + t] = best;   // debug instances only (mppi_chain_debug_slots)
        const WinRowD r = s_wind[best];
        ex = px - r.x;
        ey = py - r.y;
        e1 = x.dq[0] - r.d1;
        e2 = x.dq[1] - r.d2;
        S += fma(kd[kOffSw], ex * ex, fma(kd[kOffSw + 1], ey * ey, fma(kd[kOffSw + 2], e1 * e1, kd[kOffSw + 3] * (e2 * e2)))) + g;
    }
    if constexpr (OBST) *hits = nhit + (hit_last ? 1 : 0);
    if constexpr (SELF) *shits = nself + (self_last ? 1 : 0);
    // terminal cost, control.py:109
    return S + fma(kd[kOffTw], ex * ex, fma(kd[kOffTw + 1], ey * ey, fma(kd[kOffTw + 2], e1 * e1, kd[kOffTw + 3] * (e2 * e2))));
}

// ---------------------------------------------------------------- 4 lanes per sample
//
// When K is too small to give every SIMD a wave (config 5 sharded 8 ways: K =
// 16384 per GPU is 256 waves on 1024 SIMDs), the four lanes of a quad share one
// sample: lane p holds the link pair (2p, 2p+1) — exactly one f32x2 of
// ChainState's representation — and the quad exchanges values with DPP
// quad_perm (one instruction per broadcast or scan step).  Per lane and step:
// one pair's sincos, prefix / suffix sums as 4-lane scans, the rows (2p, 2p+1)
// of D' and of its right-looking L D L^T factorization (each pivot and each
// L[kk][j] broadcast from the lane that owns it, so every lane ends with all of
// L), the forward solve on the pairs with each y_j broadcast, the backward solve
// redundantly from those broadcast values, and 8 of the 30 window slots.
// ~0.52x the instructions per lane of one lane per sample, on 4x the lanes.

// v from lane Q of each quad
template <int Q>
__device__ __forceinline__ float qbc(float v) {
    return dpp_f32<Q * 0x55>(v);   // quad_perm [Q, Q, Q, Q]
}
// sum over the lanes p' < p of the quad (m1 = p >= 1 as 1.f / 0.f): the shift with a zero at lane 0 (its
// own x times 0), then two Hillis-Steele steps whose out-of-range reads land on that 0 — no mask after the
// first step, so every DPP move folds into its v_mul / v_add (v_mul_f32_dpp, v_add_f32_dpp)
__device__ __forceinline__ float q_excl_prefix(float x, float m1) {
#pragma clang fp contract(off)   // a contracted e + dpp(e) would re-read x through an unfolded move
    const float e = dpp_f32<0x90>(x) * m1;   // quad_perm [0, 0, 1, 2]: (0, x0, x1, x2)
    const float f = e + dpp_f32<0x90>(e);    // + e_{p-1}: (0, x0, x0 + x1, x1 + x2)
    return f + dpp_f32<0x40>(f);            // quad_perm [0, 0, 0, 1]: + f_{p-2}
}
// sum over the lanes p' > p of the quad (u1 = p <= 2), the mirror image: the zero sits at lane 3
__device__ __forceinline__ float q_excl_suffix(float x, float u1) {
#pragma clang fp contract(off)
    const float e = dpp_f32<0xF9>(x) * u1;   // quad_perm [1, 2, 3, 3]: (x1, x2, x3, 0)
    const float f = e + dpp_f32<0xF9>(e);    // + e_{p+1}
    return f + dpp_f32<0xFE>(f);            // quad_perm [2, 3, 3, 3]: + f_{p+2}
}
__device__ __forceinline__ float q_sum(float x) {
    x += dpp_f32<0xB1>(x);   // quad_perm xor 1
    return x + dpp_f32<0x4E>(x);
}
__device__ __forceinline__ double q_sum_f64(double x) {
    x += dpp_f64<0xB1>(x);
    return x + dpp_f64<0x4E>(x);
}
template <int J>
__device__ __forceinline__ float elem(f32x2 v) {
    return (J & 1) ? v.y : v.x;
}

// The quad stepped in absolute angles (theta_a = q_1 + ... + q_a, kept in
// revolutions, the unit of v_sin_f32 / v_cos_f32) and their rates: the solve
// gives theta_ddot directly; the joint rates the damping needs are one
// difference (theta_dot of link a0 - 1 from the lane below).  Scheduled for one
// wave per SIMD, where every latency is exposed:
// - D' = L D L^T (unit lower L) instead of Cholesky: 1 / d_j is the rcp of the
//   broadcast pivot, each L entry and each y_j one multiply with its broadcast
//   folded in, and the back solve has no scaling (no square roots, no column
//   scalings, 7 fewer multiplies per step);
// - the state's end effector, window search and LDS row read sit inside the
//   factorization (after column kSearchAt), whose pivot chain leaves issue
//   slots idle; the state's stage cost is taken one step later, when its row
//   has long arrived.  State 0 carries no cost (control.py:95-109), so step 0
//   has no search, and the last state's search follows the loop;
// - noise rows through a buffer resource (the row offset in soffset, the
//   lane's in its VGPR: no 64-bit address arithmetic per step), prefetched two
//   steps ahead; the per-step constants from a 2-deep register ring.
// The stage cost's four terms go to two lanes, two apiece (lane 0 has both joint
// rates of the cost in its own pair), so it needs no broadcast.
// CLAMP: the lane's pair of sampled controls is clipped (v_med3_f32) against its pair of fp32 limits, held in
// four VGPRs for the whole horizon (they differ by lane, so neither can be a scalar operand), before the pad
// factor: the pad link of an odd chain stays exactly 0 whatever the limits.
// OBST: lane p tests its own two links against the discs after every step.  The base of its pair is the quad's
// exclusive prefix sum of fk (cos, sin) over the lanes below (the scan the dynamics use, DPP quad_perm); the
// flag is OR-ed across the quad, so every lane of the quad keeps the sample's count and the owner's S carries it.
// The pad link of an odd chain (and the links of lanes past the chain) has length 0 and sits at the end effector:
// its comparisons are masked off, it never hits.  ODBG: the masks and directions go to od.
// MOVE: ob.rec holds one row of records per step (stage_obst_row), and step t reads row t.
// SELF: lane p tests its own two links, packed as the pair it holds, against every joint of the chain; the joints are
// the pair's base (the same prefix scan) and its middle, traded inside the quad by DPP broadcasts.  Each lane gathers
// the "near" bits of its rows (link, joint) and the "ends on opposite sides" bits (link, other link) into one 16-bit
// word, the quad trades the four words, and every lane holds the 8 x 8 bit matrix M[L][m]: links a, a + k cross when
// M[a][a + k] and M[a + k][a] are both set, which for all a at once is (M >> k) & (M >> 8 k) on the diagonal bits.
// Rows of the pad link and of lanes past the chain are masked off.  *shits, SDBG and sd as in chain_horizon_f64.
template <int N, bool CLAMP, bool OBST = false, bool ODBG = false, bool MOVE = false, bool SELF = false, bool SDBG = false>
__device__ __forceinline__ double chain_horizon_q4(const ChainConst& c, const ChainStep* st, const float* dyn,
                                                   const float* noise, int k, float exf, float4* s_ua4,
                                                   float4* s_win, int* slots, unsigned long long* dbg,
                                                   const ChainClampK& cl, const ObstR& ob = ObstR{}, int* hits = nullptr,
                                                   const ObstDbg& od = ObstDbg{}, float sdd = 0.f, int* shits = nullptr,
                                                   const SelfDbg& sd = SelfDbg{}) {
    static_assert(N <= 8, "four link pairs");
    // the column after which the search is placed: after 2 / 3 / 4 / 5 / 6 measured 77.0 / 76.6 / 77.6 / 75.3 /
    // 77.3 us at K = 16384 (one process, profiles/r13/chain_quad_search_at_ab.txt)
    constexpr int kSearchAt = N > 5 ? 5 : N - 1;
    const int tid = threadIdx.x, sub = tid & 3, K = c.K_local, T = c.T;
    if (tid < kSlots) s_win[tid] = st->win[tid];
    for (int i = tid; i < (T + kQPF) * 4; i += kCT) {
        const int t = min(i >> 2, T - 1), p = i & 3;
        const float* r = st->ua[t];
        s_ua4[i] = make_float4(r[2 * p], r[2 * p + 1], r[kCMax + 2 * p], r[kCMax + 2 * p + 1]);
    }
    Search<4, true> sr;
    sr.load(st->key, st->ctr, sub);
    const int a0 = 2 * sub, a1 = 2 * sub + 1;   // this lane's links
    const float m1 = sub >= 1 ? 1.f : 0.f, u1 = sub <= 2 ? 1.f : 0.f;
    // the stage cost's four terms split over two lanes, two apiece: lane 0 the joint-rate terms (its own
    // theta_dot pair gives q_dot_1, q_dot_2), lane 1 the position terms; lanes 2, 3 weigh theirs by 0
    const bool l0 = sub == 0;
    const f32x2 pad = {a0 < N ? 1.f : 0.f, a1 < N ? 1.f : 0.f};
    f32x2 vlo = {0.f, 0.f}, vhi = {0.f, 0.f};   // CLAMP: the limits of links (a0, a1); -inf / +inf past the chain
    if constexpr (CLAMP) {
        const bool b0 = sub & 1, b1 = sub & 2;
        vlo = b1 ? (b0 ? f32x2{cl.v_lo[6], cl.v_lo[7]} : f32x2{cl.v_lo[4], cl.v_lo[5]})
                 : (b0 ? f32x2{cl.v_lo[2], cl.v_lo[3]} : f32x2{cl.v_lo[0], cl.v_lo[1]});
        vhi = b1 ? (b0 ? f32x2{cl.v_hi[6], cl.v_hi[7]} : f32x2{cl.v_hi[4], cl.v_hi[5]})
                 : (b0 ? f32x2{cl.v_hi[2], cl.v_hi[3]} : f32x2{cl.v_hi[0], cl.v_hi[1]});
    }
    const f32x2 l2 = {dyn[kOffL + a0], dyn[kOffL + a1]}, nu2 = {dyn[kOffNu + a0], dyn[kOffNu + a1]};
    const f32x2 damp2 = {dyn[kOffDamp + a0], dyn[kOffDamp + a1]}, fk2 = {dyn[kOffFk + a0], dyn[kOffFk + a1]};
    const float dt = dyn[kOffDt], g = dyn[kOffG];
    constexpr float kRev = 0.15915494309189535f;   // 1 / (2 pi)
    const float dtr = dt * kRev;
    const f32x2 sw2 = l0 ? f32x2{dyn[kOffSw + 2], dyn[kOffSw + 3]}
                         : (sub == 1 ? f32x2{dyn[kOffSw], dyn[kOffSw + 1]} : f32x2{0.f, 0.f});
    const f32x2 tw2 = l0 ? f32x2{dyn[kOffTw + 2], dyn[kOffTw + 3]}
                         : (sub == 1 ? f32x2{dyn[kOffTw], dyn[kOffTw + 1]} : f32x2{0.f, 0.f});
    const float2* const s_win2 = reinterpret_cast<const float2*>(s_win) + (l0 ? 1 : 0);   // (rdq1, rdq2) / (rx, ry)
    // column a of D' on rows (a0, a1): l_a nu_i cos(th_a - th_i) from the broadcast (l c, l s) of link a, plus
    // corr[a]: Dd_a - l_a nu_a on the diagonal (the product gives l_a nu_a there) and -J_{a+1} below it
    f32x2 corr[N];
    {
        const float dc0 = dyn[kOffDd + a0] - l2.x * nu2.x, dc1 = dyn[kOffDd + a1] - l2.y * nu2.y;
        const float j0 = a0 >= 1 ? dyn[kOffJ + 2 * (a0 - 1) + (a0 & 1)] : 0.f;   // -J_{a0} at (a0, a0 - 1)
        const float j1 = dyn[kOffJ + 2 * (a1 - 1) + (a1 & 1)];                    // -J_{a1} at (a1, a1 - 1)
#pragma unroll
        for (int a = 0; a < N; ++a)
            corr[a] = f32x2{a0 == a ? dc0 : (a0 == a + 1 ? j0 : 0.f), a1 == a ? dc1 : (a1 == a + 1 ? j1 : 0.f)};
    }
    // absolute angles (revolutions) and rates of this lane's pair from x0 = (q, q_dot)
    f32x2 TH, THD, C, Sn;
    {
        const f32x2 Q = {a0 < N ? st->x0[a0] : 0.f, a1 < N ? st->x0[a1] : 0.f};
        const f32x2 DQ = {a0 < N ? st->x0[N + a0] : 0.f, a1 < N ? st->x0[N + a1] : 0.f};
        const float tq = Q.x + Q.y, e = q_excl_prefix(tq, m1);
        const float td = DQ.x + DQ.y, ed = q_excl_prefix(td, m1);
        TH = f32x2{e + Q.x, e + tq} * splat(kRev);
        THD = f32x2{ed + DQ.x, ed + td};
    }
    auto angles = [&]() {
        C = f32x2{__builtin_amdgcn_cosf(TH.x), __builtin_amdgcn_cosf(TH.y)};
        Sn = f32x2{__builtin_amdgcn_sinf(TH.x), __builtin_amdgcn_sinf(TH.y)};
    };
    angles();
    // noise of links (a0, a1) at step t: floats (t K + k) N + d; pad links read link N - 1 (masked below);
    // the host keeps T N K 4 below 2^31 for this kernel (mppi_chain_ctx_create)
    const unsigned o0 = (unsigned)(k * N + min(a0, N - 1)) * 4u, o1 = (unsigned)(k * N + min(a1, N - 1)) * 4u;
    const __amdgpu_buffer_rsrc_t nrs = rows_rsrc(noise, T * N * K * 4);
    const int rowb = N * K * 4;
    auto nrow = [&](int t) {
        const int so = min(t, T - 1) * rowb;
        return f32x2{__builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(nrs, (int)o0, so, 0)),
                     __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(nrs, (int)o1, so, 0))};
    };
    f32x2 ring[kQPF];
#pragma unroll
    for (int j = 0; j < kQPF; ++j) ring[j] = nrow(j);
    __syncthreads();
    float4 uar[kQPF];
#pragma unroll
    for (int j = 0; j < kQPF; ++j) uar[j] = s_ua4[j * 4 + sub];

    int nhit = 0;            // colliding states so far (OBST)
    bool hit_last = false;   // the last step's flag: the final state counts once more
    // the new state (C, Sn) of step t against the discs in use (a scalar branch per pair: ob.n is wave-uniform)
    auto quad_hits = [&](int t) {
        const bool live0 = a0 < N, live1 = a1 < N;   // pad links and lanes past the chain never hit
        const f32x2 fx = fk2 * C, fy = fk2 * Sn;
        const float bx = q_excl_prefix(fx.x + fx.y, m1), by = q_excl_prefix(fy.x + fy.y, m1);   // the pair's base
        bool any = false;
        ObstMask m = 0;
#pragma unroll
        for (int p = 0; p < kObstPairs; ++p) {
            if (2 * p >= ob.n) break;
            const DiscPair d = load_pair(MOVE ? ObstR{ob.rec + t * kObstRow, ob.n} : ob, p);
            f32x2 qX = d.cX - splat(bx), qY = d.cY - splat(by);
            bool h0a, h0b, h1a, h1b;
            seg_hits(qX, qY, f32x2{C.x, Sn.x}, fk2.x, d.r2, h0a, h0b);
            qX = pfma(splat(-fk2.x), splat(C.x), qX);
            qY = pfma(splat(-fk2.x), splat(Sn.x), qY);
            seg_hits(qX, qY, f32x2{C.y, Sn.y}, fk2.y, d.r2, h1a, h1b);
            h0a &= live0;
            h0b &= live0;
            h1a &= live1;
            h1b &= live1;
            if constexpr (ODBG)
                m |= ((ObstMask)h0a << (16 * p + a0)) | ((ObstMask)h0b << (16 * p + 8 + a0)) |
                     ((ObstMask)h1a << (16 * p + a1)) | ((ObstMask)h1b << (16 * p + 8 + a1));
            else any |= (h0a | h0b) | (h1a | h1b);
        }
        if constexpr (ODBG) {
            if (k < od.K) {
                // (the mask buffer arrives zeroed; each lane adds the bits of its own links)
                if (m) atomicOr(&od.mask[(size_t)k * T + t], m);
                float* dr = od.dir + ((size_t)k * T + t) * 2 * N;
                if (live0) {
                    dr[a0] = C.x;
                    dr[N + a0] = Sn.x;
                }
                if (live1) {
                    dr[a1] = C.y;
                    dr[N + a1] = Sn.y;
                }
            }
        } else {
            hit_last = q_sum(any ? 1.f : 0.f) != 0.f;
            nhit += hit_last ? 1 : 0;
        }
    };
    static_assert(!SELF || (N >= 3 && N <= 7), "the 8 x 8 bit matrix: links 0 .. 6, joints 0 .. 7");
    int nself = 0;            // self-colliding states so far (SELF)
    bool self_last = false;
    // which of this lane's tests count: bit j (link a0) / 8 + j (link a1): joint j is tested against the link
    // (self_need); bit m / 8 + m of rows: link m is a partner of the link (exists and is not adjacent)
    unsigned needj = 0, rows = 0;
    if constexpr (SELF) {
#pragma unroll
        for (int l = 0; l < 2; ++l) {
            const int L = a0 + l;
#pragma unroll
            for (int j = 0; j <= N; ++j) needj |= (unsigned)(L < N && self_need(N, j, L)) << (8 * l + j);
#pragma unroll
            for (int m = 0; m < N; ++m) rows |= (unsigned)(L < N && self_apart(m, L)) << (8 * l + m);
        }
    }
    auto quad_self = [&](int t) {
        const float ex = fmaf(fk2.y, C.y, fk2.x * C.x), ey = fmaf(fk2.y, Sn.y, fk2.x * Sn.x);   // the pair's extent
        const float bx = q_excl_prefix(ex, m1), by = q_excl_prefix(ey, m1);                     // joint a0
        const float mx = fmaf(fk2.x, C.x, bx), my = fmaf(fk2.x, Sn.x, by);                      // joint a1
        const f32x2 BX = {bx, mx}, BY = {by, my};
        unsigned nb = 0, sb = 0;
        f32x2 cprev = {0.f, 0.f};
        unroll_seq([&](auto j_c) {
            constexpr int j = decltype(j_c)::value;
            const float Jx = (j & 1) ? qbc<j / 2>(mx) : qbc<j / 2>(bx);
            const float Jy = (j & 1) ? qbc<j / 2>(my) : qbc<j / 2>(by);
            const f32x2 rx = splat(Jx) - BX, ry = splat(Jy) - BY;
            const f32x2 s = pfma(ry, Sn, rx * C);
            const f32x2 cc = pfma(rx, -Sn, ry * C);
            const f32x2 tc = {__builtin_amdgcn_fmed3f(s.x, 0.f, fk2.x), __builtin_amdgcn_fmed3f(s.y, 0.f, fk2.y)};
            const f32x2 ox = pfma(-tc, C, rx), oy = pfma(-tc, Sn, ry);
            const f32x2 d = pfma(oy, oy, ox * ox);
            nb |= (d.x < sdd ? 1u << j : 0u) | (d.y < sdd ? 1u << (8 + j) : 0u);
            if constexpr (j > 0) {   // the ends of link j - 1
                const f32x2 p = cprev * cc;
                sb |= (p.x < 0.f ? 1u << (j - 1) : 0u) | (p.y < 0.f ? 1u << (8 + j - 1) : 0u);
            }
            cprev = cc;
        }, std::make_integer_sequence<int, N + 1>{});
        nb &= needj;
        sb &= rows;
        auto trade = [&](unsigned w) {   // the four lanes' words: row L at bits 8 L .. 8 L + 7
            const unsigned w0 = (unsigned)__builtin_amdgcn_mov_dpp((int)w, 0x00, 0xF, 0xF, kDppBC);
            const unsigned w1 = (unsigned)__builtin_amdgcn_mov_dpp((int)w, 0x55, 0xF, 0xF, kDppBC);
            const unsigned w2 = (unsigned)__builtin_amdgcn_mov_dpp((int)w, 0xAA, 0xF, 0xF, kDppBC);
            const unsigned w3 = (unsigned)__builtin_amdgcn_mov_dpp((int)w, 0xFF, 0xF, 0xF, kDppBC);
            return ((unsigned long long)(w2 | (w3 << 16)) << 32) | (w0 | (w1 << 16));
        };
        // bit 7 of a lane's first row (no link 7): one of its near bits is set
        const unsigned long long Mn = trade(sb | (nb ? 0x80u : 0u));
        const unsigned long long M = Mn & 0x7F7F7F7F7F7F7F7Full;
        if constexpr (SDBG) {
            const unsigned long long NB = trade(nb), Q = NB | (NB >> 1);   // Q[L][m]: joint m or m + 1 is near link L
            SelfMask mk = 0;
#pragma unroll
            for (int a = 0; a < N; ++a)
#pragma unroll
                for (int b = a + 2; b < N; ++b) {
                    const unsigned long long h = (Q >> (8 * a + b)) | (Q >> (8 * b + a)) | ((M >> (8 * a + b)) & (M >> (8 * b + a)));
                    mk |= (SelfMask)(h & 1ull) << self_bit(N, a, b);
                }
            if (k < sd.K) {
                if (sub == 0) sd.mask[(size_t)k * T + t] = mk;
                float* dr = sd.dir + ((size_t)k * T + t) * 2 * N;
                if (a0 < N) {
                    dr[a0] = C.x;
                    dr[N + a0] = Sn.x;
                }
                if (a1 < N) {
                    dr[a1] = C.y;
                    dr[N + a1] = Sn.y;
                }
            }
        } else {
            unsigned long long X = 0;
#pragma unroll
            for (int kk = 2; kk < N; ++kk) X |= (M >> kk) & (M >> (8 * kk));
            self_last = ((X & 0x8040201008040201ull) | (Mn & 0x8080808080808080ull)) != 0ull;
            nself += self_last ? 1 : 0;
        }
    };
    double S = 0.0;
    f32x2 S2 = {0.f, 0.f};   // this lane's two stage-cost terms
    f32x2 G2 = {0.f, 0.f};   // this lane's (gamma u^T Sigma^-1) v terms
    // the pending stage cost (the previous step's state): this lane's two values and their window-row entries,
    // all zero until the first search, so the cost taken in steps 0 and 1 is exactly 0; (nAB, nrw) this step's
    f32x2 pAB = {0.f, 0.f}, prw = {0.f, 0.f}, nAB = {0.f, 0.f}, nrw = {0.f, 0.f};
    auto search_state = [&](int t, float anchor) {   // the current state (t): end effector, nearest slot, row
        const f32x2 fx = fk2 * C, fy = fk2 * Sn;
        float px = q_sum(fx.x + fx.y), py = q_sum(fy.x + fy.y);
        asm volatile("" : "+v"(px), "+v"(py) : "v"(anchor));   // no earlier than the anchor (and opaque: the
                                                                 // SLP vectoriser would pair the two sums)
        // lane 0: q_dot_1 = theta_dot_1, q_dot_2 = theta_dot_2 - theta_dot_1; the others: the position
        nAB = l0 ? f32x2{THD.x, THD.y - THD.x} : f32x2{px, py};
        const unsigned j = sr.nearest(px, py);
        if (slots && sub == 0) slots[(size_t)k * T + t - 1] = (int)j;   // debug instances only
        const float2 r2 = s_win2[2 * j];
        nrw = f32x2{r2.x, r2.y};
    };
    auto step = [&](int t, auto slot_c, auto srch_c) {
        constexpr int slot = decltype(slot_c)::value;
        constexpr bool srch = decltype(srch_c)::value;
        // the slot's values are taken here (volatile asm keeps its place against the previous step's
        // PIN_LOADS): left free, the scheduler hoists their uses into the previous step, where waiting for
        // them means waiting for every load in flight (as rollout_kernel's dstep)
        f32x2 nz = ring[slot];
        f32x4 ua = {uar[slot].x, uar[slot].y, uar[slot].z, uar[slot].w};
        asm volatile("" : "+v"(nz), "+v"(ua));
        f32x2 v = __builtin_elementwise_fma(splat(exf), f32x2{ua.x, ua.y}, nz);              // control.py:99-101
        if constexpr (CLAMP) v = f32x2{clamp_v(v.x, vlo.x, vhi.x), clamp_v(v.y, vlo.y, vhi.y)};  // _g, control.py:104
        v = v * pad;
        G2 = __builtin_elementwise_fma(f32x2{ua.z, ua.w}, v, G2);                          // control.py:106
        ring[slot] = nrow(t + kQPF);
        uar[slot] = s_ua4[(t + kQPF) * 4 + sub];
        PIN_LOADS();
        // ---- dynamics in absolute angles: bias, D' rows (a0, a1), L D L^T with the forward solve
        const f32x2 w = THD * THD;   // thdot^2
        const f32x2 lc = l2 * C, ls = l2 * Sn, vc = nu2 * C, vs = nu2 * Sn;
        const f32x2 wvc = w * vc, wvs = w * vs, wlc = w * lc, wls = w * ls;
        const float sC = q_excl_suffix(wvc.x + wvc.y, u1), sS = q_excl_suffix(wvs.x + wvs.y, u1);
        const float pC = q_excl_prefix(wlc.x + wlc.y, m1), pS = q_excl_prefix(wls.x + wls.y, m1);
        const f32x2 Cs = {wvc.y + sC, sC}, Ss = {wvs.y + sS, sS};
        const f32x2 Cp = {pC, wlc.x + pC}, Sp = {pS, wls.x + pS};
        const f32x2 X = __builtin_elementwise_fma(l2, Cs, nu2 * Cp);
        const f32x2 Y = __builtin_elementwise_fma(l2, Ss, nu2 * Sp);
        const float thd_prev = dpp_f32<0x90>(THD.y) * m1;                // theta_dot of link a0 - 1 (0 at the base)
        const f32x2 qd = THD - f32x2{thd_prev, THD.x};                   // joint rates q_dot of (a0, a1)
        const f32x2 ve = __builtin_elementwise_fma(-damp2, qd, v);
        const float ve_next = dpp_f32<0xF9>(ve.x) * u1;                 // link a1 + 1 (0 past the quad)
        f32x2 r = {ve.x - ve.y, ve.y - ve_next};                         // tau
        r = __builtin_elementwise_fma(C, Y, __builtin_elementwise_fma(-Sn, X, __builtin_elementwise_fma(splat(-g), vc, r)));
        f32x2 col[N];
        unroll_seq([&](auto a_c) {
            constexpr int a = decltype(a_c)::value;
            const float la = qbc<a / 2>(elem<a>(lc)), sa = qbc<a / 2>(elem<a>(ls));
            col[a] = __builtin_elementwise_fma(splat(la), vc, __builtin_elementwise_fma(splat(sa), vs, corr[a]));
        }, std::make_integer_sequence<int, N>{});
        // right-looking on the raw columns, every factor kept negated: -1 / d_j is the rcp of the negated
        // broadcast pivot (a source modifier of the DPP form), -L[kk][j] and -y_j are the broadcast entries
        // times it, so no product needs a negation that would take it out of the VOP2 encoding the broadcast
        // folds into; every lane keeps every -L[kk][j] and -y_j (y = D^-1 L^-1 r: the back solve needs no
        // scaling)
        float Ln[N][N], yn[N];
        unroll_seq([&](auto j_c) {
            constexpr int j = decltype(j_c)::value;
            const float nrd = __builtin_amdgcn_rcpf(-qbc<j / 2>(elem<j>(col[j])));
            yn[j] = qbc<j / 2>(elem<j>(r)) * nrd;
            r = __builtin_elementwise_fma(splat(yn[j]), col[j], r);
            unroll_seq([&](auto k_c) {
                constexpr int kk = decltype(k_c)::value;
                if constexpr (kk > j) {
                    Ln[kk][j] = qbc<kk / 2>(elem<kk>(col[j])) * nrd;
                    // the last row's products, left free, are paired by the SLP vectoriser into a v_pk_mul_f32,
                    // which has no DPP form: their broadcasts come back as separate moves (7 per step)
                    if constexpr (kk == N - 1) asm volatile("" : "+v"(Ln[kk][j]));
                    col[kk] = __builtin_elementwise_fma(splat(Ln[kk][j]), col[j], col[kk]);
                }
            }, std::make_integer_sequence<int, N>{});
            if constexpr (srch && j == kSearchAt) search_state(t, nrd);
        }, std::make_integer_sequence<int, N>{});
        float x[N];   // L^T x = y: theta_ddot, redundantly in every lane; the oldest x first
#pragma unroll
        for (int i = N - 1; i >= 0; --i) {
            float e = -yn[i];
#pragma unroll
            for (int kk = N - 1; kk > i; --kk) e = fmaf(Ln[kk][i], x[kk], e);
            x[i] = e;
        }
        auto xs = [&](int i) { return i < N ? x[i] : 0.f; };
        const bool b0 = sub & 1, b1 = sub & 2;
        const float xa = b1 ? (b0 ? xs(6) : xs(4)) : (b0 ? xs(2) : xs(0));
        const float xb = b1 ? (b0 ? xs(7) : xs(5)) : (b0 ? xs(3) : xs(1));
        THD = __builtin_elementwise_fma(f32x2{xa, xb}, splat(dt), THD);  // semi-implicit Euler (chain_oracle.py)
        TH = __builtin_elementwise_fma(THD, splat(dtr), TH);
        angles();
        if constexpr (OBST && !SDBG) quad_hits(t);
        if constexpr (SELF) quad_self(t);
        {   // the pending (previous state's) stage cost, control.py:174-185; the row is taken only now (the
            // asm needs TH, this step's last dynamics result)
            f32x2 rw = prw;
            asm volatile("" : "+v"(rw) : "v"(TH));
            const f32x2 e = pAB - rw;
            S2 = __builtin_elementwise_fma(sw2, e * e, S2);
        }
        if constexpr (srch) {
            pAB = nAB;
            prw = nrw;
        }
        if constexpr (slot == kQPF - 1) {
            S += (double)((S2.x + S2.y) + (G2.x + G2.y));
            S2 = f32x2{0.f, 0.f};
            G2 = f32x2{0.f, 0.f};
        }
    };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    using I3 = std::integral_constant<int, 3>;
    using Y = std::true_type;
    STAMP(12, NOW());   // stamp builds: the prologue's end, then the first steps and the horizon's middle
    step(0, I0{}, std::false_type{});
    int t = 1;
    if constexpr (kQPF == 2) {
        for (; t + 2 <= T; t += 2) {
            step(t, I1{}, Y{});
            step(t + 1, I0{}, Y{});
        }
        if (t < T) step(t, I1{}, Y{});
    } else {
        static_assert(kQPF == 4, "a 2- or 4-deep ring");
        for (; t + 4 <= T; t += 4) {   // slots 1, 2, 3, 0
            step(t, I1{}, Y{});
            step(t + 1, I2{}, Y{});
            step(t + 2, I3{}, Y{});
            step(t + 3, I0{}, Y{});
#ifdef MPPI_STAMPS
            if (t == 1) STAMP(13, NOW());
            if (t + 4 == T / 2 + 1) STAMP(14, NOW());
#endif
        }
        if (t < T) step(t, I1{}, Y{});   // remainder: slots 1, 2, 3 in order
        if (t + 1 < T) step(t + 1, I2{}, Y{});
        if (t + 2 < T) step(t + 2, I3{}, Y{});
    }
    {   // state T - 1's pending cost, then the last state's search: its stage and terminal cost
        // (control.py:106-109) on the same state
        const f32x2 e = pAB - prw;
        S2 = __builtin_elementwise_fma(sw2, e * e, S2);
    }
    search_state(T, TH.x);
    const f32x2 e = nAB - nrw, ee = e * e;
    S2 = __builtin_elementwise_fma(sw2, ee, S2);
    S += (double)((S2.x + S2.y) + (G2.x + G2.y));
    const f32x2 te = tw2 * ee;
    S += (double)(te.x + te.y);
    if constexpr (OBST) *hits = nhit + (hit_last ? 1 : 0);
    if constexpr (SELF) *shits = nself + (self_last ? 1 : 0);
    return q_sum_f64(S);
}

// POLL / counter: the hand-off form of the partial rows (handoff_merge in mppi_merge.h, shared with rollout_kernel).
// SLOTS (debug instances, mppi_chain_debug_slots): dbg receives the window slot
// each sample picked at each step, int32 [k][t].
// CLAMP: the sampled controls are clipped to the torque limits cl (clamp_mode != 0) and, with cl.mode == 2, so
// is the fused update's nominal; the CLAMP = false instantiations never read cl.
// OBST: every step's new state, and the final state once more, is tested against the discs of ob (staged in LDS by
// one thread); the count of colliding states times ob.w is added to S once, in fp64, after the terminal cost.
// Built with CLAMP only: without torque limits cl holds -+inf, the median and the fp64 compares return v untouched
// and cl.mode = 0 clips no nominal.  The OBST = false instantiations never read ob.
// ODBG (mppi_chain_debug_obstacle_hits; CLAMP and OBST): the same prologue and horizon, which record the masks and
// directions of the first `flags` samples instead of counting (gslab: the masks, slab: the directions), and
// nothing after the horizon.
// SELF (mppi_chain_set_self_collision; built on the CLAMP + OBST kernels only, for N >= 3): every step's new state,
// and the final state once more, is tested against itself; the count of self-colliding states times sk.w is added to
// S after the discs' product, as one fp64 multiply and add.  Without discs ob.n = 0 and the scalar branch per disc
// pair skips the disc test.  sk is the last argument, behind ob; the SELF = false instantiations never read it.
// SDBG (mppi_chain_debug_self_hits): the same prologue and horizon, which record the pair masks and directions of
// the first `flags` samples (gslab: the masks, slab: the directions) and nothing after the horizon.
template <int N, bool POLL, bool F64, int LPS, bool SLOTS = false, bool CLAMP = false, bool OBST = false,
          bool ODBG = false, bool MOVE = false, bool SELF = false, bool SDBG = false>
__global__ __launch_bounds__(kCT) __attribute__((amdgpu_waves_per_eu(2, 2))) void chain_rollout_kernel(
    const ChainConst c, const ChainStep* __restrict__ st, const float* __restrict__ dyn,
    const float* __restrict__ noise, double* __restrict__ S_out, double* __restrict__ slab, double* __restrict__ gslab,
    unsigned* __restrict__ counters, double* __restrict__ partial_out, double* __restrict__ w_eps_out,
    ChainStep* __restrict__ nxt, unsigned flags, const XDesc xd, unsigned* __restrict__ epoch, unsigned* __restrict__ tmo,
    unsigned long long* __restrict__ runmin, unsigned long long* __restrict__ dbg, const ChainClampK cl,
    const ChainObstK ob, const ChainSelfK sk) {
    static_assert(N <= kCMax && N >= 2, "links");
    static_assert(!(SLOTS && CLAMP), "the slot-recording instances are unclamped");
    static_assert(CLAMP || !OBST, "the OBST kernels are built with CLAMP only");
    static_assert(OBST || !ODBG, "the obstacle-debug instances are OBST kernels");
    static_assert(OBST || !MOVE, "moving discs are discs");
    static_assert(!SELF || (OBST && N >= 3), "the SELF kernels are CLAMP + OBST kernels of chains with a non-adjacent pair");
    static_assert(SELF || !SDBG, "the self-collision debug instances are SELF kernels");
    static_assert(!(ODBG && SDBG), "one recording at a time");
    static_assert(kMaxT <= kCT, "thread t stages step t's disc records");
    __shared__ float4 s_win[kSlots];
    __shared__ KeyPair s_keys[kKeyPairs];
    __shared__ WinRowD s_wind[F64 ? kSlots : 1];
    __shared__ float4 s_ua4[LPS == 4 ? (kMaxT + kQPF) * 4 : 1];
    __shared__ float s_vhi[CLAMP && !F64 && LPS == 1 ? kCMax : 1];   // the upper fp32 limits (one lane per sample)
    __shared__ double s_redd[kCT / 64];
    __shared__ int s_cnt[kCT / 64];
    __shared__ int s_k[kCT];
    __shared__ double s_e[kCT];
    __shared__ unsigned s_flag, s_parity;
    __shared__ double s_run;
    __shared__ CScratch sm;

    static_assert(LPS == 1 || (LPS == 4 && !F64), "lanes per sample: 1, or 4 for the fp32 rollout");
    constexpr int NS = kCT / LPS;   // samples per workgroup
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k_raw = (blockIdx.x * kCT + tid) / LPS;
    if (c.fair) draw_cu_ticket(counters + c.cu_off, &s_parity);
    const bool valid = k_raw < c.K_local;
    const bool owner = valid && (tid & (LPS - 1)) == 0;   // the lane that stands for its sample
    const int k = valid ? k_raw : c.K_local - 1;
    const float exf = (c.k_offset + k) < c.k_exploit ? 1.f : 0.f;  // control.py:98-101
    const int K = c.K_local, T = c.T;
    int* const slots = SLOTS ? reinterpret_cast<int*>(dbg) : nullptr;

    STAMP(0, NOW());
#ifdef MPPI_STAMPS
    STAMP(8, (unsigned long long)__builtin_amdgcn_s_getreg(0xF804));   // HW_ID
    STAMP(9, (unsigned long long)__builtin_amdgcn_s_getreg(0xF814));   // XCC_ID
#endif
    // poll tags are never 0 (fresh memory)
    unsigned tag_v = POLL ? __hip_atomic_load(epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u : 0u;
    if (POLL && tag_v == 0u) tag_v = 1u;
    // the one-lane-per-sample fp32 CLAMP kernel reads the nominal only when it updates it: at n = 7 it has no
    // registers to hold the prefetch across the horizon (the eight went to scratch)
    constexpr bool kLateNominal = CLAMP && !F64 && LPS == 1;
    double u_cur[kMedRun];
    if constexpr (!kLateNominal) chain_nominal_prefetch<N>(st, T, flags & MPPI_FLAG_FUSED_UPDATE, u_cur);
    double S = 0.0;
    // OBST: the discs in LDS, published by the horizon's first barrier
    ObstR od{};
    const double* obd = nullptr;
    int nd = 0;
    if constexpr (OBST) {
        nd = __builtin_amdgcn_readfirstlane(ob.n);
        if constexpr (MOVE) {
            // a row of records per step, the discs where that step's new state meets them: thread t writes step t's,
            // every centre one explicit fma of the velocity, the time (t + 1) dt and the centre at x0 (in the
            // rollout's precision; fp32: stage_obst_row, mppi_device.h, with the time rounded once from fp64)
            if constexpr (F64) {
                __shared__ double s_obd[kMaxT * kObstRowD];
                if (tid < T) {
                    const double tau = (double)(tid + 1) * ob.dt;
                    double* row = s_obd + tid * kObstRowD;
#pragma unroll
                    for (int j = 0; j < MPPI_MAX_OBSTACLES; ++j) {
                        row[j] = fma(ob.vxd[j], tau, ob.cxd[j]);
                        row[MPPI_MAX_OBSTACLES + j] = fma(ob.vyd[j], tau, ob.cyd[j]);
                        row[2 * MPPI_MAX_OBSTACLES + j] = ob.r2d[j];
                    }
                }
                obd = s_obd;
            } else {
                __shared__ float4 s_obst[kMaxT * kObstRow];
                if (tid < T) stage_obst_row(s_obst + tid * kObstRow, ob, tid);
                od = ObstR{s_obst, nd};
            }
        } else if constexpr (F64) {
            __shared__ double s_obd[kObstRowD];
            if (tid == 0) {
#pragma unroll
                for (int j = 0; j < MPPI_MAX_OBSTACLES; ++j) {
                    s_obd[j] = ob.cxd[j];
                    s_obd[MPPI_MAX_OBSTACLES + j] = ob.cyd[j];
                    s_obd[2 * MPPI_MAX_OBSTACLES + j] = ob.r2d[j];
                }
            }
            obd = s_obd;
        } else {
            __shared__ float4 s_obst[2 * kObstPairs];
            if (tid == 0) stage_obst(s_obst, ob);
            od = ObstR{s_obst, nd};
        }
    }
    ObstDbg odbg{};
    if constexpr (ODBG) odbg = ObstDbg{reinterpret_cast<ObstMask*>(gslab), reinterpret_cast<float*>(slab), valid ? (int)flags : 0};
    int hits = 0;   // colliding states of this sample, the final one counted twice (OBST)
    SelfDbg sdbg{};
    if constexpr (SDBG) sdbg = SelfDbg{reinterpret_cast<SelfMask*>(gslab), reinterpret_cast<float*>(slab), valid ? (int)flags : 0};
    int shits = 0;   // self-colliding states of this sample, the final one counted twice (SELF)
    if constexpr (F64) {
        S = chain_horizon_f64<N, CLAMP, OBST, ODBG, MOVE, SELF, SDBG>(c, st, (cdouble*)(dyn + kDynF64Off), noise, k, exf, s_wind,
                                                                      slots, cl, obd, nd, &hits, odbg, sk.d2d, &shits, sdbg);
    } else if constexpr (LPS == 4) {
        S = chain_horizon_q4<N, CLAMP, OBST, ODBG, MOVE, SELF, SDBG>(c, st, dyn, noise, k, exf, s_ua4, s_win, slots, dbg, cl, od,
                                                                     &hits, odbg, sk.d2, &shits, sdbg);
    } else {
    bool hit_last = false;
    bool self_last = false;
    if (tid < kSlots) s_win[tid] = st->win[tid];
    if constexpr (CLAMP) {
        if (tid < kCMax) s_vhi[tid] = dyn[kDynLimOff + kCMax + tid];
    }
    // window keys in LDS (broadcast reads): the 90 key registers would cost the
    // chain kernel its second wave per SIMD; precise keys: the config-5 start
    // pose sits on a waypoint
    SearchLDS<true>::fill(s_keys, st->key, tid);
    SearchLDS<true> sr{s_keys, st->ctr.x, st->ctr.y};
    ChainState<N> x;
    x.load(st->x0);
    // noise (t, d) of sample k: noise[(t K + k) N + d] (a sample's N values of a step contiguous); prefetches
    // past the last step read step T - 1 again (never used)
    // (uniform step base + a 32-bit lane byte offset: the saddr form of global_load)
    const unsigned kb = (unsigned)k * (unsigned)N * 4u;
    auto nrow = [&](int t, int d) {
        const char* row = (const char*)(noise + (size_t)min(t, T - 1) * K * N + d);
        return *(const float*)(row + kb);
    };
    cfloat* cua = (cfloat*)(&st->ua[0][0]);
    float ring[kCPF][N];
    float uring[kCPU][2 * N];
#pragma unroll
    for (int j = 0; j < kCPF; ++j)
#pragma unroll
        for (int d = 0; d < N; ++d) ring[j][d] = nrow(j, d);
#pragma unroll
    for (int j = 0; j < kCPU; ++j)
#pragma unroll
        for (int d = 0; d < 2 * N; ++d) uring[j][d] = cua[j * 2 * kCMax + (d < N ? d : kCMax + d - N)];
    __syncthreads();

    const DynMem kd{(cfloat*)dyn};
    // Horizon loop (control.py:95-109 with the chain model), S in fp64.
    float S4 = 0.f;
    float ex = 0.f, ey = 0.f, e1 = 0.f, e2 = 0.f;
    // (always_inline: with the OBST test in it the body passes the inliner's threshold, and a called step keeps its
    // captures in scratch; the other instantiations were inlined already)
    auto step = [&](int t, auto i_c) __attribute__((always_inline)) {
        constexpr int i = decltype(i_c)::value;
        float v[N];
        float g = 0.f;
#pragma unroll
        for (int d = 0; d < N; ++d) {
            v[d] = fmaf(exf, uring[i % kCPU][d], ring[i % kCPF][d]);   // u_t + eps or eps
            // _g, control.py:104: v_med3_f32 takes one scalar operand, the lower limit (read like the other
            // constants); the upper one comes from LDS into a VGPR that lives for this instruction only
            if constexpr (CLAMP) v[d] = clamp_v(v[d], kd.p[kDynLimOff + d], s_vhi[d]);
            g = fmaf(uring[i % kCPU][N + d], v[d], g);                 // (gamma u_t^T Sigma^-1) v, control.py:106
        }
#pragma unroll
        for (int d = 0; d < N; ++d) ring[i % kCPF][d] = nrow(t + kCPF, d);
#pragma unroll
        for (int d = 0; d < 2 * N; ++d)
            uring[i % kCPU][d] = cua[(t + kCPU) * 2 * kCMax + (d < N ? d : kCMax + d - N)];
        PIN_LOADS();
        x.step(v, kd);
        const ObstR odt = MOVE ? ObstR{od.rec + t * kObstRow, od.n} : od;   // MOVE: step t's row of records
        if constexpr (ODBG) {
            if (k < odbg.K) {
                odbg.mask[(size_t)k * T + t] = chain_hits<N, kObstNP1, true>(odt, x, kd);
#pragma unroll
                for (int a = 0; a < N; ++a) {
                    odbg.dir[((size_t)k * T + t) * 2 * N + a] = get(x.c, a);
                    odbg.dir[((size_t)k * T + t) * 2 * N + N + a] = get(x.s, a);
                }
            }
        } else if constexpr (OBST && !SDBG) {
            // on the (cos, sin) row pairs the step just produced, the ones effector() reads below
            hit_last = chain_hits<N, kObstNP1, false>(odt, x, kd) != 0;
            hits += hit_last ? 1 : 0;
        }
        if constexpr (SDBG) {
            if (k < sdbg.K) {
                sdbg.mask[(size_t)k * T + t] = chain_self_hits<N, true>(x, kd, sk.d2);
#pragma unroll
                for (int a = 0; a < N; ++a) {
                    sdbg.dir[((size_t)k * T + t) * 2 * N + a] = get(x.c, a);
                    sdbg.dir[((size_t)k * T + t) * 2 * N + N + a] = get(x.s, a);
                }
            }
        } else if constexpr (SELF) {
            self_last = chain_self_hits<N, false>(x, kd, sk.d2) != 0;
            shits += self_last ? 1 : 0;
        }
        float px, py;
        x.effector(kd, &px, &py);
        const unsigned j = sr.nearest(px, py);
        if constexpr (SLOTS) slots[(size_t)k * T + t] = (int)j;
        const float4 r = s_win[j];
        ex = px - r.x;
        ey = py - r.y;
        e1 = x.dqa(0) - r.z;
        e2 = x.dqa(1) - r.w;
        const float sw[4] = {kd.p[kOffSw], kd.p[kOffSw + 1], kd.p[kOffSw + 2], kd.p[kOffSw + 3]};   // control.py:185
        S4 += weighted_sq(ex, ey, e1, e2, sw) + g;
        if constexpr ((i & 3) == 3) {
            S += (double)S4;
            S4 = 0.f;
        }
    };
    int t = 0;
    const unsigned parity = c.fair ? __builtin_amdgcn_readfirstlane(s_parity) : 2u;
    for (; t + 4 <= T; t += 4) {
        if (parity < 2u) fair_priority(parity);
        unroll_seq([&](auto i_c) { step(t + decltype(i_c)::value, i_c); }, std::make_integer_sequence<int, 4>{});
    }
    unroll_seq([&](auto i_c) {
        if (t + decltype(i_c)::value < T) step(t + decltype(i_c)::value, i_c);
    }, std::make_integer_sequence<int, 3>{});
    S += (double)S4;
    S += (double)weighted_sq(ex, ey, e1, e2, c.dyn + kOffTw);  // terminal cost, control.py:109
    if constexpr (OBST) hits += hit_last ? 1 : 0;              // the final state once more
    if constexpr (SELF) shits += self_last ? 1 : 0;
    }
    if constexpr (ODBG || SDBG) return;
    // the penalty in one fp64 multiply and add: the count is exact, so no order of summation can change it
    if constexpr (OBST) S += ob.w * (double)hits;
    if constexpr (SELF) S += sk.w * (double)shits;             // ... the discs' product first, then this one

    STAMP(1, NOW());
    if (S_out && owner) S_out[k] = S;

    // ---- workgroup partial: rho_b, eta_b, N_b (control.py:112-118 over this block)
    // With a quad per sample (one workgroup per CU, every workgroup finishing at once) the running minimum
    // (below) is read before the block minimum, so its round trip runs under it, and the workgroup's own
    // atomic goes out after the last barrier, unwaited; with one lane per sample (two workgroups per CU,
    // finishing spread out) the atomic's fresher return skips more gathers (measured: +1.7 % with the early
    // read at config 5, -1.7 % at its shard)
    constexpr bool kEarlyRun = LPS == 4;
    unsigned long long run0 = ~0ull;
    if (kEarlyRun && tid == 0) run0 = __hip_atomic_load(runmin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const double rho_b = block_min_f64<kCT>(owner ? S : INFINITY, sm);
    // the epilogue's stages: mppi_device.h, "the rollout epilogue"
    const LaneWeight lw = block_weigh(owner, S, rho_b, c.inv_lambda, lane, wave, s_cnt, s_redd);
    // The running minimum of the workgroups' rho_b (one 64-bit atomic min per
    // workgroup on an order-preserving key; reset by the final merger).  The final
    // rho is at most any minimum over published rho_b, so a workgroup whose rho_b
    // is 2^-64 or more below it in weight can carry no weight in any merge: it
    // publishes rho_b = +inf and skips the gather of its weighted samples' noise —
    // each of those is T n scattered 4-B reads, one cache line apiece (1.14x the
    // algorithmic bytes at config 5).
    if (tid == 0) {
        const unsigned long long key = ord_key(rho_b);
        unsigned long long run;
        if constexpr (kEarlyRun) {
            run = min(run0, key);
        } else {
            const unsigned long long old = __hip_atomic_fetch_min(runmin, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            run = old < key ? old : key;
        }
        s_run = ord_val(run);
    }
    __syncthreads();
    const bool skip = exp((s_run - rho_b) * c.inv_lambda) < kMergeFloor;   // uniform
    double eta_b;
    int nl = block_compact<kCT>(lw, k, wave, s_cnt, s_redd, s_k, s_e, &eta_b);
    __syncthreads();
    // past the barriers (a barrier's fence would wait for the atomic to complete): fire and forget; the
    // gather's loads, issued after it, return after it anyway
    if (kEarlyRun && tid == 0) __hip_atomic_fetch_min(runmin, ord_key(rho_b), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int nval = T * N;
    const RowGeo geo(nval);
    const int stride = geo.stride;
    const int nrows = c.nblocks;
    const int ngroups = (nrows + kGroup - 1) / kGroup;
    constexpr int kValBytes = POLL ? 16 : 8;
    const __amdgpu_buffer_rsrc_t slab_r = rows_rsrc(slab, nrows * stride * kValBytes);
    const __amdgpu_buffer_rsrc_t gslab_r = rows_rsrc(gslab, ngroups * stride * kValBytes);
    const unsigned tag = __builtin_amdgcn_readfirstlane(tag_v);
    auto publish = [&](int idx, double v) {
        if constexpr (POLL) st_gran(slab_r, idx, v, tag);
        else st_wt(slab_r, idx, v);
    };
    // rho_b and eta_b leave first, together: rho_b waits for the skip test (rollout_kernel publishes its own
    // straight after the block minimum)
    nl = __builtin_amdgcn_readfirstlane(nl);
    if (tid == 0) {
        publish(blockIdx.x * stride, skip ? INFINITY : rho_b);
        publish(blockIdx.x * stride + 1, eta_b);
    }
    if (skip) {
        // no merge reads this row past rho
    } else if (nl <= kSparseMax) {
        // column (t, d) = t N + d of the noise: sample k's value at noise[(t K + k) N + d]
        for (int col = tid; col < nval; col += kCT) {
            const int tt = col / N;
            const float* base = noise + (size_t)tt * K * N + (col - tt * N);
            publish(blockIdx.x * stride + 2 + col, gather_col(base, N, s_k, s_e, nl));
        }
    } else {
        constexpr int PER = (NS + 63) / 64;
        constexpr int kRowBatch = 4;
        const int k0 = blockIdx.x * NS;
        double w[PER];
        dense_weights<kCT, NS>(lw, k, K, s_e, w);
        for (int cb = wave * kRowBatch; cb < nval; cb += (kCT / 64) * kRowBatch) {
            float e[kRowBatch][PER];
#pragma unroll
            for (int r = 0; r < kRowBatch; ++r) {
                const int cr = min(cb + r, nval - 1);
#pragma unroll
                for (int i = 0; i < PER; ++i) {
                    const int tt = cr / N;
                    e[r][i] = noise[((size_t)tt * K + min(k0 + lane + 64 * i, K - 1)) * N + (cr - tt * N)];
                }
            }
#pragma unroll
            for (int r = 0; r < kRowBatch; ++r) {
                double a = 0.0;
#pragma unroll
                for (int i = 0; i < PER; ++i) a = fma(w[i], (double)e[r][i], a);
                a = wave_sum_f64(a);
                if (lane == 0 && cb + r < nval) publish(blockIdx.x * stride + 2 + cb + r, a);
            }
        }
    }
    STAMP(2, NOW());
    STAMP(5, (unsigned long long)nl);
    if (!handoff_merge<kCT, kCMaxCh, POLL>(slab_r, gslab_r, nrows, geo, c.inv_lambda, sm, counters, c.acquire != 0, &s_flag,
                                           partial_out, w_eps_out, tag, epoch, tmo, dbg, nullptr))
        return;
    // every row is in: the running minimum is reset for the next launch
    if (threadIdx.x == 0) __hip_atomic_store(runmin, ~0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    STAMP(11, NOW());
    STAMP(6, (unsigned long long)sm.nrel);
    // with the exchange, the update is computed while the ranks' statuses travel: it lands in the ping-pong
    // block the host makes current only after a good verdict (on failure the host keeps its block)
    const unsigned xtag = (flags & MPPI_FLAG_EXCHANGE)
                              ? exchange_send_merge<kCT, kCMaxCh>(xd, geo, c.inv_lambda, sm, w_eps_out, tmo) : 0u;
    if (tid == 0 && w_eps_out) w_eps_out[nval] = sm.eta;   // the weights' spread (mppi_chain_last_eta)
    if constexpr (kLateNominal) chain_nominal_prefetch<N>(st, T, flags & MPPI_FLAG_FUSED_UPDATE, u_cur);
    if (flags & MPPI_FLAG_FUSED_UPDATE) chain_update_block<N, CLAMP>(nxt, c, sm, u_cur, cl);
    if (flags & MPPI_FLAG_EXCHANGE) exchange_verdict<kCT>(xd, geo, xtag, tmo);
    STAMP(7, NOW());
}

// Merge of the all-gathered per-device rows (multi-GPU), plus the fused update.
template <int N, bool CLAMP>
__global__ __launch_bounds__(kCT) void chain_merge_kernel(const ChainConst c, const ChainStep* cur, const double* parts,
                                                          int n, double* w_eps_out, ChainStep* nxt, unsigned flags,
                                                          const ChainClampK cl) {
    __shared__ CScratch sm;
    const int tid = threadIdx.x, T = c.T;
    double u_cur[kMedRun];
    chain_nominal_prefetch<N>(cur, T, flags & MPPI_FLAG_FUSED_UPDATE, u_cur);
    const RowGeo geo(T * N);
    const __amdgpu_buffer_rsrc_t r = rows_rsrc(parts, n * geo.stride * 8);
    merge_rows_block<kCT, kCMaxCh, true, RowsVia::Wt>(r, 0, n, geo, c.inv_lambda, sm, nullptr, 0, nullptr, w_eps_out,
                                                      0u, nullptr);
    if (tid == 0 && w_eps_out) w_eps_out[T * N] = sm.eta;
    if (flags & MPPI_FLAG_FUSED_UPDATE) chain_update_block<N, CLAMP>(nxt, c, sm, u_cur, cl);
}

// Trajectory re-roll (control.py:129-145 with the chain): control(t) =
// base[(t-1) mod T] (+ eps); out[k][t][2N] = (q, dq) after step t.  As in
// traj_kernel, the states of kChainTB steps go through an LDS tile and each
// flush writes every sample's kChainTB * 2N floats as one contiguous run.
// CLAMP (clamp_mode >= 1): the control fed to the dynamics is clipped, _g(u[t-1]) / _g(v[k, t-1]) of
// control.py:133,143.
constexpr int kChainTB = 2;
template <int N, bool NOISE, bool CLAMP>
__global__ __launch_bounds__(kCT) void chain_traj_kernel(const ChainConst c, const ChainStep* __restrict__ st,
                                                         const float* __restrict__ base,
                                                         const float* __restrict__ noise, int Kn,
                                                         float* __restrict__ out, const ChainClampK cl) {
    constexpr int W = 2 * N;   // floats per state
    __shared__ float tile[kChainTB][W][kCT];
    const int tid = threadIdx.x;
    const int k0 = blockIdx.x * kCT;
    const int k = min(k0 + tid, Kn - 1);   // lanes past Kn recompute the last sample, never stored
    const int nk = min(kCT, Kn - k0);
    const int T = c.T;
    const float exf = NOISE ? ((c.k_offset + k) < c.k_exploit ? 1.f : 0.f) : 1.f;
    ChainState<N> x;
    x.load(st->x0);
    // a tile's noise is loaded one tile ahead (see traj_kernel)
    auto load_tile = [&](int t0, float (&e)[kChainTB][N]) {
#pragma unroll
        for (int j = 0; j < kChainTB; ++j) {
            const int t = min(t0 + j, T - 1);
            const int ti = t == 0 ? T - 1 : t - 1;
#pragma unroll
            for (int d = 0; d < N; ++d) e[j][d] = NOISE ? noise[((size_t)ti * c.K_local + k) * N + d] : 0.f;
        }
    };
    float cur[kChainTB][N];
    load_tile(0, cur);
    for (int t0 = 0; t0 < T; t0 += kChainTB) {
        const int nt = min(kChainTB, T - t0);
        float nxt[kChainTB][N];
        load_tile(t0 + kChainTB, nxt);
#pragma unroll
        for (int j = 0; j < kChainTB; ++j) {
            if (j >= nt) break;
            const int t = t0 + j;
            const int ti = t == 0 ? T - 1 : t - 1;
            float v[N];
#pragma unroll
            for (int d = 0; d < N; ++d) {
                v[d] = base[ti * N + d];
                if (NOISE) v[d] = fmaf(exf, v[d], cur[j][d]);
                if constexpr (CLAMP) v[d] = clamp_v(v[d], cl.v_lo[d], cl.v_hi[d]);
            }
            x.step(v, DynArg{c.dyn});
#pragma unroll
            for (int a = 0; a < N; ++a) {
                tile[j][a][tid] = x.qa(a);
                tile[j][N + a][tid] = x.dqa(a);
            }
        }
        __syncthreads();
        const int run = nt * W;   // floats of one sample in this flush
        for (int i = tid; i < nk * run; i += kCT) {
            const int s = i / run, r = i - s * run;
            out[((size_t)(k0 + s) * T + t0) * W + r] = tile[r / W][r % W][s];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kChainTB; ++j)
#pragma unroll
            for (int d = 0; d < N; ++d) cur[j][d] = nxt[j][d];
    }
}

// eps[t][k][d] = (L z)_d, z ~ N(0, I) from Philox4x32-10 counters (global k, t,
// call) + Box-Muller: a shard generates exactly its slice of the unsharded draw.
// The factor travels by value (kernel argument, scalar loads) and the link count
// is a template argument, so the matvec unrolls and z stays in registers (a
// runtime-n loop indexed z dynamically and sent it to scratch: 504 us at config 5).
struct CholArg {
    float L[kCMax * kCMax];   // lower triangle, row-major, x kBoxMullerScale (box_muller's constant)
};
template <int N>
__global__ __launch_bounds__(kCT) void chain_philox_kernel(int K_local, int T, long long k_offset,
                                                           unsigned long long seed, unsigned long long step,
                                                           const CholArg Lc, float* __restrict__ out) {
    // grid (ceil(K_local / kCT), T): no 64-bit divide per thread
    const int k = (int)blockIdx.x * kCT + (int)threadIdx.x;
    if (k >= K_local) return;
    const int t = (int)blockIdx.y;
    const unsigned long long kg = (unsigned long long)(k_offset + k);
    const uint2 key = make_uint2((unsigned)seed, (unsigned)(seed >> 32) ^ (unsigned)(step >> 32));
    float z[kCMax];
#pragma unroll
    for (int call = 0; call < kCMax / 4; ++call) {
        const uint4 ctr = make_uint4((unsigned)kg, (unsigned)(kg >> 32), (unsigned)(t * 4 + call), (unsigned)step);
        const uint4 r = philox4x32_10(ctr, key);
        const float2 a = box_muller(r.x, r.y), b = box_muller(r.z, r.w);
        z[4 * call] = a.x;
        z[4 * call + 1] = a.y;
        z[4 * call + 2] = b.x;
        z[4 * call + 3] = b.y;
    }
    float* row = out + ((size_t)t * K_local + k) * N;
#pragma unroll
    for (int d = 0; d < N; ++d) {
        float e = 0.f;
#pragma unroll
        for (int j = 0; j <= d; ++j) e = fmaf(Lc.L[d * kCMax + j], z[j], e);
        row[d] = e;
    }
}

}  // namespace

// ================================================================ host side

struct mppi_chain_ctx {
    mppi_chain_config cfg;
    int device = 0, n = 0;
    hipStream_t stream = nullptr;
    int nblocks = 0;
    mppi_host::Handoff hand;       // hand-off form, its buffers and the time-out words
    ChainConst kc;
    ChainClampK ck{};              // torque limits (mode 0: none)
    ChainObstK ok{};               // workspace obstacles of the next launch (n = 0: none), mppi_chain_set_obstacles
    int obst_per_cu = 0;           // occupancy of the context's OBST rollout kernel (workgroups per CU)
    int move_per_cu = 0;           // ... and of its MOVE form
    ChainSelfK sk{};               // self-collision of the next launch (on = 0: none), mppi_chain_set_self_collision
    int self_per_cu = 0;           // occupancy of the context's SELF rollout kernel (n >= 3)
    int self_move_per_cu = 0;      // ... and of its MOVE form
    mppi_host::DevBuf<ChainStep> d_step;      // [2] ping-pong
    int cur = 0;
    mppi_host::PinnedBuf<ChainStep> h_step;   // pinned staging
    mppi_host::Event staged;
    // running minimum of the workgroups' rho_b (ord_key), ~0 between launches
    mppi_host::DevBuf<unsigned long long> d_runmin;
    mppi_host::DevBuf<double> d_weps;
    mppi_host::PinnedBuf<double> h_buf;
    mppi_host::DevBuf<float> d_base;
    mppi_host::PinnedBuf<float> h_base;
    CholArg chol{};                // Cholesky factor of Sigma x kBoxMullerScale (kCMax x kCMax, fp32) for the Philox noise
    mppi_host::DevBuf<float> d_dyn;   // packed per-step constants (DynMem), then the same in fp64 at kDynF64Off
    double h_dynd[kCDyn] = {};     // the fp64 constants on the host (the optimal trajectory)
    bool upd_valid = false;        // the current step block holds a fused update's output
    bool pub_valid = false;        // ... and h_pub is its shifted nominal as mppi_chain_wait_outputs returned it
    mppi_host::PinnedBuf<double> h_out;   // MPPI_FLAG_HOST_OUT: the update's read-back, queued right behind the launch
    mppi_host::Event out_ev;       // ... recorded after that copy
    bool out_posted = false;
    bool x_flipped = false;        // the last launch flipped the ping-pong and exchanged (undone on MPPI_E_EXCHANGE)
    double last_eta = NAN;         // the weights' spread of the last update / weighted noise read back
    double h_pub[kCMaxVals] = {};
    bool f64 = false;              // cfg.precision == 1
    int lps = 1;                   // lanes per sample: 1, or 4 (fp32 rollout at small K)
    unsigned long long* d_dbg = nullptr;
    mppi_host::Exchange ex;        // node-level exchange (mppi_chain_exchange_*)
};

namespace {

using mppi_host::fail;
using mppi_host::launch_check;

// a chain has a pair of non-adjacent links, and with it SELF kernels, from three links on
constexpr int kSelfMinN = 3;

template <int N, bool P, bool F64, int LPS, bool CL, bool OB, bool SF = false>
void launch_rollout(mppi_chain_ctx* c, const ChainStep* cur, const float* noise, double* S, double* part, ChainStep* nxt,
                    unsigned flags, int* slots = nullptr) {
    const mppi_host::Handoff& h = c->hand;
    if (slots) {   // the debug instance: identical arithmetic, plus the slot stores (unclamped contexts only)
        if constexpr (N == kCDebugN && !CL)
            hipLaunchKernelGGL((chain_rollout_kernel<N, P, F64, LPS, true>), dim3(c->nblocks), dim3(kCT), 0, c->stream, c->kc,
                               cur, c->d_dyn, noise, S, h.d_slab, h.d_gslab, h.d_counter, part, c->d_weps, nxt, flags,
                               c->ex.xd, h.d_epoch, h.h_tmo.dev, c->d_runmin,
                               reinterpret_cast<unsigned long long*>(slots), c->ck, c->ok, c->sk);
        return;
    }
    auto go = [&](auto move, auto self) {
        hipLaunchKernelGGL((chain_rollout_kernel<N, P, F64, LPS, false, CL, OB, false, move, self>), dim3(c->nblocks),
                           dim3(kCT), 0, c->stream, c->kc, cur, c->d_dyn, noise, S, h.d_slab, h.d_gslab, h.d_counter,
                           part, c->d_weps, nxt, flags, c->ex.xd, h.d_epoch, h.h_tmo.dev, c->d_runmin, c->d_dbg, c->ck,
                           c->ok, c->sk);
    };
    if constexpr (OB) {
        // a disc has a velocity: the MOVE form, which reads a row of disc records per step
        if constexpr (SF && N >= kSelfMinN) {
            if (c->ok.moving) go(std::true_type{}, std::true_type{});
            else go(std::false_type{}, std::true_type{});
            return;
        }
        if (c->ok.moving) {
            go(std::true_type{}, std::false_type{});
            return;
        }
    }
    go(std::false_type{}, std::false_type{});
}

// the link counts with an instantiated kernel: f(N) for N = n as an integral constant
template <class F>
void with_links(int n, F&& f) {
    mppi_host::with_value<2, 3, 4, 5, 6, 7>(n, f);
}

// The instantiated rollout kernels: links x POLL x (fp64 at one lane per sample, fp32 at one or four) x (plain,
// CLAMP, CLAMP + OBST).  Calls f(n, poll, f64, lps, clamp, obst), the context's instance as integral constants, in
// the hand-off form `poll`.  With `obst` the CLAMP + OBST kernel, whether or not there are torque limits (without
// them ChainClampK and the device copy of its fp32 limits hold -+inf, and clamp_mode 0 clips no nominal).
// `self`: the SELF form of the CLAMP + OBST kernel (self-collision, with or without discs); f's last argument.  A
// 2-link chain has no such kernel: its f is called with self = false.
template <class F>
void with_rollout(const mppi_chain_ctx* c, bool poll, bool obst, bool self, F&& f) {
    using L1 = std::integral_constant<int, 1>;
    using L4 = std::integral_constant<int, 4>;
    with_links(c->n, [&](auto n) {
        mppi_host::with_bool(poll, [&](auto p) {
            auto form = [&](auto cl, auto ob, auto sf) {
                if (c->f64) f(n, p, std::true_type{}, L1{}, cl, ob, sf);
                else if (c->lps == 4) f(n, p, std::false_type{}, L4{}, cl, ob, sf);
                else f(n, p, std::false_type{}, L1{}, cl, ob, sf);
            };
            if constexpr (decltype(n)::value >= kSelfMinN) {
                if (self) {
                    form(std::true_type{}, std::true_type{}, std::true_type{});
                    return;
                }
            }
            if (obst) form(std::true_type{}, std::true_type{}, std::false_type{});
            else mppi_host::with_bool(c->ck.mode != 0, [&](auto cl) { form(cl, std::false_type{}, std::false_type{}); });
        });
    });
}

// After a launch: a fused update made the other ping-pong block current.
void note_update(mppi_chain_ctx* c, unsigned flags) {
    const bool upd = (flags & MPPI_FLAG_FUSED_UPDATE) != 0;
    if (upd) c->cur ^= 1;
    c->x_flipped = upd && (flags & MPPI_FLAG_EXCHANGE);   // undone on MPPI_E_EXCHANGE
    c->upd_valid = upd;
    if (upd) c->pub_valid = false;
}

// Queues the read-back of the current block's update into h_out: the shifted nominal, then {u_first, eta}.
int queue_update_readback(mppi_chain_ctx* c) {
    const char* blk = (const char*)(c->d_step + c->cur);
    HIP_TRY(hipMemcpyAsync(c->h_out, blk + offsetof(ChainStep, u), (size_t)c->cfg.T * kCMax * sizeof(double),
                           hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(c->h_out + kCMaxVals, blk + offsetof(ChainStep, u_first), (kCMax + 1) * sizeof(double),
                           hipMemcpyDeviceToHost, c->stream));
    return MPPI_OK;
}

// Lanes per sample of the fp32 rollout: 4 while one lane per sample would leave
// SIMDs without a wave (K <= 32768: at most 512 waves of 64 samples on 1024 SIMDs);
// measured in DESIGN §3b.  The fp64 rollout keeps one lane per sample.
int chain_auto_lps(int K_local, bool f64) {
    if (f64) return 1;
    return K_local <= 32768 ? 4 : 1;
}

int check_tmo(mppi_chain_ctx* c) {
    unsigned v;
    const int rc = c->hand.take_timeout(&v);
    if (v == kTmoExchange) {
        // every rank of the step reports it and none applied the update: back to the nominal before the launch
        if (c->x_flipped) c->cur ^= 1;
        c->x_flipped = false;
        c->upd_valid = false;
        c->pub_valid = false;
        c->out_posted = false;
    } else if (v & kTmoLocal) {
        // an aborted merge left the running minimum set: clear it for the next launch
        (void)hipMemsetAsync(c->d_runmin, 0xFF, sizeof(unsigned long long), c->stream);
    }
    return rc;
}

// The device side of mppi_chain_ctx_create: the hand-off form from the rollout kernel's occupancy, then
// every buffer (on an error the caller deletes the half-built context, whose members free what they hold).
int alloc(mppi_chain_ctx* c) {
    HIP_TRY(hipSetDevice(c->device));
    int ncu = 0, per_cu = 0;
    HIP_TRY(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, c->device));
    with_rollout(c, true, false, false, [&](auto n, auto p, auto f64, auto lps, auto cl, auto ob, auto) {   // always of the POLL form
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(
            &per_cu, (const void*)chain_rollout_kernel<n, p, f64, lps, false, cl, ob>, kCT, 0);
    });
    // the kernel a launch with discs goes through: mppi_chain_set_obstacles refuses discs if it does not fit a CU
    with_rollout(c, true, true, false, [&](auto n, auto p, auto f64, auto lps, auto cl, auto ob, auto) {
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(
            &c->obst_per_cu, (const void*)chain_rollout_kernel<n, p, f64, lps, false, cl, ob>, kCT, 0);
        // ... and with moving discs (the per-step records: 16 KB of LDS more, 24 KB in fp64)
        if constexpr (ob)
            (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(
                &c->move_per_cu, (const void*)chain_rollout_kernel<n, p, f64, lps, false, cl, ob, false, true>, kCT, 0);
    });
    // ... and the ones a launch with self-collision goes through (mppi_chain_set_self_collision refuses likewise).  The
    // hand-off form below is fixed for the context's life, so it takes the smallest occupancy among the instances
    // the context may come to launch: one that does not fit is refused by its setter and never launched.
    with_rollout(c, true, true, true, [&](auto n, auto p, auto f64, auto lps, auto cl, auto ob, auto sf) {
        if constexpr (sf) {
            (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(
                &c->self_per_cu, (const void*)chain_rollout_kernel<n, p, f64, lps, false, cl, ob, false, false, true>, kCT, 0);
            (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(
                &c->self_move_per_cu, (const void*)chain_rollout_kernel<n, p, f64, lps, false, cl, ob, false, true, true>, kCT, 0);
        }
    });
    for (int o : {c->obst_per_cu, c->move_per_cu, c->self_per_cu, c->self_move_per_cu})
        if (o >= 1 && o < per_cu) per_cu = o;
    // behind the counters: the per-CU ticket words of the issue fairness (mppi_device.h)
    if (int rc = c->hand.setup(c->nblocks, ncu, per_cu, 2 + c->cfg.T * c->n, kCuSlots)) return rc;
    c->kc.acquire = c->hand.acquire;
    c->kc.cu_off = (int)c->hand.extra_off;
    c->kc.fair = c->nblocks > ncu ? 1 : 0;
    if (int rc = c->d_step.alloc_zeroed(2)) return rc;
    if (int rc = c->d_runmin.alloc(256 / sizeof(unsigned long long))) return rc;
    HIP_TRY(hipMemset(c->d_runmin, 0xFF, 256));
    if (int rc = c->d_weps.alloc_zeroed(kCMaxVals + 1)) return rc;
    if (int rc = c->d_base.alloc(kCMaxVals)) return rc;
    if (int rc = c->d_dyn.alloc(kDynBlockFloats)) return rc;   // the fp32 table, then h_dynd, then the fp32 limits
    static_assert(offsetof(ChainClampK, v_hi) == offsetof(ChainClampK, v_lo) + kCMax * sizeof(float), "v_lo, then v_hi");
    HIP_TRY(hipMemcpy(c->d_dyn + kDynLimOff, c->ck.v_lo, 2 * kCMax * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->d_dyn + kDynF64Off, c->h_dynd, sizeof(c->h_dynd), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->d_dyn, c->kc.dyn, sizeof(c->kc.dyn), hipMemcpyHostToDevice));
    if (int rc = c->h_step.alloc(1)) return rc;
    if (int rc = c->h_buf.alloc(kCMaxVals + kCMax)) return rc;
    if (int rc = c->h_base.alloc(kCMaxVals)) return rc;
    if (int rc = c->h_out.alloc(kCMaxVals + kCMax + 1)) return rc;
    if (int rc = c->staged.create()) return rc;
    if (int rc = c->out_ev.create()) return rc;
    HIP_TRY(hipDeviceSynchronize());
    memset(c->h_step, 0, sizeof(ChainStep));
    return MPPI_OK;
}

}  // namespace

extern "C" {

void mppi_chain_config_init(mppi_chain_config* cfg) {
    if (!cfg) return;
    memset(cfg, 0, sizeof(*cfg));
    cfg->param_gamma = NAN;   // lambda (1 - alpha), control.py:45
    cfg->chain.g = 9.81;      // sys_params.py:13
}

int mppi_chain_ctx_create(const mppi_chain_config* cfg, int device, void* stream, mppi_chain_ctx** out) {
    if (!cfg || !out) return fail(MPPI_E_ARG, "null argument");
    *out = nullptr;
    const int n = cfg->chain.n;
    if (n < 2 || n > 7) return fail(MPPI_E_ARG, "chain.n must be in [2, 7]");
    if (cfg->T < 1 || cfg->T > MPPI_MAX_T) return fail(MPPI_E_ARG, "T must be in [1, 128]");
    if (cfg->T * n + 1 > kCMaxCh * kCT) return fail(MPPI_E_ARG, "T * n too large");
    if (cfg->precision != 0 && cfg->precision != 1) return fail(MPPI_E_ARG, "precision must be 0 (fp32) or 1 (fp64)");
    if (cfg->clamp_mode < 0 || cfg->clamp_mode > 2) return fail(MPPI_E_ARG, "clamp_mode must be 0, 1 or 2");
    if (cfg->clamp_mode > 0)
        for (int d = 0; d < n; ++d) {
            if (isnan(cfg->u_min[d])) return fail(MPPI_E_ARG, "u_min: a limit is NaN (use -inf for no limit)");
            if (isnan(cfg->u_max[d])) return fail(MPPI_E_ARG, "u_max: a limit is NaN (use +inf for no limit)");
            if (cfg->u_min[d] > cfg->u_max[d]) return fail(MPPI_E_ARG, "u_min[d] > u_max[d]: the limits are crossed");
        }
    if (int rc = mppi_host::check_sample_geometry(cfg->K_local, cfg->K_total, cfg->k_offset)) return rc;
    if ((long long)cfg->K_local * cfg->T * n >= (1LL << 31)) return fail(MPPI_E_ARG, "too many samples");
    // Sigma: symmetric positive definite (Cholesky), inverse for the control cost
    double Lc[kCMax][kCMax] = {}, Si[kCMax * kCMax] = {};
    {
        const double* S = cfg->sigma;
        for (int j = 0; j < n; ++j) {
            double d = S[j * n + j];
            for (int q = 0; q < j; ++q) d -= Lc[j][q] * Lc[j][q];
            if (!(d > 0.0) || !isfinite(d)) return fail(MPPI_E_SINGULAR, "Sigma is not positive definite");
            Lc[j][j] = sqrt(d);
            for (int i = j + 1; i < n; ++i) {
                double e = 0.5 * (S[i * n + j] + S[j * n + i]);
                for (int q = 0; q < j; ++q) e -= Lc[i][q] * Lc[j][q];
                Lc[i][j] = e / Lc[j][j];
            }
        }
        for (int col = 0; col < n; ++col) {   // Sigma^-1 = L^-T L^-1, column by column
            double y[kCMax] = {};
            for (int i = 0; i < n; ++i) {
                double e = i == col ? 1.0 : 0.0;
                for (int q = 0; q < i; ++q) e -= Lc[i][q] * y[q];
                y[i] = e / Lc[i][i];
            }
            for (int i = n - 1; i >= 0; --i) {
                double e = y[i];
                for (int q = i + 1; q < n; ++q) e -= Lc[q][i] * y[q];
                y[i] = e / Lc[i][i];
            }
            for (int i = 0; i < n; ++i) Si[i * n + col] = y[i];
        }
    }
    auto c = std::make_unique<mppi_chain_ctx>();
    c->cfg = *cfg;
    c->device = device;
    c->n = n;
    c->stream = (hipStream_t)stream;
    c->f64 = cfg->precision == 1;
    c->lps = cfg->lanes_per_sample > 0 ? cfg->lanes_per_sample : chain_auto_lps(cfg->K_local, c->f64);
    if (c->lps != 1 && c->lps != 4) return fail(MPPI_E_ARG, "lanes_per_sample must be 0 (auto), 1 or 4");
    if (c->lps == 4 && c->f64) return fail(MPPI_E_ARG, "lanes_per_sample 4 is for the fp32 rollout");
    if (c->lps == 4 && (long long)cfg->K_local * cfg->T * n * 4 >= (1LL << 31)) {   // its noise buffer offsets
        if (cfg->lanes_per_sample > 0)
            return fail(MPPI_E_ARG, "lanes_per_sample 4 needs K_local * T * n * 4 below 2^31 bytes of noise");
        c->lps = 1;
    }
    c->nblocks = (int)(((long long)cfg->K_local * c->lps + kCT - 1) / kCT);
    ChainConst& k = c->kc;
    memset(&k, 0, sizeof(k));
    mppi_host::set_common_consts(k, *cfg, c->nblocks);
    k.n = n;
    const mppi_chain_params& P = cfg->chain;
    // the packed constants in fp64 (the fp64 rollout, the host's optimal trajectory); the fp32 rollout's
    // table is the same layout rounded entry by entry
    double* dynd = c->h_dynd;
    for (int a = 0; a < kCMax; ++a) dynd[kOffDd + a] = 1.0;   // pad rows
    for (int a = 0; a < n; ++a) {
        double tail = 0.0;
        for (int q = a + 1; q < n; ++q) tail += P.m[q];
        const double Jn = a + 1 < n ? P.J[a + 1] : 0.0;
        dynd[kOffL + a] = P.l[a];
        dynd[kOffNu + a] = P.m[a] * P.lc[a] + P.l[a] * tail;
        dynd[kOffDd + a] = P.m[a] * P.lc[a] * P.lc[a] + P.l[a] * P.l[a] * tail + P.I[a] + P.J[a] + Jn;
        dynd[kOffJ + 2 * a + ((a + 1) & 1)] = -Jn;   // row a+1 within its pair
        dynd[kOffDamp + a] = P.b[a];
        dynd[kOffFk + a] = P.fk[a];
    }
    for (int i = 0; i < 4; ++i) {
        dynd[kOffSw + i] = cfg->stage_cost_weight[i] * 10000.0;     // control.py:185
        dynd[kOffTw + i] = cfg->terminal_cost_weight[i] * 10000.0;  // control.py:198
    }
    dynd[kOffDt] = cfg->delta_t;
    dynd[kOffG] = P.g;
    for (int i = 0; i < kCDyn; ++i) k.dyn[i] = (float)dynd[i];
    for (int i = 0; i < n * n; ++i) k.sig_inv[i] = Si[i];
    ChainClampK& ck = c->ck;
    ck.mode = cfg->clamp_mode;
    for (int d = 0; d < kCMax; ++d) {
        // without limits the fields are never read; entries past the chain (the quad's pad link) never clip;
        // the fp32 rollouts clip against the limits rounded to nearest
        const bool on = cfg->clamp_mode && d < n;
        ck.u_lo[d] = on ? cfg->u_min[d] : -INFINITY;
        ck.u_hi[d] = on ? cfg->u_max[d] : INFINITY;
        ck.v_lo[d] = (float)ck.u_lo[d];
        ck.v_hi[d] = (float)ck.u_hi[d];
    }

    for (int j = 0; j < MPPI_MAX_OBSTACLES; ++j) {   // no discs
        c->ok.r2[j] = -1.f;
        c->ok.r2d[j] = -1.0;
    }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) c->chol.L[i * kCMax + j] = (float)(Lc[i][j] * kBoxMullerScale);   // box_muller's constant
    if (int rc = alloc(c.get())) return rc;
    *out = c.release();
    return MPPI_OK;
}

void mppi_chain_ctx_destroy(mppi_chain_ctx* c) {
    if (!c) return;
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    (void)hipDeviceSynchronize();
    delete c;
}

int mppi_chain_set_stream(mppi_chain_ctx* c, void* stream) {
    if (!c) return fail(MPPI_E_ARG, "null context");
    c->stream = (hipStream_t)stream;
    return MPPI_OK;
}

int mppi_chain_ctx_info(const mppi_chain_ctx* c, int* blocks, int* threads, int* poll, int* lanes_per_sample) {
    if (!c) return fail(MPPI_E_ARG, "null context");
    if (lanes_per_sample) *lanes_per_sample = c->lps;
    if (blocks) *blocks = c->nblocks;
    if (threads) *threads = kCT;
    if (poll) *poll = c->hand.poll ? 1 : 0;
    return MPPI_OK;
}

int mppi_chain_set_step_inputs(mppi_chain_ctx* c, const double* x0, const double* window, int W, const double* u) {
    if (!c || !x0 || !window) return fail(MPPI_E_ARG, "null argument");
    if (W < 1 || W > MPPI_SEARCH_LEN) return fail(MPPI_E_ARG, "window rows must be in [1, 30]");
    const int n = c->n, T = c->cfg.T;
    HIP_TRY(hipEventSynchronize(c->staged));
    ChainStep* h = c->h_step;
    mppi_host::stage_window(window, W, h->win, h->key, &h->ctr);
    for (int a = 0; a < 2 * kCMax; ++a) h->x0[a] = a < 2 * n ? (float)x0[a] : 0.f;
    // fp64 rollout: x0 as [q(n), dq(n)] and the window rows unrounded
    for (int a = 0; a < 2 * kCMax; ++a) h->x0d[a] = a < 2 * n ? x0[a] : 0.0;
    for (int j = 0; j < kSlots; ++j)
        for (int i = 0; i < 4; ++i) h->wind[j][i] = j < W ? window[4 * j + i] : 0.0;
    size_t bytes = offsetof(ChainStep, ua);
    // the caller's u is the nominal the last fused launch wrote and wait_outputs returned: the device block
    // already holds it with the same (u, a) bits the staging below would compute, so only x0 and the window go
    bool same = u && c->pub_valid;
    for (int t = 0; same && t < T; ++t)
        for (int d = 0; d < n; ++d) same = same && u[t * n + d] == c->h_pub[t * kCMax + d];
    if (same) u = nullptr;
    if (u) {
        const ChainConst& k = c->kc;
        for (int t = 0; t < T; ++t) {
            for (int d = 0; d < kCMax; ++d) {
                h->ua[t][d] = d < n ? (float)u[t * n + d] : 0.f;
                h->u[t][d] = d < n ? u[t * n + d] : 0.0;
                double a = 0.0;
                if (d < n)
                    for (int e2 = 0; e2 < n; ++e2) a += (k.gamma * u[t * n + e2]) * k.sig_inv[e2 * n + d];
                h->ua[t][kCMax + d] = (float)a;
                h->a[t][d] = a;
            }
        }
        bytes = sizeof(ChainStep);
        c->upd_valid = false;   // the block now holds the staged nominal, not a fused update's output
        c->pub_valid = false;
    }
    HIP_TRY(hipMemcpyAsync(c->d_step + (c->cur ^ 1), h, offsetof(ChainStep, ua), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_step + c->cur, h, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipEventRecord(c->staged, c->stream));
    return MPPI_OK;
}

}  // extern "C"

namespace {
// slots: the debug instances (kCDebugN links) record every sample's window slot per step
int chain_rollout(mppi_chain_ctx* c, const float* noise_dev, double* S_dev, double* partial_dev, unsigned flags,
                  int* slots) {
    if (!c || !noise_dev) return fail(MPPI_E_ARG, "null argument");
    if ((flags & MPPI_FLAG_FUSED_UPDATE) && c->cfg.T < 5)
        return fail(MPPI_E_ARG, "device median filter needs T >= 5 (use the host update)");
    if (flags & MPPI_FLAG_EXCHANGE) {
        if (c->ex.xd.world < 1) return fail(MPPI_E_ARG, "MPPI_FLAG_EXCHANGE before mppi_chain_exchange_attach");
        if (partial_dev) return fail(MPPI_E_ARG, "MPPI_FLAG_EXCHANGE merges on device: no partial_out");
        partial_dev = c->ex.d_xrow;
    }
    const ChainStep* cur = c->d_step + c->cur;
    ChainStep* nxt = c->d_step + (c->cur ^ 1);
    with_rollout(c, c->hand.poll, c->ok.n > 0, c->sk.on != 0, [&](auto n, auto p, auto f64, auto lps, auto cl, auto ob, auto sf) {
        launch_rollout<n, p, f64, lps, cl, ob, sf>(c, cur, noise_dev, S_dev, partial_dev, nxt, flags, slots);
    });
    if (int rc = launch_check("chain_rollout_kernel")) return rc;
    note_update(c, flags);
    c->out_posted = false;
    if ((flags & MPPI_FLAG_FUSED_UPDATE) && (flags & MPPI_FLAG_HOST_OUT)) {
        // the update's read-back right behind the launch, so what the caller queues next (the next
        // step's noise) does not delay mppi_chain_wait_outputs
        if (int rc = queue_update_readback(c)) return rc;
        HIP_TRY(hipEventRecord(c->out_ev, c->stream));
        c->out_posted = true;
    }
    return MPPI_OK;
}
}  // namespace

extern "C" {

int mppi_chain_rollout(mppi_chain_ctx* c, const float* noise_dev, double* S_dev, double* partial_dev, unsigned flags) {
    return chain_rollout(c, noise_dev, S_dev, partial_dev, flags, nullptr);
}

int mppi_chain_debug_slots(mppi_chain_ctx* c, const float* noise_dev, double* S_dev, int* slots_dev) {
    if (!c || !noise_dev || !slots_dev) return fail(MPPI_E_ARG, "null argument");
    if (c->n != kCDebugN) return fail(MPPI_E_ARG, "slot recording is built for the 7-link chain only");
    if (c->ck.mode != 0) return fail(MPPI_E_ARG, "slot recording is built without torque limits (clamp_mode 0 only)");
    if (c->ok.n > 0) return fail(MPPI_E_ARG, "slot recording is built without obstacles (remove the discs first)");
    if (c->sk.on) return fail(MPPI_E_ARG, "slot recording is built without self collision (disable it first)");
    return chain_rollout(c, noise_dev, S_dev, nullptr, 0u, slots_dev);
}

int mppi_chain_set_obstacles(mppi_chain_ctx* c, int n, const double* discs, double cost) {
    return mppi_chain_set_moving_obstacles(c, n, discs, nullptr, cost);
}

int mppi_chain_set_moving_obstacles(mppi_chain_ctx* c, int n, const double* discs, const double* vel, double cost) {
    if (!c) return fail(MPPI_E_ARG, "null context");
    if (n < 0 || n > MPPI_MAX_OBSTACLES) return fail(MPPI_E_ARG, "obstacles: n must be in [0, 8]");
    if (n > 0 && !discs) return fail(MPPI_E_ARG, "obstacles: null discs");
    if (!(cost >= 0.0) || isinf(cost)) return fail(MPPI_E_ARG, "obstacles: the cost must be finite and >= 0");
    if (n > 0 && c->obst_per_cu < 1) return fail(MPPI_E_ARG, "obstacles: the rollout kernel with discs does not fit a CU");
    ChainObstK k{};
    for (int j = 0; j < MPPI_MAX_OBSTACLES; ++j) {   // below every squared distance: never touched
        k.r2[j] = -1.f;
        k.r2d[j] = -1.0;
    }
    for (int j = 0; j < n; ++j) {
        const double cx = discs[3 * j], cy = discs[3 * j + 1], r = discs[3 * j + 2];
        if (!isfinite((float)cx) || !isfinite((float)cy)) return fail(MPPI_E_ARG, "obstacles: a centre is not finite");
        if (!(r >= 0.0)) return fail(MPPI_E_ARG, "obstacles: a radius is NaN or negative");
        k.cx[j] = (float)cx;
        k.cy[j] = (float)cy;
        k.r2[j] = (float)(r * r);
        k.cxd[j] = cx;
        k.cyd[j] = cy;
        k.r2d[j] = r * r;
        if (!vel) continue;
        const double vx = vel[2 * j], vy = vel[2 * j + 1];
        if (!isfinite((float)vx) || !isfinite((float)vy)) return fail(MPPI_E_ARG, "obstacles: a velocity is not finite");
        k.vx[j] = (float)vx;
        k.vy[j] = (float)vy;
        k.vxd[j] = vx;
        k.vyd[j] = vy;
        if (k.vx[j] != 0.f || k.vy[j] != 0.f) k.moving = 1;   // else the kernels of discs at rest, as vel = NULL
        // the last row of the kernels' table (step T - 1), the farthest the disc gets
        const float tau = (float)((double)c->cfg.T * c->cfg.delta_t);
        if (!isfinite(fmaf(k.vx[j], tau, k.cx[j])) || !isfinite(fmaf(k.vy[j], tau, k.cy[j])))
            return fail(MPPI_E_ARG, "obstacles: a centre is not finite at the end of the horizon");
    }
    if (k.moving && c->move_per_cu < 1)
        return fail(MPPI_E_ARG, "obstacles: the rollout kernel with moving discs does not fit a CU");
    if (k.moving && c->sk.on && c->self_move_per_cu < 1)
        return fail(MPPI_E_ARG, "obstacles: the rollout kernel with moving discs and self collision does not fit a CU");
    k.dt = c->cfg.delta_t;
    k.w = cost;
    k.n = n;
    c->ok = k;   // read by the next launch of any kind (a kernel argument, by value): no device call
    return MPPI_OK;
}

int mppi_chain_debug_obstacle_hits(mppi_chain_ctx* c, const float* noise_dev, int K, unsigned long long* mask_dev,
                                   float* dir_dev) {
    if (!c || !noise_dev || !mask_dev || !dir_dev || K < 1 || K > c->cfg.K_local) return fail(MPPI_E_ARG, "bad argument");
    if (c->obst_per_cu < 1 || c->move_per_cu < 1)
        return fail(MPPI_E_ARG, "obstacles: the rollout kernel with discs does not fit a CU");
    // the quad form adds each lane's bits to its sample's mask
    HIP_TRY(hipMemsetAsync(mask_dev, 0, (size_t)K * c->cfg.T * sizeof(unsigned long long), c->stream));
    // the context's own form of the OBST kernel, always with a row of disc records per step (at rest the rows are
    // equal: fma(0, tau, c) = c), counter hand-off (it ends before any hand-off), over the
    // workgroups that hold the first K samples; the masks travel in gslab's place, the directions in slab's and K
    // in flags'; no timeline buffer
    const int blocks = (int)(((long long)K * c->lps + kCT - 1) / kCT);
    const mppi_host::Handoff& h = c->hand;
    const ChainStep* cur = c->d_step + c->cur;
    with_rollout(c, false, true, false, [&](auto n, auto p, auto f64, auto lps, auto cl, auto ob, auto) {
        if constexpr (ob && !p)   // (with_rollout also instantiates this lambda for the other kernels)
            hipLaunchKernelGGL((chain_rollout_kernel<n, p, f64, lps, false, cl, ob, true, true>), dim3(blocks), dim3(kCT), 0,
                               c->stream, c->kc, cur, c->d_dyn, noise_dev, (double*)nullptr,
                               reinterpret_cast<double*>(dir_dev), reinterpret_cast<double*>(mask_dev), h.d_counter,
                               (double*)nullptr, (double*)nullptr, (ChainStep*)nullptr, (unsigned)K, c->ex.xd, h.d_epoch,
                               h.h_tmo.dev, c->d_runmin, (unsigned long long*)nullptr, c->ck, c->ok, c->sk);
    });
    return launch_check("chain_rollout_kernel (obstacle debug)");
}

int mppi_chain_set_self_collision(mppi_chain_ctx* c, int enable, double clearance, double cost) {
    if (!c) return fail(MPPI_E_ARG, "null context");
    if (!(clearance >= 0.0) || isinf(clearance))
        return fail(MPPI_E_ARG, "self collision: the clearance must be finite and >= 0");
    if (!(cost >= 0.0) || isinf(cost)) return fail(MPPI_E_ARG, "self collision: the cost must be finite and >= 0");
    const bool on = enable != 0 && c->n >= kSelfMinN;   // a 2-link chain has no non-adjacent pair: accepted, no effect
    if (on && c->self_per_cu < 1) return fail(MPPI_E_ARG, "self collision: the rollout kernel with it does not fit a CU");
    if (on && c->ok.moving && c->self_move_per_cu < 1)
        return fail(MPPI_E_ARG, "self collision: the rollout kernel with it and moving discs does not fit a CU");
    ChainSelfK k{};
    k.d2d = clearance * clearance;
    k.d2 = (float)k.d2d;   // rounded once, from the fp64 product
    k.w = cost;
    k.on = on ? 1 : 0;
    c->sk = k;   // read by the next launch of any kind (a kernel argument, by value): no device call
    return MPPI_OK;
}

int mppi_chain_debug_self_hits(mppi_chain_ctx* c, const float* noise_dev, int K, unsigned* mask_dev, float* dir_dev) {
    if (!c || !noise_dev || !mask_dev || !dir_dev || K < 1 || K > c->cfg.K_local) return fail(MPPI_E_ARG, "bad argument");
    // every form writes each of the first K samples' masks once, so only a chain without pairs needs the zeroes
    HIP_TRY(hipMemsetAsync(mask_dev, 0, (size_t)K * c->cfg.T * sizeof(unsigned), c->stream));
    if (c->n < kSelfMinN) {   // no pairs, no kernel: no bit is ever set, and the directions stay zero
        HIP_TRY(hipMemsetAsync(dir_dev, 0, (size_t)K * c->cfg.T * 2 * c->n * sizeof(float), c->stream));
        return MPPI_OK;
    }
    if (c->self_per_cu < 1) return fail(MPPI_E_ARG, "self collision: the rollout kernel with it does not fit a CU");
    // the context's own form of the SELF kernel with the clearance in effect, discs at rest skipped (the recording
    // instances run no disc test), counter hand-off (it ends before any hand-off), over the workgroups that hold the
    // first K samples; the masks travel in gslab's place, the directions in slab's and K in flags'
    const int blocks = (int)(((long long)K * c->lps + kCT - 1) / kCT);
    const mppi_host::Handoff& h = c->hand;
    const ChainStep* cur = c->d_step + c->cur;
    with_rollout(c, false, true, true, [&](auto n, auto p, auto f64, auto lps, auto cl, auto ob, auto sf) {
        if constexpr (sf && !p)
            hipLaunchKernelGGL((chain_rollout_kernel<n, p, f64, lps, false, cl, ob, false, false, true, true>), dim3(blocks),
                               dim3(kCT), 0, c->stream, c->kc, cur, c->d_dyn, noise_dev, (double*)nullptr,
                               reinterpret_cast<double*>(dir_dev), reinterpret_cast<double*>(mask_dev), h.d_counter,
                               (double*)nullptr, (double*)nullptr, (ChainStep*)nullptr, (unsigned)K, c->ex.xd, h.d_epoch,
                               h.h_tmo.dev, c->d_runmin, (unsigned long long*)nullptr, c->ck, c->ok, c->sk);
    });
    return launch_check("chain_rollout_kernel (self-collision debug)");
}


int mppi_chain_exchange_handle(mppi_chain_ctx* c, int world, void* handle_out) {
    if (!c || !handle_out || world < 1 || world > kMaxWorld) return fail(MPPI_E_ARG, "bad argument");
    return c->ex.handle(c->device, 2 + c->cfg.T * c->n, world, handle_out);
}

int mppi_chain_exchange_attach(mppi_chain_ctx* c, int rank, int world, const void* handles) {
    if (!c || !handles || world < 1 || rank < 0 || rank >= world) return fail(MPPI_E_ARG, "bad argument");
    if (!c->ex.d_inbox || c->ex.world_alloc != world) return fail(MPPI_E_ARG, "call mppi_chain_exchange_handle(world) first");
    return c->ex.attach(c->device, rank, world, handles);
}

int mppi_chain_merge_partials(mppi_chain_ctx* c, const double* partials_dev, int nparts, unsigned flags) {
    if (!c || !partials_dev || nparts < 1) return fail(MPPI_E_ARG, "bad argument");
    if ((flags & MPPI_FLAG_FUSED_UPDATE) && c->cfg.T < 5)
        return fail(MPPI_E_ARG, "device median filter needs T >= 5 (use the host update)");
    const ChainStep* cur = c->d_step + c->cur;
    ChainStep* nxt = c->d_step + (c->cur ^ 1);
    with_links(c->n, [&](auto n) {
        mppi_host::with_bool(c->ck.mode != 0, [&](auto cl) {
            hipLaunchKernelGGL((chain_merge_kernel<n, cl>), dim3(1), dim3(kCT), 0, c->stream, c->kc, cur, partials_dev,
                               nparts, c->d_weps, nxt, flags, c->ck);
        });
    });
    if (int rc = launch_check("chain_merge_kernel")) return rc;
    note_update(c, flags);
    return MPPI_OK;
}

int mppi_chain_get_weighted_noise(mppi_chain_ctx* c, double* w_eps_host) {
    if (!c || !w_eps_host) return fail(MPPI_E_ARG, "null argument");
    const size_t bytes = (size_t)c->cfg.T * c->n * sizeof(double);
    HIP_TRY(hipMemcpyAsync(c->h_buf, c->d_weps, bytes + sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    memcpy(w_eps_host, c->h_buf, bytes);
    c->last_eta = c->h_buf[(size_t)c->cfg.T * c->n];
    return check_tmo(c);
}

int mppi_chain_get_nominal(mppi_chain_ctx* c, double* u_host) {
    if (!c || !u_host) return fail(MPPI_E_ARG, "null argument");
    const int n = c->n, T = c->cfg.T;
    HIP_TRY(hipMemcpyAsync(c->h_buf, (const char*)(c->d_step + c->cur) + offsetof(ChainStep, u),
                           (size_t)T * kCMax * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int t = 0; t < T; ++t)
        for (int d = 0; d < n; ++d) u_host[t * n + d] = c->h_buf[t * kCMax + d];
    return check_tmo(c);
}

int mppi_chain_last_eta(const mppi_chain_ctx* c, double* eta) {
    if (!c || !eta) return fail(MPPI_E_ARG, "null argument");
    *eta = c->last_eta;
    return MPPI_OK;
}

}  // extern "C"

namespace {
// control.py:129-134 for the chain in fp64 on the host: x_{t+1} = F(x_t, u_new[t - 1]) (u_new[-1] at t = 0),
// the same ChainStateD step as the fp64 rollout.  One sequential trajectory: the host's fp64 is ~5x the
// device's single lane here (~1.7 us per step of dependent VALU on one wave).
// lim: the torque limits (u_lo[kCMax], u_hi[kCMax]) when the context has them: the control is clipped as it is
// fed to the step (_g(u[t-1]), control.py:133), u_new itself untouched; null: none.
template <int N>
__attribute__((always_inline)) inline void chain_traj_body(const double* kd, const double* x0, const double* u_new,
                                                           int T, double* out, const double* lim) {
    ChainStateD<N> x;
    x.load(x0);
    for (int t = 0; t < T; ++t) {
        const double* ut = u_new + (size_t)N * (t == 0 ? T - 1 : t - 1);
        double v[N];
        for (int d = 0; d < N; ++d) v[d] = lim ? clamp_u(ut[d], lim[d], lim[kCMax + d]) : ut[d];
        x.step(v, kd);
        for (int a = 0; a < N; ++a) {
            out[(size_t)t * 2 * N + a] = x.q[a];
            out[(size_t)t * 2 * N + N + a] = x.dq[a];
        }
    }
}
// The step's fma() calls as the hardware instruction where the CPU has it (the baseline x86-64 target calls
// libm's fma ~600 times per step set); fma is correctly rounded either way, and the host side of this file is
// compiled with -ffp-contract=off (build.py), so no other multiply-add is fused in either instance: the same
// bits (MPPI_HOST_FMA=0 forces the baseline instance; tests/test_gpu_chain.py compares the two).
template <int N>
__attribute__((target("fma"))) void chain_traj_host_fma(const double* kd, const double* x0, const double* u_new,
                                                        int T, double* out, const double* lim) {
    chain_traj_body<N>(kd, x0, u_new, T, out, lim);
}
template <int N>
void chain_traj_host(const double* kd, const double* x0, const double* u_new, int T, double* out, const double* lim) {
    static const bool hw_fma = __builtin_cpu_supports("fma");
    const char* force = getenv("MPPI_HOST_FMA");
    if (hw_fma && !(force && force[0] == '0')) chain_traj_host_fma<N>(kd, x0, u_new, T, out, lim);
    else chain_traj_body<N>(kd, x0, u_new, T, out, lim);
}
}  // namespace

extern "C" {

int mppi_chain_wait_outputs(mppi_chain_ctx* c, const double* x0, double* u_out, double* traj_out) {
    if (!c || !u_out || (traj_out && !x0)) return fail(MPPI_E_ARG, "bad argument");
    if (!c->upd_valid) return fail(MPPI_E_ARG, "no fused update to read (mppi_chain_rollout with MPPI_FLAG_FUSED_UPDATE)");
    const int n = c->n, T = c->cfg.T;
    const double* h = c->h_out;
    if (c->out_posted) {   // MPPI_FLAG_HOST_OUT: the copy is already queued behind the launch
        HIP_TRY(hipEventSynchronize(c->out_ev));
    } else {
        if (int rc = queue_update_readback(c)) return rc;
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    if (int rc = check_tmo(c)) return rc;
    c->last_eta = h[kCMaxVals + kCMax];
    for (int t = 0; t < T; ++t)
        for (int d = 0; d < n; ++d) u_out[t * n + d] = h[t * kCMax + d];
    memcpy(c->h_pub, h, (size_t)T * kCMax * sizeof(double));
    c->pub_valid = true;
    if (traj_out) {
        // the update before the shift: u_new[0] from the block, u_new[t] = shifted[t - 1] for t >= 1
        double un[kMaxT * kCMax];
        for (int d = 0; d < n; ++d) un[d] = h[kCMaxVals + d];
        for (int t = 1; t < T; ++t)
            for (int d = 0; d < n; ++d) un[t * n + d] = h[(t - 1) * kCMax + d];
        return mppi_chain_optimal_traj_host(c, x0, un, traj_out);
    }
    return MPPI_OK;
}

int mppi_chain_optimal_traj_host(mppi_chain_ctx* c, const double* x0, const double* u_new, double* traj_out) {
    if (!c || !x0 || !u_new || !traj_out) return fail(MPPI_E_ARG, "null argument");
    static_assert(offsetof(ChainClampK, u_hi) == offsetof(ChainClampK, u_lo) + kCMax * sizeof(double), "u_lo, then u_hi");
    const double* lim = c->ck.mode != 0 ? c->ck.u_lo : nullptr;   // clamp_mode >= 1: the control is clipped in fp64
    with_links(c->n, [&](auto n) { chain_traj_host<n>(c->h_dynd, x0, u_new, c->cfg.T, traj_out, lim); });
    return MPPI_OK;
}

int mppi_chain_rollout_traj(mppi_chain_ctx* c, const double* base_u, const float* noise_dev, int K, float* out_dev) {
    if (!c || !out_dev || K < 1 || K > c->cfg.K_local) return fail(MPPI_E_ARG, "bad argument");
    const int n = c->n, T = c->cfg.T;
    const ChainStep* cur = c->d_step + c->cur;
    if (base_u) {
        HIP_TRY(hipEventSynchronize(c->staged));
        for (int i = 0; i < T * n; ++i) c->h_base[i] = (float)base_u[i];
        HIP_TRY(hipMemcpyAsync(c->d_base, c->h_base, (size_t)T * n * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipEventRecord(c->staged, c->stream));
    } else {
        // the nominal u of the current step block: ua[t][0:n], row stride 2 kCMax floats
        HIP_TRY(hipMemcpy2DAsync(c->d_base, n * sizeof(float), (const char*)cur + offsetof(ChainStep, ua),
                                 2 * kCMax * sizeof(float), n * sizeof(float), T, hipMemcpyDeviceToDevice, c->stream));
    }
    const int blocks = (K + kCT - 1) / kCT;
    with_links(n, [&](auto nl) {
        mppi_host::with_bool(noise_dev != nullptr, [&](auto noisy) {
            mppi_host::with_bool(c->ck.mode != 0, [&](auto cl) {
                hipLaunchKernelGGL((chain_traj_kernel<nl, noisy, cl>), dim3(blocks), dim3(kCT), 0, c->stream, c->kc, cur,
                                   c->d_base, noise_dev, K, out_dev, c->ck);
            });
        });
    });
    return launch_check("chain_traj_kernel");
}

int mppi_chain_noise_philox(mppi_chain_ctx* c, unsigned long long seed, unsigned long long step, float* out_dev) {
    if (!c || !out_dev) return fail(MPPI_E_ARG, "null argument");
    const dim3 grid((unsigned)((c->cfg.K_local + kCT - 1) / kCT), (unsigned)c->cfg.T);
    with_links(c->n, [&](auto n) {
        hipLaunchKernelGGL(chain_philox_kernel<n>, grid, dim3(kCT), 0, c->stream, c->cfg.K_local, c->cfg.T,
                           (long long)c->cfg.k_offset, seed, step, c->chol, out_dev);
    });
    return launch_check("chain_philox_kernel");
}

int mppi_chain_sync(mppi_chain_ctx* c) {
    if (!c) return fail(MPPI_E_ARG, "null context");
    HIP_TRY(hipStreamSynchronize(c->stream));
    return check_tmo(c);
}

int mppi_chain_debug_set_buffer(mppi_chain_ctx* c, void* dbg_dev) {
    if (!c) return fail(MPPI_E_ARG, "null context");
    c->d_dbg = (unsigned long long*)dbg_dev;
    return MPPI_OK;
}

}  // extern "C"
