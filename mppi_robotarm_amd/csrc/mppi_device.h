// mppi_device.h — device building blocks shared by the MPPI kernels for gfx950 (mppi_rocm.hip: the reference's
// 2-link arm; mppi_chain.hip: the n-link chain of BASELINE config 5): DPP wave reductions, the window search, the
// sparse epilogue gather, the rollout epilogue's stages, the median-of-10 network, Philox, the issue fairness between
// co-resident workgroups.  Ends by including mppi_merge.h: the rows handed between workgroups and their merges.
#pragma once

#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include <type_traits>
#include <utility>

#include "mppi_rocm.h"  // MPPI_SEARCH_LEN, MPPI_MAX_T

namespace mppi {

// Diagnostic builds only (-DMPPI_STAMPS, a separate .so): per-workgroup
// timeline in s_memrealtime ticks (100 MHz) + counters.  Never in the product.
#ifdef MPPI_STAMPS
#define STAMP(slot, val) do { if (dbg && threadIdx.x == 0) dbg[(size_t)blockIdx.x * 16 + (slot)] = (val); } while (0)
#define NOW() __builtin_amdgcn_s_memrealtime()
#else
#define STAMP(slot, val) do { (void)dbg; } while (0)
#define NOW() 0ull
#endif

constexpr int kMaxT = MPPI_MAX_T;

constexpr int kSlots = 32;             // window slots (>= MPPI_SEARCH_LEN), index fits 5 bits
constexpr float kPadKey = 1.0e30f;
constexpr int kMaxWaves = 16;          // up to 1024-thread workgroups
constexpr int kGroup = 16;             // workgroups per first-level merge group
// A partial whose rescale factor s = exp((rho - rho_i) / lambda) is below 2^-64
// changes eta and N by less than 2^-64 * 512 relative to the leading term
// (which has s = 1 and eta >= 1): far below the fp64 resolution of the result.
constexpr double kMergeFloor = 5.421010862427522e-20;  // 2^-64
constexpr int kDirectRows = 256;       // workgroup rows the direct merge scans (4 per lane)
constexpr int kDirectMax = 16;         // weighted rows it merges; more go through the group rows
constexpr int kSparseMax = 16;         // weighted samples per workgroup handled by the epilogue gather

// ------------------------------------------------------------------ helpers

// Hardware v_sin_f32 / v_cos_f32 (argument pre-scaled by 1/(2 pi)): 30 % faster
// rollouts than OCML's sincosf at K=65536 T=64, parity unchanged (S rel-err
// budget 5e-5 in tests/test_gpu_parity.py).
__device__ __forceinline__ void sincos_f32(float x, float* s, float* c) { __sincosf(x, s, c); }

// np.clip of one fp64 control (lo <= hi; a NaN passes through, as everywhere outside the contract)
__host__ __device__ __forceinline__ double clamp_u(double u, double lo, double hi) { return u < lo ? lo : (u > hi ? hi : u); }

// Every control used here (quad_perm, row_mirror, row_half_mirror, row_ror) reads
// a valid lane, so bound_ctrl changes no value; set, it lets the compiler fold the
// move into a VOP1 / VOP2 consumer (v_mul_f32_dpp, v_add_f32_dpp, v_rsq_f32_dpp:
// GCNDPPCombine takes a move with an undefined old value only under bound_ctrl).
constexpr bool kDppBC = true;
template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xF, 0xF, kDppBC));
}

__device__ __forceinline__ int lanes_below(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_mov_dpp((int)b, CTRL, 0xF, 0xF, kDppBC);
    const int hi = __builtin_amdgcn_mov_dpp((int)(b >> 32), CTRL, 0xF, 0xF, kDppBC);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

// v from lane l as a wave-uniform (scalar) value
__device__ __forceinline__ double readlane_f64(double v, int l) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)b, l);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
__device__ __forceinline__ float readlane_f32(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

// v_min_f64 / v_max_f64 issued directly: fmin()/fmax() make hipcc canonicalise
// both operands first (a v_max_f64 x, x each).  Same results for every input
// but signalling NaNs (IEEE minNum / maxNum, like fmin / fmax).
__device__ __forceinline__ double min_raw_f64(double a, double b) {
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ double max_raw_f64(double a, double b) {
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// Whole-wave reductions (all 64 lanes active), result wave-uniform: DPP
// quad_perm xor 1 / xor 2, row_half_mirror, row_mirror reduce each row of 16
// in registers, then the four row results are combined from v_readlane — no
// LDS round trips (a ds_bpermute butterfly costs six of them).  The combine
// order is fixed, so sums are deterministic.
template <class T, class Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
    if constexpr (sizeof(T) == 8) {
        v = op(v, dpp_f64<0xB1>(v));
        v = op(v, dpp_f64<0x4E>(v));
        v = op(v, dpp_f64<0x141>(v));
        v = op(v, dpp_f64<0x140>(v));
        return op(op(readlane_f64(v, 0), readlane_f64(v, 16)), op(readlane_f64(v, 32), readlane_f64(v, 48)));
    } else {
        v = op(v, dpp_f32<0xB1>(v));
        v = op(v, dpp_f32<0x4E>(v));
        v = op(v, dpp_f32<0x141>(v));
        v = op(v, dpp_f32<0x140>(v));
        return op(op(readlane_f32(v, 0), readlane_f32(v, 16)), op(readlane_f32(v, 32), readlane_f32(v, 48)));
    }
}
struct OpMin {
    __device__ double operator()(double a, double b) const { return min_raw_f64(a, b); }
};
struct OpAdd {
    template <class T>
    __device__ T operator()(T a, T b) const { return a + b; }
};
__device__ __forceinline__ double wave_min_f64(double v) { return wave_reduce(v, OpMin{}); }
__device__ __forceinline__ double wave_sum_f64(double v) { return wave_reduce(v, OpAdd{}); }
__device__ __forceinline__ float wave_sum_f32(float v) { return wave_reduce(v, OpAdd{}); }

// The k-th (0-based) set bit of m; k < popcount(m).
__device__ __forceinline__ int select_bit(unsigned long long m, int k) {
    int pos = 0;
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) {
        const int cnt = __popcll(m & ((1ull << w) - 1));
        if (k >= cnt) {
            k -= cnt;
            m >>= w;
            pos += w;
        }
    }
    return pos;
}

template <class F, int... I>
__device__ __forceinline__ void unroll_seq(F&& f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}

// Scheduling boundary after each prefetch: an empty asm statement with a
// memory clobber keeps the load where it is written (otherwise the scheduler
// sinks it next to its use and every step pays the full memory latency).
#define PIN_LOADS() asm volatile("" ::: "memory")

// The per-step constants are read through the constant address space: scalar
// (SMEM) loads that stay scalar across the scheduling boundaries above.  Their
// block is written only by host copies or by the PREVIOUS launch (ping-pong).
typedef __attribute__((address_space(4))) const float cfloat;
__device__ __forceinline__ float4 const_ld4(cfloat* p) { return make_float4(p[0], p[1], p[2], p[3]); }

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// v_min3_f32 / v_min_f32 issued directly: the operands are bit-packed keys, and
// fminf() would make hipcc canonicalise every one of them (v_max x, x) first.
__device__ __forceinline__ float min3_raw(float a, float b, float c) {
    float r;
    asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ float min_raw(float a, float b) {
    float r;
    asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// ------------------------------------------------------------ window search

// Minimum of N packed keys as a tree of v_min3 (depth ceil(log3 N))
template <int N>
__device__ __forceinline__ float min_tree(const float (&k)[N]) {
    if constexpr (N == 1) {
        return k[0];
    } else {
        constexpr int M = (N + 2) / 3;
        float r[M];
#pragma unroll
        for (int g = 0; g < M; ++g) {
            const int a = 3 * g;
            if (a + 2 < N) r[g] = min3_raw(k[a], k[a + 1], k[a + 2]);
            else if (a + 1 < N) r[g] = min_raw(k[a], k[a + 1]);
            else r[g] = k[a];
        }
        return min_tree<M>(r);
    }
}

// Nearest waypoint of the shared window (control.py:200-232): the window is
// uploaded as centred keys (-2 rx', -2 ry', rx'^2 + ry'^2; pads 1e30 — the
// factor -2 is exact, so it costs nothing to fold it into the table), and
//   argmin_j |p - r_j|^2 = argmin_j (|r'_j|^2 - 2 p'.r'_j),
// two slots per v_pk_fma_f32; the slot index is packed into the 5 low mantissa
// bits so one v_min3 per two slots carries the argmin (first occurrence: equal
// keys resolve to the lower slot); the LPS lanes of a sample split the window
// and close the min with DPP.
//
// Precision: packing quantises a key to 2^-18 of its magnitude, ~|r'|^2 (the
// window's half-extent squared, ~5e-4 m^2 on xydq_circle.txt), so two
// waypoints whose squared distances differ by less than ~1e-9 m^2 may resolve
// to the lower slot.  PRECISE adds |p'|^2 to every key before packing (one
// v_pk_add per two slots): the key is then the squared distance itself, the
// quantisation acts on it, and what remains is the fp32 rounding of the key
// (~1e-10 m^2).  The 2-link engine keeps the cheaper form (its parity on the
// reference's fixtures is unaffected, +10 % instructions otherwise); the chain
// engine, whose config-5 start pose sits ON a waypoint, uses PRECISE.
template <int LPS, bool PRECISE = false>
struct Search {
    static constexpr int SL = ((MPPI_SEARCH_LEN + LPS - 1) / LPS + 1) & ~1;  // slots per lane, even
    static constexpr int SP = SL / 2;
    f32x2 krx[SP], kry[SP], kc[SP];
    int sub;
    float cx, cy;

    // key: the centred keys (kSlots float4), ctr: the window centre
    __device__ __forceinline__ void load(const float4* key, float4 ctr, int lane_sub) {
        static_assert(SL * LPS <= kSlots, "window slots");
        if (LPS == 1) {
            // lane-opaque zero: keeps the 30 window slots in VGPRs (as uniform
            // values they would go to SGPRs and spill)
            int z;
            asm volatile("v_mov_b32 %0, 0" : "=v"(z));
            sub = z;
        } else {
            sub = lane_sub;
        }
#pragma unroll
        for (int i = 0; i < SP; ++i) {
            const float4 k0 = key[sub * SL + 2 * i];
            const float4 k1 = key[sub * SL + 2 * i + 1];
            krx[i] = f32x2{k0.x, k1.x};
            kry[i] = f32x2{k0.y, k1.y};
            kc[i] = f32x2{k0.z, k1.z};
        }
        cx = ctr.x;
        cy = ctr.y;
    }

    __device__ __forceinline__ unsigned nearest(float px, float py) const { return nearest_d(px - cx, py - cy); }

    // dx, dy: the position relative to the window centre
    __device__ __forceinline__ unsigned nearest_d(float dx, float dy) const {
        const f32x2 ax2 = {dx, dx}, ay2 = {dy, dy};
        const float pp = fmaf(dx, dx, dy * dy);
        const f32x2 pp2 = {pp, pp};
        float kk[2 * SP];
#pragma unroll
        for (int i = 0; i < SP; ++i) {
            f32x2 key = __builtin_elementwise_fma(ax2, krx[i], __builtin_elementwise_fma(ay2, kry[i], kc[i]));
            if constexpr (PRECISE) key = key + pp2;   // |p - r_j|^2
            // through the opaque sub even at LPS = 1: measured 2.5% faster than a
            // constant index (v_and + v_or3 packing schedules better there; tools/ab.py)
            const unsigned j = (unsigned)(sub * SL + 2 * i);
            const float k0 = __uint_as_float((__float_as_uint(key.x) & ~31u) | j);
            const float k1 = __uint_as_float((__float_as_uint(key.y) & ~31u) | (j + 1));
            kk[2 * i] = k0;
            kk[2 * i + 1] = k1;
        }
        // the same v_min3 count as a running minimum, but 4 levels deep instead of
        // 15 (the keys carry distinct indices, so the order of the minima is free)
        float best = min_tree<2 * SP>(kk);
        if (LPS >= 2) best = min_raw(best, dpp_f32<0xB1>(best));  // quad_perm xor 1
        if (LPS >= 4) best = min_raw(best, dpp_f32<0x4E>(best));  // quad_perm xor 2
        if (LPS >= 8) best = min_raw(best, dpp_f32<0x141>(best));  // row_half_mirror: the other quad of 8
        if (LPS >= 16) best = min_raw(best, dpp_f32<0x128>(best));  // row_ror:8: the other half of the row
        return __float_as_uint(best) & 31u;
    }
};

// The same search with the window keys in LDS instead of registers: the keys
// are uniform across the workgroup, so every read is a broadcast ds_read_b128
// (two per two slots: {rx'0, rx'1, ry'0, ry'1}, {c'0, c'1, -, -}).  Costs one
// LDS read per slot and per step, frees the 3 x 30 key registers — for kernels
// whose per-lane state is large (the n-link chain) that buys occupancy.
struct alignas(16) KeyPair {
    float4 xy;   // -2 rx'(2i), -2 rx'(2i+1), -2 ry'(2i), -2 ry'(2i+1)
    float4 c;    // c'(2i), c'(2i+1), 0, 0
};
constexpr int kKeyPairs = kSlots / 2;

template <bool PRECISE = false>
struct SearchLDS {
    const KeyPair* kp;   // LDS, kKeyPairs entries
    float cx, cy;

    // cooperative fill by the first kKeyPairs threads; a barrier must follow
    __device__ __forceinline__ static void fill(KeyPair* dst, const float4* key, int tid) {
        if (tid < kKeyPairs) {
            const float4 k0 = key[2 * tid], k1 = key[2 * tid + 1];
            dst[tid].xy = make_float4(k0.x, k1.x, k0.y, k1.y);
            dst[tid].c = make_float4(k0.z, k1.z, 0.f, 0.f);
        }
    }

    __device__ __forceinline__ unsigned nearest(float px, float py) const {
        const float dx = px - cx, dy = py - cy;
        const f32x2 ax2 = {dx, dx}, ay2 = {dy, dy};
        const float pp = fmaf(dx, dx, dy * dy);
        const f32x2 pp2 = {pp, pp};
        float best = 3.0e38f;
        constexpr int SP = (MPPI_SEARCH_LEN + 1) / 2;
#pragma unroll
        for (int i = 0; i < SP; ++i) {
            const float4 xy = kp[i].xy, cc = kp[i].c;
            f32x2 key = __builtin_elementwise_fma(ax2, f32x2{xy.x, xy.y},
                                                  __builtin_elementwise_fma(ay2, f32x2{xy.z, xy.w}, f32x2{cc.x, cc.y}));
            if constexpr (PRECISE) key = key + pp2;   // |p - r_j|^2
            const unsigned j = (unsigned)(2 * i);
            const float k0 = __uint_as_float((__float_as_uint(key.x) & ~31u) | j);
            const float k1 = __uint_as_float((__float_as_uint(key.y) & ~31u) | (j + 1));
            best = min3_raw(best, k0, k1);
        }
        return __float_as_uint(best) & 31u;
    }
};

// Epilogue gather of one noise column for the workgroup's listed samples:
// sum_l w_l eps[k_l] in ascending l (fp64 fma), the NL loads of the column
// issued together.  NL is a compile-time bucket >= nl, so a workgroup with one
// weighted sample issues one load per column, not kSparseMax.
template <int NL>
__device__ __forceinline__ double gather_col_n(const float* base, int kstride, const int* s_k, const double* s_e,
                                               int nl) {
    float e[NL];
#pragma unroll
    for (int l = 0; l < NL; ++l) e[l] = base[(size_t)(nl > 0 ? s_k[min(l, nl - 1)] : 0) * kstride];
    double acc = 0.0;
#pragma unroll
    for (int l = 0; l < NL; ++l)
        if (l < nl) acc = fma(s_e[l], (double)e[l], acc);
    return acc;
}
// nl: wave-uniform, <= kSparseMax
__device__ __forceinline__ double gather_col(const float* base, int kstride, const int* s_k, const double* s_e,
                                             int nl) {
    static_assert(kSparseMax == 16, "buckets");
    if (nl <= 1) return gather_col_n<1>(base, kstride, s_k, s_e, nl);
    if (nl <= 2) return gather_col_n<2>(base, kstride, s_k, s_e, nl);
    if (nl <= 4) return gather_col_n<4>(base, kstride, s_k, s_e, nl);
    if (nl <= 8) return gather_col_n<8>(base, kstride, s_k, s_e, nl);
    return gather_col_n<16>(base, kstride, s_k, s_e, nl);
}

// stage / terminal cost terms (control.py:185-198, weights x 10000 folded in)
__device__ __forceinline__ float weighted_sq(float ex, float ey, float e1, float e2, const float* w) {
    return fmaf(w[0], ex * ex, fmaf(w[1], ey * ey, fmaf(w[2], e1 * e1, w[3] * e2 * e2)));
}

// ------------------------------------------------------- the rollout epilogue
// Both rollout kernels (rollout_kernel, chain_rollout_kernel) end the same way: the samples' costs S become
// the workgroup's partial row {rho_b, eta_b, N_b} (control.py:112-118 over the workgroup), which travels
// through the two-level hand-off merge.  The stages below are that common text; the LDS arrays are the
// kernels' own (declared there, so each kernel keeps its layout), and so are the barriers between the stages,
// the publishing of rho_b and eta_b, the chain's running minimum and the gathers' row loads, which differ.

// A lane's soft-min weight relative to the workgroup minimum, and its wave's ballot of the weights kept.
struct LaneWeight {
    double wgt;
    bool nz;
    unsigned long long bal;
};

// Weights exp((rho_b - S) / lambda) in fp64, like the reference's; those below 2^-64 of the workgroup's
// best are dropped (see kMergeFloor), and a wave whose samples all lie below the floor (exp(-44.4) = 2^-64:
// the usual case, S spread >> lambda) skips the exp.  Leaves each wave's count and sum of kept weights in
// s_cnt / s_redd; the caller's barrier comes before block_compact.  lane, wave: the thread's, passed as the
// kernel's own values (recomputed here they cost every instance two or three instructions).
__device__ __forceinline__ LaneWeight block_weigh(bool owner, double S, double rho_b, double inv_lambda, int lane,
                                                  int wave, int* s_cnt, double* s_redd) {
    const double warg = (rho_b - S) * inv_lambda;
    double wgt = 0.0;
    if (__any(owner && warg >= -45.0)) wgt = owner ? exp(warg) : 0.0;
    const bool nz = wgt >= kMergeFloor;
    const unsigned long long bal = __ballot(nz);
    const double esum = wave_sum_f64(nz ? wgt : 0.0);
    if (lane == 0) {
        s_cnt[wave] = __popcll(bal);
        s_redd[wave] = esum;
    }
    return LaneWeight{wgt, nz, bal};
}

// The kept samples (index k, weight) in thread order into s_k / s_e; returns their number and sets eta_b,
// the sum of their weights in wave order.  The caller's barrier comes before s_k / s_e are read.
template <int NT>
__device__ __forceinline__ int block_compact(const LaneWeight& lw, int k, int wave, const int* s_cnt,
                                             const double* s_redd, int* s_k, double* s_e, double* eta_b) {
    int off = 0, nl = 0;
    double eta = 0.0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) {
        off += (w < wave) ? s_cnt[w] : 0;
        nl += s_cnt[w];
        eta += s_redd[w];
    }
    if (lw.nz) {
        const int pos = off + lanes_below(lw.bal);
        s_k[pos] = k;
        s_e[pos] = lw.wgt;
    }
    *eta_b = eta;
    return nl;
}

// Dense weights (more than kSparseMax kept samples): the weight of the workgroup's sample ks in s_e[ks]
// (0 where dropped), then lane l's samples l, l + 64, ... in w (0 past K).  Each wave then takes whole
// noise rows, coalesced, and reduces them with DPP (the kernels' own loops: their noise layouts differ).
template <int NT, int NS>
__device__ __forceinline__ void dense_weights(const LaneWeight& lw, int k, int K, double* s_e,
                                              double (&w)[(NS + 63) / 64]) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int k0 = blockIdx.x * NS;
    if (tid < NS) s_e[tid] = 0.0;
    __syncthreads();
    if (lw.nz) s_e[k - k0] = lw.wgt;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < (NS + 63) / 64; ++i) {
        const int ks = lane + 64 * i;
        w[i] = (ks < NS && k0 + ks < K) ? s_e[ks] : 0.0;
    }
}

// Upper median of 10 (rank 5): a 29-comparator sorting network (verified on all
// 2^10 0/1 inputs), the element scipy.ndimage.median_filter(size=10) returns.
__device__ __forceinline__ double median10(double* v) {
#define CX(i, j) { const double lo = min_raw_f64(v[i], v[j]), hi = max_raw_f64(v[i], v[j]); v[i] = lo; v[j] = hi; }
    CX(4, 9) CX(3, 8) CX(2, 7) CX(1, 6) CX(0, 5) CX(1, 4) CX(6, 9) CX(0, 3) CX(5, 8) CX(0, 2)
    CX(3, 6) CX(7, 9) CX(0, 1) CX(2, 4) CX(5, 7) CX(8, 9) CX(1, 2) CX(4, 6) CX(7, 8) CX(3, 5)
    CX(2, 5) CX(6, 8) CX(1, 3) CX(4, 7) CX(2, 3) CX(6, 7) CX(3, 4) CX(5, 6) CX(4, 5)
#undef CX
    return v[5];
}

// scipy.ndimage.median_filter(size=10, mode='reflect') of column d of the
// T x du array sm.weps at row t (control.py:319-327, window [t-5, t+4]; one
// reflection suffices for T >= 5).
template <class SM>
__device__ __forceinline__ double median_at(const SM& sm, int t, int d, int T, int du) {
    double v[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        int m = t - 5 + i;
        m = m < 0 ? -m - 1 : m;
        m = m >= T ? 2 * T - 1 - m : m;
        v[i] = sm.weps[m * du + d];
    }
    return median10(v);
}

// ------------------------------------------------------------------ Philox

// Philox4x32-10 (Salmon et al., SC'11).  Each round's two 32 x 32 -> 64-bit
// products are one v_mad_u64_u32 apiece (the 64-bit product of zero-extended
// words, which the compiler emits as one), not a v_mul_lo_u32 + v_mul_hi_u32
// pair: half the quarter-rate multiplies.  The round's two three-way XORs
// (hi ^ word ^ key) are one v_bitop3_b32 each (truth table 0x96), the key word
// from an SGPR (it must be wave-uniform: the "s" constraint takes lane 0's
// value).  With the hardware Box-Muller below: 13.4 -> 8.35 us for config 3's
// draw (profiles/r11/philox_ab.txt).
__device__ __forceinline__ unsigned long long mul_wide(unsigned a, unsigned m) {
    return (unsigned long long)a * m;
}
__device__ __forceinline__ unsigned xor3(unsigned a, unsigned b, unsigned k) {
    unsigned r;
    asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x96" : "=v"(r) : "v"(a), "v"(b), "s"(k));
    return r;
}
__device__ __forceinline__ uint4 philox4x32_10(uint4 ctr, uint2 key) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = mul_wide(ctr.x, 0xD2511F53u);
        const unsigned long long p1 = mul_wide(ctr.z, 0xCD9E8D57u);
        ctr = make_uint4(xor3((unsigned)(p1 >> 32), ctr.y, key.x), (unsigned)p1,
                         xor3((unsigned)(p0 >> 32), ctr.w, key.y), (unsigned)p0);
        key.x += 0x9E3779B9u;
        key.y += 0xBB67AE85u;
    }
    return ctr;
}

// Two standard normals from two 32-bit uniforms (Box-Muller) on the hardware
// transcendentals: v_log_f32 (log2), v_sqrt_f32, and v_sin_f32 / v_cos_f32, whose
// input is in revolutions — exactly u1, so no 2 pi scaling and no range
// reduction.  Returned WITHOUT the constant sqrt(2 ln 2) (kBoxMullerScale): the
// callers fold it into their Cholesky factor, so the value is
//   sqrt(-log2 u0) (cos 2 pi u1, sin 2 pi u1) = z / sqrt(2 ln 2).
// u0 = (a + 1) 2^-32 in [2^-32, 1] (a normal float: no denormal path) is one fma:
// scaling by 2^-32 is exact, so fma(a, 2^-32, 2^-32) rounds the same real as
// (float(a) + 1) * 2^-32, and it never exceeds 1 (float(a) <= 2^32, and 2^32 + 1
// rounds to 2^32), so no clamp.  The negation of log2 u0 <= 0 is a source modifier.
constexpr double kBoxMullerScale = 1.1774100225154747;   // sqrt(2 ln 2)
__device__ __forceinline__ float2 box_muller(unsigned a, unsigned b) {
    const float inv = 2.3283064365386963e-10f;  // 2^-32
    const float u0 = fmaf((float)a, inv, inv), u1 = (float)b * inv;
    const float r = __builtin_amdgcn_sqrtf(-__builtin_amdgcn_logf(u0));
    return make_float2(r * __builtin_amdgcn_cosf(u1), r * __builtin_amdgcn_sinf(u1));
}

// Issue fairness between workgroups that share a CU.  The SIMD arbiter serves
// the oldest ready wave first, so of two co-resident rollout waves the younger
// one only fills the older one's issue gaps and then finishes alone at the
// single-wave rate (measured on the chain kernel: older workgroups 174 us,
// younger 277 us).  Each workgroup draws a per-CU ticket with one relaxed
// atomic (co-resident workgroups draw consecutive tickets: different
// parities), and waves raise their priority in alternate real-time phases of
// 2^kPrioShift ticks (100 MHz: ~41 us), the phase flipped by the ticket parity.
// Priority steers scheduling only; no result depends on it.
constexpr int kCuSlots = 2048;   // (XCC, SE, SH, CU) keys
constexpr int kPrioShift = 12;
__device__ __forceinline__ unsigned cu_key() {
    const unsigned hw = __builtin_amdgcn_s_getreg(0xF804);    // HW_ID
    const unsigned xcc = __builtin_amdgcn_s_getreg(0xF814);   // XCC_ID
    return ((xcc & 7u) << 8) | (((hw >> 13) & 7u) << 5) | (((hw >> 12) & 1u) << 4) | ((hw >> 8) & 0xFu);
}
// Thread 0 draws the ticket into *s_parity (read after the caller's next barrier).
__device__ __forceinline__ void draw_cu_ticket(unsigned* cu_ctr, unsigned* s_parity) {
    if (threadIdx.x == 0)
        *s_parity = __hip_atomic_fetch_add(cu_ctr + cu_key(), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 1u;
}
__device__ __forceinline__ void fair_priority(unsigned parity) {
    if ((((unsigned)__builtin_amdgcn_s_memrealtime() >> kPrioShift) & 1u) ^ parity)
        __builtin_amdgcn_s_setprio(1);
    else
        __builtin_amdgcn_s_setprio(0);
}

// ---- workspace obstacles: what the arm's and the chain's collision tests share (mppi_set_obstacles,
// mppi_chain_set_obstacles).  The discs of a launch as the test reads them: in LDS, two discs per 32-byte record
// (cx, cx', cy, cy', r2, r2', 0, 0), read back with uniform addresses (a broadcast).  Scalar registers would be the
// natural home of wave-uniform values, but the rollout kernels have none to spare (they spill ~90 already, into
// VGPR lanes), and an LDS read takes no VALU issue slot where a v_readlane per operand does.
constexpr int kObstPairs = MPPI_MAX_OBSTACLES / 2;
struct ObstR {
    const float4* rec;   // [2 * kObstPairs] in LDS
    int n;               // scalar
};
struct DiscPair {
    f32x2 cX, cY, r2;
};
// One thread writes the records (constant kernel-argument offsets: a run-time index into the by-value struct would
// send it through a private copy); the caller's barrier publishes them.  OB: the kernel's by-value disc argument
// (fp32 cx, cy, r2 of MPPI_MAX_OBSTACLES entries).
template <class OB>
__device__ __forceinline__ void stage_obst(float4* rec, const OB& ob) {
#pragma unroll
    for (int p = 0; p < kObstPairs; ++p) {
        rec[2 * p] = make_float4(ob.cx[2 * p], ob.cx[2 * p + 1], ob.cy[2 * p], ob.cy[2 * p + 1]);
        rec[2 * p + 1] = make_float4(ob.r2[2 * p], ob.r2[2 * p + 1], 0.f, 0.f);
    }
}
// Moving discs (mppi_set_moving_obstacles): one row of records per rollout step, kObstRow float4 each, so the
// horizon loop reads step t's discs at an address that walks with the step and gains no arithmetic.  The calling
// thread writes step t's kObstRow records to rec: the centres at the time of the state that step produces, c + v tau
// with tau the fp32 rounding of the fp64 (t + 1) dt, one explicit fma per coordinate (so a rollout and its debug
// kernel agree); at rest (v = 0) the fma returns c, and every row is the row stage_obst writes.  OB: as stage_obst,
// with vx, vy and the fp64 dt.
constexpr int kObstRow = 2 * kObstPairs;
template <class OB>
__device__ __forceinline__ void stage_obst_row(float4* rec, const OB& ob, int t) {
    const float tau = (float)((double)(t + 1) * ob.dt);
#pragma unroll
    for (int p = 0; p < kObstPairs; ++p) {
        rec[2 * p] = make_float4(__builtin_fmaf(ob.vx[2 * p], tau, ob.cx[2 * p]),
                                 __builtin_fmaf(ob.vx[2 * p + 1], tau, ob.cx[2 * p + 1]),
                                 __builtin_fmaf(ob.vy[2 * p], tau, ob.cy[2 * p]),
                                 __builtin_fmaf(ob.vy[2 * p + 1], tau, ob.cy[2 * p + 1]));
        rec[2 * p + 1] = make_float4(ob.r2[2 * p], ob.r2[2 * p + 1], 0.f, 0.f);
    }
}
__device__ __forceinline__ DiscPair load_pair(const ObstR& o, int p) {
    const float4 a = o.rec[2 * p], b = o.rec[2 * p + 1];
    return DiscPair{f32x2{a.x, a.y}, f32x2{a.z, a.w}, f32x2{b.x, b.y}};
}

// Does a link touch a disc: two discs (the halves of pX, pY, r2) against the segment from the origin of
// (pX, pY) — the disc centres relative to the link's base — along the unit direction cs = (cos, sin), length L.
// The well-conditioned form: project the centre on the direction, clip the parameter to [0, L] with one
// v_med3_f32 (0 <= L), subtract the foot point and square the offset; nothing cancels at the magnitude of the
// centre.  Five roundings on the way to d (two in s, one in each offset component, two in the sum of their
// squares), each at magnitude <= |centre| + L.  Every product-sum is an explicit fma, so a rollout and its debug
// kernel (mppi_debug_obstacle_hits, mppi_chain_debug_obstacle_hits) evaluate the same operations whatever the
// compiler would contract.
__device__ __forceinline__ void seg_hits(f32x2 pX, f32x2 pY, f32x2 cs, float L, f32x2 r2, bool& ha, bool& hb) {
    const f32x2 s = __builtin_elementwise_fma(pY, f32x2{cs.y, cs.y}, pX * f32x2{cs.x, cs.x});
    const f32x2 t = {__builtin_amdgcn_fmed3f(s.x, 0.f, L), __builtin_amdgcn_fmed3f(s.y, 0.f, L)};
    const f32x2 oX = __builtin_elementwise_fma(-t, f32x2{cs.x, cs.x}, pX);
    const f32x2 oY = __builtin_elementwise_fma(-t, f32x2{cs.y, cs.y}, pY);
    const f32x2 d = __builtin_elementwise_fma(oY, oY, oX * oX);
    ha = d.x < r2.x;
    hb = d.y < r2.y;
}

}  // namespace mppi

#include "mppi_merge.h"
