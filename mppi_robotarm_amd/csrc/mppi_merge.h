// mppi_merge.h — the partial rows {rho, eta, N[nval]} handed between workgroups (control.py:112-118 over some set
// of samples in log-sum-exp form: rho = min S, eta = sum e^{-(S - rho)/lambda}, N = sum e^{-(S - rho)/lambda} eps;
// nval = T * du values) and their merges: row buffers and tagged granules, merge_rows_block, direct_merge,
// handoff_merge, deferred_merge and the node-level exchange.  Included at the end of mppi_device.h.
#pragma once

namespace mppi {

// ------------------------------------------------ rows handed between workgroups

// Rows {rho, eta, N} handed between workgroups of one launch travel write-through: every store and every load of
// them is a `sc1` buffer access (MI355X guide G16, "Valid forms" row 1), so neither side needs an agent-scope fence
// (~1.7 us each): 8-B words behind an arrival counter, or 16-B tagged granules polled without any counter.
typedef unsigned int u32x2 __attribute__((__vector_size__(2 * sizeof(unsigned int))));
typedef unsigned int u32x4 __attribute__((__vector_size__(4 * sizeof(unsigned int))));
constexpr int kSC1 = 16;  // buffer aux bit: sc1

__device__ __forceinline__ __amdgpu_buffer_rsrc_t rows_rsrc(const void* p, int bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, 0x00020000);
}
__device__ __forceinline__ double ld_wt(__amdgpu_buffer_rsrc_t r, int idx) {
    return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, idx * 8, 0, kSC1));
}
// A row value of the PREVIOUS launch (the deferred finish): visible since the kernel boundary, so an ordinary
// cached load; the workgroups of an XCD, which all read the same rows, share its L2 lines.
__device__ __forceinline__ double ld_prev(__amdgpu_buffer_rsrc_t r, int idx) {
    return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, idx * 8, 0, 0));
}
__device__ __forceinline__ void st_wt(__amdgpu_buffer_rsrc_t r, int idx, double v) {
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), r, idx * 8, 0, kSC1);
}
// Element index past every rows buffer: a raw buffer load beyond num_records
// returns 0 without a memory access, so a predicated-off load needs no branch
// (a branch around each load makes the compiler wait for it at the join).
constexpr int kOffRange = 1 << 26;  // x 16 B = 1 GiB > any rows buffer, no int overflow

// Tagged granules (MI355X guide, Guideline 16 R2: "the data IS the flag").  One fp64 value travels as {lo32, tag,
// hi32, tag} in ONE 16-B sc1 store; each 8-B half is a naturally aligned {value, tag} granule, so a reader that sees
// both tags equal to this launch's epoch holds the whole value — no drain, no flag, no counter.  Tags come from a
// device-resident epoch (never a kernel argument: graph replay freezes those), zeroed once at context creation.
__device__ __forceinline__ void st_gran(__amdgpu_buffer_rsrc_t r, int idx, double v, unsigned tag) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const u32x4 x = {(unsigned)b, tag, (unsigned)(b >> 32), tag};
    __builtin_amdgcn_raw_buffer_store_b128(x, r, idx * 16, 0, kSC1);
}
// Poll loads are plain sc1 loads; every spin loop opens with an empty asm memory clobber so the loads are re-issued
// each pass (without it LLVM hoists the read-only loads out of the loop — nothing else in it writes memory — and
// polls registers).
__device__ __forceinline__ u32x4 ld_gran(__amdgpu_buffer_rsrc_t r, int idx) {
    return __builtin_amdgcn_raw_buffer_load_b128(r, idx * 16, 0, kSC1);
}
__device__ __forceinline__ bool gran_ok(u32x4 x, unsigned tag) { return x[1] == tag && x[3] == tag; }
__device__ __forceinline__ double gran_val(u32x4 x) {
    return __longlong_as_double((long long)(((unsigned long long)x[2] << 32) | x[0]));
}
// Bounded spins: ~1 s of polling, then the hand-off reports a timeout (host
// error word) instead of hanging the GPU; results of that launch are invalid.
constexpr unsigned kSpinMax = 1u << 20;
// The host-mapped timeout words: tmo[0] = kTmoLocal (a hand-off of this launch gave up), tmo[1] = the
// exchange's verdict bits (kTmoExchange, kTmoSplit below).  Separate words, plain stores (no read-modify-write
// over the host link), so the exchange's verdict never overwrites a local cause; the host ORs them.
__device__ __forceinline__ void report_timeout(unsigned* tmo) {
    if (tmo) __hip_atomic_store(tmo, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
#define MPPI_SPIN_OR_GIVE_UP(spins, tmo, lane) MPPI_SPIN_OR_GIVE_UP_L(spins, 0ull, tmo, lane, (void)0)
// with a deadline of its own (s_memrealtime ticks, 100 MHz; 0: the spin bound alone) and a statement run
// when it gives up (the exchange's polls)
#define MPPI_SPIN_OR_GIVE_UP_L(spins, deadline, tmo, lane, on_give_up)                                   \
    if (spins >= kSpinMax || ((deadline) && __builtin_amdgcn_s_memrealtime() > (deadline))) {            \
        if ((lane) == 0) report_timeout(tmo);                                                            \
        on_give_up;                                                                                      \
        break;                                                                                           \
    }                                                                                                    \
    __builtin_amdgcn_s_sleep(1)

// How a merge reads its rows: this launch's polled tagged granules (16-B sc1 loads), this launch's write-through
// rows behind an arrival counter (8-B sc1 loads), or the previous launch's rows (the deferred finish: 8-B cached).
enum class RowsVia { Gran, Wt, Prev };

// Order-preserving 64-bit key of a double (unsigned order == numeric order; NaN
// above +inf) for integer atomic min / max, and its inverse.
__device__ __forceinline__ unsigned long long ord_key(double x) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | (1ull << 63));
}
__device__ __forceinline__ double ord_val(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & ~(1ull << 63)) : ~k));
}

// ------------------------------------------------------------ merge scratch

template <int MAXV>
struct MergeScratch {
    double red[kMaxWaves];
    double weps[MAXV];
    double unew[MAXV];
    double rho[kDirectRows];  // direct merge: the rows' rho, polled by wave 0
    double part[2 * kDirectRows];  // direct merge: per row-group column sums (one group per ncol threads)
    double eta;                    // the final merge's eta = sum_k e^{-(S_k - rho)/lambda} (>= 1; 1: one-hot)
    double rho_fin;                // the final merge's rho
    int nrel;
};

// Workgroup minimum.  One use per kernel: the caller's next barrier protects
// sm.red before any reuse.
template <int NT, class SM>
__device__ __forceinline__ double block_min_f64(double v, SM& sm) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    v = wave_min_f64(v);
    if (lane == 0) sm.red[wave] = v;
    __syncthreads();
    double r = sm.red[0];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) r = min_raw_f64(r, sm.red[w]);
    return r;
}

// Geometry of a partial row {rho, eta, N[nval]}: stride values, merged columns
// (col 0 = eta, 1 + j = N[j]).  Thread tid owns columns tid + ch * NT, ch < MAXCH.
struct RowGeo {
    int stride, ncol;
    __device__ explicit RowGeo(int nval) : stride(2 + nval), ncol(1 + nval) {}
};

// Final merged row: {rho, eta, N} to out_row (plain, read after the launch) and
// w_eps = N / eta (control.py:112-118) to sm.weps and w_eps_out.
template <int NT, int MAXCH, class SM>
__device__ __forceinline__ void put_final(double rho, const double (&acc)[MAXCH], double eta, int nrel,
                                          const RowGeo& geo, SM& sm, double* out_row, double* w_eps_out) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int ch = 0; ch < MAXCH; ++ch) {
        const int col = tid + ch * NT;
        if (col >= geo.ncol) continue;
        if (col == 0) {
            sm.nrel = nrel;
            sm.eta = eta;
            sm.rho_fin = rho;
            if (out_row) {
                out_row[0] = rho;
                out_row[1] = acc[ch];
            }
        } else {
            if (out_row) out_row[1 + col] = acc[ch];
            const double w = acc[ch] / eta;
            sm.weps[col - 1] = w;
            if (w_eps_out) w_eps_out[col - 1] = w;
        }
    }
    __syncthreads();
}

// Merge n rows (read write-through from `rows`, rows row0 .. row0 + n - 1) with
// a log-sum-exp rescale: rho = min rho_i, s_i = exp((rho - rho_i) / lambda),
// eta = sum s_i eta_i, N = sum s_i N_i, in ascending row order (deterministic);
// rows whose factor is below 2^-64 of the running best are skipped.  Rows go in
// rounds with an online rescale of the running sums when a round lowers rho.
// Wave-local: every wave reads the round's rho_i into its lanes, reduces them
// with DPP and evaluates the s_i itself; the s_i reach the column FMAs as
// scalars (v_readlane) — no LDS traffic and no barrier per round.
//
// RowsVia::Wt: 8-B sc1 words behind an arrival counter.  With one column chunk
//   (MAXCH = 1) every load of a round — rho, eta and all entries of 32 rows —
//   is issued together (one memory round trip per round); with more chunks the
//   rounds are structured exactly as Gran's (below) with plain sc1 loads, so
//   both hand-off forms rescale and accumulate identically (same bits).
// RowsVia::Gran: 16-B tagged granules polled until every tag matches `tag`: rho first,
//   one lane per row (16 rows per round), then eta and the entries of only the
//   rows that carry weight, 16 / MAXCH rows per load batch.
// The merged row goes to out_wt (same format, next level) or, with `final`,
// to put_final.
template <int NT, int MAXCH, bool final, RowsVia VIA, class SM>
__device__ __forceinline__ void merge_rows_block(__amdgpu_buffer_rsrc_t rows, int row0, int n, const RowGeo& geo,
                                                 double inv_lambda, SM& sm, const __amdgpu_buffer_rsrc_t* out_wt,
                                                 int out_idx, double* out_row, double* w_eps_out, unsigned tag,
                                                 unsigned* tmo, unsigned long long deadline = 0ull,
                                                 bool* failed = nullptr) {
    // deadline / failed: the polls' deadline (s_memrealtime; 0: the spin bound alone), and (when given) whether
    // any poll of the workgroup gave up (uniform).
    constexpr bool GRAN = VIA == RowsVia::Gran;
    constexpr bool EAGER = !GRAN && MAXCH == 1;  // one round trip per round of 32 rows
    constexpr int LB = EAGER ? 32 : 16;         // loads per batch per thread
    constexpr int RB = LB / MAXCH;              // rows per load batch
    constexpr int R1 = EAGER ? 32 : 16;         // rows per round
    static_assert(RB >= 1 && R1 <= 64, "one row per lane");
    const int tid = threadIdx.x, lane = tid & 63;
    const int stride = geo.stride, ncol = geo.ncol;
    double acc[MAXCH], eta = 0.0, rho = INFINITY;
#pragma unroll
    for (int ch = 0; ch < MAXCH; ++ch) acc[ch] = 0.0;
    int nrel = 0;
    bool gave_up = false;
    for (int r0 = 0; r0 < n; r0 += R1) {
        const int nr = min(R1, n - r0);   // uniform
        const int rb = row0 + r0;
        const int lrow = lane < nr ? (rb + lane) * stride : kOffRange;
        double rho_r, eta_l = 0.0, v[EAGER ? LB : 1];
        if constexpr (GRAN) {
            u32x4 gr;
            for (unsigned spins = 0;; ++spins) {
                asm volatile("" ::: "memory");
                gr = ld_gran(rows, lrow);
                if (__all(lane >= nr || gran_ok(gr, tag))) break;
                MPPI_SPIN_OR_GIVE_UP_L(spins, deadline, tmo, lane, gave_up = true);
            }
            rho_r = gran_val(gr);
        } else if constexpr (!EAGER) {
            rho_r = ld_wt(rows, lrow);
        } else {
            rho_r = ld_wt(rows, lrow);
            eta_l = ld_wt(rows, lrow + 1);
#pragma unroll
            for (int j = 0; j < LB; ++j) {
                const int i = j / MAXCH, col = tid + (j % MAXCH) * NT;
                v[j] = ld_wt(rows, (i < nr && col < ncol) ? (rb + i) * stride + 1 + col : kOffRange);
            }
        }
        const double rho_l = lane < nr ? rho_r : INFINITY;
        const double rnew = min_raw_f64(rho, wave_min_f64(rho_l));
        double s_l = 0.0;
        if (lane < nr) {
            const double s = exp((rnew - rho_l) * inv_lambda);
            s_l = s >= kMergeFloor ? s : 0.0;
        }
        const unsigned long long rel = __ballot(s_l != 0.0);   // rows that carry weight (uniform)
        const int nrr = __popcll(rel);
        nrel += nrr;
        if (rnew < rho && rho != INFINITY) {  // uniform: rescale the running sums to the new minimum
            const double f = exp((rnew - rho) * inv_lambda);
#pragma unroll
            for (int ch = 0; ch < MAXCH; ++ch) acc[ch] *= f;
            eta *= f;
        }
        rho = rnew;
        if constexpr (EAGER) {
#pragma unroll
            for (int j = 0; j < LB; ++j) {
                const int i = j / MAXCH, ch = j % MAXCH;
                if (i < nr) {
                    const double s = readlane_f64(s_l, i);
                    if (s != 0.0) {
                        acc[ch] = fma(s, v[j], acc[ch]);
                        if (ch == 0) eta = fma(s, readlane_f64(eta_l, i), eta);
                    }
                }
            }
        } else {
            // lane k < nrr: the round's k-th weighted row (ascending)
            const int krow = lane < nrr ? select_bit(rel, lane) : 0;
            for (int b0 = 0; b0 < nrr; b0 += RB) {
                const bool eta_on = b0 == 0 && lane < nrr;
                const int eidx = eta_on ? (rb + krow) * stride + 1 : kOffRange;
                double x[LB];
                if constexpr (GRAN) {
                    u32x4 ge, gv[LB];
                    for (unsigned spins = 0;; ++spins) {
                        asm volatile("" ::: "memory");
                        ge = ld_gran(rows, eidx);
                        bool ok = !eta_on || gran_ok(ge, tag);
#pragma unroll
                        for (int j = 0; j < LB; ++j) {
                            const int i = b0 + j / MAXCH, col = tid + (j % MAXCH) * NT;
                            const bool on = i < nrr && col < ncol;
                            gv[j] = ld_gran(rows, on ? (rb + __builtin_amdgcn_readlane(krow, i)) * stride + 1 + col
                                                     : kOffRange);
                            ok = ok && (!on || gran_ok(gv[j], tag));
                        }
                        if (__all(ok)) break;
                        MPPI_SPIN_OR_GIVE_UP_L(spins, deadline, tmo, lane, gave_up = true);
                    }
                    if (eta_on) eta_l = gran_val(ge);
#pragma unroll
                    for (int j = 0; j < LB; ++j) x[j] = gran_val(gv[j]);
                } else {
                    if (b0 == 0) eta_l = ld_wt(rows, eidx);
#pragma unroll
                    for (int j = 0; j < LB; ++j) {
                        const int i = b0 + j / MAXCH, col = tid + (j % MAXCH) * NT;
                        x[j] = ld_wt(rows, (i < nrr && col < ncol)
                                               ? (rb + __builtin_amdgcn_readlane(krow, i)) * stride + 1 + col
                                               : kOffRange);
                    }
                }
#pragma unroll
                for (int j = 0; j < LB; ++j) {
                    const int i = b0 + j / MAXCH, ch = j % MAXCH;
                    if (i < nrr) {
                        const double s = readlane_f64(s_l, __builtin_amdgcn_readlane(krow, i));
                        acc[ch] = fma(s, x[j], acc[ch]);
                        if (ch == 0) eta = fma(s, readlane_f64(eta_l, i), eta);
                    }
                }
            }
        }
    }
    if (failed) *failed = __syncthreads_or(gave_up);
    if constexpr (final) {
        put_final<NT, MAXCH>(rho, acc, eta, nrel, geo, sm, out_row, w_eps_out);
    } else {
        auto put = [&](int col, double x) {  // col 0 = rho, 1 = eta, 2 + j = N[j]
            if constexpr (GRAN) st_gran(*out_wt, out_idx * stride + col, x, tag);
            else st_wt(*out_wt, out_idx * stride + col, x);
        };
#pragma unroll
        for (int ch = 0; ch < MAXCH; ++ch) {
            const int col = tid + ch * NT;
            if (col >= ncol) continue;
            if (col == 0) put(0, rho);
            put(1 + col, acc[ch]);
        }
    }
}

// Single-level finish for the usual regime (few weighted rows, S spread >> lambda):
// read rho of EVERY workgroup row (n <= kDirectRows), and when at most
// kDirectMax rows carry weight relative to the global minimum, merge exactly
// those rows in ascending order straight from the workgroup slab — one hand-off
// on the critical path instead of two.  Returns false (uniformly) when more rows
// carry weight; the caller then merges through the group rows.  Wave-local
// like merge_rows_block; the result goes out as in a final merge.
// RowsVia::Prev: the caller has loaded the rows' rho already (rho_pre: row lane + 64 j in slot j, INFINITY past n).
template <int NT, int MAXCH, RowsVia VIA, class SM>
__device__ __forceinline__ bool direct_merge(__amdgpu_buffer_rsrc_t rows, int n, const RowGeo& geo,
                                             double inv_lambda, SM& sm, double* out_row, double* w_eps_out,
                                             unsigned tag, unsigned* tmo, unsigned long long* dbg = nullptr,
                                             const double* rho_pre = nullptr) {
    constexpr bool GRAN = VIA == RowsVia::Gran, PRE = VIA == RowsVia::Prev;
    constexpr int P = kDirectRows / 64;
    // the rows of this launch travel write-through (sc1); PRE: the previous launch's, through the caches
    auto ld = [](__amdgpu_buffer_rsrc_t r, int idx) { return PRE ? ld_prev(r, idx) : ld_wt(r, idx); };
    constexpr int LB = 16;                      // loads per batch per thread
    constexpr int RB = LB / MAXCH;              // rows per load batch
    const int tid = threadIdx.x, lane = tid & 63;
    const int stride = geo.stride, ncol = geo.ncol;
    // phase 1: rho of row lane + 64 j in slot j
    double rho_l[P];
    if constexpr (GRAN) {
        // ONE wave polls (a hop's latency sits in the polling CU's memory queue:
        // MI355X guide, polling-cost / handoff-1to1) and hands the values over in LDS
        if (tid < 64) {
            u32x4 gr[P];
            for (unsigned spins = 0;; ++spins) {
                asm volatile("" ::: "memory");
                bool ok = true;
#pragma unroll
                for (int j = 0; j < P; ++j) {
                    const int r = lane + 64 * j;
                    gr[j] = ld_gran(rows, r < n ? r * stride : kOffRange);
                    ok = ok && (r >= n || gran_ok(gr[j], tag));
                }
                if (__all(ok)) break;
                MPPI_SPIN_OR_GIVE_UP(spins, tmo, lane);
            }
#pragma unroll
            for (int j = 0; j < P; ++j) sm.rho[lane + 64 * j] = lane + 64 * j < n ? gran_val(gr[j]) : INFINITY;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < P; ++j) rho_l[j] = sm.rho[lane + 64 * j];
    } else if constexpr (PRE) {
#pragma unroll
        for (int j = 0; j < P; ++j) rho_l[j] = rho_pre[j];
    } else {
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const int r = lane + 64 * j;
            const double x = ld_wt(rows, r < n ? r * stride : kOffRange);
            rho_l[j] = r < n ? x : INFINITY;
        }
    }
    double m = rho_l[0];
#pragma unroll
    for (int j = 1; j < P; ++j) m = min_raw_f64(m, rho_l[j]);
    const double rho = wave_min_f64(m);
    double s_l[P];
    unsigned long long rel[P];
    int nrel = 0;
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const double s = exp((rho - rho_l[j]) * inv_lambda);
        s_l[j] = (lane + 64 * j < n && s >= kMergeFloor) ? s : 0.0;
        rel[j] = __ballot(s_l[j] != 0.0);
        nrel += __popcll(rel[j]);
    }
    // Phase 2 spreads the weighted rows over row groups when the merged columns
    // fill less than the workgroup (one column chunk: G = NT / ncol groups of
    // ncol threads, group g taking every G-th row), so one batch of loads covers
    // kDirectMax * G rows; up to two batches (and 64 rows, one lane each) stay
    // direct.  With one group (config 3's 129 columns) the measured optimum is
    // one batch of 16 rows (the group mergers' overlap wins beyond it).
    const int G = MAXCH == 1 ? max(1, NT / ncol) : 1;
    if (nrel > (G > 1 ? min(64, 2 * kDirectMax * G) : kDirectMax)) return false;
    // lane k < nrel: the k-th weighted row (ascending) and its factor
    int k = lane, row = 0;
    bool found = false;
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const int cnt = __popcll(rel[j]);
        if (!found && k < cnt) {
            row = 64 * j + select_bit(rel[j], k);
            found = true;
        } else if (!found) {
            k -= cnt;
        }
    }
    double sk = 0.0;
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const double sj = __shfl(s_l[j], row & 63);
        if ((row >> 6) == j) sk = sj;
    }
    const bool mine = lane < nrel;
    STAMP(13, NOW());
    // phase 2: eta and the (row, column chunk) entries of the weighted rows
    double acc[MAXCH], eta = 0.0, eta_k = 0.0;
#pragma unroll
    for (int ch = 0; ch < MAXCH; ++ch) acc[ch] = 0.0;
    if (G == 1) {
        // one group: the rows of a batch are wave-uniform (v_readlane); eta as a
        // scalar in the same row order as column 0
        for (int b0 = 0; b0 < nrel; b0 += RB) {
            double v[LB];
            if constexpr (GRAN) {
                const bool eta_on = b0 == 0 && mine;
                u32x4 ge, gv[LB];
                for (unsigned spins = 0;; ++spins) {
                    asm volatile("" ::: "memory");
                    ge = ld_gran(rows, eta_on ? row * stride + 1 : kOffRange);
                    bool ok = !eta_on || gran_ok(ge, tag);
#pragma unroll
                    for (int j = 0; j < LB; ++j) {
                        const int i = b0 + j / MAXCH, col = tid + (j % MAXCH) * NT;
                        const bool on = i < nrel && col < ncol;
                        gv[j] = ld_gran(rows, on ? __builtin_amdgcn_readlane(row, i) * stride + 1 + col : kOffRange);
                        ok = ok && (!on || gran_ok(gv[j], tag));
                    }
                    if (__all(ok)) break;
                    MPPI_SPIN_OR_GIVE_UP(spins, tmo, lane);
                }
                if (eta_on) eta_k = gran_val(ge);
#pragma unroll
                for (int j = 0; j < LB; ++j) v[j] = gran_val(gv[j]);
            } else {
                if (b0 == 0) eta_k = ld(rows, mine ? row * stride + 1 : kOffRange);
#pragma unroll
                for (int j = 0; j < LB; ++j) {
                    const int i = b0 + j / MAXCH, col = tid + (j % MAXCH) * NT;
                    v[j] = ld(rows, (i < nrel && col < ncol) ? __builtin_amdgcn_readlane(row, i) * stride + 1 + col
                                                              : kOffRange);
                }
            }
#pragma unroll
            for (int j = 0; j < LB; ++j) {
                const int i = b0 + j / MAXCH, ch = j % MAXCH;
                if (i < nrel) {
                    const double s = readlane_f64(sk, i);
                    acc[ch] = fma(s, v[j], acc[ch]);
                    if (ch == 0) eta = fma(s, readlane_f64(eta_k, i), eta);
                }
            }
        }
    } else {
        // G groups of ncol threads (one column chunk), group g taking weighted rows
        // g, g + G, ...: the row of a load varies by lane and comes through
        // ds_bpermute, read for every lane before any per-lane test (a cross-lane
        // read returns nothing from a lane the EXEC mask has off)
        const int grp = tid / ncol, gcol = tid - grp * ncol;
        const bool active = grp < G;
        for (int b0 = 0; b0 < nrel; b0 += RB * G) {
            double v[LB], sf[LB];
            int roff[LB];
            bool on[LB];
#pragma unroll
            for (int j = 0; j < LB; ++j) {
                const int i = b0 + grp + G * j;
                on[j] = active && i < nrel;
                const int r = __builtin_amdgcn_ds_bpermute(min(i, 63) << 2, row);
                sf[j] = __shfl(sk, min(i, 63));
                roff[j] = on[j] ? r * stride + 1 + gcol : kOffRange;
            }
            if constexpr (GRAN) {
                u32x4 gv[LB];
                for (unsigned spins = 0;; ++spins) {
                    asm volatile("" ::: "memory");
                    bool ok = true;
#pragma unroll
                    for (int j = 0; j < LB; ++j) {
                        gv[j] = ld_gran(rows, roff[j]);
                        ok = ok && (!on[j] || gran_ok(gv[j], tag));
                    }
                    if (__all(ok)) break;
                    MPPI_SPIN_OR_GIVE_UP(spins, tmo, lane);
                }
#pragma unroll
                for (int j = 0; j < LB; ++j) v[j] = gran_val(gv[j]);
            } else {
#pragma unroll
                for (int j = 0; j < LB; ++j) v[j] = ld(rows, roff[j]);
            }
#pragma unroll
            for (int j = 0; j < LB; ++j)
                if (on[j]) acc[0] = fma(sf[j], v[j], acc[0]);
        }
        // fold the groups' column sums in group order; eta is column 0
        if (active) sm.part[tid] = acc[0];
        __syncthreads();
        if (grp == 0) {
            double a = sm.part[gcol];
            for (int g = 1; g < G; ++g) a += sm.part[g * ncol + gcol];
            acc[0] = a;
            if (tid == 0) sm.red[0] = a;
        }
        __syncthreads();
        eta = sm.red[0];
    }
    STAMP(14, NOW());
    put_final<NT, MAXCH>(rho, acc, eta, nrel, geo, sm, out_row, w_eps_out);
    return true;
}

// Arrive on `counter` after this workgroup's write-through stores; true in
// every thread of the workgroup that arrived last (which re-arms the counter).
// sc1 loads alone stand in for the acquire only at one workgroup per CU (the
// measured form, MI355X guide "Valid forms"); with `acquire` (larger grids)
// the last arriver also runs an agent-scope acquire before the barrier.
__device__ __forceinline__ bool arrive_last(unsigned* counter, unsigned expected, unsigned* s_flag, bool acquire) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave drains its sc1 stores
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned prev = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool last = prev == expected - 1;
        if (last) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (last && acquire) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        *s_flag = last ? 1u : 0u;
    }
    __syncthreads();
    return *s_flag != 0;
}

// The two-level hand-off merge of the nrows workgroup rows in `slab` (group rows in `gslab`).  Returns
// (uniformly) whether this workgroup now holds the final merged row in sm; every other workgroup is done.
// POLL: the rows travel as tagged granules (see st_gran) to consumer workgroups that poll for them — the
//   first workgroup of each group of kGroup merges its group (the first dispatched are the first done, so
//   the merger is waiting when the last row lands), workgroup 0 merges the group rows, or every row directly
//   when few carry weight (direct_merge) — so no workgroup drains its stores or waits on a counter, and the
//   merges overlap the stragglers.  Needs every workgroup resident at once (the host enables it when the
//   grid is at most one workgroup per CU); correctness does not depend on placement or order, every value
//   is tag-checked.  The final merger stores the launch's tag as the new epoch.
// !POLL: the last workgroup of each group to arrive on its counter merges the group, the last group to
//   arrive finishes the step, with the same direct_merge decision (identical results either way).
// direct_dbg: the stamp buffer of direct_merge's own stamps (diagnostic builds; nullptr: none).
template <int NT, int MAXCH, bool POLL, class SM>
__device__ __forceinline__ bool handoff_merge(__amdgpu_buffer_rsrc_t slab_r, __amdgpu_buffer_rsrc_t gslab_r, int nrows,
                                              const RowGeo& geo, double inv_lambda, SM& sm, unsigned* counters,
                                              bool acquire, unsigned* s_flag, double* partial_out, double* w_eps_out,
                                              unsigned tag, unsigned* epoch, unsigned* tmo, unsigned long long* dbg,
                                              unsigned long long* direct_dbg) {
    constexpr RowsVia VIA = POLL ? RowsVia::Gran : RowsVia::Wt;
    const int ngroups = (nrows + kGroup - 1) / kGroup;
    const int g = blockIdx.x / kGroup;
    const int gsz = min(kGroup, nrows - g * kGroup);
    if constexpr (POLL) {
        // ---- level 1: the group's first workgroup polls and merges its rows
        if ((int)blockIdx.x != g * kGroup) return false;
        STAMP(3, NOW());
        if (ngroups == 1) {
            merge_rows_block<NT, MAXCH, true, VIA>(slab_r, 0, gsz, geo, inv_lambda, sm, nullptr, 0, partial_out,
                                                   w_eps_out, tag, tmo);
        } else if (blockIdx.x == 0 && nrows <= kDirectRows &&
                   direct_merge<NT, MAXCH, VIA>(slab_r, nrows, geo, inv_lambda, sm, partial_out, w_eps_out, tag, tmo,
                                                direct_dbg)) {
            // few weighted rows: finished straight from the workgroup rows
        } else {
            merge_rows_block<NT, MAXCH, false, VIA>(slab_r, g * kGroup, gsz, geo, inv_lambda, sm, &gslab_r, g, nullptr,
                                                    nullptr, tag, tmo);
            STAMP(10, NOW());
            // ---- level 2: workgroup 0 polls and merges the group rows
            if (blockIdx.x != 0) return false;
            STAMP(4, NOW());
            merge_rows_block<NT, MAXCH, true, VIA>(gslab_r, 0, ngroups, geo, inv_lambda, sm, nullptr, 0, partial_out,
                                                   w_eps_out, tag, tmo);
        }
        // every workgroup read the epoch before publishing, and all have published
        if (threadIdx.x == 0) __hip_atomic_store(epoch, tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
        // ---- level 1: the last workgroup of each group of kGroup merges the group
        if (!arrive_last(counters + g, (unsigned)gsz, s_flag, acquire)) return false;
        STAMP(3, NOW());
        merge_rows_block<NT, MAXCH, false, VIA>(slab_r, g * kGroup, gsz, geo, inv_lambda, sm, &gslab_r, g, nullptr,
                                                nullptr, 0u, nullptr);
        STAMP(10, NOW());
        // ---- level 2: the last group merges the group rows and finishes the step
        if (!arrive_last(counters + ngroups, (unsigned)ngroups, s_flag, acquire)) return false;
        STAMP(4, NOW());
        if (!(ngroups > 1 && nrows <= kDirectRows &&
              direct_merge<NT, MAXCH, VIA>(slab_r, nrows, geo, inv_lambda, sm, partial_out, w_eps_out, 0u, nullptr)))
            merge_rows_block<NT, MAXCH, true, VIA>(gslab_r, 0, ngroups, geo, inv_lambda, sm, nullptr, 0, partial_out,
                                                   w_eps_out, 0u, nullptr);
    }
    return true;
}

// The same merge one launch later (the deferred finish of the 2-DoF device loop, mppi_rocm.hip): the n <=
// kDirectRows rows of the PREVIOUS launch, plain 8-byte values that became visible at the kernel boundary, merged
// by every workgroup for itself (RowsVia::Prev).  No poll, no tag, no counter, no spin.  The decision and the
// arithmetic are handoff_merge's, so the result has the same bits: direct_merge when more than one group exists and
// few rows carry weight; otherwise the group merges (each group's rows in ascending order against the group's
// minimum) followed by the merge of the group rows (ascending, against the global minimum), both of which are one
// round of merge_rows_block here (a group has kGroup <= 32 rows, and there are at most kDirectRows / kGroup <= 16
// groups).  Only the rho column is read of every row; of the rest, the rows whose own factor and whose group's
// factor are both non-zero, the ones merge_rows_block would have added.  The group sums stay in registers instead of
// going through a group row, which changes no bit.
// The rows' rho come from a compact copy behind the rows (value n * stride + r: 16 cache lines for 256 rows where
// the column inside the rows touches 256), which the deferred rollout's epilogue stores beside each row's own.
// l_row: kDirectRows ints of LDS.  Leaves w_eps in sm.weps (and w_eps_out when given) behind a barrier.
template <int NT, class SM>
__device__ __forceinline__ void deferred_merge(__amdgpu_buffer_rsrc_t rows, int n, const RowGeo& geo, double inv_lambda,
                                               SM& sm, int* l_row, double* w_eps_out) {
    constexpr int P = kDirectRows / 64;
    // row loads in flight per thread.  64 measured no faster than 32: with many weighted rows (a converged c3 step
    // that takes this path weights rows in 12 of its 16 groups) the walk below is bound by the lone wave's issue
    // rate, three uniform LDS reads and two branches per row, not by the round trips
    constexpr int LB = 32;
    static_assert(kGroup == 16, "a group is one DPP row of lanes");
    static_assert(kDirectRows / kGroup <= 16, "the group rows merge in one round in either hand-off form");
    const int tid = threadIdx.x, lane = tid & 63;
    const int stride = geo.stride, ncol = geo.ncol;   // ncol <= NT: one column per thread
    double rho_l[P];
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const int r = lane + 64 * j;
        const double x = ld_prev(rows, r < n ? n * stride + r : kOffRange);
        rho_l[j] = r < n ? x : INFINITY;
    }
    if (n > kGroup && direct_merge<NT, 1, RowsVia::Prev>(rows, n, geo, inv_lambda, sm, nullptr, w_eps_out, 0u, nullptr,
                                                           nullptr, rho_l))
        return;
    // level 1: row lane + 64 j belongs to group (lane >> 4) + 4 j, the 16 lanes of a DPP row in slot j
    double rho_g[P], m = INFINITY;
#pragma unroll
    for (int j = 0; j < P; ++j) {
        double v = rho_l[j];
        v = min_raw_f64(v, dpp_f64<0xB1>(v));
        v = min_raw_f64(v, dpp_f64<0x4E>(v));
        v = min_raw_f64(v, dpp_f64<0x141>(v));
        v = min_raw_f64(v, dpp_f64<0x140>(v));
        rho_g[j] = v;
        m = min_raw_f64(m, v);
    }
    const double rho = wave_min_f64(m);
    if (tid < 64) {
        int base = 0;
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const bool in = lane + 64 * j < n;
            const double s1 = exp((rho_g[j] - rho_l[j]) * inv_lambda);   // the row in its group
            const double s2 = exp((rho - rho_g[j]) * inv_lambda);        // the group among the groups
            const bool need = in && s1 >= kMergeFloor && s2 >= kMergeFloor;
            const unsigned long long bal = __ballot(need);
            if (need) {
                const int pos = base + lanes_below(bal);
                l_row[pos] = lane + 64 * j;
                sm.rho[pos] = s1;
                sm.part[pos] = s2;
            }
            base += __popcll(bal);
        }
        if (lane == 0) sm.nrel = base;
    }
    __syncthreads();
    const int nn = sm.nrel;   // >= 1: the row of the global minimum
    double acc = 0.0, accg = 0.0;
    for (int b0 = 0; b0 < nn; b0 += LB) {
        double v[LB];
#pragma unroll
        for (int j = 0; j < LB; ++j) {
            const int i = b0 + j;
            v[j] = ld_prev(rows, (i < nn && tid < ncol) ? l_row[i] * stride + 1 + tid : kOffRange);
        }
#pragma unroll
        for (int j = 0; j < LB; ++j) {
            const int i = b0 + j;
            if (i < nn) {
                accg = fma(sm.rho[i], v[j], accg);
                if (i + 1 == nn || (l_row[i + 1] / kGroup) != (l_row[i] / kGroup)) {   // the group's last row
                    acc = fma(sm.part[i], accg, acc);
                    accg = 0.0;
                }
            }
        }
    }
    if (tid == 0) {   // column 0 is eta
        sm.eta = acc;
        sm.rho_fin = rho;
    }
    __syncthreads();
    if (tid >= 1 && tid < ncol) {
        const double w = acc / sm.eta;
        sm.weps[tid - 1] = w;
        if (w_eps_out) w_eps_out[tid - 1] = w;
    }
    __syncthreads();
}

// ------------------------------------------------------ node-level exchange
// Multi-GPU (one process per GPU, one node) without a collective call per step:
// the launch's final workgroup writes this rank's merged row {rho, eta, N} as
// tagged granules into slot [parity][rank] of EVERY rank's inbox (IPC-mapped
// device memory; remote ranks over xGMI, system-scope stores), then polls its
// own inbox until the world rows of this step carry the tag and merges them in
// rank order with the same granule merge as inside a launch.  The pattern is
// RCCL's LL protocol (flagged stores into a peer's buffer); the inbox is
// uncached device memory, so a poll never reads a stale L2 line.  Tags come
// from a per-rank exchange epoch advanced once per exchange launch: every rank
// runs the same launches, so the epochs agree.  Two parity halves: a rank can
// write step n + 1 while a slower peer still reads step n, never step n + 2
// (it needs that peer's step n + 1 row first).
constexpr int kMaxWorld = MPPI_MAX_WORLD;
struct XDesc {
    const void* peer[kMaxWorld];   // inbox base of every rank (own rank: local memory)
    double* row;                   // this rank's merged row, written by the launch's final merge
    unsigned* epoch;               // this rank's exchange epoch
    int rank, world, bytes;        // bytes: inbox size (2 x world rows of `stride` granules, 2 x world statuses)
    unsigned timeout_ticks;        // the exchange polls' bound in s_memrealtime ticks (10 ns; 0: the ~1 s spin
                                   // bound), MPPI_EXCHANGE_TIMEOUT_US at attach
};
// host timeout word, cause bits: an in-launch hand-off of this launch timed out (its results are invalid; not
// retryable) / the step's exchange failed on every rank (retryable over the all-gather) / this rank had every
// row but not every rank's status in time, so the other ranks may have applied the step (not retryable)
constexpr unsigned kTmoLocal = 1u, kTmoExchange = 2u, kTmoSplit = 4u;
__device__ __forceinline__ void st_gran_sys(__amdgpu_buffer_rsrc_t r, int idx, double v, unsigned tag) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const u32x4 x = {(unsigned)b, tag, (unsigned)(b >> 32), tag};
    __builtin_amdgcn_raw_buffer_store_b128(x, r, idx * 16, 0, kSC1 | 1);   // sc0 sc1: system scope
}

// Called by the final workgroup after its merge wrote x.row (put_final ends with
// a barrier, so the row is visible to the whole workgroup).
//
// Failure semantics (a rank late past the bound, or gone): after the row round,
// every rank writes a status granule (+1: it had every row in time, -1: not) to
// every inbox and polls all of them; the step holds only if every rank reports
// +1.  A rank that gave up wrote its -1 before leaving, so a late rank, whenever
// it arrives, finds that status next to the rows it needs: every rank of the
// step reaches the same verdict.  On failure the launch reports kTmoExchange
// (the host raises MPPI_E_EXCHANGE and keeps the nominal: no update is applied)
// and the caller runs the step again over the collective fallback.  The epoch
// advances either way, so the ranks stay in step for the next exchange.
//
// Two halves, so the caller can compute the fused update while the statuses
// travel: exchange_send_merge (rows out, merge, this rank's status out; returns
// the step's tag) and exchange_verdict (the statuses in).  The update written in
// between goes only to the ping-pong block the host has not yet made current and
// to outputs the host reads after the verdict; on failure the host keeps the
// block it had and ignores them.
template <int NT, int MAXCH, class SM>
__device__ __forceinline__ unsigned exchange_send_merge(const XDesc& x, const RowGeo& geo, double inv_lambda, SM& sm,
                                                        double* w_eps_out, unsigned* tmo) {
    // the previous exchange launch's final store; kernel boundaries order it
    const unsigned tag = (unsigned)__builtin_amdgcn_readfirstlane((int)*x.epoch) + 1u;
    const int par = (int)(tag & 1u), stride = geo.stride;
    for (int idx = threadIdx.x; idx < stride; idx += NT) {
        const double v = x.row[idx];
        for (int p = 0; p < x.world; ++p)
            st_gran_sys(rows_rsrc(x.peer[p], x.bytes), (par * x.world + x.rank) * stride + idx, v, tag);
    }
    bool late = false;
    const unsigned long long dl = x.timeout_ticks ? __builtin_amdgcn_s_memrealtime() + x.timeout_ticks : 0ull;
    merge_rows_block<NT, MAXCH, true, RowsVia::Gran>(rows_rsrc(x.peer[x.rank], x.bytes), par * x.world, x.world, geo,
                                                     inv_lambda, sm, nullptr, 0, nullptr, w_eps_out, tag, nullptr, dl,
                                                     &late);
    // this rank's own row is invalid if an in-launch hand-off of this launch timed out
    late = __syncthreads_or(late || (threadIdx.x == 0 && tmo &&
                                     __hip_atomic_load(tmo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u));
    const int sbase = 2 * x.world * stride + par * x.world;   // status granules follow the rows: [parity][rank]
    if ((int)threadIdx.x < x.world)
        st_gran_sys(rows_rsrc(x.peer[threadIdx.x], x.bytes), sbase + x.rank, late ? -1.0 : 1.0, tag);
    return tag;
}

template <int NT>
__device__ __forceinline__ bool exchange_verdict(const XDesc& x, const RowGeo& geo, unsigned tag, unsigned* tmo) {
    const int par = (int)(tag & 1u);
    const int sbase = 2 * x.world * geo.stride + par * x.world;
    const int tid = threadIdx.x, lane = tid & 63;
    bool bad = false, split = false;
    if (tid < 64) {   // wave 0 polls every rank's status (world <= 64)
        const __amdgpu_buffer_rsrc_t own = rows_rsrc(x.peer[x.rank], x.bytes);
        u32x4 g;
        bool missing = false;
        const unsigned long long dl = x.timeout_ticks ? __builtin_amdgcn_s_memrealtime() + x.timeout_ticks : 0ull;
        for (unsigned spins = 0;; ++spins) {
            asm volatile("" ::: "memory");
            g = ld_gran(own, lane < x.world ? sbase + lane : kOffRange);
            if (__all(lane >= x.world || gran_ok(g, tag))) break;
            MPPI_SPIN_OR_GIVE_UP_L(spins, dl, nullptr, lane, missing = true);
        }
        bad = __any(lane < x.world && !(gran_ok(g, tag) && gran_val(g) > 0.0)) || missing;
        // A status that never came while this rank's own is not a -1: the ranks whose statuses all arrived may
        // have applied the step, so re-running it here would pair this rank's retry with their next step.
        // Only a rank that reported -1 itself knows every rank fails (each waits for, or times out on, its -1).
        split = missing && !__any(lane == x.rank && gran_ok(g, tag) && gran_val(g) < 0.0);
    }
    bad = __syncthreads_or(bad);
    split = __syncthreads_or(split);
    if (tid == 0) {
        if (bad)
            __hip_atomic_store(tmo + 1, split ? kTmoExchange | kTmoSplit : kTmoExchange, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_SYSTEM);
        *x.epoch = tag;
    }
    return !bad;
}

}  // namespace mppi
