// mppi_host.h — the host-side plumbing shared by the translation units of
// libmppi_rocm.so: the one error channel behind mppi_last_error(), HIP_TRY,
// the owners of every HIP buffer, event and stream the four contexts hold,
// and what the 2-link context (mppi_rocm.hip) and the chain's (mppi_chain.hip)
// both carry: the launch constants fixed at construction, the staging of the
// waypoint window, the in-launch hand-off's buffers and time-out verdict, and
// the node-level exchange.  Header-only (inline functions, one C++17 inline
// variable), so a stand-alone host program can include it without the library
// (tests/host_plumbing_main.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <type_traits>

#include "mppi_device.h"  // (with mppi_merge.h) XDesc, kSlots, kPadKey, kGroup, kMaxWorld, kTmo*
#include "mppi_rocm.h"

namespace mppi_host {

inline thread_local std::string g_err;

// Records msg as this thread's last error (mppi_last_error) and returns code.
inline int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
inline const char* last_error() { return g_err.c_str(); }

// The in-launch exchange's poll bound in s_memrealtime ticks (10 ns): MPPI_EXCHANGE_TIMEOUT_US when set
// (tests bound it to milliseconds), else 0 (the device's spin bound, ~1 s).
inline unsigned exchange_timeout_ticks() {
    const char* e = getenv("MPPI_EXCHANGE_TIMEOUT_US");
    const long v = e ? strtol(e, nullptr, 10) : 0;
    return v > 0 && v < 40000000 ? (unsigned)(v * 100) : 0u;   // s_memrealtime runs at 100 MHz
}

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return mppi_host::fail(MPPI_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

inline int launch_check(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MPPI_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
    return MPPI_OK;
}

// ------------------------------------------------- owners of HIP resources
//
// What a context allocates is a member of one of these: the destructor releases it, so a half-built context and
// a destroyed one end the same way and no *_destroy lists buffers.  Not copyable and not movable (the contexts
// are heap objects that never move); each converts to its raw pointer or handle, so launches and copies read as
// with raw members.  What can fail returns a code through HIP_TRY and leaves the owner empty; n counts elements.
template <class H, auto Drop>
struct Owner {
    H h = nullptr;
    Owner() = default;
    Owner(const Owner&) = delete;
    Owner& operator=(const Owner&) = delete;
    ~Owner() { reset(); }
    operator H() const { return h; }
    void reset() {
        if (h) (void)Drop(h);
        h = nullptr;
    }
};

template <class T>
struct DevBuf : Owner<T*, hipFree> {
    size_t cap = 0;
    void reset(T* block = nullptr, size_t n = 0) {   // frees; with a block, takes it over (Exchange's uncached inbox)
        Owner<T*, hipFree>::reset();
        this->h = block;
        cap = n;
    }
    int alloc(size_t n) {
        reset();
        HIP_TRY(hipMalloc(&this->h, n * sizeof(T)));
        cap = n;
        return MPPI_OK;
    }
    int alloc_zeroed(size_t n) {
        if (int rc = alloc(n)) return rc;
        HIP_TRY(hipMemset(this->h, 0, n * sizeof(T)));
        return MPPI_OK;
    }
    // At least n elements: untouched while cap suffices, else freed first and allocated anew (contents are not
    // carried over), which *fresh = true reports.
    int reserve(size_t n, bool* fresh) {
        if (n <= cap) return MPPI_OK;
        *fresh = true;
        return alloc(n);
    }
};

template <class T>
struct PinnedBuf : Owner<T*, hipHostFree> {
    T* operator->() const { return this->h; }
    int alloc(size_t n, unsigned flags = hipHostMallocDefault) {
        this->reset();
        HIP_TRY(hipHostMalloc(&this->h, n * sizeof(T), flags));
        return MPPI_OK;
    }
};

constexpr unsigned kCoherent = hipHostMallocCoherent;   // MappedBuf::alloc's flag
template <class T>
struct MappedBuf : PinnedBuf<T> {   // host-mapped: converts to the host pointer, dev is its device view
    T* dev = nullptr;
    void reset() { PinnedBuf<T>::reset(), dev = nullptr; }
    int alloc(size_t n, unsigned flags) {   // flags: 0 or kCoherent
        reset();
        if (int rc = PinnedBuf<T>::alloc(n, hipHostMallocMapped | flags)) return rc;
        HIP_TRY(hipHostGetDevicePointer((void**)&dev, this->h, 0));
        return MPPI_OK;
    }
};

struct Event : Owner<hipEvent_t, hipEventDestroy> {
    int create() {
        reset();
        HIP_TRY(hipEventCreateWithFlags(&h, hipEventDisableTiming));
        return MPPI_OK;
    }
};

struct Stream : Owner<hipStream_t, hipStreamDestroy> {
    int create() {
        reset();
        HIP_TRY(hipStreamCreateWithFlags(&h, hipStreamNonBlocking));
        return MPPI_OK;
    }
};

// Run-time values as template arguments: f(std::integral_constant<int, V>{}) for the V equal to v (f is not
// called when there is none), f(std::true_type{}) or f(std::false_type{}) for b.  A context names the kernel
// instance it uses through these, so each file lists its instantiated kernels once.
template <int... V, class F>
void with_value(int v, F&& f) {
    (void)((v == V && (f(std::integral_constant<int, V>{}), true)) || ...);
}
template <class F>
void with_bool(bool b, F&& f) {
    b ? f(std::true_type{}) : f(std::false_type{});
}

// ------------------------------------------------- launch constants fixed at construction

inline int check_sample_geometry(int K_local, int K_total, int k_offset) {
    if (K_local < 1 || K_total < K_local || k_offset < 0 || k_offset + (long long)K_local > K_total)
        return fail(MPPI_E_ARG, "bad sample geometry (K_local, K_total, k_offset)");
    return MPPI_OK;
}

// Samples [0, k_exploit) of the K_total add the nominal to their noise; the rest explore (control.py:98).
inline int exploit_count(double param_exploration, int K_total) {
    const double thr = (1.0 - param_exploration) * (double)K_total;
    long long kx = thr <= 0.0 ? 0 : (long long)ceil(thr);
    if (kx > K_total) kx = K_total;
    return (int)kx;
}

// control.py:45 fixes gamma at construction; the caller passes it as given (NaN: lambda (1 - alpha))
inline double resolve_gamma(double param_gamma, double param_lambda, double param_alpha) {
    return isnan(param_gamma) ? param_lambda * (1.0 - param_alpha) : param_gamma;
}

// The fields KConst and ChainConst share, from mppi_config / mppi_chain_config.
template <class KC, class Cfg>
void set_common_consts(KC& k, const Cfg& cfg, int nblocks) {
    k.K_local = cfg.K_local;
    k.T = cfg.T;
    k.k_offset = cfg.k_offset;
    k.k_exploit = exploit_count(cfg.param_exploration, cfg.K_total);
    k.nblocks = nblocks;
    k.lambda = cfg.param_lambda;
    k.inv_lambda = 1.0 / cfg.param_lambda;
    k.gamma = resolve_gamma(cfg.param_gamma, cfg.param_lambda, cfg.param_alpha);
}

// ------------------------------------------------- window staging

// The W window rows (x, y, dq1, dq2 in fp64) as the search reads them: win[j] the row in fp32, key[j] its
// centred search key (-2 rx', -2 ry', rx'^2 + ry'^2, 0) about the window's mean, computed in fp64 and
// rounded last; slots W..kSlots-1 are pads no sample can be nearest to; ctr = (cx, cy, W, 0).  The search
// kernels of both libraries depend on these bits: keep the operation order.
inline void stage_window(const double* window, int W, float4* win, float4* key, float4* ctr) {
    double cx = 0.0, cy = 0.0;
    for (int j = 0; j < W; ++j) {
        cx += window[4 * j];
        cy += window[4 * j + 1];
    }
    cx /= W;
    cy /= W;
    for (int j = 0; j < mppi::kSlots; ++j) {
        if (j < W) {
            const double* r = window + 4 * j;
            win[j] = make_float4((float)r[0], (float)r[1], (float)r[2], (float)r[3]);
            const double rx = r[0] - cx, ry = r[1] - cy;
            key[j] = make_float4((float)(-2.0 * rx), (float)(-2.0 * ry), (float)(rx * rx + ry * ry), 0.f);
        } else {
            win[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            key[j] = make_float4(0.f, 0.f, mppi::kPadKey, 0.f);
        }
    }
    *ctr = make_float4((float)cx, (float)cy, (float)W, 0.f);
}

// ------------------------------------------------- in-launch hand-off

// Reads and clears the two host-mapped time-out words (tmo[0]: a local hand-off gave up, kTmoLocal; tmo[1]:
// the exchange's verdict bits, mppi_merge.h) and records the verdict's message: MPPI_OK when neither is
// set.  *bits gets the verdict, for the caller's own roll-back: kTmoExchange alone means every rank of the
// step reports it and none applied the update, so the step can run again from the nominal before the launch.
inline int take_timeout(unsigned* h_tmo, unsigned* bits) {
    const unsigned v = h_tmo ? __atomic_load_n(h_tmo, __ATOMIC_ACQUIRE) | __atomic_load_n(h_tmo + 1, __ATOMIC_ACQUIRE)
                             : 0u;
    *bits = v;
    if (!v) return MPPI_OK;
    h_tmo[0] = h_tmo[1] = 0;
    if (v == mppi::kTmoExchange)
        return fail(MPPI_E_EXCHANGE, "multi-GPU exchange: a rank's row did not arrive within the bound on every "
                                     "rank of this step; no rank applied the update (run the step again)");
    if (v & mppi::kTmoSplit)
        return fail(MPPI_E_HIP, "multi-GPU exchange: this rank had every row but not every rank's verdict within "
                                "the bound; other ranks may have applied the step, so it cannot be re-run");
    return fail(MPPI_E_HIP, "in-launch hand-off timed out (workgroups not co-resident?); results invalid");
}

// Hand-off form and buffers of one context.  Tagged-granule polling when every workgroup is resident at once
// (at most one per CU, the measured form); arrival counters otherwise, with an agent acquire once workgroups
// share CUs.  MPPI_HANDOFF=counter forces the counter form (tests).
struct Handoff {
    bool poll = false;              // granule hand-off (grid <= one workgroup per CU)
    int acquire = 0;                // the counter form's merges need an agent acquire (kernel constant)
    int ngroups = 0;
    size_t slab = 0, gslab = 0;     // bytes of the workgroup rows and of the group rows
    size_t extra_off = 0;           // word offset of the caller's extra words in the counter block (256-B aligned)
    size_t ctr_bytes = 0;
    DevBuf<double> d_slab, d_gslab;
    DevBuf<unsigned> d_counter;     // [ngroups + 1] arrival counters (counter hand-off), then the epoch word
    unsigned* d_epoch = nullptr;    // granule epoch (poll hand-off), inside the d_counter block
    MappedBuf<unsigned> h_tmo;      // host-mapped: a bounded in-launch spin gave up

    // Form and sizes (no HIP call).  per_cu: the rollout kernel's occupancy (0: not known); stride: values of
    // a partial row; extra_words: counter words of the caller's own behind the block.
    void plan(int nblocks, int ncu, int per_cu, int stride, size_t extra_words) {
        poll = per_cu >= 1 && nblocks <= ncu;
        if (const char* ev = getenv("MPPI_HANDOFF")) {
            if (!strcmp(ev, "counter")) poll = false;
        }
        acquire = (!poll && nblocks > ncu) ? 1 : 0;
        const size_t val = poll ? 16 : sizeof(double);  // granule or plain fp64
        ngroups = (nblocks + mppi::kGroup - 1) / mppi::kGroup;
        slab = (size_t)nblocks * stride * val;
        gslab = (size_t)ngroups * stride * val;
        extra_off = (((size_t)(ngroups + 2) * sizeof(unsigned) + 255) & ~(size_t)255) / sizeof(unsigned);
        ctr_bytes = (extra_off + extra_words) * sizeof(unsigned);
    }
    // plan(), then the buffers, zeroed (the caller synchronizes the device before the first launch).
    int setup(int nblocks, int ncu, int per_cu, int stride, size_t extra_words) {
        plan(nblocks, ncu, per_cu, stride, extra_words);
        if (int rc = d_slab.alloc_zeroed(slab / sizeof(double))) return rc;
        if (int rc = d_gslab.alloc_zeroed(gslab / sizeof(double))) return rc;
        if (int rc = d_counter.alloc_zeroed(ctr_bytes / sizeof(unsigned))) return rc;
        if (int rc = h_tmo.alloc(256 / sizeof(unsigned), 0)) return rc;
        h_tmo[0] = h_tmo[1] = 0;
        d_epoch = d_counter + ngroups + 1;
        return MPPI_OK;
    }
    int take_timeout(unsigned* bits) { return mppi_host::take_timeout(h_tmo, bits); }
};

// ------------------------------------------------- node-level exchange (mppi_exchange_*, mppi_chain_exchange_*)

// The inbox, this rank's row, its epoch and the peers' mappings behind the kernels' XDesc.
struct Exchange {
    mppi::XDesc xd{};
    DevBuf<char> d_inbox;           // hipDeviceMallocUncached
    DevBuf<double> d_xrow;
    DevBuf<unsigned> d_xepoch;
    int world_alloc = 0;
    void* opened[mppi::kMaxWorld] = {};

    ~Exchange() {   // the peers' mappings close before the members free the inbox
        for (void* p : opened)
            if (p) (void)hipIpcCloseMemHandle(p);
    }

    // Allocates the inbox for `world` ranks' rows of `stride` values on first use; its IPC handle.
    int handle(int device, int stride, int world, void* handle_out) {
        if (d_inbox && world_alloc != world) return fail(MPPI_E_ARG, "inbox already sized for another world");
        if (!d_inbox) {
            const size_t bytes = (size_t)2 * world * (stride + 1) * 16;   // rows and statuses, two parities
            HIP_TRY(hipSetDevice(device));
            void* inbox = nullptr;
            HIP_TRY(hipExtMallocWithFlags(&inbox, bytes, hipDeviceMallocUncached));
            d_inbox.reset(static_cast<char*>(inbox), bytes);
            HIP_TRY(hipMemset(d_inbox, 0, bytes));
            if (int rc = d_xrow.alloc(stride)) return rc;
            if (int rc = d_xepoch.alloc_zeroed(256 / sizeof(unsigned))) return rc;
            HIP_TRY(hipDeviceSynchronize());
            world_alloc = world;
            xd.bytes = (int)bytes;
        }
        HIP_TRY(hipIpcGetMemHandle(static_cast<hipIpcMemHandle_t*>(handle_out), d_inbox));
        return MPPI_OK;
    }
    // Maps every other rank's inbox (handles: world hipIpcMemHandle_t in rank order) and arms the descriptor.
    int attach(int device, int rank, int world, const void* handles) {
        if (xd.world) return fail(MPPI_E_ARG, "already attached");
        HIP_TRY(hipSetDevice(device));
        const hipIpcMemHandle_t* h = static_cast<const hipIpcMemHandle_t*>(handles);
        for (int p = 0; p < world; ++p) {
            if (p == rank) {
                xd.peer[p] = d_inbox;
                continue;
            }
            void* ptr = nullptr;
            HIP_TRY(hipIpcOpenMemHandle(&ptr, h[p], hipIpcMemLazyEnablePeerAccess));
            opened[p] = ptr;
            xd.peer[p] = ptr;
        }
        xd.row = d_xrow;
        xd.epoch = d_xepoch;
        xd.rank = rank;
        xd.world = world;
        xd.timeout_ticks = exchange_timeout_ticks();
        return MPPI_OK;
    }
};

}  // namespace mppi_host
