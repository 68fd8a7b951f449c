// Stand-alone host program over csrc/mppi_host.h (tests/test_host_plumbing.py builds it host-only under
// AddressSanitizer and UBSan and compares its output with NumPy).  No device is touched: the helpers make no
// HIP call, and `owners` runs where none is visible, so its HIP calls fail.  One command per line on stdin,
// doubles as C hex floats; one result line each (a window: one line per slot array; owners: one per member).
//   window W <4 W doubles>               -> win / key / ctr as fp32 bit patterns
//   exploit <param_exploration> K_total  -> k_exploit
//   gamma <gamma> <lambda> <alpha>       -> the resolved gamma
//   geometry K_local K_total k_offset    -> return code
//   timeout w0 w1                        -> return code, verdict bits, the two words afterwards, the message
//   handoff nblocks ncu per_cu stride extra_words -> form and sizes
//   owners                               -> per failing member: return code, 1 if the owner stayed empty, the message
#include <stdio.h>
#include <string.h>

#include <vector>

#include "mppi_host.h"

namespace {
unsigned bits(float f) {
    unsigned u;
    memcpy(&u, &f, sizeof(u));
    return u;
}
void print_slots(const char* name, const float4* v, int n) {
    printf("%s", name);
    for (int j = 0; j < n; ++j) printf(" %08x %08x %08x %08x", bits(v[j].x), bits(v[j].y), bits(v[j].z), bits(v[j].w));
    printf("\n");
}

void owner_line(const char* name, int rc, bool empty) {
    printf("owners %s %d %d %s\n", name, rc, (int)empty, rc ? mppi_host::last_error() : "");
}

// Every member of the owners that can fail, where no device is visible: the return code, whether the owner is
// still empty, the message.  Each is reset twice afterwards and destructed at the end of the function.
void owners() {
    using namespace mppi_host;
    DevBuf<double> dev;
    owner_line("DevBuf.alloc", dev.alloc(16), !dev && dev.cap == 0);
    owner_line("DevBuf.alloc_zeroed", dev.alloc_zeroed(16), !dev && dev.cap == 0);
    bool fresh = false;
    owner_line("DevBuf.reserve", dev.reserve(16, &fresh), !dev && dev.cap == 0 && fresh);
    fresh = false;
    owner_line("DevBuf.reserve0", dev.reserve(0, &fresh), !dev && dev.cap == 0 && !fresh);   // nothing to do: MPPI_OK
    PinnedBuf<float> pinned;
    owner_line("PinnedBuf.alloc", pinned.alloc(16), !pinned);
    MappedBuf<unsigned> mapped;
    owner_line("MappedBuf.alloc", mapped.alloc(64, kCoherent), !mapped && !mapped.dev);
    Event ev;
    owner_line("Event.create", ev.create(), !ev);
    Stream st;
    owner_line("Stream.create", st.create(), !st);
    for (int i = 0; i < 2; ++i) dev.reset(), pinned.reset(), mapped.reset(), ev.reset(), st.reset();
    Handoff hand;
    owner_line("Handoff.setup", hand.setup(256, 256, 1, 130, 0), !hand.d_slab && !hand.d_counter && !hand.h_tmo);
    Exchange ex;
    hipIpcMemHandle_t handle;
    owner_line("Exchange.handle", ex.handle(0, 130, 2, &handle), !ex.d_inbox && ex.world_alloc == 0);
}
}  // namespace

int main() {
    char cmd[32];
    while (scanf("%31s", cmd) == 1) {
        if (!strcmp(cmd, "window")) {
            int W = 0;
            if (scanf("%d", &W) != 1 || W < 1 || W > MPPI_SEARCH_LEN) return 2;
            std::vector<double> window(4 * (size_t)W);   // exactly W rows: a read past them is an ASan report
            for (double& v : window)
                if (scanf("%la", &v) != 1) return 2;
            std::vector<float4> win(mppi::kSlots), key(mppi::kSlots);
            float4 ctr;
            mppi_host::stage_window(window.data(), W, win.data(), key.data(), &ctr);
            print_slots("win", win.data(), mppi::kSlots);
            print_slots("key", key.data(), mppi::kSlots);
            print_slots("ctr", &ctr, 1);
        } else if (!strcmp(cmd, "exploit")) {
            double p;
            int K;
            if (scanf("%la %d", &p, &K) != 2) return 2;
            printf("exploit %d\n", mppi_host::exploit_count(p, K));
        } else if (!strcmp(cmd, "gamma")) {
            double g, l, a;
            if (scanf("%la %la %la", &g, &l, &a) != 3) return 2;
            printf("gamma %a\n", mppi_host::resolve_gamma(g, l, a));
        } else if (!strcmp(cmd, "geometry")) {
            int kl, kt, ko;
            if (scanf("%d %d %d", &kl, &kt, &ko) != 3) return 2;
            printf("geometry %d\n", mppi_host::check_sample_geometry(kl, kt, ko));
        } else if (!strcmp(cmd, "timeout")) {
            unsigned tmo[2], v = ~0u;
            if (scanf("%u %u", &tmo[0], &tmo[1]) != 2) return 2;
            const int rc = mppi_host::take_timeout(tmo, &v);
            printf("timeout %d %u %u %u %s\n", rc, v, tmo[0], tmo[1], rc ? mppi_host::last_error() : "");
        } else if (!strcmp(cmd, "handoff")) {
            int nblocks, ncu, per_cu, stride;
            unsigned long extra;
            if (scanf("%d %d %d %d %lu", &nblocks, &ncu, &per_cu, &stride, &extra) != 5) return 2;
            mppi_host::Handoff h;
            h.plan(nblocks, ncu, per_cu, stride, extra);
            printf("handoff %d %d %d %zu %zu %zu %zu\n", (int)h.poll, h.acquire, h.ngroups, h.slab, h.gslab, h.extra_off,
                   h.ctr_bytes);
        } else if (!strcmp(cmd, "owners")) {
            owners();
        } else {
            return 2;
        }
    }
    return 0;
}
