// Stand-alone host program over the library's four translation units (tests/test_host_contexts.py compiles them
// whole under AddressSanitizer and UBSan, links them with this file and runs the result directly): the four
// context constructors with small valid configurations.  Run where no device is visible, each fails in its first
// HIP call and gives the half-built context back through its members' destructors; one line per call:
//   <name> <return code> <1 if *out is null> <mppi_last_error()>
// Exit status 0 unless a sanitizer (leak check included) reports.
#include <stdio.h>

#include "mppi_rocm.h"

int main() {
    mppi_config cfg;
    mppi_config_init(&cfg);
    cfg.K_local = cfg.K_total = 1024;
    cfg.T = 20;
    cfg.delta_t = 0.01;
    cfg.param_lambda = 50.0;
    cfg.param_alpha = 0.98;
    cfg.sigma[0] = cfg.sigma[3] = 20.0;
    mppi_ctx* arm = reinterpret_cast<mppi_ctx*>(&cfg);   // any non-null value: create must clear it
    int rc = mppi_ctx_create(&cfg, 0, nullptr, &arm);
    printf("arm %d %d %s\n", rc, arm == nullptr, mppi_last_error());

    mppi_chain_config cc;
    mppi_chain_config_init(&cc);
    cc.K_local = cc.K_total = 1024;
    cc.T = 20;
    cc.delta_t = 0.006;
    cc.param_lambda = 100.0;
    cc.param_alpha = 0.98;
    cc.chain.n = 3;
    for (int i = 0; i < 3; ++i) {
        cc.sigma[i * 3 + i] = 4.0;
        cc.chain.m[i] = 1.0;
        cc.chain.l[i] = 0.5;
        cc.chain.lc[i] = 0.25;
        cc.chain.I[i] = 0.02;
        cc.chain.fk[i] = 0.5;
    }
    mppi_chain_ctx* chain = reinterpret_cast<mppi_chain_ctx*>(&cc);
    rc = mppi_chain_ctx_create(&cc, 0, nullptr, &chain);
    printf("chain %d %d %s\n", rc, chain == nullptr, mppi_last_error());

    static double log_params[MPPI_NP_LOG_DATA];
    mppi_np_ctx* np = reinterpret_cast<mppi_np_ctx*>(log_params);
    rc = mppi_np_ctx_create(0, log_params, &np);
    printf("np %d %d %s\n", rc, np == nullptr, mppi_last_error());

    mppi_readback* rb = reinterpret_cast<mppi_readback*>(&cfg);
    rc = mppi_readback_create(0, 2, 2, 4096, 2, &rb);
    printf("readback %d %d %s\n", rc, rb == nullptr, mppi_last_error());
    return 0;
}
