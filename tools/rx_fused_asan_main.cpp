// Stand-alone host-sanitizer check of the fused receive front end's argument validation
// (ldpc5g_sch_demod_raterecover, ldpc5g_sch_rx_decode, ldpc5g_sch_rx_scratch_elems): every call
// below returns before any kernel launch, so it needs no GPU.  Build it against the
// host-sanitized library (python -m python_5gtoolbox_amd.build --asan -> build/asan/libldpc5g.so):
//
//   CXX=/opt/rocm/lib/llvm/bin/clang++
//   RT=$(dirname $($CXX --print-file-name=libclang_rt.asan-x86_64.so))
//   $CXX -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -shared-libasan \
//       -Iinclude tools/rx_fused_asan_main.cpp -Lbuild/asan -lldpc5g -Wl,-rpath,$PWD/build/asan \
//       -Wl,-rpath,$RT -o build/asan/rx_fused_asan_main && build/asan/rx_fused_asan_main
//
// Exit status 0 and "rx_fused_asan_main: ok" mean every check held and no sanitizer report.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "ldpc5g.h"

static int fails = 0;
#define EXPECT(cond)                                                              \
    do {                                                                          \
        if (!(cond)) {                                                            \
            printf("FAILED %s:%d: %s  [%s]\n", __FILE__, __LINE__, #cond, ldpc5g_last_error()); \
            ++fails;                                                              \
        }                                                                         \
    } while (0)

int main() {
    ldpc5g_sch_cfg_t cfg, big, bpsk;
    EXPECT(ldpc5g_sch_config(12000, 4, 517.0, 1, 0, 30000, 25000, &cfg) == LDPC5G_OK);
    EXPECT(ldpc5g_sch_config(2000, 2, 500.0, 1, 0, 60000, 60000, &big) == LDPC5G_OK);
    EXPECT(ldpc5g_sch_config(9000, 1, 400.0, 1, 0, 0, 19998, &bpsk) == LDPC5G_OK);
    const int64_t nsym = cfg.E_total / cfg.Qm, nw = (cfg.E_total + 31) / 32;
    char buf[64];   // stands for every device buffer: never dereferenced by the validation
    void* P = buf;
    const float* NV = (const float*)buf;
    const uint32_t* W = (const uint32_t*)buf;

    auto front = [&](const ldpc5g_sch_cfg_t* c, const void* sym, int sdt, int64_t lds, const float* nv, int64_t ldnv,
                     const uint32_t* w, int64_t ldw, int mod, int T, void* dn, int ddt, void* ws, int64_t ldws) {
        return ldpc5g_sch_demod_raterecover(sym, sdt, lds, nv, ldnv, w, ldw, mod, c, T, nullptr, dn, ddt, ws, ldws, nullptr);
    };
    // |mod| != Qm, unknown modulation, dtypes
    EXPECT(front(&cfg, P, LDPC5G_F32, nsym, NV, nsym, nullptr, 0, 2, 2, P, LDPC5G_F32, nullptr, 0) == LDPC5G_ESIZE);
    EXPECT(strlen(ldpc5g_last_error()) > 0);
    EXPECT(front(&cfg, P, LDPC5G_F32, nsym, NV, nsym, nullptr, 0, -1, 2, P, LDPC5G_F32, nullptr, 0) == LDPC5G_ESIZE);
    EXPECT(front(&cfg, P, LDPC5G_F32, nsym, NV, nsym, nullptr, 0, 3, 2, P, LDPC5G_F32, nullptr, 0) == LDPC5G_ESIZE);
    EXPECT(front(&cfg, P, 7, nsym, NV, nsym, nullptr, 0, 4, 2, P, LDPC5G_F32, nullptr, 0) == LDPC5G_ESIZE);
    EXPECT(front(&cfg, P, LDPC5G_F64, nsym, NV, nsym, nullptr, 0, 4, 2, P, -1, nullptr, 0) == LDPC5G_ESIZE);
    // strides with T > 1
    EXPECT(front(&cfg, P, LDPC5G_F32, nsym - 1, NV, nsym, nullptr, 0, 4, 2, P, LDPC5G_F32, nullptr, 0) == LDPC5G_ESIZE);
    EXPECT(front(&cfg, P, LDPC5G_F32, nsym, NV, nsym - 1, nullptr, 0, 4, 2, P, LDPC5G_F32, nullptr, 0) == LDPC5G_ESIZE);
    EXPECT(front(&cfg, P, LDPC5G_F32, nsym, NV, nsym, W, nw - 1, 4, 2, P, LDPC5G_F32, nullptr, 0) == LDPC5G_ESIZE);
    // null buffers, null / inconsistent cfg, negative T
    EXPECT(front(&cfg, nullptr, LDPC5G_F32, nsym, NV, nsym, nullptr, 0, 4, 1, P, LDPC5G_F32, nullptr, 0) == LDPC5G_ESIZE);
    EXPECT(front(&cfg, P, LDPC5G_F32, nsym, nullptr, nsym, nullptr, 0, 4, 1, P, LDPC5G_F32, nullptr, 0) == LDPC5G_ESIZE);
    EXPECT(front(&cfg, P, LDPC5G_F32, nsym, NV, nsym, nullptr, 0, 4, 1, nullptr, LDPC5G_F32, nullptr, 0) == LDPC5G_ESIZE);
    EXPECT(front(nullptr, P, LDPC5G_F32, nsym, NV, nsym, nullptr, 0, 4, 1, P, LDPC5G_F32, nullptr, 0) == LDPC5G_ESIZE);
    ldpc5g_sch_cfg_t bad = cfg;
    bad.K_apo += 1;
    EXPECT(front(&bad, P, LDPC5G_F32, nsym, NV, nsym, nullptr, 0, 4, 1, P, LDPC5G_F32, nullptr, 0) == LDPC5G_ESIZE);
    EXPECT(front(&cfg, P, LDPC5G_F32, nsym, NV, nsym, nullptr, 0, 4, -1, P, LDPC5G_F32, nullptr, 0) == LDPC5G_ESIZE);
    // empty batch
    EXPECT(front(&cfg, nullptr, LDPC5G_F32, 0, nullptr, 0, nullptr, 0, 4, 0, nullptr, LDPC5G_F32, nullptr, 0) == LDPC5G_OK);
    EXPECT(strlen(ldpc5g_last_error()) == 0);
    // a row larger than the stage: scratch needed, and its stride checked
    EXPECT(ldpc5g_sch_rx_scratch_elems(&big, 2, LDPC5G_F32) == big.E_total);
    EXPECT(ldpc5g_sch_rx_scratch_elems(&cfg, 4, LDPC5G_F64) == 0);
    EXPECT(ldpc5g_sch_rx_scratch_elems(&cfg, 2, LDPC5G_F64) == LDPC5G_ESIZE);
    EXPECT(ldpc5g_sch_rx_scratch_elems(nullptr, 2, LDPC5G_F64) == LDPC5G_ESIZE);
    EXPECT(ldpc5g_sch_rx_scratch_elems(&bpsk, 1, LDPC5G_F32) == 0);
    EXPECT(ldpc5g_sch_rx_scratch_elems(&bpsk, -1, LDPC5G_F64) == 0);
    EXPECT(ldpc5g_sch_rx_scratch_elems(&bpsk, 1, LDPC5G_F64) == bpsk.E_total);
    const int64_t bs = big.E_total / big.Qm;
    EXPECT(front(&big, P, LDPC5G_F32, bs, NV, bs, nullptr, 0, 2, 2, P, LDPC5G_F32, nullptr, 0) == LDPC5G_ESIZE);
    EXPECT(strstr(ldpc5g_last_error(), "LDS stage") != nullptr);
    EXPECT(front(&big, P, LDPC5G_F32, bs, NV, bs, nullptr, 0, 2, 2, P, LDPC5G_F32, P, big.E_total - 1) == LDPC5G_ESIZE);

    auto chain = [&](const void* sym, int mod, int T) {
        return ldpc5g_sch_rx_decode(sym, LDPC5G_F32, nsym, NV, nsym, nullptr, 0, mod, &cfg, T, nullptr, P, LDPC5G_F32,
                                    nullptr, 0, nullptr, nullptr, nullptr, 8, 0.8, 0.0, LDPC5G_LAYERED, nullptr, cfg.B,
                                    nullptr, nullptr, nullptr, nullptr);
    };
    EXPECT(chain(P, 6, 1) == LDPC5G_ESIZE);
    EXPECT(chain(nullptr, 4, 1) == LDPC5G_ESIZE);
    EXPECT(chain(P, 4, 0) == LDPC5G_OK);
    if (fails) return 1;
    printf("rx_fused_asan_main: ok\n");
    return 0;
}
