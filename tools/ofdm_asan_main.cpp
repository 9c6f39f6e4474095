// Stand-alone host-sanitizer check of the argument validation of the OFDM low-PHY
// (ldpc5g_ofdm_demod, ldpc5g_ofdm_mod): every call below returns before any kernel launch, so it
// needs no GPU.  Build it against the host-sanitized library (python -m python_5gtoolbox_amd.build
// --asan -> build/asan/libldpc5g.so):
//
//   CXX=/opt/rocm/lib/llvm/bin/clang++
//   RT=$(dirname $($CXX --print-file-name=libclang_rt.asan-x86_64.so))
//   $CXX -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -shared-libasan \
//       -Iinclude tools/ofdm_asan_main.cpp -Lbuild/asan -lldpc5g -Wl,-rpath,$PWD/build/asan \
//       -Wl,-rpath,$RT -o build/asan/ofdm_asan_main && build/asan/ofdm_asan_main
//
// Exit status 0 and "ofdm_asan_main: ok" mean every check held and no sanitizer report.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <initializer_list>

#include "ldpc5g.h"

static int fails = 0;
#define EXPECT(cond)                                                              \
    do {                                                                          \
        if (!(cond)) {                                                            \
            printf("FAILED %s:%d: %s  [%s]\n", __FILE__, __LINE__, #cond, ldpc5g_last_error()); \
            ++fails;                                                              \
        }                                                                         \
    } while (0)
#define REFUSED(a, word)                                             \
    do {                                                             \
        EXPECT(call(a) == LDPC5G_ESIZE);                             \
        EXPECT(strstr(ldpc5g_last_error(), word) != nullptr);        \
    } while (0)

struct Ofdm {   // a valid call of either entry point: the 24-PRB carrier, two slots, two antennas, complex64
    bool demod = true;
    const void* td;
    const void* grid;
    const double* dm = nullptr;
    int64_t ld_td_slot = -1, ld_td_ant = -1, ld_g_slot = -1, ld_g_ant = -1;   // -1: the contiguous [t][r][.] stride
    int32_t dtype = LDPC5G_F32, T = 2, Nr = 2, nfft = 512, carrier_re = 288, scs = 30;
    int64_t hz = 3840000000ll;
};

static int call(const Ofdm& a) {
    const int64_t S = 15 * (int64_t)a.nfft, W = 14 * (int64_t)a.carrier_re;
    const int64_t ts = a.ld_td_slot == -1 ? a.Nr * S : a.ld_td_slot, ta = a.ld_td_ant == -1 ? S : a.ld_td_ant;
    const int64_t gs = a.ld_g_slot == -1 ? a.Nr * W : a.ld_g_slot, ga = a.ld_g_ant == -1 ? W : a.ld_g_ant;
    if (a.demod)
        return ldpc5g_ofdm_demod(a.td, ts, ta, (void*)a.grid, gs, ga, a.dtype, a.T, a.Nr, a.nfft, a.carrier_re, a.scs, a.hz,
                                 nullptr);
    return ldpc5g_ofdm_mod(a.grid, gs, ga, a.dm, (void*)a.td, ts, ta, a.dtype, a.T, a.Nr, a.nfft, a.carrier_re, a.scs, a.hz,
                           nullptr);
}

int main() {
    alignas(16) char buf[64];   // stands for every device buffer: never dereferenced by the validation
    for (bool demod : {true, false}) {
        Ofdm ok;
        ok.demod = demod, ok.td = buf, ok.grid = buf;
        Ofdm a;
        // every supported shape passes every size check (the buffer check comes last)
        int shapes = 0;
        for (int nfft : {128, 256, 512, 1024, 2048, 4096})
            for (int cre = 12; cre <= nfft; cre += 12)
                for (int scs : {15, 30})
                    for (int dt = 0; dt < 2; ++dt)
                        for (int Nr : {1, 2, 4}) {
                            a = ok, a.nfft = nfft, a.carrier_re = cre, a.scs = scs, a.dtype = dt, a.Nr = Nr, a.td = nullptr;
                            REFUSED(a, "null");
                            ++shapes;
                        }
        EXPECT(shapes == 12 * (10 + 21 + 42 + 85 + 170 + 341));
        for (int n : {0, -512, 64, 384, 513, 8192, INT32_MAX, INT32_MIN}) { a = ok, a.nfft = n; REFUSED(a, "nfft"); }
        for (int c : {0, -12, 100, 516, 12 * 276, INT32_MAX, INT32_MIN}) { a = ok, a.carrier_re = c; REFUSED(a, "carrier_re"); }
        a = ok, a.nfft = 128, a.carrier_re = 132; REFUSED(a, "carrier_re");
        for (int s : {0, -15, 60, 120, INT32_MAX}) { a = ok, a.scs = s; REFUSED(a, "scs"); }
        for (int T : {0, -1, 65536, INT32_MAX, INT32_MIN}) { a = ok, a.T = T; REFUSED(a, "T="); }
        for (int n : {0, 3, 8, -1, INT32_MAX}) { a = ok, a.Nr = n; REFUSED(a, demod ? "Nr" : "num_ant"); }
        for (int dt : {-1, 2, 7}) { a = ok, a.dtype = dt; REFUSED(a, "dtype"); }
        for (int64_t ld : {(int64_t)0, (int64_t)15 * 512 - 1, (int64_t)-2, INT64_MIN}) {   // -1 stands for the default here
            a = ok, a.ld_td_slot = ld; REFUSED(a, "ld_td_slot");
            a = ok, a.ld_td_ant = ld; REFUSED(a, "ld_td_ant");
        }
        for (int64_t ld : {(int64_t)0, (int64_t)14 * 288 - 1, (int64_t)-2, INT64_MIN}) {
            a = ok, a.ld_g_slot = ld; REFUSED(a, "ld_g_slot");
            a = ok, a.ld_g_ant = ld; REFUSED(a, "ld_g_ant");
        }
        // a size-1 dimension's stride is not read: any value passes
        a = ok, a.T = 1, a.ld_td_slot = 0, a.ld_g_slot = INT64_MIN, a.grid = nullptr; REFUSED(a, "null");
        a = ok, a.Nr = 1, a.ld_td_slot = 15 * 512, a.ld_g_slot = 14 * 288, a.ld_td_ant = 0, a.ld_g_ant = INT64_MIN, a.grid = nullptr;
        REFUSED(a, "null");
        // the waveform layout [r][slot * S + n] and the largest strides
        a = ok, a.ld_td_slot = 15 * 512, a.ld_td_ant = 2 * 15 * 512, a.td = nullptr; REFUSED(a, "null");
        a = ok, a.ld_td_slot = INT64_MAX, a.ld_td_ant = INT64_MAX, a.ld_g_slot = INT64_MAX, a.ld_g_ant = INT64_MAX, a.td = nullptr;
        REFUSED(a, "null");
        // every carrier frequency is reduced mod the sample rate without overflow
        for (int64_t hz : {(int64_t)0, (int64_t)-3500500000ll, INT64_MAX, INT64_MIN, (int64_t)15360000}) {
            a = ok, a.hz = hz, a.T = 65535, a.Nr = 4, a.td = nullptr; REFUSED(a, "null");
        }
        a = ok, a.td = nullptr; REFUSED(a, "td");
        a = ok, a.grid = nullptr; REFUSED(a, "grid");
        a = ok, a.td = buf + 4; REFUSED(a, "td");
        a = ok, a.grid = buf + 4; REFUSED(a, "grid");
        a = ok, a.dtype = LDPC5G_F64, a.td = buf + 8; REFUSED(a, "td");
        a = ok, a.dtype = LDPC5G_F64, a.grid = buf + 8; REFUSED(a, "grid");
        if (!demod) { a = ok, a.dm = (const double*)(buf + 4); REFUSED(a, "dm"); }
    }
    EXPECT(strlen(ldpc5g_last_error()) > 0);
    if (fails) return 1;
    printf("ofdm_asan_main: ok\n");
    return 0;
}
