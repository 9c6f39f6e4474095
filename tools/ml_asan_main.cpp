// Stand-alone host-sanitizer check of the ML detectors' argument validation (ldpc5g_ml_detect):
// every call below returns before any kernel launch, so it needs no GPU.  Build it against the
// host-sanitized library (python -m python_5gtoolbox_amd.build --asan -> build/asan/libldpc5g.so):
//
//   CXX=/opt/rocm/lib/llvm/bin/clang++
//   RT=$(dirname $($CXX --print-file-name=libclang_rt.asan-x86_64.so))
//   $CXX -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -shared-libasan \
//       -Iinclude tools/ml_asan_main.cpp -Lbuild/asan -lldpc5g -Wl,-rpath,$PWD/build/asan \
//       -Wl,-rpath,$RT -o build/asan/ml_asan_main && build/asan/ml_asan_main
//
// Exit status 0 and "ml_asan_main: ok" mean every check held and no sanitizer report.
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

struct Args {   // a valid call: T = 2, R = 72, (Nr, NL) = (4, 2), 16QAM, ML-IRC-soft, complex128, all REs
    const void *y, *h, *cov;
    void* llr;
    void *sym = nullptr, *nv = nullptr;
    int8_t* hb = nullptr;
    const uint32_t* prbs = nullptr;
    const int32_t* re_idx = nullptr;
    int64_t R = 72, nre = 72, ldy = -1, ldh = -1, ldcov = -1, ldllr = -1, ldsym = -1, ldnv = -1, ldhb = -1, ldw = -1;
    int32_t dtype = LDPC5G_F64, llr_dtype = LDPC5G_F64, rpc = 12, T = 2, Nr = 4, NL = 2, mod = 4,
            algo = LDPC5G_ML_SOFT, irc = 1;
};

static int call(const Args& a) {
    const int64_t ncov = a.rpc > 0 ? (a.R + a.rpc - 1) / a.rpc : 1;
    const int Qm = a.mod < 0 ? 1 : a.mod;
    const int64_t nb = a.nre * a.NL * Qm;
    return ldpc5g_ml_detect(a.y, a.ldy < 0 ? a.R * a.Nr : a.ldy, a.h, a.ldh < 0 ? a.R * a.Nr * a.NL : a.ldh, a.cov,
                            a.ldcov < 0 ? ncov * a.Nr * a.Nr : a.ldcov, a.dtype, a.re_idx, a.R, a.nre, a.rpc, a.T,
                            a.Nr, a.NL, a.mod, a.algo, a.irc, a.prbs, a.ldw < 0 ? (nb + 31) / 32 : a.ldw, a.llr,
                            a.llr_dtype, a.ldllr < 0 ? nb : a.ldllr, a.sym, a.ldsym < 0 ? a.nre * a.NL : a.ldsym,
                            a.nv, a.ldnv < 0 ? a.nre * a.NL : a.ldnv, a.hb, a.ldhb < 0 ? nb : a.ldhb, nullptr);
}

int main() {
    char buf[64];   // stands for every device buffer: never dereferenced by the validation
    Args ok;
    ok.y = ok.h = ok.cov = buf, ok.llr = buf;
    const int32_t* IDX = (const int32_t*)buf;
    Args a;

    // every supported shape / modulation / algorithm / irc / dtype passes up to the buffer check,
    // every combination over the exhaustive cap is refused with the way out named
    const int shapes[7][2] = {{1, 1}, {2, 1}, {2, 2}, {4, 1}, {4, 2}, {4, 3}, {4, 4}};
    for (const auto& s : shapes)
        for (int mod : {-1, 1, 2, 4, 6, 8, 10})
            for (int algo = 0; algo < 5; ++algo)
                for (int irc = 0; irc < 2; ++irc)
                    for (int dt = 0; dt < 2; ++dt) {
                        a = ok, a.Nr = s[0], a.NL = s[1], a.mod = mod, a.algo = algo, a.irc = irc, a.dtype = dt;
                        a.llr_dtype = dt, a.y = nullptr;
                        const int Qm = mod < 0 ? 1 : mod;
                        const bool exhaustive = algo <= LDPC5G_ML2_SOFT || (algo == LDPC5G_ML_OPT_RANK2 && s[1] != 2);
                        EXPECT(call(a) == LDPC5G_ESIZE);
                        if (exhaustive && s[1] * Qm > 16)
                            EXPECT(strstr(ldpc5g_last_error(), "opt-rank2-ML") != nullptr);
                        else
                            EXPECT(strstr(ldpc5g_last_error(), "null") != nullptr);
                    }
    const int bad_shapes[8][2] = {{3, 1}, {8, 2}, {0, 0}, {2, 3}, {4, 5}, {4, 0}, {1, 2}, {-1, 1}};
    for (const auto& s : bad_shapes) {
        a = ok, a.Nr = s[0], a.NL = s[1];
        EXPECT(call(a) == LDPC5G_ESIZE);
        EXPECT(strstr(ldpc5g_last_error(), "Nr") != nullptr);
    }
    for (int mod : {0, 3, 5, 12, -2, INT32_MIN}) { a = ok, a.mod = mod; EXPECT(call(a) == LDPC5G_ESIZE); }
    for (int algo : {-1, 5, 1 << 30}) { a = ok, a.algo = algo; EXPECT(call(a) == LDPC5G_ESIZE); }
    for (int irc : {-1, 2}) { a = ok, a.irc = irc; EXPECT(call(a) == LDPC5G_ESIZE); }
    for (int dt : {-1, 2, 7}) {
        a = ok, a.dtype = dt; EXPECT(call(a) == LDPC5G_ESIZE);
        a = ok, a.llr_dtype = dt; EXPECT(call(a) == LDPC5G_ESIZE);
    }
    for (int rpc : {0, -12, INT32_MIN}) { a = ok, a.rpc = rpc; EXPECT(call(a) == LDPC5G_ESIZE); }
    // sizes
    a = ok, a.T = 0; EXPECT(call(a) == LDPC5G_ESIZE);
    a = ok, a.T = -1; EXPECT(call(a) == LDPC5G_ESIZE);
    a = ok, a.T = 1 << 20; EXPECT(call(a) == LDPC5G_ESIZE);
    a = ok, a.R = 0, a.nre = 0; EXPECT(call(a) == LDPC5G_ESIZE);
    a = ok, a.R = -5; EXPECT(call(a) == LDPC5G_ESIZE);
    a = ok, a.R = int64_t(1) << 31, a.nre = 1, a.re_idx = IDX; EXPECT(call(a) == LDPC5G_ESIZE);
    a = ok, a.re_idx = IDX, a.nre = 0; EXPECT(call(a) == LDPC5G_ESIZE);
    a = ok, a.re_idx = IDX, a.nre = -1; EXPECT(call(a) == LDPC5G_ESIZE);
    a = ok, a.re_idx = IDX, a.nre = 73; EXPECT(call(a) == LDPC5G_ESIZE);
    a = ok, a.nre = 54; EXPECT(call(a) == LDPC5G_ESIZE);   // NULL re_idx means all R
    // strides, T = 1 included; the optional outputs only when given
    for (int T : {1, 2}) {
        a = ok, a.T = T, a.ldy = 72 * 4 - 1; EXPECT(call(a) == LDPC5G_ESIZE);
        a = ok, a.T = T, a.ldh = 72 * 8 - 1; EXPECT(call(a) == LDPC5G_ESIZE);
        a = ok, a.T = T, a.ldcov = 6 * 16 - 1; EXPECT(call(a) == LDPC5G_ESIZE);
        a = ok, a.T = T, a.ldllr = 72 * 8 - 1; EXPECT(call(a) == LDPC5G_ESIZE);
        a = ok, a.T = T, a.sym = buf, a.ldsym = 72 * 2 - 1; EXPECT(call(a) == LDPC5G_ESIZE);
        a = ok, a.T = T, a.nv = buf, a.ldnv = 72 * 2 - 1; EXPECT(call(a) == LDPC5G_ESIZE);
        a = ok, a.T = T, a.hb = (int8_t*)buf, a.ldhb = 72 * 8 - 1; EXPECT(call(a) == LDPC5G_ESIZE);
        a = ok, a.T = T, a.prbs = (const uint32_t*)buf, a.ldw = 72 * 8 / 32 - 1; EXPECT(call(a) == LDPC5G_ESIZE);
        EXPECT(strstr(ldpc5g_last_error(), "stride") != nullptr);
    }
    a = ok, a.R = 73, a.nre = 73, a.ldcov = 6 * 16; EXPECT(call(a) == LDPC5G_ESIZE);   // a 7th covariance block
    // null buffers
    a = ok, a.h = nullptr; EXPECT(call(a) == LDPC5G_ESIZE);
    a = ok, a.cov = nullptr; EXPECT(call(a) == LDPC5G_ESIZE);
    a = ok, a.llr = nullptr; EXPECT(call(a) == LDPC5G_ESIZE);
    EXPECT(strlen(ldpc5g_last_error()) > 0);
    if (fails) return 1;
    printf("ml_asan_main: ok\n");
    return 0;
}
