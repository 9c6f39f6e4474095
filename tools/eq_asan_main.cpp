// Stand-alone host-sanitizer check of the equaliser's argument validation (ldpc5g_equalize): every
// call below returns before any kernel launch, so it needs no GPU.  Build it against the
// host-sanitized library (python -m python_5gtoolbox_amd.build --asan -> build/asan/libldpc5g.so):
//
//   CXX=/opt/rocm/lib/llvm/bin/clang++
//   RT=$(dirname $($CXX --print-file-name=libclang_rt.asan-x86_64.so))
//   $CXX -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -shared-libasan \
//       -Iinclude tools/eq_asan_main.cpp -Lbuild/asan -lldpc5g -Wl,-rpath,$PWD/build/asan \
//       -Wl,-rpath,$RT -o build/asan/eq_asan_main && build/asan/eq_asan_main
//
// Exit status 0 and "eq_asan_main: ok" mean every check held and no sanitizer report.
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

struct Args {   // a valid call: T = 2, R = 72, (Nr, NL) = (4, 2), MMSE-IRC, complex128, all REs
    const void *y, *h, *cov;
    void* sym;
    float* nv;
    const int32_t* re_idx = nullptr;
    int64_t R = 72, nre = 72, ldy = -1, ldh = -1, ldcov = -1, ldsym = -1, ldnv = -1;
    int32_t dtype = LDPC5G_F64, rpc = 12, T = 2, Nr = 4, NL = 2, algo = LDPC5G_EQ_MMSE_IRC;
};

static int call(const Args& a) {
    const int64_t ncov = a.rpc > 0 ? (a.R + a.rpc - 1) / a.rpc : 1;
    return ldpc5g_equalize(a.y, a.ldy < 0 ? a.R * a.Nr : a.ldy, a.h, a.ldh < 0 ? a.R * a.Nr * a.NL : a.ldh, a.cov,
                           a.ldcov < 0 ? ncov * a.Nr * a.Nr : a.ldcov, a.dtype, a.re_idx, a.R, a.nre, a.rpc, a.T,
                           a.Nr, a.NL, a.algo, a.sym, a.ldsym < 0 ? a.nre * a.NL : a.ldsym, a.nv,
                           a.ldnv < 0 ? a.nre * a.NL : a.ldnv, nullptr);
}

int main() {
    char buf[64];   // stands for every device buffer: never dereferenced by the validation
    Args ok;
    ok.y = ok.h = ok.cov = buf, ok.sym = buf, ok.nv = (float*)buf;
    const int32_t* IDX = (const int32_t*)buf;
    Args a;

    // every supported shape / algorithm / dtype passes the checks up to the buffer check
    const int shapes[7][2] = {{1, 1}, {2, 1}, {2, 2}, {4, 1}, {4, 2}, {4, 3}, {4, 4}};
    for (const auto& s : shapes)
        for (int algo = 0; algo < 4; ++algo)
            for (int dt = 0; dt < 2; ++dt) {
                a = ok, a.Nr = s[0], a.NL = s[1], a.algo = algo, a.dtype = dt, a.y = nullptr;
                EXPECT(call(a) == LDPC5G_ESIZE);
                EXPECT(strstr(ldpc5g_last_error(), "null") != nullptr);
            }
    // unsupported shapes
    const int bad_shapes[8][2] = {{3, 1}, {8, 2}, {0, 0}, {2, 3}, {4, 5}, {4, 0}, {1, 2}, {-1, 1}};
    for (const auto& s : bad_shapes) {
        a = ok, a.Nr = s[0], a.NL = s[1];
        EXPECT(call(a) == LDPC5G_ESIZE);
        EXPECT(strstr(ldpc5g_last_error(), "Nr") != nullptr);
    }
    for (int algo : {-1, 4, 1 << 30}) { a = ok, a.algo = algo; EXPECT(call(a) == LDPC5G_ESIZE); }
    for (int dt : {-1, 2, 7}) { a = ok, a.dtype = dt; EXPECT(call(a) == LDPC5G_ESIZE); }
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
    // strides, T = 1 included
    for (int T : {1, 2}) {
        a = ok, a.T = T, a.ldy = 72 * 4 - 1; EXPECT(call(a) == LDPC5G_ESIZE);
        a = ok, a.T = T, a.ldh = 72 * 8 - 1; EXPECT(call(a) == LDPC5G_ESIZE);
        a = ok, a.T = T, a.ldcov = 6 * 16 - 1; EXPECT(call(a) == LDPC5G_ESIZE);
        a = ok, a.T = T, a.ldsym = 72 * 2 - 1; EXPECT(call(a) == LDPC5G_ESIZE);
        a = ok, a.T = T, a.ldnv = 72 * 2 - 1; EXPECT(call(a) == LDPC5G_ESIZE);
        EXPECT(strstr(ldpc5g_last_error(), "stride") != nullptr);
    }
    a = ok, a.R = 73, a.nre = 73, a.ldcov = 6 * 16; EXPECT(call(a) == LDPC5G_ESIZE);   // a 7th covariance block
    // null buffers
    a = ok, a.h = nullptr; EXPECT(call(a) == LDPC5G_ESIZE);
    a = ok, a.cov = nullptr; EXPECT(call(a) == LDPC5G_ESIZE);
    a = ok, a.sym = nullptr; EXPECT(call(a) == LDPC5G_ESIZE);
    a = ok, a.nv = nullptr; EXPECT(call(a) == LDPC5G_ESIZE);
    EXPECT(strlen(ldpc5g_last_error()) > 0);
    if (fails) return 1;
    printf("eq_asan_main: ok\n");
    return 0;
}
