// Stand-alone host-sanitizer check of the channel estimator's argument validation
// (ldpc5g_channel_estimate, ldpc5g_to_compensate): every call below returns before any kernel
// launch, so it needs no GPU.  Build it against the host-sanitized library
// (python -m python_5gtoolbox_amd.build --asan -> build/asan/libldpc5g.so):
//
//   CXX=/opt/rocm/lib/llvm/bin/clang++
//   RT=$(dirname $($CXX --print-file-name=libclang_rt.asan-x86_64.so))
//   $CXX -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -shared-libasan \
//       -Iinclude tools/ce_asan_main.cpp -Lbuild/asan -lldpc5g -Wl,-rpath,$PWD/build/asan \
//       -Wl,-rpath,$RT -o build/asan/ce_asan_main && build/asan/ce_asan_main
//
// Exit status 0 and "ce_asan_main: ok" mean every check held and no sanitizer report.
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

struct Args {   // a valid call: T = 2, 20 PRB (N = 60, D = 4), 4x2, [2, 11], DFT_symmetric (M = 168)
    const void* h_ls;
    void *h, *cov, *work, *h_ls_comp = nullptr;
    int32_t sym[8] = {2, 11, 0, 0, 0, 0, 0, 0};
    const int32_t* sym_ptr = nullptr;   // nullptr: use sym
    bool null_sym = false;
    int64_t ldhls = -1, ldh = -1, ldcov = -1, ldhc = -1, work_bytes = -1;
    int32_t dtype = LDPC5G_F64, T = 2, S = 2, N = 60, Nr = 4, Nt = 2, D = 4, algo = LDPC5G_CE_DFT_SYMMETRIC, eK = 12,
            L_left = 28, L_right = 28, cdm = 2, to_comp = 0, scs = 30;
};

static int call(const Args& a) {
    const int64_t NE = (int64_t)a.Nr * a.Nt;
    const int64_t ws = a.work_bytes >= 0 ? a.work_bytes : ldpc5g_ce_workspace_bytes(a.T, a.S, a.N, a.Nr, a.Nt, a.D);
    return ldpc5g_channel_estimate(
        a.h_ls, a.ldhls < 0 ? (int64_t)a.S * a.N * NE : a.ldhls, a.dtype, a.T, a.S, a.N, a.Nr, a.Nt, a.D,
        a.null_sym ? nullptr : a.sym, a.algo, a.eK, a.L_left, a.L_right, a.cdm, a.to_comp, a.scs, a.h,
        a.ldh < 0 ? 14 * (int64_t)a.N * a.D * NE : a.ldh, a.cov,
        a.ldcov < 0 ? 14 * ((int64_t)a.N * a.D / 12) * a.Nr * a.Nr : a.ldcov, a.work, ws, a.h_ls_comp,
        a.ldhc < 0 ? (int64_t)a.S * a.N * NE : a.ldhc, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}

struct Comp {   // a valid ldpc5g_to_compensate call
    const void* y;
    void* out;
    const double* to_avg;
    int64_t ldy = -1, ldo = -1, nsym = 12, RE = 240;
    int32_t dtype = LDPC5G_F32, T = 2, Nr = 2, scs = 30;
};

static int call(const Comp& c) {
    return ldpc5g_to_compensate(c.y, c.ldy < 0 ? c.nsym * c.RE * c.Nr : c.ldy, c.out,
                                c.ldo < 0 ? c.nsym * c.RE * c.Nr : c.ldo, c.dtype, c.to_avg, c.T, c.nsym, c.RE, c.Nr,
                                c.scs, nullptr);
}

int main() {
    char buf[64], buf2[64];   // stand for every device buffer: never dereferenced by the validation
    Args ok;
    ok.h_ls = buf, ok.h = ok.cov = ok.work = buf;
    Args a;

    // every supported shape / algorithm / dtype / D / S passes the checks up to the buffer check
    const int shapes[7][2] = {{1, 1}, {2, 1}, {2, 2}, {4, 1}, {4, 2}, {4, 3}, {4, 4}};
    for (const auto& s : shapes)
        for (int algo = 0; algo < 4; ++algo)
            for (int dt = 0; dt < 2; ++dt)
                for (int D : {2, 4})
                    for (int S = 1; S <= 4; ++S) {
                        a = ok, a.Nr = s[0], a.Nt = s[1], a.algo = algo, a.dtype = dt, a.D = D, a.N = D == 2 ? 96 : 60;
                        a.S = S, a.sym[0] = 2, a.sym[1] = 5, a.sym[2] = 8, a.sym[3] = 11, a.L_left = a.L_right = 10;
                        a.h = nullptr;
                        REFUSED(a, "null");
                    }
    const int bad_shapes[7][2] = {{3, 1}, {8, 2}, {0, 0}, {2, 3}, {4, 5}, {4, 0}, {1, 2}};
    for (const auto& s : bad_shapes) { a = ok, a.Nr = s[0], a.Nt = s[1]; REFUSED(a, "Nr"); }
    for (int S : {0, 5, -1, INT32_MAX}) { a = ok, a.S = S; REFUSED(a, "S="); }
    a = ok, a.sym[0] = 11, a.sym[1] = 2; REFUSED(a, "sym_idx");
    a = ok, a.sym[1] = 2; REFUSED(a, "sym_idx");
    a = ok, a.sym[1] = 14; REFUSED(a, "sym_idx");
    a = ok, a.sym[0] = -1; REFUSED(a, "sym_idx");
    a = ok, a.null_sym = true; REFUSED(a, "sym_idx");
    for (int D : {3, 1, 0, 6, -4}) { a = ok, a.D = D; REFUSED(a, "D="); }
    a = ok, a.N = 45; REFUSED(a, "PRB");
    a = ok, a.N = 61; REFUSED(a, "multiple of 12");
    for (int N : {0, -60, INT32_MAX}) { a = ok, a.N = N, a.work_bytes = 1 << 20; REFUSED(a, "N="); }
    a = ok, a.N = 825, a.eK = 201; REFUSED(a, "M=");
    a = ok, a.N = 2040, a.algo = LDPC5G_CE_DFT; REFUSED(a, "M=");
    a = ok, a.eK = INT32_MAX; REFUSED(a, "eK");
    a = ok, a.eK = -1; REFUSED(a, "eK");
    a = ok, a.N = 825, a.eK = 24, a.L_left = a.L_right = 100, a.cov = nullptr; REFUSED(a, "null");   // M = 1748
    const int Ls[6][2] = {{84, 84}, {168, 0}, {0, 168}, {-1, 5}, {5, -1}, {INT32_MAX, INT32_MAX}};
    for (const auto& l : Ls) { a = ok, a.L_left = l[0], a.L_right = l[1]; REFUSED(a, "L_left"); }
    for (int dt : {-1, 2, 7}) { a = ok, a.dtype = dt; REFUSED(a, "dtype"); }
    for (int algo : {-1, 4, 1 << 30}) { a = ok, a.algo = algo; REFUSED(a, "algo"); }
    for (int scs : {0, 60, 120, -15}) { a = ok, a.scs = scs; REFUSED(a, "scs"); }
    for (int cdm : {0, 4, -1}) { a = ok, a.cdm = cdm; REFUSED(a, "num_cdm_groups"); }
    for (int T : {0, -1, 1 << 20}) { a = ok, a.T = T, a.work_bytes = 1 << 30; REFUSED(a, "T="); }
    for (int T : {1, 2}) {
        a = ok, a.T = T, a.ldhls = 2 * 60 * 8 - 1; REFUSED(a, "stride");
        a = ok, a.T = T, a.ldh = 14 * 240 * 8 - 1; REFUSED(a, "stride");
        a = ok, a.T = T, a.ldcov = 14 * 20 * 16 - 1; REFUSED(a, "stride");
        a = ok, a.T = T, a.to_comp = 1, a.h_ls_comp = buf2, a.ldhc = 2 * 60 * 8 - 1; REFUSED(a, "stride");
    }
    a = ok, a.work_bytes = ldpc5g_ce_workspace_bytes(2, 2, 60, 4, 2, 4) - 1; REFUSED(a, "workspace");
    EXPECT(ldpc5g_ce_workspace_bytes(0, 2, 60, 4, 2, 4) == 0);
    a = ok, a.h_ls = nullptr; REFUSED(a, "null");
    a = ok, a.h = nullptr; REFUSED(a, "null");
    a = ok, a.cov = nullptr; REFUSED(a, "null");
    a = ok, a.work = nullptr; REFUSED(a, "null");
    a = ok, a.h_ls_comp = buf2; REFUSED(a, "h_ls_comp");
    a = ok, a.to_comp = 1, a.h_ls_comp = buf; REFUSED(a, "overlap");

    Comp cok;
    cok.y = buf, cok.out = buf, cok.to_avg = (const double*)buf2;
    Comp c;
    c = cok, c.y = nullptr; REFUSED(c, "null");
    c = cok, c.out = nullptr; REFUSED(c, "null");
    c = cok, c.to_avg = nullptr; REFUSED(c, "null");
    for (int Nr : {0, -1, 65}) { c = cok, c.Nr = Nr; REFUSED(c, "Nr"); }
    for (int dt : {-1, 2}) { c = cok, c.dtype = dt; REFUSED(c, "dtype"); }
    for (int scs : {0, 60}) { c = cok, c.scs = scs; REFUSED(c, "scs"); }
    c = cok, c.T = 0; REFUSED(c, "sizes");
    c = cok, c.T = 1 << 20; REFUSED(c, "sizes");
    c = cok, c.nsym = 0; REFUSED(c, "sizes");
    c = cok, c.nsym = INT64_MAX, c.ldy = c.ldo = 1; REFUSED(c, "sizes");
    c = cok, c.RE = 0; REFUSED(c, "sizes");
    c = cok, c.RE = INT64_MAX, c.ldy = c.ldo = 1; REFUSED(c, "sizes");
    for (int T : {1, 2}) {
        c = cok, c.T = T, c.ldy = 12 * 240 * 2 - 1; REFUSED(c, "stride");
        c = cok, c.T = T, c.ldo = 12 * 240 * 2 - 1; REFUSED(c, "stride");
    }
    EXPECT(strlen(ldpc5g_last_error()) > 0);
    if (fails) return 1;
    printf("ce_asan_main: ok\n");
    return 0;
}
