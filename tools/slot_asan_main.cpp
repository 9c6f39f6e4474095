// Stand-alone host-sanitizer check of the slot front end's argument validation
// (ldpc5g_slot_rx_frontend, ldpc5g_slot_map): every call below returns before any kernel launch,
// so it needs no GPU.  Build it against the host-sanitized library
// (python -m python_5gtoolbox_amd.build --asan -> build/asan/libldpc5g.so):
//
//   CXX=/opt/rocm/lib/llvm/bin/clang++
//   RT=$(dirname $($CXX --print-file-name=libclang_rt.asan-x86_64.so))
//   $CXX -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -shared-libasan \
//       -Iinclude tools/slot_asan_main.cpp -Lbuild/asan -lldpc5g -Wl,-rpath,$PWD/build/asan \
//       -Wl,-rpath,$RT -o build/asan/slot_asan_main && build/asan/slot_asan_main
//
// Exit status 0 and "slot_asan_main: ok" mean every check held and no sanitizer report.
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

struct Dmrs {   // what both entry points share: 16 PRB at 3 of 24, DMRS symbols [2, 11]
    const int32_t* slots;
    int32_t sym[8] = {2, 11, 0, 0, 0, 0, 0, 0};
    bool null_sym = false;
    int32_t T = 2, carrier_re = 288, rb_start = 3, rb_size = 16, S = 2, nid = 1, nscid = 0, cdm = 2;
};

struct Rx : Dmrs {   // a valid ldpc5g_slot_rx_frontend call: 2x2, complex64
    const void* grid;
    void *h_ls, *y;
    int32_t ports[8] = {0, 1, 2, 3, 0, 0, 0, 0};
    bool null_ports = false;
    int64_t ldgrid = -1, ldh = -1, ldy = -1;
    int32_t dtype = LDPC5G_F32, Nr = 2, Nt = 2;
};

static int call(const Rx& a) {
    const int64_t N = 3 * (int64_t)a.rb_size;
    return ldpc5g_slot_rx_frontend(a.grid, a.ldgrid < 0 ? (int64_t)a.Nr * 14 * a.carrier_re : a.ldgrid, a.dtype, a.slots,
                                   a.T, a.carrier_re, a.rb_start, a.rb_size, a.Nr, a.Nt, a.null_ports ? nullptr : a.ports,
                                   a.S, a.null_sym ? nullptr : a.sym, a.nid, a.nscid, a.cdm, a.h_ls,
                                   a.ldh < 0 ? a.S * N * a.Nr * a.Nt : a.ldh, a.y, a.ldy < 0 ? 14 * 4 * N * a.Nr : a.ldy,
                                   nullptr);
}

struct Map : Dmrs {   // a valid ldpc5g_slot_map call: two layers on two antennas, identity
    const void* sym_buf;
    const int32_t* re_idx;
    void* grid;
    const float* precoding = nullptr;
    int64_t nre = 1920, ldsym = -1, ldgrid = -1;
    int32_t num_ant = 2, NL = 2;
};

static int call(const Map& a) {
    return ldpc5g_slot_map(a.sym_buf, a.ldsym < 0 ? a.nre * a.NL : a.ldsym, a.re_idx, a.nre, a.slots, a.T, a.carrier_re,
                           a.rb_start, a.rb_size, a.num_ant, a.NL, a.precoding, a.S, a.null_sym ? nullptr : a.sym, a.nid,
                           a.nscid, a.cdm, a.grid, a.ldgrid < 0 ? (int64_t)a.num_ant * 14 * a.carrier_re : a.ldgrid,
                           nullptr);
}

template <typename A>
static void shared_checks(const A& ok) {
    A a;
    for (int S : {0, 5, -1, INT32_MAX}) { a = ok, a.S = S; REFUSED(a, "S="); }
    a = ok, a.sym[0] = 11, a.sym[1] = 2; REFUSED(a, "sym_idx");
    a = ok, a.sym[1] = 2; REFUSED(a, "sym_idx");
    a = ok, a.sym[1] = 14; REFUSED(a, "sym_idx");
    a = ok, a.sym[0] = -1; REFUSED(a, "sym_idx");
    a = ok, a.null_sym = true; REFUSED(a, "sym_idx");
    for (int rb : {0, -1, 276, INT32_MAX}) { a = ok, a.rb_size = rb; REFUSED(a, "rb_size"); }
    for (int st : {9, -1, 24, INT32_MAX}) { a = ok, a.rb_start = st; REFUSED(a, "rb_start"); }
    for (int cre : {0, 287, 12 * 276, -12, INT32_MAX}) { a = ok, a.carrier_re = cre, a.rb_start = 0, a.rb_size = 1; REFUSED(a, "carrier_re"); }
    for (int nid : {-1, 65536}) { a = ok, a.nid = nid; REFUSED(a, "nNIDnSCID"); }
    for (int ns : {-1, 2}) { a = ok, a.nscid = ns; REFUSED(a, "nSCID"); }
    for (int cdm : {0, 3, -1}) { a = ok, a.cdm = cdm; REFUSED(a, "num_cdm_groups"); }
    for (int T : {0, -1, 65536}) { a = ok, a.T = T; REFUSED(a, "T="); }
    a = ok, a.slots = nullptr; REFUSED(a, "null");
    a = ok, a.grid = nullptr; REFUSED(a, "null");
    for (int T : {1, 2}) { a = ok, a.T = T, a.ldgrid = 2 * 14 * 288 - 1; REFUSED(a, "stride"); }
    // the largest carrier and allocation pass every size check
    a = ok, a.carrier_re = 12 * 275, a.rb_start = 0, a.rb_size = 275, a.slots = nullptr; REFUSED(a, "null");
}

int main() {
    alignas(16) char buf[64];   // stands for every device buffer: never dereferenced by the validation
    Rx ok;
    ok.grid = buf, ok.h_ls = ok.y = buf, ok.slots = (const int32_t*)buf;
    Rx a;

    // every supported shape / dtype / S passes the checks up to the buffer check, with either half
    for (int Nr : {1, 2, 4})
        for (int Nt = 1; Nt <= 4; ++Nt)
            for (int dt = 0; dt < 2; ++dt)
                for (int S = 1; S <= 4; ++S)
                    for (int half = 0; half < 3; ++half) {
                        a = ok, a.Nr = Nr, a.Nt = Nt, a.dtype = dt, a.S = S;
                        a.sym[0] = 2, a.sym[1] = 5, a.sym[2] = 8, a.sym[3] = 11;
                        if (half == 1) a.h_ls = nullptr;
                        if (half == 2) a.y = nullptr;
                        a.slots = nullptr;
                        REFUSED(a, "null");
                    }
    shared_checks(ok);
    for (int Nr : {0, 3, 8, -1, INT32_MAX}) { a = ok, a.Nr = Nr; REFUSED(a, "Nr"); }
    for (int Nt : {0, 5, -1, INT32_MAX}) { a = ok, a.Nt = Nt; REFUSED(a, "Nt"); }
    a = ok, a.ports[1] = 4; REFUSED(a, "ports");
    a = ok, a.ports[0] = -1; REFUSED(a, "ports");
    a = ok, a.ports[1] = 0; REFUSED(a, "ports");
    a = ok, a.null_ports = true; REFUSED(a, "ports");
    for (int dt : {-1, 2, 7}) { a = ok, a.dtype = dt; REFUSED(a, "dtype"); }
    for (int T : {1, 2}) {
        a = ok, a.T = T, a.ldh = 2 * 48 * 4 - 1; REFUSED(a, "stride");
        a = ok, a.T = T, a.ldy = 14 * 192 * 2 - 1; REFUSED(a, "stride");
    }
    a = ok, a.h_ls = a.y = nullptr; REFUSED(a, "null");
    a = ok, a.dtype = LDPC5G_F64, a.grid = buf + 8; REFUSED(a, "aligned");
    a = ok, a.y = buf + 4; REFUSED(a, "aligned");

    Map mok;
    mok.sym_buf = buf, mok.re_idx = (const int32_t*)buf, mok.grid = buf, mok.slots = (const int32_t*)buf;
    Map m;
    shared_checks(mok);
    for (int na : {0, 3, 8, -1}) { m = mok, m.num_ant = na; REFUSED(m, "num_ant"); }
    for (int NL : {0, 5, -1}) { m = mok, m.NL = NL; REFUSED(m, "NL"); }
    m = mok, m.NL = 4; REFUSED(m, "precoding");
    float w[32] = {};
    for (int na : {1, 2, 4})
        for (int NL = 1; NL <= 4; ++NL) { m = mok, m.num_ant = na, m.NL = NL, m.precoding = w, m.grid = nullptr; REFUSED(m, "null"); }
    for (int64_t nre : {(int64_t)-1, (int64_t)14 * 192 + 1, INT64_MAX}) { m = mok, m.nre = nre, m.ldsym = INT64_MAX; REFUSED(m, "nre"); }
    for (int T : {1, 2}) { m = mok, m.T = T, m.ldsym = 1920 * 2 - 1; REFUSED(m, "stride"); }
    m = mok, m.sym_buf = nullptr; REFUSED(m, "null");
    m = mok, m.re_idx = nullptr; REFUSED(m, "null");
    m = mok, m.nre = 0, m.sym_buf = nullptr, m.re_idx = nullptr, m.grid = nullptr; REFUSED(m, "null");
    m = mok, m.grid = buf + 4; REFUSED(m, "aligned");
    EXPECT(strlen(ldpc5g_last_error()) > 0);
    if (fails) return 1;
    printf("slot_asan_main: ok\n");
    return 0;
}
