// Stand-alone host-sanitizer check of the argument validation of PUSCH transform precoding
// (ldpc5g_transform_precode, ldpc5g_low_papr_seq, ldpc5g_slot_rx_frontend_tp, ldpc5g_slot_map_tp):
// every call below returns before any kernel launch, so it needs no GPU.  Build it against the
// host-sanitized library (python -m python_5gtoolbox_amd.build --asan -> build/asan/libldpc5g.so):
//
//   CXX=/opt/rocm/lib/llvm/bin/clang++
//   RT=$(dirname $($CXX --print-file-name=libclang_rt.asan-x86_64.so))
//   $CXX -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -shared-libasan \
//       -Iinclude tools/tp_asan_main.cpp -Lbuild/asan -lldpc5g -Wl,-rpath,$PWD/build/asan \
//       -Wl,-rpath,$RT -o build/asan/tp_asan_main && build/asan/tp_asan_main
//
// Exit status 0 and "tp_asan_main: ok" mean every check held and no sanitizer report.
#include <math.h>
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

struct Dft {   // a valid ldpc5g_transform_precode call: 16 PRB, three symbols, in place
    const void* x;
    void* out;
    int64_t ldx = -1, ldo = -1;
    int32_t dtype = LDPC5G_F32, T = 2, nsym = 3, rb_size = 16, inverse = 0;
};

static int call(const Dft& a) {
    const int64_t row = (int64_t)a.nsym * 12 * a.rb_size;
    return ldpc5g_transform_precode(a.x, a.ldx < 0 ? row : a.ldx, a.out, a.ldo < 0 ? row : a.ldo, a.dtype, a.T, a.nsym,
                                    a.rb_size, a.inverse, nullptr);
}

struct Seq {   // a valid ldpc5g_low_papr_seq call
    const int32_t *u, *v;
    void* out;
    int32_t n = 3, MZC = 72;
    double alpha = 0.0;
};

static int call(const Seq& a) { return ldpc5g_low_papr_seq(a.u, a.v, a.n, a.alpha, a.MZC, a.out, nullptr); }

struct Dmrs {   // what the two slot entry points share: 16 PRB at 3 of 24, DMRS symbols [2, 11], group hopping
    const int32_t* slots;
    const void* base_seq = nullptr;
    int32_t sym[8] = {2, 11, 0, 0, 0, 0, 0, 0};
    bool null_sym = false;
    int32_t T = 2, carrier_re = 288, rb_start = 3, rb_size = 16, port = 0, S = 2, nid = 77, hopping = 1;
};

struct Rx : Dmrs {   // a valid ldpc5g_slot_rx_frontend_tp call: 1x2, complex64
    const void* grid;
    void *h_ls, *y;
    int64_t ldgrid = -1, ldh = -1, ldy = -1;
    int32_t dtype = LDPC5G_F32, Nr = 2;
};

static int call(const Rx& a) {
    const int64_t N = 3 * (int64_t)a.rb_size;
    return ldpc5g_slot_rx_frontend_tp(a.grid, a.ldgrid < 0 ? (int64_t)a.Nr * 14 * a.carrier_re : a.ldgrid, a.dtype, a.slots,
                                      a.T, a.carrier_re, a.rb_start, a.rb_size, a.Nr, a.port, a.S,
                                      a.null_sym ? nullptr : a.sym, a.nid, a.hopping, a.base_seq, a.h_ls,
                                      a.ldh < 0 ? a.S * N * a.Nr : a.ldh, a.y, a.ldy < 0 ? 14 * 4 * N * a.Nr : a.ldy, nullptr);
}

struct Map : Dmrs {   // a valid ldpc5g_slot_map_tp call: one layer on two antennas, identity
    const void* sym_buf;
    const int32_t* re_idx;
    void* grid;
    const float* precoding = nullptr;
    int64_t nre = 1920, ldsym = -1, ldgrid = -1;
    int32_t num_ant = 2;
};

static int call(const Map& a) {
    return ldpc5g_slot_map_tp(a.sym_buf, a.ldsym < 0 ? a.nre : a.ldsym, a.re_idx, a.nre, a.slots, a.T, a.carrier_re,
                              a.rb_start, a.rb_size, a.num_ant, a.port, a.precoding, a.S, a.null_sym ? nullptr : a.sym,
                              a.nid, a.hopping, a.base_seq, a.grid,
                              a.ldgrid < 0 ? (int64_t)a.num_ant * 14 * a.carrier_re : a.ldgrid, nullptr);
}

static bool smooth(int n) {
    for (int f : {2, 3, 5})
        while (n % f == 0) n /= f;
    return n == 1;
}

template <typename A>
static void shared_checks(const A& ok, const void* buf) {
    A a;
    for (int rb : {0, -1, 7, 11, 14, 276, INT32_MAX}) { a = ok, a.rb_start = 0, a.rb_size = rb; REFUSED(a, "rb_size"); }
    for (int st : {9, -1, 24, INT32_MAX}) { a = ok, a.rb_start = st; REFUSED(a, "rb_start"); }
    for (int cre : {0, 287, 12 * 276, -12, INT32_MAX}) { a = ok, a.carrier_re = cre, a.rb_start = 0; REFUSED(a, "carrier_re"); }
    for (int h : {-1, 3, INT32_MAX}) { a = ok, a.hopping = h; REFUSED(a, "hopping"); }
    for (int id : {-1, 1008, INT32_MAX}) { a = ok, a.nid = id; REFUSED(a, "nPuschID"); }
    for (int p : {-1, 4}) { a = ok, a.port = p; REFUSED(a, "port"); }
    for (int rb : {1, 2, 3, 4}) { a = ok, a.rb_size = rb; REFUSED(a, "base_seq"); }
    a = ok, a.base_seq = (const char*)buf + 8; REFUSED(a, "base_seq");
    for (int S : {0, 5, -1, INT32_MAX}) { a = ok, a.S = S; REFUSED(a, "S="); }
    a = ok, a.sym[0] = 11, a.sym[1] = 2; REFUSED(a, "sym_idx");
    a = ok, a.sym[1] = 14; REFUSED(a, "sym_idx");
    a = ok, a.null_sym = true; REFUSED(a, "sym_idx");
    for (int T : {0, -1, 65536}) { a = ok, a.T = T; REFUSED(a, "T="); }
    a = ok, a.slots = nullptr; REFUSED(a, "null");
    a = ok, a.grid = nullptr; REFUSED(a, "null");
    for (int T : {1, 2}) { a = ok, a.T = T, a.ldgrid = 2 * 14 * 288 - 1; REFUSED(a, "stride"); }
    // every allocation 2^a 3^b 5^c passes every size check, with base_seq where it is required
    for (int rb = 1; rb <= 275; ++rb)
        if (smooth(rb)) {
            a = ok, a.carrier_re = 12 * 275, a.rb_start = 0, a.rb_size = rb, a.base_seq = rb <= 4 ? buf : nullptr;
            a.slots = nullptr;
            REFUSED(a, "null");
        }
}

int main() {
    alignas(16) char buf[64];   // stands for every device buffer: never dereferenced by the validation
    Dft dok;
    dok.x = buf, dok.out = buf;
    Dft d;
    int lengths = 0;
    for (int rb = 1; rb <= 275; ++rb)
        for (int dt = 0; dt < 2; ++dt)
            for (int inv = 0; inv < 2; ++inv) {
                d = dok, d.rb_size = rb, d.dtype = dt, d.inverse = inv, d.nsym = 14, d.x = nullptr;
                if (smooth(rb)) { REFUSED(d, "null"); lengths += dt == 0 && inv == 0; } else { REFUSED(d, "rb_size"); }
            }
    EXPECT(lengths == 53);
    for (int rb : {0, -1, 276, INT32_MAX}) { d = dok, d.rb_size = rb; REFUSED(d, "rb_size"); }
    for (int T : {0, -1, 65536}) { d = dok, d.T = T; REFUSED(d, "T="); }
    for (int n : {0, 15, -1}) { d = dok, d.nsym = n; REFUSED(d, "nsym"); }
    for (int i : {-1, 2}) { d = dok, d.inverse = i; REFUSED(d, "inverse"); }
    for (int dt : {-1, 2, 7}) { d = dok, d.dtype = dt; REFUSED(d, "dtype"); }
    for (int T : {1, 2}) {
        d = dok, d.T = T, d.ldx = 3 * 192 - 1; REFUSED(d, "stride");
        d = dok, d.T = T, d.ldo = 3 * 192 - 1; REFUSED(d, "stride");
    }
    d = dok, d.out = nullptr; REFUSED(d, "null");
    d = dok, d.dtype = LDPC5G_F64, d.x = buf + 8; REFUSED(d, "aligned");
    d = dok, d.out = buf + 4; REFUSED(d, "aligned");
    d = dok, d.ldo = 3 * 192 + 1; REFUSED(d, "in place");

    Seq sok;
    sok.u = sok.v = (const int32_t*)buf, sok.out = buf;
    Seq s;
    for (int m : {6, 12, 18, 24, 0, -6, 35, 3306, INT32_MAX}) { s = sok, s.MZC = m; REFUSED(s, "MZC"); }
    for (int m = 30; m <= 3300; m += 6) { s = sok, s.MZC = m, s.out = nullptr; REFUSED(s, "null"); }
    for (int n : {0, -1, 65536}) { s = sok, s.n = n; REFUSED(s, "n="); }
    s = sok, s.alpha = NAN; REFUSED(s, "alpha");
    s = sok, s.alpha = INFINITY; REFUSED(s, "alpha");
    s = sok, s.u = nullptr; REFUSED(s, "null");
    s = sok, s.v = nullptr; REFUSED(s, "null");
    s = sok, s.out = buf + 8; REFUSED(s, "aligned");
    s = sok, s.v = (const int32_t*)(buf + 2); REFUSED(s, "aligned");

    Rx ok;
    ok.grid = buf, ok.h_ls = ok.y = buf, ok.slots = (const int32_t*)buf;
    Rx a;
    for (int Nr : {1, 2, 4})
        for (int port = 0; port < 4; ++port)
            for (int dt = 0; dt < 2; ++dt)
                for (int hop = 0; hop < 3; ++hop)
                    for (int half = 0; half < 3; ++half) {
                        a = ok, a.Nr = Nr, a.port = port, a.dtype = dt, a.hopping = hop, a.S = 4;
                        a.sym[0] = 2, a.sym[1] = 5, a.sym[2] = 8, a.sym[3] = 11;
                        if (half == 1) a.h_ls = nullptr;
                        if (half == 2) a.y = nullptr;
                        a.slots = nullptr;
                        REFUSED(a, "null");
                    }
    shared_checks(ok, buf);
    for (int Nr : {0, 3, 8, -1, INT32_MAX}) { a = ok, a.Nr = Nr; REFUSED(a, "Nr"); }
    for (int dt : {-1, 2, 7}) { a = ok, a.dtype = dt; REFUSED(a, "dtype"); }
    for (int T : {1, 2}) {
        a = ok, a.T = T, a.ldh = 2 * 48 * 2 - 1; REFUSED(a, "stride");
        a = ok, a.T = T, a.ldy = 14 * 192 * 2 - 1; REFUSED(a, "stride");
    }
    a = ok, a.h_ls = a.y = nullptr; REFUSED(a, "null");
    a = ok, a.dtype = LDPC5G_F64, a.grid = buf + 8; REFUSED(a, "aligned");
    a = ok, a.y = buf + 4; REFUSED(a, "aligned");

    Map mok;
    mok.sym_buf = buf, mok.re_idx = (const int32_t*)buf, mok.grid = buf, mok.slots = (const int32_t*)buf;
    Map m;
    mok.nre = 12;   // fits every allocation of shared_checks
    shared_checks(mok, buf);
    mok.nre = 1920;
    for (int na : {0, 3, 8, -1}) { m = mok, m.num_ant = na; REFUSED(m, "num_ant"); }
    float w[8] = {};
    for (int na : {1, 2, 4}) { m = mok, m.num_ant = na, m.precoding = w, m.grid = nullptr; REFUSED(m, "null"); }
    for (int64_t nre : {(int64_t)-1, (int64_t)14 * 192 + 1, INT64_MAX}) { m = mok, m.nre = nre, m.ldsym = INT64_MAX; REFUSED(m, "nre"); }
    for (int T : {1, 2}) { m = mok, m.T = T, m.ldsym = 1919; REFUSED(m, "stride"); }
    m = mok, m.sym_buf = nullptr; REFUSED(m, "null");
    m = mok, m.re_idx = nullptr; REFUSED(m, "null");
    m = mok, m.nre = 0, m.sym_buf = nullptr, m.re_idx = nullptr, m.grid = nullptr; REFUSED(m, "null");
    m = mok, m.grid = buf + 4; REFUSED(m, "aligned");
    EXPECT(strlen(ldpc5g_last_error()) > 0);
    if (fails) return 1;
    printf("tp_asan_main: ok\n");
    return 0;
}
