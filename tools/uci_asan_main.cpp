// Stand-alone host-sanitizer check of the UCI-on-PUSCH host code (ldpc5g_uci_rm_info, ldpc5g_uci_map_plan)
// and of the argument validation of ldpc5g_uci_mux / _demux / _scramble_modulate and
// ldpc5g_smallblock_encode / _decode: every call below returns before any kernel launch, so it needs no
// GPU.  Build it against the host-sanitized library (python -m python_5gtoolbox_amd.build --asan ->
// build/asan/libldpc5g.so):
//
//   CXX=/opt/rocm/lib/llvm/bin/clang++
//   RT=$(dirname $($CXX --print-file-name=libclang_rt.asan-x86_64.so))
//   $CXX -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -shared-libasan \
//       -Iinclude tools/uci_asan_main.cpp -Lbuild/asan -lldpc5g -Wl,-rpath,$PWD/build/asan \
//       -Wl,-rpath,$RT -o build/asan/uci_asan_main && build/asan/uci_asan_main
//
// Exit status 0 and "uci_asan_main: ok" mean every check held and no sanitizer report.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <initializer_list>
#include <vector>

#include "ldpc5g.h"

static int fails = 0;
#define EXPECT(cond)                                                              \
    do {                                                                          \
        if (!(cond)) {                                                            \
            printf("FAILED %s:%d: %s  [%s]\n", __FILE__, __LINE__, #cond, ldpc5g_last_error()); \
            ++fails;                                                              \
        }                                                                         \
    } while (0)
#define REFUSED(expr, word)                                          \
    do {                                                             \
        EXPECT((expr) == LDPC5G_ESIZE);                              \
        EXPECT(strstr(ldpc5g_last_error(), word) != nullptr);        \
    } while (0)

static const int kDmrsLists[4][4] = {{2, -1, -1, -1}, {2, 11, -1, -1}, {2, 7, 11, -1}, {2, 5, 8, 11}};

int main() {
    alignas(16) char buf[64];   // stands for every device buffer: never dereferenced by the validation
    // ---- rm_info and the plan builder over a grid of configurations: exact-size buffers, so an overrun is a report
    int built = 0, refused = 0, rm_refused = 0;
    for (int RB : {1, 2, 3, 24, 273})
        for (int nd = 1; nd <= 4; ++nd)
            for (int start : {0, 2})
                for (int NL : {1, 4})
                    for (int Qm : {1, 2, 4, 6, 8})
                        for (int cdm : {1, 2})
                            for (int oack : {0, 1, 2, 3, 11, 20})
                                for (int ocsi1 : {0, 7, 40})
                                    for (int ocsi2 : {0, 15, 400}) {
                                        if (RB == 273 && (oack % 3 || ocsi1 == 7)) continue;   // keep the run short
                                        const int nsym = 14 - start;
                                        const int* dm = kDmrsLists[nd - 1];
                                        int64_t nre = 0;
                                        for (int s = start; s < 14; ++s) {
                                            bool d = false;
                                            for (int i = 0; i < nd; ++i) d = d || dm[i] == s;
                                            nre += d ? (cdm == 1 ? RB * 6 : 0) : RB * 12;
                                        }
                                        const int64_t G = nre * NL * Qm;
                                        for (int en : {1, 0}) {
                                            int64_t rm[9];
                                            const int rc = ldpc5g_uci_rm_info(RB, start, nsym, dm, nd, NL, Qm, 517.0, G / 2 + 8, en, oack, ocsi1,
                                                                              ocsi1 ? ocsi2 : 0, 9, 6, 6, en ? 1.0 : 0.65, G, rm);
                                            if (rc != 0) {
                                                EXPECT(rc == LDPC5G_ESIZE && strlen(ldpc5g_last_error()) > 0);
                                                ++rm_refused;
                                                continue;
                                            }
                                            const int o2 = ocsi1 ? ocsi2 : 0;
                                            const int64_t n = ldpc5g_uci_map_plan(RB, start, nsym, dm, nd, cdm, NL, Qm, oack, ocsi1, o2, en, 0, rm[0],
                                                                                  rm[2], rm[4], rm[6], rm[8], G, nullptr, 0);
                                            if (n < 0) {
                                                EXPECT(n == LDPC5G_ESIZE && strlen(ldpc5g_last_error()) > 0);
                                                ++refused;
                                                continue;
                                            }
                                            std::vector<char> plan((size_t)n);
                                            // the size is known before the map is built: a configuration whose UCI does not fit its
                                            // symbols (the reference indexes past a list there) is refused only now
                                            const int64_t n2 = ldpc5g_uci_map_plan(RB, start, nsym, dm, nd, cdm, NL, Qm, oack, ocsi1, o2, en, 0, rm[0],
                                                                                   rm[2], rm[4], rm[6], rm[8], G, plan.data(), n);
                                            if (n2 < 0) {
                                                EXPECT(n2 == LDPC5G_ESIZE && strstr(ldpc5g_last_error(), "fit") != nullptr);
                                                ++refused;
                                                continue;
                                            }
                                            EXPECT(n2 == n);
                                            REFUSED(ldpc5g_uci_map_plan(RB, start, nsym, dm, nd, cdm, NL, Qm, oack, ocsi1, o2, en, 0, rm[0], rm[2], rm[4],
                                                                        rm[6], rm[8], G, plan.data(), n - 1), "plan_bytes");
                                            int32_t h[20];
                                            memcpy(h, plan.data(), sizeof h);
                                            EXPECT(h[2] == n && h[3] == G && h[4] == Qm && h[10] == (en ? rm[8] : 0) && h[11] == (oack ? rm[0] : 0));
                                            EXPECT(h[17] == h[10] + h[11] + h[12] + h[13] && h[15] == 128 + 4 * G);
                                            // every position has one owner or none; every stream element has a position below Gtotal
                                            const uint32_t* inv = (const uint32_t*)(plan.data() + h[15]);
                                            for (int j = 0; j < h[17]; ++j) EXPECT((int64_t)(inv[j] & 0xFFFFFF) < G);
                                            ++built;
                                        }
                                    }
    EXPECT(built > 1000 && rm_refused > 100);
    // ---- refusals of rm_info's own arguments
    const int dm[2] = {2, 11};
    int64_t rm[9];
    REFUSED(ldpc5g_uci_rm_info(4, 0, 14, nullptr, 2, 1, 6, 517.0, 1760, 1, 4, 11, 15, 9, 6, 6, 1.0, 3168, rm), "null");
    REFUSED(ldpc5g_uci_rm_info(4, 0, 14, dm, 2, 1, 6, 517.0, 1760, 1, 4, 11, 15, 9, 6, 6, 1.0, 3168, nullptr), "null");
    for (int v : {-1, 14, INT32_MAX, INT32_MIN}) {   // a DMRS symbol outside the slot: refused by both, the same way
        const int bad[2] = {2, v}, bad0[2] = {v, 11};
        REFUSED(ldpc5g_uci_rm_info(4, 0, 14, bad, 2, 1, 6, 517.0, 1760, 1, 4, 11, 15, 9, 6, 6, 1.0, 3168, rm), "dmrs_symlist");
        REFUSED(ldpc5g_uci_rm_info(4, 0, 14, bad0, 2, 1, 6, 517.0, 1760, 1, 4, 11, 15, 9, 6, 6, 1.0, 3168, rm), "dmrs_symlist");
        REFUSED(ldpc5g_uci_map_plan(4, 0, 14, bad, 2, 2, 1, 6, 4, 11, 15, 1, 0, 96, 48, 90, 0, 2934, 3168, nullptr, 0), "dmrs_symlist");
    }
    for (int nd : {0, 15, -1, INT32_MAX}) {
        REFUSED(ldpc5g_uci_rm_info(4, 0, 14, dm, nd, 1, 6, 517.0, 1760, 1, 4, 11, 15, 9, 6, 6, 1.0, 3168, rm), "allocation");
        REFUSED(ldpc5g_uci_map_plan(4, 0, 14, dm, nd, 2, 1, 6, 4, 11, 15, 1, 0, 96, 48, 90, 0, 2934, 3168, nullptr, 0), "allocation");
    }
    for (int RB : {0, -1, 276, INT32_MAX, INT32_MIN}) REFUSED(ldpc5g_uci_rm_info(RB, 0, 14, dm, 2, 1, 6, 517.0, 1760, 1, 4, 11, 15, 9, 6, 6, 1.0, 3168, rm), "allocation");
    for (int n : {0, 15, -3, INT32_MAX}) REFUSED(ldpc5g_uci_rm_info(4, 0, n, dm, 2, 1, 6, 517.0, 1760, 1, 4, 11, 15, 9, 6, 6, 1.0, 3168, rm), "allocation");
    for (int i : {-1, 16, INT32_MAX, INT32_MIN}) REFUSED(ldpc5g_uci_rm_info(4, 0, 14, dm, 2, 1, 6, 517.0, 1760, 1, 4, 11, 15, i, 6, 6, 1.0, 3168, rm), "I_HARQ_ACK_offset");
    for (int i : {-1, 19, INT32_MAX, INT32_MIN}) {
        REFUSED(ldpc5g_uci_rm_info(4, 0, 14, dm, 2, 1, 6, 517.0, 1760, 1, 4, 11, 15, 9, i, 6, 1.0, 3168, rm), "I_CSI1offset");
        REFUSED(ldpc5g_uci_rm_info(4, 0, 14, dm, 2, 1, 6, 517.0, 1760, 1, 4, 11, 15, 9, 6, i, 1.0, 3168, rm), "I_CSI2offset");
    }
    for (int o : {-1, 1707, INT32_MAX, INT32_MIN}) REFUSED(ldpc5g_uci_rm_info(4, 0, 14, dm, 2, 1, 6, 517.0, 1760, 1, o, 11, 15, 9, 6, 6, 1.0, 3168, rm), "payload");
    REFUSED(ldpc5g_uci_rm_info(4, 0, 14, dm, 2, 1, 5, 517.0, 1760, 1, 4, 11, 15, 9, 6, 6, 1.0, 3168, rm), "Qm");
    REFUSED(ldpc5g_uci_rm_info(4, 0, 14, dm, 2, 1, 6, 517.0, 0, 1, 4, 11, 15, 9, 6, 6, 1.0, 3168, rm), "ULSCH_size");
    REFUSED(ldpc5g_uci_rm_info(4, 0, 14, dm, 2, 1, 6, 517.0, 1760, 1, 4, 11, 15, 9, 6, 6, 0.0, 3168, rm), "UCIScaling");
    REFUSED(ldpc5g_uci_rm_info(4, 0, 14, dm, 2, 1, 6, 517.0, 1760, 1, 4, 11, 15, 9, 6, 6, 1.0, 100, rm), "Gtotal");
    // ---- refusals of the plan's own arguments, on the ALL case (3168 bits: 4 PRB, 64QAM, DMRS 2 / 7 / 11)
    const int d3[3] = {2, 7, 11};
    EXPECT(ldpc5g_uci_rm_info(4, 0, 14, d3, 3, 1, 6, 517.0, 1760, 1, 4, 11, 15, 9, 6, 6, 1.0, 3168, rm) == 0);
    EXPECT(rm[0] == 96 && rm[2] == 48 && rm[4] == 90 && rm[8] == 2934);
#define PLAN(RB, HOP, CDM, EA, GU, G, P, PB) \
    ldpc5g_uci_map_plan(RB, 0, 14, d3, 3, CDM, 1, 6, 4, 11, 15, 1, HOP, EA, rm[2], rm[4], rm[6], GU, G, P, PB)
    const int64_t n = PLAN(4, 0, 2, rm[0], rm[8], 3168, nullptr, 0);
    EXPECT(n == 128 + 4 * 3168 + 4 * (2934 + 96 + 48 + 90));
    std::vector<char> plan((size_t)n);
    EXPECT(PLAN(4, 0, 2, rm[0], rm[8], 3168, plan.data(), n) == n);
    REFUSED(PLAN(4, 1, 2, rm[0], rm[8], 3168, nullptr, 0), "hopping");
    REFUSED(PLAN(4, 0, 3, rm[0], rm[8], 3168, nullptr, 0), "NumCDMGroups");
    REFUSED(PLAN(4, 0, 2, rm[0] + 1, rm[8], 3168, nullptr, 0), "multiple");
    std::vector<char> big((size_t)n + 8192);   // the checks below need the map itself, not only its size
    REFUSED(PLAN(4, 0, 2, rm[0], rm[8] - 6, 3168, big.data(), (int64_t)big.size()), "G_ULSCH");
    REFUSED(PLAN(4, 0, 2, rm[0], rm[8], 3162, nullptr, 0), "Gtotal");
    REFUSED(PLAN(0, 0, 2, rm[0], rm[8], 3168, nullptr, 0), "allocation");
    REFUSED(PLAN(4, 0, 2, (int64_t)1200, rm[8], 3168, big.data(), (int64_t)big.size()), "G_ULSCH");   // more ACK than the UL-SCH was sized for
    REFUSED(ldpc5g_uci_map_plan(4, 0, 14, nullptr, 3, 2, 1, 6, 4, 11, 15, 1, 0, rm[0], rm[2], rm[4], rm[6], rm[8], 3168, nullptr, 0), "null");
    // ---- refusals of the entry points
    const void* ph = plan.data();
    int8_t* b8 = (int8_t*)buf;
    const uint32_t* w32 = (const uint32_t*)buf;
    REFUSED(ldpc5g_uci_mux(nullptr, ph, b8, 2934, b8, 96, b8, 48, b8, 90, b8, 3168, 1, nullptr), "plan_dev");
    REFUSED(ldpc5g_uci_mux(buf, nullptr, b8, 2934, b8, 96, b8, 48, b8, 90, b8, 3168, 1, nullptr), "plan_host");
    REFUSED(ldpc5g_uci_mux(buf, ph, nullptr, 2934, b8, 96, b8, 48, b8, 90, b8, 3168, 1, nullptr), "g_ulsch");
    REFUSED(ldpc5g_uci_mux(buf, ph, b8, 2934, b8, 95, b8, 48, b8, 90, b8, 3168, 1, nullptr), "g_ack");
    REFUSED(ldpc5g_uci_mux(buf, ph, b8, 2934, b8, 96, b8, 48, b8, 90, nullptr, 3168, 1, nullptr), "g_seq");
    REFUSED(ldpc5g_uci_mux(buf, ph, b8, 2934, b8, 96, b8, 48, b8, 90, b8, 3167, 1, nullptr), "ldg");
    for (int T : {0, -1, 65536, INT32_MAX, INT32_MIN}) {
        REFUSED(ldpc5g_uci_mux(buf, ph, b8, 2934, b8, 96, b8, 48, b8, 90, b8, 3168, T, nullptr), "T=");
        REFUSED(ldpc5g_uci_demux(buf, ph, buf, LDPC5G_F32, 3168, w32, 99, 1, buf, 2934, buf, 96, buf, 48, buf, 90, T, nullptr), "T=");
        REFUSED(ldpc5g_uci_scramble_modulate(b8, 3168, w32, 99, T, 3168, 6, buf, 528, nullptr), "T=");
        REFUSED(ldpc5g_smallblock_encode(b8, 11, 11, 2, b8, 32, 32, T, nullptr), "T=");
    }
    for (int T : {0, -1, (1 << 22) + 1, INT32_MIN}) REFUSED(ldpc5g_smallblock_decode(buf, LDPC5G_F64, 32, 32, 11, 2, b8, 11, T, nullptr), "T=");
    REFUSED(ldpc5g_uci_demux(buf, ph, nullptr, LDPC5G_F32, 3168, w32, 99, 1, buf, 2934, buf, 96, buf, 48, buf, 90, 1, nullptr), "llr");
    REFUSED(ldpc5g_uci_demux(buf, ph, buf, 7, 3168, w32, 99, 1, buf, 2934, buf, 96, buf, 48, buf, 90, 1, nullptr), "dtype");
    REFUSED(ldpc5g_uci_demux(buf, ph, buf, LDPC5G_F32, 3167, w32, 99, 1, buf, 2934, buf, 96, buf, 48, buf, 90, 1, nullptr), "ldl");
    REFUSED(ldpc5g_uci_demux(buf, ph, buf, LDPC5G_F32, 3168, w32, 98, 1, buf, 2934, buf, 96, buf, 48, buf, 90, 1, nullptr), "ldw");
    REFUSED(ldpc5g_uci_demux(buf, ph, buf, LDPC5G_F32, 3168, w32, 99, 2, buf, 2934, buf, 96, buf, 48, buf, 90, 1, nullptr), "erase_punctured");
    REFUSED(ldpc5g_uci_demux(buf, ph, buf, LDPC5G_F64, 3168, nullptr, 0, 0, buf, 2934, buf, 96, nullptr, 48, buf, 90, 1, nullptr), "g_csi1");
    REFUSED(ldpc5g_uci_demux(buf, ph, buf, LDPC5G_F64, 3168, nullptr, 0, 0, buf, 2934, buf, 96, buf, 48, buf, 89, 1, nullptr), "g_csi2");
    for (int64_t ld : {(int64_t)0, (int64_t)-3168, INT64_MIN}) {
        REFUSED(ldpc5g_uci_demux(buf, ph, buf, LDPC5G_F32, ld, w32, 99, 1, buf, 2934, buf, 96, buf, 48, buf, 90, 1, nullptr), "ldl");
        REFUSED(ldpc5g_uci_mux(buf, ph, b8, ld, b8, 96, b8, 48, b8, 90, b8, 3168, 1, nullptr), "g_ulsch");
        REFUSED(ldpc5g_uci_scramble_modulate(b8, ld, w32, 99, 1, 3168, 6, buf, 528, nullptr), "ldb");
        REFUSED(ldpc5g_smallblock_encode(b8, ld, 11, 2, b8, 32, 32, 1, nullptr), "ldb");
        REFUSED(ldpc5g_smallblock_decode(buf, LDPC5G_F64, ld, 32, 11, 2, b8, 11, 1, nullptr), "ldl");
    }
    // a damaged plan: magic, version, sizes the kernels would index by
    for (int word : {0, 1, 2, 3, 10, 15, 17}) {
        std::vector<char> bad(plan);
        int32_t v;
        memcpy(&v, bad.data() + 4 * word, 4);
        v = word == 3 ? 1 << 25 : v + 4;
        memcpy(bad.data() + 4 * word, &v, 4);
        const char* what = word == 0 ? "magic" : word == 1 ? "version" : "range";
        REFUSED(ldpc5g_uci_mux(buf, bad.data(), b8, 4000, b8, 96, b8, 48, b8, 90, b8, 3168, 1, nullptr), what);
        REFUSED(ldpc5g_uci_demux(buf, bad.data(), buf, LDPC5G_F32, 3168, w32, 99, 1, buf, 4000, buf, 96, buf, 48, buf, 90, 1, nullptr), what);
    }
    for (int mod : {0, 3, 10, -2, INT32_MAX}) REFUSED(ldpc5g_uci_scramble_modulate(b8, 3168, w32, 99, 1, 3168, mod, buf, 528, nullptr), "modulation");
    REFUSED(ldpc5g_uci_scramble_modulate(b8, 3168, w32, 99, 1, 3167, 6, buf, 528, nullptr), "sizes");
    REFUSED(ldpc5g_uci_scramble_modulate(b8, 3168, nullptr, 99, 1, 3168, 6, buf, 528, nullptr), "null");
    REFUSED(ldpc5g_uci_scramble_modulate(b8, 3168, w32, 98, 1, 3168, 6, buf, 528, nullptr), "ldw");
    REFUSED(ldpc5g_uci_scramble_modulate(b8, 3168, w32, 99, 1, 3168, 6, buf, 527, nullptr), "ldsym");
    for (int K : {0, 12, -1, INT32_MAX, INT32_MIN}) {
        REFUSED(ldpc5g_smallblock_encode(b8, 11, K, 2, b8, 32, 32, 1, nullptr), "K=");
        REFUSED(ldpc5g_smallblock_decode(buf, LDPC5G_F32, 32, 32, K, 2, b8, 11, 1, nullptr), "K=");
    }
    for (int Qm : {0, 3, 10, -2, INT32_MAX}) {
        REFUSED(ldpc5g_smallblock_encode(b8, 11, 1, Qm, b8, 32, 32, 1, nullptr), "Qm=");
        REFUSED(ldpc5g_smallblock_decode(buf, LDPC5G_F32, 32, 32, 2, Qm, b8, 11, 1, nullptr), "Qm=");
    }
    for (int E : {0, -1, 8193, INT32_MAX, INT32_MIN}) {
        REFUSED(ldpc5g_smallblock_encode(b8, 11, 11, 2, b8, 8192, E, 1, nullptr), "E=");
        REFUSED(ldpc5g_smallblock_decode(buf, LDPC5G_F32, 8192, E, 11, 2, b8, 11, 1, nullptr), "E=");
    }
    REFUSED(ldpc5g_smallblock_encode(b8, 11, 11, 2, b8, 31, 32, 1, nullptr), "ldo");
    REFUSED(ldpc5g_smallblock_decode(buf, LDPC5G_F32, 32, 32, 11, 2, b8, 10, 1, nullptr), "ldo");
    REFUSED(ldpc5g_smallblock_decode(buf, 5, 32, 32, 11, 2, b8, 11, 1, nullptr), "dtype");
    REFUSED(ldpc5g_smallblock_decode(nullptr, LDPC5G_F32, 32, 32, 11, 2, b8, 11, 1, nullptr), "null");
    if (fails) return 1;
    printf("uci_asan_main: ok (%d plans built, %d refused; rm_info refused %d)\n", built, refused, rm_refused);
    return 0;
}
