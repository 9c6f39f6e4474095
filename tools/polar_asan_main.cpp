// Stand-alone host-sanitizer check of the polar plan builder (ldpc5g_polar_plan) and of the argument
// validation of ldpc5g_polar_encode / _rate_match / _rate_recover / _decode: every call below returns
// before any kernel launch, so it needs no GPU.  Build it against the host-sanitized library (python -m
// python_5gtoolbox_amd.build --asan -> build/asan/libldpc5g.so):
//
//   CXX=/opt/rocm/lib/llvm/bin/clang++
//   RT=$(dirname $($CXX --print-file-name=libclang_rt.asan-x86_64.so))
//   $CXX -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -shared-libasan \
//       -Iinclude tools/polar_asan_main.cpp -Lbuild/asan -lldpc5g -Wl,-rpath,$PWD/build/asan \
//       -Wl,-rpath,$RT -o build/asan/polar_asan_main && build/asan/polar_asan_main
//
// Exit status 0 and "polar_asan_main: ok" mean every check held and no sanitizer report.
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

int main() {
    alignas(16) char buf[64];   // stands for every device buffer: never dereferenced by the validation
    // ---- the plan builder over every (K, E) class: exact-size buffers, so an overrun is a report
    int built = 0, refused = 0;
    for (int cfg = 0; cfg < 3; ++cfg) {
        const int nMax = cfg == 0 ? 9 : 10, iIL = cfg == 0 ? 1 : 0, crclen = cfg == 0 ? 24 : (cfg == 1 ? 6 : 11);
        for (int K = 1; K <= 1100; K += (K < 200 ? 1 : 37))
            for (int E : {K, K + 1, K + 3, K + 9, 2 * K, 3 * K + 1, 5 * K, 8 * K, 31, 32, 33, 64, 127, 216, 512, 1000, 1024, 2100,
                          8191, 8192, 8193}) {
                const int64_t n = ldpc5g_polar_plan(K, E, nMax, iIL, crclen, cfg == 0, 0xabcdef, nullptr, 0);
                if (n < 0) {
                    EXPECT(n == LDPC5G_ESIZE && strlen(ldpc5g_last_error()) > 0);
                    ++refused;
                    continue;
                }
                std::vector<char> plan((size_t)n);
                EXPECT(ldpc5g_polar_plan(K, E, nMax, iIL, crclen, cfg == 0, 0xabcdef, plan.data(), n) == n);
                REFUSED(ldpc5g_polar_plan(K, E, nMax, iIL, crclen, cfg == 0, 0xabcdef, plan.data(), n - 1), "plan_bytes");
                int32_t h[20];
                memcpy(h, plan.data(), sizeof h);
                EXPECT(h[2] == n && h[3] == K && h[4] == E && h[10] == (1 << h[11]) && h[10] >= 32 && h[10] <= (1 << nMax));
                // the argument checks with this plan
                const void* pd = buf;
                const void* ph = plan.data();
                const int N = h[10];
                REFUSED(ldpc5g_polar_encode(pd, ph, nullptr, K, (int8_t*)buf, N, 4, nullptr), "null");
                REFUSED(ldpc5g_polar_encode(pd, ph, (const int8_t*)buf, K - 1, (int8_t*)buf, N, 4, nullptr), "ldb");
                REFUSED(ldpc5g_polar_rate_match(pd, ph, (const int8_t*)buf, N, (int8_t*)buf, E - 1, 4, 1, nullptr), "ldo");
                REFUSED(ldpc5g_polar_rate_recover(pd, ph, (const double*)buf, E, (double*)buf, N - 1, 4, 1, 20.0, 0, nullptr), "ldo");
                REFUSED(ldpc5g_polar_decode(pd, ph, (const double*)buf, N, (int8_t*)buf, K, nullptr, (double*)buf, 4,
                                            LDPC5G_POLAR_SCL, 32, nullptr), "status");
                ++built;
            }
    }
    EXPECT(built > 1000 && refused > 1000);
    // ---- refusals of the plan's own arguments
    REFUSED(ldpc5g_polar_plan(64, 216, 8, 1, 24, 0, 0, nullptr, 0), "nMax");
    REFUSED(ldpc5g_polar_plan(64, 216, 9, 0, 24, 0, 0, nullptr, 0), "nMax");
    REFUSED(ldpc5g_polar_plan(64, 216, 10, 0, 24, 0, 0, nullptr, 0), "nMax");
    for (int E : {0, -1, 8193, INT32_MAX, INT32_MIN}) REFUSED(ldpc5g_polar_plan(64, E, 9, 1, 24, 0, 0, nullptr, 0), "E=");
    for (int K : {0, -1, 24, INT32_MIN}) REFUSED(ldpc5g_polar_plan(K, 216, 9, 1, 24, 0, 0, nullptr, 0), "CRC");
    for (int K : {165, 1000, INT32_MAX}) REFUSED(ldpc5g_polar_plan(K, 8192, 9, 1, 24, 0, 0, nullptr, 0), "interleaver");
    for (int K : {12, 17, 26, 30}) REFUSED(ldpc5g_polar_plan(K, 100, 10, 0, 11, 0, 0, nullptr, 0), "UL ranges");
    for (int K : {1024, 5000, INT32_MAX}) REFUSED(ldpc5g_polar_plan(K, 8192, 10, 0, 11, 0, 0, nullptr, 0), "N=1024");
    REFUSED(ldpc5g_polar_plan(64, 216, 9, 1, 24, 2, 0, nullptr, 0), "padCRC");
    REFUSED(ldpc5g_polar_plan(64, 216, 9, 1, 24, 0, -1, nullptr, 0), "rnti");
    REFUSED(ldpc5g_polar_plan(64, 216, 9, 1, 24, 0, 1 << 24, nullptr, 0), "rnti");
    // ---- refusals of the entry points
    const int64_t n = ldpc5g_polar_plan(64, 216, 9, 1, 24, 1, 0x1234, nullptr, 0);
    std::vector<char> plan((size_t)n);
    EXPECT(ldpc5g_polar_plan(64, 216, 9, 1, 24, 1, 0x1234, plan.data(), n) == n);
    const void* ph = plan.data();
    int8_t* b8 = (int8_t*)buf;
    double* f8 = (double*)buf;
    uint8_t* u8 = (uint8_t*)buf;
    REFUSED(ldpc5g_polar_decode(nullptr, ph, f8, 256, b8, 64, u8, f8, 1, LDPC5G_POLAR_SCL, 8, nullptr), "plan_dev");
    REFUSED(ldpc5g_polar_decode(buf, nullptr, f8, 256, b8, 64, u8, f8, 1, LDPC5G_POLAR_SCL, 8, nullptr), "plan_host");
    for (int L : {0, -1, 33, INT32_MAX, INT32_MIN})
        REFUSED(ldpc5g_polar_decode(buf, ph, f8, 256, b8, 64, u8, f8, 1, LDPC5G_POLAR_SCL, L, nullptr), "L=");
    for (int algo : {-1, 2, INT32_MAX}) REFUSED(ldpc5g_polar_decode(buf, ph, f8, 256, b8, 64, u8, f8, 1, algo, 8, nullptr), "algo");
    for (int B : {0, -1, (1 << 22) + 1, INT32_MIN}) {
        REFUSED(ldpc5g_polar_decode(buf, ph, f8, 256, b8, 64, u8, f8, B, LDPC5G_POLAR_SCL, 8, nullptr), "B=");
        REFUSED(ldpc5g_polar_encode(buf, ph, b8, 64, b8, 256, B, nullptr), "B=");
        REFUSED(ldpc5g_polar_rate_match(buf, ph, b8, 256, b8, 216, B, 0, nullptr), "B=");
        REFUSED(ldpc5g_polar_rate_recover(buf, ph, f8, 216, f8, 256, B, 0, 20.0, 0, nullptr), "B=");
    }
    for (int64_t ld : {(int64_t)0, (int64_t)255, (int64_t)-256, INT64_MIN}) {
        REFUSED(ldpc5g_polar_decode(buf, ph, f8, ld, b8, 64, u8, f8, 1, LDPC5G_POLAR_SCL, 8, nullptr), "ldl");
        REFUSED(ldpc5g_polar_encode(buf, ph, b8, 64, b8, ld, 1, nullptr), "ldo");
        REFUSED(ldpc5g_polar_rate_match(buf, ph, b8, ld, b8, 216, 1, 0, nullptr), "ldi");
    }
    REFUSED(ldpc5g_polar_decode(buf, ph, f8, 256, b8, 63, u8, f8, 1, LDPC5G_POLAR_SCL, 8, nullptr), "ldc");
    REFUSED(ldpc5g_polar_decode(buf, ph, (const double*)(buf + 4), 256, b8, 64, u8, f8, 1, LDPC5G_POLAR_SCL, 8, nullptr), "aligned");
    REFUSED(ldpc5g_polar_rate_match(buf, ph, b8, 256, b8, 216, 1, 2, nullptr), "iBIL");
    REFUSED(ldpc5g_polar_rate_recover(buf, ph, f8, 216, f8, 256, 1, 0, 20.0, 3, nullptr), "reference_repetition");
    // a damaged plan: magic, version, sizes the kernels would index by
    for (int word : {0, 1, 10, 11, 3}) {
        std::vector<char> bad(plan);
        int32_t v;
        memcpy(&v, bad.data() + 4 * word, 4);
        v = word == 3 ? 100000 : v + 1;
        memcpy(bad.data() + 4 * word, &v, 4);
        REFUSED(ldpc5g_polar_encode(buf, bad.data(), b8, 64, b8, 256, 1, nullptr), word == 0 ? "magic" : word == 1 ? "version" : "range");
        REFUSED(ldpc5g_polar_decode(buf, bad.data(), f8, 256, b8, 64, u8, f8, 1, LDPC5G_POLAR_SC, 1, nullptr),
                word == 0 ? "magic" : word == 1 ? "version" : "range");
    }
    if (fails) return 1;
    printf("polar_asan_main: ok (%d plans built, %d refused)\n", built, refused);
    return 0;
}
