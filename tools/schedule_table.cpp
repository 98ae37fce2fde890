// tools/schedule_table.cpp -- print every host-side scheduling decision of the library (fft_wgpu_amd/csrc/schedule.h) as text.
//
//     g++ -std=c++17 -I fft_wgpu_amd/csrc tools/schedule_table.cpp -o schedule_table
//     ./schedule_table             the decision table; tests/test_schedule.py compares it with tests/golden/tiled_schedule.txt
//     ./schedule_table families    per valid factor triple: families(lg, lf), then the families of the 16 flag settings
//
// Plain C++17, no device: the header is pure integer logic.
#include <cstdio>
#include <cstring>

#include "schedule.h"

using namespace fwa_int;

static const char *name(TiledKernel k)
{
    static const char *const n[] = {"-", "colsw", "cols32", "p1gen", "tilec", "rows32", "tiler"};
    return n[(int)k];
}

template <class F>
static void for_each_triple(F f)
{
    for (uint32_t lg = 12; lg <= 30; ++lg)
        for (uint32_t a = 0; a <= 13; ++a)
            for (uint32_t b = 0; b <= 13; ++b) {
                const uint32_t lf[3] = {a, b, lg - a - b};
                if (a + b <= lg && lf[2] <= 13) f(lg, lf);
            }
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "families")) {
        for_each_triple([](uint32_t lg, const uint32_t lf[3]) {
            if (!factors_valid(lg, lf)) return;
            printf("F %u %u,%u,%u %x :", lg, lf[0], lf[1], lf[2], families(lg, lf));
            for (uint32_t i = 0; i < 16; ++i) printf(" %x", resolve_tiled(lg, lf, flag_setting(i)).families);
            printf("\n");
        });
        return 0;
    }
    printf("# D <lg n> <batch> <path> <factors> <colsw>: choose_path\n");
    for (uint32_t lg = 0; lg <= 30; ++lg) {
        const uint64_t edge = (1ull << 20) >> lg;
        const uint64_t batches[] = {1, 2, 3, 4, 5, edge - 1, edge, edge + 1, 1ull << 40};
        for (uint64_t batch : batches) {
            uint32_t lf[3];
            bool colsw = false;
            const int64_t path = choose_path(1u << lg, batch, lf, &colsw);
            printf("D %u %llu %lld %u,%u,%u %d\n", lg, (unsigned long long)batch, (long long)path, lf[0], lf[1], lf[2], (int)colsw);
        }
    }
    printf("# T <lg n> <factors> invalid | { <pass A>/<B>/<C> <ring_cw> <passes> <default xcd_swizzle> <flag settings> }...\n"
           "# flag settings: hex mask, bit i = the setting colsw = i & 1, rows32 = i >> 1 & 1, p1_gen = i >> 2 & 1, tile_ring = i >> 3\n");
    for_each_triple([](uint32_t lg, const uint32_t lf[3]) {
        printf("T %u %u,%u,%u", lg, lf[0], lf[1], lf[2]);
        if (!factors_valid(lg, lf)) { printf(" invalid\n"); return; }
        char text[16][64];
        uint32_t mask[16], n = 0;
        for (uint32_t i = 0; i < 16; ++i) {
            const TiledSchedule s = resolve_tiled(lg, lf, flag_setting(i));
            char t[64];
            snprintf(t, sizeof t, "%s/%s/%s %u %u %u", name(s.a), name(s.b), name(s.c), s.ring_cw, s.passes, s.xcd_swizzle);
            uint32_t j = 0;
            while (j < n && strcmp(text[j], t)) ++j;
            if (j == n) { strcpy(text[n], t); mask[n++] = 0; }
            mask[j] |= 1u << i;
        }
        for (uint32_t j = 0; j < n; ++j) printf(" | %s %x", text[j], mask[j]);
        printf("\n");
    });
    return 0;
}
