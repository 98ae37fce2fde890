// schedule.h -- which kernels a plan launches, as pure integer logic without HIP: the kernel limits that the launchers of
// kernels_*.hip enforce (through kernels.h), the default path and factors (choose_path) and the kernel of every pass of a tiled
// plan (resolve_tiled).  plan.cpp, tuning.cpp and tables.cpp ask here and restate none of it; tools/schedule_table.cpp prints
// the whole decision table on a CPU and tests/test_schedule.py pins it to tests/golden/tiled_schedule.txt.
#pragma once
#include <cstdint>

enum fwa_path : int64_t {
    PATH_SMALL = 0,       // n <= 32768: one launch (k_chunk / k_small32)
    PATH_TWOPASS_1M = 1,  // n = 2^20: k_p1_1m + k_p2_1m per group of transforms
    PATH_R2_GLOBAL = 2,   // the reference recurrence literally, one launch per stage (forced only)
    PATH_NORMALIZE = 3,
    PATH_IDENTITY = 4,    // n = 1
    PATH_RING_1M = 5,     // n = 2^20: the same two passes as ONE persistent launch with a small ring (k_ring_1m)
    // 8 was the L2-resident team path (k_team, rounds 2-5; removed in round 6: profiles/round6/lab_pruned_families.patch)
    PATH_TILED = 7,       // n = N1*N2[*N3], each 64..1024: 2-3 k_tile passes
};

namespace fwa {
// ---- kernel limits: the log2 FFT lengths each pass kernel exists for ----
constexpr bool rows32_supported(uint32_t lg_l) { return lg_l >= 9 && lg_l <= 12; }
// tile-contiguous ring input of width in_cw (written by k_colsw): rows of >= 32*in_cw points
constexpr bool rows32_ring_supported(uint32_t lg_l, uint32_t in_cw) { return (in_cw == 32 || in_cw == 64) && lg_l >= 10 && lg_l <= 12 && (1u << (lg_l - 5)) >= in_cw; }
constexpr bool colsw_supported(uint32_t lg_l) { return lg_l == 8 || lg_l == 9; }
constexpr uint32_t colsw_width(uint32_t lg_l) { return 1u << (14 - lg_l); }
constexpr bool cols32_supported(uint32_t lg_l) { return lg_l == 11; }
constexpr bool p1_gen_supported(uint32_t lg_l) { return lg_l == 10; }
constexpr bool tile_supported(uint32_t lg_l) { return lg_l >= 6 && lg_l <= 10; }
constexpr uint32_t LG_N_MAX_32 = 28;  // k_colsw, k_cols32 and k_rows32 address a transform with 32-bit byte offsets: n <= 2^28
}  // namespace fwa

namespace fwa_int {

inline uint32_t ilog2(uint32_t n) { uint32_t l = 0; while ((1u << l) < n) ++l; return l; }

// Path and per-pass FFT lengths (log2) for a transform length; shared by fwa_plan_create and fwa_describe_path.
// `batch` separates two regimes (profiles/round2/sweep_small_batch_latency.jsonl):
//  * throughput (n * batch > 2^20 samples): few passes of fat tiles -- a 1024-point first pass (k_p1_gen / the 2^20
//    pipeline, 64 KiB tiles of 512 threads) and 32-point-per-thread rows;
//  * latency (at most 2^20 samples in flight, or a single 2^21 / 2^22 transform, or fewer than FEW_1M transforms of
//    2^20): fat tiles leave most of the 256 CUs idle (one 2^16 transform = FOUR 1024 x 16 tiles), so the plan uses the
//    smallest tiles instead -- balanced two passes up to 2^17, balanced three passes of 64/128-point tiles above
//    (2^16 x 1: 11.9 us against 16.2; 2^18 x 1: 12.7 against 18.4; 2^20 x 1: 19 against 24).
constexpr uint64_t FEW_1M = 4;
inline int64_t choose_path(uint32_t n, uint64_t batch, uint32_t lf[3], bool *colsw = nullptr)
{
    lf[0] = lf[1] = lf[2] = 0;
    if (colsw) *colsw = false;
    const uint32_t lg = ilog2(n);
    if (n == 1) return PATH_IDENTITY;
    if (n <= 32768) { lf[0] = lg; return PATH_SMALL; }
    const bool few = (lg < 20 && batch <= ((1ull << 20) >> lg)) || (lg == 20 && batch < FEW_1M)
        || ((lg == 21 || lg == 22) && batch == 1);
    if (n == (1u << 20) && !few) { lf[0] = lf[1] = 10; return PATH_TWOPASS_1M; }
    if (n <= (1u << 30)) {
        // factors of 64..1024 each, 2048 for the rows of a two-pass plan (re-tunable: key "factors").  Throughput
        // regime: two passes up to 2^19 and at 2^21 .. 2^23 (2048 / 4096-point passes), three otherwise; a 1024-point
        // first pass (k_p1_gen) wherever the other factors stay >= 64, measured faster than a balanced split except
        // at 2^22 (level) (profiles/round2/p1gen_sweep.jsonl, factor_sweep.jsonl, sweep_rows32.jsonl). Round 3
        // (profiles/round3/sweep_colsw_32GiB.jsonl, sweep_factors_24_28_colsw.jsonl): short columns in wide tiles
        // (k_colsw: 256 x 64 / 512 x 32, 512- / 256-byte row segments) beat the 1024 x 16 tile of k_p1_gen as pass A
        // wherever the last pass keeps <= 1024-point rows: 2^16 .. 2^19 + 7-9 %, three-pass sizes 2^24 .. 2^28 + 2-16 %
        // 1024 x 4096: k_p1_gen + k_rows32 (8 rows of 4096 per workgroup)
        if (!few && lg == 22) { lf[0] = 10; lf[1] = 12; }
        else if (!few && lg == 23) { lf[0] = 11; lf[1] = 12; }  // 2048 x 4096: k_cols32 + k_rows32
        else if (few && lg <= 17) { lf[0] = lg / 2; lf[1] = lg - lf[0]; }
        else if (!few && lg <= 18) { lf[0] = 8; lf[1] = lg - 8; if (colsw) *colsw = true; }   // 256 x (256 .. 1024)
        else if (!few && lg == 19) { lf[0] = 9; lf[1] = 10; if (colsw) *colsw = true; }       // 512 x 1024
        else if (!few && lg == 21) { lf[0] = 10; lf[1] = lg - 10; }
        else if (!few && lg >= 24 && lg <= 28) {
            lf[0] = 9; lf[1] = (lg - 9) / 2; lf[2] = lg - 9 - lf[1];
            if (colsw) *colsw = true;
        }
        else if (!few && lg >= 29) { lf[0] = 10; lf[1] = (lg - 10) / 2; lf[2] = lg - 10 - lf[1]; }
        // 16.4 us against 18.2 for 64 x 128 x 128 (sweep_factor_permutations_batch1.jsonl)
        else if (few && lg == 20) { lf[0] = lf[1] = 6; lf[2] = 8; }
        else for (uint32_t i = 0; i < 3; ++i) lf[i] = lg / 3 + (i >= 3 - lg % 3 ? 1 : 0);
        return PATH_TILED;
    }
    return PATH_R2_GLOBAL;
}

// The paths that run groups of transforms through a scratch ring, over chains (keys "group", "streams", "xcd_swizzle").
constexpr bool is_pipelined(int64_t path) { return path == PATH_TWOPASS_1M || path == PATH_TILED; }

// Kernel families, one bit each, paired with their setup functions in kFamilySetups (plan.cpp): each raises the dynamic-LDS
// limits of its kernels (kernels.h), once per context, before the first plan that may launch one of them.
enum : uint32_t { FAM_SMALL32 = 1, FAM_1M = 2, FAM_ROWS32 = 4, FAM_COLSW = 8, FAM_COLS32 = 16, FAM_TILE = 32, FAM_P1_GEN = 64, FAM_LAB_RING = 128 };

// ---- the tiled path (PATH_TILED): n = N1*N2[*N3] = 2^lf[0] * 2^lf[1] [* 2^lf[2]], pass A over N1, [B over N2,] C over the last ----
// The keys of the same names (tuning.cpp); which of them takes effect is resolve_tiled's business alone.
struct TiledFlags {
    int64_t colsw = 0;      // first factor 256 / 512: 1 = k_colsw (64 / 32-column tiles) as pass A
    int64_t rows32 = 1;     // two passes with a 512..4096-point second factor: 1 = k_rows32 last
    int64_t p1_gen = 1;     // first factor 1024: 1 = k_p1_gen as pass A, 0 = k_tile
    int64_t tile_ring = 1;  // k_colsw + k_rows32: 1 = tile-contiguous ring slab, 0 = matrix layout
};

enum class TiledKernel : uint8_t { NONE, COLSW, COLS32, P1_GEN, TILE_COLS, ROWS32, TILE_ROWS };
constexpr uint32_t kFamilyOf[] = {0u, FAM_COLSW, FAM_COLS32, FAM_P1_GEN, FAM_TILE, FAM_ROWS32, FAM_TILE};  // by TiledKernel

struct TiledSchedule {
    TiledKernel a = TiledKernel::NONE, b = TiledKernel::NONE, c = TiledKernel::NONE;  // NONE for a, c: no kernel of that length
    // k_colsw writes the slab tile-contiguously ([tile][k1][ring_cw]) when the last pass (k_rows32) can read it back
    uint32_t ring_cw = 0;      // 0 = matrix layout
    uint32_t passes = 2;
    uint32_t xcd_swizzle = 0;  // the plan's block -> tile map while the key "xcd_swizzle" is unset
    uint32_t families = 0;     // FAM_* of the chosen kernels
};

constexpr TiledSchedule resolve_tiled(uint32_t lg, const uint32_t lf[3], const TiledFlags &fl)
{
    using K = TiledKernel;
    TiledSchedule s;
    const bool three = lf[2] != 0, fits32 = lg <= fwa::LG_N_MAX_32;
    s.passes = three ? 3 : 2;
    s.a = fl.colsw && fwa::colsw_supported(lf[0]) && fits32  ? K::COLSW      // 256 x 64 / 512 x 32 column tiles
          : fwa::cols32_supported(lf[0]) && fits32            ? K::COLS32     // 2048-point columns
          : fwa::p1_gen_supported(lf[0]) && fl.p1_gen         ? K::P1_GEN     // the 2^20 column kernel at run-time pitch
          : fwa::tile_supported(lf[0])                        ? K::TILE_COLS
                                                              : K::NONE;
    if (three) s.b = fwa::tile_supported(lf[1]) ? K::TILE_COLS : K::NONE;
    if (s.a == K::COLSW && fl.tile_ring && !three && fwa::rows32_ring_supported(lf[1], fwa::colsw_width(lf[0])))
        s.ring_cw = fwa::colsw_width(lf[0]);
    const uint32_t last = lf[three ? 2 : 1];
    // 2048 / 4096-point rows and the tile ring exist only in k_rows32
    s.c = !three && fits32 && fwa::rows32_supported(last) && (fl.rows32 || last > 10 || s.ring_cw) ? K::ROWS32
          : fwa::tile_supported(last)                                                              ? K::TILE_ROWS
                                                                                                   : K::NONE;
    // Block -> tile map (xcd_map, device_common.h), measured per size at the 32-GiB footprint, three interleaved runs
    // (profiles/round4/sweep_tiled_block_maps.jsonl): the k_colsw plans gain 2-4 % from XCD-contiguous runs (2^17 .. 2^19:
    // bit 0; 2^16 and 1024 x 2048: with the CU pairs, bits 0 + 2); 2^22 and up lose 1-10 %.
    if (!three) {
        if (fl.colsw && lg == 16) s.xcd_swizzle = 5u;
        else if (fl.colsw && lg >= 17 && lg <= 19) s.xcd_swizzle = 1u;
        else if (lg == 21 && lf[0] == 10 && lf[1] == 11) s.xcd_swizzle = 5u;
    }
    s.families = kFamilyOf[(int)s.a] | kFamilyOf[(int)s.b] | kFamilyOf[(int)s.c];
    return s;
}

constexpr TiledFlags flag_setting(uint32_t i) { return TiledFlags{i & 1, (i >> 1) & 1, (i >> 2) & 1, (i >> 3) & 1}; }

// Every family some setting of the four flag keys can launch with these factors: what setup_path prepares, so that no
// flag key needs a setup of its own and no exec can meet a kernel whose LDS limit was never raised.
constexpr uint32_t families(uint32_t lg, const uint32_t lf[3])
{
    uint32_t f = 0;
    for (uint32_t i = 0; i < 16; ++i) f |= resolve_tiled(lg, lf, flag_setting(i)).families;
    return f;
}

// Every pass has a kernel of its length under some flag setting (the key "factors" checks the product itself).
constexpr bool factors_valid(uint32_t lg, const uint32_t lf[3])
{
    uint32_t ok = lf[2] ? 0u : 2u;  // bit 0 / 1 / 2: pass A / B / C
    for (uint32_t i = 0; i < 16; ++i) {
        const TiledSchedule s = resolve_tiled(lg, lf, flag_setting(i));
        ok |= (s.a != TiledKernel::NONE) | (s.b != TiledKernel::NONE) << 1 | (s.c != TiledKernel::NONE) << 2;
    }
    return ok == 7u;
}

// k_p1_gen's first-stage table (Tables::tw_inner) belongs to the tables of these factors
constexpr bool needs_inner_table(const uint32_t lf[3]) { return fwa::p1_gen_supported(lf[0]); }

}  // namespace fwa_int
