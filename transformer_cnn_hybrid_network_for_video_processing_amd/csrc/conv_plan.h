// Everything the HOST decides about the forward (or dgrad) conv3x3 of a non-first stage, decided once (a path decision
// is one predicate that the dispatcher and the size query both ask).  conv_fwd_plan() is pure host code; the dispatchers of conv_fwd.hip and
// conv_v2.hip launch what it says, and hyb_conv_dgrad_planar_ok, hyb_conv3x3_pool_fused, hyb_conv3x3_pool_ext, hyb_conv_stats_rows and
// hyb_conv3x3_fwd_variant return what it says.
#pragma once
#include "hyb_internal.h"

// kernel families; hyb_conv3x3_fwd_variant returns 100 * family + row
enum { CONV_GEN1 = 0, CONV_RING = 1, CONV_K32 = 2 };

// The asynchronous kernels (conv_v2.hip), one line per instantiated variant: X(family, row, NT, CB, PGR, PGC, R).  A workgroup is
// CB x PGR x PGC waves and covers a 4 PGR x 28 PGC pixel tile of CB * NT * 16 output channels; R = weight-ring depth (conv3x3_k32_kernel keeps
// its weights in registers: its geometry is V2Geom<2, CB, PGR, PGC, 3>).  Within a family the rows are ordered by channels per workgroup, and
// the rows of one channel count are the tile orientations the plan chooses between by cost (8 x 28 first: it wins ties).
// Measured on the 224 x 224 clip stages: two four-wave workgroups per CU (their epilogues and MFMA phases interleave) win up to 128 channels
// per workgroup; 256-channel blocks need the whole CU's LDS for a deep weight ring, i.e. one eight-wave workgroup.
#define HYB_CONV_ASYNC_ROWS(X)                                                                  \
    X(CONV_RING, 0, 2, 1, 4, 1, 4)                                                              \
    X(CONV_RING, 1, 2, 2, 2, 1, 4) X(CONV_RING, 2, 2, 2, 1, 2, 4)                               \
    X(CONV_RING, 3, 4, 2, 2, 1, 4) X(CONV_RING, 4, 4, 2, 1, 2, 4)                               \
    X(CONV_RING, 5, 4, 4, 2, 1, 6) X(CONV_RING, 6, 4, 4, 1, 2, 6)                               \
    X(CONV_K32, 0, 2, 2, 2, 1, 3) X(CONV_K32, 1, 2, 2, 1, 2, 3)
// The first-generation kernel (conv_fwd.hip: fp32 storage, HYB_CONV_V2=0, shapes the asynchronous kernels refuse): X(row, NT, CB, PG), a
// workgroup of 4 waves = CB channel blocks x PG pixel groups, tile 8 x 16 (PG 1), 16 x 16 (PG 2) or 16 x 32 (PG 4) pixels
#define HYB_CONV_GEN1_ROWS(X) X(0, 4, 4, 1) X(1, 4, 2, 2) X(2, 4, 1, 4) X(3, 2, 1, 4)

// Which asynchronous variants have an EXT instantiation.  The eight-wave ones with 64 channels per wave (NT = 4) do not: their STATS siblings
// already use all 256 registers and with the extremes each of them spills (88 - 124 bytes of scratch per lane).  A variant that spills is not
// built; its shapes keep the conv -> bn_relu_pool pair.
constexpr bool v2_ext_built(int NT, int NW) { return NT == 2 || NW == 4; }

struct ConvRow { int family, row, nt, th, tw, cbw, waves; bool pool, ext; };        // cbw = output channels per workgroup
constexpr ConvRow CONV_ASYNC_ROWS[] = {
#define X(FAM, ROW, NT, CB, PGR, PGC, R) {FAM, ROW, NT, 4 * PGR, 28 * PGC, CB * NT * 16, CB * PGR * PGC, true, v2_ext_built(NT, CB * PGR * PGC)},
    HYB_CONV_ASYNC_ROWS(X)
#undef X
};
constexpr int conv_gen1_th(int PG) { return PG == 1 ? 8 : 16; }
constexpr int conv_gen1_tw(int PG) { return PG == 4 ? 32 : 16; }
constexpr ConvRow CONV_GEN1_ROWS[] = {
#define X(ROW, NT, CB, PG) {CONV_GEN1, ROW, NT, conv_gen1_th(PG), conv_gen1_tw(PG), CB * NT * 16, 4, false, false},
    HYB_CONV_GEN1_ROWS(X)
#undef X
};
constexpr int CONV_MAX_STAT_ROWS = 512;       // partial-statistics rows of one conv at the most (hyb_conv_stats_workspace holds that many)
constexpr int CONV_FIRST_TH = 16, CONV_FIRST_TW = 32;       // tile of the first = 1 kernel of hyb_conv3x3_fwd (conv3x3_first_kernel)

struct ConvFwdPlan {
    ConvRow v;                          // the variant: family, table row, tile, POOL / EXT availability
    int tiles_x, tiles_y;
    long long num_tiles;
    int gy;                             // grid y: Cop / v.cbw
    int gx, gx_stats;                   // grid x without / with partial statistics (POOL / plain: gx; STATS / EXT: gx_stats)
    int stat_rows;                      // partial-statistics rows the caller is promised (hyb_conv_stats_rows): every one is written
    int code() const { return 100 * v.family + v.row; }
};

inline int conv_stat_rows(int N, int H, int W, int th, int tw) {
    const long long tiles = (long long)N * hyb_cdiv(W, tw) * hyb_cdiv(H, th);
    return (int)(tiles < CONV_MAX_STAT_ROWS ? tiles : CONV_MAX_STAT_ROWS);
}
// relative cost of covering N images of H x W with the row's tiles on 256 persistent workgroups
inline double conv_row_cost(const ConvRow& r, int N, int H, int W, int Cop) {
    const long long tiles = (long long)N * hyb_cdiv(W, r.tw) * hyb_cdiv(H, r.th) * (Cop / r.cbw);
    return (double)((tiles + 255) / 256) * r.th * r.tw;
}
// The row of `rows` for Cop output channels: of the rows (of `family`) with the most channels per workgroup that divide Cop, the cheapest;
// the first of equals.  No row divides Cop (not a multiple of 32: only hyb_conv_stats_rows is asked that): the last, narrowest one.
template <int NR>
inline ConvRow conv_pick_row(const ConvRow (&rows)[NR], int family, int N, int H, int W, int Cop) {
    const ConvRow* best = nullptr;
    for (const ConvRow& r : rows) {
        if (r.family != family || Cop % r.cbw != 0 || (best && r.cbw < best->cbw)) continue;
        if (!best || r.cbw > best->cbw || conv_row_cost(r, N, H, W, Cop) < conv_row_cost(*best, N, H, W, Cop)) best = &r;
    }
    return best ? *best : rows[NR - 1];
}

// Which shapes the asynchronous kernels take: every channel count that is a multiple of 32 has a variant; the bounds keep a halo row block
// and a weight block inside 32-bit buffer offsets
inline bool conv_async_shape_ok(int W, int Cip, int Cop) {
    return Cip > 0 && Cop > 0 && Cip % 32 == 0 && Cop % 32 == 0 && (long long)40 * W * Cip < (1ll << 29) && (long long)256 * 9 * Cip < (1ll << 29);
}

inline ConvFwdPlan conv_fwd_plan(int dtype, int N, int H, int W, int Cip, int Cop) {
    ConvFwdPlan p{};
    const ConvRow g1 = conv_pick_row(CONV_GEN1_ROWS, CONV_GEN1, N, H, W, Cop);
    // the asynchronous kernels write the row count of the first-generation tiling too (rows past their grid are zero-filled): the count
    // does not depend on HYB_CONV_V2, and the grid it gives fixes the order of the fixed-order sums
    p.stat_rows = conv_stat_rows(N, H, W, g1.th, g1.tw);
    if (dtype == HYB_BF16 && hyb_sw_conv_v2() && conv_async_shape_ok(W, Cip, Cop)) {
        // 32 input channels = one channel block per tile: weights in registers, one barrier per tile (conv3x3_k32_kernel, 64 channels per
        // workgroup); 256-channel blocks stay with the eight-wave ring kernel
        const bool k32 = Cip == 32 && Cop % 64 == 0 && Cop % 256 != 0;
        p.v = conv_pick_row(CONV_ASYNC_ROWS, k32 ? CONV_K32 : CONV_RING, N, H, W, Cop);
    } else {
        p.v = g1;
    }
    p.tiles_x = hyb_cdiv(W, p.v.tw);
    p.tiles_y = hyb_cdiv(H, p.v.th);
    p.num_tiles = (long long)N * p.tiles_x * p.tiles_y;
    p.gy = Cop / p.v.cbw;
    if (p.v.family == CONV_GEN1) {
        p.gx = p.gx_stats = p.stat_rows < 1 ? 1 : p.stat_rows;         // one partial row per workgroup
    } else {
        // persistent workgroups, each a contiguous run of ceil(num_tiles / gx) tiles (no run empty); with statistics never more than rows
        auto runs = [&](long long cap) {
            long long g = p.num_tiles < cap ? p.num_tiles : cap;
            if (g < 1) g = 1;
            return hyb_cdiv(p.num_tiles, hyb_cdiv(p.num_tiles, g));
        };
        const int slots = p.v.waves == 8 ? 256 : 512;                  // resident workgroups on 256 CUs
        p.gx = runs(slots);
        p.gx_stats = runs(slots < p.stat_rows ? slots : p.stat_rows);
    }
    return p;
}
// The part of the plan that N and H cannot change -- the family, the channels per workgroup and with them POOL / EXT: the orientations of one
// channel count share NT and the wave count -- for the queries that know only W and the channels
constexpr bool conv_orientations_agree() {
    for (const ConvRow& a : CONV_ASYNC_ROWS)
        for (const ConvRow& b : CONV_ASYNC_ROWS)
            if (a.family == b.family && a.cbw == b.cbw && (a.nt != b.nt || a.waves != b.waves || a.pool != b.pool || a.ext != b.ext)) return false;
    return true;
}
static_assert(conv_orientations_agree(), "the rows the cost comparison chooses between must differ in the tile only");
inline ConvRow conv_fwd_path(int dtype, int W, int Cip, int Cop) { return conv_fwd_plan(dtype, 1, 1, W, Cip, Cop).v; }
