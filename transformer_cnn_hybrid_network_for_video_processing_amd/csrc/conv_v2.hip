// conv3x3 (stride 1, zero pad 1), bf16, NHWC: the asynchronous implicit-GEMM kernel used for forward (nn.Conv2d of
// UNet.py:58) and dgrad (mode-1 packed weights) whenever the channel counts allow it.
//
// A workgroup is NW = CB x PGR x PGC waves (CB channel blocks x pixel groups), persistent over image tiles: either one
// 8-wave workgroup per CU (all 160 KiB of LDS: deep weight ring for 256-channel blocks) or two independent 4-wave workgroups
// per CU, whose epilogues (vector work) and MFMA phases interleave on the SIMDs.
//   * a wave owns a strip of 7 patches (4 x 28 pixels) x NT*16 output channels: 28 | 224/2^k, so the stages of a 224 x 224
//     clip tile without remainder in x;
//   * the input halo of a 32-channel block and the per-tap weight slices never pass through registers: both are written
//     into LDS by buffer_load_dwordx4 ... lds (LDS-DMA).  Out-of-image halo lanes are sent out of the descriptor's range and
//     the hardware writes zeros for them (the zero padding costs no branch).  Halo images are double buffered, weight slices
//     live in a ring of R slots, so the loads of block j+1 / step s+R-1 are in flight while block j / step s is computed;
//   * every wave issues the same, compile-time-known number of DMA instructions per step, which makes the only
//     synchronisation of a step one counted `s_waitcnt vmcnt(N)` + one raw `s_barrier` (no vmcnt(0) in the loop); after a
//     full-tile epilogue the count also steps over that tile's output stores, which stay in flight;
//   * the A fragments and the patch fragments of step s+1 are read from LDS between the MFMA groups of step s;
//   * output channels are permuted inside the MFMA tiles so that a lane ends up with 8 consecutive channels per 32-channel
//     half: an epilogue store instruction writes 64 contiguous bytes per pixel;
//   * the BatchNorm batch statistics (UNet.py:59) are folded into the epilogue from the fp32 accumulators, reduced in a fixed
//     order (bit-reproducible);
//   * POOL instantiations (inference, hyb_conv_v2_pool) never store the raw convolution: the epilogue applies the BatchNorm affine to the
//     fp32 accumulators, takes the 2 x 2 maximum across lanes, applies the ReLU and stores the pooled map (pool_affine_max below);
//   * EXT instantiations (training, hyb_conv_v2_ext) do everything the STATS ones do and also store, at a quarter of the resolution, the
//     raw extreme of every 2 x 2 window (pool_raw_extreme below): BatchNorm + ReLU + MaxPool2d then never re-read the raw output.
#include <type_traits>
#include "hyb_common.h"
#include "hyb_internal.h"
#include "conv_plan.h"

namespace {

typedef __attribute__((address_space(3))) void lds_void_t;

template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// LDS-DMA of 16 bytes per lane through a buffer descriptor: LDS destination = wave-uniform base + lane * 16, source =
// descriptor base + voff + soff.  A lane whose voff is outside the descriptor's range writes ZEROS (measured on gfx950):
// that is how the out-of-image part of a halo gets its zero padding, without a branch or a zero page.
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t rsrc, unsigned voff, unsigned soff, bf16* lds_dst_wave_base) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_void_t*)lds_dst_wave_base, 16, voff, soff, 0, 0);
}
constexpr unsigned V2_OOB = 0xfffffff0u;        // beyond every descriptor below (num_records = 2^31)
constexpr unsigned V2_RECORDS = 0x80000000u;

template <int S> using step_c = std::integral_constant<int, S>;

// ---- POOL epilogue: BatchNorm affine + MaxPool2d(2, 2) + ReLU on the accumulators ---------------------------------------------------------
// A lane holds pixel (py, px) = (p >> 2, p & 3) of a 4 x 4 patch, p = lane & 15; the other three pixels of its 2 x 2 window are lanes p ^ 1,
// p ^ 4 and p ^ 5 of the same 16-lane DPP row.  Two DPP exchanges per value, no LDS: quad_perm [1,0,3,2] brings lane p ^ 1, a row rotation by
// four brings the lane one patch row away.  Whichever way the rotation turns, the lanes on ONE side of it (py even or py odd) read the other
// row of their own window and end up with the whole window's maximum; pool_store_lane finds that side by rotating the lane index itself, so
// nothing here depends on the rotation's direction.  Affine before the maximum (the scale may be negative), ReLU after it (monotone), like
// bn_relu_pool_fwd_kernel -- but on fp32 accumulators, so the pooled value is rounded to bf16 once.
__device__ __forceinline__ float pool_affine_max(float acc, float scale, float shift) {
    float a = fmaf(acc, scale, shift);
    a = fmaxf(a, hyb_dpp_mov<0xB1>(a));          // quad_perm [1,0,3,2]: lane p ^ 1
    a = fmaxf(a, hyb_dpp_mov<0x124>(a));         // row_ror:4: lane p ^ 4 on the storing side
    return fmaxf(a, 0.f);
}
// the lanes that store a window: px even, and the patch row whose rotation partner is the window's other row
__device__ __forceinline__ bool pool_store_lane(int p) {
    const int partner = __builtin_amdgcn_update_dpp(0, p, 0x124, 0xf, 0xf, false);
    return partner == (p ^ 4) && !(p & 1);
}

// ---- EXT epilogue: the raw extreme of every 2 x 2 window, beside the raw output and its statistics (training) ---------------------------------
// Per channel v -> v * scale + shift is monotone and its direction is the sign of scale = gamma * invstd, i.e. of gamma (invstd > 0), which is
// known BEFORE the batch statistics are: max over the window of (y * scale + shift) = ext * scale + shift with ext the window's maximum of y
// where gamma >= 0 and its minimum where gamma < 0.  Rounding to bf16 is monotone too, so the extreme of the fp32 accumulators, rounded once,
// is the extreme of the bf16 values y_raw holds.  The minimum is the maximum between two flips of the sign bit (exact): `flip` is 0x80000000
// for a lane's channels with gamma < 0, else 0.  Lane mapping, exchanges and storing lanes are pool_affine_max's / pool_store_lane's.
// bn_relu_apply_pooled_kernel (bn_pool.hip) turns the stored extremes into relu(ext * scale + shift) in place once the statistics exist.
// (fmaxf would quiet both operands first -- the compiler cannot see that accumulators hold no signalling NaN -- three v_max_f32 per exchange;
// the instruction itself is all that is needed.)
__device__ __forceinline__ float raw_max(float a, float b) {
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float pool_raw_extreme(float acc, unsigned flip) {
    float a = __uint_as_float(__float_as_uint(acc) ^ flip);
    a = raw_max(a, hyb_dpp_mov<0xB1>(a));          // quad_perm [1,0,3,2]: lane p ^ 1
    a = raw_max(a, hyb_dpp_mov<0x124>(a));         // row_ror:4: lane p ^ 4 on the storing side
    return __uint_as_float(__float_as_uint(a) ^ flip);
}
// bit t * 4 + r of the result: the lane's accumulator value (t, r) belongs to a channel with gamma < 0 (channels >= Co: padding, never read)
template <int NT> __device__ __forceinline__ unsigned ext_negative_mask(const float* __restrict__ gamma, int Co, int co_base, int q) {
    unsigned m = 0;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int c = co_base + (t >> 1) * 32 + q * 8 + (t & 1) * 4 + r;
            if (c < Co && gamma[c] < 0.f) m |= 1u << (t * 4 + r);
        }
    return m;
}
__device__ __forceinline__ unsigned ext_flip(unsigned mask, int bit) { return (mask << (31 - bit)) & 0x80000000u; }
// what the EXT instantiations get beside the STATS arguments: the pooled map [N][H/2][W/2][Cop] to fill with extremes, and gamma[Co]
struct V2Ext { bf16* pooled; const float* gamma; int Co; };

template <int NT, int CB, int PGR, int PGC, int R>
struct V2Geom {
    static constexpr int PG = PGR * PGC, MT = 7;
    static constexpr int NW = CB * PG;                       // waves per workgroup: 8 (one workgroup per CU) or 4 (two per CU)
    static constexpr int TH = 4 * PGR, TW = 28 * PGC, HH = TH + 2, HW_ = TW + 2, HP = HH * HW_;
    static constexpr int NHW = (HP * 4 + 63) / 64;          // halo wave-instructions (64 x 16 B each)
    static constexpr int HT = (NHW + NW - 1) / NW;          // ... per wave
    static constexpr int HBUF = NHW * 512;                  // bf16 elements per halo buffer
    static constexpr int CBW = CB * NT * 16;                // output channels per workgroup
    static constexpr int WSLOT = CBW * 32;                  // bf16 elements per ring slot
    static constexpr int NWW = CBW / 16;                    // weight wave-instructions per slice
    static constexpr int WI = NWW >= NW ? NWW / NW : 1;     // ... per wave (duplicated when the slice has fewer pieces than waves)
    static constexpr int NHS = 10 - R;                      // halo pieces are issued in steps 0 .. NHS-1 (see wait rule)
    static constexpr int STAT_FLOATS = NW * 2 * NT * 16;
    static constexpr size_t LDS_BYTES = (size_t)(2 * HBUF + R * WSLOT) * 2 + STAT_FLOATS * 4;
    static_assert(NW == 8 || NW == 4, "four or eight waves");
    static_assert(LDS_BYTES <= (NW == 8 ? 160 : 80) * 1024, "160 KiB of LDS per CU");
    static_assert(HW_ % 4 == 2, "halo swizzle assumes halo width = 2 mod 4");
    static_assert(R >= 3 && R <= 6, "ring depth");
    // halo pieces of step s
    static constexpr int hi(int s) { s = ((s % 9) + 9) % 9; return s < NHS ? (HT + NHS - 1 - s) / NHS : 0; }
    static constexpr int hstart(int s) { int a = 0; for (int j = 0; j < s; ++j) a += hi(j); return a; }
    // DMA instructions younger than the weights of step s+2 when step s ends (= the vmcnt to wait for)
    static constexpr int wait_n(int s) {
        int n = hi(s - R + 3);
        for (int j = s - R + 4; j <= s; ++j) n += WI + hi(j);
        return n;
    }
    // the largest wait_n of the steps that step over a full tile's stores (S < R - 3)
    static constexpr int max_wait_after_store() { int n = 0; for (int s = 0; s < R - 3; ++s) n = wait_n(s) > n ? wait_n(s) : n; return n; }
};

// POOL: y is the pooled map [N][H/2][W/2][Cop] and `stats` carries the BatchNorm scale/shift rows [2][Cop] (read only)
// EXT (with STATS): also ext.pooled = the raw 2 x 2 extremes (pool_raw_extreme)
template <int NT, int CB, int PGR, int PGC, int R, bool STATS, bool POOL = false, bool EXT = false>
__global__ __launch_bounds__(CB * PGR * PGC * 64, CB * PGR * PGC == 4 ? 2 : 1) void conv3x3_v2_kernel(const bf16* __restrict__ x, const bf16* __restrict__ wp,
                                                            bf16* __restrict__ y, float* __restrict__ stats,
                                                            int N, int H, int W, int Cip, int Cop,
                                                            int tilesX, int tilesY, int numTiles, int stat_rows, int xpix, long long xblk, V2Ext ext) {
    // input addressing: element stride between pixels (Cip for NHWC) and between 32-channel blocks (32 for NHWC); a "block-planar"
    // input [Cip/32][N][H][W][32] has xpix = 32, xblk = N*H*W*32: a block's halo then uses whole 128-byte lines (see hyb_convstage_bwd)
    using G = V2Geom<NT, CB, PGR, PGC, R>;
    constexpr int MT = G::MT, TH = G::TH, TW = G::TW, HW_ = G::HW_, HP = G::HP, HT = G::HT, NHW = G::NHW;
    constexpr int CBW = G::CBW, WSLOT = G::WSLOT, NWW = G::NWW, WI = G::WI, PG = G::PG, NW = G::NW, NTHR = NW * 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    bf16* const hbuf = reinterpret_cast<bf16*>(smem_raw);                       // [2][HBUF]
    bf16* const wring = hbuf + 2 * G::HBUF;                                     // [R][WSLOT]
    float* const wgstat = reinterpret_cast<float*>(wring + R * WSLOT);          // [NW waves][2][NT*16]; POOL: scale/shift [2][CBW]
    static_assert(!(STATS && POOL), "the pooled epilogue keeps no batch statistics");
    static_assert(!POOL || NT >= 2, "the pooled epilogue stores whole 32-channel halves");
    static_assert(!EXT || (STATS && NT >= 2), "the extremes ride on the training epilogue and are stored as whole 32-channel halves");

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cb = wave % CB, pg = wave / CB;
    const int prow = pg / PGC, pstrip = pg % PGC;
    const int p = lane & 15, q = lane >> 4, py = p >> 2, px = p & 3;
    const int co_wg = blockIdx.y * CBW;
    const int co_base = co_wg + cb * (NT * 16);
    const int nCblk = Cip / 32;
    const long long wrow = (long long)9 * Cip;                                  // packed row: [Cip/32][9][32]

    if (STATS) {
        for (int i = tid; i < G::STAT_FLOATS; i += NTHR) wgstat[i] = 0.f;
    }
    if (POOL) {      // this workgroup's scale/shift: up to 32 values per lane at NT = 4, kept in LDS (2 CBW <= STAT_FLOATS) and read per tile
        for (int i = tid; i < 2 * CBW; i += NTHR) wgstat[i] = stats[(long long)(i / CBW) * Cop + co_wg + (i % CBW)];
        __syncthreads();
    }
    const bool pool_lane = (POOL || EXT) && pool_store_lane(p);
    const unsigned ext_neg = EXT ? ext_negative_mask<NT>(ext.gamma, ext.Co, co_base, q) : 0u;

    // ---- halo DMA pieces of this lane: byte offset from the halo origin pixel, and (hy, hx) for the bounds test
    constexpr bool HOFF_REG = true;              // large halos: recompute the offset per piece instead of holding it (registers)
    unsigned hoff[HOFF_REG ? HT : 1];
    int hyx[HT];
#pragma unroll
    for (int k = 0; k < HT; ++k) {
        int wi = k * NW + wave;
        if (wi > NHW - 1) wi = NHW - 1;                                         // duplicate the last piece: equal counts per wave
        const int u = wi * 64 + lane, hp = u >> 2, sp = u & 3;
        const int hy = hp / HW_, hx = hp - hy * HW_;
        const int s = sp ^ ((hy & 1) << 1);                                     // halo swizzle for 32-channel pixels
        if (HOFF_REG) hoff[k] = (unsigned)(((hy * W + hx) * xpix + s * 8) * 2);
        hyx[k] = hp < HP ? ((hy << 20) | (hx << 4) | s) : (0x7ff << 20);
    }
    // ---- weight DMA pieces of this lane: byte offset inside this workgroup's CBW packed rows
    unsigned woff[WI];
    int wdst[WI];
#pragma unroll
    for (int i = 0; i < WI; ++i) {
        const int wi = (i * NW + wave) % NWW;
        const int u = wi * 64 + lane, row = u >> 2, sp = u & 3;
        const int f = (4 - ((row >> 3) & 3)) & 3;
        woff[i] = (unsigned)(((long long)row * wrow + ((sp ^ f) << 3)) * 2);
        wdst[i] = wi * 512;
    }
    const __amdgpu_buffer_rsrc_t wrsrc = hyb_rsrc((wp + (long long)co_wg * wrow), V2_RECORDS);
    // ---- fragment addresses.  Row (t, p) of the MFMA tile holds channel (t>>1)*32 + (p>>2)*8 + (t&1)*4 + (p&3).
    const int aoff0 = (cb * (NT * 16) + (p >> 2) * 8 + (p & 3)) * 32 + ((q ^ ((4 - (p >> 2)) & 3)) << 3);
    auto aoff = [&](int t) { return aoff0 + ((t >> 1) * 32 + (t & 1) * 4) * 32; };
    const int lane_el = ((prow * 4 + py) * HW_ + pstrip * 28 + px) * 32;

    // block descriptors (wave-uniform)
    struct Blk { int n, ty0, tx0, cblk; };
    auto decode = [&](int tile, int cblk) {
        Blk b;
        b.n = tile / (tilesX * tilesY);
        const int trem = tile - b.n * (tilesX * tilesY);
        b.ty0 = (trem / tilesX) * TH;
        b.tx0 = (trem % tilesX) * TW;
        b.cblk = cblk;
        return b;
    };
    // descriptor of a block's halo: base = the halo origin pixel (may lie before the tensor for border tiles: such lanes are
    // sent out of range and never dereference it)
    auto halo_rsrc = [&](const Blk& b) {
        const long long base = ((long long)(b.n * H + b.ty0 - 1) * W + (b.tx0 - 1)) * xpix + b.cblk * xblk;
        return hyb_rsrc((x + base), V2_RECORDS);
    };
    auto halo_piece = [&](const Blk& b, __amdgpu_buffer_rsrc_t rs, bf16* hb, int k) {
        const int hy = hyx[k] >> 20, hx = (hyx[k] >> 4) & 0xffff;
        const int gy = b.ty0 - 1 + hy, gx = b.tx0 - 1 + hx;
        const bool valid = ((unsigned)gy < (unsigned)H) && ((unsigned)gx < (unsigned)W);
        const unsigned off = HOFF_REG ? hoff[HOFF_REG ? k : 0] : (unsigned)(((hy * W + hx) * xpix + (hyx[k] & 15) * 8) * 2);
        int wi = k * NW + wave;
        if (wi > NHW - 1) wi = NHW - 1;
        dma16(rs, valid ? off : V2_OOB, 0, hb + wi * 512);
    };
    auto weight_pieces = [&](int cblk, int tap, int slot) {
        const unsigned so = (unsigned)((cblk * 9 + tap) * 64);
#pragma unroll
        for (int i = 0; i < WI; ++i) dma16(wrsrc, woff[i], so, wring + slot * WSLOT + wdst[i]);
    };
    auto bptr_of = [&](const bf16* hb, int tap) {
        const int kh = tap / 3, kw = tap % 3;
        const int sw = ((py + kh) & 1) << 1;
        return hb + lane_el + (kh * HW_ + kw) * 32 + ((q ^ sw) << 3);
    };

    // a workgroup walks a contiguous run of tiles (row-major inside an image): the halo rows/columns neighbouring tiles share are
    // re-read from this XCD's L2.  The host sizes the grid so that no run is empty.
    const int tchunk = (numTiles + (int)gridDim.x - 1) / (int)gridDim.x;
    int tile = blockIdx.x * tchunk;
    const int tile_end = tile + tchunk < numTiles ? tile + tchunk : numTiles;
    Blk cur = decode(tile, 0);
    int hsel = 0, slot_cur = 0;
    bool after_store = false;                       // the previous block ended with a full-tile epilogue (NS stores per wave)
    // store instructions per wave of a full tile: one per patch and 32-channel half, and as many again (lane-masked) for the extremes
    constexpr int NS = (EXT ? 2 : 1) * MT * ((NT + 1) / 2);
    static_assert(G::max_wait_after_store() + NS <= 63, "the counted waits must fit vmcnt's six bits");

    // ---- prologue: halo of the first block, weights of steps 0 .. R-2
    {
        const __amdgpu_buffer_rsrc_t rs0 = halo_rsrc(cur);
#pragma unroll
        for (int k = 0; k < HT; ++k) halo_piece(cur, rs0, hbuf, k);
    }
#pragma unroll
    for (int s = 0; s < R - 1; ++s) weight_pieces(0, s, s);
    wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();

    Frag<bf16> a_cur[NT], bfr[MT];
#pragma unroll
    for (int t = 0; t < NT; ++t) frag_load(a_cur[t], wring + aoff(t));
    {
        const bf16* bp = bptr_of(hbuf, 0);
#pragma unroll
        for (int m = 0; m < MT; ++m) frag_load(bfr[m], bp + m * 128);
    }

    f32x4 acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};

    while (true) {
        // next block: the following channel block of this tile, else the first block of this workgroup's next tile
        const bool last_cblk = cur.cblk + 1 >= nCblk;
        const int ntile = last_cblk ? (tile + 1 < tile_end ? tile + 1 : tile) : tile;
        const Blk nxt = decode(ntile, last_cblk ? 0 : cur.cblk + 1);
        bf16* const hb_cur = hbuf + hsel * G::HBUF;
        bf16* const hb_nxt = hbuf + (hsel ^ 1) * G::HBUF;
        const __amdgpu_buffer_rsrc_t nrs = halo_rsrc(nxt);

        auto step = [&](auto S_) __attribute__((always_inline)) {
            constexpr int S = decltype(S_)::value;
            // (1) DMA: weights of step S+R-1 into the slot freed by step S-1, then this step's share of the next halo
            {
                constexpr int FT = (S + R - 1) % 9;
                const int fc = (S + R - 1 >= 9) ? nxt.cblk : cur.cblk;
                int slot_fill = slot_cur - 1;
                if (slot_fill < 0) slot_fill += R;
                weight_pieces(fc, FT, slot_fill);
#pragma unroll
                for (int k = 0; k < G::hi(S); ++k) halo_piece(nxt, nrs, hb_nxt, G::hstart(S) + k);
            }
            // (2) A fragments of step S+1 (their slot was published by the barrier that ended step S-1)
            int slot_next = slot_cur + 1;
            if (slot_next >= R) slot_next -= R;
            Frag<bf16> a_nxt[NT];
            {
                const bf16* as = wring + slot_next * WSLOT;
#pragma unroll
                for (int t = 0; t < NT; ++t) frag_load(a_nxt[t], as + aoff(t));
            }
            // (3) MFMAs of step S; each patch fragment is replaced by the one step S+1 needs as soon as it has been used
            const bf16* bp = bptr_of(S == 8 ? hb_nxt : hb_cur, (S + 1) % 9);
#pragma unroll
            for (int m = 0; m < MT; ++m) {
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[m][t] = mma32(a_cur[t], bfr[m], acc[m][t]);
                frag_load(bfr[m], bp + m * 128);
            }
            // pin the interleave: the LDS reads of step S+1 trickle out between the MFMA groups of step S
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                __builtin_amdgcn_sched_group_barrier(0x008, NT, 0);                      // MFMA
                if (m < NT) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);           // DS read (A of S+1 first, then patches)
                else __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) a_cur[t] = a_nxt[t];
            slot_cur = slot_next;
            // (4) the weights of step S+2 (and everything older) have landed for this wave; publish
            //     After a full-tile epilogue the NS output stores are younger than the weights waited for in the first R-3 steps
            //     (those were issued before the epilogue): counting them keeps the stores in flight instead of draining them.
            if constexpr (S < R - 3) {
                if (after_store) wait_vmcnt<G::wait_n(S) + NS>(); else wait_vmcnt<G::wait_n(S)>();
            } else {
                wait_vmcnt<G::wait_n(S)>();
            }
            __builtin_amdgcn_s_barrier();
        };
        step(step_c<0>{}); step(step_c<1>{}); step(step_c<2>{}); step(step_c<3>{}); step(step_c<4>{});
        step(step_c<5>{}); step(step_c<6>{}); step(step_c<7>{}); step(step_c<8>{});

        if (last_cblk) {
            // ---- epilogue: the lane holds 8 consecutive channels per 32-channel half of one pixel per patch
            const int n = cur.n, ty0 = cur.ty0, tx0 = cur.tx0;
            const bool full = (ty0 + TH <= H) && (tx0 + TW <= W);
            float s1[NT][4], s2[NT][4];
            if (STATS) {
#pragma unroll
                for (int t = 0; t < NT; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) { s1[t][r] = 0.f; s2[t][r] = 0.f; }
            }
            const int gy = ty0 + prow * 4 + py;
            auto emit_pool = [&](auto FULL_) __attribute__((always_inline)) {
                constexpr bool FULL = decltype(FULL_)::value;
                f32x4 sc[NT], sh[NT];
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const float* sp = wgstat + cb * (NT * 16) + (t >> 1) * 32 + q * 8 + (t & 1) * 4;
                    sc[t] = *reinterpret_cast<const f32x4*>(sp);
                    sh[t] = *reinterpret_cast<const f32x4*>(sp + CBW);
                }
                const int Ho = H >> 1, Wo = W >> 1;
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    const int gx = tx0 + pstrip * 28 + m * 4 + px;
                    Vec8<bf16> v[(NT + 1) / 2];
#pragma unroll
                    for (int t = 0; t < NT; ++t)
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[t >> 1].set((t & 1) * 4 + r, pool_affine_max(acc[m][t][r], sc[t][r], sh[t][r]));
                    // floor semantics (bn_relu_pool_fwd_kernel): a window exists when both of its rows and columns are inside the image;
                    // a full tile issues exactly NS lane-masked store instructions per wave
                    if (pool_lane && (FULL || (((gy | 1) < H) && ((gx | 1) < W)))) {
                        bf16* dst = y + ((long long)(n * Ho + (gy >> 1)) * Wo + (gx >> 1)) * Cop + co_base + q * 8;
#pragma unroll
                        for (int h = 0; h < (NT + 1) / 2; ++h) v[h].store(dst + h * 32);
                    }
#pragma unroll
                    for (int t = 0; t < NT; ++t) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
            };
            auto emit_raw = [&](auto FULL_) __attribute__((always_inline)) {
                constexpr bool FULL = decltype(FULL_)::value;
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    const int gx = tx0 + pstrip * 28 + m * 4 + px;
                    const bool valid = FULL || ((gy < H) && (gx < W));
                    if (valid) {
                        bf16* dst = y + ((long long)(n * H + gy) * W + gx) * Cop + co_base + q * 8;
#pragma unroll
                        for (int h = 0; h < (NT + 1) / 2; ++h) {
                            Vec8<bf16> v;
#pragma unroll
                            for (int j = 0; j < 8; ++j) v.set(j, acc[m][NT == 1 ? 0 : h * 2 + (j >> 2)][j & 3]);
                            v.store(dst + h * 32);
                        }
                        if (STATS) {
#pragma unroll
                            for (int t = 0; t < NT; ++t)
#pragma unroll
                                for (int r = 0; r < 4; ++r) {
                                    const float v = acc[m][t][r];
                                    s1[t][r] += v;
                                    s2[t][r] = fmaf(v, v, s2[t][r]);
                                }
                        }
                    }
                    if constexpr (EXT) {     // every lane takes part in the exchanges; windows follow emit_pool's floor rule and store count
                        // One 32-channel half at a time, fenced: left to itself the scheduler starts both halves of several patches at once and
                        // the 64-channel variants, whose STATS siblings already use all 256 registers, spill.
                        const bool st_lane = pool_lane && (FULL || (((gy | 1) < H) && ((gx | 1) < W)));
                        bf16* dst = ext.pooled + ((long long)(n * (H >> 1) + (gy >> 1)) * (W >> 1) + (gx >> 1)) * Cop + co_base + q * 8;
#pragma unroll
                        for (int h = 0; h < (NT + 1) / 2; ++h) {
                            __builtin_amdgcn_sched_barrier(0);
                            Vec8<bf16> e;
#pragma unroll
                            for (int j = 0; j < 8; ++j) e.set(j, pool_raw_extreme(acc[m][h * 2 + (j >> 2)][j & 3], ext_flip(ext_neg, h * 8 + j)));
                            if (st_lane) e.store(dst + h * 32);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
#pragma unroll
                    for (int t = 0; t < NT; ++t) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
            };
            auto emit = [&](auto FULL_) __attribute__((always_inline)) {
                if constexpr (POOL) emit_pool(FULL_); else emit_raw(FULL_);
            };
            if (full) {
                emit(std::true_type{});          // exactly NS store instructions per wave: the next waits step over them by count
                after_store = true;
            } else {
                emit(std::false_type{});         // edge tile: the store count depends on the lane masks, so drain instead
                wait_vmcnt<0>();
                after_store = false;
            }
            if (STATS) {
#pragma unroll
                for (int t = 0; t < NT; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float a = row16_sum(s1[t][r]), b = row16_sum(s2[t][r]);
                        if (p == 0) {
                            const int cl = (t >> 1) * 32 + q * 8 + (t & 1) * 4 + r;
                            wgstat[(wave * 2 + 0) * (NT * 16) + cl] += a;
                            wgstat[(wave * 2 + 1) * (NT * 16) + cl] += b;
                        }
                    }
            }
            if (tile + 1 >= tile_end) break;
            ++tile;
        }
        else after_store = false;
        cur = nxt;
        hsel ^= 1;
    }

    wait_vmcnt<0>();                 // the run-ahead DMA of the (non-existent) next block must not outlive the workgroup
    if (STATS) {
        __syncthreads();
        for (int i = tid; i < 2 * CBW; i += NTHR) {
            const int which = i / CBW, cl = i % CBW;
            const int cbi = cl / (NT * 16), c16 = cl % (NT * 16);
            float a = 0.f;
#pragma unroll
            for (int g = 0; g < PG; ++g) a += wgstat[((g * CB + cbi) * 2 + which) * (NT * 16) + c16];     // wave = pg*CB + cb
            stats[((long long)blockIdx.x * 2 + which) * Cop + co_wg + cl] = a;
            // the caller sums a fixed number of partial rows: rows no workgroup owns are zero
            for (int rrow = blockIdx.x + gridDim.x; rrow < stat_rows; rrow += gridDim.x) stats[((long long)rrow * 2 + which) * Cop + co_wg + cl] = 0.f;
        }
    }
}

// ---- 32 input channels (one channel block per tile): the weights live in REGISTERS ------------------------------------------------------
// conv3x3_v2_kernel synchronises once per (tap, channel block) step -- the price of streaming weight slices through an LDS ring.  With
// Cip = 32 a step is only MT x NT = 14 MFMAs per wave (224 matrix-pipe cycles) and the barrier, the counted wait and the ring traffic cost as
// much as the arithmetic: stage 2's forward conv (32 -> 64 channels, 308 MB) ran at 3.6 TB/s, memory-bound on paper.  Here a wave keeps all
// nine taps' fragments of its 32 output channels (72 registers) for the whole kernel, the halo images are a ring of THREE filled two tiles
// ahead by LDS-DMA, and a tile costs ONE counted wait + ONE barrier.  Same tiles, fragment layout, swizzle, epilogue and statistics order
// per tile as conv3x3_v2_kernel<2, CB, PGR, PGC, .>; the per-lane statistics are folded across lanes once, at the end.
// POOL: as conv3x3_v2_kernel; the 16 scale/shift values of a lane live in the registers the statistics of the STATS sibling use.
// EXT: as conv3x3_v2_kernel.
template <int CB, int PGR, int PGC, bool STATS, bool POOL = false, bool EXT = false>
__global__ __launch_bounds__(CB * PGR * PGC * 64, 2) void conv3x3_k32_kernel(const bf16* __restrict__ x, const bf16* __restrict__ wp, bf16* __restrict__ y,
                                                                            float* __restrict__ stats, int N, int H, int W, int Cip, int Cop, int tilesX,
                                                                            int tilesY, int numTiles, int stat_rows, int xpix, long long xblk, V2Ext ext) {
    constexpr int NT = 2, HBN = 3;
    using G = V2Geom<NT, CB, PGR, PGC, 3>;
    constexpr int MT = G::MT, TH = G::TH, TW = G::TW, HW_ = G::HW_, HP = G::HP, HT = G::HT, NHW = G::NHW, CBW = G::CBW, PG = G::PG, NW = G::NW,
                  NTHR = NW * 64;
    static_assert(NW == 4, "two four-wave workgroups per CU");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    bf16* const hbuf = reinterpret_cast<bf16*>(smem_raw);                       // [3][HBUF]
    float* const wgstat = reinterpret_cast<float*>(hbuf + HBN * G::HBUF);       // [NW waves][2][NT*16]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cb = wave % CB, pg = wave / CB;
    const int prow = pg / PGC, pstrip = pg % PGC;
    const int p = lane & 15, q = lane >> 4, py = p >> 2, px = p & 3;
    const int co_wg = blockIdx.y * CBW;
    const int co_base = co_wg + cb * (NT * 16);
    const long long wrow = (long long)9 * Cip;
    (void)xblk;
    static_assert(!(STATS && POOL), "the pooled epilogue keeps no batch statistics");
    static_assert(!EXT || STATS, "the extremes ride on the training epilogue");
    f32x4 sc[NT], sh[NT];
    if (POOL) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const float* sp = stats + co_base + (t >> 1) * 32 + q * 8 + (t & 1) * 4;
            sc[t] = *reinterpret_cast<const f32x4*>(sp);
            sh[t] = *reinterpret_cast<const f32x4*>(sp + Cop);
        }
    }
    const bool pool_lane = (POOL || EXT) && pool_store_lane(p);
    const unsigned ext_neg = EXT ? ext_negative_mask<NT>(ext.gamma, ext.Co, co_base, q) : 0u;

    // the wave's weights: row (t, p) of the MFMA tile holds channel (t >> 1) * 32 + (p >> 2) * 8 + (t & 1) * 4 + (p & 3) (conv3x3_v2_kernel)
    Frag<bf16> aw[9][NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const bf16* row = wp + (long long)(co_base + (t >> 1) * 32 + (p >> 2) * 8 + (t & 1) * 4 + (p & 3)) * wrow + 8 * q;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) frag_load(aw[tap][t], row + tap * 32);
    }
    unsigned hoff[HT];
    int hyx[HT];
#pragma unroll
    for (int k = 0; k < HT; ++k) {
        int wi = k * NW + wave;
        if (wi > NHW - 1) wi = NHW - 1;
        const int u = wi * 64 + lane, hp = u >> 2, sp = u & 3;
        const int hy = hp / HW_, hx = hp - hy * HW_;
        const int s = sp ^ ((hy & 1) << 1);
        hoff[k] = (unsigned)(((hy * W + hx) * xpix + s * 8) * 2);
        hyx[k] = hp < HP ? ((hy << 20) | (hx << 4) | s) : (0x7ff << 20);
    }
    const int lane_el = ((prow * 4 + py) * HW_ + pstrip * 28 + px) * 32;
    struct Tl { int n, ty0, tx0; };
    auto decode = [&](int tile) {
        Tl b;
        b.n = tile / (tilesX * tilesY);
        const int trem = tile - b.n * (tilesX * tilesY);
        b.ty0 = (trem / tilesX) * TH;
        b.tx0 = (trem % tilesX) * TW;
        return b;
    };
    auto halo_dma = [&](const Tl& b, bf16* hb) {
        const long long base = ((long long)(b.n * H + b.ty0 - 1) * W + (b.tx0 - 1)) * xpix;
        const __amdgpu_buffer_rsrc_t rs = hyb_rsrc((x + base), V2_RECORDS);
#pragma unroll
        for (int k = 0; k < HT; ++k) {
            const int hy = hyx[k] >> 20, hx = (hyx[k] >> 4) & 0xffff;
            const int gy = b.ty0 - 1 + hy, gx = b.tx0 - 1 + hx;
            const bool valid = ((unsigned)gy < (unsigned)H) && ((unsigned)gx < (unsigned)W);
            int wi = k * NW + wave;
            if (wi > NHW - 1) wi = NHW - 1;
            dma16(rs, valid ? hoff[k] : V2_OOB, 0, hb + wi * 512);
        }
    };
    auto bptr_of = [&](const bf16* hb, int tap) {
        const int kh = tap / 3, kw = tap % 3;
        const int sw = ((py + kh) & 1) << 1;
        return hb + lane_el + (kh * HW_ + kw) * 32 + ((q ^ sw) << 3);
    };

    const int tchunk = (numTiles + (int)gridDim.x - 1) / (int)gridDim.x;
    const int tile0 = blockIdx.x * tchunk;
    const int tile_end = tile0 + tchunk < numTiles ? tile0 + tchunk : numTiles;
    const int ntiles = tile_end - tile0;
    auto tl = [&](int i) { return decode(tile0 + (i < ntiles ? i : ntiles - 1)); };
    constexpr int NS = (EXT ? 2 : 1) * MT * ((NT + 1) / 2);       // stores per wave of a full tile (conv3x3_v2_kernel)
    static_assert(HT + 2 * NS <= 63, "the counted waits must fit vmcnt's six bits");

    halo_dma(tl(0), hbuf);
    halo_dma(tl(1), hbuf + G::HBUF);
    wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();

    Frag<bf16> bfr[MT];
    {
        const bf16* bp = bptr_of(hbuf, 0);
#pragma unroll
        for (int m = 0; m < MT; ++m) frag_load(bfr[m], bp + m * 128);
    }
    f32x4 acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    float s1[NT][4], s2[NT][4];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) { s1[t][r] = 0.f; s2[t][r] = 0.f; }

    int hsel = 0;
    bool prev_full = false;
    for (int it = 0; it < ntiles; ++it) {
        const Tl cur = tl(it);
        const int h1 = hsel + 1 >= HBN ? 0 : hsel + 1, h2 = h1 + 1 >= HBN ? 0 : h1 + 1;
        const bf16* hb_cur = hbuf + hsel * G::HBUF;
        const bf16* hb_nxt = hbuf + h1 * G::HBUF;
        halo_dma(tl(it + 2), hbuf + h2 * G::HBUF);            // two tiles ahead; its image was tile it - 1's: every wave left it at the last barrier
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const bf16* bp = bptr_of(tap == 8 ? hb_nxt : hb_cur, (tap + 1) % 9);
#pragma unroll
            for (int m = 0; m < MT; ++m) {
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[m][t] = mma32(aw[tap][t], bfr[m], acc[m][t]);
                frag_load(bfr[m], bp + m * 128);
            }
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                __builtin_amdgcn_sched_group_barrier(0x008, NT, 0);                      // MFMA
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                       // DS read
            }
        }
        // ---- epilogue (conv3x3_v2_kernel's): the lane holds 8 consecutive channels of one pixel per patch
        const int n = cur.n, ty0 = cur.ty0, tx0 = cur.tx0;
        const bool full = (ty0 + TH <= H) && (tx0 + TW <= W);
        const int gy = ty0 + prow * 4 + py;
        auto emit_pool = [&](auto FULL_) __attribute__((always_inline)) {
            constexpr bool FULL = decltype(FULL_)::value;
            const int Ho = H >> 1, Wo = W >> 1;
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const int gx = tx0 + pstrip * 28 + m * 4 + px;
                Vec8<bf16> v;
#pragma unroll
                for (int j = 0; j < 8; ++j) v.set(j, pool_affine_max(acc[m][j >> 2][j & 3], sc[j >> 2][j & 3], sh[j >> 2][j & 3]));
                if (pool_lane && (FULL || (((gy | 1) < H) && ((gx | 1) < W))))       // full tile: exactly NS lane-masked stores per wave
                    v.store(y + ((long long)(n * Ho + (gy >> 1)) * Wo + (gx >> 1)) * Cop + co_base + q * 8);
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        };
        auto emit_raw = [&](auto FULL_) __attribute__((always_inline)) {
            constexpr bool FULL = decltype(FULL_)::value;
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const int gx = tx0 + pstrip * 28 + m * 4 + px;
                const bool valid = FULL || ((gy < H) && (gx < W));
                if (valid) {
                    bf16* dst = y + ((long long)(n * H + gy) * W + gx) * Cop + co_base + q * 8;
                    Vec8<bf16> v;
#pragma unroll
                    for (int j = 0; j < 8; ++j) v.set(j, acc[m][j >> 2][j & 3]);
                    v.store(dst);
                    if (STATS) {
#pragma unroll
                        for (int t = 0; t < NT; ++t)
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const float a = acc[m][t][r];
                                s1[t][r] += a;
                                s2[t][r] = fmaf(a, a, s2[t][r]);
                            }
                    }
                }
                if constexpr (EXT) {         // every lane takes part in the exchanges; windows follow emit_pool's floor rule and store count
                    Vec8<bf16> e;
#pragma unroll
                    for (int j = 0; j < 8; ++j) e.set(j, pool_raw_extreme(acc[m][j >> 2][j & 3], ext_flip(ext_neg, j)));
                    if (pool_lane && (FULL || (((gy | 1) < H) && ((gx | 1) < W))))
                        e.store(ext.pooled + ((long long)(n * (H >> 1) + (gy >> 1)) * (W >> 1) + (gx >> 1)) * Cop + co_base + q * 8);
                }
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        };
        auto emit = [&](auto FULL_) __attribute__((always_inline)) {
            if constexpr (POOL) emit_pool(FULL_); else emit_raw(FULL_);
        };
        // the next tile's halo (issued one iteration ago) must have landed: in issue order the outstanding operations are [this wave's DMA pieces of
        // iteration it - 1] [its NS stores, if that tile was full] [HT pieces of this iteration] [NS stores]: leave the last three groups in flight
        if (full) {
            emit(std::true_type{});
            if (prev_full) wait_vmcnt<HT + 2 * NS>(); else wait_vmcnt<HT + NS>();
        } else {
            emit(std::false_type{});         // edge tile: the store count depends on the lane masks, so drain
            wait_vmcnt<0>();
        }
        prev_full = full;
        __builtin_amdgcn_s_barrier();
        hsel = h1;
    }
    wait_vmcnt<0>();                 // the run-ahead DMA must not outlive the workgroup
    if (STATS) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float a = row16_sum(s1[t][r]), b = row16_sum(s2[t][r]);
                if (p == 0) {
                    const int cl = (t >> 1) * 32 + q * 8 + (t & 1) * 4 + r;
                    wgstat[(wave * 2 + 0) * (NT * 16) + cl] = a;
                    wgstat[(wave * 2 + 1) * (NT * 16) + cl] = b;
                }
            }
        __syncthreads();
        for (int i = tid; i < 2 * CBW; i += NTHR) {
            const int which = i / CBW, cl = i % CBW;
            const int cbi = cl / (NT * 16), c16 = cl % (NT * 16);
            float a = 0.f;
#pragma unroll
            for (int g = 0; g < PG; ++g) a += wgstat[((g * CB + cbi) * 2 + which) * (NT * 16) + c16];     // wave = pg*CB + cb
            stats[((long long)blockIdx.x * 2 + which) * Cop + co_wg + cl] = a;
            for (int rrow = blockIdx.x + gridDim.x; rrow < stat_rows; rrow += gridDim.x) stats[((long long)rrow * 2 + which) * Cop + co_wg + cl] = 0.f;
        }
    }
}

// One line of HYB_CONV_ASYNC_ROWS as the launcher sees it: the kernel of each flavour, its geometry and its LDS size
template <int FAM, int NT, int CB, int PGR, int PGC, int R>
struct V2Variant {
    using G = V2Geom<NT, CB, PGR, PGC, R>;
    static constexpr bool K32 = FAM == CONV_K32;
    static constexpr size_t LDS = K32 ? (size_t)3 * G::HBUF * 2 + G::STAT_FLOATS * 4 : G::LDS_BYTES;      // (k32: three halo images, no weight ring)
    static constexpr bool HAS_EXT = v2_ext_built(NT, G::NW);
    static_assert(!K32 || (NT == 2 && R == 3 && G::NW == 4 && LDS <= 80 * 1024), "conv3x3_k32_kernel: V2Geom<2, CB, PGR, PGC, 3>, two workgroups per CU");
    template <bool STATS, bool POOL, bool EXT> static constexpr auto kernel() {
        if constexpr (K32) return &conv3x3_k32_kernel<CB, PGR, PGC, STATS, POOL, EXT>;
        else return &conv3x3_v2_kernel<NT, CB, PGR, PGC, R, STATS, POOL, EXT>;
    }
};

// xblk / xpix: see conv3x3_v2_kernel.  ss != NULL (with part == NULL): the POOL instantiation, y = the pooled map; ext.pooled != NULL (with
// part): the EXT instantiation
struct V2Args { const bf16* x; const bf16* wp; bf16* y; float* part; const float* ss; int N, H, W, Cip, Cop, xpix; long long xblk; V2Ext ext; hipStream_t st; };

template <class V, bool STATS, bool POOL, bool EXT>
int launch_flavour(const ConvFwdPlan& p, const V2Args& a) {
    static HybAttrOnce once;                                   // per kernel instantiation, per device
    const auto kernel = V::template kernel<STATS, POOL, EXT>();
    if (int e = hyb_set_lds_attr(once, (const void*)kernel, (int)V::LDS)) return e;
    hipLaunchKernelGGL(kernel, dim3(STATS ? p.gx_stats : p.gx, p.gy), dim3(V::G::NW * 64), V::LDS, a.st, a.x, a.wp, a.y, POOL ? const_cast<float*>(a.ss) : a.part,
                       a.N, a.H, a.W, a.Cip, a.Cop, p.tiles_x, p.tiles_y, (int)p.num_tiles, STATS ? p.stat_rows : 0, a.xpix, a.xblk, EXT ? a.ext : V2Ext{});
    HYB_LAUNCH_CHECK();
    return 0;
}
template <class V>
int launch_variant(const ConvFwdPlan& p, const V2Args& a) {
    if (a.ss) return launch_flavour<V, false, true, false>(p, a);
    if (a.ext.pooled) {
        if constexpr (V::HAS_EXT) return a.part ? launch_flavour<V, true, false, true>(p, a) : HYB_E_ARG;
        else return HYB_NO_VARIANT;
    }
    return a.part ? launch_flavour<V, true, false, false>(p, a) : launch_flavour<V, false, false, false>(p, a);
}

// p = conv_fwd_plan of this shape; HYB_NO_VARIANT when it is not an asynchronous one.  part: partial-statistics rows [plan.stat_rows][2][Cop] (may be
// NULL), all of them written.  xblk = 0: NHWC input; else the block-planar input's block stride in elements (see conv3x3_v2_kernel)
int conv_v2_dispatch(const ConvFwdPlan& p, const void* x, const void* wp, void* y, float* part, const float* ss, int N, int H, int W, int Cip, int Cop, hipStream_t st,
                     long long xblk, V2Ext ext = V2Ext{}) {
    const V2Args a{(const bf16*)x, (const bf16*)wp, (bf16*)y, part, ss, N, H, W, Cip, Cop, xblk ? 32 : Cip, xblk ? xblk : 32, ext, st};
    switch (p.code()) {
#define X(FAM, ROW, NT, CB, PGR, PGC, R) case 100 * FAM + ROW: return launch_variant<V2Variant<FAM, NT, CB, PGR, PGC, R>>(p, a);
        HYB_CONV_ASYNC_ROWS(X)
#undef X
    }
    return HYB_NO_VARIANT;
}

}  // namespace

// Internal (conv_fwd.hip): y = conv3x3(x, wp), with the partial statistics when part != NULL
int hyb_conv_v2(const ConvFwdPlan& p, const void* x, const void* wp, void* y, float* part, int N, int H, int W, int Cip, int Cop, hipStream_t st, long long xblk) {
    return conv_v2_dispatch(p, x, wp, y, part, nullptr, N, H, W, Cip, Cop, st, xblk);
}

// Internal (hyb_convstage_infer): pooled[N][H/2][W/2][Cop] = maxpool2x2(relu(conv3x3(x, wp) * scale + shift)), ss = [2][Cop] scale | shift, the raw
// convolution never stored.  HYB_NO_VARIANT for the shapes hyb_conv_v2 does not take.
int hyb_conv_v2_pool(const ConvFwdPlan& p, const void* x, const void* wp, void* pooled, const float* ss, int N, int H, int W, int Cip, int Cop, hipStream_t st) {
    if (!ss || H < 2 || W < 2) return HYB_NO_VARIANT;
    return conv_v2_dispatch(p, x, wp, pooled, nullptr, ss, N, H, W, Cip, Cop, st, 0);
}

// Internal (hyb_conv3x3_fwd_ext): hyb_conv_v2 with partial statistics, and pooled[N][H/2][W/2][Cop] = the raw extreme of every 2 x 2 window of y
// (its maximum where gamma >= 0, its minimum where gamma < 0; channels >= Co count as non-negative).  HYB_NO_VARIANT as hyb_conv_v2.
int hyb_conv_v2_ext(const ConvFwdPlan& p, const void* x, const void* wp, void* y, float* part, void* pooled, const float* gamma, int Co, int N, int H, int W, int Cip, int Cop,
                    hipStream_t st) {
    if (!part || !pooled || !gamma || H < 2 || W < 2 || Co < 1 || Co > Cop) return HYB_E_ARG;
    return conv_v2_dispatch(p, x, wp, y, part, nullptr, N, H, W, Cip, Cop, st, 0, V2Ext{(bf16*)pooled, gamma, Co});
}
