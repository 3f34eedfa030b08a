// orb_kernels.hip -- hand-written gfx950 kernels for ORBextractor::operator()
// (reference: corbslam_client/src/ORBextractor.cc:1043-1105 and the routines it calls).
//
// Launch sequence per (half-)batch of images, corb_launch_orb_pipeline():
//   orb_pyramid_kernel                ComputePyramid, all levels  (:1107-1132, cv::resize INTER_LINEAR; orb_resize_kernel per level = fallback for tiny images)
//   orb_fast_kernel                   per-cell FAST-9/16 + NMS    (:789-829,  cv::FAST)
//   orb_octree_kernel                 DistributeOctTree           (:539-763), one workgroup per (image, level)
//   orb_blur_kernel                   7x7 Gaussian, sigma 2       (:1085-1086, cv::GaussianBlur)
//   orb_describe_kernel               IC_Angle + steered BRIEF + output assembly (:77-147, :1075-1104)
//
// Integer paths are bit-exact restatements; float paths use explicit non-fused IEEE operations
// (__fmul_rn/__fadd_rn/...), so results do not depend on compiler contraction.
#include "corb_internal.h"
#include "lane_exchange.h"
#include "orb_fast_tile.h"
#include <atomic>
#include <cstring>
#include <cstdlib>
#include "brief_pattern.h"

#define WAVE 64

// per-lane constants of orb_describe_kernel, filled once by corb_orb_device_init():
//   patb[lane] = the BRIEF test pairs 64 r + lane (r = 0..3) of the lane, one dword per pair: bytes {x0, x1, y0, y1} + 16
struct CorbDescribeTab { uint4 patb[64]; };
__device__ CorbDescribeTab g_dsc_tab;


// ------------------------------------------------------------------------------------------------
// cv::resize(8UC1, INTER_LINEAR): 11-bit fixed-point, horizontal then vertical (OpenCV 2.4.8 scalar).
// Tables (host-built, same arithmetic as the oracle): xofs | xa0 | xa1 | ys0 | ys1 | yb0 | yb1
#define RS_ROWS 8
__global__ __launch_bounds__(256) void orb_resize_kernel(const CorbOrbParams p, int level)
{
    // one thread: 4 adjacent output pixels x RS_ROWS output rows (x tables loaded once, rows pipelined)
    const CorbLevel& D = p.lv[level];
    const CorbLevel& S = p.lv[level - 1];
    const int img = p.img_base + blockIdx.z;
    const int x4 = (blockIdx.x * 64 + threadIdx.x) * 4;
    const int yb = (blockIdx.y * 4 + threadIdx.y) * RS_ROWS;
    if (x4 >= D.w || yb >= D.h) return;
    const short* tab = p.resize_tab + D.resize_tab_off;
    const short* xofs = tab, * xa0 = tab + D.w, * xa1 = tab + 2 * D.w;
    const short* ys0 = tab + 3 * D.w, * ys1 = ys0 + D.h, * yb0 = ys1 + D.h, * yb1 = yb0 + D.h;
    const uint8_t* src = p.pyr + (size_t)img * p.arena_per_image + S.plane_off;
    uint8_t* dstp = p.pyr + (size_t)img * p.arena_per_image + D.plane_off;
    int sx[4], sx1[4], a0[4], a1[4];
    int nvalid = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int x = min(x4 + k, D.w - 1);
        sx[k] = xofs[x]; sx1[k] = min(sx[k] + 1, S.w - 1); a0[k] = xa0[x]; a1[k] = xa1[x];
        nvalid += (x4 + k < D.w) ? 1 : 0;
    }
    const int yend = min(yb + RS_ROWS, D.h);
#pragma unroll 2
    for (int y = yb; y < yend; y++) {
        const uint8_t* S0 = src + (size_t)ys0[y] * S.pitch;
        const uint8_t* S1 = src + (size_t)ys1[y] * S.pitch;
        const int b0 = yb0[y], b1 = yb1[y];
        uint32_t packed = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int d0 = __mul24(S0[sx[k]], a0[k]) + __mul24(S0[sx1[k]], a1[k]);
            const int d1 = __mul24(S1[sx[k]], a0[k]) + __mul24(S1[sx1[k]], a1[k]);
            const uint32_t v = (uint32_t)((((__mul24(b0, d0 >> 4)) >> 16) + ((__mul24(b1, d1 >> 4)) >> 16) + 2) >> 2) & 0xFFu;   // operands < 2^24
            packed |= v << (8 * k);
        }
        uint8_t* dst = dstp + (size_t)y * D.pitch + x4;
        if (nvalid == 4) *reinterpret_cast<uint32_t*>(dst) = packed;
        else for (int k = 0; k < nvalid; k++) dst[k] = (uint8_t)(packed >> (8 * k));
    }
}

// 24-bit multiplies, spelled out: the compiler turns __mul24 into a 32-bit v_mul_lo_u32 / 64-bit mads whenever its range
// analysis loses track of the operands
__device__ __forceinline__ uint32_t mul24u(uint32_t a, uint32_t b) { uint32_t d; asm("v_mul_u32_u24 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b)); return d; }
__device__ __forceinline__ uint32_t mad24u(uint32_t a, uint32_t b, uint32_t c) { uint32_t d; asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c)); return d; }
// SDWA forms: the sub-dword operand select is free, so a byte / word extract costs no instruction of its own
template <int B> __device__ __forceinline__ uint32_t mul24_byte(uint32_t packed, uint32_t b)       // packed.byte[B] * b
{
    uint32_t d;
    if constexpr (B == 0) asm("v_mul_u32_u24_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_0 src1_sel:DWORD" : "=v"(d) : "v"(packed), "v"(b));
    if constexpr (B == 1) asm("v_mul_u32_u24_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_1 src1_sel:DWORD" : "=v"(d) : "v"(packed), "v"(b));
    if constexpr (B == 2) asm("v_mul_u32_u24_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_2 src1_sel:DWORD" : "=v"(d) : "v"(packed), "v"(b));
    if constexpr (B == 3) asm("v_mul_u32_u24_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_3 src1_sel:DWORD" : "=v"(d) : "v"(packed), "v"(b));
    return d;
}
__device__ __forceinline__ uint32_t mul24_hiword(uint32_t a, uint32_t b)                             // (a >> 16) * b
{ uint32_t d; asm("v_mul_u32_u24_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1 src1_sel:DWORD" : "=v"(d) : "v"(a), "v"(b)); return d; }
__device__ __forceinline__ uint32_t add_hiwords(uint32_t a, uint32_t b)                              // (a >> 16) + (b >> 16)
{ uint32_t d; asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1 src1_sel:WORD_1" : "=v"(d) : "v"(a), "v"(b)); return d; }
template <int B> __device__ __forceinline__ void shr_into_byte(uint32_t& packed, uint32_t sh, uint32_t x)   // packed.byte[B] = x >> sh
{
    if constexpr (B == 0) asm("v_lshrrev_b32_sdwa %0, %1, %2 dst_sel:BYTE_0 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD" : "+v"(packed) : "v"(sh), "v"(x));
    if constexpr (B == 1) asm("v_lshrrev_b32_sdwa %0, %1, %2 dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD" : "+v"(packed) : "v"(sh), "v"(x));
    if constexpr (B == 2) asm("v_lshrrev_b32_sdwa %0, %1, %2 dst_sel:BYTE_2 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD" : "+v"(packed) : "v"(sh), "v"(x));
    if constexpr (B == 3) asm("v_lshrrev_b32_sdwa %0, %1, %2 dst_sel:BYTE_3 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD" : "+v"(packed) : "v"(sh), "v"(x));
}
// byte `o` (0..11) of three consecutive little-endian dwords
__device__ __forceinline__ int pick_byte(uint32_t w0, uint32_t w1, uint32_t w2, int o)
{
    const uint32_t a = o < 4 ? w0 : (o < 8 ? w1 : w2);
    return (int)((a >> ((o & 3) * 8)) & 255u);
}

// Whole pyramid in ONE launch: a workgroup owns a horizontal strip of an image and builds, level after
// level, exactly the rows its next level needs (host-computed closure, rows on strip borders are built by
// both neighbours with identical values), so levels are separated by workgroup barriers instead of kernel
// boundaries.  Same arithmetic as orb_resize_kernel.
// One output pixel of the 4-pixel group: horizontal taps with the coefficients pre-shifted by 12 (so that the
// reference's d >> 4 is the high word of the 32-bit sum), vertical taps, (+2) >> 2 written straight into byte K.
template <int K> __device__ __forceinline__ void pyr_px(uint32_t& packed, uint32_t P0, uint32_t P1, uint32_t Q0, uint32_t Q1,
                                                         uint32_t A0, uint32_t A1, uint32_t b0, uint32_t b1, uint32_t two)
{
    const uint32_t d0 = mul24_byte<K>(P0, A0) + mul24_byte<K>(P1, A1);     // (p*a0 + p'*a1) << 12, < 2^32
    const uint32_t d1 = mul24_byte<K>(Q0, A0) + mul24_byte<K>(Q1, A1);
    const uint32_t m0 = mul24_hiword(d0, b0), m1 = mul24_hiword(d1, b1);   // b * (d >> 4)
    shr_into_byte<K>(packed, two, add_hiwords(m0, m1) + 2u);               // ((m0 >> 16) + (m1 >> 16) + 2) >> 2  (<= 255)
}

// A workgroup = one strip x one column tile, PYR_T threads.  (One workgroup of 1 024 threads per strip over the full width was as fast alone, but a
// 16-wavefront workgroup needs 16 free wave slots on ONE CU at once: beside the other part-batch's kernels, whose one-wavefront workgroups keep
// refilling the slots, the pyramid launches were stretched 2.8x.)
//
// Work mapping inside the workgroup, per level (rows [r0, r1) x 4-px column groups [g0, g1) of the tile):
//   * each of the 4 wavefronts takes a quarter of the rows and walks the tile's column groups in chunks of W <= 64 groups (pyr_chunk_width);
//   * a chunk of W groups holds R = 64 / W row runs side by side: lane = (run, group), and a lane builds CONSECUTIVE output rows of its run.
//     Output row y reads source rows ys0[y] and ys1[y]; whenever ys0[y] == ys1[y - 1] (5 rows of 6 at scale 1.2) the horizontal pass of the upper
//     source row is the one the previous output row kept (four 32-bit sums), so only the lower row is loaded, gathered and multiplied: 1.2 horizontal
//     passes and 3.6 dword loads per output row instead of 2 and 6.  The decision is taken from the row indices of the y records (first row of a run,
//     a source step of 2 and anything else that does not line up recompute) and is wave-uniform: with R > 1 all lanes recompute when any lane must;
//   * with R == 1 (every chunk of 48..64 groups: the bulk of KITTI levels 1 and 2, half of level 3) everything indexed by y is wave-uniform: the y records
//     are read through the scalar cache, b0 | b1, the source / destination row bases and the loop control live in SGPRs (PyrUni; checked in the ISA: the
//     trip's records are s_load_dwordx2, the keep-or-recompute decisions s_cmp + s_cbranch, a row's address one VALU add of a scalar row offset);
//   * the records travel one trip ahead of the rows.  PyrUni: the loads of FOUR output rows (12 .. 24 dwords) are issued before the first is consumed;
//     per-lane runs: two rows (their runs are a few rows long, and four more rows' records per lane do not fit into 64 VGPRs).
// Busy lanes per KITTI level (1241 x 376, scale 1.2, 4 x 4 tiles with their overlap rows and groups; lane-trips with a row to build out of all lane-trips of the
// wavefronts' row loops) and horizontal passes per output row (2 without the kept row; 1.2 is the floor at this scale, every run's first row costs one more):
//   level   groups / tile   rows / strip   chunks (W x R)                  busy lanes   passes / row
//     1       69 .. 74        83 .. 85     64x1 + 5x12 | 10x6                98 %         1.26
//     2       57 .. 61        69 .. 70     57x1 | 61x1                       92 %         1.25
//     3       47 .. 50        57 .. 58     32x2 + 15x4 | 50x1                84 %         1.29
//     4       39 .. 41        47 .. 48     32x2 + 7x9 | 9x7                  93 %         1.39
//     5       32 .. 34        39 .. 40     32x2 (+ 1x64 | 2x32)              91 %         1.32
//     6       26 .. 28        32 .. 33     26x2 | 27x2 | 28x2                82 %         1.38
//     7       21 .. 22        26 .. 27     21x3 | 16x4 + 6x10                76 %         1.71
// 64 VGPRs, no scratch, 8 wavefronts per SIMD.
#define PYR_T 256
typedef const uint64_t __attribute__((address_space(4)))* pyr_yrec_ptr;      // constant address space: uniform reads become scalar loads although the kernel stores between them
struct PyrUni { static constexpr bool value = true; };                        // one row run per wavefront: y is wave-uniform
struct PyrLane { static constexpr bool value = false; };                      // several runs per wavefront: y per lane
// width of the next chunk when `rem` column groups are left: all of them when the R = 64 / rem runs that fit fill >= 3/4 of the wavefront, else the
// largest power of two (which divides 64: all lanes busy) with the remainder left to the next chunk
__device__ __forceinline__ int pyr_chunk_width(int rem)
{
    if (rem >= 64) return 64;
    return (64 / rem) * rem * 4 >= 3 * 64 ? rem : 1 << (31 - __clz(rem));
}
__global__ __launch_bounds__(PYR_T, 8) void orb_pyramid_kernel(const CorbOrbParams p)
{
    const int strip = blockIdx.x / p.pyr_ctiles, ctile = blockIdx.x - strip * p.pyr_ctiles, img = p.img_base + blockIdx.y;
    uint8_t* base = p.pyr + (size_t)img * p.arena_per_image;
    const uint32_t two = 2u;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
    for (int level = 1; level < p.nlevels; level++) {
        const CorbLevel& D = p.lv[level];
        const CorbLevel& S = p.lv[level - 1];
        const int2* xrec = p.resize_rec + D.resize_rec_off;          // per x: {sx, a0 | a1 << 16}
        const pyr_yrec_ptr yrec = (pyr_yrec_ptr)(uintptr_t)(xrec + ((D.w + 3) & ~3));   // per y: {ys0 | ys1 << 16, b0 | b1 << 16}
        const uint8_t* src = base + S.plane_off;
        uint8_t* dstp = base + D.plane_off;
        const int r0 = p.pyr_r0[strip][level], r1 = p.pyr_r1[strip][level];
        const int gfirst = p.pyr_g0[ctile][level], gend = p.pyr_g1[ctile][level];         // this tile's 4-px column groups [gfirst, gend)
        const int wq = (r1 - r0 + 3) >> 2, wr0 = r0 + wave * wq, wr1 = min(wr0 + wq, r1); // this wavefront's rows [wr0, wr1)
        for (int gbase = gfirst, W = 0; gbase < gend && wr0 < wr1; gbase += W) {
            W = pyr_chunk_width(gend - gbase);
            const int R = 64 / W, len = (wr1 - wr0 + R - 1) / R;                          // R runs of len rows side by side
            const int run = lane / W, tx = lane - run * W;
            const int y0 = wr0 + run * len, y1 = min(y0 + len, wr1);
            if (run >= R || y0 >= y1) continue;
            const int x4 = (gbase + tx) * 4;
            int sx[4], sx1[4];
            uint32_t A0[4], A1[4];
            int nvalid = 0;
            const int4 xr01 = *reinterpret_cast<const int4*>(xrec + x4), xr23 = *reinterpret_cast<const int4*>(xrec + x4 + 2);   // padded to a multiple of 4
            const int xs[4] = {xr01.x, xr01.z, xr23.x, xr23.z}, xa[4] = {xr01.y, xr01.w, xr23.y, xr23.w};
#pragma unroll
            for (int k = 0; k < 4; k++) {
                sx[k] = xs[k]; sx1[k] = min(sx[k] + 1, S.w - 1);
                A0[k] = (uint32_t)(xa[k] & 0xFFFF) << 12; A1[k] = (uint32_t)(xa[k] >> 16) << 12;     // <= 2^23: 24-bit operands
                nvalid += (x4 + k < D.w) ? 1 : 0;
            }
            // the 8 source bytes of a row live in 12 aligned bytes: 3 coalesced dword loads instead of 8 byte gathers
            const int bx = sx[0] & ~3;
            const bool wide = (sx1[3] - bx) < 12;           // false only for scale factors > 2
            // v_perm selectors gathering the 4 left / 4 right taps of the group out of the 12 bytes: first from {w1,w0}
            // (offsets 0..7, others zero), then patched from w2 (offsets 8..11; the identity for a lane that needs no patch)
            uint32_t s1a = 0, s2a = 0, s1b = 0, s2b = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int oa = sx[k] - bx, ob = sx1[k] - bx;
                s1a |= (uint32_t)(oa < 8 ? oa : 0x0c) << (8 * k); s2a |= (uint32_t)(oa < 8 ? k : oa - 4) << (8 * k);
                s1b |= (uint32_t)(ob < 8 ? ob : 0x0c) << (8 * k); s2b |= (uint32_t)(ob < 8 ? k : ob - 4) << (8 * k);
            }
            if (wide) {
                // horizontal pass of one source row: d[k] = (p * a0 + p' * a1) << 12 of the group's 4 pixels
                auto hpass = [&](const uint32_t (&w)[3], uint32_t (&d)[4]) {
                    const uint32_t P0 = __builtin_amdgcn_perm(w[2], __builtin_amdgcn_perm(w[1], w[0], s1a), s2a), P1 = __builtin_amdgcn_perm(w[2], __builtin_amdgcn_perm(w[1], w[0], s1b), s2b);
                    d[0] = mul24_byte<0>(P0, A0[0]) + mul24_byte<0>(P1, A1[0]); d[1] = mul24_byte<1>(P0, A0[1]) + mul24_byte<1>(P1, A1[1]);
                    d[2] = mul24_byte<2>(P0, A0[2]) + mul24_byte<2>(P1, A1[2]); d[3] = mul24_byte<3>(P0, A0[3]) + mul24_byte<3>(P1, A1[3]);
                };
                auto rows = [&](auto mode) {
                    constexpr bool UNI = decltype(mode)::value;
                    auto uni = [](int v) { if constexpr (UNI) return __builtin_amdgcn_readfirstlane(v); else return v; };
                    auto rec = [&](int yy) { const uint64_t v = yrec[yy]; return make_uint2((uint32_t)v, (uint32_t)(v >> 32)); };
                    // the upper source row of an output row is recomputed unless it is the row whose horizontal pass the previous output row kept
                    auto fresh = [](uint32_t s0, uint32_t kept) -> bool { if constexpr (UNI) return s0 != kept; else return __any(s0 != kept) != 0; };
                    auto load_row = [&](uint32_t s, uint32_t (&w)[3]) {
                        const uint32_t* q;
                        if constexpr (UNI) q = reinterpret_cast<const uint32_t*>(src + s * (uint32_t)S.pitch + (uint32_t)bx);     // scalar row base + the lane's column offset
                        else q = reinterpret_cast<const uint32_t*>(src + (uint32_t)(__mul24((int)s, S.pitch) + bx));
                        w[0] = q[0]; w[1] = q[1]; w[2] = q[2];
                    };
                    uint32_t dk[4] = {0u, 0u, 0u, 0u};                   // horizontal pass of source row `kept`
                    uint32_t kept = 0xFFFFu;                               // no level has that many rows: the first row of a run recomputes
                    // vertical pass and store of output row yy; the lower row's horizontal pass becomes the kept one
                    auto emit = [&](int yy, bool fr, const uint32_t (&t)[3], const uint32_t (&b)[3], uint32_t bb) {
                        const uint32_t b0 = bb & 0xFFFFu, b1 = bb >> 16;
                        uint32_t dt[4];
                        if (fr) hpass(t, dt);
                        else { dt[0] = dk[0]; dt[1] = dk[1]; dt[2] = dk[2]; dt[3] = dk[3]; }
                        hpass(b, dk);
                        uint32_t packed = 0;
                        shr_into_byte<0>(packed, two, add_hiwords(mul24_hiword(dt[0], b0), mul24_hiword(dk[0], b1)) + 2u);    // ((b0 * (d0 >> 4) >> 16) + (b1 * (d1 >> 4) >> 16) + 2) >> 2  (<= 255)
                        shr_into_byte<1>(packed, two, add_hiwords(mul24_hiword(dt[1], b0), mul24_hiword(dk[1], b1)) + 2u);
                        shr_into_byte<2>(packed, two, add_hiwords(mul24_hiword(dt[2], b0), mul24_hiword(dk[2], b1)) + 2u);
                        shr_into_byte<3>(packed, two, add_hiwords(mul24_hiword(dt[3], b0), mul24_hiword(dk[3], b1)) + 2u);
                        uint8_t* dst;
                        if constexpr (UNI) dst = dstp + (uint32_t)yy * (uint32_t)D.pitch + (uint32_t)x4;
                        else dst = dstp + (uint32_t)(__mul24(yy, D.pitch) + x4);
                        if (nvalid == 4) *reinterpret_cast<uint32_t*>(dst) = packed;
                        else for (int k = 0; k < nvalid; k++) dst[k] = (uint8_t)(packed >> (8 * k));
                    };
                    int y = uni(y0);
                    const int yend = uni(y1), ylast = r1 - 1;
                    // the rows' records travel one trip ahead of the rows: the row loads depend on addresses from the records
                    uint2 ra = rec(min(y, ylast)), rb = rec(min(y + 1, ylast));
                    if constexpr (UNI) {
                        // FOUR output rows per trip: their 12 .. 24 dword loads are issued before the first is consumed (the kernel waits on its loads)
                        uint2 rc = rec(min(y + 2, ylast)), rd = rec(min(y + 3, ylast));
#pragma unroll 1
                        for (; y + 3 < yend; y += 4) {
                            uint32_t ta[3], tb[3], tc[3], td[3], ba[3], bb[3], bc[3], bd[3];
                            const bool fa = fresh(ra.x & 0xFFFFu, kept), fb = fresh(rb.x & 0xFFFFu, ra.x >> 16), fc = fresh(rc.x & 0xFFFFu, rb.x >> 16), fd = fresh(rd.x & 0xFFFFu, rc.x >> 16);
                            if (fa) load_row(ra.x & 0xFFFFu, ta);
                            load_row(ra.x >> 16, ba);
                            if (fb) load_row(rb.x & 0xFFFFu, tb);
                            load_row(rb.x >> 16, bb);
                            if (fc) load_row(rc.x & 0xFFFFu, tc);
                            load_row(rc.x >> 16, bc);
                            if (fd) load_row(rd.x & 0xFFFFu, td);
                            load_row(rd.x >> 16, bd);
                            const uint2 na = rec(min(y + 4, ylast)), nb = rec(min(y + 5, ylast)), nc = rec(min(y + 6, ylast)), nd = rec(min(y + 7, ylast));
                            emit(y, fa, ta, ba, ra.y); emit(y + 1, fb, tb, bb, rb.y); emit(y + 2, fc, tc, bc, rc.y); emit(y + 3, fd, td, bd, rd.y);
                            kept = rd.x >> 16;
                            ra = na; rb = nb; rc = nc; rd = nd;
                        }
                    }
                    // two rows per trip: the rest of a wave-uniform run, and all of the per-lane runs (at most a quarter of the tile's rows / R long: short, and the
                    // records of four more rows per lane do not fit into 64 VGPRs beside 24 row dwords)
#pragma unroll 1
                    for (; y + 1 < yend; y += 2) {
                        uint32_t ta[3], tb[3], ba[3], bb[3];
                        const bool fa = fresh(ra.x & 0xFFFFu, kept), fb = fresh(rb.x & 0xFFFFu, ra.x >> 16);
                        if (fa) load_row(ra.x & 0xFFFFu, ta);
                        load_row(ra.x >> 16, ba);
                        if (fb) load_row(rb.x & 0xFFFFu, tb);
                        load_row(rb.x >> 16, bb);
                        const uint2 na = rec(min(y + 2, ylast)), nb = rec(min(y + 3, ylast));
                        emit(y, fa, ta, ba, ra.y); emit(y + 1, fb, tb, bb, rb.y);
                        kept = rb.x >> 16;
                        ra = na; rb = nb;
                    }
                    if (y < yend) {
                        uint32_t ta[3], ba[3];
                        const bool fa = fresh(ra.x & 0xFFFFu, kept);
                        if (fa) load_row(ra.x & 0xFFFFu, ta);
                        load_row(ra.x >> 16, ba);
                        emit(y, fa, ta, ba, ra.y);
                    }
                };
                if (R == 1) rows(PyrUni{}); else rows(PyrLane{});
            } else {
#pragma unroll 1
                for (int y = y0; y < y1; y++) {
                    const uint64_t yv = yrec[y];
                    const int2 yr = make_int2((int)(uint32_t)yv, (int)(uint32_t)(yv >> 32));
                    const uint8_t* S0 = src + (uint32_t)__mul24(yr.x & 0xFFFF, S.pitch);
                    const uint8_t* S1 = src + (uint32_t)__mul24(yr.x >> 16, S.pitch);
                    const uint32_t b0 = yr.y & 0xFFFF, b1 = (uint32_t)yr.y >> 16;
                    uint32_t packed = 0;
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const uint32_t d0 = mad24u(S0[sx[k]], A0[k] >> 12, mul24u(S0[sx1[k]], A1[k] >> 12));
                        const uint32_t d1 = mad24u(S1[sx[k]], A0[k] >> 12, mul24u(S1[sx1[k]], A1[k] >> 12));
                        const uint32_t v = (((mul24u(b0, d0 >> 4) >> 16) + (mul24u(b1, d1 >> 4) >> 16) + 2u) >> 2) & 0xFFu;
                        packed |= v << (8 * k);
                    }
                    uint8_t* dst = dstp + (uint32_t)(__mul24(y, D.pitch) + x4);
                    if (nvalid == 4) *reinterpret_cast<uint32_t*>(dst) = packed;
                    else for (int k = 0; k < nvalid; k++) dst[k] = (uint8_t)(packed >> (8 * k));
                }
            }
        }
        __threadfence_block();
        __syncthreads();                                  // level `level` rows of this strip are complete and visible
    }
}

// ------------------------------------------------------------------------------------------------
// Per-cell FAST-9/16 with non-max suppression and the iniThFAST -> minThFAST fallback.
// One workgroup per detection cell; the cell sub-image (interior + 3-px ring) lives in LDS.
// s(p) = max over the 16 arcs of 9 contiguous circle pixels of min|I(p)-I(q)| (one-sided) minus 1;
// p is a corner at threshold t  <=>  s(p) >= t, and s(p) is cv::FAST's response for every corner,
// so ONE score pass reproduces both cv::FAST calls of the reference (C/src/ORBextractor.cc:809-816):
//   ismax(p) = s(p) > s(q) for the 8 neighbours q inside the cell interior (outside counts as 0)
//   keep(p)  = ismax(p) && s(p) >= 20   if any such p exists in the cell, else ismax(p) && s(p) >= 7

// ---- packed FAST-9/16 ----
// score(p) = max( max_arcs min_arc(ring) - p , p - min_arcs max_arc(ring) ) - 1   (cv::FAST cornerScore: the centre is a
// monotone shift, so the 9-of-16 sliding min/max run on the raw ring bytes).  Two horizontally adjacent pixels are
// processed per 32-bit register: the LDS tile keeps a pixel per 16-bit slot, so a tile dword already holds the two 16-bit
// halves [b,0 | b',0] once its score bytes are masked off (orb_fast_kernel below); they are reduced with gfx950's packed 3-input v_pk_minimum3_f16 / v_pk_maximum3_f16 -- the halves
// 0x0000..0x00ff are non-negative f16 denormals (kernel FP mode keeps f16 denormals), whose order is the integer order.
__device__ __forceinline__ uint32_t pk_min3(uint32_t a, uint32_t b, uint32_t c)
{ uint32_t d; asm("v_pk_minimum3_f16 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c)); return d; }
__device__ __forceinline__ uint32_t pk_max3(uint32_t a, uint32_t b, uint32_t c)
{ uint32_t d; asm("v_pk_maximum3_f16 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c)); return d; }
typedef short corb_short2 __attribute__((ext_vector_type(2)));

// The 9-of-16 sliding chain of one polarity on packed ring values v[i] = [ring_i(A), 0 | ring_i(B), 0]: 16 3-windows, 16 9-windows, the reduction
// over the 16 arcs (40 packed ops).  BRIGHT: max over the arcs of the arc's minimum; otherwise min over the arcs of the arc's maximum.
template <bool BRIGHT> __device__ __forceinline__ uint32_t fast_arc_chain(const uint32_t (&v)[16])
{
    auto in3 = [](uint32_t a, uint32_t b, uint32_t c) { return BRIGHT ? pk_min3(a, b, c) : pk_max3(a, b, c); };
    auto out3 = [](uint32_t a, uint32_t b, uint32_t c) { return BRIGHT ? pk_max3(a, b, c) : pk_min3(a, b, c); };
    uint32_t w3[16], w9[16], r5[5];
#pragma unroll
    for (int i = 0; i < 16; i++) w3[i] = in3(v[i], v[(i + 1) & 15], v[(i + 2) & 15]);
#pragma unroll
    for (int i = 0; i < 16; i++) w9[i] = in3(w3[i], w3[(i + 3) & 15], w3[(i + 6) & 15]);
#pragma unroll
    for (int i = 0; i < 5; i++) r5[i] = out3(w9[3 * i], w9[3 * i + 1], w9[3 * i + 2]);
    return out3(out3(r5[0], r5[1], r5[2]), out3(r5[3], r5[4], w9[15]), r5[0]);
}

// Scores of the two pixels of a pair from its 16 packed ring values v[i] = [ring_i(A),0 | ring_i(B),0] (cv::FAST order) and centres cpk; 0 = below the threshold t.
// cornerScore = max(B - c, c - D) - 1 with B = max_arcs min_arc(ring), D = min_arcs max_arc(ring).  Every arc of 9 holds two adjacent compass
// points, so B <= m and D >= n of fast_compass: a side whose compass test fails at t stays below t and cannot be the score of a pixel that
// scores >= t.  Nearly every listed pixel passes on one side only (both: 0.3 % of the passing pixels on the synthetic frames), and the dark
// side is the bright side of the complemented bytes, c - D(v) = B(255 - v) - (255 - c): ring and centre are XOR-ed with 0x00ff in the halves
// that pass on the dark side only and ONE chain scores both halves.  When a half of any lane passes on both sides the wave also runs the dual
// chain on the same values (wave-uniform branch) and takes the maximum, which is the two-sided score whatever the halves' masks are.
// kb = t + 0x200, kd = 0x200 - t - 1 in both halves: the side tests as plain 32-bit adds whose halves stay in 1 .. 0x3fe (no borrow across).
__device__ __forceinline__ uint32_t fast_pair_score(uint32_t (&v)[16], uint32_t cpk, uint32_t th2, uint32_t kb, uint32_t kd)
{
    const uint32_t e0 = pk_max3(v[0], v[8], v[8]), e1 = pk_max3(v[4], v[12], v[12]), f0 = pk_min3(v[0], v[8], v[8]), f1 = pk_min3(v[4], v[12], v[12]);
    const uint32_t m = pk_min3(e0, e1, e1), n = pk_max3(f0, f1, f1);                // as in fast_compass
    const uint32_t nbright = (cpk + kb) - m;                                       // 0x200 + c + t - m     : bit 9 <=> NOT m - c > t
    const uint32_t dark = ((cpk + kd) - n) & 0x02000200u;                          // 0x200 + c - n - t - 1 : bit 9 <=> c - n > t
    const uint32_t donly = dark & nbright, both = dark ^ donly;
    const uint32_t xm = (donly >> 1) - (donly >> 9);                               // 0x00ff in the dark-only halves
#pragma unroll
    for (int i = 0; i < 16; i++) v[i] ^= xm;
    const corb_short2 c = __builtin_bit_cast(corb_short2, cpk ^ xm) + (short)1;
    corb_short2 s = __builtin_bit_cast(corb_short2, fast_arc_chain<true>(v)) - c;
    if (__any(both != 0u)) s = __builtin_elementwise_max(s, c - (short)2 - __builtin_bit_cast(corb_short2, fast_arc_chain<false>(v)));
    const corb_short2 keep = s >= __builtin_bit_cast(corb_short2, th2);            // -1 / 0 per half
    return __builtin_bit_cast(uint32_t, (corb_short2)(s & keep));                  // [s,0 | s',0]
}

// Compass test of a pixel pair from its packed compass values v0, v4, v8, v12 (circle positions 0, 4, 8, 12) and centres cpk: any arc of 9 contiguous circle pixels holds two
// ADJACENT compass points (circle positions 0, 4, 8, 12), so   corner at t  =>  max over adjacent compass pairs of min(v_i, v_i+1) > c + t
// or c - t > min over the pairs of max(v_i, v_i+1).  With a, b, c', d the four compass values in circle order the max over the four adjacent
// pairs of their minima is min(max(a, c'), max(b, d)) (max[min(a,b), min(a,d)] = min(a, max(b,d)), the same for c', and
// max[min(a,M), min(c',M)] = min(max(a,c'), M)), and the min over the pairs of their maxima is max(min(a, c'), min(b, d)): 6 min/max instead
// of 12.  Returns Q = max(that max-min - c, c - that min-max) per half: "Q > t" is an EXACT necessary condition (never rejects a corner),
// 9 instructions per pixel pair and 3 tile rows instead of 109 and 7.
__device__ __forceinline__ uint32_t fast_compass(uint32_t v0, uint32_t v4, uint32_t v8, uint32_t v12, uint32_t cpk)
{
    const uint32_t m = pk_min3(pk_max3(v0, v8, v8), pk_max3(v4, v12, v12), pk_max3(v4, v12, v12));
    const uint32_t n = pk_max3(pk_min3(v0, v8, v8), pk_min3(v4, v12, v12), pk_min3(v4, v12, v12));
    const corb_short2 c = __builtin_bit_cast(corb_short2, cpk);
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(corb_short2, m) - c, c - __builtin_bit_cast(corb_short2, n)));
}
__device__ __forceinline__ int mbcnt64(unsigned long long m) { return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)); }

// One WAVEFRONT per cell (64-thread workgroups: barriers are free).
// LDS tile (orb_fast_tile.h): one 16-bit slot per pixel, pixel | score << 8, so an aligned dword of a row is a pixel pair [b,s | b',s'] and the
// byte-to-pair conversion is paid once per loaded dword when the tile is written (two v_perm_b32 that also re-align the global dword, one
// ds_write_b64) instead of once per ring value of every window.  The score lives in the slot's high byte -- a separate tile of score bytes
// would take the cell from 4.2 to 5.7 KB of LDS and the compute unit from 32 cells to 28, which costs more than the shuffles save
// (profiles/HISTORY_r10.md) -- and is masked off where pixels are read.  The cell's interior (scored pixels) starts at column 4 = byte 8 of a row, its
// 3-px halo at column 1; a 4-pixel group is one aligned 8-byte word.  Ring and compass values at an even dx are dwords as they stand (one
// v_and_b32 drops the scores; phase 1 skips it while no score has been written), those at an odd dx one v_perm_b32 of two adjacent dwords whose
// zero selectors drop them.  TP = compile-time tile pitch in slots.
//
// The two cv::FAST calls of the reference (C/src/ORBextractor.cc:809-816) are two PASSES of the same three phases, the second one only for a
// cell without a corner at iniThFAST (< 2 % of the cells):
//   1. compass test at the pass' threshold for every pixel (a lane owns a group of 4 pixels = two packed pairs, lanes are an ng x (64/ng)
//      patch sliding down the cell); the pixel PAIRS with a pixel that passes (11 % of the pairs at t = 20 on the synthetic KITTI-size frames) are
//      appended to a list in LDS (two ballots and lane-prefix counts per sweep, no atomics);
//   2. the 9-of-16 arc score only for the listed pairs and only on the side each pixel passed on (fast_pair_score), one pair per lane (the pair's
//      position enters the LDS address only: 23 dword reads, 10 v_perm_b32, 7 v_and_b32); scores >= threshold go to the slots' high bytes (everything else stays
//      0 -- for cv::FAST's NMS a non-corner scores 0);
//   3. strict 8-neighbour NMS on the slots' score bytes (9 v_perm_b32 per pair), over the listed pairs, survivors as per-row bit masks, compacted in row-major order.
// Scoring every pixel at minThFAST (round 1: one pass, 218 VALU per 4 px, the kernel sat on its VALU issue bound) computed 10x more arc scores
// than the reference's first call needs; a list of 4-pixel groups (first form of round 2) scored 306 pixels per cell in 1.7 trips of the wave,
// the pair list scores 202 in 2.1 half-cost trips.
// inclusive prefix sum over the wavefront in 6 DPP adds (row_shr 1, 2, 4, 8 inside the rows of 16, then row_bcast 15 / 31 across them) -- a
// shuffle-based scan costs an LDS permute and ~6 VALU per step
__device__ __forceinline__ int wave_incl_scan(int v)
{
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, true);
    return v;
}
// (occupancy capped at 4 / 6 wavefronts per SIMD by amdgpu_waves_per_eu, 512-frame steps: 104.0 k -> 88.8 k / 99.1 k stereo fps, profiles/r04_variants_wpe.txt)
template <int TP>
__global__ __launch_bounds__(64) void orb_fast_kernel(const CorbOrbParams p)
{
    constexpr int P = TP / 4;                           // pitch of the 16-bit tile in 8-byte words
    constexpr int PD = TP / 2;                          // pitch of the 16-bit tile in dwords (fast_tile_row_dwords)
    extern __shared__ __attribute__((aligned(16))) uint8_t fast_smem[];
    __shared__ uint16_t plist[FAST_LIST_CAP];           // pixel pairs with a pixel that passed the compass test: (y << 6) | (g << 1) | pair   (y = tile row)
    uint32_t* tile = reinterpret_cast<uint32_t*>(fast_smem);
    // per interior row: NMS survivors of the current pass (fast_th - 6 rows).  The kernel's LDS decides how many cells a CU holds (the launch
    // requests fast_dynamic_lds_bytes; figures per pitch in profiles/HISTORY_r10.md): the 7 KB of a 1 024-entry list and 64 mask rows admitted
    // 22 cells where 5.5 KB admitted 28, FAST alone 520 -> 480 us per 256 images
    uint32_t (*rowm)[2] = reinterpret_cast<uint32_t (*)[2]>(tile + PD * p.fast_th);
    const int nrowm = p.fast_th - 6;
    uint8_t* tb = reinterpret_cast<uint8_t*>(tile);   // a slot's high byte is the pixel's score (0 = not a corner at the pass' threshold)
    int cell, img; corb_xcd_remap(cell, img); img += p.img_base;
    const int lane = threadIdx.x;
    // the cell's geometry depends on the handle alone: one record per cell, built at create (CorbFastCell), read through the scalar cache
    uint4 rec = reinterpret_cast<const uint4*>(p.fast_cells)[cell];
    asm volatile("" : "+s"(rec.x));                    // keeps the record ONE scalar load: otherwise src_off is sunk to its use as a vector load of its own
    int* out_count = p.cell_count + (size_t)img * p.cells_per_image + cell;
    if (rec.y >> 31) { if (lane == 0) *out_count = 0; return; }           // cw < 7 || ch < 7: subsumes the skips at :796, :805
    const CorbLevel& L = p.lv[(rec.y >> 24) & 15u];
    const int c = cell - L.cell_base;
    const int ox = (int)(rec.y & 0xFFFu), oy = (int)((rec.y >> 12) & 0xFFFu);     // first interior pixel, coordinates - CORB_MIN_BORDER
    const int cw = (int)(rec.z & 0xFFu), ch = (int)((rec.z >> 8) & 0xFFu);
    const int iw = cw - 6, ih = ch - 6;                  // interior; iw, ih <= 64 (checked at create)
    {
        // tile column k <-> image x = iniX - 1 + k  (column 0 is padding)
        const uint32_t a = (uint32_t)ox & 3u;           // (iniX - 1) & 3: iniX - 1 = ox + 12
        const uint8_t* src = p.pyr + (size_t)img * p.arena_per_image + rec.x;      // aligned dword holding tile column 0 of the cell's first row
        const int jlast = (int)(rec.w >> 20);            // aligned dword holding the last cell pixel
        const int r0 = lane / P, wc = lane - r0 * P;
        constexpr int RPI = 64 / P;
        // bytes a .. a+3 of the two loaded dwords, spread to four slots: columns 4 wc, 4 wc + 1 | 4 wc + 2, 4 wc + 3 (wave-uniform selectors).
        // Every lane wc < P of every row y < ch stores: all TP slots of the rows 0 .. ch-1 are byte-valued (the padding rule of orb_fast_tile.h)
        const uint32_t sel_lo = 0x0c000c00u | a | ((a + 1u) << 16), sel_hi = sel_lo + 0x00020002u;
        if (r0 < RPI) {
            const int j0 = min(wc, jlast), j1 = min(wc + 1, jlast);
            for (int y = r0; y < ch; y += 4 * RPI) {        // four row groups per trip: eight loads in flight, then the stores
                uint32_t w0[4], w1[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const uint32_t* g = reinterpret_cast<const uint32_t*>(src + (uint32_t)__mul24(min(y + k * RPI, ch - 1), L.pitch));
                    w0[k] = g[j0]; w1[k] = g[j1];
                }
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (y + k * RPI < ch) {
                        const int yy = y + k * RPI;
                        reinterpret_cast<uint2*>(tile)[yy * P + wc] = make_uint2(__builtin_amdgcn_perm(w1[k], w0[k], sel_lo), __builtin_amdgcn_perm(w1[k], w0[k], sel_hi));
                    }
            }
        }
    }
    __syncthreads();
    const int rstep = (int)((rec.z >> 16) & 0xFFu), ng = (int)(rec.z >> 24);      // 4-pixel groups per interior row (<= 16), 64 / ng
    const int r = (int)(((uint32_t)lane * (rec.w & 0xFFFFFu)) >> 16), g = lane - r * ng;      // lane / ng for lane < 64, ng <= 16 (exact 16.16 reciprocal)
    const bool active = r < rstep;
    const int nvalid = min(4, iw - 4 * g);               // pixels of this group inside the interior
    const uint32_t smask0 = nvalid >= 2 ? 0x80008000u : nvalid == 1 ? 0x00008000u : 0u, smask1 = nvalid >= 4 ? 0x80008000u : nvalid == 3 ? 0x00008000u : 0u;
    unsigned long long mine = 0;
    auto odd = [](uint32_t hi, uint32_t lo) { return __builtin_amdgcn_perm(hi, lo, 0x0c040c02u); };   // [pixel of lo's high slot | pixel of hi's low slot], score bytes dropped
    bool dirty = false;                                  // scores may stand in the slots' high bytes
    for (int pass = 0; pass < 2; pass++) {
        const int th = pass == 0 ? p.ini_th : p.min_th;
        const uint32_t th2 = (uint32_t)th * 0x00010001u;
        const uint32_t kb = th2 + 0x02000200u, kd = 0x02000200u - th2 - 0x00010001u;      // side tests of phase 2 (fast_pair_score)
        if (lane < nrowm) { rowm[lane][0] = 0u; rowm[lane][1] = 0u; }
        int y0 = 3, nbatch = 0, base = 0, nscore = 0;
        while (y0 < ch - 3) {
            nbatch++;
            // ---- phase 1: compass test; the pixel PAIRS with a survivor are appended to plist (room for a whole sweep of the patch: 128) ----
            base = 0;
            for (; y0 < ch - 3 && base + FAST_LIST_SWEEP <= FAST_LIST_CAP; y0 += rstep) {
                const int y = y0 + r;
                uint32_t d0 = 0u, d1 = 0u;                       // idle lanes keep 0: the ballots below compare d0, d1 themselves (no 0/1 flag carried out of the branch)
                if (active && y < ch - 3) {
                    const uint2* t = reinterpret_cast<const uint2*>(tile + y * PD) + g;      // 8-byte word left of the group: columns 4g .. 4g+3
                    uint2 up = t[-3 * P + 1], dn = t[3 * P + 1];                              // the group's own columns 4g+4 .. 4g+7, rows y - 3 / y + 3
                    const uint2 wl = t[0], wr = t[2]; uint2 wc = t[1];                      // row y: columns 4g .. 4g+11
                    if (dirty) { up.x &= 0x00ff00ffu; up.y &= 0x00ff00ffu; dn.x &= 0x00ff00ffu; dn.y &= 0x00ff00ffu; }
                    const uint2 wcm = make_uint2(wc.x & 0x00ff00ffu, wc.y & 0x00ff00ffu);
                    // pair 0 (columns 4g+4, 4g+5): dx = -3 is columns 4g+1, 4g+2, dx = +3 columns 4g+7, 4g+8; pair 1 the same two columns further
                    const uint32_t q0 = fast_compass(dn.x, odd(wr.x, wc.y), up.x, odd(wl.y, wl.x), dirty ? wcm.x : wc.x);
                    const uint32_t q1 = fast_compass(dn.y, odd(wr.y, wr.x), up.y, odd(wc.x, wl.y), dirty ? wcm.y : wc.y);
                    // Q > th  <=>  (th - Q) < 0 per half: the sign bits of the four pixels, those past the interior masked off
                    d0 = __builtin_bit_cast(uint32_t, (corb_short2)(__builtin_bit_cast(corb_short2, th2) - __builtin_bit_cast(corb_short2, q0))) & smask0;
                    d1 = __builtin_bit_cast(uint32_t, (corb_short2)(__builtin_bit_cast(corb_short2, th2) - __builtin_bit_cast(corb_short2, q1))) & smask1;
                }
                asm("" : "+v"(d0), "+v"(d1));                   // keeps the two compares below the join: sunk into the branch they come back as v_cndmask 0/1 + v_cmp_ne each
                const bool hit0 = d0 != 0u, hit1 = d1 != 0u;
                const unsigned long long b0 = __ballot(hit0), b1 = __ballot(hit1);
                const int n0 = __popcll(b0);
                const uint32_t ent = (uint32_t)((y << 6) | (g << 1));
                if (hit0) plist[base + mbcnt64(b0)] = (uint16_t)ent;
                if (hit1) plist[base + n0 + mbcnt64(b1)] = (uint16_t)(ent | 1u);
                base += n0 + __popcll(b1);
            }
            __syncthreads();
            // ---- phase 2: arc scores of the listed pairs, one per lane (the window of pair 1 is the window of pair 0 two bytes further) ----
            // The pairs that score are compacted in place (the writes never pass the reads): phase 3 sweeps those only.
            nscore = 0;
            for (int i0 = 0; i0 < base; i0 += 64) {
                const int i = i0 + lane;
                bool has = false;
                uint32_t e = 0;
                if (i < base) {
                e = plist[i];
                const int y = e >> 6, ge = (e >> 1) & 31;
                const uint32_t sh = (e & 1u) * 2u;
                // the pair's own dword (fast_tile_pair_dword(ge, e & 1) = 2 + the entry's low 6 bits): which pair of the group it is enters the address only
                const uint32_t* t = tile + y * PD + 2 + (e & 63u);
                constexpr uint32_t PX = 0x00ff00ffu;
                uint32_t v[16];
                {
                    const uint32_t* u = t + 3 * PD;               // row y + 3: dx = 0, 1 and -1
                    const uint32_t a = u[-1], b = u[0], c = u[1];
                    v[0] = b & PX; v[1] = odd(c, b); v[15] = odd(b, a);
                }
                { const uint32_t* u = t + 2 * PD; v[14] = u[-1] & PX; v[2] = u[1] & PX; }                              // row y + 2: dx = -2, 2
                { const uint32_t* u = t + PD; v[13] = odd(u[-1], u[-2]); v[3] = odd(u[2], u[1]); }           // row y + 1: dx = -3, 3
                const uint32_t cpk = t[0] & PX;
                v[12] = odd(t[-1], t[-2]); v[4] = odd(t[2], t[1]);                                           // row y
                { const uint32_t* u = t - PD; v[11] = odd(u[-1], u[-2]); v[5] = odd(u[2], u[1]); }           // row y - 1
                { const uint32_t* u = t - 2 * PD; v[10] = u[-1] & PX; v[6] = u[1] & PX; }                              // row y - 2
                {
                    const uint32_t* u = t - 3 * PD;               // row y - 3: dx = 1, 0, -1
                    const uint32_t a = u[-1], b = u[0], c = u[1];
                    v[7] = odd(c, b); v[8] = b & PX; v[9] = odd(b, a);
                }
                const uint32_t s0 = fast_pair_score(v, cpk, th2, kb, kd);                  // [s,0 | s',0]
                const int px = 4 * ge + (int)sh;                                  // interior column of the pair's first pixel (< iw: it passed the mask)
                const uint32_t s2 = px + 1 >= iw ? s0 & 0xFFu : s0;
                uint8_t* sb = tb + 4 * (t - tile);
                sb[1] = (uint8_t)s2; sb[3] = (uint8_t)(s2 >> 16);
                has = s2 != 0u;
                }
                const unsigned long long bs = __ballot(has);
                if (has) plist[nscore + mbcnt64(bs)] = (uint16_t)e;
                nscore += __popcll(bs);
            }
            dirty = true;
            __syncthreads();
        }
        // ---- phase 3: strict 8-neighbour NMS (non-corners score 0).  Only listed groups can hold a corner: when the whole cell went through one
        // list (the usual case) the sweep runs over the list instead of over every group of the cell ----
        // scores of the pair at dword q of row y against their 8 neighbours: bit 0 / 1 = the first / second pixel is a strict maximum
        auto nms_pair = [&](const uint32_t* t) -> uint32_t {
            auto mid = [](uint32_t d) { return __builtin_amdgcn_perm(0u, d, 0x0c030c01u); };                    // [s, 0 | s', 0] of a dword's two slots
            auto lft = [](uint32_t d, uint32_t dm) { return __builtin_amdgcn_perm(d, dm, 0x0c050c03u); };       // the pair one column left of d (dm = the dword before d)
            const uint32_t a0 = t[-PD - 1], a1 = t[-PD], a2 = t[-PD + 1], b0 = t[-1], b1 = t[0], b2 = t[1], c0 = t[PD - 1], c1 = t[PD], c2 = t[PD + 1];
            const uint32_t ctr = mid(b1);
            const uint32_t nb = pk_max3(pk_max3(lft(a1, a0), mid(a1), lft(a2, a1)), pk_max3(lft(c1, c0), mid(c1), lft(c2, c1)), pk_max3(lft(b1, b0), lft(b2, b1), lft(b2, b1)));
            // strict 8-neighbour maximum: ctr > nb  <=>  (nb - ctr) < 0 per half
            const uint32_t dm = __builtin_bit_cast(uint32_t, (corb_short2)(__builtin_bit_cast(corb_short2, nb) - __builtin_bit_cast(corb_short2, ctr)));
            return ((dm >> 15) & 1u) | ((dm >> 30) & 2u);
        };
        if (nbatch == 1) {
            for (int i = lane; i < nscore; i += 64) {
                const uint32_t e = plist[i];                       // only the pairs that scored are listed
                const int y = e >> 6, ge = (e >> 1) & 31;
                const uint32_t sh = (e & 1u) * 2u;
                const uint32_t bits = nms_pair(tile + y * PD + 2 + (e & 63u));
                if (bits) atomicOr(&rowm[y - 3][ge >> 3], bits << (4 * (ge & 7) + sh));
            }
        } else if (active) {
            for (int y = 3 + r; y < ch - 3; y += rstep) {
                const uint32_t* t = tile + y * PD + 2 * g + 2;
                uint32_t bits = 0;
                if (t[0] & 0xff00ff00u) bits = nms_pair(t);
                if (t[1] & 0xff00ff00u) bits |= nms_pair(t + 1) << 2;
                if (bits) atomicOr(&rowm[y - 3][g >> 3], bits << (4 * (g & 7)));
            }
        }
        __syncthreads();
        mine = lane < ih ? ((unsigned long long)rowm[lane][1] << 32) | rowm[lane][0] : 0ull;
        if (__any(mine != 0ull)) break;                   // the cell has a corner at this threshold: the second cv::FAST call does not happen
        __syncthreads();                                  // (rowm is cleared at the top of the next pass)
    }
    unsigned long long mask = mine;
    const int cnt = __popcll(mask);
    const int incl = wave_incl_scan(cnt);
    const int total = __builtin_amdgcn_readlane(incl, 63);
    uint32_t* out = p.cand + (size_t)img * p.cand_per_image + L.cand_base + (size_t)c * L.cell_cap;
    int off = incl - cnt;
    while (mask) {                                         // row-major inside the cell: lane = row, bits = columns
        const int x = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        if (off < L.cell_cap)
            out[off] = (uint32_t)(ox + x) | ((uint32_t)(oy + lane) << 12) |
                       ((uint32_t)tb[2 * ((lane + 3) * TP + x + 4) + 1] << 24);
        off++;
    }
    if (lane == 0) { *out_count = min(total, L.cell_cap); if (total > L.cell_cap) p.status[img] = CORB_ERR_OVERFLOW; }
}

// ------------------------------------------------------------------------------------------------
// cv::GaussianBlur(7x7, sigma 2, BORDER_REFLECT_101) on 8U, OpenCV 2.4.8 scalar path:
// 8-bit fixed-point taps {18,34,49,55,49,34,18} per axis, row pass exact int, column (sum+2^15)>>16.
// Register rolling window, no LDS: a thread owns a 4-px-wide column strip of BL_ROWS output rows.  Per input row it loads
// three aligned 32-bit words (columns x-4 .. x+7, neighbours overlap in L1).  Both passes are dot-product instructions:
//   horizontal: the 7 taps of pixel k are bytes 1+k .. 7+k of those 12 bytes -- instead of re-aligning the data, the WEIGHTS
//               are shifted: 10 v_dot4_u32_u8 with constant weight words give the 4 row sums (<= 257*255 = 65535: 16 bits);
//   vertical  : the row sums of two consecutive input rows are kept as one (lo, hi) 16-bit pair; an output row is
//               4 v_dot2_u32_u16 over the 4 live pairs (even / odd output rows use two weight sets), accumulator preloaded
//               with the rounding bias.  (sum + 2^15) >> 16 saturates through v_sat_pk_u8_i16.
// 33 VALU per 4 px of one row instead of the 141 of the shift/mask/mad24 form (SQ_INSTS_VALU, profiles/).
#define BL_ROWS 32
#define BL_CHUNK 8
__device__ __forceinline__ int reflect101(int v, int n) { if (v < 0) v = -v; if (v >= n) v = 2 * n - 2 - v; return min(max(v, 0), n - 1); }
#define BLW4(b0, b1, b2, b3) ((uint32_t)(b0) | ((uint32_t)(b1) << 8) | ((uint32_t)(b2) << 16) | ((uint32_t)(b3) << 24))
#define BLW2(lo, hi) ((uint32_t)(lo) | ((uint32_t)(hi) << 16))
typedef unsigned short bl_us2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t bl_dot2(uint32_t a, uint32_t w, uint32_t c)
{ return __builtin_amdgcn_udot2(__builtin_bit_cast(bl_us2, a), __builtin_bit_cast(bl_us2, w), c, false); }
__device__ __forceinline__ uint32_t bl_sat_pk(uint32_t a) { uint32_t d; asm("v_sat_pk_u8_i16 %0, %1" : "=v"(d) : "v"(a)); return d; }

// INTERIOR: every live lane of the wave has its 12 bytes inside the row (no column reflection, full 4-px stores)
template <bool INTERIOR>
__device__ __forceinline__ void blur_strip(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int x, int y0, int y1, int h, int pitch, int wimg)
{
    const int xl = max(x - 4, 0);
    // a chunk = BL_CHUNK input rows fetched back to back: 24 loads in flight per lane.  Rows are reflected (BORDER_REFLECT_101) only in the
    // chunks that touch the first / last rows of the level (wave-uniform test); everywhere else a row address is one add
    auto load_chunk = [&](uint32_t (&W)[BL_CHUNK][3], int first_row) {
        if (__all(first_row >= 0 && first_row + BL_CHUNK <= h)) {
            const uint32_t o0 = (uint32_t)__mul24(first_row, pitch) + (uint32_t)xl;
#pragma unroll
            for (int i = 0; i < BL_CHUNK; i++) {
                const uint32_t* row = reinterpret_cast<const uint32_t*>(src + (o0 + (uint32_t)(i * pitch)));     // i * pitch: scalar
                W[i][0] = row[0]; W[i][1] = row[1]; W[i][2] = row[2];
            }
            return;
        }
#pragma unroll
        for (int i = 0; i < BL_CHUNK; i++) {
            const uint32_t off = (uint32_t)__mul24(reflect101(first_row + i, h), pitch) + (uint32_t)xl;   // 32-bit offset from the uniform plane base
            const uint32_t* row = reinterpret_cast<const uint32_t*>(src + off);
            W[i][0] = row[0]; W[i][1] = row[1]; W[i][2] = row[2];
        }
    };
    // image-border wave: the 12 bytes "columns x-4 .. x+7 after BORDER_REFLECT_101" are byte gathers of the 12 loaded bytes with
    // per-lane v_perm selectors (computed once per strip): word j = perm(w1:w0, selA[j]) | perm(w2, selB[j]), 0x0c = zero byte
    uint32_t selA[3] = {0, 0, 0}, selB[3] = {0, 0, 0};
    if (!INTERIOR) {
#pragma unroll
        for (int k = 0; k < 12; k++) {
            const uint32_t q = (uint32_t)min(max(reflect101(x - 4 + k, wimg) - xl, 0), 11);
            selA[k >> 2] |= (q < 8 ? q : 0x0cu) << ((k & 3) * 8);
            selB[k >> 2] |= (q < 8 ? 0x0cu : q - 8) << ((k & 3) * 8);
        }
    }
    auto hsum = [&](const uint32_t (&w)[3], uint32_t (&o)[4]) {            // horizontal taps of one input row, 4 columns
        uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
        if (!INTERIOR) {
            const uint32_t v0 = __builtin_amdgcn_perm(w[1], w[0], selA[0]) | __builtin_amdgcn_perm(0u, w[2], selB[0]);
            const uint32_t v1 = __builtin_amdgcn_perm(w[1], w[0], selA[1]) | __builtin_amdgcn_perm(0u, w[2], selB[1]);
            const uint32_t v2 = __builtin_amdgcn_perm(w[1], w[0], selA[2]) | __builtin_amdgcn_perm(0u, w[2], selB[2]);
            w0 = v0; w1 = v1; w2 = v2;
        }
        o[0] = __builtin_amdgcn_udot4(w1, BLW4(55, 49, 34, 18), __builtin_amdgcn_udot4(w0, BLW4(0, 18, 34, 49), 0u, false), false);
        o[1] = __builtin_amdgcn_udot4(w2, BLW4(18, 0, 0, 0), __builtin_amdgcn_udot4(w1, BLW4(49, 55, 49, 34), __builtin_amdgcn_udot4(w0, BLW4(0, 0, 18, 34), 0u, false), false), false);
        o[2] = __builtin_amdgcn_udot4(w2, BLW4(34, 18, 0, 0), __builtin_amdgcn_udot4(w1, BLW4(34, 49, 55, 49), __builtin_amdgcn_udot4(w0, BLW4(0, 0, 0, 18), 0u, false), false), false);
        o[3] = __builtin_amdgcn_udot4(w2, BLW4(49, 34, 18, 0), __builtin_amdgcn_udot4(w1, BLW4(18, 34, 49, 55), 0u, false), false);
    };
    auto hpair = [&](const uint32_t (&wa)[3], const uint32_t (&wb)[3], uint32_t (&q)[4]) {      // rows r, r+1 -> (lo, hi) pairs
        uint32_t a[4], b[4];
        hsum(wa, a); hsum(wb, b);
#pragma unroll
        for (int k = 0; k < 4; k++) q[k] = a[k] | (b[k] << 16);
    };
    const uint32_t bias = 1u << 15;
    auto emit = [&](const uint32_t (&acc)[4], int oy) {
        if (oy >= y1) return;
        // acc < 2^25: (acc >> 16) of two pixels as two i16, saturated to u8
        const uint32_t s01 = bl_sat_pk(__builtin_amdgcn_perm(acc[1], acc[0], 0x07060302u));
        const uint32_t s23 = bl_sat_pk(__builtin_amdgcn_perm(acc[3], acc[2], 0x07060302u));
        const uint32_t packed = __builtin_amdgcn_perm(s23, s01, 0x05040100u);
        uint8_t* d = dst + ((uint32_t)__mul24(oy, pitch) + (uint32_t)x);
        if (INTERIOR || x + 4 <= wimg) *reinterpret_cast<uint32_t*>(d) = packed;
        else {
            if (x < wimg) d[0] = (uint8_t)packed;
            if (x + 1 < wimg) d[1] = (uint8_t)(packed >> 8);
            if (x + 2 < wimg) d[2] = (uint8_t)(packed >> 16);
        }
    };
    // input row i (relative to y0 - 3); pair m = rows 2m, 2m+1; output rows 2s, 2s+1 read pairs s .. s+3
    uint32_t Q[4][4];
    uint32_t A[BL_CHUNK][3];
    load_chunk(A, y0 - 3);                                                 // rows 0 .. 7 : pairs 0 .. 3
    hpair(A[0], A[1], Q[0]); hpair(A[2], A[3], Q[1]); hpair(A[4], A[5], Q[2]);
    uint32_t carry[2][3] = {{A[6][0], A[6][1], A[6][2]}, {A[7][0], A[7][1], A[7][2]}};
    load_chunk(A, y0 + 5);                                                 // rows 8 .. 15
    auto step = [&](const uint32_t (&ra)[3], const uint32_t (&rb)[3], int s, int oy) {     // s = pair phase (static after unrolling)
        hpair(ra, rb, Q[(s + 3) & 3]);
        uint32_t e[4], o[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            e[k] = bl_dot2(Q[(s + 3) & 3][k], BLW2(18, 0), bl_dot2(Q[(s + 2) & 3][k], BLW2(49, 34), bl_dot2(Q[(s + 1) & 3][k], BLW2(49, 55), bl_dot2(Q[s & 3][k], BLW2(18, 34), bias))));
            o[k] = bl_dot2(Q[(s + 3) & 3][k], BLW2(34, 18), bl_dot2(Q[(s + 2) & 3][k], BLW2(55, 49), bl_dot2(Q[(s + 1) & 3][k], BLW2(34, 49), bl_dot2(Q[s & 3][k], BLW2(0, 18), bias))));
        }
        emit(e, oy); emit(o, oy + 1);
    };
    // 8 output rows per chunk: steps s = 0..3 consume rows (carry0, carry1), W[0..1], W[2..3], W[4..5]; W[6..7] carry over
    auto run8 = [&](const uint32_t (&W)[BL_CHUNK][3], int base) {
        step(carry[0], carry[1], 0, base);
        step(W[0], W[1], 1, base + 2);
        step(W[2], W[3], 2, base + 4);
        step(W[4], W[5], 3, base + 6);
#pragma unroll
        for (int c = 0; c < 3; c++) { carry[0][c] = W[6][c]; carry[1][c] = W[7][c]; }
    };
    // single buffer: the next chunk is requested right after the current one is consumed; a second buffer costs occupancy and
    // was measured slower (115 vs 104 us per 128 KITTI images)
    for (int base = y0; base < y1; base += BL_CHUNK) {
        run8(A, base);
        if (base + BL_CHUNK < y1) load_chunk(A, base + 13);                // relative rows (base - y0) + 16 .. + 23
    }
}

__global__ __launch_bounds__(CORB_BLUR_T) void orb_blur_kernel(const CorbOrbParams p)
{
    int tile, img; corb_xcd_remap(tile, img); img += p.img_base;
    int level = 0;
    for (int l = 1; l < p.nlevels; l++) if (tile >= p.lv[l].blur_tile_base) level = l;
    const CorbLevel& L = p.lv[level];
    const int t = tile - L.blur_tile_base;
    // work items of a level = (row strip, 4-px column group) in row-major order, CORB_BLUR_T per workgroup: a wave may straddle two strips,
    // so the only idle lanes are in the last wave of a level (blur_tiles_x = column groups, blur_tiles_y = strips)
    const int item = t * CORB_BLUR_T + (int)threadIdx.x;
    const int strip = item / L.blur_tiles_x, xg = item - strip * L.blur_tiles_x;
    const int x = xg * 4, y0 = strip * BL_ROWS;
    const bool live = strip < L.blur_tiles_y;
    const uint8_t* src = p.pyr + (size_t)img * p.arena_per_image + L.plane_off;
    uint8_t* dst = p.blur + (size_t)img * p.arena_per_image + L.plane_off;
    const bool interior = (x >= 4) && (x + 8 <= L.w);                // words x-4 .. x+7 fully inside the row
    const bool wave_interior = __all(interior || !live);
    if (!live) return;
    const int y1 = min(y0 + BL_ROWS, L.h);
    if (wave_interior) blur_strip<true>(src, dst, x, y0, y1, L.h, L.pitch, L.w);
    else blur_strip<false>(src, dst, x, y0, y1, L.h, L.pitch, L.w);
}

// ------------------------------------------------------------------------------------------------
// DistributeOctTree as an array algorithm (validated against the serial oracle by
// tools/octree_proto.py).  The node table is always held in std::list order and rebuilt per pass:
//   phase A pass : new = reverse(flatten_i children(e_i)) ++ [old nodes holding one key]
//   phase B iter : candidates (children of the last pass with >1 keys) processed by
//                  (count desc, list position asc) until size >= N;
//                  new = reverse(flatten_t children(v_t)) ++ [old nodes not processed]
// The reference orders equal-size candidates by heap address (C/src/ORBextractor.cc:684); the
// defined order is node creation order, i.e. list position ascending == created later first.
// OT (template parameter): threads per (image, level).  corb_launch_orb_pipeline can split the launch into two level groups -- the large levels with OT_BIG
// threads, the levels whose node table holds at most OT_SMALL_CAP nodes with OT_SMALL (one wavefront: that instantiation has no workgroup barrier left) -- each
// carving its LDS for its own largest level.  Round 5 measured the split against round 4's account of the kernel (0.93 ms per 512-image launch inside the
// pipeline, 0.21 ms alone: "its four-wavefront, 39 KB workgroups wait for their slot beside the other part-batch's one-wavefront FAST workgroups"):
// 128 + 64 threads in two launches DO shorten the kernel inside the pipeline (2 x 0.26 ms), and the step gets LONGER -- 104.8 k -> 101.9 k stereo fps; 256 + 64,
// 64 + 64, 128 + 128 and one launch of 64 everywhere: 102.0 / 100.9 / 102.1 / 102.5 k (profiles/r05_variants_octree.txt, two alternations on one box, all
// byte-exact).  The kernel was never on the step's critical path (round 3: the step without it is 1.8 % shorter): it runs underneath the other part's
// issue-bound kernels, and more, smaller workgroups take more of the wave slots those kernels live on.  Default: one launch, 256 threads (OT_SMALL_CAP 0).
#ifndef OT_BIG
#define OT_BIG 256
#endif
#ifndef OT_SMALL
#define OT_SMALL 64
#endif
#ifndef OT_SMALL_CAP
#define OT_SMALL_CAP 0       // node_cap up to which a level goes to the OT_SMALL group (260 = KITTI's levels 3-7)
#endif
// A client's per-frame call (corb_stereo_frames, 2 images) launches 16 workgroups on an empty GPU: there the kernel IS the critical path of the call (76 of
// 213 us at B = 1 with 256 threads), and a level's passes shorten with the threads that share its keys.  Launches of up to OT_LAT_MAX_IMAGES images take OT_LAT threads.
#ifndef OT_LAT
#define OT_LAT 512
#endif
#ifndef OT_LAT_MAX_IMAGES
#define OT_LAT_MAX_IMAGES 16
#endif
#ifndef OT_WIDE_LDS
#define OT_WIDE_LDS (48 * 1024)
#endif
#ifndef OT_KREG
#define OT_KREG 16          // keys per thread kept in registers (levels with up to 4096 candidates; larger levels reload their keys in chunks)
#endif
#ifndef OT_KSUB
#define OT_KSUB 4           // slots whose stages are issued together
#endif
#ifndef OT_WAVES
#define OT_WAVES 6          // waves per SIMD the register budget is sized for
#endif
struct OtNode { short x0, x1, y0, y1; };

template <int OT> __device__ __forceinline__ int ot_block_scan_excl(int v, int* wtmp, int& total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int incl = wave_incl_scan(v);
    if (lane == 63) wtmp[wave] = incl;
    __syncthreads();
    int woff = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < OT / 64; w++) { const int t = wtmp[w]; if (w < wave) woff += t; tot += t; }
    __syncthreads();
    total = tot;
    return woff + incl - v;
}

// in-place exclusive scan of an LDS array a[0..n); returns the total (all threads)
template <int OT> __device__ __forceinline__ int ot_array_scan_excl(int* a, int n, int* wtmp)
{
    const int per = (n + OT - 1) / OT;
    const int b = min((int)threadIdx.x * per, n), e = min(b + per, n);
    int s = 0;
    for (int i = b; i < e; i++) s += a[i];
    int total;
    int base = ot_block_scan_excl<OT>(s, wtmp, total);
    for (int i = b; i < e; i++) { const int t = a[i]; a[i] = base; base += t; }
    __syncthreads();
    return total;
}



size_t corb_octree_lds_bytes(int cap, int ncell)
{
    // nodeA,nodeB (8B) cntA,cntB (4B) ccntA,ccntB (16B) expf (4B) cb (4B) pk/best (4B) skey (4B) nidc (8B) newidKeep (4B)
    size_t per_node = 8 * 2 + 4 * 2 + 16 * 2 + 4 + 4 + 4 + 4 + 8 + 4;
    return (size_t)(cap + 4) * per_node + (size_t)(ncell + 1) * 4 + 64 * 4;
}

// A pass costs 5 workgroup barriers (7 in phase B): [per-node flags] -> packed scan (children | keepers) -> [children, quadrant
// counters of the new nodes cleared] -> [key sweep: every key moves to its new node AND is counted into that node's quadrant
// for the next pass].  Phase B ranks its candidates (count desc, list position asc) by counting over one packed sort key per
// node, read four at a time; the same loop accumulates the children created before a candidate, which gives the stop point
// (:730) and the child base without a scan in rank order.
template <int OT> __global__ __launch_bounds__(OT, (OT >= 1024 ? 4 : OT_WAVES)) void orb_octree_kernel(const CorbOrbParams p, const int lvl0, const int cap_grp, const int ncell_grp)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // level-major dispatch order (all level-0 workgroups first): the workgroups of the big levels run 2-3x longer than those of the
    // small ones, so longest-first keeps the tail short when the launch needs more than one round of workgroup slots; consecutive
    // workgroups are consecutive images, which keeps image i on XCD i % 8 like the other kernels
    const unsigned Blin = blockIdx.x + gridDim.x * blockIdx.y;
    const int level = lvl0 + (int)(Blin / gridDim.y);
    const int img = (int)(Blin % gridDim.y) + p.img_base;
    const int tid = threadIdx.x;
    const CorbLevel& L = p.lv[level];
    const int capm = cap_grp + 4;               // the group's largest node table
    OtNode* nodeA = reinterpret_cast<OtNode*>(smem);
    OtNode* nodeB = nodeA + capm;
    int* cntA = reinterpret_cast<int*>(nodeB + capm);
    int* cntB = cntA + capm;
    int* ccntA = cntB + capm;              // [cap][4] keys per quadrant of node i (valid for nodes holding > 1 key)
    int* ccntB = ccntA + 4 * capm;
    int* expf = ccntB + 4 * capm;
    int* cb = expf + capm;                 // child base of an expanded node (position among the new children, processing order)
    int* pk = cb + capm;                   // scan array: children | keepers << 16; later `best`
    int* skey = pk + capm;                 // phase B sort keys
    unsigned short* nidc = reinterpret_cast<unsigned short*>(skey + capm);   // [cap][4] new node id of child c
    int* newidKeep = reinterpret_cast<int*>(nidc + 4 * capm);
    int* celloff = newidKeep + capm;       // [ncell_max+1]
    int* wtmp = celloff + ncell_grp + 1;   // scan scratch
    int* ctl = wtmp + 16;                  // control words, two sets (pass parity): [0] children created, [1] children holding > 1 key
    int* best = pk;

    const int N = L.quota;
    const int ncell = L.nCols * L.nRows;
    const int* cc = p.cell_count + (size_t)img * p.cells_per_image + L.cell_base;
    const uint32_t* cand = p.cand + (size_t)img * p.cand_per_image + L.cand_base;
    uint32_t* keys = p.keys + (size_t)img * p.cand_per_image + L.cand_base;
    uint16_t* key_node = p.key_node + (size_t)img * p.cand_per_image + L.cand_base;
    uint32_t* kp_out = p.kp + (size_t)img * p.kp_per_image + L.kp_base;
    int* kp_count = p.kp_count + (size_t)img * CORB_MAX_LEVELS + level;

    // (a) candidates of this level in reference order: cell-row-major, in-cell scan order (:789-829)
    for (int i = tid; i < ncell; i += OT) celloff[i] = cc[i];
    if (tid == 0) celloff[ncell] = 0;
    if (tid < 8) ctl[tid] = 0;
    __syncthreads();
    const int n = ot_array_scan_excl<OT>(celloff, ncell + 1, wtmp);
    if (n == 0) { if (tid == 0) *kp_count = 0; return; }
    if (n >= (1 << 18)) { if (tid == 0) { p.status[img] = CORB_ERR_OVERFLOW; *kp_count = 0; } return; }    // 18-bit key counts in the phase B sort key
    // (b) initial nodes (:543-570)
    const int nIni = L.nIni;
    const int H = L.maxBY - CORB_MIN_BORDER;
    for (int i = tid; i < nIni; i += OT) {
        OtNode nd; nd.x0 = (short)(int)__fmul_rn(L.hX, (float)i); nd.x1 = (short)(int)__fmul_rn(L.hX, (float)(i + 1));
        nd.y0 = 0; nd.y1 = (short)H;
        nodeA[i] = nd; cntA[i] = 0; expf[i] = 0;
    }
    __syncthreads();
    // Keys are handled in chunks of OT_KREG per thread (key t = (chunk * OT_KREG + j) * OT + tid <-> slot j).  A level with up to
    // OT_KREG * OT keys is one chunk that stays in REGISTERS for all passes; larger levels reload each chunk from the global
    // keys / key_node arrays (uniform branch).  Inside a chunk every stage is issued for all slots before the next stage starts,
    // so the dependent LDS / global latencies of the slots overlap.
    const bool in_regs = n <= OT_KREG * OT;
    const int nchunks = (n + OT_KREG * OT - 1) / (OT_KREG * OT);
    const int nslots = in_regs ? (n + OT - 1) / OT : OT_KREG;              // slots in use (uniform): the unrolled slot loops skip the rest
    uint32_t rkey[OT_KREG], rnode[OT_KREG];
    int steps = 0; while ((1 << steps) < ncell) steps++;                    // binary search depth over the cell offsets
    for (int ch = 0; ch < nchunks; ch++) {
        int cell[OT_KREG];
#pragma unroll
        for (int j = 0; j < OT_KREG; j++) cell[j] = 0;
        for (int sdep = steps - 1; sdep >= 0; sdep--) {                    // largest c with celloff[c] <= t, all slots in lock step
#pragma unroll
            for (int j = 0; j < OT_KREG; j++) {
                if (j < nslots) {                                           // (a guard, not a break: the slot arrays must stay statically indexed)
                    const int t = (ch * OT_KREG + j) * OT + tid, c = cell[j] + (1 << sdep);
                    if (celloff[min(c, ncell)] <= t) cell[j] = c;           // celloff[ncell] = n > t: an index past the table never wins
                }
            }
        }
#pragma unroll
        for (int j = 0; j < OT_KREG; j++) {
            const int t = (ch * OT_KREG + j) * OT + tid;
            rkey[j] = (j < nslots && t < n) ? cand[(size_t)cell[j] * L.cell_cap + (t - celloff[cell[j]])] : 0u;
        }
#pragma unroll
        for (int j = 0; j < OT_KREG; j++) {
            const int t = (ch * OT_KREG + j) * OT + tid;
            if (t < n) {
                const uint32_t e = rkey[j];
                keys[t] = e;                                               // the final best-key gather reads this copy
                int b = (int)__fdiv_rn((float)(e & 0xFFF), L.hX);
                b = min(b, nIni - 1);
                atomicAdd(&cntA[b], 1);
                rnode[j] = (uint32_t)b;
                if (!in_regs) key_node[t] = (uint16_t)b;
            }
        }
    }
    __syncthreads();
    // drop empty initial nodes (:574-586), keeping order
    if (tid == 0) {
        int m = 0;
        for (int i = 0; i < nIni; i++) {
            if (cntA[i] > 0) { nodeB[m] = nodeA[i]; cntB[m] = cntA[i]; newidKeep[i] = m; ccntB[4 * m] = 0; ccntB[4 * m + 1] = 0; ccntB[4 * m + 2] = 0; ccntB[4 * m + 3] = 0; m++; }
            else newidKeep[i] = -1;
        }
        ctl[6] = m;
    }
    __syncthreads();
    int size = ctl[6];

    // key sweep: key (e, nd) moves to its node of the NEW list (nodeB / cntB) and is counted into that node's quadrant
    auto sweep = [&]() {
        for (int ch = 0; ch < nchunks; ch++) {
#pragma unroll
            for (int jb = 0; jb < OT_KREG; jb += OT_KSUB) {
                if (jb < nslots) {                                          // slots in use only (uniform)
                    uint32_t ex[OT_KSUB], nk[OT_KSUB]; OtNode q[OT_KSUB]; int cn[OT_KSUB];
    #pragma unroll
                    for (int jj = 0; jj < OT_KSUB; jj++) {
                        const int j = jb + jj, t = (ch * OT_KREG + j) * OT + tid;
                        if (!in_regs && t < n) { rkey[j] = keys[t]; rnode[j] = key_node[t]; }
                    }
    #pragma unroll
                    for (int jj = 0; jj < OT_KSUB; jj++) {
                        const int j = jb + jj, t = (ch * OT_KREG + j) * OT + tid;
                        const uint32_t nd = t < n ? rnode[j] : 0u;
                        ex[jj] = (uint32_t)expf[nd]; nk[jj] = (uint32_t)newidKeep[nd]; q[jj] = nodeA[nd];
                    }
    #pragma unroll
                    for (int jj = 0; jj < OT_KSUB; jj++) {
                        const int j = jb + jj, t = (ch * OT_KREG + j) * OT + tid;
                        const uint32_t e = rkey[j], nd = t < n ? rnode[j] : 0u;
                        const int sx = q[jj].x0 + ((q[jj].x1 - q[jj].x0 + 1) >> 1), sy = q[jj].y0 + ((q[jj].y1 - q[jj].y0 + 1) >> 1);
                        const int qd = ((int)(e & 0xFFF) >= sx ? 1 : 0) + ((int)((e >> 12) & 0xFFF) >= sy ? 2 : 0);
                        const uint32_t child = nidc[4 * nd + qd];
                        nk[jj] = ex[jj] ? child : nk[jj];
                    }
    #pragma unroll
                    for (int jj = 0; jj < OT_KSUB; jj++) {
                        const int j = jb + jj, t = (ch * OT_KREG + j) * OT + tid;
                        const uint32_t nd = t < n ? nk[jj] : 0u;
                        cn[jj] = cntB[nd]; q[jj] = nodeB[nd];
                    }
    #pragma unroll
                    for (int jj = 0; jj < OT_KSUB; jj++) {
                        const int j = jb + jj, t = (ch * OT_KREG + j) * OT + tid;
                        if (t < n) {
                            const uint32_t e = rkey[j];
                            rnode[j] = nk[jj];
                            if (!in_regs) key_node[t] = (uint16_t)nk[jj];
                            if (cn[jj] > 1) {
                                const int sx = q[jj].x0 + ((q[jj].x1 - q[jj].x0 + 1) >> 1), sy = q[jj].y0 + ((q[jj].y1 - q[jj].y0 + 1) >> 1);
                                const int qd = ((int)(e & 0xFFF) >= sx ? 1 : 0) + ((int)((e >> 12) & 0xFFF) >= sy ? 2 : 0);
                                atomicAdd(&ccntB[4 * nk[jj] + qd], 1);
                            }
                        }
                    }
                }
            }
        }
    };
    sweep();                                                                // expf = 0: every key follows newidKeep
    __syncthreads();
    { OtNode* tn = nodeA; nodeA = nodeB; nodeB = tn; int* tc = cntA; cntA = cntB; cntB = tc; tc = ccntA; ccntA = ccntB; ccntB = tc; }

    bool phaseB = false;
    int C_front = 0;
    int overflow = 0;
    for (int pass = 0;; pass++) {
        const int prev_size = size;
        int* ctlp = ctl + 2 * (pass & 1);                                   // this pass' control words (cleared during the previous pass)
        int C, keepers;
        if (phaseB) {
            // sort key of a candidate: keys held (desc), list position (asc); low 2 bits = children - 1
            const int size4 = (size + 3) & ~3;
            for (int i = tid; i < size4; i += OT) {
                uint32_t k = 0;
                if (i < C_front && cntA[i] > 1) {
                    const int inc = (ccntA[4 * i] > 0) + (ccntA[4 * i + 1] > 0) + (ccntA[4 * i + 2] > 0) + (ccntA[4 * i + 3] > 0) - 1;
                    k = ((uint32_t)cntA[i] << 14) | ((uint32_t)(4095 - i) << 2) | (uint32_t)inc;
                }
                skey[i] = (int)k;
            }
            __syncthreads();
            for (int v = tid; v < size; v += OT) {
                const uint32_t kv = (uint32_t)skey[v];
                int e = 0;
                if (kv) {
                    // r = candidates processed before v, sgt = nodes they add beyond themselves
                    int r = 0, sgt = 0;
                    const uint4* s4 = reinterpret_cast<const uint4*>(skey);
                    const int lim = (C_front + 3) >> 2;
                    for (int u = 0; u < lim; u++) {
                        const uint4 kk = s4[u];
                        const int g0 = kk.x > kv, g1 = kk.y > kv, g2 = kk.z > kv, g3 = kk.w > kv;
                        r += g0 + g1 + g2 + g3;
                        sgt += (g0 ? kk.x & 3 : 0) + (g1 ? kk.y & 3 : 0) + (g2 ? kk.z & 3 : 0) + (g3 ? kk.w & 3 : 0);
                    }
                    if (prev_size + sgt < N) {                              // the list is still short when v's turn comes (:730)
                        e = 1; cb[v] = sgt + r;
                        atomicAdd(&ctlp[0], (int)(kv & 3) + 1);
                    }
                }
                expf[v] = e;
                pk[v] = (e ? 0 : 1) << 16;
            }
            __syncthreads();
            C = ctlp[0];
            keepers = ot_array_scan_excl<OT>(pk, size, wtmp) >> 16;
        } else {
            for (int i = tid; i < size; i += OT) {
                const int e = cntA[i] > 1;
                const int nc = e ? (ccntA[4 * i] > 0) + (ccntA[4 * i + 1] > 0) + (ccntA[4 * i + 2] > 0) + (ccntA[4 * i + 3] > 0) : 0;
                expf[i] = e; pk[i] = nc | ((e ? 0 : 1) << 16);
            }
            if (size > OT) __syncthreads();
            const int tot = ot_array_scan_excl<OT>(pk, size, wtmp);
            C = tot & 0xFFFF; keepers = tot >> 16;
        }
        if (tid < 2) ctl[2 * ((pass + 1) & 1) + tid] = 0;                   // every thread is past the previous pass' reads (barriers of the scan)
        const int new_size = C + keepers;
        if (new_size > L.node_cap || new_size > cap_grp) { overflow = 1; break; }
        for (int i = tid; i < size; i += OT) {
            if (expf[i]) {
                const OtNode q = nodeA[i];
                const int sx = q.x0 + ((q.x1 - q.x0 + 1) >> 1), sy = q.y0 + ((q.y1 - q.y0 + 1) >> 1);
                const int base = phaseB ? cb[i] : (pk[i] & 0xFFFF);
                int rk = 0, multi = 0;
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    const int cn = ccntA[4 * i + c];
                    if (cn > 0) {
                        const int np = C - 1 - (base + rk);
                        OtNode chn;
                        chn.x0 = (c & 1) ? (short)sx : q.x0; chn.x1 = (c & 1) ? q.x1 : (short)sx;
                        chn.y0 = (c & 2) ? (short)sy : q.y0; chn.y1 = (c & 2) ? q.y1 : (short)sy;
                        nodeB[np] = chn; cntB[np] = cn; nidc[4 * i + c] = (unsigned short)np;
                        ccntB[4 * np] = 0; ccntB[4 * np + 1] = 0; ccntB[4 * np + 2] = 0; ccntB[4 * np + 3] = 0;
                        multi += cn > 1 ? 1 : 0;
                        rk++;
                    }
                }
                if (multi) atomicAdd(&ctlp[1], multi);
            } else {
                const int np = C + (pk[i] >> 16);
                nodeB[np] = nodeA[i]; cntB[np] = cntA[i]; newidKeep[i] = np;
                ccntB[4 * np] = 0; ccntB[4 * np + 1] = 0; ccntB[4 * np + 2] = 0; ccntB[4 * np + 3] = 0;
            }
        }
        __syncthreads();
        sweep();
        __syncthreads();
        { OtNode* tn = nodeA; nodeA = nodeB; nodeB = tn; int* tc = cntA; cntA = cntB; cntB = tc; tc = ccntA; ccntA = ccntB; ccntB = tc; }
        size = new_size;
        C_front = C;
        const int nToExpand = ctlp[1];
        if (size >= N || size == prev_size) break;                       // :669, :734
        if (!phaseB && size + 3 * nToExpand > N) phaseB = true;           // :673
    }
    if (overflow) { if (tid == 0) { p.status[img] = CORB_ERR_OVERFLOW; *kp_count = 0; } return; }
    // best key of each node: max response, first in candidate order on ties (:741-760)
    for (int i = tid; i < size; i += OT) best[i] = 0;
    __syncthreads();
    for (int ch = 0; ch < nchunks; ch++) {
#pragma unroll
        for (int j = 0; j < OT_KREG; j++) {
            const int t = (ch * OT_KREG + j) * OT + tid;
            if (t < n) {
                const uint32_t e = in_regs ? rkey[j] : keys[t];
                const uint32_t nd = in_regs ? rnode[j] : (uint32_t)key_node[t];
                atomicMax(reinterpret_cast<unsigned int*>(&best[nd]), (e & 0xFF000000u) | (0xFFFFFFu - (uint32_t)t));
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < size; i += OT) {
        const uint32_t t = 0xFFFFFFu - ((uint32_t)best[i] & 0xFFFFFFu);
        const uint32_t e = keys[t];
        kp_out[i] = ((e & 0xFFF) + CORB_MIN_BORDER) | ((((e >> 12) & 0xFFF) + CORB_MIN_BORDER) << 12) | (e & 0xFF000000u);
    }
    if (tid == 0) *kp_count = size;
}

// ------------------------------------------------------------------------------------------------
// cv::fastAtan2 (OpenCV 2.4.8 polynomial form), explicit non-fused float ops.
__device__ __forceinline__ float corb_fast_atan2(float y, float x)
{
    const float p1 = 0.9997878412794807f * (float)(180 / 3.1415926535897932384626433832795);
    const float p3 = -0.3258083974640975f * (float)(180 / 3.1415926535897932384626433832795);
    const float p5 = 0.1555786518463281f * (float)(180 / 3.1415926535897932384626433832795);
    const float p7 = -0.04432655554792128f * (float)(180 / 3.1415926535897932384626433832795);
    const float eps = 2.220446049250313e-16f;      // (float)DBL_EPSILON
    const float ax = fabsf(x), ay = fabsf(y);
    // (one division and one polynomial for both branches of the reference: the operands are selected, the operations are the same)
    const bool xmaj = ax >= ay;
    const float c = __fdiv_rn(xmaj ? ay : ax, __fadd_rn(xmaj ? ax : ay, eps));
    const float c2 = __fmul_rn(c, c);
    float a = __fmul_rn(__fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(p7, c2), p5), c2), p3), c2), p1), c);
    if (!xmaj) a = __fsub_rn(90.f, a);
    if (x < 0) a = __fsub_rn(180.f, a);
    if (y < 0) a = __fsub_rn(360.f, a);
    return a;
}

// sin/cos of a float angle: double Cody-Waite reduction + Taylor polynomials with explicit fma,
// rounded to float -- the numerics contract shared with the oracle (oracle/orc_orb.c orc_sincosf).
__device__ __forceinline__ void corb_sincosf(float xf, float* s, float* c)
{
    const double TWO_OVER_PI = 0.63661977236758134308;
    const double PIO2_HI = 1.57079632679489655800e+00;
    const double PIO2_LO = 6.12323399573676603587e-17;
    const double x = (double)xf;
    const double q = rint(__dmul_rn(x, TWO_OVER_PI));
    double r = __fma_rn(-q, PIO2_HI, x);
    r = __fma_rn(-q, PIO2_LO, r);
    const double r2 = __dmul_rn(r, r);
    double ps = 2.81145725434552076320e-15;
    ps = __fma_rn(ps, r2, -7.64716373181981647590e-13);
    ps = __fma_rn(ps, r2, 1.60590438368216145994e-10);
    ps = __fma_rn(ps, r2, -2.50521083854417187751e-08);
    ps = __fma_rn(ps, r2, 2.75573192239858906526e-06);
    ps = __fma_rn(ps, r2, -1.98412698412698412698e-04);
    ps = __fma_rn(ps, r2, 8.33333333333333333333e-03);
    ps = __fma_rn(ps, r2, -1.66666666666666666667e-01);
    const double sr = __fma_rn(__dmul_rn(r, r2), ps, r);
    double pc = 4.77947733238738529744e-14;
    pc = __fma_rn(pc, r2, -1.14707455977297247139e-11);
    pc = __fma_rn(pc, r2, 2.08767569878680989792e-09);
    pc = __fma_rn(pc, r2, -2.75573192239858906526e-07);
    pc = __fma_rn(pc, r2, 2.48015873015873015873e-05);
    pc = __fma_rn(pc, r2, -1.38888888888888888889e-03);
    pc = __fma_rn(pc, r2, 4.16666666666666666667e-02);
    pc = __fma_rn(pc, r2, -0.5);
    const double cr = __fma_rn(r2, pc, 1.0);
    const long long n = (long long)q;
    double sv, cv;
    switch (n & 3) {
        case 0: sv = sr; cv = cr; break;
        case 1: sv = cr; cv = -sr; break;
        case 2: sv = -sr; cv = -cr; break;
        default: sv = -cr; cv = sr; break;
    }
    *s = (float)sv; *c = (float)cv;
}

__device__ __forceinline__ int wave_sum_i32(int v)
{
    return lx_wave_sum_i(v);
}

// One wavefront (= one 64-thread workgroup) per DSC_KPW keypoints: IC_Angle on the raw level (:77-104), steered
// BRIEF on the blurred level (:108-147, 4 x 64-lane ballots = 256 bits), and the final cv::KeyPoint /
// descriptor row in the reference's output order: levels concatenated, quadtree list order inside a
// level (:1075-1104).  All global reads run along image rows, 16 bytes per lane: the 31x31 raw patch in one sweep (2 lanes per row),
// the 37x37 blurred patch (BRIEF reach = cvRound(13*sqrt 2) = 18) in two (3 lanes per row), staged in LDS.
#define DSC_R 18
#define DSC_W 37
#define DSC_P 40            // LDS pitch of a blurred patch row: 37 + 3 bytes of alignment (fetched as three 16-byte pieces, the last one stored as 8 bytes): 5.9 KB per group
#define DSC_SLOTS 2          // patches in LDS at a time
#define DSC_KPW 4            // keypoints per wavefront: all their load sweeps are in flight before the first is consumed
typedef float corb_float2 __attribute__((ext_vector_type(2)));
#ifndef CORB_DSC_WPE
#define CORB_DSC_WPE 5            // 4 / 5 / 7 in the 512-frame step: 103.9 k / 103.9 k / 105.1 k stereo fps (profiles/r04_variants_wpe.txt): inside the run-to-run spread
#endif
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(CORB_DSC_WPE))) void orb_describe_kernel(const CorbOrbParams p)
{
    __shared__ __attribute__((aligned(16))) uint8_t patch_flat[DSC_SLOTS * DSC_W * DSC_P];   // blurred 37 x 40 patches of the group's keypoints
    int grp, img; corb_xcd_remap(grp, img); img += p.img_base;
    const int lane = threadIdx.x;
    const int slot0 = grp * DSC_KPW;                       // level bases are multiples of 4: one level per group
    const int* kpc = p.kp_count + (size_t)img * CORB_MAX_LEVELS;
    if (grp == 0 && lane == 0) {
        int tot = 0;
        for (int l = 0; l < p.nlevels; l++) tot += kpc[l];
        p.out_count[img] = min(tot, p.out_cap);
        if (tot > p.out_cap) p.status[img] = CORB_ERR_OVERFLOW;
    }
    int level = 0;
    for (int l = 1; l < p.nlevels; l++) if (slot0 >= p.lv[l].kp_base) level = l;
    const CorbLevel& L = p.lv[level];
    const int i0 = slot0 - L.kp_base;
    int nk = min(kpc[level] - i0, DSC_KPW);                // keypoints of this group
    if (nk <= 0) return;
    int off0 = i0;
    for (int l = 0; l < level; l++) off0 += kpc[l];
    nk = min(nk, p.out_cap - off0);
    if (nk <= 0) return;
    const int pitch = L.pitch;
    const uint8_t* rawp = p.pyr + (size_t)img * p.arena_per_image + L.plane_off;
    const uint8_t* blrp = p.blur + (size_t)img * p.arena_per_image + L.plane_off;
    const uint32_t* kpe = p.kp + (size_t)img * p.kp_per_image + slot0;
    // The vector-memory front end bounds this kernel, not the VALU (profiles/r02_dsc): its cost follows the number of 4-lane groups an
    // instruction spreads over cache segments, so the patches are fetched 16 bytes per lane -- 3 lanes per 48-byte row of the blurred patch
    // (2 sweeps per keypoint), 2 lanes per 32-byte row of the raw patch (1 sweep) -- instead of 4 bytes per lane (10 sweeps).
    constexpr int NB = 2;
    uint32_t e[DSC_KPW];
    uint4 bw[DSC_KPW][NB], rw[DSC_KPW];
#pragma unroll
    for (int k = 0; k < DSC_KPW; k++) e[k] = kpe[min(k, nk - 1)];
    // per-lane byte offsets of the sweeps relative to the patch origin (shared by the 4 keypoints; 32-bit arithmetic)
    int boff[NB];
#pragma unroll
    for (int it = 0; it < NB; it++) {
        const int idx = min(lane + 64 * it, DSC_W * 3 - 1);               // the second sweep is partial: clamp (stores are masked)
        const int r = (idx * 171) >> 9, c = idx - 3 * r;                   // idx / 3, idx % 3 for idx < 128
        boff[it] = __mul24(r - DSC_R, pitch) + 16 * c;
    }
    const int rrow = min(lane >> 1, 30), hf = lane & 1;                    // raw patch: row, 16-byte half (lanes 62, 63 repeat the last row with weight 0)
    const int roff = __mul24(rrow - CORB_HALF_PATCH, pitch) + 16 * hf;
    // ---- issue every global load of the group ----
#pragma unroll
    for (int k = 0; k < DSC_KPW; k++) {
        const int x = e[k] & 0xFFF, y = (e[k] >> 12) & 0xFFF;
        const int borg = __mul24(y, pitch) + x - DSC_R - ((x - DSC_R) & 3);     // 4-byte aligned (plane base and pitch are)
#pragma unroll
        for (int it = 0; it < NB; it++) __builtin_memcpy(&bw[k][it], blrp + (uint32_t)(borg + boff[it]), 16);   // global_load_dwordx4, dword-aligned
        const int rorg = __mul24(y, pitch) + x - CORB_HALF_PATCH;
        __builtin_memcpy(&rw[k], rawp + (uint32_t)(rorg + roff), 16);                                            // global_load_dwordx4, byte-aligned
    }
    // ---- intensity centroid (IC_Angle): per-lane byte weights of the circular patch, shared by the 4 keypoints ----
    // m10 = sum u*I, m01 = sum v*I over |u| <= umax[|v|]; exact integers, so the summation order is free.  v_dot4_u32_u8 with the
    // unsigned weights (u+16 / v+16 inside the circle, 0 outside) gives m10 + 16*sum(I) and m01 + 16*sum(I); a 0/1 weight word gives sum(I).
    const unsigned long long UMAX = 0x3689ABCDDEEEFFFFull;      // umax[v] = (UMAX >> 4v) & 15 = {15,15,15,15,14,14,14,13,13,12,11,10,9,8,6,3}
    uint32_t wu[4], wv[4], wm[4];
    {
        const int v = rrow - CORB_HALF_PATCH;
        const int av = v < 0 ? -v : v;
        const int d = lane < 62 ? (int)((UMAX >> (4 * (av & 15))) & 15ull) : -1;
#pragma unroll
        for (int t = 0; t < 4; t++) {
            uint32_t m = 0;
#pragma unroll
            for (int bb = 0; bb < 4; bb++) {
                const int u = -CORB_HALF_PATCH + 16 * hf + 4 * t + bb;
                m |= ((u < 0 ? -u : u) <= d) ? 1u << (8 * bb) : 0u;
            }
            wm[t] = m;
            wu[t] = (m * 0xFFu) & (0x03020100u + (uint32_t)(16 * hf + 4 * t + 1) * 0x01010101u);      // u + 16 = 16 hf + 4 t + 1 + byte
            wv[t] = m * (uint32_t)(v + 16);
        }
    }
    int part[2 * DSC_KPW];                                  // [2k] = m10, [2k+1] = m01 partial sums of this lane
#pragma unroll
    for (int k = 0; k < DSC_KPW; k++) {
        const uint32_t w[4] = {rw[k].x, rw[k].y, rw[k].z, rw[k].w};
        uint32_t a10 = 0, a01 = 0, sall = 0;
#pragma unroll
        for (int t = 0; t < 4; t++) {
            a10 = __builtin_amdgcn_udot4(w[t], wu[t], a10, false);
            a01 = __builtin_amdgcn_udot4(w[t], wv[t], a01, false);
            sall = __builtin_amdgcn_udot4(w[t], wm[t], sall, false);
        }
        part[2 * k] = (int)a10 - 16 * (int)sall; part[2 * k + 1] = (int)a01 - 16 * (int)sall;
    }
    // transposing butterfly: 8 values x 64 lanes -> lane l holds the total of value ((l>>3)&7): 10 exchanges instead of 48
    int t4[4], t2[2], tot;
    {
        // (lane_exchange.h: v_permlane32 / 16 swaps and DPP moves instead of eleven ds_bpermute_b32)
        const bool h3 = lane & 8;
#pragma unroll
        for (int j = 0; j < 4; j++) t4[j] = lx_xadd32_i(part[j], part[j + 4]);
#pragma unroll
        for (int j = 0; j < 2; j++) t2[j] = lx_xadd16_i(t4[j], t4[j + 2]);
        tot = (h3 ? t2[1] : t2[0]) + lx_xor_i<8>(h3 ? t2[0] : t2[1]);
        tot += lx_xor_i<4>(tot); tot += lx_xor_i<2>(tot); tot += lx_xor_i<1>(tot);
        const int other = lx_xor_i<8>(tot);
        t2[0] = h3 ? other : tot;                           // m10 of keypoint (lane >> 4)
        t2[1] = h3 ? tot : other;                           // m01
    }
    // every lane evaluates the angle of keypoint (lane >> 4): one pass for the whole group
    const float angle_l = corb_fast_atan2((float)t2[1], (float)t2[0]);
    const float factorPI = (float)(3.1415926535897932384626433832795 / 180.f);
    float a_l, b_l;
    corb_sincosf(__fmul_rn(angle_l, factorPI), &b_l, &a_l);
    // the 256 test pairs: lane's pairs 64 r + lane as bytes {x0, x1, y0, y1} + 16 (one 16-byte load per lane)
    float4 pat[4];
    {
        const uint4 pb = g_dsc_tab.patb[lane];
        const uint32_t pw4[4] = {pb.x, pb.y, pb.z, pb.w};
#pragma unroll
        for (int r = 0; r < 4; r++)
            pat[r] = make_float4((float)(pw4[r] & 0xFFu) - 16.f, (float)((pw4[r] >> 8) & 0xFFu) - 16.f, (float)((pw4[r] >> 16) & 0xFFu) - 16.f, (float)(pw4[r] >> 24) - 16.f);
    }
    // all blurred patches of the group go to LDS first (one barrier), so the gathers of the keypoints can overlap
    int soff[NB]; bool swide[NB];
#pragma unroll
    for (int it = 0; it < NB; it++) {
        const int idx = min(lane + 64 * it, DSC_W * 3 - 1);
        const int r = (idx * 171) >> 9, c = idx - 3 * r;
        soff[it] = r * DSC_P + 16 * c; swide[it] = c < 2;
    }
    // (the patches pass through LDS DSC_SLOTS at a time: the LDS of a group decides how many groups a CU holds)
    auto stage = [&](int k) {
        uint8_t* pk = patch_flat + (k % DSC_SLOTS) * DSC_W * DSC_P;
#pragma unroll
        for (int it = 0; it < NB; it++) {
            if (lane + 64 * it < DSC_W * 3) {                       // rows are 8-byte aligned: two 8-byte stores, the second only for the first two pieces of a row
                uint2* q = reinterpret_cast<uint2*>(pk + soff[it]);
                q[0] = make_uint2(bw[k][it].x, bw[k][it].y);
                if (swide[it]) q[1] = make_uint2(bw[k][it].z, bw[k][it].w);
            }
        }
    };
    // (row, col) = (rn(x*b + y*a), rn(x*a - y*b)), every product and sum rounded separately (packed fp32, no contraction).  rn() is one more
    // add: s + 1.5 * 2^23 is rounded to an integer by the adder (ties to even, like cvRound's rint), and the integer sits in the low mantissa
    // bits: bits(s + M) = 0x4B400000 + rn(s) for |s| < 2^22.  The byte address row * 40 + col comes out of ONE 24-bit multiply-add on those
    // bit patterns (its low 24 bits are 0x400000 + row); the constant it leaves behind is folded into the patch origin.
    const corb_float2 magic = {12582912.f, 12582912.f};
    constexpr uint32_t MAGIC_LEFT = 0x400000u * (uint32_t)DSC_P + 0x4B400000u;
#pragma unroll
    for (int k = 0; k < DSC_KPW; k++) {
        if (k >= nk) break;
        if (k % DSC_SLOTS == 0) {
            if (k) __syncthreads();
#pragma unroll
            for (int j = 0; j < DSC_SLOTS; j++) stage(k + j);
            __syncthreads();
        }
        const int x = e[k] & 0xFFF, y = (e[k] >> 12) & 0xFFF, s = e[k] >> 24;
        const float angle = __shfl(angle_l, 16 * k), a = __shfl(a_l, 16 * k), b = __shfl(b_l, 16 * k);
        unsigned long long word[4];
        const uint32_t pc = (uint32_t)((k % DSC_SLOTS) * DSC_W * DSC_P + DSC_R * DSC_P + DSC_R + ((x - DSC_R) & 3)) - MAGIC_LEFT;
        const corb_float2 aa = {a, a}, bb = {b, b};
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const corb_float2 X = {pat[r].x, pat[r].y}, Y = {pat[r].z, pat[r].w};
            const corb_float2 ROW = X * bb + Y * aa + magic, COL = X * aa - Y * bb + magic;      // left to right: (X*bb + Y*aa) + magic
            const uint32_t i0 = __umul24(__float_as_uint(ROW.x), DSC_P) + __float_as_uint(COL.x) + pc;     // (by value: __builtin_bit_cast of a vector element reads element 0)
            const uint32_t i1 = __umul24(__float_as_uint(ROW.y), DSC_P) + __float_as_uint(COL.y) + pc;
            const int t0 = patch_flat[i0], t1 = patch_flat[i1];
            word[r] = __ballot(t0 < t1);
        }
        const int off = off0 + k;
        if (lane < 4) {
            unsigned long long* d = reinterpret_cast<unsigned long long*>(p.out_desc + ((size_t)img * p.out_cap + off) * 32);
            d[lane] = lane == 0 ? word[0] : lane == 1 ? word[1] : lane == 2 ? word[2] : word[3];
        }
        if (lane == 0) {
            CorbKeyPoint kq;
            kq.x = level ? __fmul_rn((float)x, L.scale) : (float)x;
            kq.y = level ? __fmul_rn((float)y, L.scale) : (float)y;
            kq.size = (float)L.patch_size; kq.angle = angle; kq.response = (float)s; kq.octave = level; kq.class_id = -1;
            p.out_kp[(size_t)img * p.out_cap + off] = kq;
        }
    }
}

// debugging / test aid: expand the candidate list of one level into cv::KeyPoint form (pre-quadtree)
__global__ __launch_bounds__(64) void orb_candidates_kernel(const CorbOrbParams* __restrict__ pp, int img, int level, CorbKeyPoint* out, int cap, int* n_out)
{
    const CorbOrbParams& p = *pp;
    const CorbLevel& L = p.lv[level];
    if (blockIdx.x != 0) return;
    const int lane = threadIdx.x;
    const int ncell = L.nCols * L.nRows;
    const int* cc = p.cell_count + (size_t)img * p.cells_per_image + L.cell_base;
    const uint32_t* cand = p.cand + (size_t)img * p.cand_per_image + L.cand_base;
    int n = 0;                                            // candidates before this chunk of 64 cells (cell order = reference order)
    for (int c0 = 0; c0 < ncell; c0 += 64) {
        const int c = c0 + lane;
        const int cnt = c < ncell ? cc[c] : 0;
        int incl = cnt;
        incl = lx_wave_incl_scan_i(incl);
        int pos = n + incl - cnt;
        for (int k = 0; k < cnt; k++, pos++) {
            const uint32_t e = cand[(size_t)c * L.cell_cap + k];
            if (pos < cap) { CorbKeyPoint kp; kp.x = (float)(e & 0xFFF); kp.y = (float)((e >> 12) & 0xFFF); kp.size = 7.f; kp.angle = -1.f;
                             kp.response = (float)(e >> 24); kp.octave = 0; kp.class_id = -1; out[pos] = kp; }
        }
        n += __shfl(incl, 63);
    }
    if (lane == 0) *n_out = n;
}

void corb_launch_candidates(const CorbOrbParams* dp, int img, int level, CorbKeyPoint* out, int cap, int* n_out, hipStream_t stream)
{
    hipLaunchKernelGGL(orb_candidates_kernel, dim3(1), dim3(64), 0, stream, dp, img, level, out, cap, n_out);
}

// ------------------------------------------------------------------------------------------------
// Input images arrive as ONE contiguous copy into a device staging buffer (a strided hipMemcpy2D of a 1241-byte-wide image takes
// 2.6 ms, a contiguous 466 KB copy 0.1 ms); this kernel lays the rows out at the pyramid's level-0 pitch.
__global__ __launch_bounds__(256) void orb_ingest_kernel(const uint8_t* __restrict__ src, int w, int h, uint8_t* __restrict__ dst, int pitch, size_t dst_image_stride)
{
    const int x4 = (blockIdx.x * 256 + threadIdx.x) * 4, y = blockIdx.y, img = blockIdx.z;
    if (x4 >= w) return;
    const uint8_t* s = src + ((size_t)img * h + y) * w + x4;
    uint8_t* d = dst + (size_t)img * dst_image_stride + (size_t)y * pitch + x4;
    if (x4 + 4 <= w) { uint32_t v; __builtin_memcpy(&v, s, 4); *reinterpret_cast<uint32_t*>(d) = v; }     // unaligned load, aligned store
    else for (int k = 0; x4 + k < w; k++) d[k] = s[k];
}
void corb_launch_ingest(const uint8_t* stage, int w, int h, int n_images, uint8_t* plane, int pitch, size_t image_stride, hipStream_t stream)
{
    hipLaunchKernelGGL(orb_ingest_kernel, dim3((w + 1023) / 1024, h, n_images), dim3(256), 0, stream, stage, w, h, plane, pitch, image_stride);
}

void corb_orb_device_init()
{
    static CorbDescribeTab tab;
    for (int lane = 0; lane < 64; lane++) {
        uint32_t w[4];
        for (int r = 0; r < 4; r++) {
            const signed char* pt = &corb_brief_pattern_host[(64 * r + lane) * 4];      // {x0, y0, x1, y1}, |.| <= 13
            w[r] = (uint32_t)(pt[0] + 16) | ((uint32_t)(pt[2] + 16) << 8) | ((uint32_t)(pt[1] + 16) << 16) | ((uint32_t)(pt[3] + 16) << 24);
        }
        tab.patb[lane] = make_uint4(w[0], w[1], w[2], w[3]);
    }
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_dsc_tab), &tab, sizeof(tab));
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(orb_octree_kernel<OT_BIG>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(orb_octree_kernel<OT_SMALL>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(orb_octree_kernel<OT_LAT>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
}

void corb_launch_orb_pipeline(const CorbOrbParams& p0, int img_base, int n_images, size_t octree_lds, hipStream_t stream, CorbProfiler* prof, hipEvent_t after_fast)
{
    CorbOrbParams p = p0; p.img_base = img_base;          // the parameter block travels by value (kernarg)
    // development aid (CORB_ORB_SKIP=pyramid,fast,octree,blur,describe): leave launches out after the first 16 pipeline calls have filled every buffer -- the
    // step time without a kernel is the weight that kernel has on the critical path of the overlapped pipeline (results are stale, timing only)
    static const char* skip_env = corb_dev_env("CORB_ORB_SKIP");      // -DCORB_DEV builds only: the shipped library never skips a launch
    static std::atomic<int> calls{0};
    const bool skipping = skip_env && calls.fetch_add(1) >= 16;
    auto skip = [&](const char* name) { return skipping && strstr(skip_env, name) != nullptr; };
    if (skip("pyramid")) {}
    else if (p.pyr_strips > 0)
        CORB_LAUNCH(prof, "orb_pyramid_kernel", orb_pyramid_kernel, dim3(p.pyr_strips * p.pyr_ctiles, n_images), dim3(PYR_T), 0, stream, p);
    else
    for (int l = 1; l < p.nlevels; l++) {
        const CorbLevel& D = p.lv[l];
        dim3 grid((D.w + 255) / 256, (D.h + 4 * RS_ROWS - 1) / (4 * RS_ROWS), n_images), block(64, 4);
        CORB_LAUNCH(prof, "orb_resize_kernel", orb_resize_kernel, grid, block, 0, stream, p, l);
    }
#ifndef CORB_STAGE_AFTER
#define CORB_STAGE_AFTER 1          // the next part-batch of the run starts after this part's: 0 pyramid, 1 FAST, 2 quadtree, 3 blur -- 512-frame steps (tools/gpu_variants.sh,
                                    // profiles/r04_variants_stage.txt): 93.3 k / 103.4 k / 90.6 k / 90.3 k stereo fps
#endif
    if (CORB_STAGE_AFTER == 0 && after_fast) (void)hipEventRecord(after_fast, stream);
    // (cells up to 32 px wide -- KITTI's 31 / 32 -- fit a 40-slot tile pitch; the LDS of a cell is fast_cell_lds_bytes(TP, fast_th), orb_fast_tile.h)
    if (skip("fast")) {}
    else if (fast_tile_pitch_class(p.fast_tp) == 40) CORB_LAUNCH(prof, "orb_fast_kernel", orb_fast_kernel<40>, dim3(p.cells_per_image, n_images), dim3(64), (size_t)fast_dynamic_lds_bytes(40, p.fast_th), stream, p);
    else if (fast_tile_pitch_class(p.fast_tp) == 48) CORB_LAUNCH(prof, "orb_fast_kernel", orb_fast_kernel<48>, dim3(p.cells_per_image, n_images), dim3(64), (size_t)fast_dynamic_lds_bytes(48, p.fast_th), stream, p);
    else CORB_LAUNCH(prof, "orb_fast_kernel", orb_fast_kernel<80>, dim3(p.cells_per_image, n_images), dim3(64), (size_t)fast_dynamic_lds_bytes(80, p.fast_th), stream, p);
    if (CORB_STAGE_AFTER == 1 && after_fast) (void)hipEventRecord(after_fast, stream);      // the next part-batch of the run starts here (corb_orb.cpp: corb_run_parts)
    if (!skip("octree")) {
        // two level groups: [0, split) with OT_BIG threads per (image, level), [split, nlevels) with one wavefront; LDS carved per group
        int split = 0;
        while (split < p.nlevels && p.lv[split].node_cap > OT_SMALL_CAP) split++;
        auto group = [&](int l0, int l1, int& cap, int& ncell) { cap = 0; ncell = 0; for (int l = l0; l < l1; l++) { cap = std::max(cap, p.lv[l].node_cap); ncell = std::max(ncell, p.lv[l].nCols * p.lv[l].nRows); } };
        int cap, ncell;
        // ... and so do handles whose node tables leave room for at most three workgroups per CU (1920 x 1080 / 4000 features: 73 KB each, two per CU = 8 wavefronts):
        // the launch is short of wavefronts, not of slots -- 24.5-24.7 k -> 25.6-25.7 k stereo fps at that size (round 5), where this kernel is the longest of the chain
        group(0, p.nlevels, cap, ncell);
        const bool few_per_cu = corb_octree_lds_bytes(cap, ncell) > (size_t)OT_WIDE_LDS;
        if ((n_images <= OT_LAT_MAX_IMAGES || few_per_cu) && OT_LAT != OT_BIG) {
            CORB_LAUNCH(prof, "orb_octree_kernel", orb_octree_kernel<OT_LAT>, dim3(p.nlevels, n_images), dim3(OT_LAT), corb_octree_lds_bytes(cap, ncell), stream, p, 0, cap, ncell);
            split = p.nlevels;
        } else
        if (split > 0) {
            group(0, split, cap, ncell);
            CORB_LAUNCH(prof, "orb_octree_kernel", orb_octree_kernel<OT_BIG>, dim3(split, n_images), dim3(OT_BIG), corb_octree_lds_bytes(cap, ncell), stream, p, 0, cap, ncell);
        }
        if (split < p.nlevels) {
            group(split, p.nlevels, cap, ncell);
            CORB_LAUNCH(prof, "orb_octree_kernel", orb_octree_kernel<OT_SMALL>, dim3(p.nlevels - split, n_images), dim3(OT_SMALL), corb_octree_lds_bytes(cap, ncell), stream, p, split, cap, ncell);
        }
    }
    if (CORB_STAGE_AFTER == 2 && after_fast) (void)hipEventRecord(after_fast, stream);
    // One stream, one chain.  (Running the blur on a side stream next to FAST + quadtree was measured: the three
    // kernels fight for the same VGPR/wave slots and the chain is not shorter; batches in flight on independent
    // handles are the way to fill the latency-bound phases.  Round 4, 512-frame steps: the quadtree kernel on a high- / low-priority side stream with the blur
    // beside it on the part's stream, 101.0 k -> 94.4 k / 92.5 k stereo fps, profiles/r04_variants_octree.txt.)  The blur runs last so its output is the freshest data
    // in L2/MALL when the describe kernel gathers its 37x37 patches.
    // (Round 5, per-frame chain of corb_stereo_frames captured with the blur as a second branch beside FAST + quadtree: 0.1828 -> 0.1824 ms of kernels at
    // B = 1 -- a graph's cross-stream edges cost what the 12 us branch saves; dropped.)
    if (!skip("blur")) CORB_LAUNCH(prof, "orb_blur_kernel", orb_blur_kernel, dim3(p.blur_tiles_per_image, n_images), dim3(CORB_BLUR_T), 0, stream, p);
    if (CORB_STAGE_AFTER == 3 && after_fast) (void)hipEventRecord(after_fast, stream);
    if (!skip("describe")) CORB_LAUNCH(prof, "orb_describe_kernel", orb_describe_kernel, dim3((p.kp_per_image + DSC_KPW - 1) / DSC_KPW, n_images), dim3(64), 0, stream, p);
}
