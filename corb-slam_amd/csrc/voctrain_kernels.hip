// voctrain_kernels.hip -- DBoW2's vocabulary training (TemplatedVocabulary::create) on the device for gfx950, one tree level at a time (arithmetic: csrc/voctrain_math.h;
// definition: tests/voctrain_reference.py).  A level is a permutation that holds every active node's descriptors as one contiguous segment in original relative order,
// a segment table, and <= k centres per segment.  Two kernel families compute the same integers:
//   vt_small_kernel     : one workgroup per node whose descriptors fit in LDS: k-means++ seeding, ALL iterations and the stable partition by cluster in one launch.
//   multi-workgroup     : for larger nodes, tiles of VT_TILE positions that never span two segments --
//     vt_first_kernel     draw 0 and the first centre (and the trivial node n <= k) per segment
//     vt_seed_dist_kernel min_dists against the newest centre, and the tile's sum (64-bit integers)
//     vt_seed_pick_kernel per segment: the sum over its tiles, cut_d, the tile and then the position whose running sum first reaches cut_d; the new centre
//     vt_assign_kernel    one descriptor per lane and pass of 256, two 16-byte loads, centres in LDS, four popcounts per centre, strict first minimum; a per-segment
//                         "changed" flag against the previous association
//     vt_converge_kernel  per segment: ended by itself (first unchanged pass), capped, or still running
//     vt_count_kernel     256 bit counters per cluster in LDS, one lane per bit (a lane owns its column: no LDS atomics), flushed with integer atomics
//     vt_majority_kernel  FORB::meanValue's rule per cluster, a wavefront's ballot is one 64-bit word of the centre; an empty cluster keeps its centre and is counted
//     vt_hist / vt_scan / vt_scatter_kernel  the stable partition by cluster: per-tile counts, per-segment offsets, ordered writes
//   vt_ni_kernel        setNodeWeights' Ni: a word bitmap per image and integer atomics (the descent itself is bow_descend_kernel)
// Everything is integer except the comparison against cut_d (vt_reached), so no result depends on launch geometry or arrival order.  Integer atomics only.  No
// device-side printf / assert; every launch is on the caller's stream; all LDS is dynamic and carved in multiples of 16 bytes.
#include "voctrain_internal.h"
#include <mutex>

extern __shared__ __attribute__((aligned(16))) unsigned char vt_lds[];

namespace {

__device__ __forceinline__ int vt_ham(const unsigned long long* a, unsigned long long b0, unsigned long long b1, unsigned long long b2, unsigned long long b3)
{
    return __popcll(a[0] ^ b0) + __popcll(a[1] ^ b1) + __popcll(a[2] ^ b2) + __popcll(a[3] ^ b3);
}
// the cluster of one descriptor: distance first, then the centre's position -- strict `<` in centre order keeps the first minimum (:734-745)
__device__ __forceinline__ int vt_nearest(const unsigned long long* cent, int nc, unsigned long long d0, unsigned long long d1, unsigned long long d2, unsigned long long d3)
{
    unsigned best = 0xFFFFFFFFu;
    for (int c = 0; c < nc; c++) best = min(best, bow_child_key(vt_ham(cent + c * 4, d0, d1, d2, d3), c));
    return (int)(best & 0xFF);
}

// The position whose running sum of md[0 .. n) first reaches cut, given that the sum before md[0] is `before`; n - 1 if none does.  Called by a whole workgroup of 256:
// every lane sums a contiguous chunk into part[], lane 0 walks the 256 partial sums and then one chunk.  Returns in every lane (through *slot).
__device__ int vt_pick_position(const int* md, int n, unsigned long long before, double cut, unsigned long long* part, int* slot)
{
    const int t = threadIdx.x, chunk = (n + 255) / 256, lo = min(n, t * chunk), hi = min(n, lo + chunk);
    unsigned long long s = 0;
    for (int i = lo; i < hi; i++) s += (unsigned long long)md[i];
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        unsigned long long up = before; int pick = n - 1;
        for (int q = 0; q < 256; q++) {
            if (vt_reached(up + part[q], cut)) {
                const int a = min(n, q * chunk), b = min(n, a + chunk);
                for (int i = a; i < b; i++) { up += (unsigned long long)md[i]; if (vt_reached(up, cut)) { pick = i; break; } }
                break;
            }
            up += part[q];
        }
        *slot = pick;
    }
    __syncthreads();
    return *slot;
}

// per-lane counts of the clusters among 4 (or `chunk`) consecutive positions, then per cluster an exclusive scan over the lanes by lane c: cnt[c * 256 + t] becomes the
// rank, inside [0, n), of lane t's first member of cluster c among the members of c.  tot[c] = members of c.
__device__ void vt_rank_clusters(const unsigned char* assoc, int n, int chunk, int k, int* cnt, int* tot)
{
    const int t = threadIdx.x, lo = min(n, t * chunk), hi = min(n, lo + chunk);
    for (int c = 0; c < k; c++) cnt[c * 256 + t] = 0;
    for (int i = lo; i < hi; i++) cnt[(int)assoc[i] * 256 + t]++;
    __syncthreads();
    if (t < k) { int run = 0; for (int q = 0; q < 256; q++) { const int v = cnt[t * 256 + q]; cnt[t * 256 + q] = run; run += v; } tot[t] = run; }
    __syncthreads();
}

// ---------------------------------------------------------------- one workgroup per node ----------------------------------------------------------------
struct VtSmallLds { unsigned long long* desc; unsigned long long* cent; int* cnt; int* md; unsigned long long* part; double* cut; int* misc; unsigned char* assoc; };
__device__ __forceinline__ VtSmallLds vt_small_carve(int max_n)
{
    VtSmallLds l; unsigned char* p = vt_lds;
    l.desc = (unsigned long long*)p; p += (size_t)max_n * 32;
    l.cent = (unsigned long long*)p; p += BOW_MAX_K * 32;
    l.cnt = (int*)p; p += BOW_MAX_K * 256 * 4;
    l.md = (int*)p; p += (size_t)((max_n + 3) & ~3) * 4;
    l.part = (unsigned long long*)p; p += 256 * 8;
    l.cut = (double*)p; p += 16;
    l.misc = (int*)p; p += 64 * 4;                                  // [0] pick [1] changed [2] empties [8 .. 8 + k) members [32 .. 32 + k) bases
    l.assoc = p;
    return l;
}

__global__ __launch_bounds__(256) void vt_small_kernel(VtLevelDev lv, int max_n)
{
    const int si = lv.small_list[blockIdx.x];
    const VtSegDev sg = lv.seg[si];
    const int n = sg.n, k = lv.k, t = threadIdx.x;
    if (n > max_n) return;                                          // (the host sizes max_n from the same table)
    const VtSmallLds l = vt_small_carve(max_n);
    int* members = l.misc + 8; int* base = l.misc + 32;
    for (int i = t; i < n * 4; i += 256) l.desc[i] = lv.desc[(size_t)lv.perm[sg.begin + (i >> 2)] * 4 + (i & 3)];
    if (t < 64) l.misc[t] = 0;
    __syncthreads();
    int nc = 0, iters = 0, capped = 0;
    if (n <= k) {                                                   // :660 one cluster per feature
        nc = n;
        if (t < n) { l.assoc[t] = (unsigned char)t; members[t] = 1; }
        if (t < n * 4) l.cent[t] = l.desc[t];
        __syncthreads();
    } else {
        // ---- initiateClustersKMpp (:833-913) ----
        unsigned j = 1;                                             // lane 0's draw counter
        if (t == 0) l.misc[0] = vt_first_index(vt_draw(lv.seed, sg.key, 0), n);
        __syncthreads();
        const int chunk = (n + 255) / 256, lo = min(n, t * chunk), hi = min(n, lo + chunk);
        for (;;) {
            const int pick = l.misc[0];
            if (t < 4) l.cent[nc * 4 + t] = l.desc[pick * 4 + t];
            nc++;
            __syncthreads();
            if (nc == k) break;
            const unsigned long long c0 = l.cent[(nc - 1) * 4], c1 = l.cent[(nc - 1) * 4 + 1], c2 = l.cent[(nc - 1) * 4 + 2], c3 = l.cent[(nc - 1) * 4 + 3];
            unsigned long long s = 0;
            for (int i = lo; i < hi; i++) { const int d = vt_ham(l.desc + i * 4, c0, c1, c2, c3), m = nc == 1 ? d : min(l.md[i], d); l.md[i] = m; s += (unsigned long long)m; }
            l.part[t] = s;
            __syncthreads();
            if (t == 0) {
                unsigned long long total = 0;
                for (int q = 0; q < 256; q++) total += l.part[q];
                l.misc[0] = total == 0 ? -1 : 0;                    // :908 dist_sum == 0: the node keeps fewer than k centres
                if (total) l.cut[0] = vt_next_cut(lv.seed, sg.key, &j, total);
            }
            __syncthreads();
            if (l.misc[0] < 0) break;
            vt_pick_position(l.md, n, 0, l.cut[0], l.part, &l.misc[0]);
        }
        // ---- the while(goon) loop (:681-781), bounded by max_iterations ----
        for (int it = 1;; it++) {
            if (it > 1) {
                for (int c = 0; c < nc; c++) l.cnt[c * 256 + t] = 0;
                for (int i = 0; i < n; i++) l.cnt[(int)l.assoc[i] * 256 + t] += (int)((l.desc[i * 4 + (t >> 6)] >> (t & 63)) & 1ULL);     // lane t owns bit t
                for (int c = 0; c < nc; c++) {
                    const int m = members[c];                       // uniform
                    if (m == 0) { if (t == 0) l.misc[2]++; continue; }
                    const unsigned long long word = __ballot(l.cnt[c * 256 + t] >= vt_majority_threshold(m));
                    if ((t & 63) == 0) l.cent[c * 4 + (t >> 6)] = word;
                }
                __syncthreads();
            }
            if (t < nc) members[t] = 0;
            if (t == 0) l.misc[1] = 0;
            __syncthreads();
            for (int i = t; i < n; i += 256) {
                const int w = vt_nearest(l.cent, nc, l.desc[i * 4], l.desc[i * 4 + 1], l.desc[i * 4 + 2], l.desc[i * 4 + 3]);
                if (it > 1 && w != (int)l.assoc[i]) l.misc[1] = 1;
                l.assoc[i] = (unsigned char)w;
                atomicAdd(&members[w], 1);
            }
            __syncthreads();
            iters = it;
            if (it > 1 && l.misc[1] == 0) break;
            if (it == lv.max_iterations) { capped = 1; break; }
            __syncthreads();                                        // every lane has read the flag before lane 0 clears it
        }
    }
    // ---- results, and the stable partition by cluster into the same range of the next permutation ----
    if (t < nc * 4) lv.centres[(size_t)si * k * 4 + t] = l.cent[t];
    if (t < k) lv.csize[(size_t)si * k + t] = t < nc ? members[t] : 0;
    if (t == 0) { lv.n_centres[si] = nc; lv.iters[si] = iters; lv.capped[si] = capped; lv.empties[si] = l.misc[2]; }
    const int chunk = (n + 255) / 256;
    vt_rank_clusters(l.assoc, n, chunk, nc, l.cnt, base);
    if (t == 0) { int run = 0; for (int c = 0; c < nc; c++) { const int v = base[c]; base[c] = run; run += v; } }
    __syncthreads();
    for (int i = min(n, t * chunk), hi = min(n, i + chunk); i < hi; i++) {
        const int c = l.assoc[i];
        lv.perm_next[sg.begin + base[c] + l.cnt[c * 256 + t]++] = lv.perm[sg.begin + i];
    }
}

// ---------------------------------------------------------------- multi-workgroup family ----------------------------------------------------------------
__global__ void vt_first_kernel(VtLevelDev lv)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= lv.n_large) return;
    const int si = lv.large_list[q]; const VtSegDev sg = lv.seg[si]; const int k = lv.k;
    lv.iters[si] = 0; lv.capped[si] = 0; lv.empties[si] = 0; lv.changed[si] = 0;
    if (sg.n <= k) {
        for (int i = 0; i < sg.n; i++) {
            for (int w = 0; w < 4; w++) lv.centres[((size_t)si * k + i) * 4 + w] = lv.desc[(size_t)lv.perm[sg.begin + i] * 4 + w];
            lv.assoc[sg.begin + i] = (unsigned char)i;
        }
        lv.n_centres[si] = sg.n; lv.seeding[si] = 0; lv.done[si] = 1;
        return;
    }
    const int first = vt_first_index(vt_draw(lv.seed, sg.key, 0), sg.n);
    for (int w = 0; w < 4; w++) lv.centres[(size_t)si * k * 4 + w] = lv.desc[(size_t)lv.perm[sg.begin + first] * 4 + w];
    lv.n_centres[si] = 1; lv.draw[si] = 1; lv.seeding[si] = 1; lv.done[si] = 0;
}

__global__ __launch_bounds__(256) void vt_seed_dist_kernel(VtLevelDev lv)
{
    const VtTileDev tl = lv.tile[blockIdx.x];
    if (!lv.seeding[tl.seg]) return;
    unsigned long long* part = (unsigned long long*)vt_lds;
    const int nc = lv.n_centres[tl.seg], t = threadIdx.x;
    const unsigned long long* c = lv.centres + ((size_t)tl.seg * lv.k + (nc - 1)) * 4;
    const unsigned long long c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3];
    unsigned long long s = 0;
    for (int i = t; i < tl.n; i += 256) {
        const int pos = tl.begin + i;
        const ulonglong2* dp = reinterpret_cast<const ulonglong2*>(lv.desc + (size_t)lv.perm[pos] * 4);
        const ulonglong2 a = dp[0], b = dp[1];
        const int d = __popcll(a.x ^ c0) + __popcll(a.y ^ c1) + __popcll(b.x ^ c2) + __popcll(b.y ^ c3), m = nc == 1 ? d : min(lv.min_d[pos], d);
        lv.min_d[pos] = m; s += (unsigned long long)m;
    }
    part[t] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) { if (t < h) part[t] += part[t + h]; __syncthreads(); }      // integers: any order gives the same sum
    if (t == 0) lv.tile_sum[blockIdx.x] = part[0];
}

__global__ __launch_bounds__(256) void vt_seed_pick_kernel(VtLevelDev lv)
{
    const int si = lv.large_list[blockIdx.x];
    if (!lv.seeding[si]) return;
    const VtSegDev sg = lv.seg[si];
    unsigned long long* part = (unsigned long long*)vt_lds;         // [256] partial sums, [256] the tile's sum before, [257] cut_d's bits
    int* slot = (int*)(part + 260);                                 // [0] pick [1] tile or -1
    const int t = threadIdx.x, n_tiles = (sg.n + VT_TILE - 1) / VT_TILE;
    if (t == 0) {
        unsigned long long total = 0;
        for (int q = 0; q < n_tiles; q++) total += lv.tile_sum[sg.tile_first + q];
        slot[1] = -1;
        if (total > 0) {
            unsigned j = lv.draw[si];
            const double cut = vt_next_cut(lv.seed, sg.key, &j, total);
            lv.draw[si] = j;
            unsigned long long up = 0; int tile = n_tiles - 1;
            for (int q = 0; q < n_tiles; q++) { const unsigned long long v = lv.tile_sum[sg.tile_first + q]; if (vt_reached(up + v, cut)) { tile = q; break; } if (q < n_tiles - 1) up += v; }
            slot[1] = tile; part[256] = up; part[257] = (unsigned long long)__double_as_longlong(cut);
        }
    }
    __syncthreads();
    const int tile = slot[1];
    if (tile < 0) { if (t == 0) lv.seeding[si] = 0; return; }      // :908 dist_sum == 0
    const unsigned long long before = part[256]; const double cut = __longlong_as_double((long long)part[257]);
    const VtTileDev tl = lv.tile[sg.tile_first + tile];
    __syncthreads();
    int pick = vt_pick_position(lv.min_d + tl.begin, tl.n, before, cut, part, slot);
    // "the last index if none is": none inside the last tile means the last position of the segment, which is that tile's last
    const int nc = lv.n_centres[si];
    if (t < 4) lv.centres[((size_t)si * lv.k + nc) * 4 + t] = lv.desc[(size_t)lv.perm[tl.begin + pick] * 4 + t];
    __syncthreads();
    if (t == 0) { lv.n_centres[si] = nc + 1; if (nc + 1 == lv.k) lv.seeding[si] = 0; }
}

__global__ __launch_bounds__(256) void vt_assign_kernel(VtLevelDev lv, int it)
{
    const VtTileDev tl = lv.tile[blockIdx.x];
    if (lv.done[tl.seg]) return;
    unsigned long long* cent = (unsigned long long*)vt_lds;
    const int nc = lv.n_centres[tl.seg], t = threadIdx.x;
    if (t < nc * 4) cent[t] = lv.centres[(size_t)tl.seg * lv.k * 4 + t];
    __syncthreads();
    bool moved = false;
    for (int i = t; i < tl.n; i += 256) {
        const int pos = tl.begin + i;
        const ulonglong2* dp = reinterpret_cast<const ulonglong2*>(lv.desc + (size_t)lv.perm[pos] * 4);
        const ulonglong2 a = dp[0], b = dp[1];
        const int w = vt_nearest(cent, nc, a.x, a.y, b.x, b.y);
        moved |= w != (int)lv.assoc[pos];
        lv.assoc[pos] = (unsigned char)w;
    }
    if (it > 1 && moved) lv.changed[tl.seg] = 1;                    // every writer stores the same value
}

__global__ void vt_converge_kernel(VtLevelDev lv, int it)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= lv.n_large) return;
    const int si = lv.large_list[q];
    if (lv.done[si]) return;
    if (it > 1 && !lv.changed[si]) { lv.done[si] = 1; lv.iters[si] = it; }
    else if (it == lv.max_iterations) { lv.done[si] = 1; lv.iters[si] = it; lv.capped[si] = 1; }
    else lv.running[0] = 1;
    lv.changed[si] = 0;
}

__global__ __launch_bounds__(256) void vt_count_kernel(VtLevelDev lv)
{
    const VtTileDev tl = lv.tile[blockIdx.x];
    if (lv.done[tl.seg]) return;
    const int nc = lv.n_centres[tl.seg], t = threadIdx.x, k = lv.k, q = lv.seg[tl.seg].large;
    int* cnt = (int*)vt_lds; int* mem = cnt + BOW_MAX_K * 256;
    unsigned long long* d = (unsigned long long*)(mem + 32); unsigned char* as = (unsigned char*)(d + VT_TILE * 4);      // the tile's descriptors and clusters, staged once
    for (int c = 0; c < nc; c++) cnt[c * 256 + t] = 0;
    if (t < nc) mem[t] = 0;
    for (int i = t; i < tl.n * 4; i += 256) d[i] = lv.desc[(size_t)lv.perm[tl.begin + (i >> 2)] * 4 + (i & 3)];
    for (int i = t; i < tl.n; i += 256) as[i] = lv.assoc[tl.begin + i];
    __syncthreads();
    for (int i = 0; i < tl.n; i++) cnt[(int)as[i] * 256 + t] += (int)((d[i * 4 + (t >> 6)] >> (t & 63)) & 1ULL);      // lane t owns bit t; a wavefront reads one address
    for (int i = t; i < tl.n; i += 256) atomicAdd(&mem[(int)as[i]], 1);
    __syncthreads();
    for (int c = 0; c < nc; c++) { const int v = cnt[c * 256 + t]; if (v) atomicAdd(&lv.counters[((size_t)q * k + c) * 256 + t], (unsigned)v); }
    if (t < nc && mem[t]) atomicAdd(&lv.members[(size_t)q * k + t], mem[t]);
}

__global__ __launch_bounds__(256) void vt_majority_kernel(VtLevelDev lv)
{
    const int q = blockIdx.x, si = lv.large_list[q], t = threadIdx.x, k = lv.k;
    if (lv.done[si]) return;
    const int nc = lv.n_centres[si];
    int empties = 0;
    for (int c = 0; c < nc; c++) {
        const int m = lv.members[(size_t)q * k + c];
        unsigned* ctr = lv.counters + ((size_t)q * k + c) * 256;
        if (m == 0) { empties++; continue; }                        // the centre stays (its counters are zero already)
        const unsigned long long word = __ballot((int)ctr[t] >= vt_majority_threshold(m));
        if ((t & 63) == 0) lv.centres[((size_t)si * k + c) * 4 + (t >> 6)] = word;
        ctr[t] = 0;                                                 // ready for the next pass
    }
    __syncthreads();
    if (t < nc) lv.members[(size_t)q * k + t] = 0;
    if (t == 0) lv.empties[si] += empties;
}

__global__ __launch_bounds__(256) void vt_hist_kernel(VtLevelDev lv)
{
    const VtTileDev tl = lv.tile[blockIdx.x];
    int* cnt = (int*)vt_lds; int* tot = cnt + BOW_MAX_K * 256;
    const int nc = lv.n_centres[tl.seg];
    vt_rank_clusters(lv.assoc + tl.begin, tl.n, VT_TILE / 256, nc, cnt, tot);
    if ((int)threadIdx.x < lv.k) lv.tile_hist[(size_t)blockIdx.x * lv.k + threadIdx.x] = (int)threadIdx.x < nc ? tot[threadIdx.x] : 0;
}

// per segment: the members of every cluster, and for every (tile, cluster) where the tile's members of the cluster start inside the segment
__global__ __launch_bounds__(64) void vt_scan_kernel(VtLevelDev lv)
{
    const int si = lv.large_list[blockIdx.x], c = threadIdx.x, k = lv.k;
    const VtSegDev sg = lv.seg[si];
    int* size = (int*)vt_lds;
    const int n_tiles = (sg.n + VT_TILE - 1) / VT_TILE;
    if (c < k) {
        int total = 0;
        for (int q = 0; q < n_tiles; q++) total += lv.tile_hist[(size_t)(sg.tile_first + q) * k + c];
        size[c] = total; lv.csize[(size_t)si * k + c] = total;
    }
    __syncthreads();
    if (c < k) {
        int run = 0;
        for (int j = 0; j < c; j++) run += size[j];
        for (int q = 0; q < n_tiles; q++) { int* h = &lv.tile_hist[(size_t)(sg.tile_first + q) * k + c]; const int v = *h; *h = run; run += v; }
    }
}

__global__ __launch_bounds__(256) void vt_scatter_kernel(VtLevelDev lv)
{
    const VtTileDev tl = lv.tile[blockIdx.x];
    int* cnt = (int*)vt_lds; int* tot = cnt + BOW_MAX_K * 256;
    const int nc = lv.n_centres[tl.seg], t = threadIdx.x, chunk = VT_TILE / 256, seg_begin = lv.seg[tl.seg].begin;
    vt_rank_clusters(lv.assoc + tl.begin, tl.n, chunk, nc, cnt, tot);
    for (int i = min(tl.n, t * chunk), hi = min(tl.n, i + chunk); i < hi; i++) {
        const int c = lv.assoc[tl.begin + i];
        lv.perm_next[seg_begin + lv.tile_hist[(size_t)blockIdx.x * lv.k + c] + cnt[c * 256 + t]++] = lv.perm[tl.begin + i];
    }
}

// setNodeWeights (:968-983): features [first, first + n) belong to images [image_first, image_first + image_count); one bit per (image, word)
__global__ __launch_bounds__(256) void vt_ni_kernel(const int32_t* feat_word, const int32_t* offset, int image_first, int image_count, int first, int n, int words32, unsigned* bitmap, int* ni)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int f = first + i;
    int lo = image_first, hi = image_first + image_count - 1;      // the image with offset[img] <= f < offset[img + 1]
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (offset[mid] <= f) lo = mid; else hi = mid - 1; }
    const int w = feat_word[f];
    const unsigned bit = 1u << (w & 31);
    const unsigned old = atomicOr(&bitmap[(size_t)(lo - image_first) * words32 + (w >> 5)], bit);
    if (!(old & bit)) atomicAdd(&ni[w], 1);
}

}  // namespace

size_t vt_small_lds_bytes(int max_n)
{
    return (size_t)max_n * 32 + BOW_MAX_K * 32 + BOW_MAX_K * 256 * 4 + (size_t)((max_n + 3) & ~3) * 4 + 256 * 8 + 16 + 64 * 4 + (size_t)((max_n + 15) & ~15);
}

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-device attribute of a kernel: opt in once on every device that launches it
hipError_t vt_opt_in_lds()
{
    static std::mutex mu; static bool done[64];
    int dev = 0; (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= 64) return hipErrorInvalidDevice;
    std::lock_guard<std::mutex> lk(mu);
    if (done[dev]) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(vt_small_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)vt_small_lds_bytes(VT_SMALL_MAX));
    done[dev] = e == hipSuccess;
    return e;
}

static const size_t VT_CNT_LDS = BOW_MAX_K * 256 * 4 + 32 * 4, VT_COUNT_LDS = VT_CNT_LDS + VT_TILE * 32 + VT_TILE;

int vt_launch_small(const VtLevelDev& lv, int max_n, hipStream_t s)
{
    if (lv.n_small <= 0) return 0;
    hipLaunchKernelGGL(vt_small_kernel, dim3(lv.n_small), dim3(256), vt_small_lds_bytes(max_n), s, lv, max_n);
    return 1;
}

int vt_launch_seed(const VtLevelDev& lv, hipStream_t s)
{
    if (lv.n_large <= 0) return 0;
    int launches = 1;
    hipLaunchKernelGGL(vt_first_kernel, dim3((lv.n_large + 255) / 256), dim3(256), 0, s, lv);
    for (int c = 1; c < lv.k; c++) {
        hipLaunchKernelGGL(vt_seed_dist_kernel, dim3(lv.n_tile), dim3(256), 256 * 8, s, lv);
        hipLaunchKernelGGL(vt_seed_pick_kernel, dim3(lv.n_large), dim3(256), 264 * 8, s, lv);
        launches += 2;
    }
    return launches;
}

int vt_launch_iteration(const VtLevelDev& lv, int it, hipStream_t s)
{
    if (lv.n_large <= 0) return 0;
    int launches = 2;
    if (it > 1) {
        hipLaunchKernelGGL(vt_count_kernel, dim3(lv.n_tile), dim3(256), VT_COUNT_LDS, s, lv);
        hipLaunchKernelGGL(vt_majority_kernel, dim3(lv.n_large), dim3(256), 0, s, lv);
        launches += 2;
    }
    hipLaunchKernelGGL(vt_assign_kernel, dim3(lv.n_tile), dim3(256), BOW_MAX_K * 32, s, lv, it);
    hipLaunchKernelGGL(vt_converge_kernel, dim3((lv.n_large + 255) / 256), dim3(256), 0, s, lv, it);
    return launches;
}

int vt_launch_partition(const VtLevelDev& lv, hipStream_t s)
{
    if (lv.n_large <= 0) return 0;
    hipLaunchKernelGGL(vt_hist_kernel, dim3(lv.n_tile), dim3(256), VT_CNT_LDS, s, lv);
    hipLaunchKernelGGL(vt_scan_kernel, dim3(lv.n_large), dim3(64), 32 * 4, s, lv);
    hipLaunchKernelGGL(vt_scatter_kernel, dim3(lv.n_tile), dim3(256), VT_CNT_LDS, s, lv);
    return 3;
}

int vt_launch_count_images(const int32_t* feat_word, const int32_t* offset, int image_first, int image_count, int first, int n, int words32, unsigned* bitmap, int* ni, hipStream_t s)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(vt_ni_kernel, dim3((n + 255) / 256), dim3(256), 0, s, feat_word, offset, image_first, image_count, first, n, words32, bitmap, ni);
    return 1;
}
