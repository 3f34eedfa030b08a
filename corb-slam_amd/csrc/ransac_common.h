// ransac_common.h -- what the three RANSAC routes share (Sim3Solver: sim3_ransac_kernels.hip / corb_sim3_ransac.cpp, PnPsolver: pnp_ransac_kernels.hip /
// corb_pnp_ransac.cpp, Initializer: init_math.h / corb_initializer.cpp), each rule stated once: the draw, SetRansacParameters' iteration cap, the range check of
// rand_values, the scatter of an inlier mask into byte flags, the inlier loop of a hypothesis wave, the record routes' correspondence set, and a call's buffers, launches and read-back.  The first part is plain
// C++ that a stand-alone host program compiles (tests/host/ransac_common_main.cpp; tests/ransac_reference.py restates it); the second part needs HIP.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RANSAC_HD __host__ __device__ __forceinline__
#else
#define RANSAC_HD inline
#endif

// The n <= MAX draws of one iteration (Sim3Solver.cc:163-177, PnPsolver.cc:233-246, Initializer.cc:87-96 with DUtils::Random::RandomInt): randi = int(rand() /
// (RAND_MAX + 1.0) * size) over the shrinking vAvailableIndices, RAND_MAX + 1 = 2^31, each pick replaced by the vector's back.  The vector is 0 .. N-1 apart from the
// at most MAX positions written so far, kept as (position, value) pairs; a position at or behind the new size is never read.  MAX is a constant so that the loops
// unroll and the pairs live in registers.
template <int MAX> RANSAC_HD void ransac_draw(const int* r, int n, int N, int* idx)
{
    int pos[MAX], val[MAX];
#pragma unroll
    for (int k = 0; k < MAX; k++) {
        if (k >= n) break;
        const int size = N - k;
        const int randi = (int)(((double)r[k] * (1.0 / 2147483648.0)) * (double)size);
        int v = randi, back = size - 1;
#pragma unroll
        for (int j = 0; j < k; j++) { if (pos[j] == randi) v = val[j]; if (pos[j] == size - 1) back = val[j]; }
        idx[k] = v; pos[k] = randi; val[k] = back;
    }
}

// the record routes' correspondence set, [n_cand][cap] each: prepare writes dense and flag per feature, the exclusive scan of the flags (+1 entry) places the accepted
// ones, compaction leaves the N of them in ascending feature order in corr, their features in index and N in ncorr [n_cand].  Host arrays: corr and ncorr alone.
template <class Corr> struct RansacCorrSet { Corr* dense; int* flag; int* scan; int* index; Corr* corr; int* ncorr; };
// what the hypotheses of a call leave: [n_cand][its] records and [n_cand][its][words] inlier mask words
template <class Hyp> struct RansacHyps { Hyp* hyp; unsigned long long* mask; };

// ---- host rules ----
void corb_set_error(const char* fmt, ...);

// mRansacMaxIts of SetRansacParameters (Sim3Solver.cc:125-135, PnPsolver.cc:186-196) from the caller's nMinInliers and float epsilon, with the reference's own
// expression and the host's libm; 0 = iterate() sets bNoMore at once
inline int ransac_iteration_cap(int N, int nMinInliers, float epsilon, double probability, int max_iterations)
{
    if (N < nMinInliers) return 0;
    int nIterations;
    if (nMinInliers == N) nIterations = 1;
    else {
        const double x = ceil(log(1 - probability) / log(1 - pow((double)epsilon, 3.0)));
        nIterations = !(x < (double)max_iterations) ? max_iterations : (x < 1 ? 1 : (int)x);
    }
    const int capped = nIterations < max_iterations ? nIterations : max_iterations;
    return capped < 1 ? 1 : capped;
}
// every rand_values entry is a result of rand(): in [0, 2^31)
inline bool ransac_rand_values_ok(const char* who, const int32_t* rand_values, size_t count)
{
    for (size_t i = 0; i < count; i++) if (rand_values[i] < 0) { corb_set_error("%s: rand_values[%zu] is outside [0, 2^31)", who, i); return false; }
    return true;
}
// the byte flags of one event: bit k of the mask sets flag index[k] (k itself without an index), inside [0, stride) only
inline void ransac_scatter_flags(const unsigned long long* mask_words, int N, const int* index, int stride, uint8_t* flags)
{
    for (int k = 0; k < N; k++) if ((mask_words[k >> 6] >> (k & 63)) & 1ull) { const int f = index ? index[k] : k; if (f >= 0 && f < stride) flags[f] = 1; }
}
// a record call's n_corr and index before anything runs, and for candidate c after the read-back: N = the device's count inside [0, n1], the first N features; -> N
inline void ransac_corr_preset(int n_cand, int n1, int32_t* n_corr, int32_t* index)
{
    for (int c = 0; c < n_cand; c++) n_corr[c] = 0;
    for (size_t i = 0; index && i < (size_t)n_cand * n1; i++) index[i] = -1;
}
inline int ransac_corr_out(const int* h_n, const int* h_index, int c, int n1, int32_t* n_corr, int32_t* index)
{
    const int N = h_n[c] < 0 ? 0 : (h_n[c] > n1 ? n1 : h_n[c]);
    n_corr[c] = N;
    if (index) for (int k = 0; k < N; k++) index[(size_t)c * n1 + k] = h_index[(size_t)c * n1 + k];
    return N;
}

#if defined(__HIPCC__)
#include "corb_workspace.h"
#include "host_util.h"
#include "device_util.h"

// CheckInliers' loop in a hypothesis wave: the lanes stride over the N correspondences, pred(i) is the test of correspondence i, one ballot and one mask word per 64
// (lane 0 stores); the count comes back in every lane.  The ballot needs the full wave: call it from a single-wave workgroup that has taken only wave-uniform
// early returns.
template <class Pred> __device__ __forceinline__ int ransac_inlier_words(int N, int words, unsigned long long* mask, Pred pred)
{
    const int lane = threadIdx.x;
    int count = 0;
    for (int w = 0; w < words; w++) {
        const int i = w * 64 + lane;
        const unsigned long long bits = __ballot(i < N && pred(i));
        if (lane == 0) mask[w] = bits;
        count += __popcll(bits);
    }
    return count;
}
// the body of a compaction kernel over the grid of ransac_launch_corr_set
template <class Corr> __device__ __forceinline__ void ransac_compact(const RansacCorrSet<Corr>& s, int cap)
{
    const int i = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
    const size_t base = (size_t)c * cap;
    if (i == 0) s.ncorr[c] = s.scan[base + cap] - s.scan[base];
    if (i >= cap || !s.flag[base + i]) return;
    const int k = s.scan[base + i] - s.scan[base];
    s.corr[base + k] = s.dense[base + i];
    s.index[base + k] = i;
}
// prepare over (cap, n_cand), and on the record route the scan of the flags and the compaction; Dev holds n_cand, cap and the set
template <class Dev> void ransac_launch_corr_set(void (*prepare)(Dev), void (*compact)(Dev), const Dev& d, bool record_route, int* scan_scratch, hipStream_t s)
{
    const dim3 per_corr((d.cap + 255) / 256, d.n_cand);
    hipLaunchKernelGGL(prepare, per_corr, dim3(256), 0, s, d);
    if (!record_route) return;
    corb_launch_exclusive_scan(d.set.flag, d.set.scan, (size_t)d.n_cand * d.cap, scan_scratch, s);
    hipLaunchKernelGGL(compact, per_corr, dim3(256), 0, s, d);
}

// one {hyp, mask} pair of a call and where its read-back goes
template <class Hyp> struct RansacRead { RansacHyps<Hyp>* dev; std::vector<Hyp>* hyp; std::vector<unsigned long long>* mask; };
// A call's device work behind its uploads: the buffers of the set (host arrays: corr alone, ncorr is uploaded) and of nh hypotheses per pair out of the call's arena,
// the launches, and the one read-back -- every pair, and on the record route N and the feature indices.  Nothing is preset: the host reads only what a kernel has
// written (a hypothesis below its candidate's count of iterations, an index below N).
template <class Hyp, class Dev>
int ransac_run(CorbScratch& pool, Dev& d, bool record_route, size_t nh, void (*launch)(const Dev&, int, int*, hipStream_t), int grid_its,
               std::initializer_list<RansacRead<Hyp>> reads, std::vector<int>* h_n, std::vector<int>* h_index)
{
    const size_t slots = (size_t)d.n_cand * d.cap;
    d.words = (d.cap + 63) / 64;
    int* scan_scratch = nullptr;
    HIPCHK(pool.alloc(&d.set.corr, slots));
    if (record_route) {
        HIPCHK(pool.alloc(&d.set.dense, slots)); HIPCHK(pool.alloc(&d.set.flag, slots + 1)); HIPCHK(pool.alloc(&d.set.scan, slots + 1)); HIPCHK(pool.alloc(&d.set.index, slots));
        HIPCHK(pool.alloc(&d.set.ncorr, (size_t)d.n_cand)); HIPCHK(pool.alloc(&scan_scratch, corb_scan_scratch_ints(slots)));
    }
    for (const RansacRead<Hyp>& r : reads) { HIPCHK(pool.alloc(&r.dev->hyp, nh)); HIPCHK(pool.alloc(&r.dev->mask, nh * d.words)); }
    launch(d, grid_its, scan_scratch, pool.stream);
    HIPCHK(hipGetLastError());
    for (const RansacRead<Hyp>& r : reads) {
        r.hyp->resize(nh); r.mask->resize(nh * d.words);
        HIPCHK(pool.d2h(r.hyp->data(), r.dev->hyp, nh * sizeof(Hyp))); HIPCHK(pool.d2h(r.mask->data(), r.dev->mask, nh * d.words * 8));
    }
    if (record_route) {
        h_n->resize((size_t)d.n_cand); h_index->resize(slots);
        HIPCHK(pool.d2h(h_n->data(), d.set.ncorr, (size_t)d.n_cand * 4)); HIPCHK(pool.d2h(h_index->data(), d.set.index, slots * 4));
    }
    HIPCHK(pool.fetch_finish());
    return CORB_OK;
}
#endif
