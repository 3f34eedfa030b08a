// distinctive.h -- the selection of MapPoint::ComputeDistinctiveDescriptors (C/src/MapPoint.cc:371-395) for one wavefront, shared by the kernels that run it on
// descriptors they gathered (map_kernels.hip: corb_distinctive_descriptors, corb_mp_store_replace; kfinsert_kernels.hip: corb_kfi_process_new_keyframe).  Device code only.
#pragma once
#include "corb_internal.h"

#define DD_MAX_OBS 1024        // observations per map point held in LDS (more is reported, never truncated silently)

__device__ __forceinline__ int mk_hamming(const unsigned long long* a, const unsigned long long* b)
{ return __popcll(a[0] ^ b[0]) + __popcll(a[1] ^ b[1]) + __popcll(a[2] ^ b[2]) + __popcll(a[3] ^ b[3]); }

// the row of the N x N Hamming matrix with the least median (first on ties): MapPoint.cc:371-395.  One wavefront; dist = N shorts of LDS; D = N descriptors (4 x 64 bit)
__device__ __forceinline__ int distinctive_best(const unsigned long long* D, int N, unsigned short* dist, int lane)
{
    const int kth = (int)(0.5 * (double)(N - 1));                   // vDists[0.5*(N-1)]
    int best_median = 0x7FFFFFFF, best = 0;
    for (int i = 0; i < N; i++) {
        const unsigned long long a[4] = { D[(size_t)i * 4], D[(size_t)i * 4 + 1], D[(size_t)i * 4 + 2], D[(size_t)i * 4 + 3] };
        for (int j = lane; j < N; j += 64) dist[j] = (unsigned short)(j == i ? 0 : mk_hamming(a, D + (size_t)j * 4));
        // k-th smallest of dist[0..N): fix the bits from the top; `cand` = elements agreeing with the prefix so far
        int prefix = 0, k = kth;
        for (int bit = 8; bit >= 0; bit--) {
            int zeros = 0;
            for (int j0 = 0; j0 < N; j0 += 64) {
                const int j = j0 + lane;
                const bool is_zero = j < N && ((dist[j] >> (bit + 1)) == (prefix >> (bit + 1))) && !((dist[j] >> bit) & 1);
                zeros += __popcll(__ballot(is_zero));
            }
            if (k >= zeros) { k -= zeros; prefix |= 1 << bit; }
        }
        if (prefix < best_median) { best_median = prefix; best = i; }
    }
    return best;
}
