// bow_device.h -- device pieces of the keyframe database shared by bow_kernels.hip (one query scattered into a dense array) and fusion_kernels.hip (many queries,
// looked up in their sorted word lists): the workgroup's bitonic sort, the words an entry shares with a query, and the L1 score's in-order sum.  The query is a
// functor value_of(word) that returns the query's value of a word, 0 where the query lacks it (a BowVector holds positive values only).
#pragma once
#include "bow_internal.h"

__device__ __forceinline__ double bow_readlane(double v, int lane)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// ascending bitonic sort of keys[0 .. P), P a power of two, by the whole workgroup
template <class Swap> __device__ __forceinline__ void bow_bitonic(unsigned long long* keys, int P, Swap swap_payload)
{
    const int tid = threadIdx.x, T = blockDim.x;
    for (int k2 = 2; k2 <= P; k2 <<= 1)
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += T) {
                const int x = i ^ j;
                if (x > i) {
                    const unsigned long long a = keys[i], b = keys[x];
                    if ((a > b) == ((i & k2) == 0)) { keys[i] = b; keys[x] = a; swap_payload(i, x); }
                }
            }
            __syncthreads();
        }
}

// words the entry (w[0 .. nw) ascending) shares with the query: count and the first of them (lane-uniform results)
template <class Present> __device__ __forceinline__ int bow_wave_common(const uint32_t* w, int nw, int lane, Present present, uint32_t* first)
{
    int common = 0; uint32_t fw = 0;
    for (int base = 0; base < nw; base += 64) {
        const int i = base + lane;
        uint32_t wi = 0; bool c = false;
        if (i < nw) { wi = w[i]; c = present(wi); }
        const unsigned long long m = __ballot(c);
        if (m) {
            if (!common) fw = (uint32_t)__builtin_amdgcn_readlane((int)wi, __ffsll((long long)m) - 1);
            common += __popcll(m);
        }
    }
    *first = fw;
    return common;
}

// L1Scoring::score of the query against the entry (w, val)[0 .. nw): the common words' terms in ascending word order (lane-uniform result)
template <bool TIMED, class ValueOf> __device__ __forceinline__ double bow_wave_score(const uint32_t* w, const double* val, int nw, int lane, ValueOf value_of, unsigned long long& sum_ticks)
{
    double sum = 0.0;
    for (int base = 0; base < nw; base += 64) {
        const int i = base + lane;
        double term = 0.0; bool c = false;
        if (i < nw) { const double q = value_of(w[i]); if (q > 0.0) { c = true; term = bow_score_term(q, val[i]); } }
        unsigned long long m = __ballot(c);
        const unsigned long long t0 = TIMED ? wall_clock64() : 0;
        while (m) { const int j = __ffsll((long long)m) - 1; m &= m - 1; sum += bow_readlane(term, j); }
        if (TIMED) sum_ticks += wall_clock64() - t0;
    }
    return bow_score_finish(sum);
}
