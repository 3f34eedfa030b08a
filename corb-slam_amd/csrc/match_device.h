// match_device.h -- device pieces of SearchByBoW shared by match_kernels.hip (one keyframe pair per launch) and fusion_kernels.hip (many pairs per launch): one
// wavefront's walk over one common vocabulary node, and the rotation-histogram filter of one pair.
#pragma once
#include "corb_internal.h"
#include "match_internal.h"
#include "lane_exchange.h"

// (wave reductions through v_permlane swaps and DPP moves: lane_exchange.h)
__device__ __forceinline__ int wmin_i32(int v) { return lx_wave_min_i(v); }
__device__ __forceinline__ unsigned wmin_u32(unsigned v) { return lx_wave_min_u(v); }
__device__ __forceinline__ int hamming256(const unsigned long long* a, const unsigned long long* b) {
    return __popcll(a[0] ^ b[0]) + __popcll(a[1] ^ b[1]) + __popcll(a[2] ^ b[2]) + __popcll(a[3] ^ b[3]);
}

__device__ __forceinline__ int rot_bin(float a1, float a2)
{
    float rot = __fsub_rn(a1, a2);
    if (rot < 0.0f) rot = __fadd_rn(rot, 360.0f);
    int bin = (int)roundf(__fmul_rn(rot, 1.0f / CORB_HISTO_LENGTH));
    if (bin == CORB_HISTO_LENGTH) bin = 0;
    return bin;
}

// SearchByBoW inside one vocabulary node common to both feature vectors (node na of fv1, nb of fv2), by one wavefront.  The reference's order dependence (a Frame
// feature can be claimed once, ORBmatcher.cc:212 / 711) is kept by walking the KF features serially while the 64 lanes scan the other side's features.
// d.valid2 is read for variant 1 only.
__device__ __forceinline__ void bow_match_node(const CorbBowDev& d, int na, int nb, int lane)
{
    const int a0 = d.off1[na], a1 = d.off1[na + 1], b0 = d.off2[nb], b1 = d.off2[nb + 1];
    const int nB = b1 - b0;
    unsigned long long claimed = 0;                 // bit k: list position lane + 64k already matched
    for (int i1 = a0; i1 < a1; i1++) {
        const int idx1 = d.idx1[i1];
        if (!d.valid1[idx1]) continue;
        const unsigned long long* q = d.desc1 + (size_t)idx1 * 4;
        unsigned long long a[4] = {q[0], q[1], q[2], q[3]};
        unsigned b1key = (256u << 16) | 0xFFFFu;    // bestDist1 = 256, first position wins ties
        int b2 = 256;
        for (int k = 0, pos = lane; pos < nB; pos += 64, k++) {
            if ((claimed >> k) & 1ull) continue;
            const int idx2 = d.idx2[b0 + pos];
            if (d.variant == 1 && !d.valid2[idx2]) continue;
            const int dist = hamming256(a, d.desc2 + (size_t)idx2 * 4);
            const unsigned key = ((unsigned)dist << 16) | (unsigned)pos;
            if (key < b1key) { b2 = (int)(b1key >> 16); b1key = key; }
            else if (dist < b2) b2 = dist;
        }
        const unsigned win = wmin_u32(b1key);
        const int second = wmin_i32(b1key == win ? b2 : (int)(b1key >> 16));
        const int bestDist1 = (int)(win >> 16), bestDist2 = min(second, 256);
        const bool pass = d.variant == 0 ? (bestDist1 <= CORB_TH_LOW) : (bestDist1 < CORB_TH_LOW);
        if (pass && (float)bestDist1 < __fmul_rn(d.nnratio, (float)bestDist2)) {
            const int pos = (int)(win & 0xFFFFu);
            if ((pos & 63) == lane) claimed |= 1ull << (pos >> 6);
            if (lane == 0) {
                const int idx2 = d.idx2[b0 + pos];
                const int slot = d.variant == 0 ? idx2 : idx1;
                d.match[slot] = d.variant == 0 ? idx1 : idx2;
                if (d.check_ori) { const int bin = rot_bin(d.angle1[idx1], d.angle2[idx2]); d.bin[slot] = bin; atomicAdd(&d.hist[bin], 1); }
                atomicAdd(d.n_matches, 1);
            }
        }
    }
}

// ComputeThreeMaxima (ORBmatcher.cc:1746-1787) + removal of matches outside the 3 dominant bins, by one workgroup of 256; ind = 3 ints of its LDS
__device__ __forceinline__ void rot_finalize(int* match, int* bin, int n_slots, int* hist, int* n_matches, int stride, int* ind)
{
    if (threadIdx.x == 0) {
        int max1 = 0, max2 = 0, max3 = 0, i1 = -1, i2 = -1, i3 = -1;
        for (int i = 0; i < CORB_HISTO_LENGTH; i++) {
            const int s = hist[i];
            if (s > max1) { max3 = max2; max2 = max1; max1 = s; i3 = i2; i2 = i1; i1 = i; }
            else if (s > max2) { max3 = max2; max2 = s; i3 = i2; i2 = i; }
            else if (s > max3) { max3 = s; i3 = i; }
        }
        if ((float)max2 < __fmul_rn(0.1f, (float)max1)) { i2 = -1; i3 = -1; }
        else if ((float)max3 < __fmul_rn(0.1f, (float)max1)) { i3 = -1; }
        ind[0] = i1; ind[1] = i2; ind[2] = i3;
    }
    __syncthreads();
    int removed = 0;
    for (int s = threadIdx.x; s < n_slots; s += 256) {
        const int b = bin[s];
        if (b < 0 || b == ind[0] || b == ind[1] || b == ind[2]) continue;
        match[(size_t)s * stride] = -1; removed++;
    }
    if (removed) atomicSub(n_matches, removed);
}
