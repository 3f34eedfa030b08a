// covis_device.h -- device helpers of the kernels that walk the stores' records with the covisibility graph (covis_kernels.hip, localmap_kernels.hip)
#pragma once
#include "covis_internal.h"
#include "lane_exchange.h"

// entries a row is sorted as: the power of two at or above max_connections, at least a wavefront
__host__ __device__ static inline int covis_pow2(int M) { int p = 64; while (p < M) p <<= 1; return p; }
__device__ __forceinline__ const KfHeader* covis_kf(const CovisStores& S, int slot) { return reinterpret_cast<const KfHeader*>(S.kf_base + (size_t)slot * S.kf_bytes); }
__device__ __forceinline__ int covis_kf_n(const CovisStores& S, int slot) { return min(max(covis_kf(S, slot)->n, 0), S.F); }
// the record of a non-bad map point by id, or nullptr (getMapPoint() is NULL, or isBad())
__device__ __forceinline__ const char* covis_good_point(const CovisStores& S, unsigned long long id, int* slot_out)
{
    if (id == CORB_NO_MAP_POINT) return nullptr;
    const int ms = corb_idtab_find(S.mpid, id);
    if (ms < 0 || ms >= S.mp_capacity) return nullptr;
    const char* r = S.mp_base + (size_t)ms * S.mp_bytes;
    if (reinterpret_cast<const CorbMapPointRecord*>(r)->flags & CORB_MP_BAD) return nullptr;
    *slot_out = ms;
    return r;
}
__device__ __forceinline__ int covis_n_obs(const CovisStores& S, const char* mrec) { return min(max(reinterpret_cast<const CorbMapPointRecord*>(mrec)->n_obs, 0), S.O); }

// a[0 .. n) -> exclusive prefix sums in place, the total returned to every thread; a thread owns ceil(n / COVIS_T) consecutive entries
__device__ __forceinline__ int covis_block_scan(int* a, int n, int* sh)
{
    const int per = (n + COVIS_T - 1) / COVIS_T;
    const int b = min((int)threadIdx.x * per, n), e = min(b + per, n);
    int sum = 0;
    for (int i = b; i < e; i++) sum += a[i];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int inc = lx_wave_incl_scan_i(sum);
    if (lane == 63) sh[w] = inc;
    __syncthreads();
    int base = 0, total = 0;
    for (int i = 0; i < COVIS_T / 64; i++) { if (i < w) base += sh[i]; total += sh[i]; }
    int run = base + inc - sum;
    for (int i = b; i < e; i++) { const int v = a[i]; a[i] = run; run += v; }
    __syncthreads();
    return total;
}
// P entries (id, slot) in LDS -> ascending id (LightKeyFrame::operator<); pads carry COVIS_NO_ID and sort behind every entry
__device__ __forceinline__ void covis_sort_by_id(unsigned long long* sid, int* sslot, int P)
{
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < P; i += COVIS_T) {
                const int x = i ^ j;
                if (x > i) {
                    const bool up = (i & k) == 0;
                    const unsigned long long a = sid[i], b = sid[x];
                    if (up ? a > b : a < b) { const int sa = sslot[i]; sid[i] = b; sid[x] = a; sslot[i] = sslot[x]; sslot[x] = sa; }
                }
            }
            __syncthreads();
        }
    }
}
