// bow_kernels.hip -- DBoW2 on the device for gfx950 (arithmetic: csrc/bow_math.h; definition: tests/dbow_reference.py):
//   bow_descend_kernel<G>  : TemplatedVocabulary::transform of one feature (:1218-1259) by a group of G = 16 or 32 lanes, one lane per child: a level is one coalesced read of
//                            the children's descriptors (contiguous in child order), 4 x u64 xor + popcount per lane, and a minimum over bow_child_key (distance, then
//                            child position: the first minimum wins) -- DPP moves inside a row of 16 lanes, one ds_bpermute more for G = 32.  Latency-bound: L dependent levels.
//   bow_build_kernel       : one workgroup per descriptor set builds both sorted outputs in LDS: a bitonic sort of (word, feature) keys, the value of every word by repeated
//                            addition of its weight (BowVector::addWeight, one lane per word), the L1 norm summed by ONE lane in ascending word order (BowVector::normalize;
//                            the order is part of the definition), the division; then the same sort on (node, feature) keys and a ballot compaction into CorbFeatVec form.
//                            16 bytes of LDS per feature slot: BOW_MAX_FEATURES = 8192 features use 128 KiB of the 160.
//   kfdb_scatter_kernel    : the query's BowVector into a dense array over the words (and the loop query's connected keyframes into flags); kfdb_unscatter_kernel undoes it
//   kfdb_count_kernel      : one wavefront per live entry: words in common with the query and the first of them (ballots over the entry's ascending words), then the
//                            entry's fields by bow_visit_loop / bow_visit_reloc and maxCommonWords by an atomic maximum
//   kfdb_score_kernel      : one wavefront per entry that entered the list with more than minCommonWords: the L1 score's terms of 64 words at a time, added in ascending
//                            word order through v_readlane of the lanes a ballot names; kept entries are appended with the key (first common word, sequence number)
//   kfdb_select_kernel     : one workgroup: bitonic sort of the kept entries by that key (the reference's list order), bow_accumulate per entry, the maximum, the 0.75
//                            threshold, first appearance per best keyframe by an atomic minimum of positions, and an ordered ballot compaction of the candidates
//   kfdb_score_list_kernel : corb_kfdb_score: one wavefront per listed entry, the same in-order sum
//   kfdb_*_q_kernel        : the same bodies for the loop query of corb_loop_detect, whose id, minScore and connected set never visit the host: read from a
//                            BowLoopQuery in device memory, every kernel a no-op while its skip flag is set; kfdb_min_score_q_kernel is the minScore loop itself
// No scalar memory writes, no device-side printf / assert; every launch is on the caller's stream.
#include "bow_internal.h"
#include "bow_device.h"
#include "lane_exchange.h"
#include <mutex>

namespace {

template <int G> __global__ __launch_bounds__(256) void bow_descend_kernel(BowVocView v, const BowSetDev* sets, int levelsup, int32_t* feat_word, uint32_t* feat_node)
{
    const BowSetDev& s = sets[blockIdx.y];
    const int n = s.n;
    const int f = blockIdx.x * (256 / G) + (int)threadIdx.x / G, c = (int)threadIdx.x % G;
    if (f >= n) return;                                         // whole groups leave: every exchange below stays inside a group
    const unsigned long long* dp = s.desc + (size_t)f * 4;
    const unsigned long long d0 = dp[0], d1 = dp[1], d2 = dp[2], d3 = dp[3];
    const int nid_level = v.L - levelsup;
    int nid = nid_level <= 0 ? 0 : -1, node = 0, level = 0;
    do {
        ++level;
        const int first = v.child_first[node], cnt = v.child_count[node];
        unsigned key = 0xFFFFFFFFu;
        if (c < cnt) {
            const ulonglong2* q = reinterpret_cast<const ulonglong2*>(v.slot_desc + (size_t)(first + c) * 4);
            const ulonglong2 a = q[0], b = q[1];
            key = bow_child_key(__popcll(a.x ^ d0) + __popcll(a.y ^ d1) + __popcll(b.x ^ d2) + __popcll(b.y ^ d3), c);
        }
        key = min(key, (unsigned)lx_xor_i<1>((int)key)); key = min(key, (unsigned)lx_xor_i<2>((int)key));
        key = min(key, (unsigned)lx_xor_i<4>((int)key)); key = min(key, (unsigned)lx_xor_i<8>((int)key));
        if (G == 32) key = min(key, (unsigned)__shfl_xor((int)key, 16));
        node = v.slot_node[first + (int)(key & 0xFF)];
        if (level == nid_level) nid = node;
    } while (v.child_count[node] > 0);
    if (c == 0) { feat_word[s.feat_off + f] = v.node_word[node]; feat_node[s.feat_off + f] = (uint32_t)(nid < 0 ? node : nid); }
}

__global__ __launch_bounds__(256) void bow_build_kernel(BowVocView v, const BowSetDev* sets, const int32_t* feat_word, const uint32_t* feat_node, unsigned long long* ticks)
{
    const unsigned long long t_begin = ticks ? wall_clock64() : 0;
    extern __shared__ unsigned long long bow_smem[];            // keys[P] | vals[P]
    __shared__ int s_m, s_cnt; __shared__ double s_norm;
    const BowSetDev s = sets[blockIdx.x];
    const int tid = threadIdx.x, T = blockDim.x, n = s.n;
    int P = 1; while (P < n) P <<= 1;
    unsigned long long* keys = bow_smem; double* vals = reinterpret_cast<double*>(bow_smem + P);
    const int32_t* fw = feat_word + s.feat_off; const uint32_t* fn = feat_node + s.feat_off;
    const unsigned long long PAD = ~0ull;
    auto no_payload = [](int, int) {};

    // ---- BowVector: (word, feature) ascending; stopped features (weight <= 0, :1157) are padding ----
    if (tid == 0) s_m = 0;
    __syncthreads();
    for (int i = tid; i < P; i += T) {
        unsigned long long key = PAD;
        if (i < n) { const int w = fw[i]; if (v.word_weight[w] > 0) { key = ((unsigned long long)(unsigned)w << 32) | (unsigned)i; atomicAdd(&s_m, 1); } }
        keys[i] = key;
    }
    __syncthreads();
    bow_bitonic(keys, P, no_payload);
    const int m = s_m;
    for (int p = tid; p < m; p += T) {                          // addWeight: the word's weight once per feature (repeated addition, not count * w)
        const unsigned w = (unsigned)(keys[p] >> 32);
        if (p == 0 || (unsigned)(keys[p - 1] >> 32) != w) {
            const double wt = v.word_weight[w];
            double val = wt;
            for (int q = p + 1; q < m && (unsigned)(keys[q] >> 32) == w; q++) val += wt;
            vals[p] = val;
        }
    }
    __syncthreads();
    if (tid == 0) {                                             // normalize(L1): fabs summed in ascending word order by one lane; the words move to the front on the way
        const unsigned long long t_norm = ticks ? wall_clock64() : 0;
        int cnt = 0; double norm = 0.0; unsigned prev = 0;
        for (int p = 0; p < m; p++) {
            const unsigned w = (unsigned)(keys[p] >> 32);
            if (p == 0 || w != prev) { const double x = vals[p]; keys[cnt] = w; vals[cnt] = x; norm += fabs(x); cnt++; prev = w; }
        }
        s_cnt = cnt; s_norm = norm;
        if (ticks) atomicAdd(&ticks[0], wall_clock64() - t_norm);
    }
    __syncthreads();
    const int n_words = s_cnt; const double norm = s_norm; const bool fits = n_words <= s.max_words;
    if (fits) for (int j = tid; j < n_words; j += T) { s.bow_word[j] = (uint32_t)keys[j]; s.bow_value[j] = norm > 0.0 ? vals[j] / norm : vals[j]; }
    if (tid == 0) { *s.bow_count = fits ? n_words : -1; s.counts[0] = n_words; s.counts[2] = fits ? 0 : 1; }
    __syncthreads();

    // ---- FeatureVector: (node, feature) ascending ----
    for (int i = tid; i < P; i += T) {
        unsigned long long key = PAD;
        if (i < n && v.word_weight[fw[i]] > 0) key = ((unsigned long long)fn[i] << 32) | (unsigned)i;
        keys[i] = key;
    }
    __syncthreads();
    bow_bitonic(keys, P, no_payload);
    for (int p = tid; p < m; p += T) s.fv_idx[p] = (uint32_t)keys[p];
    if (tid < 64) {                                             // one wavefront: the nodes' first positions, compacted in order
        int cnt = 0;
        for (int base = 0; base < m; base += 64) {
            const int p = base + tid;
            const bool start = p < m && (p == 0 || (unsigned)(keys[p - 1] >> 32) != (unsigned)(keys[p] >> 32));
            const unsigned long long mask = __ballot(start);
            if (start) {
                const int at = cnt + __popcll(mask & ((1ull << tid) - 1ull));
                const uint32_t nd = (uint32_t)(keys[p] >> 32);
                s.fv_node[at] = nd; s.node_copy[at] = nd; s.fv_off[at] = p;
            }
            cnt += __popcll(mask);
        }
        if (tid == 0) { s.fv_off[cnt] = m; *s.fv_n_nodes = cnt; s.counts[1] = cnt; if (ticks) atomicAdd(&ticks[1], wall_clock64() - t_begin); }
    }
}

// ---------------------------------------------------------------- keyframe database ----------------------------------------------------------------
__global__ void kfdb_scatter_kernel(BowDbDev d, int q, int nq, int n_conn, int set)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nq) d.dense[d.words[(size_t)q * d.max_words + i]] = set ? d.values[(size_t)q * d.max_words + i] : 0.0;
    if (i < n_conn) d.conn[d.conn_list[i]] = (unsigned char)set;
    if (i < 2 && set) d.ctr[i] = 0;
}

// words the entry shares with the scattered query: count and the first of them (lane-uniform results; the ballots are bow_device.h's)
__device__ __forceinline__ int kfdb_wave_common(const BowDbDev& d, int e, int lane, uint32_t* first)
{
    const double* dense = d.dense;
    return bow_wave_common(d.words + (size_t)e * d.max_words, d.n_words[e], lane, [dense](uint32_t w) { return dense[w] > 0.0; }, first);
}

// L1Scoring::score of the scattered query against entry e: the common words' terms in ascending word order (lane-uniform result)
template <bool TIMED> __device__ __forceinline__ double kfdb_wave_score(const BowDbDev& d, int e, int lane, unsigned long long& sum_ticks)
{
    const double* dense = d.dense;
    return bow_wave_score<TIMED>(d.words + (size_t)e * d.max_words, d.values + (size_t)e * d.max_words, d.n_words[e], lane, [dense](uint32_t w) { return dense[w]; }, sum_ticks);
}

__device__ __forceinline__ void kfdb_count_body(const BowDbDev& d, int kind, unsigned long long id)
{
    const int e = blockIdx.x * 4 + (int)threadIdx.x / 64, lane = threadIdx.x & 63;
    if (e >= d.capacity) return;
    bool pushed = false; uint32_t first = 0;
    if (d.live[e] && d.n_words[e] > 0) {
        const int common = kfdb_wave_common(d, e, lane, &first);
        if (common > 0 && lane == 0) {
            BowKfState st = d.st[e];
            pushed = kind == 0 ? bow_visit_loop(st, id, common, d.conn[e] != 0) : bow_visit_reloc(st, id, common);
            d.st[e] = st;
            if (pushed) atomicMax(&d.ctr[0], kind == 0 ? st.loop_words : st.reloc_words);
        }
    }
    if (lane == 0) { d.pushed[e] = pushed ? 1 : 0; d.first_word[e] = first; }
}

__global__ __launch_bounds__(256) void kfdb_count_kernel(BowDbDev d, int kind, unsigned long long id) { kfdb_count_body(d, kind, id); }

__device__ __forceinline__ void kfdb_score_body(const BowDbDev& d, int kind, float min_score, unsigned long long* ticks)
{
    const unsigned long long t_begin = ticks ? wall_clock64() : 0; unsigned long long t_sum = 0;
    const int e = blockIdx.x * 4 + (int)threadIdx.x / 64, lane = threadIdx.x & 63;
    if (e >= d.capacity || !d.pushed[e]) return;
    const int min_common = bow_min_common(d.ctr[0]);
    const int words = kind == 0 ? d.st[e].loop_words : d.st[e].reloc_words;
    if (words <= min_common) return;
    const float si = (float)(ticks ? kfdb_wave_score<true>(d, e, lane, t_sum) : kfdb_wave_score<false>(d, e, lane, t_sum));
    if (lane != 0) return;
    if (kind == 0) d.st[e].loop_score = si; else d.st[e].reloc_score = si;
    if (kind != 0 || si >= min_score) {
        const int at = atomicAdd(&d.ctr[1], 1);
        d.skey[at] = ((unsigned long long)d.first_word[e] << 32) | d.seq[e]; d.sent[at] = e;
    }
    if (ticks) { atomicAdd(&ticks[2], t_sum); atomicAdd(&ticks[3], wall_clock64() - t_begin); }
}

__global__ __launch_bounds__(256) void kfdb_score_kernel(BowDbDev d, int kind, float min_score, unsigned long long* ticks) { kfdb_score_body(d, kind, min_score, ticks); }

__device__ __forceinline__ void kfdb_select_body(const BowDbDev& d, int kind, unsigned long long id, float min_score)
{
    __shared__ float red[1024]; __shared__ int wave_count[16];
    const int tid = threadIdx.x, T = blockDim.x, S = d.ctr[1];
    if (S == 0) { if (tid == 0) d.out[0] = 0; return; }
    const int min_common = bow_min_common(d.ctr[0]);
    int P = 1; while (P < S) P <<= 1;
    for (int i = S + tid; i < P; i += T) d.skey[i] = ~0ull;
    __syncthreads();
    int* ent = d.sent;
    bow_bitonic(d.skey, P, [ent](int a, int b) { const int t = ent[a]; ent[a] = ent[b]; ent[b] = t; });
    float best = kind == 0 ? min_score : 0.f;                   // bestAccScore (:140, :248)
    for (int i = tid; i < S; i += T) {
        const int e = d.sent[i];
        float acc; int b;
        bow_accumulate(kind, d.st, d.nb + (size_t)e * BOW_NEIGHBOURS, e, kind == 0 ? d.st[e].loop_score : d.st[e].reloc_score, id, min_common, &acc, &b);
        d.acc[i] = acc; d.best[i] = b;
        if (acc > best) best = acc;
    }
    red[tid] = best;
    __syncthreads();
    for (int o = T >> 1; o > 0; o >>= 1) { if (tid < o && red[tid + o] > red[tid]) red[tid] = red[tid + o]; __syncthreads(); }
    const float retain = 0.75f * red[0];                        // :168
    for (int i = tid; i < S; i += T) if (d.acc[i] > retain) atomicMin(&d.first_pos[d.best[i]], i);
    __syncthreads();
    int n_out = 0;
    for (int base = 0; base < S; base += T) {                   // candidates in list order, a best keyframe at its first appearance only
        const int i = base + tid;
        const bool keep = i < S && d.acc[i] > retain && d.first_pos[d.best[i]] == i;
        const unsigned long long m = __ballot(keep);
        if ((tid & 63) == 0) wave_count[tid >> 6] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < 16; w++) { const int c = w < (T >> 6) ? wave_count[w] : 0; if (w < (tid >> 6)) before += c; total += c; }
        if (keep) d.out[1 + n_out + before + __popcll(m & ((1ull << (tid & 63)) - 1ull))] = d.best[i];
        n_out += total;
        __syncthreads();
    }
    for (int i = tid; i < S; i += T) d.first_pos[d.best[i]] = BOW_NO_POS;
    if (tid == 0) d.out[0] = n_out;
}

__global__ __launch_bounds__(1024) void kfdb_select_kernel(BowDbDev d, int kind, unsigned long long id, float min_score) { kfdb_select_body(d, kind, id, min_score); }

__device__ __forceinline__ void kfdb_score_list_body(const BowDbDev& d, const int* entries, int n)
{
    const int i = blockIdx.x * 4 + (int)threadIdx.x / 64, lane = threadIdx.x & 63;
    if (i >= n) return;
    const int e = entries[i];
    unsigned long long unused = 0;
    const double s = d.n_words[e] > 0 ? kfdb_wave_score<false>(d, e, lane, unused) : bow_score_finish(0.0);
    if (lane == 0) d.score_out[i] = s;
}

__global__ __launch_bounds__(256) void kfdb_score_list_kernel(BowDbDev d, const int* entries, int n) { kfdb_score_list_body(d, entries, n); }

// ---- the loop query with its id, minScore and connected set in device memory (BowLoopQuery, bow_internal.h): the bodies above behind q->skip ----
__global__ void kfdb_scatter_q_kernel(BowDbDev d, int q, int nq, const BowLoopQuery* p, int set)
{
    if (p->skip) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nq) d.dense[d.words[(size_t)q * d.max_words + i]] = set ? d.values[(size_t)q * d.max_words + i] : 0.0;
    if (i < 2 && set) d.ctr[i] = 0;
    if (!set) for (int j = i; j < p->n_conn; j += gridDim.x * blockDim.x) d.conn[d.conn_list[j]] = 0;
}
__global__ __launch_bounds__(256) void kfdb_score_list_q_kernel(BowDbDev d, const int* entries, const BowLoopQuery* p) { if (!p->skip) kfdb_score_list_body(d, entries, p->n_score); }
// minScore (LoopClosing.cc:124-137): each score rounded to float, the minimum from 1.0f (one wavefront)
__global__ __launch_bounds__(64) void kfdb_min_score_q_kernel(BowDbDev d, BowLoopQuery* p)
{
    if (p->skip) return;
    float m = 1.0f;
    for (int i = threadIdx.x; i < p->n_score; i += 64) { const float s = (float)d.score_out[i]; if (s < m) m = s; }
    for (int o = 32; o > 0; o >>= 1) { const float t = __shfl_xor(m, o); if (t < m) m = t; }
    if (threadIdx.x == 0) p->min_score = m;
}
__global__ __launch_bounds__(256) void kfdb_count_q_kernel(BowDbDev d, const BowLoopQuery* p) { if (!p->skip) kfdb_count_body(d, 0, p->id); }
__global__ __launch_bounds__(256) void kfdb_score_q_kernel(BowDbDev d, const BowLoopQuery* p) { if (!p->skip) kfdb_score_body(d, 0, p->min_score, nullptr); }
__global__ __launch_bounds__(1024) void kfdb_select_q_kernel(BowDbDev d, const BowLoopQuery* p) { if (!p->skip) kfdb_select_body(d, 0, p->id, p->min_score); }

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-device attribute of a kernel: opt in once on every device that launches it
hipError_t bow_opt_in_lds()
{
    static std::mutex mu; static bool done[64];
    int dev = 0; (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= 64) return hipErrorInvalidDevice;
    std::lock_guard<std::mutex> lk(mu);
    if (done[dev]) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(bow_build_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, BOW_MAX_FEATURES * 16);
    done[dev] = e == hipSuccess;
    return e;
}

}  // namespace

void corb_launch_bow_transform(const BowVocView& v, const BowSetDev* sets, int n_sets, int max_n, int levelsup, int32_t* feat_word, uint32_t* feat_node, hipStream_t s, int* rc_attr)
{
    if (n_sets <= 0 || n_sets > BOW_MAX_SETS) return;
    const hipError_t ea = bow_opt_in_lds();
    if (rc_attr) *rc_attr = (int)ea;
    if (ea != hipSuccess) return;
    const BowProfile pf = corb_bow_profile_state();
    if (max_n > 0) {
        if (v.k <= 16) CORB_LAUNCH(pf.prof, "bow_descend_kernel", bow_descend_kernel<16>, dim3((max_n + 15) / 16, n_sets), dim3(256), 0, s, v, sets, levelsup, feat_word, feat_node);
        else CORB_LAUNCH(pf.prof, "bow_descend_kernel", bow_descend_kernel<32>, dim3((max_n + 7) / 8, n_sets), dim3(256), 0, s, v, sets, levelsup, feat_word, feat_node);
    }
    int P = 1; while (P < max_n) P <<= 1;
    CORB_LAUNCH(pf.prof, "bow_build_kernel", bow_build_kernel, dim3(n_sets), dim3(256), (size_t)P * 16, s, v, sets, feat_word, feat_node, pf.ticks);
}

// the descent alone: vocabulary training counts the images of every word with it (sets[i] needs desc, n and feat_off only; any number of features per set)
void corb_launch_bow_descend(const BowVocView& v, const BowSetDev* sets, int n_sets, int max_n, int32_t* feat_word, uint32_t* feat_node, hipStream_t s)
{
    if (n_sets <= 0 || n_sets > BOW_MAX_SETS || max_n <= 0) return;
    const BowProfile pf = corb_bow_profile_state();
    if (v.k <= 16) CORB_LAUNCH(pf.prof, "bow_descend_kernel", bow_descend_kernel<16>, dim3((max_n + 15) / 16, n_sets), dim3(256), 0, s, v, sets, 0, feat_word, feat_node);
    else CORB_LAUNCH(pf.prof, "bow_descend_kernel", bow_descend_kernel<32>, dim3((max_n + 7) / 8, n_sets), dim3(256), 0, s, v, sets, 0, feat_word, feat_node);
}

void corb_launch_kfdb_detect(const BowDbDev& d, int kind, int q, int nq, unsigned long long id, int n_conn, float min_score, hipStream_t s)
{
    const int n_sc = nq > n_conn ? nq : n_conn, g_sc = (((n_sc > 2 ? n_sc : 2) + 255) / 256), g_e = (d.capacity + 3) / 4;
    const BowProfile pf = corb_bow_profile_state();
    CORB_LAUNCH(pf.prof, "kfdb_scatter_kernel", kfdb_scatter_kernel, dim3(g_sc), dim3(256), 0, s, d, q, nq, n_conn, 1);
    CORB_LAUNCH(pf.prof, "kfdb_count_kernel", kfdb_count_kernel, dim3(g_e), dim3(256), 0, s, d, kind, id);
    CORB_LAUNCH(pf.prof, "kfdb_score_kernel", kfdb_score_kernel, dim3(g_e), dim3(256), 0, s, d, kind, min_score, pf.ticks);
    CORB_LAUNCH(pf.prof, "kfdb_select_kernel", kfdb_select_kernel, dim3(1), dim3(1024), 0, s, d, kind, id, min_score);
    CORB_LAUNCH(pf.prof, "kfdb_scatter_kernel", kfdb_scatter_kernel, dim3(g_sc), dim3(256), 0, s, d, q, nq, n_conn, 0);
}

void corb_launch_kfdb_score(const BowDbDev& d, int a, int na, const int* entries_b, int n, hipStream_t s)
{
    if (n <= 0) return;
    const int g_sc = ((na > 2 ? na : 2) + 255) / 256;
    hipLaunchKernelGGL(kfdb_scatter_kernel, dim3(g_sc), dim3(256), 0, s, d, a, na, 0, 1);
    hipLaunchKernelGGL(kfdb_score_list_kernel, dim3((n + 3) / 4), dim3(256), 0, s, d, entries_b, n);
    hipLaunchKernelGGL(kfdb_scatter_kernel, dim3(g_sc), dim3(256), 0, s, d, a, na, 0, 0);
}

void corb_launch_kfdb_loop_query(const BowDbDev& d, int q, int nq, BowLoopQuery* p, const int* score_entries, int max_score, hipStream_t s)
{
    const int g_sc = ((nq > 2 ? nq : 2) + 255) / 256, g_e = (d.capacity + 3) / 4;
    const BowProfile pf = corb_bow_profile_state();
    CORB_LAUNCH(pf.prof, "kfdb_scatter_kernel", kfdb_scatter_q_kernel, dim3(g_sc), dim3(256), 0, s, d, q, nq, p, 1);
    if (max_score > 0) CORB_LAUNCH(pf.prof, "kfdb_score_list_kernel", kfdb_score_list_q_kernel, dim3((max_score + 3) / 4), dim3(256), 0, s, d, score_entries, p);
    CORB_LAUNCH(pf.prof, "kfdb_min_score_kernel", kfdb_min_score_q_kernel, dim3(1), dim3(64), 0, s, d, p);
    CORB_LAUNCH(pf.prof, "kfdb_count_kernel", kfdb_count_q_kernel, dim3(g_e), dim3(256), 0, s, d, p);
    CORB_LAUNCH(pf.prof, "kfdb_score_kernel", kfdb_score_q_kernel, dim3(g_e), dim3(256), 0, s, d, p);
    CORB_LAUNCH(pf.prof, "kfdb_select_kernel", kfdb_select_q_kernel, dim3(1), dim3(1024), 0, s, d, p);
    CORB_LAUNCH(pf.prof, "kfdb_scatter_kernel", kfdb_scatter_q_kernel, dim3(g_sc), dim3(256), 0, s, d, q, nq, p, 0);
}
