// fusion_kernels.hip -- map-fusion detection for a whole submap on gfx950 (include/corb_map_fusion.h; definition: tests/fusion_reference.py on tests/dbow_reference.py).
// corb_kfdb_detect_batch: the single query scatters its BowVector into a dense array over all words; many such arrays do not fit, so a pass over n queries works on
// the sorted word lists, and what the single calls do one after the other to an entry's fields is replayed by one lane per entry that walks the queries in order:
//   fusion_common_kernel  : one workgroup per (query, 64 entries): the query's words in LDS (4 bytes a word: the database's limit of 8192 words is 32 KiB of the 160),
//                           one wavefront per entry, lanes on the entry's words, a binary search each, ballots for the common count and the first common word
//   fusion_walk_kernel    : one lane per entry walks the queries in order carrying mnRelocQuery / mnRelocWords (bow_visit_reloc): pushed, the word count and
//                           "the id matches" per (query, entry); maxCommonWords per query by an integer atomic maximum (the order the atomics land in cannot matter)
//   fusion_score_kernel   : one wavefront per (query, entry) that entered the list with more than minCommonWords: the L1 score, its terms added in ascending word
//                           order exactly as kfdb_score_kernel adds them (bow_device.h)
//   fusion_seen_kernel    : the walk once more, carrying mRelocScore: the score as query i's accumulation reads it (a neighbour that shares a word with the query
//                           but was not scored for it adds what an earlier query left), and the final fields
//   fusion_select_kernel  : one workgroup per query: what kfdb_select_kernel does for one -- bitonic sort of the kept entries by (first word, sequence number),
//                           bow_accumulate_by on the values above, the maximum, the 0.75 threshold, first appearance per best keyframe, ordered compaction
//   fusion_append_kernel  : the pass's candidates behind those of the passes before it, with the offsets
// corb_search_by_bow_slots_batch: fusion_match_kernel, one wavefront per (pair, common vocabulary node) with the node walk of bow_match_kernel (match_device.h);
// histogram, bins and count per pair; fusion_rot_kernel, one workgroup per pair.  corb_map_fusion_candidates_store: fusion_rows_kernel (kept and the ids' offsets by
// one workgroup's scan) and fusion_ids_kernel (one workgroup per kept row gathers the candidate record's map-point ids).
// No floating-point atomics: every float sum runs in the definition's order.  No scalar memory writes, no device-side printf / assert.
#include "fusion_internal.h"
#include "bow_device.h"
#include "match_device.h"

namespace {

// position of `key` in the ascending w[0 .. n), -1 if it is not there
__device__ __forceinline__ int fusion_find(const uint32_t* w, int n, uint32_t key)
{
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (w[mid] < key) lo = mid + 1; else hi = mid; }
    return lo < n && w[lo] == key ? lo : -1;
}

__global__ __launch_bounds__(256) void fusion_common_kernel(BowDbDev d, FusionDetectDev f)
{
    __shared__ uint32_t qw[BOW_MAX_FEATURES];
    const int q = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int qe = f.q_entry[q], nq = min(d.n_words[qe], BOW_MAX_FEATURES);
    const uint32_t* src = d.words + (size_t)qe * d.max_words;
    for (int i = tid; i < nq; i += 256) qw[i] = src[i];
    __syncthreads();
    for (int k = 0; k < 16; k++) {
        const int e = blockIdx.x * 64 + wave * 16 + k;              // (wave-uniform)
        if (e >= d.capacity) break;
        int common = 0; uint32_t first = 0;
        const int nw = d.n_words[e];
        if (d.live[e] && nw > 0) common = bow_wave_common(d.words + (size_t)e * d.max_words, min(nw, d.max_words), lane, [&](uint32_t w) { return fusion_find(qw, nq, w) >= 0; }, &first);
        if (lane == 0) { const size_t at = (size_t)q * d.capacity + e; f.common[at] = common; f.first_word[at] = first; }
    }
}

__global__ __launch_bounds__(256) void fusion_walk_kernel(BowDbDev d, FusionDetectDev f)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= d.capacity) return;
    BowKfState st = d.st[e];
    for (int q = 0; q < f.n; q++) {
        const size_t at = (size_t)q * d.capacity + e;
        const int common = f.common[at];
        const unsigned long long id = f.q_id[q];
        const bool pushed = common > 0 && bow_visit_reloc(st, id, common);
        f.pushed[at] = pushed ? 1 : 0; f.words[at] = st.reloc_words; f.id_match[at] = st.reloc_query == id ? 1 : 0;
        if (pushed) atomicMax(&f.max_common[q], st.reloc_words);
    }
    d.st[e].reloc_query = st.reloc_query; d.st[e].reloc_words = st.reloc_words;
}

__global__ __launch_bounds__(256) void fusion_score_kernel(BowDbDev d, FusionDetectDev f)
{
    const int q = blockIdx.y, e = blockIdx.x * 4 + (int)threadIdx.x / 64, lane = threadIdx.x & 63;
    if (e >= d.capacity) return;
    const size_t at = (size_t)q * d.capacity + e;
    const bool go = f.pushed[at] && f.words[at] > bow_min_common(f.max_common[q]);
    float si = 0.f;
    if (go) {
        const int qe = f.q_entry[q], nq = min(d.n_words[qe], d.max_words);
        const uint32_t* qw = d.words + (size_t)qe * d.max_words; const double* qv = d.values + (size_t)qe * d.max_words;
        unsigned long long unused = 0;
        si = (float)bow_wave_score<false>(d.words + (size_t)e * d.max_words, d.values + (size_t)e * d.max_words, min(d.n_words[e], d.max_words), lane,
                                          [=](uint32_t w) { const int j = fusion_find(qw, nq, w); return j >= 0 ? qv[j] : 0.0; }, unused);
    }
    if (lane == 0) { f.scored[at] = go ? 1 : 0; if (go) f.score[at] = si; }
}

__global__ __launch_bounds__(256) void fusion_seen_kernel(BowDbDev d, FusionDetectDev f)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= d.capacity) return;
    float cur = d.st[e].reloc_score;
    for (int q = 0; q < f.n; q++) {
        const size_t at = (size_t)q * d.capacity + e;
        if (f.scored[at]) cur = f.score[at];
        f.seen[at] = cur;
    }
    d.st[e].reloc_score = cur;
}

__global__ __launch_bounds__(1024) void fusion_select_kernel(BowDbDev d, FusionDetectDev f)
{
    __shared__ float red[1024]; __shared__ int wave_count[16]; __shared__ int s_S;
    const int q = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
    const size_t base = (size_t)q * d.capacity;
    unsigned long long* skey = f.skey + (size_t)q * f.P; int* sent = f.sent + (size_t)q * f.P;
    float* acc_a = f.acc + base; int* best_a = f.best + base; int* first_pos = f.first_pos + base; int* row = f.row + base;
    if (tid == 0) s_S = 0;
    __syncthreads();
    for (int e = tid; e < d.capacity; e += T)
        if (f.scored[base + e]) { const int at = atomicAdd(&s_S, 1); skey[at] = ((unsigned long long)f.first_word[base + e] << 32) | d.seq[e]; sent[at] = e; }      // (the sort below fixes the order: sequence numbers of live entries differ)
    __syncthreads();
    const int S = s_S;
    if (S == 0) { if (tid == 0) f.n_row[q] = 0; return; }
    int P = 1; while (P < S) P <<= 1;
    for (int i = S + tid; i < P; i += T) skey[i] = ~0ull;
    __syncthreads();
    bow_bitonic(skey, P, [sent](int a, int b) { const int t = sent[a]; sent[a] = sent[b]; sent[b] = t; });
    const unsigned char* idm = f.id_match + base; const float* seen = f.seen + base;
    float best = 0.f;                                           // bestAccScore (:248)
    for (int i = tid; i < S; i += T) {
        const int e = sent[i];
        float acc; int b;
        bow_accumulate_by(d.nb + (size_t)e * BOW_NEIGHBOURS, e, f.score[base + e], [=](int e2) { return idm[e2] != 0; }, [=](int e2) { return seen[e2]; }, &acc, &b);
        acc_a[i] = acc; best_a[i] = b;
        if (acc > best) best = acc;
    }
    red[tid] = best;
    __syncthreads();
    for (int o = T >> 1; o > 0; o >>= 1) { if (tid < o && red[tid + o] > red[tid]) red[tid] = red[tid + o]; __syncthreads(); }
    const float retain = 0.75f * red[0];
    for (int i = tid; i < S; i += T) if (acc_a[i] > retain) atomicMin(&first_pos[best_a[i]], i);
    __syncthreads();
    int n_out = 0;
    for (int b0 = 0; b0 < S; b0 += T) {                         // candidates in list order, a best keyframe at its first appearance only
        const int i = b0 + tid;
        const bool keep = i < S && acc_a[i] > retain && first_pos[best_a[i]] == i;
        const unsigned long long m = __ballot(keep);
        if ((tid & 63) == 0) wave_count[tid >> 6] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < 16; w++) { const int c = w < (T >> 6) ? wave_count[w] : 0; if (w < (tid >> 6)) before += c; total += c; }
        if (keep) row[n_out + before + __popcll(m & ((1ull << (tid & 63)) - 1ull))] = best_a[i];
        n_out += total;
        __syncthreads();
    }
    if (tid == 0) f.n_row[q] = n_out;
}

__global__ __launch_bounds__(256) void fusion_append_kernel(FusionDetectDev f, int capacity, int q0, int* out_offset, int* out_cand, int cap, int* total)
{
    __shared__ int run;
    const int tid = threadIdx.x;
    if (tid == 0) run = total[0];
    __syncthreads();
    for (int q = 0; q < f.n; q++) {
        const int r = run, n = f.n_row[q];
        const int* row = f.row + (size_t)q * capacity;
        if (tid == 0) out_offset[q0 + q] = r;
        for (int i = tid; i < n; i += 256) if ((long long)r + i < cap) out_cand[r + i] = row[i];
        __syncthreads();
        if (tid == 0) run = r + n;
        __syncthreads();
    }
    if (tid == 0) { total[0] = run; out_offset[q0 + f.n] = run; }
}

// ---- SearchByBoW for many pairs ----
__global__ __launch_bounds__(256) void fusion_match_kernel(FusionMatchDev m)
{
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= m.n_list) return;
    const int p = m.list[3 * i], na = m.list[3 * i + 1], nb = m.list[3 * i + 2];
    const char* ra = m.base_a + (size_t)m.pair[3 * p] * m.bytes_a; const char* rb = m.base_b + (size_t)m.pair[3 * p + 1] * m.bytes_b;
    const RecLayout La(m.Fa), Lb(m.Fb);
    CorbBowDev d;
    d.variant = m.variant; d.check_ori = m.check_ori; d.n_pairs = 1; d.nnratio = m.nnratio; d.pair_a = nullptr; d.pair_b = nullptr;
    d.off1 = (const int*)(ra + La.fv_off); d.idx1 = (const int*)(ra + La.fv_idx); d.off2 = (const int*)(rb + Lb.fv_off); d.idx2 = (const int*)(rb + Lb.fv_idx);
    d.desc1 = (const unsigned long long*)(ra + La.desc); d.desc2 = (const unsigned long long*)(rb + Lb.desc);
    d.angle1 = (const float*)(ra + La.angle); d.angle2 = (const float*)(rb + Lb.angle);
    d.valid1 = (const uint8_t*)(ra + La.flags); d.valid2 = (const uint8_t*)(rb + Lb.flags);       // (valid2 is read for variant 1 only: the Frame side of variant 0 has no validity test, :212)
    d.match = m.match + (size_t)p * m.stride; d.bin = m.bin + (size_t)p * m.stride; d.hist = m.hist + (size_t)p * CORB_HISTO_LENGTH; d.n_matches = m.n_matches + p;
    bow_match_node(d, na, nb, lane);
}

__global__ __launch_bounds__(256) void fusion_rot_kernel(FusionMatchDev m)
{
    __shared__ int ind[3];
    const int p = blockIdx.x;
    rot_finalize(m.match + (size_t)p * m.stride, m.bin + (size_t)p * m.stride, min(m.pair[3 * p + 2], m.stride), m.hist + (size_t)p * CORB_HISTO_LENGTH, m.n_matches + p, 1, ind);
}

// ---- rows of corb_map_fusion_candidates_store ----
__global__ __launch_bounds__(256) void fusion_rows_kernel(FusionRowsDev r)
{
    __shared__ long long part[256];
    const int tid = threadIdx.x, per = (r.n_rows + 255) / 256, r0 = min(tid * per, r.n_rows), r1 = min(r0 + per, r.n_rows);
    long long sum = 0;
    for (int i = r0; i < r1; i++) {
        CorbFusionRow& row = r.rows[i];
        const int pair = r.row_pair[i], nm = pair >= 0 ? r.n_matches[pair] : 0;
        bool kept = false;
        if (row.slot >= 0) { const KfHeader* h = reinterpret_cast<const KfHeader*>(r.base_g + (size_t)row.slot * r.bytes_g); kept = h->n > 0 && !(h->m.flags & CORB_KF_BAD) && nm >= r.min_matches; }
        row.n_matches = nm; row.kept = kept ? 1 : 0;
        if (kept) sum += r.q_features[row.query];
    }
    part[tid] = sum;
    __syncthreads();
    if (tid == 0) { long long run = 0; for (int t = 0; t < 256; t++) { const long long s = part[t]; part[t] = run; run += s; } *r.n_ids = run; }
    __syncthreads();
    long long off = part[tid];
    for (int i = r0; i < r1; i++) {
        CorbFusionRow& row = r.rows[i];
        if (row.kept) { row.ids_offset = off; off += r.q_features[row.query]; } else row.ids_offset = -1;
    }
}

__global__ __launch_bounds__(256) void fusion_ids_kernel(FusionRowsDev r)
{
    const CorbFusionRow row = r.rows[blockIdx.x];
    if (!row.kept) return;
    const int nq = r.q_features[row.query];
    if (row.ids_offset + nq > r.cap_ids) return;                // (the call returns CORB_ERR_OVERFLOW with the room needed)
    const int* mrow = r.match + (size_t)r.row_pair[blockIdx.x] * r.stride;
    const RecLayout L(r.Fg);
    const unsigned long long* mp = reinterpret_cast<const unsigned long long*>(r.base_g + (size_t)row.slot * r.bytes_g + L.mp_id);
    for (int iF = threadIdx.x; iF < nq; iF += 256) { const int m = mrow[iF]; r.ids[row.ids_offset + iF] = m >= 0 && m < r.Fg ? mp[m] : CORB_NO_MAP_POINT; }
}

}  // namespace

void corb_launch_fusion_detect(const BowDbDev& d, const FusionDetectDev& f, int q0, int* out_offset, int* out_cand, int cap, int* total, hipStream_t s)
{
    if (f.n <= 0) return;
    const BowProfile pf = corb_bow_profile_state();
    const int c = d.capacity;
    CORB_LAUNCH(pf.prof, "fusion_common_kernel", fusion_common_kernel, dim3((c + 63) / 64, f.n), dim3(256), 0, s, d, f);
    CORB_LAUNCH(pf.prof, "fusion_walk_kernel", fusion_walk_kernel, dim3((c + 255) / 256), dim3(256), 0, s, d, f);
    CORB_LAUNCH(pf.prof, "fusion_score_kernel", fusion_score_kernel, dim3((c + 3) / 4, f.n), dim3(256), 0, s, d, f);
    CORB_LAUNCH(pf.prof, "fusion_seen_kernel", fusion_seen_kernel, dim3((c + 255) / 256), dim3(256), 0, s, d, f);
    CORB_LAUNCH(pf.prof, "fusion_select_kernel", fusion_select_kernel, dim3(f.n), dim3(1024), 0, s, d, f);
    CORB_LAUNCH(pf.prof, "fusion_append_kernel", fusion_append_kernel, dim3(1), dim3(256), 0, s, f, c, q0, out_offset, out_cand, cap, total);
}

void corb_launch_fusion_match(const FusionMatchDev& m, hipStream_t s)
{
    if (m.n_list > 0) hipLaunchKernelGGL(fusion_match_kernel, dim3((m.n_list + 3) / 4), dim3(256), 0, s, m);
    if (m.check_ori && m.n_pairs > 0) hipLaunchKernelGGL(fusion_rot_kernel, dim3(m.n_pairs), dim3(256), 0, s, m);
}

void corb_launch_fusion_rows(const FusionRowsDev& r, hipStream_t s)
{
    if (r.n_rows <= 0) return;
    hipLaunchKernelGGL(fusion_rows_kernel, dim3(1), dim3(256), 0, s, r);
    hipLaunchKernelGGL(fusion_ids_kernel, dim3(r.n_rows), dim3(256), 0, s, r);
}
