// corb_bow.cpp -- C-ABI host side of place recognition (include/corb_accel.h, last section): the vocabulary (corb_voc_*), the transform on host arrays and on keyframe
// records (corb_voc_transform, corb_kf_store_compute_bow) and the keyframe database (corb_kfdb_*).  The vocabulary's construction and validation are csrc/bow_math.h's,
// the same text a stand-alone host program runs.  A database's buffers are allocated at create, its launches go to its own stream, and a query is five launches, one
// synchronisation and one read-back through page-locked memory.
#include "bow_internal.h"
#include "store_internal.h"
#include "store_host.h"
#include "corb_workspace.h"
#include <cstring>
#include <vector>
#include <string>
#include <mutex>

#include "host_util.h"

static_assert(sizeof(BowKfState) == sizeof(CorbKfDbState) && sizeof(CorbKfDbState) == 32, "CorbKfDbState is BowKfState, field for field");
static_assert(BOW_MAX_FEATURES == CORB_BOW_MAX_FEATURES, "the LDS limit of bow_build_kernel");

// ---- corb_bow_profile: one process-wide profiler for the launches of this file (event pairs per launch; tick counters of the two in-order sums) ----
static std::mutex g_prof_mu; static CorbProfiler g_prof; static unsigned long long* g_ticks = nullptr; static int g_prof_device = 0;
BowProfile corb_bow_profile_state() { return g_prof.enabled ? BowProfile{&g_prof, g_ticks} : BowProfile{nullptr, nullptr}; }
extern "C" int corb_bow_profile(int enable, int device)
{
    int rc = corb_select_device(device); if (rc) return rc;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (enable && !g_ticks) {
        static DevMem* const mem = new DevMem;                // (never deleted: it goes with the process, not with static destructors behind the HIP runtime's)
        HIPCHK(mem->room(4 * sizeof(unsigned long long))); HIPCHK(hipMemset(mem->as<void>(), 0, 4 * sizeof(unsigned long long)));
        g_ticks = mem->as<unsigned long long>();
    }
    if (enable) g_prof.reserve(256);
    g_prof.enabled = enable != 0; g_prof_device = device;
    return CORB_OK;
}
extern "C" int corb_bow_profile_read(CorbKernelTime* out, int cap, int* n)
{
    if (!n || cap < 0 || (cap > 0 && !out)) { corb_set_error("corb_bow_profile_read: bad argument"); return CORB_ERR_ARG; }
    std::lock_guard<std::mutex> lk(g_prof_mu);
    *n = 0;
    if (!g_ticks) return CORB_OK;
    int rc = corb_select_device(g_prof_device); if (rc) return rc;
    HIPCHK(hipDeviceSynchronize());
    std::vector<CorbKernelTime> acc(g_prof.names.size() + 4);
    for (auto& a : acc) memset(&a, 0, sizeof(a));
    for (size_t i = 0; i < g_prof.names.size(); i++) snprintf(acc[i].name, sizeof(acc[i].name), "%s", g_prof.names[i].c_str());
    for (auto& r : g_prof.recs) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) { acc[r.name_id].total_ms += ms; acc[r.name_id].launches++; }
        g_prof.pool.push_back(r.a); g_prof.pool.push_back(r.b);
    }
    g_prof.recs.clear();
    unsigned long long t[4]; int khz = 0;
    HIPCHK(hipMemcpy(t, g_ticks, sizeof(t), hipMemcpyDeviceToHost)); HIPCHK(hipMemset(g_ticks, 0, sizeof(t)));
    HIPCHK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, g_prof_device));
    static const char* tick_names[4] = {"build: norm sum, one lane", "build: lane 0 in all", "score: ordered sum, waves", "score: waves in all"};
    for (int i = 0; i < 4; i++) { CorbKernelTime& a = acc[g_prof.names.size() + i]; snprintf(a.name, sizeof(a.name), "%s", tick_names[i]); a.total_ms = khz > 0 ? (double)t[i] / khz : 0.0; a.launches = (int64_t)t[i]; }
    *n = (int)acc.size();
    for (int i = 0; i < (int)acc.size() && i < cap; i++) out[i] = acc[i];
    return CORB_OK;
}

template <class T> static hipError_t voc_upload(CorbVoc* v, const T** out, const std::vector<T>& src)
{
    T* p = nullptr; hipError_t e = v->allocs.add(&p, src.size()); if (e != hipSuccess) return e;
    *out = p;
    return src.empty() ? hipSuccess : hipMemcpy(p, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice);
}

int voc_finish(CorbVoc* v, int device, CorbVoc** out, const char* who)
{
    int rc = corb_select_device(device); if (rc) { delete v; return rc; }
    v->device = device;
    const BowVocHost& h = v->host;
    v->dev = BowVocView{h.k, h.L, h.n_nodes, h.n_words, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    if (voc_upload(v, &v->dev.child_first, h.child_first) != hipSuccess || voc_upload(v, &v->dev.child_count, h.child_count) != hipSuccess ||
        voc_upload(v, &v->dev.slot_desc, h.slot_desc) != hipSuccess || voc_upload(v, &v->dev.slot_node, h.slot_node) != hipSuccess ||
        voc_upload(v, &v->dev.node_word, h.node_word) != hipSuccess || voc_upload(v, &v->dev.word_weight, h.word_weight) != hipSuccess) {
        corb_set_error("%s: %d nodes: allocation or upload failed", who, h.n_nodes);
        delete v; return CORB_ERR_HIP;
    }
    *out = v;
    return CORB_OK;
}

extern "C" int corb_voc_create(const CorbVocDesc* d, int device, CorbVoc** out)
{
    if (!d || !out) { corb_set_error("corb_voc_create: bad argument"); return CORB_ERR_ARG; }
    *out = nullptr;
    CorbVoc* v = new CorbVoc();
    const std::string err = bow_voc_build(d->k, d->L, d->scoring, d->weighting, d->n_nodes, d->parent, d->is_leaf, d->descriptor, d->weight, &v->host);
    if (!err.empty()) { corb_set_error("corb_voc_create: %s", err.c_str()); delete v; return CORB_ERR_ARG; }
    return voc_finish(v, device, out, "corb_voc_create");
}
extern "C" int corb_voc_load_text(const char* path, int device, CorbVoc** out)
{
    if (!path || !out) { corb_set_error("corb_voc_load_text: bad argument"); return CORB_ERR_ARG; }
    *out = nullptr;
    CorbVoc* v = new CorbVoc();
    const std::string err = bow_voc_load_text(path, &v->host);
    if (!err.empty()) { corb_set_error("corb_voc_load_text: %s", err.c_str()); delete v; return CORB_ERR_ARG; }
    return voc_finish(v, device, out, "corb_voc_load_text");
}
extern "C" void corb_voc_destroy(CorbVoc* v) { handle_destroy(v); }
extern "C" int corb_voc_info(const CorbVoc* v, int32_t* k, int32_t* L, int32_t* n_nodes, int32_t* n_words)
{
    if (!v) { corb_set_error("corb_voc_info: bad argument"); return CORB_ERR_ARG; }
    if (k) *k = v->host.k;
    if (L) *L = v->host.L;
    if (n_nodes) *n_nodes = v->host.n_nodes;
    if (n_words) *n_words = v->host.n_words;
    return CORB_OK;
}

extern "C" int corb_voc_transform(CorbVoc* v, const uint8_t* desc, const int32_t* offset, int n_sets, int levelsup, uint32_t* bow_word, double* bow_value, int32_t* bow_count,
                                  uint32_t* fv_node_id, int32_t* fv_offset, uint32_t* fv_idx, int32_t* fv_n_nodes, int32_t* feat_word, uint32_t* feat_node)
{
    const char* who = "corb_voc_transform";
    if (!v || n_sets < 0 || (n_sets > 0 && (!offset || !bow_count || !fv_n_nodes || !fv_offset))) { corb_set_error("%s: bad argument", who); return CORB_ERR_ARG; }
    if (n_sets == 0) return CORB_OK;
    if (n_sets > BOW_MAX_SETS) { corb_set_error("%s: %d descriptor sets; a call takes at most %d", who, n_sets, BOW_MAX_SETS); return CORB_ERR_ARG; }
    if (offset[0] != 0) { corb_set_error("%s: offset[0] != 0", who); return CORB_ERR_ARG; }
    int max_n = 0;
    for (int s = 0; s < n_sets; s++) {
        const int n = offset[s + 1] - offset[s];
        if (n < 0 || n > BOW_MAX_FEATURES) { corb_set_error("%s: set %d has %d features; a set holds 0 .. %d", who, s, n, BOW_MAX_FEATURES); return CORB_ERR_ARG; }
        max_n = std::max(max_n, n);
    }
    const int total = offset[n_sets];
    if (total > 0 && (!desc || !bow_word || !bow_value || !fv_node_id || !fv_idx)) { corb_set_error("%s: NULL array", who); return CORB_ERR_ARG; }
    int rc = corb_select_device(v->device); if (rc) return rc;
    CorbScratch pool(0);
    unsigned long long* d_desc; uint32_t *d_word, *d_node, *d_idx, *d_fnode, *d_copy; double* d_val; int32_t *d_off, *d_fword, *d_counts, *d_bc, *d_nn; BowSetDev* d_sets;
    HIPCHK(pool.alloc(&d_desc, (size_t)total * 4 + 4)); HIPCHK(pool.h2d(d_desc, desc, (size_t)total * 32));
    HIPCHK(pool.alloc(&d_word, (size_t)total)); HIPCHK(pool.alloc(&d_val, (size_t)total)); HIPCHK(pool.alloc(&d_node, (size_t)total)); HIPCHK(pool.alloc(&d_idx, (size_t)total));
    HIPCHK(pool.alloc(&d_off, (size_t)total + n_sets)); HIPCHK(pool.alloc(&d_fword, (size_t)total)); HIPCHK(pool.alloc(&d_fnode, (size_t)total)); HIPCHK(pool.alloc(&d_copy, (size_t)total));
    HIPCHK(pool.alloc(&d_counts, (size_t)n_sets * 3)); HIPCHK(pool.alloc(&d_bc, (size_t)n_sets)); HIPCHK(pool.alloc(&d_nn, (size_t)n_sets));
    static thread_local std::vector<BowSetDev> sets; sets.resize(n_sets);
    for (int s = 0; s < n_sets; s++) {
        const int o = offset[s], n = offset[s + 1] - o;
        sets[s] = BowSetDev{d_desc + (size_t)o * 4, n, o, n, d_word + o, d_val + o, d_bc + s, d_node + o, d_off + o + s, d_idx + o, d_nn + s, d_copy + o, d_counts + 3 * s};
    }
    HIPCHK(pool.upload(&d_sets, sets));
    int attr = 0;
    corb_launch_bow_transform(v->dev, d_sets, n_sets, max_n, levelsup, d_fword, d_fnode, pool.stream, &attr);
    if (attr) { corb_set_error("%s: the sort kernel's LDS opt-in failed: %s", who, hipGetErrorString((hipError_t)attr)); return CORB_ERR_HIP; }
    HIPCHK(hipGetLastError());
    HIPCHK(pool.d2h(bow_word, d_word, (size_t)total * 4)); HIPCHK(pool.d2h(bow_value, d_val, (size_t)total * 8)); HIPCHK(pool.d2h(bow_count, d_bc, (size_t)n_sets * 4));
    HIPCHK(pool.d2h(fv_node_id, d_node, (size_t)total * 4)); HIPCHK(pool.d2h(fv_offset, d_off, ((size_t)total + n_sets) * 4)); HIPCHK(pool.d2h(fv_idx, d_idx, (size_t)total * 4));
    HIPCHK(pool.d2h(fv_n_nodes, d_nn, (size_t)n_sets * 4));
    if (feat_word) HIPCHK(pool.d2h(feat_word, d_fword, (size_t)total * 4));
    if (feat_node) HIPCHK(pool.d2h(feat_node, d_fnode, (size_t)total * 4));
    HIPCHK(pool.fetch_finish());
    return CORB_OK;
}

// ---------------------------------------------------------------- keyframe database ----------------------------------------------------------------
// (struct CorbKfDb: bow_internal.h)
template <class T> static hipError_t db_alloc(CorbKfDb* db, T** out, size_t n, int fill)
{
    hipError_t e = db->allocs.add(out, n); if (e != hipSuccess) return e;
    return hipMemset(*out, fill, std::max(n, (size_t)1) * sizeof(T));
}

extern "C" void corb_kfdb_destroy(CorbKfDb* db) { handle_destroy(db); }

extern "C" int corb_kfdb_create(CorbVoc* voc, int capacity, int max_words, CorbKfDb** out)
{
    if (!voc || !out || capacity < 1 || capacity > (1 << 24) || max_words < 1 || max_words > BOW_MAX_FEATURES) {
        corb_set_error("corb_kfdb_create: bad argument (1 <= capacity_entries <= 2^24, 1 <= max_words <= %d)", BOW_MAX_FEATURES); return CORB_ERR_ARG;
    }
    *out = nullptr;
    int rc = corb_select_device(voc->device); if (rc) return rc;
    CorbKfDb* db = new CorbKfDb();
    db->device = voc->device; db->voc = voc; db->n_words.assign(capacity, -1); db->live.assign(capacity, 0);
    BowDbDev& d = db->d; d.capacity = capacity; d.max_words = max_words; d.n_vocab_words = voc->host.n_words;
    size_t P = 1; while (P < (size_t)capacity) P <<= 1;
    const size_t c = capacity;
    const bool ok = db_alloc(db, &d.words, c * max_words, 0) == hipSuccess && db_alloc(db, &d.values, c * max_words, 0) == hipSuccess && db_alloc(db, &d.n_words, c, 0xFF) == hipSuccess &&
        db_alloc(db, &d.live, c, 0) == hipSuccess && db_alloc(db, &d.seq, c, 0) == hipSuccess && db_alloc(db, &d.st, c, 0) == hipSuccess && db_alloc(db, &d.nb, c * BOW_NEIGHBOURS, 0xFF) == hipSuccess &&
        db_alloc(db, &d.dense, (size_t)d.n_vocab_words, 0) == hipSuccess && db_alloc(db, &d.conn, c, 0) == hipSuccess && db_alloc(db, &d.conn_list, c, 0) == hipSuccess &&
        db_alloc(db, &d.ctr, 2, 0) == hipSuccess && db_alloc(db, &d.pushed, c, 0) == hipSuccess && db_alloc(db, &d.first_word, c, 0) == hipSuccess &&
        db_alloc(db, &d.skey, P, 0) == hipSuccess && db_alloc(db, &d.sent, P, 0) == hipSuccess && db_alloc(db, &d.acc, c, 0) == hipSuccess && db_alloc(db, &d.best, c, 0) == hipSuccess &&
        db_alloc(db, &d.first_pos, c, 0x7F) == hipSuccess && db_alloc(db, &d.out, c + 1, 0) == hipSuccess && db_alloc(db, &d.score_out, c, 0) == hipSuccess &&
        db->stream.create() == hipSuccess && db->pinned.room((2 * c + 2) * 4) == hipSuccess && db->pinned_score.room(c * 8) == hipSuccess;
    if (!ok) { corb_set_error("corb_kfdb_create: %d entries x %d words: allocation failed", capacity, max_words); handle_destroy(db); return CORB_ERR_HIP; }
    { const hipError_t e = hipDeviceSynchronize(); if (e != hipSuccess) { corb_set_error("corb_kfdb_create: %s", hipGetErrorString(e)); handle_destroy(db); return CORB_ERR_HIP; } }
    *out = db;
    return CORB_OK;
}

static int db_entry(CorbKfDb* db, int entry, const char* who)
{
    if (!db || entry < 0 || entry >= db->d.capacity) { corb_set_error("%s: bad database / entry", who); return CORB_ERR_ARG; }
    return corb_select_device(db->device);
}

extern "C" int corb_kfdb_set_bow(CorbKfDb* db, int entry, const uint32_t* word, const double* value, int n)
{
    const char* who = "corb_kfdb_set_bow";
    int rc = db_entry(db, entry, who); if (rc) return rc;
    if (n < 0 || n > db->d.max_words || (n > 0 && (!word || !value))) { corb_set_error("%s: %d words for a database of %d per entry", who, n, db->d.max_words); return CORB_ERR_ARG; }
    for (int i = 0; i < n; i++) if (word[i] >= (uint32_t)db->d.n_vocab_words || (i && word[i] <= word[i - 1])) { corb_set_error("%s: words must ascend and lie below the vocabulary's %d", who, db->d.n_vocab_words); return CORB_ERR_ARG; }
    for (int i = 0; i < n; i++) if (!(value[i] > 0)) { corb_set_error("%s: value[%d] is not above 0 (a BowVector holds the words that are present; the kernels mark presence by the value)", who, i); return CORB_ERR_ARG; }
    std::lock_guard<std::mutex> lk(db->mu);
    if (db->live[entry]) { corb_set_error("%s: entry %d is in the database; erase it first", who, entry); return CORB_ERR_ARG; }
    const BowKfState zero{0, 0, 0.f, 0, 0, 0.f};
    if (n) { HIPCHK(hipMemcpyAsync(db->d.words + (size_t)entry * db->d.max_words, word, (size_t)n * 4, hipMemcpyHostToDevice, db->stream));
             HIPCHK(hipMemcpyAsync(db->d.values + (size_t)entry * db->d.max_words, value, (size_t)n * 8, hipMemcpyHostToDevice, db->stream)); }
    HIPCHK(hipMemcpyAsync(db->d.n_words + entry, &n, 4, hipMemcpyHostToDevice, db->stream));
    HIPCHK(hipMemcpyAsync(db->d.st + entry, &zero, sizeof(zero), hipMemcpyHostToDevice, db->stream));
    HIPCHK(hipStreamSynchronize(db->stream));
    db->n_words[entry] = n;
    return CORB_OK;
}
extern "C" int corb_kfdb_get_bow(CorbKfDb* db, int entry, uint32_t* word, double* value, int cap, int* n)
{
    const char* who = "corb_kfdb_get_bow";
    int rc = db_entry(db, entry, who); if (rc) return rc;
    if (!n) { corb_set_error("%s: bad argument", who); return CORB_ERR_ARG; }
    std::lock_guard<std::mutex> lk(db->mu);
    if (db->n_words[entry] < 0) { corb_set_error("%s: entry %d has no BowVector", who, entry); return CORB_ERR_ARG; }
    *n = db->n_words[entry];
    if (*n > cap && (word || value)) { corb_set_error("%s: entry %d has %d words, room for %d", who, entry, *n, cap); return CORB_ERR_CAPACITY; }
    if (word && *n) HIPCHK(hipMemcpyAsync(word, db->d.words + (size_t)entry * db->d.max_words, (size_t)*n * 4, hipMemcpyDeviceToHost, db->stream));
    if (value && *n) HIPCHK(hipMemcpyAsync(value, db->d.values + (size_t)entry * db->d.max_words, (size_t)*n * 8, hipMemcpyDeviceToHost, db->stream));
    HIPCHK(hipStreamSynchronize(db->stream));
    return CORB_OK;
}
static int db_set_live(CorbKfDb* db, int entry, bool on)
{
    const unsigned char f = on ? 1 : 0;
    HIPCHK(hipMemcpyAsync(db->d.live + entry, &f, 1, hipMemcpyHostToDevice, db->stream));
    if (on) { const uint32_t q = db->next_seq++; HIPCHK(hipMemcpyAsync(db->d.seq + entry, &q, 4, hipMemcpyHostToDevice, db->stream)); }
    HIPCHK(hipStreamSynchronize(db->stream));
    db->live[entry] = (char)f;
    return CORB_OK;
}
extern "C" int corb_kfdb_add(CorbKfDb* db, int entry)
{
    int rc = db_entry(db, entry, "corb_kfdb_add"); if (rc) return rc;
    std::lock_guard<std::mutex> lk(db->mu);
    if (db->live[entry] || db->n_words[entry] < 0) { corb_set_error("corb_kfdb_add: entry %d %s", entry, db->live[entry] ? "is in the database already" : "has no BowVector"); return CORB_ERR_ARG; }
    if (db->next_seq == 0xFFFFFFFFu) { corb_set_error("corb_kfdb_add: 2^32 adds; clear the database"); return CORB_ERR_OVERFLOW; }
    return db_set_live(db, entry, true);
}
extern "C" int corb_kfdb_erase(CorbKfDb* db, int entry)
{
    int rc = db_entry(db, entry, "corb_kfdb_erase"); if (rc) return rc;
    std::lock_guard<std::mutex> lk(db->mu);
    if (!db->live[entry]) { corb_set_error("corb_kfdb_erase: entry %d is not in the database", entry); return CORB_ERR_ARG; }
    return db_set_live(db, entry, false);
}
extern "C" int corb_kfdb_clear(CorbKfDb* db)
{
    int rc = db_entry(db, 0, "corb_kfdb_clear"); if (rc) return rc;
    std::lock_guard<std::mutex> lk(db->mu);
    HIPCHK(hipMemsetAsync(db->d.live, 0, (size_t)db->d.capacity, db->stream));
    HIPCHK(hipStreamSynchronize(db->stream));
    std::fill(db->live.begin(), db->live.end(), 0); db->next_seq = 1;      // (an empty inverted file: sequence numbers only order the entries that are in it)
    return CORB_OK;
}
extern "C" int corb_kfdb_set_neighbours(CorbKfDb* db, const int32_t* entries, int n, const int32_t* nb)
{
    const char* who = "corb_kfdb_set_neighbours";
    int rc = db_entry(db, 0, who); if (rc) return rc;
    if (n < 0 || (n > 0 && (!entries || !nb))) { corb_set_error("%s: bad argument", who); return CORB_ERR_ARG; }
    for (int i = 0; i < n; i++) {
        if (entries[i] < 0 || entries[i] >= db->d.capacity) { corb_set_error("%s: entry %d is outside the database", who, entries[i]); return CORB_ERR_ARG; }
        for (int j = 0; j < BOW_NEIGHBOURS; j++) if (nb[i * BOW_NEIGHBOURS + j] < -1 || nb[i * BOW_NEIGHBOURS + j] >= db->d.capacity) { corb_set_error("%s: neighbour %d of entry %d is outside the database", who, j, entries[i]); return CORB_ERR_ARG; }
    }
    std::lock_guard<std::mutex> lk(db->mu);
    for (int i = 0; i < n; i++) HIPCHK(hipMemcpyAsync(db->d.nb + (size_t)entries[i] * BOW_NEIGHBOURS, nb + (size_t)i * BOW_NEIGHBOURS, BOW_NEIGHBOURS * 4, hipMemcpyHostToDevice, db->stream));
    HIPCHK(hipStreamSynchronize(db->stream));
    return CORB_OK;
}
extern "C" int corb_kfdb_get_state(CorbKfDb* db, int first, int n, CorbKfDbState* out)
{
    int rc = db_entry(db, 0, "corb_kfdb_get_state"); if (rc) return rc;
    if (first < 0 || n < 0 || first + n > db->d.capacity || (n > 0 && !out)) { corb_set_error("corb_kfdb_get_state: bad argument"); return CORB_ERR_ARG; }
    std::lock_guard<std::mutex> lk(db->mu);
    if (n) HIPCHK(hipMemcpyAsync(out, db->d.st + first, (size_t)n * sizeof(BowKfState), hipMemcpyDeviceToHost, db->stream));
    HIPCHK(hipStreamSynchronize(db->stream));
    return CORB_OK;
}

extern "C" int corb_kfdb_score(CorbKfDb* db, int a, const int32_t* entries_b, int n, double* score)
{
    const char* who = "corb_kfdb_score";
    int rc = db_entry(db, a, who); if (rc) return rc;
    if (n < 0 || n > db->d.capacity || (n > 0 && (!entries_b || !score))) { corb_set_error("%s: bad argument (at most capacity_entries scores per call)", who); return CORB_ERR_ARG; }
    std::lock_guard<std::mutex> lk(db->mu);
    if (db->n_words[a] < 0) { corb_set_error("%s: entry %d has no BowVector", who, a); return CORB_ERR_ARG; }
    for (int i = 0; i < n; i++) if (entries_b[i] < 0 || entries_b[i] >= db->d.capacity || db->n_words[entries_b[i]] < 0) { corb_set_error("%s: entries_b[%d] is outside the database or has no BowVector", who, i); return CORB_ERR_ARG; }
    if (n == 0) return CORB_OK;
    memcpy(db->pinned.as<int32_t>(), entries_b, (size_t)n * 4);
    HIPCHK(hipMemcpyAsync(db->d.conn_list, db->pinned.as<int32_t>(), (size_t)n * 4, hipMemcpyHostToDevice, db->stream));
    corb_launch_kfdb_score(db->d, a, db->n_words[a], db->d.conn_list, n, db->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(db->pinned_score.as<double>(), db->d.score_out, (size_t)n * 8, hipMemcpyDeviceToHost, db->stream));
    HIPCHK(hipStreamSynchronize(db->stream));
    memcpy(score, db->pinned_score.as<double>(), (size_t)n * 8);
    return CORB_OK;
}

extern "C" int corb_kfdb_detect(CorbKfDb* db, int kind, int q, uint64_t query_id, const int32_t* connected, int n_connected, float min_score, int32_t* out, int cap, int* n)
{
    const char* who = "corb_kfdb_detect";
    int rc = db_entry(db, q, who); if (rc) return rc;
    if (kind < 0 || kind > 2 || !n || cap < 0 || (cap > 0 && !out)) { corb_set_error("%s: bad argument (kind 0 loop, 1 relocalisation, 2 map fusion)", who); return CORB_ERR_ARG; }
    if (kind != 0) n_connected = 0;
    if (n_connected < 0 || n_connected > db->d.capacity || (n_connected > 0 && !connected)) { corb_set_error("%s: bad connected list", who); return CORB_ERR_ARG; }
    for (int i = 0; i < n_connected; i++) if (connected[i] < 0 || connected[i] >= db->d.capacity) { corb_set_error("%s: connected[%d] is outside the database", who, i); return CORB_ERR_ARG; }
    if (kind == 0 && !(min_score == min_score)) { corb_set_error("%s: min_score is NaN", who); return CORB_ERR_ARG; }
    std::lock_guard<std::mutex> lk(db->mu);
    if (db->n_words[q] < 0) { corb_set_error("%s: the query entry %d has no BowVector", who, q); return CORB_ERR_ARG; }
    *n = 0;
    const int c = db->d.capacity, want = std::min(cap, c);
    if (n_connected) { memcpy(db->pinned.as<int32_t>(), connected, (size_t)n_connected * 4); HIPCHK(hipMemcpyAsync(db->d.conn_list, db->pinned.as<int32_t>(), (size_t)n_connected * 4, hipMemcpyHostToDevice, db->stream)); }
    corb_launch_kfdb_detect(db->d, kind, q, db->n_words[q], query_id, n_connected, min_score, db->stream);
    HIPCHK(hipGetLastError());
    int32_t* back = db->pinned.as<int32_t>() + c;
    HIPCHK(hipMemcpyAsync(back, db->d.out, ((size_t)want + 1) * 4, hipMemcpyDeviceToHost, db->stream));
    HIPCHK(hipStreamSynchronize(db->stream));
    *n = back[0];
    if (back[0] > cap) { corb_set_error("%s: %d candidates, room for %d", who, back[0], cap); return CORB_ERR_OVERFLOW; }
    if (back[0]) memcpy(out, back + 1, (size_t)back[0] * 4);
    return CORB_OK;
}

// ---------------------------------------------------------------- ComputeBoW on records ----------------------------------------------------------------
extern "C" int corb_kf_store_compute_bow(CorbKfStore* s, const int32_t* slots, int n_slots, CorbVoc* voc, int levelsup, CorbKfDb* db, const int32_t* entries)
{
    const char* who = "corb_kf_store_compute_bow";
    if (!s || !voc || n_slots < 0 || (n_slots > 0 && !slots) || (db && n_slots > 0 && !entries)) { corb_set_error("%s: bad argument", who); return CORB_ERR_ARG; }
    if (n_slots > BOW_MAX_SETS) { corb_set_error("%s: %d slots; a call takes at most %d", who, n_slots, BOW_MAX_SETS); return CORB_ERR_ARG; }
    if (s->F > BOW_MAX_FEATURES) { corb_set_error("%s: the store holds up to %d features per keyframe; the transform sorts at most %d in one workgroup's LDS", who, s->F, BOW_MAX_FEATURES); return CORB_ERR_ARG; }
    if (s->device != voc->device || (db && db->voc != voc)) { corb_set_error("%s: store, vocabulary and database must share a device, and the database its vocabulary", who); return CORB_ERR_ARG; }
    for (int i = 0; i < n_slots; i++) {
        if (slots[i] < 0 || slots[i] >= s->capacity) { corb_set_error("%s: slot %d is outside the store", who, slots[i]); return CORB_ERR_ARG; }
        for (int j = 0; j < i; j++) if (slots[j] == slots[i] || (db && entries[j] == entries[i])) { corb_set_error("%s: a slot or an entry is listed twice", who); return CORB_ERR_ARG; }
        if (db && (entries[i] < 0 || entries[i] >= db->d.capacity)) { corb_set_error("%s: entry %d is outside the database", who, entries[i]); return CORB_ERR_ARG; }
    }
    if (n_slots == 0) return CORB_OK;
    int rc = corb_select_device(s->device); if (rc) return rc;
    std::unique_lock<std::mutex> lkd; if (db) lkd = std::unique_lock<std::mutex>(db->mu);
    if (db) for (int i = 0; i < n_slots; i++) if (db->live[entries[i]]) { corb_set_error("%s: entry %d is in the database; erase it first", who, entries[i]); return CORB_ERR_ARG; }
    std::lock_guard<std::mutex> lk(s->mu);
    int total = 0, max_n = 0;
    static thread_local std::vector<BowSetDev> sets; sets.resize(n_slots);
    for (int i = 0; i < n_slots; i++) {                                 // feature counts from the host mirror (read from the header once after a device-side fill)
        CorbKfStore::Host& h = s->host[slots[i]];
        if (!h.header_valid) {
            int hdr[4];
            HIPCHK(hipMemcpyAsync(hdr, s->rec(slots[i]), sizeof(hdr), hipMemcpyDeviceToHost, s->stream)); HIPCHK(hipStreamSynchronize(s->stream));
            if (hdr[0] < 0 || hdr[0] > s->F) { corb_set_error("%s: slot %d holds a corrupt record", who, slots[i]); return CORB_ERR_ARG; }
            h.n = hdr[0]; memcpy(&h.id, &hdr[2], 8);
        }
        sets[i].n = h.n; sets[i].feat_off = total; total += h.n; max_n = std::max(max_n, h.n);
    }
    HIPCHK(hipStreamSynchronize(s->stream));                            // pending fills of the records
    if (db) HIPCHK(hipStreamSynchronize(db->stream));
    CorbScratch pool(0);
    int32_t *d_fword, *d_counts, *d_dummy; uint32_t *d_fnode, *d_copy, *d_sw = nullptr; double* d_sv = nullptr; BowSetDev* d_sets;
    HIPCHK(pool.alloc(&d_fword, (size_t)total)); HIPCHK(pool.alloc(&d_fnode, (size_t)total)); HIPCHK(pool.alloc(&d_copy, (size_t)total));
    HIPCHK(pool.alloc(&d_counts, (size_t)n_slots * 3)); HIPCHK(pool.alloc(&d_dummy, (size_t)n_slots));
    if (!db) { HIPCHK(pool.alloc(&d_sw, (size_t)total)); HIPCHK(pool.alloc(&d_sv, (size_t)total)); }
    for (int i = 0; i < n_slots; i++) {
        char* r = s->rec(slots[i]); BowSetDev& t = sets[i];
        t.desc = (const unsigned long long*)(r + s->L.desc);
        if (db) { const size_t at = (size_t)entries[i] * db->d.max_words; t.max_words = db->d.max_words; t.bow_word = db->d.words + at; t.bow_value = db->d.values + at; t.bow_count = db->d.n_words + entries[i]; }
        else { t.max_words = t.n; t.bow_word = d_sw + t.feat_off; t.bow_value = d_sv + t.feat_off; t.bow_count = d_dummy + i; }
        t.fv_node = (uint32_t*)(r + s->L.fv_node); t.fv_off = (int32_t*)(r + s->L.fv_off); t.fv_idx = (uint32_t*)(r + s->L.fv_idx); t.fv_n_nodes = (int32_t*)(r + 4);
        t.node_copy = d_copy + t.feat_off; t.counts = d_counts + 3 * i;
    }
    HIPCHK(pool.upload(&d_sets, sets));
    if (db) for (int i = 0; i < n_slots; i++) HIPCHK(hipMemsetAsync(db->d.st + entries[i], 0, sizeof(BowKfState), pool.stream));      // a new keyframe: its six fields are zero
    int attr = 0;
    corb_launch_bow_transform(voc->dev, d_sets, n_slots, max_n, levelsup, d_fword, d_fnode, pool.stream, &attr);
    if (attr) { corb_set_error("%s: the sort kernel's LDS opt-in failed: %s", who, hipGetErrorString((hipError_t)attr)); return CORB_ERR_HIP; }
    HIPCHK(hipGetLastError());
    static thread_local std::vector<int32_t> counts; static thread_local std::vector<uint32_t> nodes;
    counts.resize((size_t)n_slots * 3); nodes.resize((size_t)total + 1);
    HIPCHK(pool.d2h(counts.data(), d_counts, counts.size() * 4)); HIPCHK(pool.d2h(nodes.data(), d_copy, (size_t)total * 4));      // the one small read-back
    HIPCHK(pool.fetch_finish());
    int overflow = -1;
    for (int i = 0; i < n_slots; i++) {
        CorbKfStore::Host& h = s->host[slots[i]];
        h.n_nodes = counts[3 * i + 1]; h.node_id.assign(nodes.begin() + sets[i].feat_off, nodes.begin() + sets[i].feat_off + h.n_nodes); h.header_valid = true;
        if (db) { db->n_words[entries[i]] = counts[3 * i + 2] ? -1 : counts[3 * i]; if (counts[3 * i + 2] && overflow < 0) overflow = i; }
    }
    if (overflow >= 0) { corb_set_error("%s: slot %d: %d words, the database holds %d per entry", who, slots[overflow], counts[3 * overflow], db->d.max_words); return CORB_ERR_CAPACITY; }
    return CORB_OK;
}
