// bow_main.cpp -- csrc/bow_math.h and tests/host/bow_host.h compiled for the host: reads a binary case file (a vocabulary, descriptor sets to transform, pairs of them to score, a scripted
// keyframe-database session) and prints every result as integers and IEEE bit patterns in hex.  tests/test_bow_math_host.py holds the output byte-equal to
// tests/dbow_reference.py.  Stand-alone (no GPU, no library): the place for a sanitizer build (g++ -fsanitize=address,undefined).  With a third argument R it repeats the
// transforms and the session R times and prints the seconds per pass of each: the serial partner of tools/bow_rate.py.
//   file: i32 k, L, scoring, weighting, n | parent[n] i32 | is_leaf[n] i32 | desc[n][32] | weight[n] f64
//         i32 n_sets | per set: i32 levelsup, n, desc[n][32]        i32 n_pairs | per pair: i32 a, b (sets)
//         i32 n_entries, levelsup, n_ops | per op: i32 code ...      0 set_bow e n desc   1 add e   2 erase e   3 clear   4 nb e nb[10]   5 query kind e id(u64) min_score(f32) nc conn[nc]
//                                                                    6 set_bow e n word[n] u32 value[n] f64 (a BowVector as given)
#include "bow_host.h"
#include <chrono>
#include <cstdlib>

#ifdef BOW_HOST_SHARED
// the same serial code as a shared object, so that a measuring process can run it in-process (tools/bow_rate.py): g++ -O3 -shared -fPIC -DBOW_HOST_SHARED
struct BowHostCtx { BowVocHost voc; BowDbHost* db = nullptr; BowVecHost bv; BowFeatVecHost fv; };
extern "C" {
void* bow_host_create(int k, int L, int n, const int32_t* parent, const int32_t* leaf, const uint8_t* desc, const double* weight)
{ BowHostCtx* c = new BowHostCtx(); if (!bow_voc_build(k, L, 0, 0, n, parent, leaf, desc, weight, &c->voc).empty()) { delete c; return nullptr; } return c; }
void bow_host_destroy(void* h) { BowHostCtx* c = (BowHostCtx*)h; if (c) { delete c->db; delete c; } }
// FeatureVector of one set in CorbFeatVec form; returns the number of nodes (arrays of n, n + 1, n entries)
int bow_host_transform(void* h, const uint8_t* desc, int n, int levelsup, uint32_t* node, int32_t* off, uint32_t* idx)
{
    BowHostCtx* c = (BowHostCtx*)h; bow_transform_host(c->voc, desc, n, levelsup, &c->bv, &c->fv);
    std::copy(c->fv.node.begin(), c->fv.node.end(), node); std::copy(c->fv.off.begin(), c->fv.off.end(), off); std::copy(c->fv.idx.begin(), c->fv.idx.end(), idx);
    return (int)c->fv.node.size();
}
void bow_host_db_create(void* h, int n) { BowHostCtx* c = (BowHostCtx*)h; delete c->db; c->db = new BowDbHost(n); }
void bow_host_db_set_add(void* h, int e, const uint32_t* w, const double* v, int n, int add)
{ BowHostCtx* c = (BowHostCtx*)h; BowVecHost b; b.word.assign(w, w + n); b.value.assign(v, v + n); c->db->set_bow(e, b); if (add) c->db->add(e); }
int bow_host_db_detect(void* h, int kind, int q, unsigned long long id, float min_score, int* out, int cap)
{ BowHostCtx* c = (BowHostCtx*)h; const std::vector<int> r = c->db->detect(kind, q, id, std::vector<int>(), min_score); for (int i = 0; i < (int)r.size() && i < cap; i++) out[i] = r[i]; return (int)r.size(); }
}
#else
static std::vector<char> buf; static size_t at = 0;
template <class T> static T rd() { T v; if (at + sizeof(T) > buf.size()) { fprintf(stderr, "truncated case file\n"); exit(2); } memcpy(&v, &buf[at], sizeof(T)); at += sizeof(T); return v; }
template <class T> static std::vector<T> rdv(size_t n) { std::vector<T> v(n); if (at + n * sizeof(T) > buf.size()) { fprintf(stderr, "truncated case file\n"); exit(2); } if (n) memcpy(v.data(), &buf[at], n * sizeof(T)); at += n * sizeof(T); return v; }
static unsigned long long bits(double v) { unsigned long long b; memcpy(&b, &v, 8); return b; }
static unsigned bits(float v) { unsigned b; memcpy(&b, &v, 4); return b; }

struct Set { int levelsup, n; std::vector<uint8_t> desc; BowVecHost bv; BowFeatVecHost fv; std::vector<int32_t> fw; std::vector<uint32_t> fn; };
struct Op { int code, e, kind, n; unsigned long long id; float min_score; std::vector<uint8_t> desc; std::vector<int> list; BowVecHost bow; };

int main(int argc, char** argv)
{
    if (argc < 3) { fprintf(stderr, "usage: bow_main cases.bin out.txt [repeats]\n"); return 1; }
    { std::ifstream f(argv[1], std::ios::binary); if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 1; } buf.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>()); }
    const int repeats = argc > 3 ? atoi(argv[3]) : 0;
    const int k = rd<int32_t>(), L = rd<int32_t>(), sc = rd<int32_t>(), wt = rd<int32_t>(), n = rd<int32_t>();
    if (n < 0) return 2;
    const auto parent = rdv<int32_t>(n), leaf = rdv<int32_t>(n); const auto desc = rdv<uint8_t>((size_t)n * 32); const auto weight = rdv<double>(n);
    BowVocHost voc;
    const std::string err = bow_voc_build(k, L, sc, wt, n, parent.data(), leaf.data(), desc.data(), weight.data(), &voc);
    if (!err.empty()) { fprintf(stderr, "%s\n", err.c_str()); return 3; }
    std::vector<Set> sets(rd<int32_t>());
    for (Set& s : sets) { s.levelsup = rd<int32_t>(); s.n = rd<int32_t>(); s.desc = rdv<uint8_t>((size_t)s.n * 32); s.fw.resize(s.n); s.fn.resize(s.n); }
    std::vector<std::pair<int, int>> pairs(rd<int32_t>());
    for (auto& p : pairs) { p.first = rd<int32_t>(); p.second = rd<int32_t>(); if (p.first < 0 || p.second < 0 || p.first >= (int)sets.size() || p.second >= (int)sets.size()) return 2; }
    const int n_entries = rd<int32_t>(), s_levelsup = rd<int32_t>(); std::vector<Op> ops(rd<int32_t>());
    for (Op& o : ops) {
        o.code = rd<int32_t>(); o.e = o.code == 3 ? 0 : rd<int32_t>();
        if (o.code != 5 && (o.e < 0 || o.e >= n_entries)) return 2;
        if (o.code == 0) { o.n = rd<int32_t>(); o.desc = rdv<uint8_t>((size_t)o.n * 32); }
        else if (o.code == 6) { o.n = rd<int32_t>(); o.bow.word = rdv<uint32_t>(o.n); o.bow.value = rdv<double>(o.n); }
        else if (o.code == 4) { const auto nb = rdv<int32_t>(BOW_NEIGHBOURS); o.list.assign(nb.begin(), nb.end()); for (int j : o.list) if (j < -1 || j >= n_entries) return 2; }
        else if (o.code == 5) { o.kind = o.e; o.e = rd<int32_t>(); if (o.e < 0 || o.e >= n_entries) return 2; o.id = rd<uint64_t>(); o.min_score = rd<float>(); const int nc = rd<int32_t>(); const auto c = rdv<int32_t>(nc); o.list.assign(c.begin(), c.end()); }
    }
    FILE* out = fopen(argv[2], "w"); if (!out) return 1;
    auto run_sets = [&]() { for (Set& s : sets) bow_transform_host(voc, s.desc.data(), s.n, s.levelsup, &s.bv, &s.fv, s.fw.data(), s.fn.data()); };
    std::vector<double> query_seconds;
    auto run_session = [&](FILE* o) {
        BowDbHost db(n_entries); BowVecHost bv; BowFeatVecHost fv;
        for (const Op& op : ops) {
            if (op.code == 0) { bow_transform_host(voc, op.desc.data(), op.n, s_levelsup, &bv, &fv); db.set_bow(op.e, bv); }
            else if (op.code == 6) db.set_bow(op.e, op.bow);
            else if (op.code == 1) db.add(op.e);
            else if (op.code == 2) db.erase(op.e);
            else if (op.code == 3) db.clear();
            else if (op.code == 4) std::copy(op.list.begin(), op.list.end(), db.nb.begin() + (size_t)op.e * BOW_NEIGHBOURS);
            else if (op.code == 5) {
                const auto q0 = std::chrono::steady_clock::now();
                const std::vector<int> c = db.detect(op.kind, op.e, op.id, op.list, op.min_score);
                if (!o) { query_seconds.push_back(std::chrono::duration<double>(std::chrono::steady_clock::now() - q0).count()); continue; }
                fprintf(o, "Q %zu", c.size()); for (int e : c) fprintf(o, " %d", e); fprintf(o, "\n");
                for (const BowKfState& s : db.st) fprintf(o, "st %llu %d %08x %llu %d %08x\n", s.loop_query, s.loop_words, bits(s.loop_score), s.reloc_query, s.reloc_words, bits(s.reloc_score));
            }
        }
    };
    run_sets();
    for (const Set& s : sets) {
        fprintf(out, "T %zu %zu\nw", s.bv.word.size(), s.fv.node.size());
        for (uint32_t w : s.bv.word) fprintf(out, " %u", w);
        fprintf(out, "\nv"); for (double v : s.bv.value) fprintf(out, " %016llx", bits(v));
        fprintf(out, "\nn"); for (uint32_t v : s.fv.node) fprintf(out, " %u", v);
        fprintf(out, "\no"); for (int32_t v : s.fv.off) fprintf(out, " %d", v);
        fprintf(out, "\ni"); for (uint32_t v : s.fv.idx) fprintf(out, " %u", v);
        fprintf(out, "\nfw"); for (int32_t v : s.fw) fprintf(out, " %d", v);
        fprintf(out, "\nfn"); for (uint32_t v : s.fn) fprintf(out, " %u", v);
        fprintf(out, "\n");
    }
    for (const auto& p : pairs) fprintf(out, "S %016llx\n", bits(bow_score_host(sets[p.first].bv, sets[p.second].bv)));
    run_session(out);
    fclose(out);
    if (repeats > 0) {
        auto t0 = std::chrono::steady_clock::now();
        for (int r = 0; r < repeats; r++) run_sets();
        auto t1 = std::chrono::steady_clock::now();
        for (int r = 0; r < repeats; r++) run_session(nullptr);
        auto t2 = std::chrono::steady_clock::now();
        printf("query_seconds"); for (double q : query_seconds) printf(" %.9f", q); printf("\n");      // every query of every repeat, in order
        printf("seconds_per_pass transform %.9f session %.9f\n", std::chrono::duration<double>(t1 - t0).count() / repeats, std::chrono::duration<double>(t2 - t1).count() / repeats);
    }
    return 0;
}
#endif
