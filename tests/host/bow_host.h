// bow_host.h -- the serial host partner of the device's place recognition, on top of csrc/bow_math.h: TemplatedVocabulary::transform, L1Scoring::score and
// KeyFrameDatabase.cc on entries.  TEST AND MEASUREMENT INFRASTRUCTURE (tests/host/bow_main.cpp, tools/bow_rate.py), not product code.
#pragma once
#include "bow_math.h"

struct BowVecHost { std::vector<uint32_t> word; std::vector<double> value; };
struct BowFeatVecHost { std::vector<uint32_t> node, idx; std::vector<int32_t> off; };

// TemplatedVocabulary::transform(features, v, fv, levelsup) (:1127-1194), serially
inline void bow_transform_host(const BowVocHost& voc, const uint8_t* desc, int n, int levelsup, BowVecHost* bv, BowFeatVecHost* fv, int32_t* feat_word = nullptr, uint32_t* feat_node = nullptr)
{
    const BowVocView v = voc.view();
    std::vector<unsigned long long> kw, kn;
    for (int i = 0; i < n; i++) {
        unsigned long long d[4]; memcpy(d, desc + (size_t)i * 32, 32);
        int w, nid; bow_descend(v, d, levelsup, &w, &nid);
        if (feat_word) feat_word[i] = w;
        if (feat_node) feat_node[i] = (uint32_t)nid;
        if (voc.word_weight[w] > 0) { kw.push_back(((unsigned long long)w << 32) | (unsigned)i); kn.push_back(((unsigned long long)nid << 32) | (unsigned)i); }
    }
    std::sort(kw.begin(), kw.end()); std::sort(kn.begin(), kn.end());
    bv->word.clear(); bv->value.clear(); fv->node.clear(); fv->idx.clear(); fv->off.clear();
    for (size_t p = 0; p < kw.size(); p++) {                            // addWeight: one addition per feature
        const uint32_t w = (uint32_t)(kw[p] >> 32);
        if (p == 0 || w != bv->word.back()) { bv->word.push_back(w); bv->value.push_back(voc.word_weight[w]); }
        else bv->value.back() += voc.word_weight[w];
    }
    double norm = 0.0;
    for (double x : bv->value) norm += fabs(x);                         // BowVector::normalize (:62-84)
    if (norm > 0.0) for (double& x : bv->value) x /= norm;
    for (size_t p = 0; p < kn.size(); p++) {
        const uint32_t nd = (uint32_t)(kn[p] >> 32);
        if (p == 0 || nd != fv->node.back()) { fv->node.push_back(nd); fv->off.push_back((int32_t)p); }
        fv->idx.push_back((uint32_t)kn[p]);
    }
    fv->off.push_back((int32_t)kn.size());
}

// L1Scoring::score (:23-68): the merge walk
inline double bow_score_host(const BowVecHost& a, const BowVecHost& b)
{
    size_t i = 0, j = 0; double s = 0;
    while (i < a.word.size() && j < b.word.size()) {
        if (a.word[i] == b.word[j]) { s += bow_score_term(a.value[i], b.value[j]); i++; j++; }
        else if (a.word[i] < b.word[j]) i = std::lower_bound(a.word.begin(), a.word.end(), b.word[j]) - a.word.begin();
        else j = std::lower_bound(b.word.begin(), b.word.end(), a.word[i]) - b.word.begin();
    }
    return bow_score_finish(s);
}

// KeyFrameDatabase.cc on entries, serially, in the form the kernels use: the inverted file is not kept; an entry's place in lKFsSharingWords is
// (its first word in common with the query, its insertion sequence number) -- query words ascend and a word's list is in insertion order.
struct BowDbHost {
    std::vector<BowVecHost> bow; std::vector<BowKfState> st; std::vector<int> nb; std::vector<char> live; std::vector<unsigned long long> seq; unsigned long long next_seq = 1;
    explicit BowDbHost(int n) : bow(n), st(n, BowKfState{0, 0, 0.f, 0, 0, 0.f}), nb((size_t)n * BOW_NEIGHBOURS, -1), live(n, 0), seq(n, 0) {}
    void set_bow(int e, const BowVecHost& b) { bow[e] = b; st[e] = BowKfState{0, 0, 0.f, 0, 0, 0.f}; }
    void add(int e) { live[e] = 1; seq[e] = next_seq++; }
    void erase(int e) { live[e] = 0; }
    void clear() { std::fill(live.begin(), live.end(), 0); }
    std::vector<int> detect(int kind, int q, unsigned long long id, const std::vector<int>& connected, float min_score)
    {
        struct Cand { unsigned long long first, seq; int e; float si; };
        std::vector<Cand> sharing; const BowVecHost& qb = bow[q];
        for (int e = 0; e < (int)bow.size(); e++) {
            if (!live[e]) continue;
            int common = 0; uint32_t first = 0; const BowVecHost& b = bow[e];
            for (size_t i = 0, j = 0; i < qb.word.size() && j < b.word.size();) {
                if (qb.word[i] == b.word[j]) { if (!common) first = qb.word[i]; common++; i++; j++; } else if (qb.word[i] < b.word[j]) i++; else j++;
            }
            if (!common) continue;
            const bool conn = kind == 0 && std::find(connected.begin(), connected.end(), e) != connected.end();
            if (kind == 0 ? bow_visit_loop(st[e], id, common, conn) : bow_visit_reloc(st[e], id, common)) sharing.push_back({first, seq[e], e, 0.f});
        }
        int max_common = 0;
        for (const Cand& c : sharing) max_common = std::max(max_common, kind == 0 ? st[c.e].loop_words : st[c.e].reloc_words);
        const int min_common = bow_min_common(max_common);
        std::vector<Cand> scored;
        for (Cand c : sharing) {
            if ((kind == 0 ? st[c.e].loop_words : st[c.e].reloc_words) <= min_common) continue;
            c.si = (float)bow_score_host(qb, bow[c.e]);
            if (kind == 0) { st[c.e].loop_score = c.si; if (!(c.si >= min_score)) continue; } else st[c.e].reloc_score = c.si;
            scored.push_back(c);
        }
        std::sort(scored.begin(), scored.end(), [](const Cand& a, const Cand& b) { return a.first != b.first ? a.first < b.first : a.seq < b.seq; });
        float best_acc = kind == 0 ? min_score : 0.f;
        std::vector<float> acc(scored.size()); std::vector<int> best(scored.size());
        for (size_t i = 0; i < scored.size(); i++) {
            bow_accumulate(kind, st.data(), &nb[(size_t)scored[i].e * BOW_NEIGHBOURS], scored[i].e, scored[i].si, id, min_common, &acc[i], &best[i]);
            if (acc[i] > best_acc) best_acc = acc[i];
        }
        const float retain = 0.75f * best_acc;
        std::vector<int> out;
        for (size_t i = 0; i < scored.size(); i++) if (acc[i] > retain && std::find(out.begin(), out.end(), best[i]) == out.end()) out.push_back(best[i]);
        return out;
    }
};
