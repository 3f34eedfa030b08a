// bow_math.h -- the arithmetic of place recognition, stated once for the kernels (bow_kernels.hip), the C-ABI host code (corb_bow.cpp) and a stand-alone host
// program (tests/host/bow_main.cpp with the serial transform and database of tests/host/bow_host.h): DBoW2's vocabulary descent (C/Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1218-1259), the BowVector's repeated addition and L1
// normalisation (BowVector.cpp:34-84), the L1 score (ScoringObject.cpp:23-68) and the per-keyframe rules of KeyFrameDatabase.cc:73-401.  tests/dbow_reference.py is the
// definition; DESIGN.md section 2 lists the readings.  No fused operations (-ffp-contract=off); sums run in the definition's order.
#pragma once
#include <stdint.h>
#include <math.h>
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define BOW_HD __host__ __device__ inline
#else
#define BOW_HD inline
#endif

#define BOW_MAX_K 20            // the text loader's bounds (TemplatedVocabulary.h:1359)
#define BOW_MAX_L 10
#define BOW_NEIGHBOURS 10       // GetBestCovisibilityKeyFrames(10) (KeyFrameDatabase.cc:146)
#define BOW_MAX_FEATURES 8192   // features per set: the sort of one set lives in the LDS of one workgroup, 16 bytes per feature slot (128 KiB of 160)

// The tree as the descent reads it.  Node 0 is the root.  The children of node i are the slots child_first[i] .. child_first[i] + child_count[i], in child order, with their
// descriptors contiguous: a level of the descent is one coalesced read.
struct BowVocView {
    int k, L, n_nodes, n_words;
    const int* child_first;                 // [n_nodes]
    const int* child_count;                 // [n_nodes]  0: the node ends the descent (isLeaf(), :1254)
    const unsigned long long* slot_desc;    // [n_nodes - 1][4]
    const int* slot_node;                   // [n_nodes - 1]
    const int* node_word;                   // [n_nodes]  word id of a leaf, -1 otherwise
    const double* word_weight;              // [n_words]
};

BOW_HD int bow_popc64(unsigned long long v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll(v);
#else
    return __builtin_popcountll(v);
#endif
}
BOW_HD int bow_hamming(const unsigned long long* a, const unsigned long long* b)
{
    return bow_popc64(a[0] ^ b[0]) + bow_popc64(a[1] ^ b[1]) + bow_popc64(a[2] ^ b[2]) + bow_popc64(a[3] ^ b[3]);
}
// the order the minimum is taken in: distance first, then the child's position -- strict `<` in child order (:1244) keeps the first minimum
BOW_HD unsigned bow_child_key(int dist, int child) { return ((unsigned)dist << 8) | (unsigned)child; }

// one feature, serially (the kernel spreads the children of a level over a group of lanes and takes the minimum of bow_child_key)
BOW_HD void bow_descend(const BowVocView& v, const unsigned long long* d, int levelsup, int* word, int* nid_out)
{
    const int nid_level = v.L - levelsup;
    int nid = nid_level <= 0 ? 0 : -1, node = 0, level = 0;
    do {
        ++level;
        const int first = v.child_first[node], cnt = v.child_count[node];
        unsigned best = 0xFFFFFFFFu;
        for (int c = 0; c < cnt; c++) { const unsigned key = bow_child_key(bow_hamming(d, v.slot_desc + (size_t)(first + c) * 4), c); if (key < best) best = key; }
        node = v.slot_node[first + (int)(best & 0xFF)];
        if (level == nid_level) nid = node;
    } while (v.child_count[node] > 0);
    *word = v.node_word[node];
    *nid_out = nid < 0 ? node : nid;        // a leaf above the recording level: the leaf itself (the source leaves nid unset)
}

// one common word's term of L1Scoring::score (:41)
BOW_HD double bow_score_term(double vi, double wi) { return fabs(vi - wi) - fabs(vi) - fabs(wi); }
BOW_HD double bow_score_finish(double sum) { return -sum / 2.0; }                          // :65
BOW_HD int bow_min_common(int max_common) { return (int)((float)max_common * 0.8f); }      // KeyFrameDatabase.cc:116

// per-keyframe fields of KeyFrameDatabase.cc, all 0 for a new keyframe
struct BowKfState { unsigned long long loop_query; int loop_words; float loop_score; unsigned long long reloc_query; int reloc_words; float reloc_score; };

// What the walk over the query's words (:82-100, :197-212, :304-319) leaves in a keyframe that shares `common` > 0 words with the query; returns whether the keyframe
// entered lKFsSharingWords.  A connected keyframe of the loop query never takes the id, so every visit resets its counter: it ends at 1.
BOW_HD bool bow_visit_loop(BowKfState& s, unsigned long long id, int common, bool connected)
{
    if (s.loop_query != id) {
        if (connected) { s.loop_words = 1; return false; }
        s.loop_query = id; s.loop_words = common; return true;
    }
    s.loop_words += common;
    return false;
}
BOW_HD bool bow_visit_reloc(BowKfState& s, unsigned long long id, int common)
{
    if (s.reloc_query != id) { s.reloc_query = id; s.reloc_words = common; return true; }
    s.reloc_words += common;
    return false;
}
// the covisibility accumulation of one scored keyframe (:143-165, :251-274): nb = its neighbours' entries (-1 padded).  counts(e2) says whether neighbour e2 takes
// part for this query and score_of(e2) is the score it holds then -- for the relocalisation / map-fusion kinds that is whatever mRelocScore the last query that
// scored it left there (a neighbour that shares a word with the query but was not scored for it adds a stale score; the reference does).
template <class Counts, class ScoreOf> BOW_HD void bow_accumulate_by(const int* nb, int entry, float si, Counts counts, ScoreOf score_of, float* acc_out, int* best_out)
{
    float best_score = si, acc = si; int best = entry;
    for (int j = 0; j < BOW_NEIGHBOURS; j++) {
        const int e2 = nb[j];
        if (e2 < 0 || !counts(e2)) continue;
        const float s2 = score_of(e2);
        acc += s2; if (s2 > best_score) { best = e2; best_score = s2; }
    }
    *acc_out = acc; *best_out = best;
}
BOW_HD void bow_accumulate(int kind, const BowKfState* st, const int* nb, int entry, float si, unsigned long long id, int min_common, float* acc_out, int* best_out)
{
    if (kind == 0) bow_accumulate_by(nb, entry, si, [=](int e2) { return st[e2].loop_query == id && st[e2].loop_words > min_common; }, [=](int e2) { return st[e2].loop_score; }, acc_out, best_out);
    else bow_accumulate_by(nb, entry, si, [=](int e2) { return st[e2].reloc_query == id; }, [=](int e2) { return st[e2].reloc_score; }, acc_out, best_out);
}

// ============================ host side: the vocabulary's construction (corb_bow.cpp and the host program share it) ============================
#include <vector>
#include <string>
#include <algorithm>
#include <fstream>
#include <sstream>
#include <cstdio>
#include <cstring>

struct BowVocHost {
    int k = 0, L = 0, n_nodes = 0, n_words = 0;
    std::vector<int> child_first, child_count, slot_node, node_word;
    std::vector<unsigned long long> slot_desc;
    std::vector<double> word_weight;
    std::vector<double> node_weight;        // [n_nodes] as given, inner nodes too (corb_voc_get returns them)
    BowVocView view() const { return BowVocView{k, L, n_nodes, n_words, child_first.data(), child_count.data(), slot_desc.data(), slot_node.data(), node_word.data(), word_weight.data()}; }
};

// flat arrays (node ids 1 .. n in array order) -> BowVocHost; an empty string, or what is wrong with the input
inline std::string bow_voc_build(int k, int L, int scoring, int weighting, int n, const int32_t* parent, const int32_t* is_leaf, const uint8_t* desc, const double* weight, BowVocHost* out)
{
    char msg[160];
    if (k < 0 || k > BOW_MAX_K || L < 1 || L > BOW_MAX_L) return "k must be in [0, 20] and L in [1, 10]";
    if (scoring != 0 || weighting != 0) return "only L1_NORM scoring (0) with TF_IDF weighting (0) is supported";
    if (n < 1 || !parent || !is_leaf || !desc || !weight) return "empty vocabulary";
    BowVocHost& v = *out; v = BowVocHost(); v.k = k; v.L = L; v.n_nodes = n + 1;
    v.child_first.assign(n + 1, 0); v.child_count.assign(n + 1, 0); v.node_word.assign(n + 1, -1); v.node_weight.assign(n + 1, 0.0);
    for (int i = 1; i <= n; i++) {
        const int p = parent[i - 1];
        v.node_weight[i] = weight[i - 1];
        if (p < 0 || p >= i) { snprintf(msg, sizeof msg, "node %d: parent %d is not before it", i, p); return msg; }
        if (v.node_word[p] >= 0) { snprintf(msg, sizeof msg, "node %d: its parent %d is a leaf", i, p); return msg; }
        if (++v.child_count[p] > k) { snprintf(msg, sizeof msg, "node %d has more than k = %d children", p, k); return msg; }
        if (is_leaf[i - 1] > 0) { v.node_word[i] = v.n_words++; v.word_weight.push_back(weight[i - 1]); }
    }
    for (int i = 1; i <= n; i++) if (v.node_word[i] < 0 && v.child_count[i] == 0) { snprintf(msg, sizeof msg, "node %d is neither a leaf nor a parent", i); return msg; }
    for (int i = 0, at = 0; i <= n; i++) { v.child_first[i] = at; at += v.child_count[i]; }
    std::vector<int> fill(n + 1, 0);
    v.slot_node.assign(n, 0); v.slot_desc.assign((size_t)n * 4, 0);
    for (int i = 1; i <= n; i++) {                                      // children keep line order (:1392)
        const int p = parent[i - 1], s = v.child_first[p] + fill[p]++;
        v.slot_node[s] = i; memcpy(&v.slot_desc[(size_t)s * 4], desc + (size_t)(i - 1) * 32, 32);
    }
    return "";
}

// the text format of loadFromTextFile (:1338-1424); blank lines make no node
inline std::string bow_voc_load_text(const char* path, BowVocHost* out)
{
    std::ifstream f(path);
    if (!f) return std::string("cannot open ") + path;
    std::string s; std::getline(f, s);
    std::stringstream ss(s); int k = -1, L = -1, n1 = -1, n2 = -1; ss >> k >> L >> n1 >> n2;
    if (!ss) return "the first line is not `k L scoring weighting`";
    std::vector<int32_t> parent, leaf; std::vector<uint8_t> desc; std::vector<double> weight;
    int line = 1;
    while (std::getline(f, s)) {
        line++;
        if (s.find_first_not_of(" \t\r\n") == std::string::npos) continue;
        std::stringstream sn(s); int pid, is_leaf; sn >> pid >> is_leaf;
        int b[32]; for (int i = 0; i < 32; i++) sn >> b[i];
        double w; sn >> w;
        if (!sn) { char msg[96]; snprintf(msg, sizeof msg, "line %d is not `parent isLeaf d0 .. d31 weight`", line); return msg; }
        for (int i = 0; i < 32; i++) { if (b[i] < 0 || b[i] > 255) return "a descriptor byte is outside [0, 255]"; desc.push_back((uint8_t)b[i]); }
        parent.push_back(pid); leaf.push_back(is_leaf); weight.push_back(w);
    }
    return bow_voc_build(k, L, n1, n2, (int)parent.size(), parent.data(), leaf.data(), desc.data(), weight.data(), out);
}
