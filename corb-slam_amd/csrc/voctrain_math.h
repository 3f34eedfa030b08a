// voctrain_math.h -- the arithmetic of vocabulary training, stated once for the kernels (voctrain_kernels.hip), the C-ABI host code (corb_voctrain.cpp) and a stand-alone
// host program (tests/host/voctrain_main.cpp): DBoW2's TemplatedVocabulary::create (C/Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:558-996) with FORB::meanValue
// (FORB.cpp:28-77).  tests/voctrain_reference.py is the definition, recursive and depth first; DESIGN.md section 2 lists the readings.  Here a tree is trained level by
// level (breadth first, as the device does) and its nodes are then renumbered into the source's order.  Everything is integer except the comparison against cut_d, which
// is two double roundings (-ffp-contract=off).
#pragma once
#include "bow_math.h"

#define VT_MAX_LEVELS BOW_MAX_L
#define VT_WORDS 4              // a descriptor is 4 x u64; bit b of the mean depends on bit b of the members only, so the counters may index bits in any fixed order

BOW_HD unsigned long long vt_mix(unsigned long long z)         // the splitmix64 finaliser
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
// draw j of the k-means node `key`: [0, 2^31 - 1], glibc's RAND_MAX
BOW_HD unsigned vt_draw(unsigned long long seed, unsigned long long key, unsigned j) { return (unsigned)(vt_mix(seed + 0x9E3779B97F4A7C15ULL * (key * 256ULL + j + 1ULL)) >> 33); }
BOW_HD unsigned long long vt_child_key(unsigned long long key, unsigned long long pow21_depth, int c) { return key + (unsigned long long)(c + 1) * pow21_depth; }
BOW_HD int vt_first_index(unsigned r, int n) { return (int)(((double)r / 2147483648.0) * (double)n); }                 // RandomInt(0, n - 1)
BOW_HD double vt_cut(unsigned r, unsigned long long dist_sum) { const double u = (double)r / 2147483647.0; return u * (double)dist_sum; }       // RandomValue<double>(0, dist_sum)
// cut_d of a seeding round: redrawn while it is 0.0 (:887-891); *j is the node's draw counter.  dist_sum > 0, so a draw with r > 0 ends the loop.
BOW_HD double vt_next_cut(unsigned long long seed, unsigned long long key, unsigned* j, unsigned long long dist_sum)
{
    double cut;
    do { cut = vt_cut(vt_draw(seed, key, *j), dist_sum); ++*j; } while (cut == 0.0);
    return cut;
}
BOW_HD bool vt_reached(unsigned long long prefix, double cut) { return (double)prefix >= cut; }                          // :897, prefix < 2^53 is exact
BOW_HD int vt_majority_threshold(int n) { return n / 2 + n % 2; }                                                       // FORB.cpp:65; n == 1 gives 1: the member is copied

// ============================ host side: training level by level ============================
struct VtStats {
    int nodes = 0, words = 0, kmeans_nodes = 0, trivial_nodes = 0, short_nodes = 0, max_iterations_seen = 0, capped_nodes = 0, empty_cluster_events = 0;
    int level_nodes[VT_MAX_LEVELS] = {0}, level_max_iterations[VT_MAX_LEVELS] = {0};
};
struct VtFlat { std::vector<int32_t> parent, is_leaf; std::vector<uint8_t> descriptor; std::vector<double> weight; };

inline std::string vt_check_arguments(int k, int L, int max_iterations, long long n_features)
{
    if (k < 2 || k > BOW_MAX_K) return "k must be in [2, 20]";
    if (L < 1 || L > BOW_MAX_L) return "L must be in [1, 10]";
    if (max_iterations < 1) return "max_iterations must be at least 1";
    if (n_features < 1) return "no training feature";
    return "";
}

// The tree in level order, as host and device build it.  A node's children are consecutive.
struct VtTree {
    std::vector<int> parent, child_first, child_count;      // node 0 is the root
    std::vector<unsigned long long> desc;                   // [nodes][4]
    int add(int p, const unsigned long long* d)
    {
        parent.push_back(p); child_first.push_back(0); child_count.push_back(0); desc.insert(desc.end(), d, d + VT_WORDS);
        return (int)parent.size() - 1;
    }
};
// one active node of a level: its descriptors are perm[begin .. begin + n), in original relative order
struct VtSegment { int node, begin, n; unsigned long long key; };

// level order -> the source's ids (:786-818: a node's clusters get consecutive ids when it finishes, then the recursion goes child by child)
inline void vt_renumber(const VtTree& t, int k, int L, VtFlat* out)
{
    const int n = (int)t.parent.size();
    std::vector<int> id(n, 0), order; order.reserve(n);
    std::vector<int> stack{0};
    int next = 1;
    while (!stack.empty()) {
        const int p = stack.back(); stack.pop_back();
        for (int c = 0; c < t.child_count[p]; c++) { id[t.child_first[p] + c] = next++; order.push_back(t.child_first[p] + c); }
        for (int c = t.child_count[p] - 1; c >= 0; c--) if (t.child_count[t.child_first[p] + c] > 0) stack.push_back(t.child_first[p] + c);
    }
    out->parent.assign(n - 1, 0); out->is_leaf.assign(n - 1, 0); out->descriptor.assign((size_t)(n - 1) * 32, 0); out->weight.assign(n - 1, 0.0);
    for (int b : order) {
        const int i = id[b] - 1;
        out->parent[i] = id[t.parent[b]]; out->is_leaf[i] = t.child_count[b] == 0; memcpy(&out->descriptor[(size_t)i * 32], &t.desc[(size_t)b * VT_WORDS], 32);
    }
}

// setNodeWeights (:962-992) from Ni; `words` is the finished vocabulary
inline void vt_set_weights(BowVocHost& words, const std::vector<int>& ni, int n_docs, VtFlat* flat)
{
    words.word_weight.assign(words.n_words, 0.0);
    for (int i = 1; i < words.n_nodes; i++) {
        const int w = words.node_word[i];
        if (w >= 0 && ni[w] > 0) { words.word_weight[w] = log((double)n_docs / (double)ni[w]); words.node_weight[i] = flat->weight[i - 1] = words.word_weight[w]; }
    }
}

// Ni on the host: the transform descent of every feature of every image
inline void vt_count_images(const BowVocHost& words, const unsigned long long* desc, const int32_t* offset, int n_images, std::vector<int>* ni)
{
    ni->assign(words.n_words, 0);
    std::vector<int> seen(words.n_words, -1);
    const BowVocView v = words.view();
    for (int s = 0; s < n_images; s++)
        for (int f = offset[s]; f < offset[s + 1]; f++) {
            int w, nid; bow_descend(v, desc + (size_t)f * VT_WORDS, 0, &w, &nid);
            if (seen[w] != s) { seen[w] = s; (*ni)[w]++; }
        }
}

// k-means of one node on the host: centres [<= k][4], the association of its n descriptors; returns the number of centres
inline int vt_node_kmeans(const unsigned long long* desc, const int* idx, int n, int k, unsigned long long seed, unsigned long long key, int max_iterations,
                          std::vector<unsigned long long>& centres, std::vector<int>& which, int* iterations, int* capped, int* empties)
{
    auto D = [&](int i) { return desc + (size_t)idx[i] * VT_WORDS; };
    centres.clear(); which.assign(n, 0); *iterations = 0; *capped = 0; *empties = 0;
    unsigned j = 0;
    const int first = vt_first_index(vt_draw(seed, key, j++), n);
    centres.insert(centres.end(), D(first), D(first) + VT_WORDS);
    std::vector<int> min_d(n);
    for (int i = 0; i < n; i++) min_d[i] = bow_hamming(D(i), &centres[0]);
    int nc = 1;
    while (nc < k) {
        unsigned long long sum = 0;
        for (int i = 0; i < n; i++) { min_d[i] = std::min(min_d[i], bow_hamming(D(i), &centres[(size_t)(nc - 1) * VT_WORDS])); sum += (unsigned long long)min_d[i]; }
        if (sum == 0) break;
        const double cut = vt_next_cut(seed, key, &j, sum);
        unsigned long long up = 0; int pick = n - 1;
        for (int i = 0; i < n; i++) { up += (unsigned long long)min_d[i]; if (vt_reached(up, cut)) { pick = i; break; } }
        centres.insert(centres.end(), D(pick), D(pick) + VT_WORDS); nc++;
    }
    std::vector<int> last(n, -1), count((size_t)nc * 256), members(nc);
    for (int it = 1;; it++) {
        if (it > 1) {
            std::fill(count.begin(), count.end(), 0); std::fill(members.begin(), members.end(), 0);
            for (int i = 0; i < n; i++) {
                const int c = last[i]; members[c]++;
                for (int w = 0; w < VT_WORDS; w++) for (unsigned long long m = D(i)[w]; m; m &= m - 1) count[(size_t)c * 256 + w * 64 + __builtin_ctzll(m)]++;
            }
            for (int c = 0; c < nc; c++) {
                if (members[c] == 0) { ++*empties; continue; }
                const int th = vt_majority_threshold(members[c]);
                unsigned long long* m = &centres[(size_t)c * VT_WORDS]; m[0] = m[1] = m[2] = m[3] = 0;
                for (int b = 0; b < 256; b++) if (count[(size_t)c * 256 + b] >= th) m[b >> 6] |= 1ULL << (b & 63);
            }
        }
        bool changed = false;
        for (int i = 0; i < n; i++) {
            unsigned best = 0xFFFFFFFFu;
            for (int c = 0; c < nc; c++) { const unsigned key_c = bow_child_key(bow_hamming(D(i), &centres[(size_t)c * VT_WORDS]), c); if (key_c < best) best = key_c; }
            which[i] = (int)(best & 0xFF); changed |= which[i] != last[i];
        }
        *iterations = it;
        if (it > 1 && !changed) break;
        if (it == max_iterations) { *capped = 1; break; }
        last = which;
    }
    return nc;
}

// create(training_features, k, L): desc [N][4] in image order, offset [n_images + 1]
inline std::string vt_train_host(const unsigned long long* desc, const int32_t* offset, int n_images, int k, int L, unsigned long long seed, int max_iterations,
                                 VtFlat* flat, VtStats* st, BowVocHost* words)
{
    const int N = offset[n_images];
    const std::string err = vt_check_arguments(k, L, max_iterations, N);
    if (!err.empty()) return err;
    *st = VtStats();
    VtTree t; const unsigned long long zero[VT_WORDS] = {0, 0, 0, 0}; t.add(-1, zero);
    std::vector<int> perm(N), next_perm(N); for (int i = 0; i < N; i++) perm[i] = i;
    std::vector<VtSegment> level{VtSegment{0, 0, N, 0}}, next;
    std::vector<unsigned long long> centres; std::vector<int> which;
    unsigned long long pow21 = 1;
    for (int lv = 1; lv <= L && !level.empty(); lv++, pow21 *= 21) {
        next.clear(); st->level_nodes[lv - 1] = (int)level.size();
        for (const VtSegment& s : level) {
            const int* idx = &perm[s.begin]; int nc;
            if (s.n <= k) {                                         // :660 one cluster per feature
                st->trivial_nodes++; nc = s.n; centres.clear(); which.resize(s.n);
                for (int i = 0; i < s.n; i++) { centres.insert(centres.end(), desc + (size_t)idx[i] * VT_WORDS, desc + (size_t)idx[i] * VT_WORDS + VT_WORDS); which[i] = i; }
            } else {
                int it, capped, empties;
                nc = vt_node_kmeans(desc, idx, s.n, k, seed, s.key, max_iterations, centres, which, &it, &capped, &empties);
                st->kmeans_nodes++; st->short_nodes += nc < k; st->capped_nodes += capped; st->empty_cluster_events += empties;
                st->max_iterations_seen = std::max(st->max_iterations_seen, it); st->level_max_iterations[lv - 1] = std::max(st->level_max_iterations[lv - 1], it);
            }
            t.child_first[s.node] = (int)t.parent.size(); t.child_count[s.node] = nc;
            int at = s.begin;
            for (int c = 0; c < nc; c++) {                          // a stable partition by cluster, in place of the segment
                const int node = t.add(s.node, &centres[(size_t)c * VT_WORDS]), begin = at;
                for (int i = 0; i < s.n; i++) if (which[i] == c) next_perm[at++] = idx[i];
                if (lv < L && at - begin > 1) next.push_back(VtSegment{node, begin, at - begin, vt_child_key(s.key, pow21, c)});
            }
        }
        perm.swap(next_perm); level.swap(next);
    }
    vt_renumber(t, k, L, flat);
    const std::string e2 = bow_voc_build(k, L, 0, 0, (int)flat->parent.size(), flat->parent.data(), flat->is_leaf.data(), flat->descriptor.data(), flat->weight.data(), words);
    if (!e2.empty()) return e2;
    std::vector<int> ni; vt_count_images(*words, desc, offset, n_images, &ni);
    vt_set_weights(*words, ni, n_images, flat);
    st->nodes = words->n_nodes; st->words = words->n_words;
    return "";
}

// saveToTextFile (:1429-1449): `k L  0 0`, every descriptor byte followed by a space, one more space, the weight (%g for digits 0: the stream default)
inline std::string vt_text(int k, int L, const VtFlat& f, int digits)
{
    std::string out; char buf[64];
    snprintf(buf, sizeof buf, "%d %d  0 0\n", k, L); out += buf;
    for (size_t i = 0; i < f.parent.size(); i++) {
        snprintf(buf, sizeof buf, "%d %d ", f.parent[i], f.is_leaf[i] ? 1 : 0); out += buf;
        for (int b = 0; b < 32; b++) { snprintf(buf, sizeof buf, "%d ", (int)f.descriptor[i * 32 + b]); out += buf; }
        if (digits == 0) snprintf(buf, sizeof buf, " %g\n", f.weight[i]); else snprintf(buf, sizeof buf, " %.*g\n", digits, f.weight[i]);
        out += buf;
    }
    return out;
}

// a vocabulary back as the flat arrays it was built from
inline void vt_flat_of(const BowVocHost& v, VtFlat* f)
{
    const int n = v.n_nodes - 1;
    f->parent.assign(n, 0); f->is_leaf.assign(n, 0); f->descriptor.assign((size_t)n * 32, 0); f->weight.assign(n, 0.0);
    for (int p = 0; p < v.n_nodes; p++)
        for (int s = v.child_first[p]; s < v.child_first[p] + v.child_count[p]; s++) {
            const int i = v.slot_node[s] - 1;
            f->parent[i] = p; memcpy(&f->descriptor[(size_t)i * 32], &v.slot_desc[(size_t)s * 4], 32);
        }
    for (int i = 1; i < v.n_nodes; i++) { f->is_leaf[i - 1] = v.node_word[i] >= 0; f->weight[i - 1] = v.node_weight[i]; }
}
