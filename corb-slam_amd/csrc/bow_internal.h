// bow_internal.h -- device views and launchers shared by bow_kernels.hip and corb_bow.cpp (vocabulary transform and keyframe database, include/corb_accel.h last section)
#pragma once
#include "corb_internal.h"
#include "bow_math.h"
#include "owned_hip.h"

// one descriptor set of a transform: where its features are and where its two vectors go (device pointers; every pointer is valid, unwanted outputs go to scratch)
struct BowSetDev {
    const unsigned long long* desc;     // [n][4]
    int n, feat_off;                    // features of the set; its first entry in the call's per-feature arrays
    int max_words;                      // room at bow_word / bow_value
    uint32_t* bow_word; double* bow_value; int* bow_count;        // BowVector; *bow_count = words, or -1 if they do not fit
    uint32_t* fv_node; int32_t* fv_off; uint32_t* fv_idx; int32_t* fv_n_nodes;      // FeatureVector in CorbFeatVec form
    uint32_t* node_copy;                // the node ids once more, compact, for the call's one read-back
    int32_t* counts;                    // [3] words, nodes, overflow -- read back with node_copy
};

struct BowDbDev {
    int capacity, max_words, n_vocab_words;
    uint32_t* words; double* values; int* n_words;                // [capacity][max_words] ascending words; n_words < 0: the entry has no BowVector
    unsigned char* live; uint32_t* seq;                           // in the inverted file; insertion sequence number of the last add
    BowKfState* st; int* nb;                                      // the six fields; [capacity][10] neighbours, -1 padded
    double* dense;                                                // [n_vocab_words] the query's BowVector scattered over the words, 0 elsewhere
    unsigned char* conn;                                          // [capacity] 1 for the loop query's connected keyframes during a query
    int* conn_list;                                               // [capacity]
    int* ctr;                                                     // [0] maxCommonWords  [1] scored keyframes kept
    unsigned char* pushed; uint32_t* first_word;                  // [capacity] entered lKFsSharingWords; first word shared with the query
    unsigned long long* skey; int* sent;                          // [pow2 >= capacity] kept keyframes: (first word, sequence number) and entry
    float* acc; int* best; int* first_pos;                        // [capacity]
    int* out;                                                     // [1 + capacity] n, candidates
    double* score_out;                                            // [capacity]
};
#define BOW_NO_POS 0x7F7F7F7F

// a vocabulary handle: the host form and its upload.  voc_finish (corb_bow.cpp) uploads v->host and hands the handle out, or frees it and returns the error.
struct CorbVoc {
    int device = 0;
    BowVocHost host;
    BowVocView dev{};                 // device pointers
    DevList allocs;
};
int voc_finish(CorbVoc* v, int device, CorbVoc** out, const char* who);

#include <mutex>
#include <vector>
// a keyframe database handle (corb_bow.cpp; the whole-submap calls of corb_fusion.cpp work on it too)
struct CorbKfDb {
    int device = 0;
    CorbVoc* voc = nullptr;
    BowDbDev d{};
    OwnedStream stream;
    std::mutex mu;
    DevList allocs;
    PinnedMem pinned;                           // [2 * capacity + 2] ints: connected list / entry lists up, candidates down
    PinnedMem pinned_score;                     // [capacity] doubles
    std::vector<int> n_words;                   // host mirror: words of an entry's BowVector, -1 = none
    std::vector<char> live;
    uint32_t next_seq = 1;
};
#define BOW_MAX_SETS 65535          // descriptor sets per transform call: the sets are one grid dimension

// corb_bow_profile: event pairs per launch, and wall-clock ticks of the two in-order sums (ticks[0] the norm loop of bow_build_kernel, [1] that kernel's lane 0 in all;
// [2] the ordered additions of kfdb_score_kernel summed over its wavefronts, [3] those wavefronts' whole time).  Both null: off.
struct BowProfile { CorbProfiler* prof; unsigned long long* ticks; };
BowProfile corb_bow_profile_state();

void corb_launch_bow_transform(const BowVocView& v, const BowSetDev* sets, int n_sets, int max_n, int levelsup, int32_t* feat_word, uint32_t* feat_node, hipStream_t s, int* rc_attr = nullptr);
void corb_launch_bow_descend(const BowVocView& v, const BowSetDev* sets, int n_sets, int max_n, int32_t* feat_word, uint32_t* feat_node, hipStream_t s);      // the descent alone, levelsup 0
void corb_launch_kfdb_detect(const BowDbDev& d, int kind, int query_entry, int query_words, unsigned long long query_id, int n_connected, float min_score, hipStream_t s);
void corb_launch_kfdb_score(const BowDbDev& d, int entry_a, int words_a, const int* entries_b, int n, hipStream_t s);

// The loop query of LoopClosing::DetectLoop with everything but the query entry in device memory (corb_loopdetect.cpp).  The kernel that fills it has also set
// d.conn for conn_list[0 .. n_conn).  skip != 0: every kernel of the launch returns at once and nothing of d changes.
struct BowLoopQuery {
    int skip;
    int n_score;                        // entries of score_entries: the covisible keyframes minScore is taken over
    int n_conn;                         // entries of d.conn_list whose d.conn flag is set
    float min_score;                    // written by the launch: min over float(score(query, score_entries[i])), from 1.0f (LoopClosing.cc:124-137)
    unsigned long long id;              // the query's mnId
};
// scatter, the scores of score_entries (at most max_score of them) with their minimum into q->min_score, then count / score / select as corb_launch_kfdb_detect(kind 0)
// runs them with q->id and q->min_score, then the unscatter, which also clears the d.conn flags.  d.out holds the candidates as after corb_launch_kfdb_detect
void corb_launch_kfdb_loop_query(const BowDbDev& d, int query_entry, int query_words, BowLoopQuery* q, const int* score_entries, int max_score, hipStream_t s);
