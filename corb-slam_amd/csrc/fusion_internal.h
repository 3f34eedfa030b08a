// fusion_internal.h -- device views and launchers shared by fusion_kernels.hip and corb_fusion.cpp (include/corb_map_fusion.h: detection for a whole submap)
#pragma once
#include "bow_internal.h"
#include "store_internal.h"
#include "corb_map_fusion.h"

// ---- corb_kfdb_detect_batch: one pass over `n` queries (a chunk) of the call.  Every per-(query, entry) array is indexed [q * capacity + e] ----
struct FusionDetectDev {
    int n;                                          // queries of this pass
    const int* q_entry; const unsigned long long* q_id;      // [n] of this pass
    int* common; uint32_t* first_word;              // fusion_common_kernel: words entry e shares with query q (0 for an entry outside the inverted file), the first of them
    unsigned char* pushed; unsigned char* id_match; // fusion_walk_kernel: e entered lKFsSharingWords of q; mnRelocQuery(e) == id(q) when q's accumulation runs
    int* words;                                     //   mnRelocWords(e) after q's walk
    int* max_common;                                // [n] zeroed by the host before the walk
    unsigned char* scored; float* score;            // fusion_score_kernel: e was scored for q (written for every pair); its score (written where scored)
    float* seen;                                    // fusion_seen_kernel: mRelocScore(e) as q's accumulation reads it
    unsigned long long* skey; int* sent;            // [n][P] fusion_select_kernel's list of scored entries: (first word, sequence number) and entry
    int P;                                          // the power of two >= capacity
    float* acc; int* best; int* first_pos;          // select: first_pos preset to BOW_NO_POS by the host
    int* row; int* n_row;                           // [n][capacity] candidates of q in order; [n] their number
};
// the five kernels of one pass, in order, then the append of the pass's candidates to the call's output: out = [offset (n_queries + 1) | cand (cap)],
// total[0] = candidates so far (zeroed by the host before the first pass); q0 = the pass's first query
void corb_launch_fusion_detect(const BowDbDev& d, const FusionDetectDev& f, int q0, int* out_offset, int* out_cand, int cap, int* total, hipStream_t s);

// ---- corb_search_by_bow_slots_batch ----
struct FusionMatchDev {
    int variant, check_ori, n_list, n_pairs, stride;
    float nnratio;
    const int* list;                                // [n_list][3] pair, node of fv(a), node of fv(b): the common vocabulary nodes of all pairs
    const int* pair;                                // [n_pairs][3] slot of a, slot of b, entries of the row
    const char* base_a; const char* base_b; size_t bytes_a, bytes_b; int Fa, Fb;      // the two stores' records
    int* match; int* bin;                           // [n_pairs][stride] preset to -1
    int* hist;                                      // [n_pairs][CORB_HISTO_LENGTH] preset to 0
    int* n_matches;                                 // [n_pairs] preset to 0
};
void corb_launch_fusion_match(const FusionMatchDev& m, hipStream_t s);

// ---- corb_map_fusion_candidates_store: kept, ids_offset and the ids of the kept rows ----
struct FusionRowsDev {
    int n_rows, min_matches;
    CorbFusionRow* rows;                            // query, entry, slot from the host; n_matches, kept, ids_offset written here
    const int* row_pair;                            // [n_rows] the row's pair of the match call, -1 without a slot
    const int* q_features;                          // [n_queries] n(query slot)
    const int* match; int stride; const int* n_matches;
    const char* base_g; size_t bytes_g; int Fg;     // the global store's records
    unsigned long long* ids; long long cap_ids; long long* n_ids;
};
void corb_launch_fusion_rows(const FusionRowsDev& r, hipStream_t s);
