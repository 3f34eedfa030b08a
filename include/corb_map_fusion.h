/* corb_map_fusion.h -- map-fusion detection for a whole submap in one call, on records (exported from libcorb_accel.so beside corb_accel.h).
 *
 * The server's detection loop (S/src/MapFusion.cpp:432-620 -> detectKeyFrameInServerMap :660-756) walks a submap's keyframes one at a time: a query of the global
 * map's database (DetectMapFusionCandidatesFromDB, C/src/KeyFrameDatabase.cc:189-295), SearchByBoWInServer against every candidate (C/src/ORBmatcher.cc:294-423),
 * the candidates with fewer than 15 matches dropped, the rest handed to the PnP RANSAC.  Until a fusion succeeds the database does not change between these steps,
 * so the three calls below take all keyframes of a submap at once and give, bit for bit, what corb_kfdb_detect / corb_search_by_bow_slots give when they are
 * called one after the other in list order.  No existing struct changes: CORB_ABI_VERSION stays as corb_accel.h states it. */
#ifndef CORB_MAP_FUSION_H
#define CORB_MAP_FUSION_H
#include "corb_accel.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CORB_KFDB_BATCH_MAX_QUERIES 65535

/* n_queries queries of kind 1 (relocalisation) or 2 (map fusion) against the database: exactly corb_kfdb_detect(db, kind, query_entries[i], query_ids[i], NULL, 0, 0, ..)
 * for i = 0 .. n_queries - 1 in list order.  cand[cand_offset[i] .. cand_offset[i + 1]) = the candidates of query i in the reference's order; afterwards the six
 * fields of every entry (corb_kfdb_get_state) are what that sequence of single calls leaves, the stale mRelocScore a neighbour adds included (an entry's fields at
 * query i come from the most recent earlier query that shared a word with it, of this call or before it).
 * CORB_ERR_ARG with nothing changed: kind 0 (one query per keyframe by nature: it needs a connected set and a minScore each; corb_loop_detect.h takes both from the device), more than
 * CORB_KFDB_BATCH_MAX_QUERIES queries, a query entry outside the database or without a BowVector (it may be in the database or not, and may be listed twice under
 * different ids), two equal query_ids.  n_queries == 0: CORB_OK, cand_offset[0] = 0.  More than cap candidates in all: CORB_ERR_OVERFLOW with *n_total = the room
 * needed, cand_offset complete and the fields updated all the same (as the single call does).
 * n_queries x capacity must stay below 2^31 (CORB_ERR_ARG): offsets and the total are 32-bit.  One synchronisation and one read-back, sized before the total is
 * known: min(cap, n_queries x capacity) candidate slots travel, so pass the cap you expect to need, not the largest possible.  Development switch CORB_KFDB_BATCH_CHUNK=n (read at every call): queries per pass over the workspace, at most what the memory bound allows;
 * every value gives the same bytes. */
int corb_kfdb_detect_batch(CorbKfDb* db, int kind, const int32_t* query_entries, const uint64_t* query_ids, int n_queries,
                           int32_t* cand_offset, int32_t* cand, int cap, int* n_total);

/* corb_search_by_bow_slots for n_pairs pairs (slots_a[p] of a, slots_b[p] of b) in one call: row p of match (match_stride entries, -1 behind the row's length:
 * n(slots_b[p]) for variant 0, n(slots_a[p]) for variant 1) and n_matches[p] are what the single call returns.  A slot may appear in many pairs; a slot without
 * features or a pair without a common vocabulary node gives a row of -1 and a count of 0.  CORB_ERR_ARG if match_stride is below the longest row.
 * One upload, one synchronisation, one read-back. */
int corb_search_by_bow_slots_batch(int variant, CorbKfStore* a, const int32_t* slots_a, CorbKfStore* b, const int32_t* slots_b, int n_pairs,
                                   float nnratio, int check_orientation, int match_stride, int32_t* match, int32_t* n_matches);

/* one candidate of one query: `entry` of the database, its record `slot` in the global store (-1: none), the matches SearchByBoW found (0 without a slot),
 * whether the row goes on to the PnP RANSAC, and where its map-point ids start in matched_ids (-1 if not kept) */
typedef struct CorbFusionRow { int32_t query, entry, slot, n_matches, kept; int64_t ids_offset; } CorbFusionRow;

/* detectKeyFrameInServerMap :662-707 for every keyframe of a submap: corb_kfdb_detect_batch with kind 2, then SearchByBoW (variant 0: keyframe side = the
 * candidate's record entry_slot[entry] of `global`, frame side = the query's record query_slots[i] of `sub`) for every candidate that has a record, then per row
 *   kept = slot >= 0, the record holds features and is not CORB_KF_BAD, n_matches >= min_matches
 * and for every kept row matched_ids[ids_offset + iF] = the map-point id the candidate's record holds at feature match[iF] (CORB_NO_MAP_POINT where iF has no
 * match), iF = 0 .. n(query_slots[query]) - 1.  The reference uses nnratio 0.75, check_orientation 1, min_matches 15.
 * rows[row_offset[i] .. row_offset[i + 1]) = the candidates of query i in detection order.  The kept rows of one query are consecutive in matched_ids, so
 * matched_ids + (the first kept row's ids_offset) with the number of kept rows is what corb_pnp_ransac_store(sub, query_slots[i], ..) reads.
 * entry_slot has one entry per database entry.  The database's fields end as corb_kfdb_detect_batch leaves them; no record changes.
 * More rows than cap_rows: CORB_ERR_OVERFLOW after the detection alone, *n_rows = the room needed, *n_ids = 0.  More ids than cap_ids: CORB_ERR_OVERFLOW with the
 * rows complete and *n_ids = the room needed.  Two synchronisations (the candidate counts size the pair list); descriptors, matches and ids stay on the device. */
int corb_map_fusion_candidates_store(CorbKfDb* db, CorbKfStore* sub, const int32_t* query_slots, const int32_t* query_entries, const uint64_t* query_ids, int n_queries,
                                     CorbKfStore* global, const int32_t* entry_slot, float nnratio, int check_orientation, int min_matches,
                                     int32_t* row_offset, CorbFusionRow* rows, int cap_rows, int* n_rows,
                                     uint64_t* matched_ids, int64_t cap_ids, int64_t* n_ids);

#ifdef __cplusplus
}
#endif
#endif
