/* corb_essential_graph.h -- Optimizer::OptimizeEssentialGraph (C/src/Optimizer.cc:840-1117) on device-resident records: the loop-edge sets of the covisibility
 * graph (KeyFrame::AddLoopEdge / GetLoopEdges, C/src/KeyFrame.cc:545-561), the flattening of the graph into vertices, edges and measurements, the solve and the
 * write-back of poses and map points.  Exported from libcorb_accel.so beside the drop-in boundary of corb_accel.h; corb_accel.h and CORB_ABI_VERSION are unchanged.
 *
 * House rules as for the other calls on records: keyframes are named by slots of the graph's keyframe store; argument errors are a status with a message in
 * corb_last_error(); the graph, then the keyframe store, then the map-point store are locked (each once) before a record is read; on CORB_ERR_CAPACITY nothing is
 * written but the counts.  corb_essential_graph_plan / _store take lane 1 of the per-device workspace (the long-optimisation lane); their outputs do not depend on
 * what the arena held before, nor on the order in which device atomics land (the only atomics are integer counters).
 *
 * The definition of every output is tests/essgraph_reference.py; it reads as follows ("held": the id resolves to a slot of the store; a slot without features
 * is not a keyframe, of two slots with one id the lower is the keyframe).
 *
 * VERTICES (:869-904).  Every held keyframe that is not CORB_KF_BAD gets a vertex; vertex r is the r-th of them in ASCENDING KEYFRAME ID (the reference walks
 *   pointer-ordered containers; the same choice corb_loop_correct_store made).  S[r] = the Corrected value if the keyframe's slot is in corr_slots (:880-884), else
 *   g2o::Sim3(Rcw, tcw, 1) of the record's float pose (:887-891) in the FP64 operation order of csrc/sim3_math.h.  snc[r] = the NonCorrected value if listed, else
 *   S[r]: what :951-956, :967-972, :994-999, :1025-1030 pick for the normal edges.  fixed[r] = slot == loop_slot || CORB_KF_FIXED (:894).
 * EDGES.  An edge is (vi, vj, kind, measurement): vertex 0 = vi is keyframe i (:931), vertex 1 = vj; measurement = Sji = Sjw * Swi (:927).
 *   kind 0, loop connections (:912-940), first: the keys of LoopConnections in ascending id, each set in ascending id.  A pair other than (cur, loop) needs
 *     GetWeight(i, j) >= min_weight (:923).  Sjw, Swi from the vertex values S.  An emitted pair enters sInsertedEdges (:938).
 *   then, per HELD keyframe i in ascending id (bad ones included: :943 has no isBad test), with Swi = snc[i]^-1 and Sjw = snc[j]:
 *   kind 1, the tree edge (:958-983) when the parent id is held;
 *   kind 2, the loop edges (:986-1009): the HELD ids of i's loop-edge set (GetLoopEdges drops the others) that are smaller than id(i), ascending;
 *   kind 3, the covisibility edges (:1012-1042): GetCovisiblesByWeight(min_weight) in list order (corb_covis_query with min_weight; a list whose every weight
 *     reaches min_weight answers nothing, as there).  A neighbour must be held (:1016 pKFn), not the parent, not a child, not in the loop-edge set (:1016), not
 *     bad, of smaller id (:1018), and not in sInsertedEdges (:1020); n_suppressed[0..5] count, in this order of tests, the neighbours each test turned away.
 * DROPPED EDGES.  Where the reference would hand g2o a null vertex -- an end of a loop connection is not held or is bad, the parent or a loop edge is bad, or
 *   keyframe i of the second loop is itself bad -- the edge is dropped and counted in n_dropped; it is never emitted and never enters sInsertedEdges.
 *
 * corb_essential_graph_store plans, solves with the Levenberg loop of corb_optimize_essential_graph (the same functions and kernels on the arrays the plan left on
 * the device: same inputs, same edge order, same bits) and commits:
 *   poses (:1053-1076)   Tcw <- [R | t * (1/s)] of the final estimate, rounded to float once, into the record of every vertex whose keyframe is not CORB_KF_FIXED
 *                        (the loop keyframe included, as in the reference);
 *   points (:1079-1115)  over the slots of the map-point index: CORB_MP_BAD and CORB_MP_FIXED points are passed over; nIDr = scratch corrected_reference if scratch
 *                        corrected_by_kf == id(cur) (:1088-1091), else ref_kf_id (CORB_NO_MAP_POINT: skipped, :1095); p <- correctedSwr.map(Srw.map(p)) in FP64,
 *                        rounded to float once, Srw the vertex's initial value S, correctedSwr the inverse of its final estimate.  A reference keyframe without a
 *                        vertex keeps the point untouched (the reference maps through two default identities and re-runs UpdateNormalAndDepth; here nothing of
 *                        the record is written).  scale_factor > 0: MapPoint::UpdateNormalAndDepth on the moved points with the committed poses (csrc/normal_depth.h);
 *                        0 leaves normal and distances alone, as corb_ba_solve_store does.
 *   ONE DEVIATION: :1057 skips getFixed() keyframes BEFORE vCorrectedSwc is filled, so the reference maps a point whose reference keyframe is fixed through an
 *   identity and throws it into that camera's frame.  corb_optimize_essential_graph (eg_apply_kernel) uses the final estimate of every vertex; this call does the
 *   same, and counts such points in n_points_fixed_ref.
 * The call writes nothing else: every other byte of every record, the graph and the scratch fields stay as they are. */
#ifndef CORB_ESSENTIAL_GRAPH_H
#define CORB_ESSENTIAL_GRAPH_H
#include "corb_accel.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- mspLoopEdges per slot: a set of keyframe ids kept in ascending id; a fresh graph holds empty sets ---- */
#define CORB_COVIS_MAX_LOOP_EDGES 32
/* AddLoopEdge(other) on `slot`, one direction per call (the reference makes two calls, LoopClosing.cc:577-578).  An id the set holds already: nothing happens.
 * A full set: CORB_ERR_CAPACITY, nothing written.  other_slot must hold a keyframe (CORB_ERR_ARG otherwise). */
int corb_covis_add_loop_edge(CorbCovis* g, int slot, int other_slot);
/* the set as it stands (held or not), ascending; more than cap: CORB_ERR_CAPACITY with *n set */
int corb_covis_get_loop_edges(CorbCovis* g, int slot, uint64_t* ids, int cap, int* n);
int corb_covis_clear_loop_edges(CorbCovis* g, int slot);

/* ---- the inputs of Optimizer::OptimizeEssentialGraph ---- */
typedef struct CorbEssentialGraphInput {
    int32_t loop_slot, cur_slot;            /* pLoopKF, pCurKF */
    int32_t n_corr, n_lc;
    const int32_t* corr_slots;              /* [n_corr] the keys of CorrectedSim3 / NonCorrectedSim3, no slot twice */
    const double* corrected;                /* [n_corr x 8] quaternion x y z w, t, s: the layout corb_loop_correct_store returns */
    const double* non_corrected;            /* [n_corr x 8] */
    const int32_t* lc_kf;                   /* [n_lc] the keys of LoopConnections as slots, no slot twice */
    const int32_t* lc_offset;               /* [n_lc + 1] CSR into lc_slots */
    const int32_t* lc_slots;                /* the sets as slots, no slot twice in a set */
    int32_t min_weight;                     /* minFeat (:866: 100) */
    int32_t pad;
} CorbEssentialGraphInput;

typedef struct CorbEssentialGraphCounts {
    int32_t n_vertices, n_edges;
    int32_t n_kind[4];                      /* 0 loop connection, 1 tree, 2 loop edge, 3 covisibility */
    int32_t n_dropped;
    int32_t n_lc_below_weight;              /* loop connections :923 turned away */
    int32_t n_suppressed[6];                /* covisibility neighbours turned away: parent, child, loop edge, bad, not of smaller id, already inserted */
} CorbEssentialGraphCounts;

/* Pure: writes nothing but its outputs.  v_slots [v_cap], S [v_cap x 8], fixed [v_cap], snc [v_cap x 8]; vi, vj, kind [e_cap], measurement [e_cap x 8]; any of
 * them may be NULL.  n_vertices > v_cap or n_edges > e_cap: CORB_ERR_CAPACITY with *counts complete and no array written.  Without a map-point index: CORB_ERR_ARG
 * (the store call's rule; the plan itself reads no map point). */
int corb_essential_graph_plan(CorbCovis* g, const CorbEssentialGraphInput* in, int v_cap, int e_cap, int32_t* v_slots, double* S, uint8_t* fixed, double* snc,
                              int32_t* vi, int32_t* vj, uint8_t* kind, double* measurement, CorbEssentialGraphCounts* counts);

typedef struct CorbEssentialGraphResult {
    CorbEssentialGraphCounts graph;
    int32_t iters_done;
    int32_t n_poses_set;
    int32_t n_points_moved, n_points_kept, n_points_skipped, n_points_fixed_ref;   /* kept: the reference keyframe has no vertex; skipped: no reference keyframe;
                                                                                      fixed_ref: moved points whose reference keyframe is CORB_KF_FIXED */
} CorbEssentialGraphResult;

/* chi2_hist (optional): iterations + 1 doubles, as corb_optimize_essential_graph fills them.  S_final (optional): [v_cap x 8] the final estimates in vertex order;
 * n_vertices > v_cap: CORB_ERR_CAPACITY with out->graph complete and nothing written anywhere.  Without a map-point index: CORB_ERR_ARG. */
int corb_essential_graph_store(CorbCovis* g, const CorbEssentialGraphInput* in, int iterations, int fix_scale, float scale_factor, double* chi2_hist,
                               double* S_final, int v_cap, CorbEssentialGraphResult* out);

#ifdef __cplusplus
}
#endif
#endif
