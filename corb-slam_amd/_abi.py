"""The C ABI of libcorb_accel.so (include/*.h) stated once for Python: the constants, the ctypes.Structure mirrors and numpy record dtypes of the C structs, each
under its C name (STRUCTS, DTYPES), and one prototype per exported function (PROTOTYPES), which bind() puts onto an opened library.  tests/test_abi_table.py checks
all of it against the headers and the compiler; nothing here calls the library."""
import ctypes as C
import numpy as np


class CorbError(RuntimeError):
    pass


ABI_VERSION = 6                                 # CORB_ABI_VERSION of the headers mirrored below (the structs carry no size fields)
SENSOR_MONOCULAR, SENSOR_RGBD = 0, 2            # CORB_SENSOR_*
DEPTH_U16, DEPTH_F32 = 0, 1                     # CORB_DEPTH_*
NO_MAP_POINT = NO_ID = 0xFFFFFFFFFFFFFFFF       # CORB_NO_MAP_POINT: "none"
KF_BAD, KF_FIXED, MP_BAD, MP_FIXED = 1, 2, 1, 2
ERR_CAPACITY = -2                               # CORB_ERR_CAPACITY
BOW_MAX_FEATURES = 8192                         # CORB_BOW_MAX_FEATURES
NP_OK, NP_NO_PARALLAX, NP_W_ZERO, NP_BEHIND_1, NP_BEHIND_2, NP_REPROJ_1, NP_REPROJ_2, NP_SCALE = range(8)                # CORB_NP_*: status of a pair in CreateNewMapPoints
INIT_OK, INIT_NO_MODEL, INIT_H_DEGENERATE, INIT_AMBIGUOUS, INIT_FEW_POINTS, INIT_LOW_PARALLAX = range(6)                # CORB_INIT_*


# ---- include/corb_accel.h: configurations, layouts, profiles ----
class OrbConfig(C.Structure):
    _fields_ = [("nfeatures", C.c_int32), ("scale_factor", C.c_float), ("nlevels", C.c_int32),
                ("ini_th_fast", C.c_int32), ("min_th_fast", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("max_images", C.c_int32), ("device", C.c_int32)]


class StereoConfig(C.Structure):
    _fields_ = [("orb", OrbConfig), ("max_frames", C.c_int32), ("fx", C.c_float), ("bf", C.c_float)]


class StereoFrameLayout(C.Structure):
    _fields_ = [("capacity", C.c_int32), ("frame_bytes", C.c_int32), ("off_kp_left", C.c_int32), ("off_kp_right", C.c_int32),
                ("off_desc_left", C.c_int32), ("off_desc_right", C.c_int32), ("off_u_right", C.c_int32), ("off_depth", C.c_int32)]


class StereoFrameTiming(C.Structure):
    _fields_ = [("ms_upload", C.c_float), ("ms_kernels", C.c_float), ("ms_download", C.c_float)]


class CameraConfig(C.Structure):
    _fields_ = [("orb", OrbConfig), ("max_frames", C.c_int32), ("sensor", C.c_int32), ("channels", C.c_int32), ("rgb", C.c_int32)] + \
               [(k, C.c_float) for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "bf", "depth_map_factor")] + [("depth_format", C.c_int32)]


class RgbdFrameLayout(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("capacity", "frame_bytes", "input_bytes", "off_keys", "off_keys_un", "off_desc", "off_u_right", "off_depth")]


class KernelTime(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("total_ms", C.c_double), ("launches", C.c_int64)]


KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])


# ---- the matchers on host pointers ----
class _FeatVec(C.Structure):
    _fields_ = [("n_nodes", C.c_int32), ("node_id", C.c_void_p), ("offset", C.c_void_p), ("idx", C.c_void_p)]


class _BowSide(C.Structure):
    _fields_ = [("desc", C.c_void_p), ("angle", C.c_void_p), ("valid", C.c_void_p), ("n", C.c_int32), ("fv", _FeatVec)]


class _TriSide(C.Structure):
    _fields_ = [("desc", C.c_void_p), ("kp", C.c_void_p), ("u_right", C.c_void_p), ("has_mappoint", C.c_void_p),
                ("n", C.c_int32), ("fv", _FeatVec)]


class _FrameView(C.Structure):
    _fields_ = [("keys_un", C.c_void_p), ("u_right", C.c_void_p), ("desc", C.c_void_p), ("n", C.c_int32), ("claimed", C.c_void_p),
                ("min_x", C.c_float), ("min_y", C.c_float), ("max_x", C.c_float), ("max_y", C.c_float), ("scale", C.c_void_p), ("nlevels", C.c_int32)]


class _KeyFrameView(C.Structure):
    _fields_ = [("keys_un", C.c_void_p), ("u_right", C.c_void_p), ("desc", C.c_void_p), ("n", C.c_int32),
                ("min_x", C.c_float), ("min_y", C.c_float), ("max_x", C.c_float), ("max_y", C.c_float),
                ("scale", C.c_void_p), ("inv_level_sigma2", C.c_void_p), ("nlevels", C.c_int32), ("log_scale_factor", C.c_float),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("bf", C.c_float)]


TRACKED_DTYPE = np.dtype([("proj_x", "<f4"), ("proj_y", "<f4"), ("proj_xr", "<f4"), ("view_cos", "<f4"), ("level", "<i4"),
                          ("valid", "u1"), ("claims", "u1"), ("pad", "u1", 2)])
LAST_DTYPE = np.dtype([("world", "<f4", 3), ("angle", "<f4"), ("octave", "<i4"), ("valid", "u1"), ("claims", "u1"), ("pad", "u1", 2)])
MP_DTYPE = np.dtype([("world", "<f4", 3), ("normal", "<f4", 3), ("min_distance", "<f4"), ("max_distance", "<f4"), ("angle", "<f4"),
                     ("valid", "u1"), ("pad", "u1", 3)])


# ---- the optimisers on host pointers ----
EDGE_DTYPE = np.dtype([("pose", "<i4"), ("point", "<i4"), ("u", "<f4"), ("v", "<f4"),
                       ("ur", "<f4"), ("inv_sigma2", "<f4")])


class _BAProblem(C.Structure):
    _fields_ = [("n_poses", C.c_int32), ("n_points", C.c_int32), ("n_edges", C.c_int32),
                ("poses", C.c_void_p), ("pose_fixed", C.c_void_p), ("points", C.c_void_p),
                ("point_fixed", C.c_void_p), ("edges", C.c_void_p),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("bf", C.c_float), ("intr", C.c_void_p)]


class _BAResult(C.Structure):
    _fields_ = [("poses", C.c_void_p), ("points", C.c_void_p), ("chi2", C.c_void_p), ("lam", C.c_void_p),
                ("iters_done", C.c_int32), ("trials_total", C.c_int32),
                ("ms_total", C.c_double), ("ms_build", C.c_double), ("ms_schur", C.c_double),
                ("ms_solve", C.c_double), ("ms_update", C.c_double), ("solver_used", C.c_int32), ("pcg_iterations", C.c_int32),
                ("free_poses", C.c_int32), ("free_points", C.c_int32), ("active_edges", C.c_int32), ("nnz_blocks", C.c_int64), ("schur_pairs", C.c_int64),
                ("pc_block", C.c_int32), ("pc_levels", C.c_int32),
                ("pcg_residual_max", C.c_double), ("pcg_residual_last", C.c_double), ("grad_inf", C.c_double), ("pcg_refined_trials", C.c_int32), ("reserved0", C.c_int32)]


class BAOptions(C.Structure):
    _fields_ = [("solver", C.c_int32), ("pcg_tol", C.c_double), ("pcg_max_iter", C.c_int32), ("pc_block", C.c_int32), ("pc_multilevel", C.c_int32), ("scale_factor", C.c_float)]


class BAStage(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("robust", C.c_int32), ("chi2_mono", C.c_float), ("chi2_stereo", C.c_float),
                ("check_depth", C.c_int32), ("recompute_inactive", C.c_int32), ("allow_reactivate", C.c_int32),
                ("reset_estimates", C.c_int32), ("float_compare", C.c_int32), ("huber_mono", C.c_float), ("huber_stereo", C.c_float)]


class _PoseOptFrame(C.Structure):
    _fields_ = [("Tcw", C.c_void_p), ("n_obs", C.c_int32), ("points", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p),
                ("u_right", C.c_void_p), ("inv_sigma2", C.c_void_p),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("bf", C.c_float)]


class _Sim3Problem(C.Structure):
    _fields_ = [("n", C.c_int32), ("p1c", C.c_void_p), ("p2c", C.c_void_p), ("obs1", C.c_void_p), ("obs2", C.c_void_p),
                ("inv_sigma2_1", C.c_void_p), ("inv_sigma2_2", C.c_void_p)] + [(k, C.c_float) for k in ("fx1", "fy1", "cx1", "cy1", "fx2", "fy2", "cx2", "cy2")]


# ---- the record stores, the push and the tracking calls on records ----
KF_META_DTYPE = np.dtype([("id", "<u8"), ("client_id", "<i4"), ("flags", "<u4"), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("bf", "<f4"),
                          ("nlevels", "<i4"), ("Tcw", "<f4", 16), ("TcwGBA", "<f4", 16), ("ba_global_for_kf", "<u8"), ("inv_level_sigma2", "<f4", 16)])
MP_RECORD_DTYPE = np.dtype([("id", "<u8"), ("ref_kf_id", "<u8"), ("descriptor", "u1", 32), ("client_id", "<i4"), ("n_obs", "<i4"), ("flags", "<u4"), ("world_pos", "<f4", 3),
                            ("normal", "<f4", 3), ("min_distance", "<f4"), ("max_distance", "<f4"), ("pos_gba", "<f4", 3), ("ba_global_for_kf", "<u8")], align=True)
MP_COUNTERS_DTYPE = np.dtype([("n_visible", "<i4"), ("n_found", "<i4"), ("replaced_by", "<u8")])
MP_SCRATCH_DTYPE = np.dtype([("first_kf_id", "<i8"), ("first_frame", "<i8"), ("track_reference_for_frame", "<u8"), ("last_frame_seen", "<u8"), ("ba_local_for_kf", "<u8"),
                             ("fuse_candidate_for_kf", "<u8"), ("loop_point_for_kf", "<u8"), ("corrected_by_kf", "<u8"), ("corrected_reference", "<u8"),
                             ("track_proj_x", "<f4"), ("track_proj_y", "<f4"), ("track_proj_xr", "<f4"), ("track_view_cos", "<f4"), ("track_scale_level", "<i4"),
                             ("n_obs_weight", "<i4"), ("track_in_view", "u1"), ("pad", "u1", 7)])
PUSH_HEADER_DTYPE = np.dtype([("status", "<i4"), ("n_kf", "<i4"), ("n_mp", "<i4"), ("kf_record_bytes", "<i4"), ("mp_record_bytes", "<i4")])
PUSH_MSG_DTYPE = np.dtype([("peer", "<i4"), ("kind", "<i4"), ("first_record", "<i4"), ("n_records", "<i4"), ("bytes", "<i8")])


class _MapPush(C.Structure):
    _fields_ = [("kf", C.c_void_p), ("kf_slots", C.c_void_p), ("n_kf", C.c_int32), ("mp", C.c_void_p), ("mp_slots", C.c_void_p), ("n_mp", C.c_int32),
                ("kf_dst_first", C.c_void_p), ("mp_dst_first", C.c_void_p), ("kf_recv_counts", C.c_void_p), ("mp_recv_counts", C.c_void_p)]


class _RcclFns(C.Structure):
    _fields_ = [("group_start", C.CFUNCTYPE(C.c_int)), ("group_end", C.CFUNCTYPE(C.c_int)),
                ("send", C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p)),
                ("recv", C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p))]


class TrackCamera(C.Structure):
    """CorbTrackCamera: Frame intrinsics, image bounds and mvScaleFactors"""
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("bf", C.c_float), ("mb", C.c_float),
                ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float), ("nlevels", C.c_int32), ("scale", C.c_float * 16)]

    @classmethod
    def make(cls, fx, fy, cx, cy, bf, mb, min_x, max_x, min_y, max_y, scale):
        c = cls(); c.fx, c.fy, c.cx, c.cy, c.bf, c.mb = fx, fy, cx, cy, bf, mb
        c.min_x, c.max_x, c.min_y, c.max_y = min_x, max_x, min_y, max_y
        c.nlevels = len(scale)
        for i, v in enumerate(scale):
            c.scale[i] = float(v)
        return c


# ---- CreateNewMapPoints, the RANSAC routes, the monocular initializer ----
class _NewPointSide(C.Structure):
    _fields_ = [("keys_un", C.c_void_p), ("u_right", C.c_void_p), ("depth", C.c_void_p), ("n", C.c_int32), ("Tcw", C.c_float * 16)] + \
               [(k, C.c_float) for k in ("fx", "fy", "cx", "cy", "bf", "mb")] + [("scale", C.c_void_p), ("nlevels", C.c_int32)]


class _Sim3RansacProblem(C.Structure):
    _fields_ = [("n", C.c_int32), ("p1c", C.c_void_p), ("p2c", C.c_void_p), ("sigma2_1", C.c_void_p), ("sigma2_2", C.c_void_p)] + \
               [(k, C.c_float) for k in ("fx1", "fy1", "cx1", "cy1", "fx2", "fy2", "cx2", "cy2")]


class _PnPRansacProblem(C.Structure):
    _fields_ = [("n", C.c_int32), ("p3dw", C.c_void_p), ("p2d", C.c_void_p), ("sigma2", C.c_void_p)] + [(k, C.c_float) for k in ("fx", "fy", "cx", "cy")]


class _InitProblem(C.Structure):
    _fields_ = [("keys1", C.c_void_p), ("n1", C.c_int32), ("keys2", C.c_void_p), ("n2", C.c_int32), ("matches12", C.c_void_p)] + [(k, C.c_float) for k in ("fx", "fy", "cx", "cy")]


SIM3_EVENT_DTYPE = np.dtype([("iteration", "<i4"), ("n_inliers", "<i4"), ("R12", "<f4", 9), ("t12", "<f4", 3), ("s12", "<f4")])
PNP_RECORD_DTYPE = np.dtype([("iteration", "<i4"), ("n_inliers", "<i4"), ("Tcw_best", "<f4", 12), ("n_refined", "<i4"), ("refine_ok", "<i4"),
                             ("Tcw_refined", "<f4", 12)])
INIT_RESULT_DTYPE = np.dtype([("status", "<i4"), ("model", "<i4"), ("n_matches", "<i4"), ("score_h", "<f4"), ("score_f", "<f4"), ("rh", "<f4"), ("best_it_h", "<i4"),
                              ("best_it_f", "<i4"), ("H21", "<f4", 9), ("F21", "<f4", 9), ("n_inliers", "<i4"), ("n_good", "<i4", 8), ("cos_parallax", "<f4", 8),
                              ("parallax", "<f4", 8), ("best_hypothesis", "<i4"), ("second_best_good", "<i4"), ("R21", "<f4", 9), ("t21", "<f4", 3),
                              ("n_triangulated", "<i4")])


# ---- the vocabulary, the keyframe database, the covisibility graph ----
class _VocDesc(C.Structure):
    _fields_ = [("k", C.c_int32), ("L", C.c_int32), ("scoring", C.c_int32), ("weighting", C.c_int32), ("n_nodes", C.c_int32),
                ("parent", C.c_void_p), ("is_leaf", C.c_void_p), ("descriptor", C.c_void_p), ("weight", C.c_void_p)]


KFDB_STATE_DTYPE = np.dtype([("loop_query", "<u8"), ("loop_words", "<i4"), ("loop_score", "<f4"), ("reloc_query", "<u8"), ("reloc_words", "<i4"), ("reloc_score", "<f4")])


class LocalMap(C.Structure):
    """CorbLocalMap: what corb_track_update_local_map reports beside its lists"""
    _fields_ = [("n_kf", C.c_int32), ("n_voted", C.c_int32), ("n_mp", C.c_int32), ("ref_slot", C.c_int32), ("ref_id", C.c_uint64), ("counter_empty", C.c_int32), ("n_cleared", C.c_int32)]


class GbaPropagation(C.Structure):
    """CorbGbaPropagation: the counts of corb_gba_propagate_store"""
    _fields_ = [(k, C.c_int32) for k in ("n_popped", "n_reached", "n_propagated", "n_revisited", "n_points_set", "n_points_moved", "n_points_skipped")]


# ---- include/corb_voc_train.h ----
class VocTrainOptions(C.Structure):
    _fields_ = [("k", C.c_int32), ("L", C.c_int32), ("max_iterations", C.c_int32), ("reserved", C.c_int32), ("seed", C.c_uint64)]


class VocTrainStats(C.Structure):
    _fields_ = [(f, C.c_int32) for f in ("nodes", "words", "kmeans_nodes", "trivial_nodes", "short_nodes", "max_iterations_seen", "capped_nodes", "empty_cluster_events")] + \
               [(f, C.c_int32 * 10) for f in ("level_nodes", "level_max_iterations", "level_launches", "level_small_nodes", "level_large_nodes")] + \
               [("launches", C.c_int32), ("small_limit", C.c_int32), ("elapsed_ms", C.c_double)]

    def as_dict(self):
        return dict((f, list(getattr(self, f)) if f.startswith("level_") else getattr(self, f)) for f, _ in self._fields_)


# ---- include/corb_map_publish.h ----
KF_POSE_PACKET_DTYPE = np.dtype([("id", "<u8"), ("Tcw", "<f4", 16)])
MP_POSE_PACKET_DTYPE = np.dtype([("id", "<u8"), ("pos", "<f4", 3), ("pad", "<u4")])
PUBLISH_TRANSFORM_DTYPE = np.dtype([("client_id", "<i4"), ("pad", "<i4"), ("T", "<f4", 16), ("Tinv", "<f4", 16)])
PUBLISH_HEADER_DTYPE = np.dtype([("status", "<i4"), ("kf_record_bytes", "<i4"), ("mp_record_bytes", "<i4"), ("counts", "<i4", 5)])


class _PublishOutputs(C.Structure):
    _fields_ = [("kind_kf_new", C.c_void_p), ("kind_mp_new", C.c_void_p), ("kind_kf_upd", C.c_void_p), ("kind_mp_upd", C.c_void_p), ("kf_new_slots", C.c_void_p),
                ("mp_new_slots", C.c_void_p), ("n_kf_inserted", C.c_int32), ("n_mp_inserted", C.c_int32), ("n_kf_updated", C.c_int32), ("n_mp_updated", C.c_int32),
                ("no_transform", C.c_int32)]


class _PublishPack(C.Structure):
    _fields_ = [("kf", C.c_void_p), ("new_kf_slots", C.c_void_p), ("n_new_kf", C.c_int32), ("upd_kf_slots", C.c_void_p), ("n_upd_kf", C.c_int32),
                ("mp", C.c_void_p), ("new_mp_slots", C.c_void_p), ("n_new_mp", C.c_int32), ("upd_mp_slots", C.c_void_p), ("n_upd_mp", C.c_int32),
                ("trans_client_id", C.c_void_p), ("trans", C.c_void_p), ("n_trans", C.c_int32)]


class _PublishApply(C.Structure):
    _fields_ = [("client_id", C.c_int32), ("dst_kf", C.c_void_p), ("kf_first", C.c_int32), ("kf_n", C.c_int32), ("kf_free_first", C.c_int32), ("kf_room", C.c_int32),
                ("dst_mp", C.c_void_p), ("mp_first", C.c_int32), ("mp_n", C.c_int32), ("mp_free_first", C.c_int32), ("mp_room", C.c_int32), ("apply", C.c_int32),
                ("out", C.POINTER(_PublishOutputs))]


# ---- include/corb_essential_graph.h ----
class _EssentialGraphInput(C.Structure):
    _fields_ = [("loop_slot", C.c_int32), ("cur_slot", C.c_int32), ("n_corr", C.c_int32), ("n_lc", C.c_int32), ("corr_slots", C.c_void_p), ("corrected", C.c_void_p),
                ("non_corrected", C.c_void_p), ("lc_kf", C.c_void_p), ("lc_offset", C.c_void_p), ("lc_slots", C.c_void_p), ("min_weight", C.c_int32), ("pad", C.c_int32)]


class EssentialGraphCounts(C.Structure):
    """CorbEssentialGraphCounts; n_kind: loop connection, tree, loop edge, covisibility; n_suppressed: parent, child, loop edge, bad, not of smaller id, inserted"""
    _fields_ = [("n_vertices", C.c_int32), ("n_edges", C.c_int32), ("n_kind", C.c_int32 * 4), ("n_dropped", C.c_int32), ("n_lc_below_weight", C.c_int32),
                ("n_suppressed", C.c_int32 * 6)]

    def as_dict(self):
        return dict(n_vertices=self.n_vertices, n_edges=self.n_edges, n_kind=list(self.n_kind), n_dropped=self.n_dropped, n_lc_below_weight=self.n_lc_below_weight,
                    n_suppressed=list(self.n_suppressed))


class EssentialGraphResult(C.Structure):
    _fields_ = [("graph", EssentialGraphCounts), ("iters_done", C.c_int32), ("n_poses_set", C.c_int32), ("n_points_moved", C.c_int32), ("n_points_kept", C.c_int32),
                ("n_points_skipped", C.c_int32), ("n_points_fixed_ref", C.c_int32)]


# ---- include/corb_stereo_rectify.h ----
class RectifyEye(C.Structure):
    _fields_ = [("K", C.c_double * 9), ("D", C.c_double * 8), ("R", C.c_double * 9), ("P", C.c_double * 12)]


class RectifyConfig(C.Structure):
    _fields_ = [("raw_width", C.c_int32), ("raw_height", C.c_int32), ("left", RectifyEye), ("right", RectifyEye)]


# every C struct of the headers under its C name: the mirror whose size (and, where the field names agree, offsets) must equal the compiler's
STRUCTS = {
    "CorbOrbConfig": OrbConfig, "CorbStereoConfig": StereoConfig, "CorbStereoFrameLayout": StereoFrameLayout, "CorbStereoFrameTiming": StereoFrameTiming,
    "CorbCameraConfig": CameraConfig, "CorbRgbdFrameLayout": RgbdFrameLayout, "CorbKernelTime": KernelTime, "CorbFeatVec": _FeatVec, "CorbBowSide": _BowSide,
    "CorbTriSide": _TriSide, "CorbFrameView": _FrameView, "CorbKeyFrameView": _KeyFrameView, "CorbBAProblem": _BAProblem, "CorbBAResult": _BAResult,
    "CorbBAOptions": BAOptions, "CorbBAStage": BAStage, "CorbPoseOptFrame": _PoseOptFrame, "CorbSim3Problem": _Sim3Problem, "CorbMapPush": _MapPush,
    "CorbRcclFns": _RcclFns, "CorbTrackCamera": TrackCamera, "CorbNewPointSide": _NewPointSide, "CorbSim3RansacProblem": _Sim3RansacProblem,
    "CorbPnPRansacProblem": _PnPRansacProblem, "CorbInitProblem": _InitProblem, "CorbVocDesc": _VocDesc, "CorbLocalMap": LocalMap, "CorbGbaPropagation": GbaPropagation,
    "CorbVocTrainOptions": VocTrainOptions, "CorbVocTrainStats": VocTrainStats, "CorbPublishOutputs": _PublishOutputs, "CorbPublishPack": _PublishPack,
    "CorbPublishApply": _PublishApply, "CorbEssentialGraphInput": _EssentialGraphInput, "CorbEssentialGraphCounts": EssentialGraphCounts,
    "CorbEssentialGraphResult": EssentialGraphResult, "CorbRectifyEye": RectifyEye, "CorbRectifyConfig": RectifyConfig,
}
DTYPES = {
    "CorbKeyPoint": KP_DTYPE, "CorbTrackedPoint": TRACKED_DTYPE, "CorbLastPoint": LAST_DTYPE, "CorbMapPointView": MP_DTYPE, "CorbBAEdge": EDGE_DTYPE,
    "CorbKeyFrameMeta": KF_META_DTYPE, "CorbMapPointRecord": MP_RECORD_DTYPE, "CorbMapPointCounters": MP_COUNTERS_DTYPE, "CorbMapPointScratch": MP_SCRATCH_DTYPE,
    "CorbPushHeader": PUSH_HEADER_DTYPE, "CorbPushMsg": PUSH_MSG_DTYPE, "CorbSim3RansacEvent": SIM3_EVENT_DTYPE, "CorbPnPRansacRecord": PNP_RECORD_DTYPE,
    "CorbInitResult": INIT_RESULT_DTYPE, "CorbKfDbState": KFDB_STATE_DTYPE, "CorbKeyFramePosePacket": KF_POSE_PACKET_DTYPE,
    "CorbMapPointPosePacket": MP_POSE_PACKET_DTYPE, "CorbPublishTransform": PUBLISH_TRANSFORM_DTYPE, "CorbPublishHeader": PUBLISH_HEADER_DTYPE,
}
NOT_MIRRORED = ()               # (C struct name, one-line reason) of a header struct that has no mirror here: none today


def _prototypes():
    """{header: {function: (restype, argtypes)}} in the headers' grouping.  A bare list stands for a function that returns int."""
    P, I, F, D, STR, SZ = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_char_p, C.c_size_t
    I32, U32, I64, U64, ptr = C.c_int32, C.c_uint32, C.c_int64, C.c_uint64, C.POINTER
    PI, PP, CAM, KFV, destroy = ptr(I), ptr(P), ptr(TrackCamera), ptr(_KeyFrameView), (None, [P])
    table = {
        "corb_accel.h": {
            "corb_last_error": (STR, []), "corb_device_count": [], "corb_version": [], "corb_abi_version": [], "corb_warmup": [I], "corb_release_scratch": [I, ptr(U64)],
            "corb_pinned_alloc": [SZ, PP], "corb_pinned_free": [P],
            "corb_orb_create": [ptr(OrbConfig), PP], "corb_orb_destroy": destroy, "corb_orb_extract": [P, P, I, I, I, P, P, I, PI], "corb_orb_tables": [P] * 7,
            "corb_orb_pyramid_level": [P, I, I, I, P, SZ, PI, PI],
            "corb_orb_upload": [P, I, P, I], "corb_orb_run": [P, I], "corb_orb_sync": [P], "corb_orb_fetch": [P, I, P, P, I, PI], "corb_orb_fetch_candidates": [P, I, I, P, I, PI],
            "corb_orb_device_image": [P, I, PP, ptr(SZ)], "corb_orb_upload_batch": [P, I, I, P], "corb_orb_capacity": [P], "corb_orb_fetch_batch": [P, I, I, P, P, P],
            "corb_stereo_upload_batch": [P, I, I, P], "corb_stereo_fetch_matches_batch": [P, I, I, P, P, P], "corb_orb_profile": [P, I],
            "corb_orb_profile_read": [P, ptr(KernelTime), I, PI],
            "corb_stereo_create": [ptr(StereoConfig), PP], "corb_stereo_destroy": destroy, "corb_stereo_orb": (P, [P]), "corb_stereo_upload": [P, I, P, P, I], "corb_stereo_run": [P, I],
            "corb_stereo_sync": [P], "corb_stereo_fetch_matches": [P, I, P, P, I, PI, PI], "corb_stereo_frame_layout": [P, ptr(StereoFrameLayout)], "corb_stereo_frames": [P, I, P, P, P],
            "corb_track_search_reloc": [P, I, P, I, P, CAM, P, F, F, I, I, P, P], "corb_search_by_sim3_store": [P, I, I, P, CAM, F, P, P, P, F, P, P, F, P, P, P],
            "corb_mp_store_set_counters": [P, I, I, P], "corb_mp_store_get_counters": [P, I, I, P], "corb_mp_store_set_scratch": [P, I, I, P], "corb_mp_store_get_scratch": [P, I, I, P],
            "corb_mp_store_replace": [P, I, I, P, I, I, P],
            "corb_descriptor_distance": [P, P, I, P, I], "corb_search_by_bow": [I, ptr(_BowSide), ptr(_BowSide), F, I, P, PI, I],
            "corb_search_for_triangulation": [ptr(_TriSide), ptr(_TriSide), P, F, F, P, P, I, I, I, P, PI, I], "corb_ba_solve": [ptr(_BAProblem), I, I, P, ptr(_BAResult), I],
            "corb_ba_solve_ex": [ptr(_BAProblem), I, I, P, ptr(_BAResult), I, ptr(BAOptions)],
            "corb_ba_solve_staged": [ptr(_BAProblem), ptr(BAStage), I, P, ptr(_BAResult), P, I, ptr(BAOptions)],
            "corb_search_by_projection_map": [ptr(_FrameView), P, P, I, F, F, P, PI, I],
            "corb_search_by_projection_frame": [ptr(_FrameView), P, P] + [F] * 6 + [P, P, I, F, I, I, P, PI, I], "corb_pose_optimization_batch": [ptr(_PoseOptFrame), I, P, P, P, I],
            "corb_search_by_projection_reloc": [KFV, P, P, P, P, I, F, I, I, P, PI, I], "corb_search_by_projection_scw": [KFV, P, P, P, P, I, F, P, PI, I],
            "corb_search_for_initialization": [ptr(_FrameView), ptr(_FrameView), P, I, F, I, P, PI, I], "corb_fuse": [KFV, P, P, I, P, P, I, F, P, P, PI, I],
            "corb_search_by_sim3": [KFV, KFV] + [P] * 6 + [F, P, P, F, P, PI, I], "corb_distinctive_descriptors": [P, P, I, P, I], "corb_rebase_map": [P, P, I, P, I, I],
            "corb_optimize_sim3": [ptr(_Sim3Problem), I, P, P, P, F, I, P, P, P, I], "corb_optimize_essential_graph": [I, P, P, I, P, P, P, I, I, P, I, P, P, P, ptr(I32), I],
            "corb_kf_store_create": [I, I, I, PP], "corb_kf_store_destroy": destroy, "corb_kf_store_record_bytes": [P], "corb_kf_store_put_from_stereo": [P, I, P, I, U64],
            "corb_kf_store_put_host": [P, I, P, P, P, P, I, U64], "corb_kf_store_set_bow": [P, I, ptr(_FeatVec)],
            "corb_kf_store_set_flags": [P, I, P], "corb_kf_store_get": [P, I] + [P] * 5 + [I, PI, ptr(U64), P, P, P, ptr(I32)], "corb_search_by_bow_slots": [I, P, I, P, I, F, I, P, PI],
            "corb_search_for_triangulation_slots": [P, I, P, I, P, F, F, P, P, I, I, I, P, PI],
            "corb_comm_unique_id": [P], "corb_comm_create": [P, I, I, I, PP], "corb_comm_destroy": destroy, "corb_map_push": [P, P, P, I, I, P, P],
            "corb_kf_store_set_meta": [P, I, P], "corb_kf_store_get_meta": [P, I, P], "corb_kf_store_set_map_points": [P, I, P], "corb_kf_store_get_map_points": [P, I, P, I],
            "corb_mp_store_create": [I, I, I, PP], "corb_mp_store_destroy": destroy, "corb_mp_store_record_bytes": [P], "corb_mp_store_put_host": [P, I, I, P, P, P, P],
            "corb_mp_store_get": [P, I, I, P, P, P],
            "corb_comm_create_local": [I, P, P], "corb_comm_rank": [P], "corb_comm_world": [P], "corb_map_push_ex": [P, ptr(_MapPush), I], "corb_map_push_plan": [I, I, P, I, I, P, P, PI],
            "corb_map_push_messages": [I, I, I, P, P, P, P, PI, P, PI], "corb_comm_test_rccl_exchange": [ptr(_RcclFns), P, I, P, I], "corb_map_push_setup": [P, I, P, P, P, P],
            "corb_map_push_begin": [P, ptr(_MapPush), I], "corb_map_push_wait": [P], "corb_rebase_map_store": [P, P, P, I, P, P, I],
            "corb_ba_solve_store": [P, P, I, P, P, I, I, I, P, U64, ptr(_BAResult), ptr(BAOptions)],
            "corb_local_ba_store": [P, P, I, I, P, P, I, ptr(BAStage), I, F, I, P, ptr(_BAResult), P, I, PI, ptr(BAOptions)],
            "corb_fuse_store": [P, I, P, P, I, CAM, P, F, F, I, P, P, P, PI], "corb_search_by_projection_scw_store": [P, I, P, P, I, CAM, P, F, F, P, P, PI],
            "corb_ba_solve_devflat": [ptr(_BAProblem), I, I, ptr(_BAResult), I, ptr(BAOptions)], "corb_kf_store_put_batch": [P, I, I] + [P] * 7, "corb_spd_solve": [P, I, P, P, PI, I],
            "corb_mp_store_build_index": [P, I, I], "corb_kf_store_count": [P, I], "corb_track_search_last_frame": [P, I, I, P, P, P, CAM, F, I, F, I, P, PI],
            "corb_track_pose_optimization": [P, I, P, CAM, P, P, I, P, ptr(I32)], "corb_track_search_local_points": [P, I, P, P, I, CAM, P, F, F, F, P, P, PI, PI],
            "corb_kf_store_put_frame": [P, I, P, P, P, P, I, P],
            "corb_rgbd_create": [ptr(CameraConfig), PP], "corb_rgbd_destroy": destroy, "corb_rgbd_orb": (P, [P]), "corb_rgbd_upload_batch": [P, I, I, P], "corb_rgbd_run": [P, I],
            "corb_rgbd_sync": [P], "corb_rgbd_fetch_batch": [P, I, I] + [P] * 6,
            "corb_rgbd_frame_layout": [P, ptr(RgbdFrameLayout)], "corb_rgbd_frames": [P, I, P, P, P], "corb_rgbd_image_bounds": [P, P], "corb_kf_store_put_from_rgbd": [P, I, P, I, U64],
            "corb_triangulate_pairs": [ptr(_NewPointSide), ptr(_NewPointSide), P, I, P, P, P, PI, I],
            "corb_create_new_map_points_store": [P, I, P, I, P, P, CAM, I, I, P, I, U64, I32, P, P, P, P, P, PI],
            "corb_sim3_ransac": [P, I, D, I, I, I, P, I, I] + [P] * 6 + [I], "corb_sim3_ransac_store": [P, I, P, I, P, CAM, P, P, D, I, I, I, P, I] + [P] * 8,
            "corb_pnp_ransac": [P, I, D, I, I, I, F, F, I, P, I, I] + [P] * 9 + [I], "corb_pnp_ransac_store": [P, I, P, CAM, P, I, D, I, I, I, F, F, I, P, I] + [P] * 11,
            "corb_mono_initialize": [P, I, F, I, F, I, P, I, I] + [P] * 6 + [I],
            "corb_voc_create": [ptr(_VocDesc), I, PP], "corb_voc_load_text": [STR, I, PP], "corb_voc_destroy": destroy, "corb_voc_info": [P] + [ptr(I32)] * 4,
            "corb_voc_transform": [P, P, P, I, I] + [P] * 9, "corb_kf_store_compute_bow": [P, P, I, P, I, P, P],
            "corb_kfdb_create": [P, I, I, PP], "corb_kfdb_destroy": destroy, "corb_kfdb_set_bow": [P, I, P, P, I], "corb_kfdb_get_bow": [P, I, P, P, I, PI], "corb_kfdb_add": [P, I],
            "corb_kfdb_erase": [P, I], "corb_kfdb_clear": [P], "corb_kfdb_set_neighbours": [P, P, I, P],
            "corb_kfdb_get_state": [P, I, I, P], "corb_kfdb_score": [P, I, P, I, P], "corb_kfdb_detect": [P, I, I, U64, P, I, F, P, I, PI], "corb_bow_profile": [I, I],
            "corb_bow_profile_read": [P, I, PI],
            "corb_covis_create": [P, P, I, PP], "corb_covis_destroy": destroy, "corb_covis_update": [P, P, I, I, P], "corb_covis_erase": [P, I],
            "corb_covis_get": [P, I, P, P, PI, P, P, PI, I], "corb_covis_query": [P, I, I, I, P, P, I, PI], "corb_covis_weight": [P, I, I, PI],
            "corb_covis_keyframe_culling": [P, I, I, F, P, P, P, P, I, PI], "corb_covis_local_window": [P, I, P, I, PI, PI, P, I, PI],
            "corb_covis_set_tree": [P, I, U64, I, P, I], "corb_covis_get_tree": [P, I, ptr(U64), PI, P, I, PI], "corb_covis_add_child": [P, I, I], "corb_covis_erase_child": [P, I, I],
            "corb_covis_change_parent": [P, I, I], "corb_covis_reparent_children": [P, I, PI, PI],
            "corb_track_update_local_map": [P, P, I, P, I, P, I, P, P, I, ptr(LocalMap)],
            "corb_loop_correct_store": [P, I, P, F, P, P, P, I, PI, PI], "corb_fuse_sim3_store": [P, I, P, P, I, CAM, P, F, F, I, P, P, P, P, PI],
            "corb_gba_propagate_store": [P, P, I, U64, I, ptr(GbaPropagation)], "corb_covis_set_pose_before_gba": [P, I, P], "corb_covis_get_pose_before_gba": [P, I, P],
            "corb_scratch_fill": [I, I, U32, U64, ptr(U64)], "corb_scratch_report": [I, I, ptr(U64), PI, ptr(U64)], "corb_scratch_read": [I, I, U64, U64, P],
        },
        # vocabulary training and export, an offline tool beside the drop-in boundary (exported from the same library)
        "corb_voc_train.h": {
            "corb_voc_train": [P, P, I, ptr(VocTrainOptions), I, PP, ptr(VocTrainStats)], "corb_voc_train_store": [P, P, I, ptr(VocTrainOptions), PP, ptr(VocTrainStats)],
            "corb_voc_get": [P, P, P, P, P, I, PI], "corb_voc_save_text": [P, STR, I],
        },
        # keyframe insertion on records
        "corb_keyframe_insert.h": {
            "corb_kfi_create": [I, I, I, PP], "corb_kfi_destroy": destroy,
            "corb_kfi_create_stereo_points": [P, P, I, P, CAM, F, I, I, I, U64, I32, I64, P, I, P, P, P, PI, PI],
            "corb_kfi_need_keyframe_counts": [P, P, I, P, F, P, I, I, I, I, PI, PI, PI], "corb_kfi_process_new_keyframe": [P, P, I, P, I, I, F, I, P, P, PI, PI],
            "corb_kfi_map_point_culling": [P, P, P, I, U64, I, P, I, I, I, P, P, PI, PI],
        },
        # the server -> clients publish on records
        "corb_map_publish.h": {
            "corb_pub_create": [I, PP], "corb_pub_destroy": destroy, "corb_pub_message_layout": [P, I, I, P], "corb_pub_pack": [P, P, P, I, P, I, P, P, I, P, I, P, P, I],
            "corb_pub_message": [P, PP, ptr(I64), P, ptr(I32), ptr(I32)], "corb_pub_message_read": [P, P, I64],
            "corb_pub_apply": [P, P, P, I, I, I32, P, I, I, I, I, P, I, I, I, I, I, ptr(_PublishOutputs)],
            "corb_map_publish_plan": [I, I, P, PI], "corb_map_publish_messages": [I, I, I, P, P, PI, P, PI], "corb_map_publish": [P, P, I, ptr(_PublishPack), ptr(_PublishApply)],
        },
        # the essential graph on records
        "corb_essential_graph.h": {
            "corb_covis_add_loop_edge": [P, I, I], "corb_covis_get_loop_edges": [P, I, P, I, PI], "corb_covis_clear_loop_edges": [P, I],
            "corb_essential_graph_plan": [P, ptr(_EssentialGraphInput), I, I] + [P] * 8 + [ptr(EssentialGraphCounts)],
            "corb_essential_graph_store": [P, ptr(_EssentialGraphInput), I, I, F, P, P, I, ptr(EssentialGraphResult)],
        },
        # stereo rectification in front of the stereo front-end
        "corb_stereo_rectify.h": {
            "corb_rect_create": [ptr(RectifyConfig), P, PP], "corb_rect_destroy": destroy, "corb_rect_maps": [P, I, P, P], "corb_rect_set_maps": [P, I, P, P],
            "corb_rect_upload_batch": [P, I, I, P], "corb_rect_frames": [P, I, P, P, P],
        },
    }
    return dict((h, dict((n, v if isinstance(v, tuple) else (I, v)) for n, v in fns.items())) for h, fns in table.items())


PROTOTYPES = _prototypes()
EXPORTS = list(PROTOTYPES["corb_accel.h"])
TRAIN_EXPORTS, KFINSERT_EXPORTS, PUBLISH_EXPORTS, ESSGRAPH_EXPORTS, RECTIFY_EXPORTS = (
    tuple(PROTOTYPES[h]) for h in ("corb_voc_train.h", "corb_keyframe_insert.h", "corb_map_publish.h", "corb_essential_graph.h", "corb_stereo_rectify.h"))


def bind(lib):
    """restype and argtypes of every PROTOTYPES entry onto the opened library `lib`.  CorbError: the library has another struct layout version, or lacks a function
    (named with its header)."""
    version = lib.corb_abi_version() if hasattr(lib, "corb_abi_version") else "< 5"
    if version != ABI_VERSION:
        raise CorbError("libcorb_accel.so was built from another corb_accel.h (struct layout version %s, this harness mirrors %d): rebuild it" % (version, ABI_VERSION))
    for header, fns in PROTOTYPES.items():
        for name, (restype, argtypes) in fns.items():
            if not hasattr(lib, name):
                raise CorbError("libcorb_accel.so lacks %s (include/%s): rebuild it" % (name, header))
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
    return lib


__all__ = [k for k in dict(globals()) if not k.startswith("__") and k not in ("C", "np", "_prototypes")]       # (the underscore mirrors are part of what the package re-exports)
