"""Registry of the C-ABI entry points that draw their device scratch from a workspace lane (csrc/corb_workspace.h), with one small case each, for
tests/test_gpu_workspace_states.py.

A lane's arena is a bump allocator that is only rewound between calls, and its page-locked staging is reused the same way: every call starts at the base address of
the call before it and finds that call's leftovers.  The library's rule is that a call reads no byte of the arena or the staging that it has not written itself.
The GPU test runs every entry on a fresh arena, a warm one and one filled with a bit pattern, and demands the same bytes back each time.

An entry's `body` is the body of the entry point's EXISTING GPU test -- the test function itself, called with one of its own cases (the smallest that still takes
the route), or a few lines that call its helpers where the function needs a pytest fixture.  So the reference and the bar of `check` are the existing test's own, by
construction; nothing is restated here.  The body runs against a recording stand-in of the package (Recorder):
  * every value a wrapper of corb-slam_amd/__init__.py returns -- whole arrays, counts, status codes, read-backs of the records -- is copied into the outputs, in call
    order (`run` returns everything the calls return; the timing fields of a BA result, which differ from run to run, are the one thing left out);
  * the C symbols the body really calls are noted, so that an entry cannot claim a symbol it does not reach;
  * in a dirty state the lane is filled again before EVERY call of a symbol that takes it, and looked at after the call: an entry of several calls shows each of them
    the pattern, not the leftovers of the call before.
`check(outputs)` raises what the existing assertions raised during that run, if anything.

LANE_SYMBOLS and NOT_ON_A_LANE partition the header's symbols (tests/test_workspace_cases.py): a new entry point forces a decision."""
import ctypes
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

FILL = 64 << 20
PATTERN_A = 0x00000001          # as an integer 1 (a plausible count, flag or index), as a float or double a denormal
PATTERN_B = 0x3F800000          # as a float 1.0, as a double about 0.0078: an accumulator, weight or score that starts from it goes visibly wrong
FIRST_MB = 1 << 20

# which lane a symbol takes: read off csrc/ (CorbScratch pool(0) / CovisCall: lane 0; ba_host.h: Pool and corb_graph.cpp: GPool: lane 1).  corb_optimize_sim3 is a
# short call and takes lane 0 (corb_sim3.cpp: DevPool = CorbScratch); corb_ba_solve_staged takes lane 1 except for a single free pose on the automatic solver, which
# it hands to the pose batch of lane 0 (corb_ba_staged.cpp -> pose_batch_run)
LANE_SYMBOLS = {
    0: frozenset("""corb_spd_solve corb_descriptor_distance corb_search_by_bow corb_search_for_triangulation corb_distinctive_descriptors corb_rebase_map
        corb_search_by_projection_map corb_search_by_projection_frame corb_search_for_initialization corb_search_by_projection_reloc corb_search_by_projection_scw corb_fuse
        corb_search_by_sim3 corb_pose_optimization_batch corb_optimize_sim3 corb_triangulate_pairs corb_create_new_map_points_store corb_sim3_ransac corb_sim3_ransac_store
        corb_pnp_ransac corb_pnp_ransac_store corb_mono_initialize corb_voc_transform corb_kf_store_compute_bow
        corb_kf_store_put_host corb_kf_store_put_frame corb_search_by_bow_slots corb_search_for_triangulation_slots corb_rebase_map_store corb_mp_store_replace
        corb_track_search_last_frame corb_track_pose_optimization corb_track_search_local_points corb_track_search_reloc corb_fuse_store corb_fuse_sim3_store
        corb_search_by_projection_scw_store corb_search_by_sim3_store
        corb_covis_update corb_covis_erase corb_covis_query corb_covis_weight corb_covis_keyframe_culling corb_covis_local_window corb_covis_set_tree corb_covis_get_tree
        corb_covis_add_child corb_covis_erase_child corb_covis_change_parent corb_covis_reparent_children corb_track_update_local_map
        corb_loop_correct_store corb_gba_propagate_store""".split()),
    1: frozenset("""corb_ba_solve corb_ba_solve_ex corb_ba_solve_devflat corb_ba_solve_staged corb_ba_solve_store corb_local_ba_store corb_optimize_essential_graph""".split()),
}
LANE_OF = {s: lane for lane, names in LANE_SYMBOLS.items() for s in names}

# everything else the header declares: handles and their own buffers (front-ends, stores, vocabulary, keyframe database, graph rows), plain copies, the communicator,
# and the calls on the lanes themselves (corb_warmup and the test aids take a lane's mutex but draw nothing from its arena)
NOT_ON_A_LANE = frozenset("""corb_last_error corb_device_count corb_version corb_abi_version corb_pinned_alloc corb_pinned_free
    corb_warmup corb_release_scratch corb_scratch_fill corb_scratch_report corb_scratch_read
    corb_orb_create corb_orb_destroy corb_orb_extract corb_orb_tables corb_orb_pyramid_level corb_orb_upload corb_orb_run corb_orb_sync corb_orb_fetch corb_orb_fetch_candidates
    corb_orb_device_image corb_orb_upload_batch corb_orb_capacity corb_orb_fetch_batch corb_orb_profile corb_orb_profile_read
    corb_stereo_create corb_stereo_destroy corb_stereo_orb corb_stereo_upload corb_stereo_run corb_stereo_sync corb_stereo_fetch_matches corb_stereo_upload_batch
    corb_stereo_fetch_matches_batch corb_stereo_frame_layout corb_stereo_frames
    corb_rgbd_create corb_rgbd_destroy corb_rgbd_orb corb_rgbd_upload_batch corb_rgbd_run corb_rgbd_sync corb_rgbd_fetch_batch corb_rgbd_frame_layout corb_rgbd_frames corb_rgbd_image_bounds
    corb_kf_store_create corb_kf_store_destroy corb_kf_store_record_bytes corb_kf_store_put_from_stereo corb_kf_store_put_from_rgbd corb_kf_store_put_batch corb_kf_store_set_bow
    corb_kf_store_set_flags corb_kf_store_get corb_kf_store_count corb_kf_store_set_meta corb_kf_store_get_meta corb_kf_store_set_map_points corb_kf_store_get_map_points
    corb_mp_store_create corb_mp_store_destroy corb_mp_store_record_bytes corb_mp_store_put_host corb_mp_store_get corb_mp_store_build_index
    corb_mp_store_set_counters corb_mp_store_get_counters corb_mp_store_set_scratch corb_mp_store_get_scratch
    corb_voc_create corb_voc_load_text corb_voc_destroy corb_voc_info corb_bow_profile corb_bow_profile_read
    corb_kfdb_create corb_kfdb_destroy corb_kfdb_set_bow corb_kfdb_get_bow corb_kfdb_add corb_kfdb_erase corb_kfdb_clear corb_kfdb_set_neighbours corb_kfdb_get_state
    corb_kfdb_score corb_kfdb_detect
    corb_covis_create corb_covis_destroy corb_covis_get corb_covis_set_pose_before_gba corb_covis_get_pose_before_gba
    corb_comm_unique_id corb_comm_create corb_comm_create_local corb_comm_destroy corb_comm_rank corb_comm_world corb_comm_test_rccl_exchange
    corb_map_push corb_map_push_ex corb_map_push_plan corb_map_push_messages corb_map_push_setup corb_map_push_begin corb_map_push_wait""".split())

_PROXIED = ("KeyFrameStore", "MapPointStore", "Covisibility", "Vocabulary", "KeyFrameDatabase", "ORBmatcher", "Optimizer", "Sim3Solver", "PnPsolver", "Initializer")
_TIMING_KEYS = ("ms", "ms_total")


class _Fn:
    """a C function of the library: fills the lane before the call where the state asks for it, notes the symbol, looks at the arena afterwards"""

    def __init__(self, rec, name, fn):
        self.__dict__.update(_rec=rec, _name=name, _fn=fn)

    def __call__(self, *a):
        self._rec.before(self._name)
        r = self._fn(*a)
        self._rec.after(self._name)
        return r

    def __getattr__(self, k):
        return getattr(self._fn, k)

    def __setattr__(self, k, v):                     # (argtypes / restype set by a wrapper)
        setattr(self._fn, k, v)


class _Lib:
    def __init__(self, rec, lib):
        self.__dict__.update(_rec=rec, _lib=lib)

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        return _Fn(self._rec, name, f) if name in LANE_OF else f


class _Inst:
    """an object of the package (a store, the graph, a matcher ...): method calls are forwarded with their results recorded"""

    def __init__(self, rec, obj, name):
        self.__dict__.update(_rec=rec, _obj=obj, _name=name)

    def __getattr__(self, k):
        a = getattr(self._obj, k)
        return self._rec.wrap("%s.%s" % (self._name, k), a) if isinstance(a, (types.MethodType, types.FunctionType)) else a

    def __setattr__(self, k, v):
        setattr(self._obj, k, v)


class _Cls:
    def __init__(self, rec, cls):
        self.__dict__.update(_rec=rec, _cls=cls)

    def __call__(self, *a, **kw):
        return _Inst(self._rec, self._cls(*_unwrap(a), **_unwrap(kw)), self._cls.__name__)

    def __getattr__(self, k):
        a = getattr(self._cls, k)
        return self._rec.wrap("%s.%s" % (self._cls.__name__, k), a) if callable(a) and not isinstance(a, type) else a


class _Pkg:
    def __init__(self, rec, pkg):
        self.__dict__.update(_rec=rec, _pkg=pkg)

    def __getattr__(self, k):
        a = getattr(self._pkg, k)
        if isinstance(a, type):
            return _Cls(self._rec, a) if k in _PROXIED else a
        if isinstance(a, types.FunctionType) and k != "load" and not k.startswith("_"):
            return self._rec.wrap(k, a)
        return a                                     # (load is replaced in the module itself while a body runs: see Recorder.run)


def _unwrap(x):
    if isinstance(x, _Inst):
        return x._obj
    if isinstance(x, (list, tuple)):
        return type(x)(_unwrap(v) for v in x)
    if isinstance(x, dict):
        return {k: _unwrap(v) for k, v in x.items()}
    return x


def _flatten(prefix, x, out):
    if x is None or isinstance(x, _Inst):
        return
    if isinstance(x, (np.ndarray, np.generic)):
        out[prefix] = np.array(x, copy=True)
    elif isinstance(x, (bool, int, float)):
        out[prefix] = np.array(x)
    elif isinstance(x, (str, bytes)):
        out[prefix] = np.frombuffer(x.encode() if isinstance(x, str) else x, np.uint8).copy()
    elif isinstance(x, (list, tuple)):
        out[prefix + ".len"] = np.array(len(x))
        for i, v in enumerate(x):
            _flatten("%s[%d]" % (prefix, i), v, out)
    elif isinstance(x, dict):
        for k in sorted(x, key=str):
            if k not in _TIMING_KEYS:
                _flatten("%s.%s" % (prefix, k), x[k], out)
    elif isinstance(x, ctypes.Structure):
        for f in x._fields_:
            _flatten("%s.%s" % (prefix, f[0]), getattr(x, f[0]), out)
    elif isinstance(x, ctypes.Array):
        out[prefix] = np.array(list(x))
    else:
        raise TypeError("workspace_cases: %s returned a %s, which the recorder cannot hold" % (prefix, type(x).__name__))


class Outputs(dict):
    """the output arrays of one run, in call order; `error` is what the body's own assertions raised during that run (None: they all passed)"""
    error = None


class Recorder:
    """one run of a body: the outputs, the symbols it called, and (dirty state) the fill before and the look after every call on a lane"""

    def __init__(self, pkg, word=None, fill=FILL):
        self.pkg = pkg; self.word = word; self.fill = fill
        self.lib = _Lib(self, pkg.load())
        self.out = Outputs(); self.seq = 0; self.called = set(); self.problems = []; self.filled = {}; self.written = {}; self.depth = 0

    def wrap(self, name, fn):
        def call(*a, **kw):
            self.depth += 1
            try:
                r = fn(*_unwrap(a), **_unwrap(kw))
            finally:
                self.depth -= 1
            for c in _PROXIED:
                if isinstance(r, getattr(self.pkg, c)):
                    return _Inst(self, r, c)
            if self.depth == 0:                      # (a wrapper that calls another wrapper: the outer result holds the inner one)
                _flatten("%04d %s" % (self.seq, name), r, self.out); self.seq += 1
            return r
        return call

    def record(self, name, value):
        _flatten("%04d %s" % (self.seq, name), value, self.out); self.seq += 1

    # Both lanes are filled and looked at around every call: corb_ba_solve_staged runs a single free pose through the pose batch of lane 0 and everything else on
    # lane 1, and a call on records may come to either; which lane a call wrote into is what the look afterwards finds.
    def before(self, sym):
        self.called.add(sym)
        if self.word is not None:
            for lane in (0, 1):
                self.filled[lane] = self.pkg.scratch_fill(lane, self.word, self.fill)

    def after(self, sym):
        if self.word is None:
            return
        for lane in (0, 1):
            cap, chunks, _ = self.pkg.scratch_report(lane)
            if (cap, chunks) != (self.filled[lane], 1):
                self.problems.append("%s left lane %d with %d chunk(s) of %d bytes in all: it took memory outside the %d filled bytes (raise the entry's fill)"
                                     % (sym, lane, chunks, cap, self.filled[lane]))
                continue
            head = self.pkg.scratch_read(lane, 0, FIRST_MB).view(np.uint32)
            if (head != np.uint32(self.word)).any():
                self.written.setdefault(lane, set()).add(sym)

    def run(self, body, synth, pyorc):
        """-> the outputs, with the exception the body's own assertions raised (or None) as their `error`"""
        real_load = self.pkg.load
        self.pkg.load = lambda: self.lib
        try:
            body(_Pkg(self, self.pkg), synth, pyorc)
        except Exception as e:                       # (an assertion of the existing test, or a call that failed: `check` raises it)
            self.out.error = e
        finally:
            self.pkg.load = real_load
        return self.out


class Entry:
    def __init__(self, name, lane, symbols, body, bigger=None, fill=FILL):
        self.name, self.lane, self.symbols, self.body, self.bigger, self.fill = name, lane, tuple(symbols.split()), body, bigger, fill

    def run(self, corb, synth, pyorc, word=None, body=None):
        """run(corb, synth, pyorc) -> dict of output arrays.  word: the pattern the entry's lanes are filled with before every call on them (None: as they are).
        The recorder of the run stays in self.last (the symbols called, what the looks at the arena found)."""
        self.last = Recorder(corb, word, self.fill)
        return self.last.run(body or self.body, synth, pyorc)

    def check(self, outputs):
        """the existing test's own assertions on the run that produced `outputs`"""
        if outputs.error is not None:
            raise outputs.error


def same_bytes(a, b):
    """the first difference between two outputs (None: byte for byte equal, array by array, NaN by bit pattern)"""
    if list(a) != list(b):
        only = sorted(set(a) ^ set(b))
        return "the runs returned different things: %s" % (only[:6] if only else "the same outputs in another order")
    for k in a:
        x, y = a[k], b[k]
        if x.dtype != y.dtype or x.shape != y.shape:
            return "%s: %s %s against %s %s" % (k, x.dtype, x.shape, y.dtype, y.shape)
        if x.tobytes() != y.tobytes():
            xb = np.frombuffer(x.tobytes(), np.uint8); yb = np.frombuffer(y.tobytes(), np.uint8)
            return "%s: %d of %d bytes differ, the first at byte %d" % (k, int((xb != yb).sum()), len(xb), int(np.nonzero(xb != yb)[0][0]))
    return None


# ================================================================ the bodies ================================================================
import test_gpu_random_ba as RB  # noqa: E402
import test_gpu_random_loop as RL  # noqa: E402
import test_gpu_random_matchers as RM  # noqa: E402
import test_gpu_random_records as RC  # noqa: E402


def _smallest(cases, key, **want):
    return min((c for c in cases if all(c[k] == v for k, v in want.items())), key=key)


def _case(fn, c):
    return lambda corb, synth, pyorc: fn(corb, pyorc, synth, c)


def _case_np(fn, c):                                 # (the tests that take no synth)
    return lambda corb, synth, pyorc: fn(corb, pyorc, c)


# ---- lane 1: bundle adjustment and the essential graph ----
def ba_case_for(route, devflat=False):
    """the smallest member of RB.BA_CASES that takes `route` (by keyframes x points per keyframe), the open case left out"""
    return _smallest([c for c in RB.BA_CASES if c["i"] not in RB.BA_OPEN], lambda c: (c["free"] * c["ppk"], c["i"]), route=route, devflat=devflat)


BA_ROUTE_CASES = {r: ba_case_for(r) for r in (RB.FUSED, RB.LDS, RB.DENSE, RB.PCG, RB.PCG_ROW, RB.PCG_ML)}
BA_DEVFLAT_CASE = _smallest(RB.BA_CASES, lambda c: (c["free"] * c["ppk"], c["i"]), devflat=True)
WINDOW_HOST_CASE, WINDOW_DEVICE_CASE = RB.WINDOW_CASES[0], RB.WINDOW_CASES[2]       # 2 047 edges: both orders on the host route; 2 049 active edges: grouped on the device


def _ba_solve_plain(corb, synth, pyorc):
    """corb_ba_solve (the call without options) on the fused case: the same reference and bars as RB.test_global_ba_random_case"""
    import ctypes as C
    c = BA_ROUTE_CASES[RB.FUSED]; p = RB.ba_case_problem(synth, c)
    poses = np.ascontiguousarray(p["poses"], np.float32).reshape(-1, 16); points = np.ascontiguousarray(p["points"], np.float32).reshape(-1, 3)
    pf = np.ascontiguousarray(p["pose_fixed"], np.uint8); qf = np.ascontiguousarray(p["point_fixed"], np.uint8); edges = np.ascontiguousarray(p["edges"], corb.EDGE_DTYPE)
    prob = corb._BAProblem(len(poses), len(points), len(edges), corb._p(poses), corb._p(pf), corb._p(points), corb._p(qf), corb._p(edges), p["fx"], p["fy"], p["cx"], p["cy"], p["bf"], None)
    oposes = np.zeros_like(poses); opoints = np.zeros_like(points); chi2 = np.zeros(11, np.float64); lam = np.zeros(10, np.float64)
    res = corb._BAResult(corb._p(oposes), corb._p(opoints), corb._p(chi2), corb._p(lam), 0, 0, 0, 0, 0, 0, 0, 0, 0)
    rc = corb.load().corb_ba_solve(C.byref(prob), 10, int(c["robust"]), None, C.byref(res), 0)
    g = dict(rc=rc, poses=oposes.reshape(-1, 4, 4), points=opoints, chi2=chi2[: res.iters_done + 1], lam=lam[: res.iters_done], iters_done=res.iters_done, trials=res.trials_total)
    corb._rec.record("corb_ba_solve", g)
    r = pyorc.ba_solve(*RB._args(p), iters=10, robust=c["robust"])
    assert rc == 0 and g["iters_done"] == r["iters_done"] and g["trials"] == r["trials"]
    assert np.allclose(g["chi2"], r["chi2"], rtol=RB.RTOL) and RB._near(g, r)


def _ba_store(corb, synth, pyorc):
    import test_gpu_local_ba_store as T
    T.test_global_ba_on_records_update_normal_and_depth(corb, pyorc, synth)


def _local_ba_store(seed, ppk):
    def body(corb, synth, pyorc):
        import test_gpu_local_ba_store as T
        T.test_local_ba_on_records_matches_the_oracle_on_map_objects(corb, pyorc, synth, seed, ppk)
    return body


# ---- lane 0 ----
def _spd_97(corb, synth, pyorc):
    """tests/test_gpu_ba.py::test_dense_spd_solver at n = 97 (one more than a tile and a half: the identity tail of the last diagonal block is in use)"""
    rng = np.random.default_rng(77); n = 97
    M = rng.normal(size=(n, n + 8)); A = M @ M.T + 0.5 * np.eye(n); b = rng.normal(size=n)
    Au = A.copy(); Au[np.triu_indices(n, 1)] = np.nan
    x, info = corb.spd_solve(Au, b)
    ref = np.linalg.solve(A, b)
    assert info == 0 and np.abs(x - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())
    A = np.eye(70); A[40, 40] = -1.0
    assert corb.spd_solve(A, np.ones(70))[1] == 41


def _kfproj(name, *args, with_matcher=True):
    def body(corb, synth, pyorc):
        import test_gpu_kfproj as T
        getattr(T, name)(corb.ORBmatcher(0.6, True) if with_matcher else corb, pyorc, synth, *args)
    return body


def _module_test(module, name, *args, order="cps"):
    """a test function of another GPU test module: order names its leading arguments (c = corb, p = pyorc, s = synth)"""
    def body(corb, synth, pyorc):
        T = __import__(module)
        getattr(T, name)(*[dict(c=corb, p=pyorc, s=synth)[o] for o in order], *args)
    return body


def _triangulate_pairs(n_pairs):
    def body(corb, synth, pyorc):
        import newpoints_reference as NP
        import test_gpu_newpoints as T
        T.test_triangulate_pairs(corb, NP.mixed_pairs(11, 257), n_pairs)
    return body


def _create_new_map_points(corb, synth, pyorc):
    import newpoints_reference as NP
    import test_gpu_newpoints as T
    cur, nbs, truth, W = NP.scene(21, 200, 3, mismatch_frac=0.3)                     # (the module's record_scene fixture)
    cur["has_mp"][::7] = 1
    FE = [NP.compute_F12(cur, nb) for nb in nbs]
    T.test_create_new_map_points_store(corb, pyorc, (cur, nbs, [f for f, _ in FE], [e for _, e in FE]), 1)


def _vocs(corb, names):
    import bow_cases as G
    out = {}
    for name in names:
        f = G.vocab(name).flat()
        out[name] = corb.Vocabulary(f["k"], f["L"], f["parent"], f["is_leaf"], f["descriptor"], f["weight"])
    return out


def _voc_transform(corb, synth, pyorc):
    import test_gpu_bow_transform as T
    vocs = _vocs(corb, ("k3L6irr",))
    try:
        T.test_transform_is_the_definition_bit_for_bit(vocs, "k3L6irr")
    finally:
        vocs["k3L6irr"].close()


def _compute_bow(corb, synth, pyorc):
    import test_gpu_bow_transform as T
    vocs = _vocs(corb, ("k10L3", "k2L1"))
    try:
        T.test_compute_bow_on_records(corb, vocs)
    finally:
        for v in vocs.values():
            v.close()


def _kfdb_session(corb, synth, pyorc):
    """the keyframe database's queries take no lane (its buffers are its own); what reaches them through a lane is the BowVector corb_kf_store_compute_bow writes
    into its entries -- every other set_bow of this session"""
    import bow_cases as G
    import test_gpu_kfdb as T
    voc = _vocs(corb, (G.SESSION_VOCAB,))[G.SESSION_VOCAB]
    try:
        T.test_session_follows_the_definition(corb, voc, 2)
    finally:
        voc.close()


def _rebase_map_store(corb, synth, pyorc):
    """corb_rebase_map_store on a few records against pyorc.rebase_map, as tests/test_gpu_mapstore.py::test_configs3_server_leg_end_to_end holds it: equal bits"""
    rng = np.random.default_rng(34); K, M = 5, 70
    To2n = np.eye(4, dtype=np.float32); Q, _ = np.linalg.qr(rng.normal(size=(3, 3))); To2n[:3, :3] = Q; To2n[:3, 3] = rng.normal(0, 2, 3)
    KF = corb.KeyFrameStore(K, 4); MP = corb.MapPointStore(M, 2)
    meta = np.zeros(K, corb.KF_META_DTYPE); meta["id"] = 1 + np.arange(K); meta["nlevels"] = 8; meta["Tcw"] = rng.normal(0, 1, (K, 16)).astype(np.float32)
    KF.put_batch(0, meta, np.arange(K + 1, dtype=np.int32), np.zeros(K, corb.KP_DTYPE))
    rec = np.zeros(M, corb.MP_RECORD_DTYPE); rec["id"] = 100 + np.arange(M); rec["world_pos"] = rng.normal(0, 20, (M, 3)).astype(np.float32)
    MP.put(0, rec, np.zeros(M + 1, np.int32), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
    ks = [0, 2, 3]; ms = list(range(5, 64))
    corb.RebaseMapStore(To2n, KF, ks, MP, ms)
    P1 = np.stack([KF.get_meta(s)["Tcw"].reshape(4, 4) for s in range(K)]); X1 = MP.get(0, M)[0]["world_pos"]
    rP, rX = pyorc.rebase_map(To2n, meta["Tcw"].reshape(K, 4, 4)[ks], rec["world_pos"][ms])
    wantP = meta["Tcw"].reshape(K, 4, 4).copy(); wantP[ks] = rP; wantX = rec["world_pos"].copy(); wantX[ms] = rX
    KF.close(); MP.close()
    assert np.array_equal(P1, wantP) and np.array_equal(X1, wantX)


def _covis(corb, synth, pyorc):
    import test_gpu_covis as T
    T.test_batches_in_two_orders(corb, "k20", 2)
    T.test_erase_then_update_again(corb)
    T.test_queries(corb)
    T.test_keyframe_culling(corb, "c3")
    T.test_local_window_lists_in_the_reference_orders(corb, "k20")


def _covis_bigger(corb, synth, pyorc):
    import test_gpu_covis as T
    T.test_batches_in_two_orders(corb, "k40_wide", 17)
    T.test_keyframe_culling(corb, "c65")


def _tree_and_local_map(corb, synth, pyorc):
    import test_gpu_localmap as T
    T.test_tree_calls_follow_the_reference_literally(corb)
    T.test_update_local_map_equals_the_definition(corb, "k8", False)
    T.test_culling_reparents_the_children_and_the_local_map_follows(corb, "k8")


def _loopfix(corb, synth, pyorc):
    import loopfix_cases as C
    import test_gpu_loopfix as T
    T.test_propagate_equals_the_definition_bit_for_bit(corb, "unmarked_origin")
    T.run_correct_loop(corb, C.LOOP_SEEDS[0], C.LOOP_CURS[0], 1.0, 1.2)


def _by_n(cases, key="n"):
    return sorted(cases, key=lambda c: (c[key], c["i"]))


TRACK_POSE_CASE = next(c for c in RC.TRACK_POSE_CASES if c["edges"] >= 10)          # ten edges: all four rounds, and the host-pointer batch call beside the record call
SIM3_SINGLE = next(c for c in RL.SIM3_CASES if c["n"] == 63)
GRAPH_CASE = next(c for c in RL.GRAPH_CASES if c["nP"] == 9 and c["iters"] == 20)

ENTRIES = [
    # ---- lane 0: the per-frame calls ----
    Entry("spd_solve_97", 0, "corb_spd_solve", _spd_97),
    Entry("descriptor_distance", 0, "corb_descriptor_distance", _module_test("test_gpu_match", "test_descriptor_distance", order="cp")),
    Entry("search_by_bow", 0, "corb_search_by_bow", _case(RM.test_search_by_bow_random_case, RM.BOW_CASES[0]), bigger=_case(RM.test_search_by_bow_random_case, RM.BOW_CASES[2])),
    Entry("search_for_triangulation", 0, "corb_search_for_triangulation", _module_test("test_gpu_match", "test_search_for_triangulation", 4)),
    Entry("distinctive_descriptors", 0, "corb_distinctive_descriptors", lambda corb, synth, pyorc: RC.test_distinctive_descriptors_with_median_ties(corb, pyorc)),
    Entry("rebase_map", 0, "corb_rebase_map", _module_test("test_gpu_map", "test_rebase_map", order="cp")),
    Entry("projection_map", 0, "corb_search_by_projection_map", _case(RM.test_search_by_projection_map_random_case, _by_n(RM.MAP_CASES)[0]),
          bigger=_case(RM.test_search_by_projection_map_random_case, _by_n(RM.MAP_CASES)[-1])),
    Entry("projection_frame", 0, "corb_search_by_projection_frame", _case(RM.test_search_by_projection_frame_random_case, _by_n(RM.FRAME_CASES)[0]),
          bigger=_case(RM.test_search_by_projection_frame_random_case, _by_n(RM.FRAME_CASES)[-1])),
    Entry("search_for_initialization", 0, "corb_search_for_initialization", _case(RM.test_search_for_initialization_random_case, _by_n(RM.INIT_CASES)[0]),
          bigger=_case(RM.test_search_for_initialization_random_case, _by_n(RM.INIT_CASES)[-1])),
    Entry("projection_reloc", 0, "corb_search_by_projection_reloc", _kfproj("test_reloc_projection", 5112, 500, 1.0, with_matcher=False)),
    Entry("projection_scw", 0, "corb_search_by_projection_scw", _case(RM.test_search_by_projection_scw_random_case, _by_n(RM.SCW_CASES)[0]),
          bigger=_case(RM.test_search_by_projection_scw_random_case, _by_n(RM.SCW_CASES)[-1])),
    Entry("fuse_both_overloads", 0, "corb_fuse", _kfproj("test_fuse_both_overloads", 5102, 700, 1.0)),
    Entry("search_by_sim3", 0, "corb_search_by_sim3", _kfproj("test_search_by_sim3", 5121, 1200)),
    Entry("track_search_last_frame", 0, "corb_track_search_last_frame corb_kf_store_put_host", _case(RC.test_track_search_last_frame_random_case, RC.TRACK_LAST_CASES[0]),
          bigger=_case(RC.test_track_search_last_frame_random_case, RC.TRACK_LAST_CASES[6])),
    Entry("track_pose_optimization", 0, "corb_track_pose_optimization corb_pose_optimization_batch", _case(RC.test_track_pose_optimization_random_case, TRACK_POSE_CASE),
          bigger=_case(RC.test_track_pose_optimization_random_case, RC.TRACK_POSE_CASES[13])),
    Entry("track_search_local_points", 0, "corb_track_search_local_points", _case(RC.test_track_search_local_points_random_case, RC.TRACK_LOCAL_CASES[0]),
          bigger=_case(RC.test_track_search_local_points_random_case, RC.TRACK_LOCAL_CASES[6])),
    Entry("track_search_reloc", 0, "corb_track_search_reloc", _case(RC.test_reloc_on_records_random_case, RC.REC_RELOC_CASES[0]),
          bigger=_case(RC.test_reloc_on_records_random_case, RC.REC_RELOC_CASES[3])),
    Entry("projection_scw_store", 0, "corb_search_by_projection_scw_store", _case(RC.test_scw_on_records_random_case, RC.REC_SCW_CASES[0]),
          bigger=_case(RC.test_scw_on_records_random_case, RC.REC_SCW_CASES[4])),
    Entry("search_by_sim3_store", 0, "corb_search_by_sim3_store", _case(RC.test_sim3_on_records_random_case, RC.REC_SIM3_CASES[0]),
          bigger=_case(RC.test_sim3_on_records_random_case, RC.REC_SIM3_CASES[4])),
    Entry("fuse_store", 0, "corb_fuse_store", _case(RC.test_fuse_on_records_random_case, RC.REC_FUSE_CASES[0]), bigger=_case(RC.test_fuse_on_records_random_case, RC.REC_FUSE_CASES[4])),
    Entry("fuse_sim3_store", 0, "corb_fuse_sim3_store", _module_test("test_gpu_fuse_sim3_store", "test_fuse_with_scw_on_records")),
    Entry("mp_store_replace", 0, "corb_mp_store_replace corb_kf_store_put_host", _case_np(RC.test_replace_long_lists_random_case, RC.REPLACE_CASES[3]),
          bigger=_case_np(RC.test_replace_long_lists_random_case, RC.REPLACE_CASES[5])),
    Entry("matchers_on_slots", 0, "corb_search_by_bow_slots corb_search_for_triangulation_slots", _module_test("test_gpu_store", "test_matchers_on_slots_equal_the_host_pointer_calls")),
    Entry("rebase_map_store", 0, "corb_rebase_map_store", _rebase_map_store),
    Entry("triangulate_pairs", 0, "corb_triangulate_pairs", _triangulate_pairs(65), bigger=_triangulate_pairs(257)),
    Entry("create_new_map_points_store", 0, "corb_create_new_map_points_store corb_kf_store_put_frame", _create_new_map_points),
    Entry("sim3_ransac", 0, "corb_sim3_ransac", _module_test("test_gpu_sim3_ransac", "test_sim3_ransac_host_arrays", "one_special", order="c"),
          bigger=_module_test("test_gpu_sim3_ransac", "test_sim3_ransac_host_arrays", "three", order="c")),
    Entry("sim3_ransac_store", 0, "corb_sim3_ransac_store", _module_test("test_gpu_sim3_ransac", "test_sim3_ransac_on_records", 1, order="c")),
    Entry("pnp_ransac", 0, "corb_pnp_ransac", _module_test("test_gpu_pnp_ransac", "test_pnp_ransac_host_arrays", "refine_sets", order="c"),
          bigger=_module_test("test_gpu_pnp_ransac", "test_pnp_ransac_host_arrays", "epsilon_02", order="c")),
    Entry("pnp_ransac_store", 0, "corb_pnp_ransac_store", _module_test("test_gpu_pnp_ransac", "test_pnp_ransac_on_records", 1, order="c")),
    Entry("mono_initialize", 0, "corb_mono_initialize", _module_test("test_gpu_initializer", "test_initialize_is_the_definition_bit_for_bit", "general65", order="c"),
          bigger=_module_test("test_gpu_initializer", "test_initialize_is_the_definition_bit_for_bit", "general200", order="c")),
    # (corb_ba_solve_staged with one free pose and the automatic solver: the fused single-pose kernel, which runs in the pose batch of lane 0)
    Entry("pose_optimization_fused", 0, "corb_ba_solve_staged", _case(RB.test_pose_optimization_random_case, _smallest(RB.POSE_CASES, lambda c: c["n"], solver=0)),
          bigger=_case(RB.test_pose_optimization_random_case, RB.POSE_CASES[10])),
    Entry("optimize_sim3", 0, "corb_optimize_sim3", _case_np(RL.test_sim3_random_case_single, SIM3_SINGLE), bigger=_case_np(RL.test_sim3_random_batch, RL.SIM3_BATCHES[3])),
    Entry("voc_transform", 0, "corb_voc_transform", _voc_transform),
    Entry("kf_store_compute_bow", 0, "corb_kf_store_compute_bow", _compute_bow),
    Entry("kfdb_session", 0, "corb_kf_store_compute_bow", _kfdb_session),
    Entry("covisibility", 0, "corb_covis_update corb_covis_erase corb_covis_query corb_covis_weight corb_covis_keyframe_culling corb_covis_local_window", _covis, bigger=_covis_bigger),
    Entry("tree_and_local_map", 0, "corb_covis_set_tree corb_covis_get_tree corb_covis_add_child corb_covis_erase_child corb_covis_change_parent corb_covis_reparent_children "
          "corb_track_update_local_map corb_covis_update corb_covis_erase", _tree_and_local_map),
    Entry("loop_correction", 0, "corb_gba_propagate_store corb_loop_correct_store corb_covis_set_tree", _loopfix),
    # ---- lane 1: every bundle-adjustment route and the essential graph ----
] + [Entry("global_ba_%s" % r.replace("-", "_"), 1, "corb_ba_solve_ex", _case(RB.test_global_ba_random_case, c)) for r, c in BA_ROUTE_CASES.items()] + [
    Entry("global_ba_devflat", 1, "corb_ba_solve_devflat", _case(RB.test_global_ba_random_case, BA_DEVFLAT_CASE)),
    Entry("global_ba_plain_call", 1, "corb_ba_solve", _ba_solve_plain),
    Entry("staged_window_host", 1, "corb_ba_solve_staged", _case(RB.test_local_window_random_case, WINDOW_HOST_CASE)),
    Entry("staged_window_device", 1, "corb_ba_solve_staged", _case(RB.test_local_window_random_case, WINDOW_DEVICE_CASE), bigger=_case(RB.test_local_window_random_case, RB.WINDOW_CASES[4])),
    Entry("pose_optimization_general_path", 1, "corb_ba_solve_staged", _case(RB.test_pose_optimization_random_case, _smallest(RB.POSE_CASES, lambda c: c["n"], solver=1))),
    Entry("essential_graph", 1, "corb_optimize_essential_graph", _case(RL.test_graph_random_case, GRAPH_CASE)),
    Entry("global_ba_store", 1, "corb_ba_solve_store", _ba_store),
    Entry("local_ba_store_host", 1, "corb_local_ba_store", _local_ba_store(2100, 25)),
    Entry("local_ba_store_device", 1, "corb_local_ba_store", _local_ba_store(2103, 140)),
]
assert len({e.name for e in ENTRIES}) == len(ENTRIES)
