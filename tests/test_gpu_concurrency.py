"""Thread safety of the host-pointer entry points: the reference calls its matchers and optimisers from several threads
(Tracking, LocalMapping, LoopClosing).  A long global BA (workspace lane 1) and per-frame matcher / pose calls (lane 0) run
concurrently from two threads and must return exactly what they return serially."""
import threading
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_ba_and_tracking_calls_from_two_threads(corb, synth):
    prob = synth.ba_problem(n_clients=8, kf_per_client=60, pts_per_kf=40, seed=1007)
    a = (prob["poses"], prob["pose_fixed"], prob["points"], prob["point_fixed"], prob["edges"], prob["fx"], prob["fy"], prob["cx"], prob["cy"], prob["bf"])
    sc = synth.tracking_scene(4000)
    q = synth.pose_opt_problem(seed=3000, n=300)
    mt = corb.ORBmatcher(0.6, True)
    def track():
        m = mt.SearchByProjection_Frame(sc["cur"], sc["Tcw"], sc["Tlw"], sc["fx"], sc["fy"], sc["cx"], sc["cy"], sc["bf"], sc["mb"], sc["last"], sc["last_desc"], 7.0, False)
        p = corb.Optimizer.PoseOptimization(q["Tcw0"], q["points"], q["obs"], q["inv_sigma2"], q["fx"], q["fy"], q["cx"], q["cy"], q["bf"])
        return m, p
    ref_ba = corb.Optimizer.GlobalBundleAdjustemnt(*a, nIterations=5, solver=1)          # dense solver: run-to-run reproducible
    ref_m, ref_p = track()
    out = {}
    def ba_thread():
        out["ba"] = [corb.Optimizer.GlobalBundleAdjustemnt(*a, nIterations=5, solver=1) for _ in range(12)]      # (round 6: each of these deviated with ~1 % probability while
    def track_thread():                                                                                             #  dense_chol.hip's panel kernel raced on its diagonal block)
        out["tr"] = [track() for _ in range(240)]
    t1 = threading.Thread(target=ba_thread); t2 = threading.Thread(target=track_thread)
    t1.start(); t2.start(); t1.join(); t2.join()
    for r in out["ba"]:
        assert np.allclose(r["chi2"], ref_ba["chi2"], rtol=1e-9) and np.abs(r["poses"] - ref_ba["poses"]).max() < 1e-6
    for m, p in out["tr"]:
        assert np.array_equal(m[0], ref_m[0]) and m[1] == ref_m[1]
        assert np.array_equal(p[1], ref_p[1]) and p[2] == ref_p[2] and np.abs(p[0] - ref_p[0]).max() < 1e-6


def _packed(synth, ids, w=640, h=240):
    fr = [synth.stereo_pair(i, w=w, h=h) for i in ids]
    return np.ascontiguousarray(np.stack([np.stack([l, r]) for l, r in fr]))


def test_part_batches_join_lazily_but_correctly(corb, synth):
    """A run of many frames is issued as part-batches on two streams that are joined only when a later call needs it (corb_orb.cpp: corb_run_parts /
    corb_join).  Back-to-back runs with new uploads in between, and fetches right after a run without a sync, must return exactly what a run of
    the same frames returns when it is issued alone, in one piece, on one stream (profile mode 2)."""
    W, H, N = 1241, 376, 48                                   # 96 KITTI-size images: the second part-batch ends ~0.2 ms after the handle's own stream
    A = _packed(synth, range(100, 100 + N), W, H); B = _packed(synth, range(300, 300 + N), W, H)
    def alone(P):
        sf = corb.StereoFrontend(nfeatures=2000, width=W, height=H, max_frames=N)
        sf.orb.profile(2)                                     # no part-batches
        sf.upload_batch(0, P); sf.run(N); sf.sync()
        out = sf.fetch_batch(0, N); sf.orb.profile(False); sf.close()
        return out
    ref_a, ref_b = alone(A), alone(B)
    sf = corb.StereoFrontend(nfeatures=2000, width=W, height=H, max_frames=N)
    def same(x, y):                                         # entries past an image's count are stale device memory: compare the valid parts
        if not (np.array_equal(x["counts"], y["counts"]) and np.array_equal(x["n_matched"], y["n_matched"])):
            return False
        for i, c in enumerate(x["counts"]):
            if x["kp"][i, :c].tobytes() != y["kp"][i, :c].tobytes() or not np.array_equal(x["desc"][i, :c], y["desc"][i, :c]):
                return False
        for f in range(N):
            c = x["counts"][2 * f]
            if x["u_right"][f, :c].tobytes() != y["u_right"][f, :c].tobytes() or x["depth"][f, :c].tobytes() != y["depth"][f, :c].tobytes():
                return False
        return True
    def last_frame_same(got, ref):                          # the LAST frame belongs to the second part-batch, which finishes after the handle's own stream
        f = N - 1
        cl, cr = ref["counts"][2 * f], ref["counts"][2 * f + 1]
        return (len(got["kl"]) == cl and len(got["kr"]) == cr and got["kl"].tobytes() == ref["kp"][2 * f, :cl].tobytes()
                and np.array_equal(got["dl"], ref["desc"][2 * f, :cl]) and np.array_equal(got["dr"], ref["desc"][2 * f + 1, :cr])
                and got["u_right"].tobytes() == ref["u_right"][f, :cl].tobytes() and got["n_matched"] == ref["n_matched"][f])
    for rep in range(3):
        sf.upload_batch(0, A); sf.run(N)                      # no sync: the next upload overwrites inputs the side stream may still be reading
        assert last_frame_same(sf.fetch(N - 1), ref_a), "last frame of run A, repetition %d (stale = the previous run's B)" % rep
        got_a = sf.fetch_batch(0, N)                          # fetch right after the run: must wait for BOTH parts
        assert same(got_a, ref_a), "run A, repetition %d" % rep
        sf.upload_batch(0, B); sf.run(N); sf.run(N)           # the same inputs twice, back to back
        sf.upload_batch(0, A)                                 # rewrites inputs while both parts of the second run may be in flight ...
        sf.upload_batch(0, B)                                 # ... and puts B back before anything is read
        sf.run(N)
        assert last_frame_same(sf.fetch(N - 1), ref_b), "last frame of run B, repetition %d" % rep
        got_b = sf.fetch_batch(0, N)
        assert same(got_b, ref_b), "run B, repetition %d" % rep
    sf.close()


def test_large_odd_run_as_two_parts_equals_unsplit(corb, synth):
    """corb_run_parts cuts every split run into TWO part-batches (round 4; parts of ~128 images, up to four, before): a run of 225 frames -- odd, so the parts are
    113 and 112 frames, and large enough for the old rule's four -- returns what the same run returns in one piece on one stream (profile mode 2)."""
    W, H, N = 640, 240, 225
    base = _packed(synth, range(700, 716), W, H)
    P = np.ascontiguousarray(base[np.arange(N) % 16])
    outs = []
    for serial in (True, False):
        sf = corb.StereoFrontend(nfeatures=1000, width=W, height=H, max_frames=N)
        if serial:
            sf.orb.profile(2)
        sf.upload_batch(0, P); sf.run(N); sf.sync()
        outs.append(sf.fetch_batch(0, N)); sf.orb.profile(False); sf.close()
    a, b = outs
    assert np.array_equal(a["counts"], b["counts"]) and np.array_equal(a["n_matched"], b["n_matched"]) and int(a["counts"].min()) > 100
    for i, c in enumerate(a["counts"]):
        assert a["kp"][i, :c].tobytes() == b["kp"][i, :c].tobytes() and np.array_equal(a["desc"][i, :c], b["desc"][i, :c]), "image %d" % i
    for f in range(N):
        c = a["counts"][2 * f]
        assert a["u_right"][f, :c].tobytes() == b["u_right"][f, :c].tobytes() and a["depth"][f, :c].tobytes() == b["depth"][f, :c].tobytes(), "frame %d" % f
    # frames 16 apart are the same images: the two halves of the run agree with each other too
    assert a["kp"][0, :a["counts"][0]].tobytes() == b["kp"][2 * 224, :b["counts"][2 * 224]].tobytes()


def test_release_scratch_beside_a_running_optimisation(corb, synth):
    """corb_release_scratch from a second thread while a global BA holds the long-optimisation lane: the lane in use is skipped (no wait, no crash), the BA returns what it
    returns alone, and a release after it frees that lane's arena"""
    prob = synth.ba_problem_fast(n_clients=4, kf_per_client=300, pts_per_kf=60, seed=1099, obs_range=(3, 6), window=5)
    a = (prob["poses"], prob["pose_fixed"], prob["points"], prob["point_fixed"], prob["edges"], prob["fx"], prob["fy"], prob["cx"], prob["cy"], prob["bf"])
    ref = corb.Optimizer.GlobalBundleAdjustemnt(*a, nIterations=8, bRobust=False, intr=prob["intr"])
    out = {}
    def ba(): out["ba"] = [corb.Optimizer.GlobalBundleAdjustemnt(*a, nIterations=8, bRobust=False, intr=prob["intr"]) for _ in range(3)]
    def rel(): out["freed"] = [corb.release_scratch(0) for _ in range(40)]
    t1 = threading.Thread(target=ba); t2 = threading.Thread(target=rel)
    t1.start(); t2.start(); t1.join(); t2.join()
    for r in out["ba"]:
        assert np.array_equal(r["chi2"], ref["chi2"]) and r["poses"].tobytes() == ref["poses"].tobytes()
    assert all(f >= 0 for f in out["freed"])
    assert corb.release_scratch(0) >= 0 and corb.release_scratch(0) == 0


def test_local_windows_and_essential_graph_beside_a_busy_second_thread(corb, synth):
    """LocalBundleAdjustment (one-workgroup, chained and dense-solver routes), OptimizeEssentialGraph (dense Cholesky) and a dense-path global BA while another thread keeps
    the GPU busy with front-end runs and tracking calls: every call returns its serial bits (tools/conc_probe4.py is the long form; round 6 found the dense Cholesky's
    panel kernel racing on its diagonal block this way)"""
    def args(p): return (p["poses"], p["pose_fixed"], p["points"], p["point_fixed"], p["edges"], p["fx"], p["fy"], p["cx"], p["cy"], p["bf"])
    jobs = []
    for kw in (dict(seed=2001), dict(seed=2002, n_local=24, n_fixed=8, pts_per_kf=40)):
        p = synth.local_ba_problem(**kw); jobs.append((lambda p=p: corb.Optimizer.LocalBundleAdjustment(*args(p)), ("poses", "points", "outlier")))
    g = synth.essential_graph(seed=7001, K=80)
    jobs.append((lambda: corb.Optimizer.OptimizeEssentialGraph(g, iterations=12), ("S", "chi2", "points")))
    pm = synth.ba_problem(n_clients=3, kf_per_client=30, pts_per_kf=30, seed=1013)
    jobs.append((lambda: corb.Optimizer.GlobalBundleAdjustemnt(*args(pm), nIterations=6, bRobust=True, solver=1), ("chi2", "poses", "points")))
    sc = synth.tracking_scene(4000); q = synth.pose_opt_problem(seed=3000, n=900); mt = corb.ORBmatcher(0.6, True)
    P = _packed(synth, range(70, 74), 1241, 376)
    sf = corb.StereoFrontend(nfeatures=2000, width=1241, height=376, max_frames=4)
    def other():
        sf.upload_batch(0, P); sf.run(4); sf.sync()
        mt.SearchByProjection_Frame(sc["cur"], sc["Tcw"], sc["Tlw"], sc["fx"], sc["fy"], sc["cx"], sc["cy"], sc["bf"], sc["mb"], sc["last"], sc["last_desc"], 7.0, False)
        corb.Optimizer.PoseOptimization(q["Tcw0"], q["points"], q["obs"], q["inv_sigma2"], q["fx"], q["fy"], q["cx"], q["cy"], q["bf"])
    refs = [f() for f, _ in jobs]
    stop = [False]
    def bg():
        while not stop[0]: other()
    t = threading.Thread(target=bg); t.start()
    try:
        for _ in range(20):
            for (f, keys), ref in zip(jobs, refs):
                r = f()
                assert all(np.asarray(r[k]).tobytes() == np.asarray(ref[k]).tobytes() for k in keys)
    finally:
        stop[0] = True; t.join(); sf.close()


def test_matchers_on_slots_from_threads_that_name_the_stores_in_opposite_order(corb, synth):
    """corb_search_by_bow_slots / corb_search_for_triangulation_slots hold both stores' locks (lower address first, one lock when the stores are one) until their last
    read of the host mirror.  Two threads name A and B in opposite argument order while a third rewrites slot (A, 0): no deadlock, and every output equals the serial
    one.  The third thread rewrites the slot's FeatureVector and flags (set_bow, set_flags: the node ids the matchers read on the host, and identical bytes on the
    device); a put of the features themselves would clear the FeatureVector until the next set_bow, and the outputs would then depend on the interleaving."""
    import time
    from test_oracle_match import _make
    rng = np.random.default_rng(2024)
    A = corb.KeyFrameStore(2, 64); B = corb.KeyFrameStore(2, 64)
    for (sa, sb), (n1, n2) in (((0, 1), (51, 49)), ((1, 0), (47, 53))):          # (A, sa) and (B, sb) see the same scene
        d1, a1, v1, fv1, d2, a2, v2, fv2 = _make(rng, synth, n1, n2, 6)
        for st, slot, n, d, a, v, fv in ((A, sa, n1, d1, a1, v1, fv1), (B, sb, n2, d2, a2, v2, fv2)):
            kp = np.zeros(n, corb.KP_DTYPE); kp["angle"] = a; kp["x"], kp["y"] = rng.uniform(0, 1241, n), rng.uniform(0, 376, n); kp["octave"] = rng.integers(0, 8, n)
            ur = np.where(rng.random(n) < 0.6, kp["x"] - 5, -1).astype(np.float32)
            st.put(slot, kp, d, ur, None, keyframe_id=10 * slot + (st is B)); st.set_bow(slot, fv); st.set_flags(slot, v)
            if st is A and slot == 0: fv_a0, flags_a0 = fv, v
    F12 = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32) + rng.normal(0, 1e-4, (3, 3)).astype(np.float32)
    scale = (np.float32(1.2) ** np.arange(8)).astype(np.float32); sigma2 = scale * scale
    calls = [lambda: A.SearchByBoW(0, B, 1, 0.9, True, 0), lambda: B.SearchByBoW(1, A, 0, 0.9, True, 0),
             lambda: A.SearchForTriangulation(0, B, 1, F12, 600.0, 180.0, scale, sigma2, False), lambda: B.SearchForTriangulation(1, A, 0, F12, 600.0, 180.0, scale, sigma2, False),
             lambda: A.SearchByBoW(0, A, 1, 0.9, True, 1)]                        # (A == B: one lock)
    t0 = time.perf_counter()
    ref = [c() for c in calls]
    serial = time.perf_counter() - t0
    assert sum(n for _, n in ref) > 0                                            # (the comparison below is not one of empty outputs)
    out = {0: [], 1: []}
    def search(t):
        order = (0, 1, 2, 3, 4) if t == 0 else (1, 0, 3, 2, 4)
        for _ in range(20):
            out[t].append([(k, calls[k]()) for k in order])
    def reput():
        for _ in range(20):
            A.set_bow(0, fv_a0); A.set_flags(0, flags_a0)
    threads = [threading.Thread(target=search, args=(0,), daemon=True), threading.Thread(target=search, args=(1,), daemon=True), threading.Thread(target=reput, daemon=True)]
    deadline = time.perf_counter() + max(10.0, 50 * serial)
    for t in threads: t.start()
    for t in threads: t.join(max(0.0, deadline - time.perf_counter()))
    assert not any(t.is_alive() for t in threads), "the calls did not finish: the stores' locks were taken in two orders"
    for t in (0, 1):
        assert len(out[t]) == 20
        for rnd in out[t]:
            for k, (m, n) in rnd:
                assert n == ref[k][1] and m.tobytes() == ref[k][0].tobytes(), (t, k)
    A.close(); B.close()
