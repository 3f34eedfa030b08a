#!/usr/bin/env python3
"""bench.py -- stereo frames/s of the ORB extract + stereo-match hot path on MI355X.

A "step" is one pass of the hot path over one batch of B synthetic KITTI-shaped stereo frames
(BASELINE.json configs[1]: 1241x376, 2000 features/frame, 8 levels, 1.2, FAST 20/7): for every frame
2 x ORBextractor::operator() + Frame::ComputeStereoMatches, all through the C-ABI of libcorb_accel.so.
Inputs are resident in HBM before the timed region.  N>1: one process per GPU (one client per GPU,
independent streams, no data-path collective => weak scaling); launched by torch.distributed.run.

Prints ONE JSON line (rank 0).  A plain run sets up, warms up, times the K steps and prints the headline
(`value`, `ms_per_step`); everything else is measured with --full only: `roofline` (the kernel with the
largest share of device time, HIP events on the library's own stream), `cpu_baseline` (the CPU oracle, a
port of the reference algorithm, 2 threads like the reference's left/right extraction threads, on a
bounded sample), the repeats, host-buffer, map-push, BA, 1080p, latency and client-loop legs.
--dump-outputs DIR writes what the last timed step computed (a fixed sample of its frames) as .npy files.
"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

NPARTS = int(os.environ["CORB_PARTS"]) if os.environ.get("CORB_PARTS") else 2        # part-batches of a run (corb_orb.cpp: corb_run_parts)
KITTI = dict(width=1241, height=376, nfeatures=2000, fx=718.856, bf=386.1448)
HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: 8.0 TB/s spec


def algorithmic_bytes(geom, counts):
    """Minimum HBM bytes per IMAGE of each kernel (DESIGN.md 'kernels and rooflines').
    geom: list of (w,h) per level; counts: dict(cand=mean candidates/image, kp=mean keypoints/image)."""
    px = [w * h for (w, h) in geom]
    allpx = sum(px)
    return {
        "orb_resize_kernel": sum(px[:-1]) + sum(px[1:]),           # read level l-1, write level l (7 launches)
        "orb_pyramid_kernel": sum(px[:-1]) + sum(px[1:]),          # the same bytes in one launch (strip-fused)
        "orb_fast_kernel": allpx + 4 * counts["cand"],             # read every level once, write packed candidates
        "orb_blur_kernel": 2 * allpx,                              # read + write every level once
        "orb_octree_kernel": 4 * counts["cand"] + 4 * counts["kp"],     # read candidates, write selected keypoints
        "orb_describe_kernel": counts["kp"] * (709 + 512 + 28 + 32),    # IC patch + 512 BRIEF samples + outputs
        "stereo_match_kernel": counts["kp"] * (28 + 32 + 40 * (4 + 28 + 32) + 0.3 * 12 * 121),   # per frame: ~40 row candidates per left kp + SAD patches
        "stereo_filter_kernel": counts["kp"] * 6,
        "stereo_rows_kernel": counts["kp"] * (28 + 4 * 9),                # right keypoints read, ~9 row entries each written
    }


def cpu_client(n_frames, synth, seed0, start_at=None):
    """one reference-style client on the CPU oracle: left/right extraction in 2 threads (Frame.cc:78-81), matcher single-threaded"""
    from oracle import pyorc
    el, er = pyorc.Extractor(native=True), pyorc.Extractor(native=True)
    tb = el.tables()
    frames = [synth.stereo_pair(seed0 + i) for i in range(min(n_frames, 8))]
    if start_at is not None:
        time.sleep(max(0.0, start_at - time.time()))          # all clients of the throughput sample start together
    t0 = time.perf_counter()
    for i in range(n_frames):
        l, r = frames[i % len(frames)]
        res = {}
        tl = threading.Thread(target=lambda: res.__setitem__("l", el.extract(l)))
        tr = threading.Thread(target=lambda: res.__setitem__("r", er.extract(r)))
        tl.start(); tr.start(); tl.join(); tr.join()
        kl, dl = res["l"]; kr, dr = res["r"]
        pyorc.stereo_match(el, er, kl, dl, kr, dr, KITTI["bf"], KITTI["fx"], tb["scale"], tb["inv_scale"])
    return time.perf_counter() - t0


def cpu_baseline(n_frames, synth, seed0):
    """The CPU oracle as the reported CPU baseline (kind 'port'), -O3 -march=native like the reference's flags: one client (2 threads) as
    `value`, and a bounded throughput sample with several independent client processes (the reference runs one process per client)."""
    import subprocess
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s", "-B", "liborc_native.so"])
    dt = cpu_client(n_frames, synth, seed0)
    out = dict(value=n_frames / dt, unit="stereo frames/s", cores=2, kind="port",
               sample="%d stereo frames of the same synthetic 1241x376 stream, oracle -O3 -march=native, host has %d cores"
                      % (n_frames, os.cpu_count() or 0))
    try:
        # independent clients (2 threads each), the reference's one-process-per-client deployment.  The sample is CAPPED at 32 clients (64 threads):
        # filling a 256-core box took 128 Python processes and most of the bench's wall time; the figure for the whole box is the
        # sample's per-client rate x floor(nproc / 2) clients -- an extrapolation that assumes the clients scale like the 32 did, stated as such
        full = max(1, (os.cpu_count() or 2) // 2); ncl = min(full, 32); per = max(8, n_frames // 4)
        start_at = time.time() + (8.0 if ncl <= 16 else 15.0)         # (the Python processes need a while to import and build their frames)
        procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--cpu-worker", str(seed0 + 64 * c), str(per), repr(start_at)],
                                  stdout=subprocess.PIPE, stderr=subprocess.DEVNULL) for c in range(ncl)]
        el = [float(p_.communicate(timeout=300)[0].decode().strip().split()[-1]) for p_ in procs]
        rate = ncl * per / max(el)
        out["throughput_mode"] = dict(value=round(rate, 2), unit="stereo frames/s", clients=ncl, cores=2 * ncl,
                                      sample="%d client processes x %d frames started together (2 threads each)" % (ncl, per),
                                      whole_box_extrapolated=dict(value=round(rate * full / ncl, 2), clients=full, cores=2 * full,
                                                                  note="measured rate x %d / %d clients: linear in the client count, an upper bound where memory bandwidth or clocks give way" % (full, ncl)))
    except Exception as e:
        out["throughput_mode"] = dict(error=str(e)[:200])
    return out


def bench_1080p(corb, synth, device, B=128, steps=12):
    """BASELINE configs[4]'s extraction half on one GPU: 1920x1080 stereo frames, 4000 features (8 levels x 1.2, FAST 20/7; fx = 1000, bf = 500 chosen here),
    inputs resident in HBM, the same calls as the headline leg (frames per step 32 / 64 / 128: 18.9 k / 23.4 k / 23.8 k stereo fps, tools/bench_1080p_sweep.py).  Parity at this size: tests/test_gpu_orb.py::test_stereo_1080p_golden."""
    W, H, NF = 1920, 1080, 4000
    sf = corb.StereoFrontend(nfeatures=NF, width=W, height=H, max_frames=B, fx=1000.0, bf=500.0, device=device)
    try:
        frames = [synth.stereo_pair(i, W, H) for i in range(8)]
        for s_ in range(B):
            l, r = frames[s_ % 8]; sf.upload(s_, l, r)
        sf.sync()
        sf.orb.profile(True); sf.orb.profile(False)
        for _ in range(3):
            sf.run(B)
        sf.sync()
        t0 = time.perf_counter()
        for i in range(steps):
            sf.orb.profile(i % 4 == 2)                 # (not step 0: it meets an empty GPU)
            sf.run(B)
        sf.sync()
        dt = (time.perf_counter() - t0) / steps
        prof = dict((k, v) for k, v in sf.orb.profile_read().items() if v[1]); sf.orb.profile(False)
        outs = [sf.fetch(s_) for s_ in range(min(B, 4))]
        kp_mean = sum(len(o["kl"]) + len(o["kr"]) for o in outs) / (2.0 * len(outs))
        cand_mean = sum(len(sf.orb.candidates(s_, l)) for s_ in range(4) for l in range(8)) / 4.0
        geom = [sf.orb.pyramid_level(0, l).shape[::-1] for l in range(8)]
        ab = algorithmic_bytes(geom, dict(cand=cand_mean, kp=kp_mean))
        parts = 2 if 2 * B >= 32 else 1
        rec = dict(value=round(B / dt, 1), unit="stereo frames/s", frames_per_step=B, ms_per_step=round(dt * 1e3, 3), steps=steps,
                   config=dict(workload="configs[4] extraction half: 1920x1080 stereo, 4000 feat/frame, 8 levels x1.2, FAST 20/7, fx 1000, bf 500", inputs="resident in HBM",
                               mean_keypoints_per_image=round(kp_mean, 1), mean_candidates_per_image=round(cand_mean, 1),
                               mean_stereo_matches_per_frame=round(sum(o["n_matched"] for o in outs) / float(len(outs)), 1)))
        # every kernel alone on the GPU (unsplit, one stream): what the pipeline's overlap stretches each launch from
        sf.orb.profile(2)
        for _ in range(2):
            sf.run(B)
        sf.sync()
        alone = dict((k, round(v[0] / v[1] * 1e3, 2)) for k, v in sf.orb.profile_read().items() if v[1]); sf.orb.profile(False)
        if prof:
            # the dominant kernel BY MEASURED TIME inside the pipeline (at this size the quadtree kernel can pass FAST: VERDICT r4 weak 8), with its own algorithmic bytes
            dom = max((k for k in prof if k in ab), key=lambda k: prof[k][0])
            ms, launches = prof[dom]
            by = ab[dom] * (2 * B) / parts
            ach = by / (ms / launches * 1e-3) / 1e9
            path = sum(geom[l][0] * geom[l][1] for l in range(8))
            per_frame = 2 * (W * H + (path - W * H) + 3 * path + kp_mean * 60)      # input + levels 1-7 written + FAST / blur reads + blurred planes + outputs, per image x 2
            traffic = None                       # counter run at THIS size: tools/gpu_pmc_1080p.sh (128 frames per step = 128 images per part-batch launch)
            try:
                pm = json.load(open(os.path.join(ROOT, "profiles", "pmc_1080p.json")))
                if int(2 * B / parts) == 128: traffic = pm.get(dom, {}).get("hbm_bytes_per_launch")
            except Exception:
                traffic = None
            rec["roofline"] = dict(bound="hbm", kernel=dom, dominant_by="summed time inside the pipeline", achieved=round(ach, 1), peak=HBM_PEAK_GBS, unit="GB/s", frac=round(ach / HBM_PEAK_GBS, 4), traffic=traffic,
                                   avg_us=round(ms / launches * 1e3, 2), algorithmic_bytes=int(by), images_per_launch=int(2 * B / parts),
                                   kernels=dict((k, dict(avg_us=round(v[0] / v[1] * 1e3, 2), launches=int(v[1]), alone_unsplit_us=alone.get(k),
                                                         GBps=round(ab[k] * (2 * B) / parts / (v[0] / v[1] * 1e-3) / 1e9, 1) if k in ab else None)) for k, v in sorted(prof.items())),
                                   whole_path=dict(algorithmic_bytes_per_frame=int(per_frame), achieved_GBps=round(per_frame * B / dt / 1e9, 1), frac=round(per_frame * B / dt / 1e9 / HBM_PEAK_GBS, 4)),
                                   note="event pairs of every 4th step on the kernels' own streams (like the headline leg); alone_unsplit_us: the same %d images in ONE launch per kernel on one stream (twice the images of a part-batch launch); traffic: profiles/pmc_1080p.json; no counter run at this size: traffic null" % (2 * B))
        return rec
    finally:
        sf.close()


def latency_bench(corb, synth, device, calls=240):
    """The reference's own operating point: a corbslam_client hands over ONE stereo frame at a time (Frame::Frame(stereo),
    corbslam_client/src/Frame.cc:61-117, per frame from Tracking::GrabImageStereo, Tracking.cc:166-203).  corb_stereo_frames: B frames per call, host
    buffers in and out (page-locked), one transfer each way around the captured kernel chain, one synchronisation.  Per B = 1, 2, 8:
      host_to_host_ms : median / p90 wall time of a call over `calls` calls, timed one by one
      stages_ms       : medians of the call's three stage times by HIP events (separate calls: the four event records cost a few us); residual = host_to_host_ms minus
                        their sum (stages and calls are timed in separate runs, so it can be a few us negative)
      resident_ms     : the kernel chain alone, inputs already in HBM and results left there (corb_stereo_run + corb_stereo_sync: direct launches)
      kernels_alone_us: every kernel of the B = 1 chain timed alone (event pairs of the handle's profiler)"""
    out = {}
    sf = corb.StereoFrontend(nfeatures=KITTI["nfeatures"], width=KITTI["width"], height=KITTI["height"], max_frames=8, fx=KITTI["fx"], bf=KITTI["bf"], device=device)
    lay = sf.frame_layout()
    frames = [np.stack(synth.stereo_pair(1000 + i)) for i in range(8)]
    for B in (1, 2, 8):
        pin_in = corb.pinned_empty((B,) + frames[0].shape, np.uint8)
        for k in range(B):
            pin_in[k] = frames[k]
        pin_out = corb.pinned_empty((B * lay.frame_bytes,), np.uint8)
        for _ in range(20):
            sf.frames(pin_in, pin_out)
        ts = []
        for i in range(calls):
            pin_in[0, 0, 0, 0] = i & 255                         # (the buffer is rewritten by the client between calls; one byte keeps the host honest)
            t0 = time.perf_counter(); sf.frames(pin_in, pin_out); ts.append(time.perf_counter() - t0)
        ts = np.sort(np.array(ts)) * 1e3
        tm = corb.StereoFrameTiming(); st = []
        for _ in range(60):
            sf.frames(pin_in, pin_out, tm); st.append((tm.ms_upload, tm.ms_kernels, tm.ms_download))
        st = np.median(np.array(st), axis=0)
        rs = []
        for _ in range(calls):
            t0 = time.perf_counter(); sf.run(B); sf.sync(); rs.append(time.perf_counter() - t0)
        o = sf.unpack_frame(pin_out, 0)
        med = float(np.median(ts))
        out["B%d" % B] = dict(host_to_host_ms=round(med, 4), p90_ms=round(float(ts[int(0.9 * len(ts))]), 4), per_frame_ms=round(med / B, 4), stereo_fps=round(B / med * 1e3, 1),
                              stages_ms=dict(upload=round(float(st[0]), 4), kernels=round(float(st[1]), 4), download=round(float(st[2]), 4),
                                             residual=round(med - float(st.sum()), 4)),
                              resident_ms=round(float(np.median(rs)) * 1e3, 4), calls=calls,
                              bytes_in=int(pin_in.nbytes), bytes_out=int(pin_out.nbytes), n_left=int(len(o["kl"])), n_matched=int(o["n_matched"]))
    sf.orb.profile(2)
    for _ in range(20):
        sf.run(1)
    sf.sync()
    out["kernels_alone_us_B1"] = dict((k, round(v[0] / v[1] * 1e3, 2)) for k, v in sf.orb.profile_read().items() if v[1])
    sf.orb.profile(False)
    out["note"] = ("corb_stereo_frames: page-locked host buffers in and out, one H2D + captured kernel chain (12 launches) + one D2H + one synchronisation per call; "
                   "a reference client is paced at 10 fps (Examples/Stereo/KITTI00-02.yaml:22)")
    sf.close()
    return out


FP64_PEAK_TFLOPS = 78.6        # public MI355X FP64 vector = matrix peak; measured here: 78.1 (v_mfma_f64_16x16x4) / 76 (v_fma_f64), profiles/r02_ubench/mfma_f64.txt


def ba_bench(corb, synth, device, cpu_kf, big_kf):
    """Secondary metric of BASELINE.json: global-BA LM iterations/s on the fused 8-client problem of SURVEY s8d(ii), server setting (10
    iterations, non-robust; corbslam_server/src/GlobalOptimize.cpp:444).  Two sizes:
      config5   : 8 x big_kf keyframes (default 6 250 = 50 000 keyframes), 100 points per keyframe (5 M), each seen by its 3..8 nearest
                  keyframes (~27.5 M observations) -- BASELINE configs[4]; GPU only (the CPU needs minutes per iteration at this size)
      same_size : 8 x cpu_kf keyframes at the same density, solved on the GPU AND by the CPU oracle with the reference's solver class
                  (block-sparse LDL^T, one thread like g2o without OpenMP) -- the two figures of this record are comparable
    iters_per_s counts wall time of the C-ABI call (host arrays in, host arrays out: flattening, transfers and the device work)."""
    out = {}
    for tag, kf in (("config5", big_kf), ("same_size", cpu_kf)):
        if kf <= 0:
            continue
        t0 = time.perf_counter()
        prob = synth.ba_problem_fast(n_clients=8, kf_per_client=kf, pts_per_kf=100, seed=1000, obs_range=(3, 8), window=6)
        gen_s = time.perf_counter() - t0
        args = (prob["poses"], prob["pose_fixed"], prob["points"], prob["point_fixed"], prob["edges"],
                prob["fx"], prob["fy"], prob["cx"], prob["cy"], prob["bf"])
        corb.Optimizer.GlobalBundleAdjustemnt(*args, nIterations=2, bRobust=False, device=device, intr=prob["intr"])        # warm-up (library loading, arena growth)
        t0 = time.perf_counter()
        g = corb.Optimizer.GlobalBundleAdjustemnt(*args, nIterations=10, bRobust=False, device=device, intr=prob["intr"])
        dt = time.perf_counter() - t0
        st = g["structure"]; ms = g["ms"]
        rec = dict(poses=int(len(prob["poses"])), points=int(len(prob["points"])), edges=int(len(prob["edges"])), generator_s=round(gen_s, 1),
                   iters=int(g["iters_done"]), trials=int(g["trials"]), wall_s=round(dt, 4),
                   iters_per_s=round(g["iters_done"] / dt, 2), device_iters_per_s=round(g["iters_done"] / (ms["total"] * 1e-3), 2),
                   device_ms=dict((k, round(v, 3)) for k, v in ms.items()), solver=int(g["solver"]), pcg_iterations=int(g["pcg_iterations"]), pc_levels=int(st.get("pc_levels", 0)),
                   structure=dict((k, int(v)) for k, v in st.items()),
                   chi2_first=float(g["chi2"][0]), chi2_last=float(g["chi2"][-1]),
                   # what the call certifies about itself (CorbBAResult): the TRUE relative residual |b - S x| / |b| of its reduced solves, recomputed in FP64 by a
                   # kernel independent of the CG kernels (max over the solves, and the last), and |J' Omega r|_inf at the returned estimates
                   certificate=dict((k, float(v)) for k, v in g.get("certificate", {}).items()))
        if g["solver"] == 2 and g["pcg_iterations"] > 0:
            # dominant kernels = one CG iteration of the reduced solve (ba_pcg_spmv_kernel + ba_pcg_step_big_kernel): HBM-bound.  Algorithmic bytes
            # per CG iteration: the 6x6 blocks of S (288 B each) + their column indices, the preconditioner's dense diagonal blocks, the vectors
            # (p, z read by the neighbours; r, q, x, p, z read and written once).  Duration = the HIP-event time of the solve phase / CG iterations.
            sp = 6 * st["free_poses"]; pcg = max(st["pc_block"], 1)
            # (blocks up to 128 x 128 are stored in single precision; like S they are symmetric and needed once: n (n + 1) / 2 entries -- the step kernel reads them as
            # upper-triangle tiles, 21 x 1 KB per 96 x 96 block, since late round 5; before, this line charged the full square the kernel then read)
            npc = 6 * pcg
            pc_bytes = (st["free_poses"] + pcg - 1) // pcg * (npc * (npc + 1) // 2) * (4 if npc <= 128 else 8) if pcg > 1 else st["free_poses"] * 288
            # S is symmetric and stored / needed once: the blocks on and above the diagonal (the strict count; until round 4 this line charged both triangles,
            # which is what a kernel that reads the lower blocks a second time MOVES, not what the product needs)
            nu_blocks = (st["nnz_blocks"] + st["free_poses"]) // 2
            by = nu_blocks * 288 + st["nnz_blocks"] * 4 + pc_bytes + 10 * sp * 8
            L = int(st.get("pc_levels", 0)); ml_bytes = 0
            if L > 0:
                # multilevel preconditioner (csrc/ba_multilevel.h): the block inverses of the coarse levels (nodes ~ poses / 8 * 4/3, 16 per 96 x 96 single-precision
                # block), the restriction / prolongation tables ((keyframe, weight) entries: level k holds <= k + 1 per keyframe; 12 B each, read twice) and the
                # residual / correction values they gather (48 B per entry, from L2)
                nodes = st["free_poses"] / 8.0 * 4.0 / 3.0; entries = st["free_poses"] * L * (L + 3) / 2.0
                ml_bytes = int(nodes / 16.0 * 96 * 96 * 4 + entries * 2 * 12)
                by += ml_bytes
            avg_s = ms["solve"] * 1e-3 / g["pcg_iterations"]
            ach = by / avg_s / 1e9
            trials = max(int(g["trials"]), 1)
            # the MFMA path (Schur complement): 216 flop per (edge, edge) pair; phase time = V + products (+ reduced rhs, formed by the row kernel) + preconditioner set-up
            schur_flops = st["schur_pairs"] * 216.0
            # kernel-level figures of the same workload from the committed rocprofv3 set (tools/gpu_profile_ba_store.sh -> tools/ba_profile_to_json.py ->
            # profiles/ba_latest.json): average kernel durations and FETCH_SIZE + WRITE_SIZE per launch, next to the phase-derived figure of this run
            kern = None; traffic = None; mf = {}
            try:
                pj = json.load(open(os.path.join(ROOT, "profiles", "ba_latest.json")))
                if int(pj.get("poses", -1)) != len(prob["poses"]):
                    raise RuntimeError("no committed profile at this size (profiles/ba_latest.json: %s keyframes)" % pj.get("poses"))
                kk = pj["kernels"]; spmv = kk["ba_pcg_spmv_kernel"]; stp = kk.get("ba_pcg_step_restrict_kernel") or kk["ba_pcg_step_big_kernel"]      # (the step kernel's launch carries the restriction)
                by_spmv = nu_blocks * 288 + st["nnz_blocks"] * 4 + 4 * sp * 8; by_step = pc_bytes + 6 * sp * 8
                mlk = dict((k, dict(avg_us=kk[k]["avg_us"], hbm_bytes_per_launch=kk[k].get("hbm_bytes_per_launch"))) for k in ("ml_apply_kernel", "ml_prolong_kernel") if k in kk)
                kern = dict(profile=pj.get("source"), multilevel=mlk, multilevel_algorithmic_bytes=ml_bytes,
                            ba_pcg_spmv_kernel=dict(avg_us=spmv["avg_us"], hbm_bytes_per_launch=spmv.get("hbm_bytes_per_launch"), algorithmic_bytes=int(by_spmv),
                                                    GBps_algorithmic=round(by_spmv / (spmv["avg_us"] * 1e-6) / 1e9, 1)),
                            ba_pcg_step_restrict_kernel=dict(avg_us=stp["avg_us"], hbm_bytes_per_launch=stp.get("hbm_bytes_per_launch"), algorithmic_bytes=int(by_step),
                                                        GBps_algorithmic=round(by_step / (stp["avg_us"] * 1e-6) / 1e9, 1)),
                            kernel_sum_us=round(spmv["avg_us"] + stp["avg_us"] + sum(v["avg_us"] for v in mlk.values()), 2),
                            note="profile = the same problem under rocprofv3 (kernels launched one by one: CORB_BA_NO_GRAPH).  An iteration is four dependent launches: SpMV, step kernel + "
                                 "restriction (one launch), coarse block solves, prolongation; avg_us of this run minus kernel_sum_us = what the dependent launches inside the captured "
                                 "graph and the chunk read-backs cost per CG iteration")
                if spmv.get("hbm_bytes_per_launch") is not None and stp.get("hbm_bytes_per_launch") is not None:
                    traffic = int(spmv["hbm_bytes_per_launch"] + stp["hbm_bytes_per_launch"])
                sm = kk.get("ba_schur_row_stream_kernel") or kk.get("ba_schur_row_kernel") or kk.get("ba_schur_mfma_kernel")
                if sm and "sq" in sm:
                    # SQ_VALU_MFMA_BUSY_CYCLES summed over the SIMDs / (kernel duration x 2.4 GHz x 1024 SIMDs)
                    mf = dict(kernel="ba_schur_row_stream_kernel" if "ba_schur_row_stream_kernel" in kk else "ba_schur_row_kernel", kernel_avg_us=sm["avg_us"], hbm_bytes_per_launch=sm.get("hbm_bytes_per_launch"), insts_mfma=int(sm["sq"].get("SQ_INSTS_MFMA", 0)),
                              busy_frac=round(sm["sq"].get("SQ_VALU_MFMA_BUSY_CYCLES", 0.0) / (sm["avg_us"] * 1e-6 * 2.4e9 * 1024), 4),
                              tflops_of_kernel=round(schur_flops / (sm["avg_us"] * 1e-6) / 1e12, 2))
            except Exception as e:
                kern = dict(unavailable=str(e)[:200])
            rec["roofline"] = dict(bound="hbm", kernel="ba_pcg_spmv_kernel + ba_pcg_step_restrict_kernel + ml_apply_kernel + ml_prolong_kernel (one CG iteration of the reduced solve)", kernels=kern,
                                   achieved=round(ach, 1), peak=HBM_PEAK_GBS, unit="GB/s", frac=round(ach / HBM_PEAK_GBS, 4), traffic=traffic,
                                   avg_us=round(avg_s * 1e6, 2), algorithmic_bytes=int(by), share_of_device_time=round(ms["solve"] / ms["total"], 3),
                                   schur_mfma=dict(flops_per_trial=int(schur_flops), phase_ms_per_trial=round(ms["schur"] / trials, 3),
                                                   tflops_of_phase=round(schur_flops / (ms["schur"] / trials * 1e-3) / 1e12, 3), peak_tflops=FP64_PEAK_TFLOPS,
                                                   note="FP64 matrix peak = FP64 vector peak on this part; phase = V + products (the row kernel also forms the reduced right-hand side) + preconditioner set-up", **mf))
        # the same problem solved FROM DEVICE-RESIDENT STORE RECORDS (what the server rank holds after a map push + re-basing): graph derived and flattened on the
        # device (store_kernels.hip, ba_flatten.hip), estimates written back into the records; nLoopKF != 0 like the server's call (GlobalOptimize.cpp:444), so the
        # records' Tcw / world_pos stay and the timed call solves the same problem as the warm-up.  Staging the records from host arrays is set-up, not timed.
        try:
            t0 = time.perf_counter()
            ma = synth.map_arrays(prob, kf, 100)
            KF = corb.KeyFrameStore(len(prob["poses"]), ma["max_features"], device=device); MP = corb.MapPointStore(len(prob["points"]), ma["max_obs"], device=device)
            KF.put_batch(0, ma["meta"], ma["feat_off"], ma["kp"], None, ma["ur"], None, ma["mp_id"])
            MP.put(0, ma["mp_records"], ma["obs_off"], ma["obs_kf"], ma["obs_idx"])
            stage_s = time.perf_counter() - t0
            ks = np.arange(len(prob["poses"]), dtype=np.int32); ms_ = np.arange(len(prob["points"]), dtype=np.int32)
            corb.GlobalBundleAdjustemntStore(KF, ks, MP, ms_, nIterations=2, bRobust=False, nLoopKF=7, fetch=False)
            t0 = time.perf_counter()
            gs = corb.GlobalBundleAdjustemntStore(KF, ks, MP, ms_, nIterations=10, bRobust=False, nLoopKF=7, fetch=False)
            dts = time.perf_counter() - t0
            rec["store"] = dict(wall_s=round(dts, 4), iters_per_s=round(gs["iters_done"] / dts, 2), device_iters_per_s=round(gs["iters_done"] / (gs["ms"]["total"] * 1e-3), 2),
                                device_ms=dict((k, round(v, 3)) for k, v in gs["ms"].items()), iters=int(gs["iters_done"]), trials=int(gs["trials"]), pcg_iterations=int(gs["pcg_iterations"]),
                                chi2_last=float(gs["chi2"][-1]), chi2_rel_diff_vs_host_arrays=float(abs(gs["chi2"][-1] - g["chi2"][-1]) / g["chi2"][-1]),
                                structure_equal=bool(all(int(gs["structure"][k]) == int(st[k]) for k in st)),
                                record_bytes=dict(keyframe=int(KF.record_bytes()), map_point=int(MP.record_bytes())), staging_s=round(stage_s, 2),
                                note="corb_ba_solve_store: keyframe / map-point records in HBM -> edges, index maps, sorted lists, block pattern by kernels -> LM -> write-back into the records; no host flattening, no uploads")
            KF.close(); MP.close()
        except Exception as e:
            rec["store"] = dict(error=str(e)[:300])
        # "a second run robust=true" -- the same problem with the Huber kernel (delta = sqrt(5.991) / sqrt(7.815), Optimizer.cc:47-48 with bRobust;
        # robust_kernel_impl.cpp:78-91): the weights change every iteration, the structure and the kernels are the same
        try:
            t0 = time.perf_counter()
            gh = corb.Optimizer.GlobalBundleAdjustemnt(*args, nIterations=10, bRobust=True, device=device, intr=prob["intr"])
            dth = time.perf_counter() - t0
            rec["huber"] = dict(wall_s=round(dth, 4), iters_per_s=round(gh["iters_done"] / dth, 2), device_iters_per_s=round(gh["iters_done"] / (gh["ms"]["total"] * 1e-3), 2),
                                device_ms=dict((k, round(v, 3)) for k, v in gh["ms"].items()), iters=int(gh["iters_done"]), trials=int(gh["trials"]), pcg_iterations=int(gh["pcg_iterations"]),
                                chi2_first=float(gh["chi2"][0]), chi2_last=float(gh["chi2"][-1]), note="bRobust = true, host arrays in / out like iters_per_s above")
        except Exception as e:
            rec["huber"] = dict(error=str(e)[:300])
        if tag == "config5":
            # what a caller who accepts a looser reduced solve gets (CorbBAOptions.pcg_tol = 1e-4, fixed: no forcing sequence, no continuation) beside the default policy
            # (1e-6 -> 1e-8, decisions guarded): informational -- the figures above are the default's.  On the oracle goldens (4 800 / 12 000 keyframes) a 1e-4 solve stays
            # 300x inside the parity bars; on noisy maps with rejected trials it does not (corb_ba.cpp: BA_PCG_TOL_LOOSE), which is why it is not the default.
            try:
                gl = corb.Optimizer.GlobalBundleAdjustemnt(*args, nIterations=10, bRobust=False, device=device, intr=prob["intr"], pcg_tol=1e-4)
                same = len(gl["chi2"]) == len(g["chi2"])
                rec["fixed_tol_1e-4"] = dict(device_iters_per_s=round(gl["iters_done"] / (gl["ms"]["total"] * 1e-3), 2), pcg_iterations=int(gl["pcg_iterations"]),
                                             chi2_rel_dev_vs_default=float(np.max(np.abs(gl["chi2"] / g["chi2"] - 1.0))) if same else None,
                                             pose_dev_vs_default=float(np.abs(gl["poses"] - g["poses"]).max()), trials=int(gl["trials"]))
            except Exception as e:
                rec["fixed_tol_1e-4"] = dict(error=str(e)[:200])
        if tag == "same_size":
            from oracle import pyorc
            pyorc.ba_set_solver(2, native=True)
            t0 = time.perf_counter()
            c = pyorc.ba_solve(*args, iters=10, robust=False, native=True, intr=prob["intr"])
            dtc = time.perf_counter() - t0
            pyorc.ba_set_solver(0, native=True)
            rec["cpu_baseline"] = dict(value=round(c["iters_done"] / dtc, 3), unit="LM iterations/s", cores=1, kind="port",
                                       sample="the same %d-keyframe / %d-point / %d-observation problem, 10 iterations, oracle with the reference's solver class "
                                              "(block-sparse LDL^T), 1 thread like g2o without OpenMP" % (len(prob["poses"]), len(prob["points"]), len(prob["edges"])),
                                       wall_s=round(dtc, 2), chi2_last=float(c["chi2"][-1]),
                                       chi2_rel_diff_vs_gpu=float(abs(c["chi2"][-1] - g["chi2"][-1]) / c["chi2"][-1]))
        out[tag] = rec
    return out


def ba_summary(rec):
    """config-5-size global BA in a dozen numbers (metric (ii) of BASELINE.json), for the objects of the line the driver's record keeps whole"""
    rf = rec.get("roofline") or {}; sm = rf.get("schur_mfma") or {}
    return dict(metric="global-BA LM iterations/s, fused 8-client map", poses=rec["poses"], points=rec["points"], observations=rec["edges"], lm_iterations=rec["iters"], trials=rec["trials"],
                device_iters_per_s=rec["device_iters_per_s"], iters_per_s_host_arrays=rec["iters_per_s"], iters_per_s_records=(rec.get("store") or {}).get("iters_per_s"),
                iters_per_s_huber=(rec.get("huber") or {}).get("iters_per_s"), device_ms=rec["device_ms"], pcg_iterations=rec["pcg_iterations"],
                bound=rf.get("bound"), kernel="one CG iteration of the reduced solve (SpMV + step/restrict + coarse + prolong)", achieved=rf.get("achieved"), peak=rf.get("peak"), unit=rf.get("unit"),
                frac=rf.get("frac"), traffic=rf.get("traffic"), algorithmic_bytes=rf.get("algorithmic_bytes"), avg_us=rf.get("avg_us"), share_of_device_time=rf.get("share_of_device_time"),
                schur_mfma=dict((k, sm.get(k)) for k in ("kernel_avg_us", "tflops_of_kernel", "busy_frac", "tflops_of_phase", "phase_ms_per_trial", "peak_tflops", "kernel") if k in sm),
                certificate=rec.get("certificate"), chi2_first=rec["chi2_first"], chi2_last=rec["chi2_last"])


def ba_cpu_summary(rec):
    """the BA problem solved on the GPU and by the CPU oracle (reference's solver class): the two comparable figures"""
    c = rec.get("cpu_baseline") or {}
    return dict(value=c.get("value"), unit=c.get("unit"), cores=c.get("cores"), kind=c.get("kind"), sample=c.get("sample"), wall_s=c.get("wall_s"),
                chi2_rel_diff_vs_gpu=c.get("chi2_rel_diff_vs_gpu"), gpu_iters_per_s=rec["iters_per_s"], gpu_device_iters_per_s=rec["device_iters_per_s"],
                gpu_iters_per_s_records=(rec.get("store") or {}).get("iters_per_s"))


def compact_line(out):
    """The line the driver parses, below 8 KB: notes, per-kernel tables and the figures already carried by roofline.ba_config5 / cpu_baseline.ba_same_size dropped
    (the long form: stderr with --full, the file of --record, or the line itself with --long-line)."""
    drop = {"note", "kernels", "structure", "sample_note", "generator_s", "record_bytes", "staging_s", "per_level", "source", "whole_step", "alone_unsplit_avg_us",
            "bytes_in", "bytes_out", "calls", "n_left", "n_matched", "p90_ms", "mean", "checks_passed", "kernels_alone_us_B1", "whole_box_extrapolated"}

    def strip(o, depth=0):
        if isinstance(o, dict):
            return dict((k, strip(v, depth + 1)) for k, v in o.items() if not (k in drop and depth > 0 and not (k == "kernels" and not isinstance(v, dict))))
        if isinstance(o, list):
            return [strip(v, depth + 1) for v in o]
        if isinstance(o, float):
            return float("%.6g" % o)
        return o
    keep_whole = dict((k, out[k]) for k in ("config",))
    c = strip(out)
    c.update(keep_whole)
    if isinstance(out.get("roofline"), dict):             # the headline kernel's table stays (it is what `frac` is read against)
        c["roofline"] = strip(dict((k, v) for k, v in out["roofline"].items() if k != "kernels"), 1)
        if "kernels" in out["roofline"]:
            c["roofline"]["kernels"] = strip(out["roofline"]["kernels"])
    cl = c.get("client_loop")
    if isinstance(cl, dict) and isinstance(cl.get("cpu_baseline"), dict):
        cl["cpu_baseline"] = dict((k, v) for k, v in cl["cpu_baseline"].items() if k in ("value", "unit", "cores", "kind", "error"))
    if isinstance(c.get("ba"), dict):
        for tag, rec in c["ba"].items():
            if isinstance(rec, dict):
                for k in ("roofline", "cpu_baseline", "certificate", "chi2_first", "solver", "pc_levels", "wall_s", "trials", "iters") + (("poses", "points", "edges", "device_ms", "chi2_last") if tag == "config5" else ()):
                    rec.pop(k, None)
                for k in ("store", "huber"):
                    if isinstance(rec.get(k), dict):
                        rec[k] = dict((kk, vv) for kk, vv in rec[k].items() if kk in ("iters_per_s", "device_iters_per_s", "pcg_iterations", "chi2_last", "structure_equal", "chi2_rel_diff_vs_host_arrays", "error"))
    return c


DUMP_FRAMES = 32            # frames of the last step's output written by --dump-outputs (~0.6 MB each as float32)


def dump_outputs(h, B, d):
    """--dump-outputs: what the timed path handed its caller in the last step (StereoFrontend.fetch of each frame), for a fixed, seeded sample of the step's
    B frames, as float32 / float64 .npy files: per-frame counts, keypoints (x, y, size, angle, response, octave, class_id), descriptor bytes, u_right, depth."""
    os.makedirs(d, exist_ok=True)
    idx = np.sort(np.random.default_rng(0).choice(B, size=min(B, DUMP_FRAMES), replace=False))
    res = [h.fetch(int(f)) for f in idx]
    kp = lambda k: np.stack([k[n].astype(np.float32) for n in k.dtype.names], 1).reshape(-1, len(k.dtype.names))
    arrs = dict(frames=idx.astype(np.float64),
                n_matched=np.array([o["n_matched"] for o in res], np.float64),
                left_counts=np.array([len(o["kl"]) for o in res], np.float64), right_counts=np.array([len(o["kr"]) for o in res], np.float64),
                left_keypoints=np.concatenate([kp(o["kl"]) for o in res]), right_keypoints=np.concatenate([kp(o["kr"]) for o in res]),
                left_descriptors=np.concatenate([o["dl"].astype(np.float32) for o in res]).reshape(-1, 32),
                right_descriptors=np.concatenate([o["dr"].astype(np.float32) for o in res]).reshape(-1, 32),
                u_right=np.concatenate([o["u_right"] for o in res]).astype(np.float32), depth=np.concatenate([o["depth"] for o in res]).astype(np.float32))
    assert sum(a.nbytes for a in arrs.values()) < 64 << 20
    for k, a in arrs.items():
        np.save(os.path.join(d, k + ".npy"), a)


def main():
    if len(sys.argv) >= 5 and sys.argv[1] == "--cpu-worker":          # one client of cpu_baseline's throughput sample (no GPU, no torch)
        import corbload
        corbload.load_pkg()
        from corb_slam_amd import synth
        print("elapsed", cpu_client(int(sys.argv[3]), synth, int(sys.argv[2]), float(sys.argv[4])))
        return
    # stdout carries exactly ONE JSON line: everything the libraries print meanwhile (RCCL's version banner, rocBLAS notices) goes to stderr
    real_stdout = os.dup(1); os.dup2(2, 1)
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--batch", type=int, default=512, help="stereo frames per step (per GPU); a run is issued as two part-batches, see corb_run_parts")
    ap.add_argument("--cpu-frames", type=int, default=96, help="with --full: frames of the CPU baseline sample (0 = skip)")
    ap.add_argument("--no-profile", action="store_true", help="with --full: no HIP-event pairs in the timed region (no roofline)")
    ap.add_argument("--no-extras", action="store_true", help="with --full: only the timed region and its roofline (for rocprofv3 runs: no stand-alone kernel timing, no host-buffer / map-push / BA / replay legs)")
    ap.add_argument("--inflight", type=int, default=1, help="batches in flight per GPU (independent handles/streams, steps alternate between them)")
    ap.add_argument("--ba-cpu-kf", type=int, default=150, help="with --full: keyframes/client (x8) of the BA problem that is solved on the GPU AND on the CPU oracle (0 = skip)")
    ap.add_argument("--replay-frames", type=int, default=400, help="with --full: frames of the configs[2] client-loop replay (0 = skip)")
    ap.add_argument("--full", action="store_true", help="besides the headline, measure everything else: roofline (event pairs in the timed region), repeats, host buffers, map push, "
                                                         "CPU baselines, BA, 1080p, latency and client loop; the long record (~16 KB) goes to stderr")
    ap.add_argument("--long-line", action="store_true", help="print the long record (every note and per-kernel table) as the line instead of the compact one (< 8 KB)")
    ap.add_argument("--record", metavar="FILE", help="also write the long record to FILE")
    ap.add_argument("--dump-outputs", metavar="DIR", help="after the timed steps, write what the last step computed (a fixed sample of %d frames) as DIR/<name>.npy" % DUMP_FRAMES)
    ap.add_argument("--ba-kf", type=int, default=6250, help="with --full: keyframes/client (x8) of the config-5-size BA problem, GPU only (0 = skip)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    profile = args.full and not args.no_profile          # a plain run times the steps alone: no event pairs, no legs beside the headline
    if not args.full or args.no_extras:
        args.no_extras = True
        args.cpu_frames = 0; args.ba_cpu_kf = 0; args.ba_kf = 0; args.replay_frames = 0

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` without a launcher: start the N ranks ourselves, one per GPU, exactly as the driver's torch.distributed.run line does
        # (its stdout -- rank 0's ONE JSON line -- is ours); a rank count the node cannot serve is an error, not a silent 1-GPU run
        os.dup2(real_stdout, 1)
        import socket
        import subprocess
        with socket.socket() as so:
            so.bind(("127.0.0.1", 0)); port = so.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1", "--master-port", str(port),
               os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.call(cmd))
    rank = int(os.environ.get("RANK", "0")); world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if os.environ.get("CORB_BENCH_RANK_MARK_DIR"):       # tests: every started rank leaves a marker file before anything can stop it (tests/test_parallel_gloo.py)
        open(os.path.join(os.environ["CORB_BENCH_RANK_MARK_DIR"], "rank%d_of_%d" % (rank, world)), "w").close()
    if world != max(args.gpus, 1) and rank == 0:
        print("bench.py: --gpus %d but the launcher started %d ranks; the line reports the ranks that ran" % (args.gpus, world), file=sys.stderr)
    import torch
    dist = None
    ndev = torch.cuda.device_count()
    dev_index = local_rank % max(ndev, 1)               # one rank per GPU (the driver launches N ranks on N GPUs)
    if world > ndev and os.environ.get("CORB_BENCH_BACKEND", "nccl") == "nccl":
        raise SystemExit("bench.py: %d ranks but %d GPUs visible -- one client per GPU (RCCL cannot place two ranks on one device)" % (world, ndev))
    backend = os.environ.get("CORB_BENCH_BACKEND", "nccl")     # "gloo" lets the N>1 logic be exercised on a 1-GPU box
    if torch.cuda.is_available():
        torch.cuda.set_device(dev_index)
    if world > 1:
        import torch.distributed as dist
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", dev_index))
        else:
            dist.init_process_group(backend=backend)
    red_dev = "cuda" if (dist is not None and backend == "nccl") else "cpu"

    import corbload
    corb = corbload.load_pkg()
    from corb_slam_amd import synth
    if corb.device_count() < 1:
        raise SystemExit("bench.py: no MI355X visible (the product has no CPU fallback)")

    # >= 2 000 frames timed after >= 200 warm-up frames, whatever --steps / --warmup the caller passes: the frames per step grow
    # (in multiples of 32, up to 256) until K steps cover 2 000 frames, and extra untimed warm-up steps are added if W steps are fewer than 200 frames
    B = args.batch
    while B < 256 and B * args.steps < 2000:
        B += 32
    warm_steps = max(args.warmup, -(-200 // B))
    NH = max(1, args.inflight)
    sfs = [corb.StereoFrontend(nfeatures=KITTI["nfeatures"], width=KITTI["width"], height=KITTI["height"],
                               max_frames=B, fx=KITTI["fx"], bf=KITTI["bf"], device=dev_index) for _ in range(NH)]
    sf = sfs[0]
    seed0 = 64 * rank                                   # each rank = one client with its own stream of frames (parallel.client_frame_offset)
    distinct = min(B, 64)
    frames = [synth.stereo_pair(seed0 + i) for i in range(distinct)]
    for h in sfs:
        for s in range(B):
            l, r = frames[s % distinct]
            h.upload(s, l, r)
        h.sync()                                        # inputs resident in HBM

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    if profile:
        for h in sfs:
            h.orb.profile(True); h.orb.profile(False)      # creates the profiler's event pool outside the timed region
    for i in range(warm_steps):
        sfs[i % NH].run(B)
    for h in sfs:
        h.sync()
    barrier()
    t0 = time.perf_counter()
    PROF_EVERY = 8                                      # the kernels of every 8th step carry an event pair (hipExtLaunchKernelGGL: the kernel's own start / stop
    PROF_AT = 4                                         # timestamps, no marker packets) -- steps 4, 12, 20 ...: NOT step 0, whose first part-batch meets an empty GPU after
    for i in range(args.steps):                          # the barrier (its FAST launch ran 0.9 instead of 1.4 ms and pulled the average 10 % under rocprofv3's)
        h = sfs[i % NH]                                  # K steps; step i runs on handle i % NH (own streams)
        if profile:
            h.orb.profile((i // NH) % PROF_EVERY == PROF_AT % PROF_EVERY if args.steps > PROF_AT else i == args.steps - 1)
        h.run(B)
    for h in sfs:
        h.sync()
    barrier()
    dt = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        dump_outputs(sfs[(args.steps - 1) % NH], B, args.dump_outputs)
    prof = {}
    if world > 1:
        # N > 1 is the scaling run: the CPU baselines, the BA legs and the client replay are single-GPU records (rank 0 at N = 1 only); what N ranks add is the
        # weak-scaling figure and the map push between them -- and the other ranks must not sit in the final barrier while rank 0 spends minutes on extras
        args.cpu_frames = 0; args.ba_cpu_kf = 0; args.ba_kf = 0; args.replay_frames = 0
    if profile:
        for h in sfs:
            for k, v in h.orb.profile_read().items():
                a = prof.get(k, (0.0, 0)); prof[k] = (a[0] + v[0], a[1] + v[1])
            h.orb.profile(False)
        # diagnostic, outside the timed region: the same B frames unsplit on one stream, i.e. every kernel alone on the GPU
        # (in the product sequence a launch shares the GPU with the other part-batch's kernels, which stretches it)
        alone = {}
        sf.orb.profile(2)
        for _ in range(0 if args.no_extras else 4):
            sf.run(B)
        sf.sync()
        for k, v in sf.orb.profile_read().items():
            if v[1]:
                alone[k] = round(v[0] / v[1] * 1e3, 2)
        sf.orb.profile(False)
    from corb_slam_amd import parallel
    dt_rank = dt
    # spread: the same K steps three more times, outside the timed region (box-to-box the figure moves by ~3 %; this shows the run-to-run part)
    repeats = []
    for _ in range(0 if args.no_extras else 3):
        barrier(); t1 = time.perf_counter()
        for i in range(args.steps):
            sfs[i % NH].run(B)
        for h in sfs:
            h.sync()
        barrier(); repeats.append(time.perf_counter() - t1)
    dt, total_frames = parallel.reduce_step_time(dist, dt, B * args.steps, device=red_dev)   # MAX time, SUM frames
    per_rank_fps = parallel.gather_scalars(dist, B * args.steps / dt_rank, device=red_dev)  # every rank's own frames/s (N = 1 comparable with the 1-GPU line)
    repeats = [parallel.reduce_step_time(dist, t, B * args.steps, device=red_dev) for t in repeats]

    # client -> server map push (replaces the ROS service batches of DataDriver.cc:135-193 / MapFusion.cpp:31-190): every rank files the keyframe of
    # its frame 0 in its device-resident keyframe store (device-to-device from the front-end) with pose / intrinsics / per-feature map-point ids, a block of
    # map-point records in its map-point store, and corb_map_push_ex sends both to the server rank: header all-gather, the root's verdict, one message per rank
    # and store on the device buffers -- C-ABI + RCCL, no torch tensors, no host staging.  torch.distributed only carries the 128-byte communicator id.  With
    # one rank the records travel rank 0 -> rank 0 through the same calls.  Outside the timed region; never fatal.
    map_push = None
    abandon = False
    try:
        if args.no_extras:
            pass
        elif dist is not None and backend != "nccl":
            map_push = dict(skipped="CORB_BENCH_BACKEND=%s: the push is RCCL-only (its bookkeeping: tests/test_push_plan.py, tests/test_gpu_mapstore.py)" % backend)
        else:
            # This leg is the only place where the ranks talk to each other through the library's own RCCL communicator.  The push itself is collective-safe
            # (every rank returns the same verdict before a record moves), but a rank that DIED here would still leave the others in a collective and the
            # run without its line, so the leg runs under a watchdog: after 120 s the rank gives it up, reports that, and leaves through os._exit.
            box = {}
            NMP = 4096                                   # map-point records per client and push
            def push_leg():
                try:
                    if torch.cuda.is_available():
                        torch.cuda.set_device(dev_index)       # (the current device is per thread)
                    cap = corb.load().corb_orb_capacity(sf.orb.h)
                    store = corb.KeyFrameStore(world + 1, cap, device=dev_index)
                    mps = corb.MapPointStore(NMP * (world + 1), 16, device=dev_index)
                    kid = 1_000_000 * rank + 1
                    store.put_from_stereo(0, sf, 0, keyframe_id=kid)
                    sf.sync()
                    nkp = len(store.get(0)["kp"])
                    T = np.eye(4, dtype=np.float32); T[0, 3] = rank
                    store.set_meta(0, id=kid, client_id=rank + 1, fx=KITTI["fx"], fy=KITTI["fx"], cx=607.1928, cy=185.2157, bf=KITTI["bf"], nlevels=8, Tcw=T.reshape(16))
                    ids = (1_000_000 * rank + 1 + (np.arange(nkp) % NMP)).astype(np.uint64); store.set_map_points(0, ids)
                    rec = np.zeros(NMP, corb.MP_RECORD_DTYPE); rec["id"] = 1_000_000 * rank + 1 + np.arange(NMP); rec["client_id"] = rank + 1; rec["ref_kf_id"] = kid
                    rec["world_pos"] = np.random.default_rng(rank).normal(0, 10, (NMP, 3))
                    mps.put(0, rec, np.arange(NMP + 1, dtype=np.int32), np.full(NMP, kid, np.uint64), (np.arange(NMP) % max(nkp, 1)).astype(np.uint32))
                    ident = [corb.Comm.unique_id() if rank == 0 else None]
                    if dist is not None:
                        dist.broadcast_object_list(ident, src=0)
                    comm = corb.Comm(ident[0], rank, world, device=dev_index)
                    kdst = list(range(1, world + 1)); mdst = [NMP * (1 + r) for r in range(world)]
                    mp_sl = np.arange(NMP, dtype=np.int32); kf_sl = np.zeros(1, np.int32)      # (slot lists as arrays: building a 4 096-entry Python list per call cost more than the push)
                    push = lambda: comm.map_push_ex(store, kf_sl, mps, mp_sl, root=0, kf_dst_first=kdst, mp_dst_first=mdst)
                    push()                                                              # warm-up (connection setup)
                    barrier()
                    t1 = time.perf_counter()
                    for _ in range(10):
                        cnt = push()
                    barrier()
                    mp_dt = (time.perf_counter() - t1) / 10
                    # the asynchronous form: layout shared once, then begin (ONE header all-gather, records enqueued) ... wait; begin_ms is what the caller's thread is held,
                    # the transfer itself overlaps whatever runs next on other streams
                    async_rec = None
                    try:
                        comm.map_push_setup(0, store if rank == 0 else None, mps if rank == 0 else None, kdst if rank == 0 else None, mdst if rank == 0 else None)
                        comm.map_push_begin(store, kf_sl, mps, mp_sl, root=0); comm.map_push_wait()
                        barrier(); tb = 0.0; t1 = time.perf_counter()
                        for _ in range(10):
                            t2 = time.perf_counter(); comm.map_push_begin(store, kf_sl, mps, mp_sl, root=0); tb += time.perf_counter() - t2
                            acnt = comm.map_push_wait()
                        barrier()
                        async_rec = dict(ms=round((time.perf_counter() - t1) / 10 * 1e3, 3), begin_ms=round(tb / 10 * 1e3, 3),
                                         counts_ok=bool(rank != 0 or (list(acnt[0]) == [1] * world and list(acnt[1]) == [NMP] * world)))
                    except Exception as e:
                        async_rec = dict(error=str(e)[:200])
                    # a push the root must refuse: every rank has to come back with the same error (no rank left in a send)
                    try:
                        comm.map_push_ex(store, kf_sl, mps, mp_sl, root=0, kf_dst_first=[world + 1] * world, mp_dst_first=mdst)      # beyond the root's store (capacity world + 1)
                        refused = False
                    except corb.CorbError as e:
                        refused = "(-1)" in str(e) or "(-2)" in str(e)
                    refused_all = parallel.gather_scalars(dist, 1.0 if refused else 0.0, device=red_dev)
                    if rank == 0:
                        mine = store.get(0); got0 = store.get(1); r0, _, _ = mps.get(0, NMP); g0, gk, gi = mps.get(NMP, NMP)
                        ok = list(cnt[0]) == [1] * world and list(cnt[1]) == [NMP] * world and got0["kp"].tobytes() == mine["kp"].tobytes() and np.array_equal(got0["desc"], mine["desc"]) and all(
                            store.get(1 + r)["id"] == 1_000_000 * r + 1 and store.get_meta(1 + r)["Tcw"][3] == r for r in range(world)) and g0.tobytes() == r0.tobytes() and all(
                            mps.get(NMP * (1 + r), 1)[0]["id"][0] == 1_000_000 * r + 1 for r in range(world)) and np.array_equal(store.get_map_points(1), ids)
                        nbytes = world * (store.record_bytes() + NMP * mps.record_bytes())
                        box["map_push"] = dict(ms=round(mp_dt * 1e3, 3), ranks=world, keyframes=world, map_points=world * NMP, bytes=int(nbytes), backend="rccl (corb_map_push_ex, device buffers)",
                                        verified=bool(ok), refused_push_returned_on_every_rank=bool(all(v == 1.0 for v in refused_all)), GBps=round(nbytes / mp_dt / 1e9, 2),
                                        asynchronous=async_rec,
                                        note="per client one %d-byte keyframe record + %d map-point records of %d bytes to the server rank: header all-gather, verdict all-gather, one "
                                             "ncclSend / ncclRecv per rank and store" % (store.record_bytes(), NMP, mps.record_bytes()))
                    comm.close(); store.close(); mps.close()
                    # the same push with FOUR ranks on this one GPU (in-process transport, one host thread per rank): the N-rank bookkeeping -- header all-gather,
                    # placement verdict, one staged message per rank and store -- measured where N GPUs are not available
                    if rank == 0 and world == 1:
                        import threading
                        W = 4; comms = corb.Comm.local(W, devices=[dev_index] * W)
                        sts = [corb.KeyFrameStore(W + 1, cap, device=dev_index) for _ in range(W)]; mss = [corb.MapPointStore(NMP * (W + 1), 16, device=dev_index) for _ in range(W)]
                        for r_ in range(W):
                            sts[r_].put_from_stereo(0, sf, 0, keyframe_id=1_000_000 * r_ + 1); sf.sync()
                            rc_ = rec.copy(); rc_["id"] = 1_000_000 * r_ + 1 + np.arange(NMP)
                            mss[r_].put(0, rc_, np.arange(NMP + 1, dtype=np.int32), np.full(NMP, 1_000_000 * r_ + 1, np.uint64), (np.arange(NMP) % max(nkp, 1)).astype(np.uint32))
                        kd4 = list(range(1, W + 1)); md4 = [NMP * (1 + r_) for r_ in range(W)]
                        kd4a = np.asarray(kd4, np.int32); md4a = np.asarray(md4, np.int32)
                        def ranks4(n_push):                  # one host thread per rank, each issuing n_push pushes back to back (the collective keeps the ranks in step)
                            out = [None] * W
                            def one(r_):
                                if torch.cuda.is_available():
                                    torch.cuda.set_device(dev_index)
                                for _ in range(n_push):
                                    out[r_] = comms[r_].map_push_ex(sts[r_], kf_sl, mss[r_], mp_sl, root=0, kf_dst_first=kd4a, mp_dst_first=md4a)
                            th = [threading.Thread(target=one, args=(r_,), daemon=True) for r_ in range(W)]
                            t1 = time.perf_counter()
                            for t_ in th: t_.start()
                            for t_ in th: t_.join(60)
                            return out, time.perf_counter() - t1
                        ranks4(2)
                        out4, dt4 = ranks4(50); dt4 /= 50
                        ok4 = out4[0] is not None and list(out4[0][0]) == [1] * W and list(out4[0][1]) == [NMP] * W and all(
                            sts[0].get(1 + r_)["id"] == 1_000_000 * r_ + 1 and mss[0].get(NMP * (1 + r_), 1)[0]["id"][0] == 1_000_000 * r_ + 1 for r_ in range(W))
                        box["map_push"]["local_4_ranks"] = dict(ms=round(dt4 * 1e3, 3), ranks=W, verified=bool(ok4), bytes=int(W * (sts[0].record_bytes() + NMP * mss[0].record_bytes())),
                                                                backend="in-process transport (corb_comm_create_local), four host threads, ONE GPU")
                        for c_ in comms: c_.close()
                        for s_ in sts + mss: s_.close()
                except Exception as e:
                    box["map_push"] = dict(error=str(e)[:300])
            th = threading.Thread(target=push_leg, daemon=True)
            th.start(); th.join(120.0)
            if th.is_alive():
                map_push = dict(error="map push leg did not finish within 120 s (abandoned; the process leaves through os._exit)")
                abandon = True
            else:
                map_push = box.get("map_push")
    except Exception as e:                                                   # the headline line must not depend on this leg
        map_push = dict(error=str(e)[:300])
    if rank == 0:
        # workload statistics for the algorithmic byte counts
        outs = [sf.fetch(s) for s in range(min(B, 8))]
        kp_mean = sum(len(o["kl"]) + len(o["kr"]) for o in outs) / (2.0 * len(outs))
        cand_mean = sum(len(sf.orb.candidates(s, l)) for s in range(min(2 * B, 4)) for l in range(8)) / float(min(2 * B, 4))
        matched = sum(o["n_matched"] for o in outs) / float(len(outs))
        geom = [sf.orb.pyramid_level(0, l).shape[::-1] for l in range(8)]
        ab = algorithmic_bytes(geom, dict(cand=cand_mean, kp=kp_mean))
        roof = None
        if prof:
            tot = sum(v[0] for v in prof.values())
            # dominant kernel: the one that needs the GPU longest when it runs ALONE (stand-alone timing above); the durations inside the pipeline are those of
            # kernels that share the GPU with the other part-batch's, and the two largest are within a few per cent of each other there
            name = max(alone, key=lambda k: alone[k]) if alone and all(k in prof for k in alone) else max(prof, key=lambda k: prof[k][0])
            if not alone and "orb_fast_kernel" in prof:      # (--no-extras, i.e. under rocprofv3: no stand-alone timing -- the dominant kernel of the full runs)
                name = "orb_fast_kernel"
            ms, launches = prof[name]
            # a run of B frames is issued as two part-batches (corb_stereo_run), so one launch covers B/2 frames = B images
            # a run of B frames is issued as two part-batches (corb_orb.cpp: corb_run_parts), so one launch covers B / parts frames
            halves = NPARTS if 2 * B >= 32 else 1
            def per_launch(k):
                units = (2 * B if k.startswith("orb_") else B) / halves      # images (orb_*) or frames (stereo_*) per launch
                return ab[k] * units / (7.0 if k == "orb_resize_kernel" else 1.0)   # 7 resize launches share the per-image figure
            bytes_per_launch = per_launch(name)
            avg_s = (ms / launches) * 1e-3
            achieved = bytes_per_launch / avg_s / 1e9
            traffic = None
            pmc = os.path.join(ROOT, "profiles", "pmc_latest.json")
            if os.path.exists(pmc):
                try:
                    traffic = json.load(open(pmc)).get(name, {}).get("hbm_bytes_per_launch")
                except Exception:
                    traffic = None
            # the kernel is bound by VALU instruction issue, not by memory: instructions per launch from the committed PMC pass
            # (profiles/pmc_sq_latest.txt, SQ_INSTS_VALU) x the measured issue cost of the packed / byte-permute ops it consists of
            valu = None
            try:
                ctr = {}
                for ln in open(os.path.join(ROOT, "profiles", "pmc_sq_latest.txt")):
                    f = ln.split()
                    if name.split("(")[0] in ln and len(f) >= 4 and f[-4] in ("SQ_INSTS_VALU", "SQ_WAVES"):
                        ctr[f[-4]] = float(f[-1])                                    # average per dispatch
                if "SQ_INSTS_VALU" in ctr and ctr.get("SQ_WAVES", 0) > 0:
                    # the counters of a PMC pass may cover the launch several times over (per-XCC instances): normalise by SQ_WAVES and scale to the
                    # wavefronts one launch really has (orb_fast_kernel: one per detection cell of every image of the part-batch)
                    per_wave = ctr["SQ_INSTS_VALU"] / ctr["SQ_WAVES"]
                    cells = sum(int((w_ - 32) / 30.0) * int((h_ - 32) / 30.0) for (w_, h_) in geom)
                    waves = cells * (2 * B // halves) if name.startswith("orb_fast") else ctr["SQ_WAVES"]
                    insts = per_wave * waves; pred = insts * 1.8e-9 / 1024
                    alone_us = alone.get(name)          # the kernel alone on the GPU, unsplit launch = two part-batch launches' worth of work
                    valu = dict(valu_per_wavefront=round(per_wave, 1), wavefronts_per_half_batch_launch=int(waves), insts_per_half_batch_launch=int(insts), ns_per_inst_per_simd=1.8, simds=1024,
                                predicted_us_per_half_batch=round(pred * 1e6, 1),
                                alone_us_per_half_batch=round(alone_us / 2, 1) if alone_us else None,
                                frac_of_issue_bound=round(2 * pred * 1e6 / alone_us, 3) if alone_us else None,
                                source="profiles/pmc_sq_latest.txt (SQ_INSTS_VALU / SQ_WAVES) x tools/ubench/valu_rate.hip (issue cost of v_perm / packed min-max)")
                # the same account for the WHOLE step: every kernel of the path, instructions per part-batch launch x launches per step -- the pipeline overlaps
                # the kernels of two part-batches, so what bounds the step is the sum of their VALU instructions, not any one kernel's time
                per_k = {}
                for ln in open(os.path.join(ROOT, "profiles", "pmc_sq_latest.txt")):
                    f = ln.split()
                    if len(f) >= 4 and f[-4] == "SQ_INSTS_VALU":
                        kn = ln.split("(")[0].split()[-1].split("<")[0]
                        if kn in prof:
                            per_k[kn] = float(f[-1])
                if valu is not None and per_k:
                    pmc_images = ctr["SQ_WAVES"] / cells if name.startswith("orb_fast") else 2 * B / halves      # images per launch in the PMC pass (FAST: one wavefront per cell)
                    tot_insts = sum(per_k.values()) * (2 * B / pmc_images)
                    pred_step = tot_insts * 1.8e-9 / 1024
                    valu["whole_step"] = dict(valu_insts_per_step=int(tot_insts), predicted_us=round(pred_step * 1e6, 1), measured_us=round(dt / args.steps * 1e6, 1),
                                              frac_of_issue_bound=round(pred_step / (dt / args.steps), 3), share={k: round(v / sum(per_k.values()), 3) for k, v in sorted(per_k.items(), key=lambda kv: -kv[1])},
                                              note="sum over the path's kernels of SQ_INSTS_VALU per part-batch launch x part-batches per step x 1.8 ns / 1 024 SIMDs")
            except Exception:
                valu = None
            roof = dict(bound="hbm", kernel=name, achieved=round(achieved, 2), peak=HBM_PEAK_GBS, unit="GB/s",
                        frac=round(achieved / HBM_PEAK_GBS, 5), traffic=traffic,
                        avg_launch_us=round(avg_s * 1e6, 2), share_of_device_time=round(ms / tot, 3),
                        algorithmic_bytes_per_launch=int(bytes_per_launch), valu_issue=valu,
                        kernels={k: dict(avg_us=round(v[0] / v[1] * 1e3, 2), launches=int(v[1]), share=round(v[0] / tot, 3),
                                         GBps=round(per_launch(k) / (v[0] / v[1] * 1e-3) / 1e9, 2))
                                 for k, v in sorted(prof.items(), key=lambda kv: -kv[1][0])},
                        alone_unsplit_avg_us=alone, dominant_by="time alone on the GPU" if alone else "time inside the pipeline")
        # never `value`: the same step with the images handed over as host buffers and every result fetched (one copy each way)
        host_buffers = None
        if not args.no_extras:
            packed = np.ascontiguousarray(np.stack([np.stack(frames[s % distinct]) for s in range(B)]))
            hb_out = sf.fetch_batch(0, B)
            def host_step():
                sf.upload_batch(0, packed); sf.run(B); sf.fetch_batch(0, B, hb_out)
            NHB = 5
            host_step()
            t1 = time.perf_counter()
            for _ in range(NHB):
                host_step()
            hb_dt = (time.perf_counter() - t1) / NHB
            host_buffers = dict(value=round(B / hb_dt, 1), unit="stereo frames/s", ms_per_step=round(hb_dt * 1e3, 3),
                                note="PCIe-inclusive: %.1f MB in + %.1f MB out per step, pageable host memory, transfers and compute serialised" % (
                                    packed.nbytes / 1e6, sum(v.nbytes for v in hb_out.values()) / 1e6))
            # the same with page-locked buffers and TWO handles in a software pipeline: while one handle's results travel back, the other
            # handle's images travel in and its kernels run (what a server fed from the network would do)
            try:
                sf_b = corb.StereoFrontend(nfeatures=KITTI["nfeatures"], width=KITTI["width"], height=KITTI["height"], max_frames=B, fx=KITTI["fx"], bf=KITTI["bf"], device=dev_index)
                pin_in = corb.pinned_empty(packed.shape, np.uint8); pin_in[...] = packed
                pin_out = [dict((k, corb.pinned_empty(v.shape, v.dtype)) for k, v in hb_out.items()) for _ in range(2)]
                pair = [sf, sf_b]
                def pipe(n):
                    pair[0].upload_batch(0, pin_in); pair[0].run(B)
                    for i in range(n):
                        pair[(i + 1) & 1].upload_batch(0, pin_in); pair[(i + 1) & 1].run(B)
                        pair[i & 1].fetch_batch(0, B, pin_out[i & 1])
                    pair[n & 1].sync()
                pipe(3)
                ok = all(np.array_equal(pin_out[j]["counts"], hb_out["counts"]) and np.array_equal(pin_out[j]["desc"][0][: hb_out["counts"][0]], hb_out["desc"][0][: hb_out["counts"][0]]) for j in range(2))
                t1 = time.perf_counter(); NP = 12
                pipe(NP)
                pp_dt = (time.perf_counter() - t1) / (NP + 1)
                host_buffers["pipelined"] = dict(value=round(B / pp_dt, 1), unit="stereo frames/s", ms_per_batch=round(pp_dt * 1e3, 3), verified=bool(ok),
                                                 h2d_GBps=round(packed.nbytes / pp_dt / 1e9, 1), d2h_GBps=round(sum(v.nbytes for v in hb_out.values()) / pp_dt / 1e9, 1),
                                                 note="page-locked host buffers, two handles: transfers of one batch overlap the kernels of the other; "
                                                      "bound by the host link (h2d_GBps = image bytes per second over PCIe), not by the kernels")
                sf_b.close()
            except Exception as e:
                host_buffers["pipelined"] = dict(error=str(e)[:200])
        cpu = cpu_baseline(args.cpu_frames, synth, seed0) if args.cpu_frames > 0 else None
        ba = ba_bench(corb, synth, dev_index, args.ba_cpu_kf, args.ba_kf) if (args.ba_cpu_kf > 0 or args.ba_kf > 0) else None
        hd = None; latency = None
        if not args.no_extras:
            try:
                hd = bench_1080p(corb, synth, dev_index)
            except Exception as e:
                hd = dict(error=str(e)[:300])
            try:
                latency = latency_bench(corb, synth, dev_index)
            except Exception as e:
                latency = dict(error=str(e)[:300])
        # BASELINE configs[2]: one client's Tracking + LocalMapping loop + the server's global BA every 50 keyframes on this GPU, synthetic sequence
        # (tools/replay_client.py; single-frame calls through the C-ABI, i.e. launch / transfer latency bound -- the per-stage times are in the record)
        client = None
        if args.replay_frames > 0:
            try:
                sys.path.insert(0, os.path.join(ROOT, "tools"))
                import replay_client
                rp = replay_client.Replay(corb, synth, None, n_frames=args.replay_frames, kf_every=4, gba_every=50, images=True, check=False, device=dev_index)
                client = rp.run(); rp.close()
                # the same loop with its per-frame tracking stages on device-resident records (corb_track_*: the frame and the map live in stores; the stage results
                # are equal to the host-pointer calls, tests/test_gpu_replay_records.py)
                try:
                    rr = replay_client.Replay(corb, synth, None, n_frames=args.replay_frames, kf_every=4, gba_every=50, images=True, check=False, device=dev_index, records=True)
                    rec = rr.run(); rr.close()
                    client["records"] = dict(client_fps=rec["client_fps"], stage_ms=rec["stage_ms"], same_run=(rec["mean"] == client["mean"] and rec["final_tracking_error_m"] == client["final_tracking_error_m"]),
                                             note="stages 2 and 3 through corb_track_search_last_frame / corb_track_pose_optimization / corb_track_search_local_points; stage 2's time includes the frame's one upload into its record")
                except Exception as e:
                    client["records"] = dict(error=str(e)[:200])
                # the CPU baseline beside it: the oracle (-O3 -march=native, one thread) doing the same calls on the same inputs, timed while it checks a shorter replay
                try:
                    from oracle import pyorc as _po
                    _po.use_native(True)
                    rc_ = replay_client.Replay(corb, synth, _po, n_frames=min(args.replay_frames, 80), kf_every=4, gba_every=50, images=True, check=True, device=dev_index)
                    rep = rc_.run(); rc_.close(); _po.use_native(False)
                    client["cpu_baseline"] = rep.get("cpu_baseline"); client["cpu_baseline_checks"] = dict(passed=int(sum(rep["checks_passed"].values())), errors=len(rep["errors"]))
                except Exception as e:
                    client["cpu_baseline"] = dict(error=str(e)[:200])
                client["note"] = "configs[2]: per-frame stereo front-end + SearchByProjection x2 + PoseOptimization x2; per keyframe (every 4th frame) SearchForTriangulation, Fuse, LocalBundleAdjustment; global BA every 50 keyframes; parity of every stage: tests/test_gpu_replay.py"
            except Exception as e:
                client = dict(error=str(e)[:300])
        out = {
            "metric": "stereo frames/sec ORB extract+match",
            "value": round(total_frames / dt, 2),
            "unit": "stereo frames/s",
            "n_gpus": world, "gpus_requested": args.gpus, "steps": args.steps, "warmup": args.warmup,
            "per_rank_fps": [round(v, 1) for v in per_rank_fps],
            "repeats_fps": [round(u / t, 1) for (t, u) in repeats],
            "ms_per_step": round(dt / args.steps * 1e3, 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "u8", "data": "synthetic",
            "config": {"workload": "configs[1]: ORB extract+match, synthetic 1241x376 stereo stream, 2000 feat/frame, 8 levels x1.2, FAST 20/7",
                       "frames_per_step_per_gpu": B, "timed_frames_per_gpu": B * args.steps, "warmup_frames_per_gpu": B * warm_steps, "batches_in_flight": NH, "launches_per_step": "%d part-batches of %d frames on %d streams, half a pipeline apart" % (NPARTS, B // NPARTS, NPARTS) if 2 * B >= 32 else "1", "distinct_frames": distinct, "parallelism": "1 client per GPU, replicas (no collective)",
                       "mean_keypoints_per_image": round(kp_mean, 1), "mean_candidates_per_image": round(cand_mean, 1),
                       "mean_stereo_matches_per_frame": round(matched, 1), "inputs": "resident in HBM"},
            "roofline": roof,
            "cpu_baseline": cpu,
            "host_buffers": host_buffers,
            "orb_1080p": hd,
            "latency": latency,
            "client_loop": client,
            "map_push": map_push,
            "ba": ba,
        }
        # BASELINE.json's metric has two halves.  The second (global-BA LM iterations/s on the fused 8-client map, configs[4]'s size) goes where the driver's record keeps
        # objects whole -- `roofline` and `cpu_baseline` -- and the line itself stays below 8 KB: the long form (every note, the per-kernel tables)
        # is written to stderr by --full and to the file of --record; `--long-line` prints it as the line instead
        if ba and isinstance(out["roofline"], dict) and "config5" in ba:
            out["roofline"]["ba_config5"] = ba_summary(ba["config5"])
        if ba and isinstance(out["cpu_baseline"], dict) and "same_size" in ba:
            out["cpu_baseline"]["ba_same_size"] = ba_cpu_summary(ba["same_size"])
        full_line = json.dumps(out)
        if args.record:
            try:
                os.makedirs(os.path.dirname(os.path.abspath(args.record)), exist_ok=True)
                with open(args.record, "w") as f:
                    f.write(full_line + "\n")
            except OSError:
                pass
        if not args.long_line:
            if args.full:
                print(full_line, file=sys.stderr)
            out = compact_line(out)
        sys.stdout.flush()
        try:
            import ctypes
            ctypes.CDLL(None).fflush(None)             # C stdio buffers of the libraries (RCCL prints its version banner with printf) go to stderr too
        except Exception:
            pass
        os.dup2(real_stdout, 1)
        print(json.dumps(out, separators=(",", ":")) if not args.long_line else full_line); sys.stdout.flush()
    if abandon:                                          # a collective of the abandoned leg may still be pending: no barrier, no destructors
        sys.stdout.flush(); sys.stderr.flush(); os._exit(0)
    for h in sfs:
        h.close()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
