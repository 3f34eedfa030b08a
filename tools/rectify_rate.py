"""Host-to-host time per call of the stereo per-frame call on raw input (corb_rect_frames, include/corb_stereo_rectify.h) beside corb_stereo_frames on the same
frames rectified beforehand, on the same handle in the same process: the difference is what rectification on the device adds to a frame.

EuRoC calibration (tests/golden/EuRoC.yaml), 752 x 480, 1200 features, 8 levels x 1.2, FAST 20/7; n = 1, 2, 8 frames per call; page-locked buffers.  The two calls
alternate call by call, so that what else the machine does meets both alike.  Per n and call: median, 10th and 90th percentile of the wall time in ms, and the
medians of the upload / kernels / download stages by HIP events (separate calls); the remap kernel alone by the handle's event profiler.
Writes profiles/rectify_rate.json and prints it as one JSON line.
usage: python tools/rectify_rate.py [--calls 400] [--out profiles/rectify_rate.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import corbload  # noqa: E402

SETTINGS = os.path.join(ROOT, "tests", "golden", "EuRoC.yaml")
WARMUP = 30


def pct(ts):
    ts = np.sort(np.asarray(ts)) * 1e3
    return dict(median_ms=round(float(np.median(ts)), 4), p10_ms=round(float(ts[int(0.1 * len(ts))]), 4), p90_ms=round(float(ts[int(0.9 * len(ts))]), 4))


def stages(call, buf_in, buf_out, tm):
    st = []
    for _ in range(100):
        call(buf_in, buf_out, tm); st.append((tm.ms_upload, tm.ms_kernels, tm.ms_download))
    st = np.median(np.array(st), axis=0)
    return dict(upload=round(float(st[0]), 4), kernels=round(float(st[1]), 4), download=round(float(st[2]), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=400)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rectify_rate.json"))
    a = ap.parse_args()
    corb = corbload.load_pkg()
    from corb_slam_amd import synth
    if corb.device_count() < 1:
        raise SystemExit("no MI355X visible")
    s = corb.StereoRectifier.read_settings(SETTINGS)
    W, H, NMAX = int(s["LEFT.width"]), int(s["LEFT.height"]), 8
    sf = corb.StereoFrontend(nfeatures=int(s["ORBextractor.nFeatures"]), scaleFactor=s["ORBextractor.scaleFactor"], nlevels=int(s["ORBextractor.nLevels"]),
                             iniThFAST=int(s["ORBextractor.iniThFAST"]), minThFAST=int(s["ORBextractor.minThFAST"]), width=W, height=H, max_frames=NMAX,
                             fx=s["Camera.fx"], bf=s["Camera.bf"])
    rect = corb.StereoRectifier.from_settings(sf, SETTINGS)
    raw = corb.pinned_empty((NMAX, 2, H, W), np.uint8)
    for f in range(NMAX):
        raw[f] = np.stack(synth.stereo_pair(3000 + f, W, H))
    # the same frames rectified beforehand (by the device: the planes the remap writes), as a client with a host rectifier would hand them over
    rect.upload_batch(0, raw)
    pre = corb.pinned_empty((NMAX, 2, H, W), np.uint8)
    for f in range(NMAX):
        for e in range(2):
            pre[f, e] = sf.orb.pyramid_level(2 * f + e, 0)
    lay = sf.frame_layout()
    res = corb.pinned_empty((NMAX * lay.frame_bytes,), np.uint8)
    tm = corb.StereoFrameTiming()
    out = dict(config=dict(settings="tests/golden/EuRoC.yaml", width=W, height=H, nfeatures=int(s["ORBextractor.nFeatures"]), calls=a.calls, warmup=WARMUP,
                           clock="time.perf_counter around a call that ends in its one synchronisation; page-locked buffers; the two calls alternate"), per_n={})
    for n in (1, 2, 8):
        r_in, p_in, r_out = raw[:n], pre[:n], res[: n * lay.frame_bytes]
        for _ in range(WARMUP):
            rect.frames(r_in, r_out); sf.frames(p_in, r_out)
        t_rect, t_pre = [], []
        for i in range(a.calls):
            r_in.reshape(-1)[0] = i & 255; p_in.reshape(-1)[0] = i & 255               # (a client rewrites the buffer between calls)
            t0 = time.perf_counter(); rect.frames(r_in, r_out); t1 = time.perf_counter(); sf.frames(p_in, r_out); t2 = time.perf_counter()
            t_rect.append(t1 - t0); t_pre.append(t2 - t1)
        o = sf.unpack_frame(r_out, 0)
        e = dict(rect_frames=pct(t_rect), stereo_frames_prerectified=pct(t_pre), n_left=int(len(o["kl"])), n_matched=int(o["n_matched"]))
        e["rect_frames"]["stages_ms"] = stages(rect.frames, r_in, r_out, tm)
        e["stereo_frames_prerectified"]["stages_ms"] = stages(sf.frames, p_in, r_out, tm)
        e["added_ms_median"] = round(e["rect_frames"]["median_ms"] - e["stereo_frames_prerectified"]["median_ms"], 4)
        e["added_ms_per_frame"] = round(e["added_ms_median"] / n, 4)
        e["bytes_in"] = int(r_in.nbytes)
        out["per_n"][str(n)] = e
    # the first kernel of each chain alone (events around the kernel itself, every kernel of the chain timed alone)
    sf.orb.profile(2)
    for n in (1, 8):
        for _ in range(20):
            rect.frames(raw[:n], res[: n * lay.frame_bytes])
        out["per_n"][str(n)]["kernels_alone_us"] = dict((k, round(v[0] / v[1] * 1e3, 2)) for k, v in sf.orb.profile_read().items() if v[1])
    sf.orb.profile(False)
    rect.close(); sf.close()
    line = json.dumps(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
