"""RGB-D front-end rates on one GPU (corb_rgbd_*), beside the stereo per-frame call in the same process for comparison.

TUM1 (Examples/RGB-D/TUM1.yaml): 640x480 RGB + uint16 depth, 1000 features, 8 levels x 1.2, FAST 20/7.  Prints one JSON line:
  batched_fps     : frames/s of corb_rgbd_run + corb_rgbd_sync on B resident frames (inputs uploaded once)
  frames_B1       : the n = 1 host-to-host corb_rgbd_frames call (page-locked buffers): median / p90 wall ms, and the medians of its upload / kernels /
                    download stages by HIP events (separate calls)
  stereo_B1       : the same for corb_stereo_frames at n = 1 on BASELINE configs[1] (1241x376 stereo, 2000 features)
  kernels_alone_us: every kernel of the n = 1 RGB-D chain timed alone (the handle's event profiler)
usage: python tools/cam_rate.py [--calls 400] [--batch 64]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import corbload  # noqa: E402

TUM1 = dict(fx=517.306408, fy=516.469215, cx=318.643040, cy=255.313989, k1=0.262383, k2=-0.953104, p1=-0.005358, p2=0.002628, k3=1.163314,
            bf=40.0, depth_map_factor=5000.0)


def one_call(fe_frames, pin_in, pin_out, calls, timing_cls):
    for _ in range(30):
        fe_frames(pin_in, pin_out)
    ts = []
    for i in range(calls):
        pin_in.reshape(-1)[0] = i & 255                       # (a client rewrites the buffer between calls)
        t0 = time.perf_counter(); fe_frames(pin_in, pin_out); ts.append(time.perf_counter() - t0)
    ts = np.sort(np.array(ts)) * 1e3
    tm = timing_cls(); st = []
    for _ in range(100):
        fe_frames(pin_in, pin_out, tm); st.append((tm.ms_upload, tm.ms_kernels, tm.ms_download))
    st = np.median(np.array(st), axis=0)
    med = float(np.median(ts))
    return dict(host_to_host_ms=round(med, 4), p90_ms=round(float(ts[int(0.9 * len(ts))]), 4),
                stages_ms=dict(upload=round(float(st[0]), 4), kernels=round(float(st[1]), 4), download=round(float(st[2]), 4)),
                bytes_in=int(pin_in.nbytes), bytes_out=int(pin_out.nbytes), calls=calls)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=400)
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    corb = corbload.load_pkg()
    from corb_slam_amd import synth
    if corb.device_count() < 1:
        raise SystemExit("no MI355X visible")
    out = {}
    B = a.batch
    fe = corb.RgbdFrontend(max_frames=B, **TUM1)
    fr = [synth.rgbd_frame(2000 + i) for i in range(8)]
    packed = fe.pack_input([fr[i % 8] for i in range(B)])
    pin = corb.pinned_empty(packed.shape, np.uint8); pin[...] = packed
    fe.upload_batch(0, pin); fe.sync()
    for _ in range(10):
        fe.run(B)
    fe.sync()
    reps = 30
    t0 = time.perf_counter()
    for _ in range(reps):
        fe.run(B)
    fe.sync()
    dt = time.perf_counter() - t0
    out["batched_fps"] = round(B * reps / dt, 1)
    out["batch"] = B
    lay = fe.layout
    pin_in = corb.pinned_empty((1, lay.input_bytes), np.uint8); pin_in[...] = packed[:1]
    pin_out = corb.pinned_empty((lay.frame_bytes,), np.uint8)
    out["frames_B1"] = one_call(fe.frames, pin_in, pin_out, a.calls, corb.StereoFrameTiming)
    out["frames_B1"]["n_keys"] = int(len(fe.unpack_frame(pin_out)["keys"]))
    fe.orb.profile(2)
    for _ in range(20):
        fe.frames(pin_in, pin_out)
    out["kernels_alone_us"] = dict((k, round(v[0] / v[1] * 1e3, 2)) for k, v in fe.orb.profile_read().items() if v[1])
    fe.orb.profile(False)
    fe.close()
    sf = corb.StereoFrontend(nfeatures=2000, width=1241, height=376, max_frames=1, fx=718.856, bf=386.1448)
    slay = sf.frame_layout()
    spin_in = corb.pinned_empty((1, 2, 376, 1241), np.uint8); spin_in[0] = np.stack(synth.stereo_pair(1000))
    spin_out = corb.pinned_empty((slay.frame_bytes,), np.uint8)
    out["stereo_B1"] = one_call(sf.frames, spin_in, spin_out, a.calls, corb.StereoFrameTiming)
    sf.close()
    out["config"] = "TUM1 640x480 RGB + u16 depth, 1000 features; stereo: configs[1] 1241x376, 2000 features"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
