"""Seeded bundle-adjustment calls shared by the development-switch tests (tests/test_gpu_ba_switches.py): the smallest shapes at which the branch behind each CORB_BA_* /
CORB_LBA_* switch is reached.  Most switches are read once per process, so every value gets a fresh child process: run as a program, this module puts the named cases
through the library and writes one .npz per case into the directory given first.

Case            call                                                        branches (ba_lm.cpp, corb_ba_staged.cpp)
row64_plain     global BA, solver 2, 64 free poses, pc_block 16, plain      row_schur (nP >= BA_ROW_MIN_POSES), v_kf, the stream kernel, pc_g > 1, the captured CG chunks
row64_huber     the same call, Huber kernel (ba-011 of test_gpu_random_ba)  the same
dense22         global BA, solver 1, 22 free poses (ba-008)                 lean multi-kernel path, blocked dense Cholesky (6 * 22 > 128), backsub_rederive
window12        local window, 11 free keyframes, LOCAL_BA_STAGES            the in-LDS solve: chain_ok, device-decided chains
staged_dev      local window grouped by point, > 2048 edges                 the device flattening (reserved0 == 1), device-decided chains
staged_host     staged_dev with one point's edges moved to the end          the host flattening, the session of corb_ba_solve_staged (CORB_BA_HOST_STAGES is read only there)
window006       WINDOW_CASES[6] of test_gpu_random_ba: 23 free keyframes    the device flattening, blocked dense Cholesky (6 * 23 > 128: no chains)
window006_host  the same window, one point's edges moved                    the host flattening of the same window"""
import numpy as np

import test_gpu_random_ba as RB

CASES = ["row64_plain", "row64_huber", "dense22", "window12", "staged_dev", "staged_host", "window006", "window006_host"]
STAGED = ("window12", "staged_dev", "staged_host", "window006", "window006_host")
FLOATS = ("poses", "points", "chi2", "lam", "outlier")
INTS = ("iters_done", "trials_total", "solver_used", "pcg_iterations", "pcg_refined_trials", "reserved0")
STRUCTURE = ("free_poses", "free_points", "active_edges", "nnz_blocks", "schur_pairs", "pc_block", "pc_levels")
MARK = "[ba_switch_cases] case "              # what the child writes to stderr in front of every case, so that the library's trace lines can be told apart by case


def _row(env, value, reach, variant, default, also=(), extra=()):
    return dict(env=env, value=value, reach=list(reach), also=list(also), extra=list(extra), variant=variant, default=default)


ROW64 = ["row64_plain", "row64_huber"]
W006 = ["window006", "window006_host"]
# One child process per row, with exactly that variable set.  reach: the cases whose trace must show the variant's marker (and, in the child without a switch, the
# default's); also: cases compared with the default child although the switch's branch is not on their path; extra: cases run for the record only.
SWITCHES = [
    _row("CORB_BA_NO_GRAPH", "1", ROW64, "cg chunk: kernel by kernel (CORB_BA_NO_GRAPH)", "cg chunk: graph replay"),
    _row("CORB_BA_ROW_UNITS", "1", ROW64, "row schur: per-unit kernel (CORB_BA_ROW_UNITS)", "row schur: stream kernel"),
    _row("CORB_BA_V_EDGE", "1", ROW64, "V blocks: edge order (CORB_BA_V_EDGE / CORB_BA_ROW_UNITS)", "V blocks: keyframe-list order"),
    _row("CORB_BA_BACKSUB_V", "1", ROW64 + ["dense22"], "backsub: stored V blocks (CORB_BA_BACKSUB_V)", "backsub: re-derived from the estimates"),
    _row("CORB_BA_PC_SQUARE", "1", ROW64, "pc step: square blocks (CORB_BA_PC_SQUARE)", "pc step: packed upper triangles"),
    _row("CORB_BA_NO_CHAIN", "1", ["window12"], "lm: host-driven loop (CORB_BA_NO_CHAIN)", "lm: device-decided chain of up to 5 iterations", extra=W006),
    _row("CORB_BA_CHAIN", "1", ["window12"], "lm: device-decided chain of up to 1 iterations", "lm: device-decided chain of up to 5 iterations", extra=W006),
    _row("CORB_BA_CHAIN", "3", ["window12"], "lm: device-decided chain of up to 3 iterations", "lm: device-decided chain of up to 5 iterations"),
    _row("CORB_BA_CTL_LAUNCH", "1", ["window12"], "lm ctl: its own launch (CORB_BA_CTL_LAUNCH)", "lm ctl: in the chi2 launch"),
    _row("CORB_LBA_HOST_FLATTEN", "1", ["staged_dev"], "window: host flattening (CORB_LBA_HOST_FLATTEN)", "window: device flattening"),
    # (corb_ba_solve_staged reads CORB_BA_HOST_STAGES behind the device window's return: staged_dev never gets there, the same window on the host flattening does)
    _row("CORB_BA_HOST_STAGES", "1", ["staged_host"], "stages: classified on the host (CORB_BA_HOST_STAGES)", "stages: classified on the device", also=["staged_dev"], extra=W006),
]


def row_id(row):
    return "%s=%s" % (row["env"], row["value"])


def _moved(p):
    q = dict(p); q["edges"] = p["edges"][RB.moved_order(p["edges"])]
    return q


def problem(synth, name):
    """-> (the problem's arrays, keyword arguments of the call); drawn again from the seed at every call"""
    if name in ("row64_plain", "row64_huber"):
        c = RB.BA_CASES[11]
        assert (c["solver"], c["free"]) == (2, 64)
        return RB.ba_case_problem(synth, c), dict(nIterations=10, bRobust=name == "row64_huber", solver=2, pc_block=16)
    if name == "dense22":
        c = RB.BA_CASES[8]
        assert (c["solver"], c["free"]) == (1, 22)
        return RB.ba_case_problem(synth, c), dict(nIterations=10, bRobust=c["robust"], solver=1)
    if name == "window12":
        return synth.local_ba_problem(seed=2012, n_local=12, n_fixed=6, pts_per_kf=40), {}
    if name in ("staged_dev", "staged_host"):              # test_gpu_staged.py: test_local_window_on_the_device_equals_the_host_route_bit_for_bit[2021]
        p = synth.local_ba_problem(seed=2021, n_local=10, n_fixed=8, pts_per_kf=90, outlier_frac=0.12)
        return (p if name == "staged_dev" else _moved(p)), {}
    if name in ("window006", "window006_host"):
        c = RB.WINDOW_CASES[6]
        assert c["n_local"] == 24
        p = RB.window_case_problem(synth, c)
        return (p if name == "window006" else _moved(p)), {}
    raise KeyError(name)


def args(p):
    return RB._args(p)


def run(corb, synth, name):
    """the case through the library -> dict of arrays (FLOATS, INTS and STRUCTURE; what a staged call does not report is empty)"""
    p, kw = problem(synth, name)
    if name in STAGED:
        g = corb.Optimizer.LocalBundleAdjustment(*args(p))
        out = dict(poses=g["poses"], points=g["points"], chi2=np.zeros(0), lam=np.zeros(0), outlier=g["outlier"], iters_done=g["iters_done"], trials_total=g["trials"],
                   solver_used=g["solver"])
    else:
        g = corb.Optimizer.GlobalBundleAdjustemnt(*args(p), **kw)
        out = dict(poses=g["poses"], points=g["points"], chi2=g["chi2"], lam=g["lam"], outlier=np.zeros(0, np.uint8), iters_done=g["iters_done"], trials_total=g["trials"],
                   solver_used=g["solver"], pcg_refined_trials=g["certificate"]["pcg_refined_trials"])
    for k in INTS:
        out.setdefault(k, g.get(k))
    for k in STRUCTURE:
        out[k] = g["structure"][k]
    return {k: np.asarray(v) for k, v in out.items()}


if __name__ == "__main__":
    # ba_switch_cases.py OUT_DIR CASE...: a fresh process per switch value; the results go to OUT_DIR/CASE.npz, the case names to stdout as one JSON line
    import json
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import corbload
    corb = corbload.load_pkg()
    from corb_slam_amd import synth
    out_dir, names = sys.argv[1], sys.argv[2:]
    for name in names:
        sys.stderr.write(MARK + name + "\n"); sys.stderr.flush()
        np.savez(os.path.join(out_dir, name + ".npz"), **run(corb, synth, name))
    print(json.dumps(names))
