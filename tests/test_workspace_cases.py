"""CPU checks of tests/workspace_cases.py, the registry behind tests/test_gpu_workspace_states.py: it is the same on every import, it accounts for every symbol the
header declares -- each is either on a workspace lane and covered by an entry, or named in NOT_ON_A_LANE, so a new entry point forces a decision -- and each
bundle-adjustment case it picked reaches the route it is registered for."""
import importlib
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import workspace_cases as W  # noqa: E402
import test_gpu_random_ba as RB  # noqa: E402
from test_cabi import _declared  # noqa: E402
from test_random_cases import _expected_route, _fingerprint  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _shape(mod):
    return [(e.name, e.lane, e.symbols, e.bigger is not None, e.fill) for e in mod.ENTRIES]


def test_registry_is_deterministic_on_reimport():
    global W
    before = _shape(W); picks = _fingerprint([W.BA_ROUTE_CASES, W.BA_DEVFLAT_CASE, W.WINDOW_HOST_CASE, W.WINDOW_DEVICE_CASE, W.TRACK_POSE_CASE, W.SIM3_SINGLE, W.GRAPH_CASE])
    lanes = (W.LANE_SYMBOLS, W.NOT_ON_A_LANE)
    W = importlib.reload(W)
    assert _shape(W) == before and (W.LANE_SYMBOLS, W.NOT_ON_A_LANE) == lanes
    assert _fingerprint([W.BA_ROUTE_CASES, W.BA_DEVFLAT_CASE, W.WINDOW_HOST_CASE, W.WINDOW_DEVICE_CASE, W.TRACK_POSE_CASE, W.SIM3_SINGLE, W.GRAPH_CASE]) == picks
    assert len({e.name for e in W.ENTRIES}) == len(W.ENTRIES) and all(re.fullmatch(r"[a-z0-9_]+", e.name) for e in W.ENTRIES)


def test_every_declared_symbol_is_on_a_lane_and_covered_or_named_as_off_the_lanes():
    declared = set(_declared())
    on_lane = W.LANE_SYMBOLS[0] | W.LANE_SYMBOLS[1]
    assert not (W.LANE_SYMBOLS[0] & W.LANE_SYMBOLS[1]) and not (on_lane & W.NOT_ON_A_LANE)
    covered = {s for e in W.ENTRIES for s in e.symbols}
    assert covered == on_lane, (sorted(on_lane - covered), sorted(covered - on_lane))
    assert covered | W.NOT_ON_A_LANE == declared, (sorted(declared - covered - W.NOT_ON_A_LANE), sorted((covered | W.NOT_ON_A_LANE) - declared))
    # an entry sits in the lane its first symbol takes (the single-pose route of corb_ba_solve_staged, which runs in lane 0's pose batch, is the one exception)
    for e in W.ENTRIES:
        assert e.lane in (0, 1) and (W.LANE_OF[e.symbols[0]] == e.lane or e.name == "pose_optimization_fused"), e.name
    # lane 0's entries come first in the GPU file
    import test_gpu_workspace_states as T
    order = [e.lane for e in T.ENTRIES]
    assert order == sorted(order) and {e.name for e in T.ENTRIES} == {e.name for e in W.ENTRIES} and T.PARTIAL_OUTPUTS == {}


def test_lane_symbols_are_the_entry_points_whose_source_takes_a_lane():
    """the C sources say which exported functions open a lane: a CorbScratch / Pool / GPool / CovisCall in the function, or in a file-local helper it calls.  Every
    function that does so directly must be in LANE_SYMBOLS, with the lane the source names"""
    csrc = os.path.join(ROOT, "corb-slam_amd", "csrc")
    direct = {}
    for f in sorted(os.listdir(csrc)):
        if not f.endswith(".cpp"):
            continue
        src = open(os.path.join(csrc, f)).read()
        heads = [(m.start(), m.group(1)) for m in re.finditer(r'^extern "C" [^\n(]*?\b(corb_[a-z0-9_]+)\s*\(', src, re.M)]
        for k, (at, name) in enumerate(heads):
            body = src[at: heads[k + 1][0] if k + 1 < len(heads) else len(src)]
            body = body[: body.find("\n}\n") + 3] if "\n}\n" in body else body
            if re.search(r"\b(GPool|Pool) pool;", body):
                direct[name] = 1
            elif re.search(r"CorbScratch \w+\(0\)|CorbScratch \w+;|DevPool pool;|CovisCall c;", body):
                direct[name] = 0
    direct.pop("corb_warmup", None)                              # (creates both lanes, draws nothing)
    assert len(direct) >= 30
    for name, lane in direct.items():
        assert W.LANE_OF.get(name) == lane, (name, lane, W.LANE_OF.get(name))


def test_registered_ba_cases_reach_the_routes_they_name(synth):
    assert set(W.BA_ROUTE_CASES) == {RB.FUSED, RB.LDS, RB.DENSE, RB.PCG, RB.PCG_ROW, RB.PCG_ML}
    for route, c in list(W.BA_ROUTE_CASES.items()) + [(W.BA_DEVFLAT_CASE["route"], W.BA_DEVFLAT_CASE)]:
        assert c["i"] not in RB.BA_OPEN and c["route"] == route
        p = RB.ba_case_problem(synth, c)
        free = int((p["pose_fixed"] == 0).sum()); nE = RB.active_edges(p)
        e = p["edges"]; act = ~((p["pose_fixed"][e["pose"]] != 0) & (p["point_fixed"][e["point"]] != 0))
        nL = len(np.unique(e["point"][act & (p["point_fixed"][e["point"]] == 0)]))
        assert _expected_route(c, free, nE, nL) == route, RB.ba_case_id(c)
        # the smallest of its route
        assert all(c["free"] * c["ppk"] <= o["free"] * o["ppk"] for o in RB.BA_CASES if o["route"] == route and o["devflat"] == c["devflat"] and o["i"] not in RB.BA_OPEN)
    assert W.BA_DEVFLAT_CASE["devflat"]
    assert not RB.window_expects_device(RB.window_case_problem(synth, W.WINDOW_HOST_CASE)) and RB.window_expects_device(RB.window_case_problem(synth, W.WINDOW_DEVICE_CASE))
    pose = {e.name: e for e in W.ENTRIES}
    assert pose["pose_optimization_fused"].lane == 0 and pose["pose_optimization_general_path"].lane == 1
    assert W.TRACK_POSE_CASE["edges"] >= 10 and W.SIM3_SINGLE["n"] == 63 and W.GRAPH_CASE["nP"] == 9
