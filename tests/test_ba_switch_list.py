"""Every environment switch the library reads is either run against the default by tests/test_gpu_ba_switches.py or listed here with the reason why not: a switch
added later without a test or a stated reason fails this test on the CPU."""
import glob
import os
import re

import ba_switch_cases as G

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "corb-slam_amd", "csrc")

# name -> why tests/test_gpu_ba_switches.py does not run it
EXCLUDED = {
    "CORB_BA_TIMING": "only prints: host phase times of a BA call on stderr",
    "CORB_BA_TRACE": "only prints: the launch and branch markers that test_gpu_ba_switches.py reads",
    "CORB_BA_HOST_THREADS": "tested elsewhere: tests/test_gpu_ba.py::test_threaded_host_flattening_equals_the_serial_one",
    "CORB_BA_HOST_FLATTEN": "tested elsewhere: tests/test_gpu_ba.py::test_large_host_array_call_takes_the_device_flattening_and_equals_the_host_one",
    "CORB_BA_TWO_LEVEL": "tested elsewhere: tests/test_gpu_ba.py::test_pcg_two_level_partial_reduction",
    "CORB_VOC_TRAIN_SMALL": "tested elsewhere: tests/test_gpu_voc_train.py::test_small_node_switch_gives_the_same_bytes",
    "CORB_BA_PCG_LOOSE": "tuning parameter: the cap of the PCG forcing sequence changes results by design",
    "CORB_BA_ML_W": "tuning parameter: the multilevel preconditioner's level weights change results by design",
    "CORB_BA_ML_STRIDE0": "tuning parameter: the multilevel preconditioner's first stride changes results by design",
    "CORB_BA_ML_STRIDE1": "tuning parameter: the multilevel preconditioner's later strides change results by design",
    "CORB_BA_ROWDBG": "exists only under -DCORB_DEV (corb_dev_env)",
    "CORB_BA_ROWABL": "exists only under -DCORB_DEV (corb_dev_env)",
    "CORB_BA_PC_PERIOD": "exists only under -DCORB_DEV (corb_dev_env)",
    "CORB_BA_SMALL_EDGES": "exists only under -DCORB_DEV (corb_dev_env)",
    "CORB_FRAME_NO_GRAPH": "exists only under -DCORB_DEV (corb_dev_env)",
    "CORB_ORB_SKIP": "exists only under -DCORB_DEV (corb_dev_env)",
    "CORB_PARTS": "read per handle: tests/test_gpu_orb.py::test_parts_switch_gives_the_same_bytes",
}


def names_read(root=CSRC):
    """every string literal passed to getenv( / corb_dev_env( in the library's sources"""
    found = set()
    for path in sorted(glob.glob(os.path.join(root, "*"))):
        if os.path.splitext(path)[1] in (".cpp", ".h", ".hip", ".hpp"):
            found.update(re.findall(r'\b(?:getenv|corb_dev_env)\s*\(\s*"([^"]+)"', open(path, errors="replace").read()))
    return found


def test_every_switch_is_tested_or_excluded_with_a_reason():
    tested = {r["env"] for r in G.SWITCHES}
    read = names_read()
    assert not (tested & set(EXCLUDED)), tested & set(EXCLUDED)
    assert read - tested - set(EXCLUDED) == set(), "switches read by the library without a test or a stated reason: %s" % sorted(read - tested - set(EXCLUDED))
    assert (tested | set(EXCLUDED)) - read == set(), "switches listed here that the library no longer reads: %s" % sorted((tested | set(EXCLUDED)) - read)
    assert all(isinstance(v, str) and len(v.split()) >= 3 and "\n" not in v for v in EXCLUDED.values())


def test_no_name_is_read_through_a_variable():
    """the collection above sees string literals only: no call passes anything else (corb_dev_env's own definition aside)"""
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if os.path.splitext(path)[1] in (".cpp", ".h", ".hip", ".hpp"):
            for m in re.finditer(r'\b(getenv|corb_dev_env)\s*\(\s*([^")][^)]*)\)', open(path, errors="replace").read()):
                assert (m.group(1), m.group(2).strip()) in (("getenv", "name"), ("corb_dev_env", "const char* name"), ("corb_dev_env", "const char*")), (path, m.group(0))


def test_switch_rows_are_well_formed():
    ids = [G.row_id(r) for r in G.SWITCHES]
    assert len(set(ids)) == len(ids)
    for r in G.SWITCHES:
        assert r["reach"] and set(r["reach"] + r["also"] + r["extra"]) <= set(G.CASES) and r["variant"] != r["default"]
