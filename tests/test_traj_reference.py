"""CPU tests of tests/traj_reference.py, the definition behind include/corb_trajectory.h: the quaternion's four branches against a float64 closed form, the inverse
and product identities, the spanning-tree walk on chains of depth 0, 1 and 2, on a broken chain and on a cycle of two bad keyframes (which must terminate and be
counted), and the text of each kind of row against literal strings."""
import numpy as np
import pytest
import traj_reference as R

RNG = np.random.default_rng(2024)


def _rand_pose(rng=RNG, scale=2.0):
    a = rng.normal(0, 1, 3)
    return R.pose(R.rot(a, rng.uniform(0.1, 3.0)), rng.normal(0, scale, 3))


@pytest.mark.parametrize("case", range(5))
def test_quaternion_branches_equal_the_closed_form(case):
    axis, angle = R.branch_rotations()[case]
    M = R.rot(axis, angle).astype(np.float32)
    t = float(M[0, 0]) + float(M[1, 1]) + float(M[2, 2])
    # the branch the case is meant for: trace > 0 for the identity and the last case, else the largest diagonal element
    if case in (0, 4):
        assert t > 0 and (case == 0 or t < 1e-3)
    else:
        assert t <= 0 and int(np.argmax(np.diag(M))) == case - 1
    q = R.quaternion(M).astype(np.float64); want = R.quaternion_closed_form(axis, angle)
    assert q.dtype == np.float64 and R.quaternion(M).dtype == np.float32
    assert np.abs(q - want).max() < 1e-6 or np.abs(q + want).max() < 1e-6
    assert abs(np.linalg.norm(q) - 1) < 1e-6                      # (not normalised by the rule: a rotation's quaternion is unit anyway)


def test_inverse_and_product_identities():
    for _ in range(8):
        A, B = _rand_pose(), _rand_pose()
        inv = R.pose_inverse(A)
        assert inv[3].tolist() == [0, 0, 0, 1] and inv[:3, :3].tobytes() == np.ascontiguousarray(A[:3, :3].T).tobytes()
        assert np.abs(R.gemm4(A, inv) - np.eye(4)).max() < 1e-5 and np.abs(R.gemm4(inv, A) - np.eye(4)).max() < 1e-5
        assert np.abs(R.gemm4(A, B).astype(np.float64) - A.astype(np.float64) @ B.astype(np.float64)).max() < 1e-5
        # the product with the identity keeps every value (a negative zero becomes +0: 0 + -0 in the double sum)
        assert np.array_equal(R.gemm4(np.eye(4, dtype=np.float32), A), A)
        # twc = -Rwc*tcw of the KITTI row is the camera centre, and the row's rotation is the transpose
        row = R.row_kitti(A, np.eye(4, dtype=np.float32)).reshape(3, 4)
        assert row[:, 3].tobytes() == R.camera_centre(A).tobytes() and np.array_equal(row[:, :3], A[:3, :3].T)
        neg = -(A[:3, :3].T.astype(np.float64) @ A[:3, 3].astype(np.float64))
        assert np.abs(row[:, 3] - neg).max() < 1e-5


def _chain_store(depth, parent_of_last=R.NO_ID, hold_root=True):
    """keyframes 1 <- 2 <- 3 in slots 2, 0, 1; the reference keyframe is id depth + 1 and everything from 2 up to it is bad"""
    ids = [2, 3, 1]
    store = []
    for s, k in enumerate(ids):
        store.append(dict(id=k, n=4, flags=R.KF_BAD if 2 <= k <= depth + 1 else 0, Tcw=_rand_pose(), parent=(k - 1) if k > 1 else parent_of_last))
    if not hold_root:
        store[2] = None
    Tcp = np.stack([_rand_pose() for _ in ids])
    return store, Tcp


@pytest.mark.parametrize("depth", [0, 1, 2])
def test_walk_on_chains_of_depth_0_1_2(depth):
    store, Tcp = _chain_store(depth)
    flags, ps, Tcw = R.arrays(store)
    assert ps.tolist() == [2, 0, -1]
    Two = R.pose_inverse(Tcw[2])
    ref = R.slot_of(store, depth + 1)
    steps, Trw = R.walk(ref, flags, ps, Tcp, Tcw, 3, Two)
    assert steps == depth
    # spelled out in the reference's association order
    want = np.eye(4, dtype=np.float32); s = ref
    for _ in range(depth):
        want = R.gemm4(want, Tcp[s]); s = ps[s]
    want = R.gemm4(R.gemm4(want, Tcw[s]), Two)
    assert s == 2 and Trw.tobytes() == want.tobytes()
    if depth == 0:                                                  # the origin itself: Trw is Tcw * Twc, the identity up to rounding
        assert np.abs(Trw - np.eye(4)).max() < 1e-5
    entries = []
    R.append(entries, store, ref, _rand_pose(), 1.25, False)
    rows, times, idx, st = R.frames(entries, store, Tcp, -1, R.KITTI)
    assert R.origin_slot(store) == 2 and st == dict(n_entries=1, n_rows=1, n_lost_skipped=0, n_ref_gone=0, n_chain_broken=0, max_chain=depth)
    assert rows[0].tobytes() == R.row_kitti(entries[0]["Tcr"], want).tobytes() and times.tolist() == [1.25] and idx.tolist() == [0]


def test_walk_on_a_broken_chain_gives_no_row_and_is_counted():
    for hold_root in (True, False):
        store, Tcp = _chain_store(2, hold_root=hold_root)
        if hold_root:
            store[0]["parent"] = R.NO_ID                            # keyframe 2 is bad and has no parent
        else:
            store.append(dict(id=9, n=4, flags=0, Tcw=_rand_pose(), parent=R.NO_ID)); Tcp = np.concatenate([Tcp, Tcp[:1]])     # something to be the origin
        flags, ps, Tcw = R.arrays(store)
        assert R.walk(1, flags, ps, Tcp, Tcw, len(store), np.eye(4, dtype=np.float32))[0] == R.CHAIN_BROKEN
        entries = []
        good = len(store) - 1 if not hold_root else 2
        R.append(entries, store, 1, _rand_pose(), 0.0, False); R.append(entries, store, good, _rand_pose(), 1.0, False)
        rows, times, idx, st = R.frames(entries, store, Tcp, -1, R.TUM)
        assert (st["n_rows"], st["n_chain_broken"], st["n_ref_gone"]) == (1, 1, 0) and idx.tolist() == [1] and len(rows) == 1


def test_a_cycle_of_two_bad_keyframes_terminates_and_is_counted():
    store, Tcp = _chain_store(2)
    store[0]["parent"] = 3                                          # 2 -> 3 -> 2 -> ...: both bad
    flags, ps, Tcw = R.arrays(store)
    assert ps.tolist() == [1, 0, -1]
    assert R.walk(1, flags, ps, Tcp, Tcw, 3, np.eye(4, dtype=np.float32)) == (R.CHAIN_BROKEN, None)
    entries = []
    R.append(entries, store, 1, _rand_pose(), 0.0, False); R.append(entries, store, 0, _rand_pose(), 0.5, True); R.append(entries, store, 2, _rand_pose(), 1.0, False)
    rows, times, idx, st = R.frames(entries, store, Tcp, 2, R.KITTI)
    assert (st["n_rows"], st["n_chain_broken"], st["max_chain"]) == (1, 2, 0) and idx.tolist() == [2]
    rows, times, idx, st = R.frames(entries, store, Tcp, 2, R.TUM)
    assert (st["n_rows"], st["n_chain_broken"], st["n_lost_skipped"]) == (1, 1, 1)


def test_an_overwritten_slot_is_counted_as_gone_and_lost_entries_repeat():
    store, Tcp = _chain_store(0)
    entries = []
    R.append(entries, store, 0, _rand_pose(), 3.0, False); R.append_copy(entries, True)
    assert entries[1]["lost"] == 1 and entries[1]["Tcr"].tobytes() == entries[0]["Tcr"].tobytes() and entries[1]["timestamp"] == 3.0
    store[0] = dict(store[0], id=77)
    rows, _, _, st = R.frames(entries, store, Tcp, -1, R.KITTI)
    assert len(rows) == 0 and st["n_ref_gone"] == 2
    assert R.bad_pose(store, 2) is None and R.bad_pose(store, 1) is None       # no parent; a parent (id 2) the store no longer holds


def test_the_text_of_each_kind_against_literal_strings():
    # -0.0 prints its sign, and so does a negative value that rounds to zero; 0.1234567895f is 0.12345679104328...; 1.0000001f is 1.00000011920928955;
    # 0.00000045f is 4.49999987495e-07 -> "0.000000450" (rounds up in the last printed digit); 0.999999999f is 1; 12345.678f is 12345.677734375
    kitti = np.array([-0.0, 1.0, 0.5, -2.25, 0.1234567895, 1.0000001, 0.00000045, 100.125, -1e-10, 3.0, 0.999999999, 12345.678], np.float32)
    assert R.format_rows(R.KITTI, kitti) == (b"-0.000000000 1.000000000 0.500000000 -2.250000000 0.123456791 1.000000119 0.000000450 100.125000000 "
                                             b"-0.000000000 3.000000000 1.000000000 12345.677734375\n")
    tum = np.array([1.5, -0.0, 2.00000095, 0.0, 0.70710677, -0.70710677, 0.00000045], np.float32)
    assert R.format_rows(R.TUM, tum, [1403636579.7635555]) == b"1403636579.763556 1.500000000 -0.000000000 2.000000954 0.000000000 0.707106769 -0.707106769 0.000000450\n"
    # precision 7: 0.70710677f = 0.707106769... -> 0.7071068 (up), 0.00000045f -> 0.0000004 (4.4999998e-7: down), 2.00000095f = 2.00000095367... -> 2.0000010 (up);
    # the double 0.0000015 lies just above the tie -> 0.000002
    assert R.format_rows(R.KEYFRAME_TUM, tum, [0.0000015]) == b"0.000002 1.5000000 -0.0000000 2.0000010 0.0000000 0.7071068 -0.7071068 0.0000004\n"
    two = R.format_rows(R.TUM, np.stack([tum, tum]), [1.0, 2.0])
    assert two.count(b"\n") == 2 and two.endswith(b"\n") and b" \n" not in two and two.split(b"\n")[1].startswith(b"2.000000 ")
    assert R.format_rows(R.KITTI, np.zeros((0, 12), np.float32)) == b""
