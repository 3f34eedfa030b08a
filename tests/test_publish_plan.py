"""CPU test of the map publish's bookkeeping (include/corb_map_publish.h): corb_map_publish_plan -- the verdict every rank computes from the gathered headers -- and
corb_map_publish_messages, and the posting order of the RCCL branch through corb_comm_test_rccl_exchange with a recording fake, as tests/test_push_plan.py does for
the push.  No GPU, no communicator: pure host arithmetic in libcorb_accel.so."""
import numpy as np
import pytest


def headers(corb, W, root, counts, kfb=1024, mpb=320):
    h = np.zeros(W, corb.PUBLISH_HEADER_DTYPE)
    h["kf_record_bytes"] = kfb; h["mp_record_bytes"] = mpb
    h["counts"][root] = counts
    return h


def test_plan_verdicts(corb):
    W, root = 4, 1
    h = headers(corb, W, root, [2, 3, 4, 5, 3])
    assert corb.map_publish_plan(h, root) == (0, -1)
    bad = h.copy(); bad["status"][3] = -3
    assert corb.map_publish_plan(bad, root) == (-3, 3)                       # a rank's local status is everybody's
    bad["status"][0] = -1
    assert corb.map_publish_plan(bad, root) == (-1, 0)                       # the first rank it is about
    bad = h.copy(); bad["kf_record_bytes"][2] = 2048
    assert corb.map_publish_plan(bad, root) == (-1, 2)                       # a receiver's keyframe records differ in size while A is not empty
    bad["counts"][root] = [0, 3, 4, 5, 3]
    assert corb.map_publish_plan(bad, root) == (0, -1)                       # ... pose packets need no matching record size
    bad = h.copy(); bad["mp_record_bytes"][0] = 0
    assert corb.map_publish_plan(bad, root) == (-1, 0)                       # a receiver without a map-point store while B is not empty
    bad["counts"][root] = [2, 0, 4, 5, 3]
    assert corb.map_publish_plan(bad, root) == (0, -1)
    bad = h.copy(); bad["counts"][root] = [2, -1, 0, 0, 0]
    assert corb.map_publish_plan(bad, root) == (-1, root)                    # a negative count
    bad = h.copy(); bad["counts"][root] = [1 << 21, 0, 0, 0, 0]
    assert corb.map_publish_plan(bad, root) == (-1, root)                    # one message of 2^31 bytes or more
    assert corb.map_publish_plan(headers(corb, 1, 0, [0] * 5), 0) == (0, -1) # a world of one, nothing to say
    assert corb.map_publish_plan(h, 4)[0] == -1                              # no such root
    # the counts of a rank that is not the root are not read
    odd = h.copy(); odd["counts"][0] = [-5, 9, 9, 9, 9]
    assert corb.map_publish_plan(odd, root) == (0, -1)


def test_layout_and_messages(corb):
    off = corb.publish_message_layout([2, 3, 5, 7, 3], 1024, 320)
    assert off.tolist() == [0, 2048, 3008, 3376, 3552, 3552 + 416]          # 5 x 72 = 360 -> 368; 7 x 24 = 168 -> 176; 3 x 136 = 408 -> 416
    assert corb.publish_message_layout([0] * 5, 0, 0).tolist() == [0] * 6
    with pytest.raises(corb.CorbError):
        corb.publish_message_layout([1, 0, 0, 0, 0], 1000, 0)                # a record that is no multiple of 16 bytes
    W, root = 4, 2
    h = headers(corb, W, root, [2, 3, 5, 7, 3])
    total = int(off[5])
    for r in range(W):
        sends, recvs = corb.map_publish_messages(h, r, root)
        if r == root:
            assert [(int(m["peer"]), int(m["bytes"]), int(m["n_records"])) for m in sends] == [(q, total, 20) for q in (0, 1, 3)] and len(recvs) == 0      # rank order, the root skipped
        else:
            assert len(sends) == 0 and [(int(m["peer"]), int(m["bytes"]), int(m["kind"]), int(m["first_record"])) for m in recvs] == [(root, total, 0, 0)]
    z = headers(corb, W, root, [0] * 5)
    for r in range(W):                                                       # an all-empty publish: nothing is exchanged
        sends, recvs = corb.map_publish_messages(z, r, root)
        assert len(sends) == 0 and len(recvs) == 0


def test_rccl_branch_posts_the_publish_in_one_group(corb):
    W, root = 4, 0
    h = headers(corb, W, root, [1, 16, 0, 100, 4], kfb=2048)
    total = int(corb.publish_message_layout([1, 16, 0, 100, 4], 2048, 320)[5])
    sends, recvs = corb.map_publish_messages(h, root, root)
    rc, log = corb.rccl_exchange_with_fake(sends, recvs)
    assert rc == 0 and log == [("group_start",), ("send", 1, total, 0), ("send", 2, total, 0), ("send", 3, total, 0), ("group_end",)]      # ncclInt8: counts are bytes
    sends, recvs = corb.map_publish_messages(h, 3, root)
    rc, log = corb.rccl_exchange_with_fake(sends, recvs)
    assert rc == 0 and log == [("group_start",), ("recv", root, total, 0), ("group_end",)]
    sends, recvs = corb.map_publish_messages(h, root, root)
    rc, log = corb.rccl_exchange_with_fake(sends, recvs, fail_at=1)
    assert rc != 0 and log[0] == ("group_start",) and log[-1] == ("group_end",) and len(log) == 4      # a failing send still closes the group, nothing is posted after it
