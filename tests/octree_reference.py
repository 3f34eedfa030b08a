"""ORBextractor::DistributeOctTree as the array formulation that orb_octree_kernel follows (tools/octree_proto.py: the node table is held in std::list
order and rebuilt per pass), restated here so that it also REPORTS which branches a key set takes.  tests/test_octree_reference.py pins it to the serial
oracle (pyorc.distribute_octree) and to the prototype on every input the GPU tests use and on seeded random key sets, so the kinds counted here are
kinds of the oracle's run.

    sel, kinds = distribute(x, y, resp, minX, maxX, minY, maxY, N)

x, y: float32 integer-valued coordinates relative to the minimum border, in candidate order; resp: float32.  sel: indices of the kept keys in list
order (the order of the final keypoints of the level).  kinds (ints):
  n, nIni         keys, initial nodes
  empty_ini       initial nodes without a key (erased before the first pass)
  ini_clamp       keys whose x / hX lands on nIni and is clamped to the last initial node
  passes_A / _B   passes that expand every node with > 1 key / iterations that expand the largest candidates first
  b_stop_mid      phase-B iterations that reach the quota with candidates left unexpanded
  b_tie_at_stop   ... in which the last expanded and the first unexpanded candidate hold the same number of keys (list position decides)
  b_tie_any       phase-B iterations with equal counts among the expanded candidates
  end_by_stall    the loop ended by size == prev_size (fewer distinct keys than N)
  end_by_quota_A / _B   the loop ended by size >= N after a phase-A pass / a phase-B iteration
  best_tie        final nodes whose largest response is held by two or more keys (the first in candidate order is kept)
  single_key, empty     n == 1, n == 0"""
import numpy as np

KIND_NAMES = ("n", "nIni", "empty_ini", "ini_clamp", "passes_A", "passes_B", "b_stop_mid", "b_tie_at_stop", "b_tie_any", "end_by_stall",
              "end_by_quota_A", "end_by_quota_B", "best_tie", "single_key", "empty")


def distribute(x, y, resp, minX, maxX, minY, maxY, N):
    kinds = dict.fromkeys(KIND_NAMES, 0)
    n = len(x)
    W, H = maxX - minX, maxY - minY
    nIni = max(int(np.floor(np.float32(W) / np.float32(H) + np.float32(0.5))), 1)          # roundf of a positive value
    kinds["n"], kinds["nIni"], kinds["single_key"], kinds["empty"] = n, nIni, int(n == 1), int(n == 0)
    if n == 0:
        return np.zeros(0, np.int64), kinds
    x = np.asarray(x, np.float32); y = np.asarray(y, np.float32); resp = np.asarray(resp, np.float32)
    hX = np.float32(W) / np.float32(nIni)
    x0 = np.array([int(hX * np.float32(i)) for i in range(nIni)], np.int64)
    x1 = np.array([int(hX * np.float32(i + 1)) for i in range(nIni)], np.int64)
    y0 = np.zeros(nIni, np.int64); y1 = np.full(nIni, H, np.int64)
    raw = (x / hX).astype(np.int64)
    kinds["ini_clamp"] = int((raw >= nIni).sum())
    node = np.minimum(raw, nIni - 1)
    cnt = np.bincount(node, minlength=nIni)
    keep = cnt > 0                                                                          # empty initial nodes are erased, the order stays
    kinds["empty_ini"] = int((~keep).sum())
    remap = np.cumsum(keep) - 1
    x0, x1, y0, y1, cnt = x0[keep], x1[keep], y0[keep], y1[keep], cnt[keep]
    node = remap[node]

    phaseB = False
    C_front = 0                      # nodes at the list front that the last pass created: the candidates of a phase-B iteration
    while True:
        prev_size = len(cnt)
        hx, hy = (x1 - x0 + 1) >> 1, (y1 - y0 + 1) >> 1                                     # ceil(extent / 2)
        q = (x >= (x0 + hx)[node]).astype(np.int64) + 2 * (y >= (y0 + hy)[node]).astype(np.int64)       # n1 = 0, n2 = 1, n3 = 2, n4 = 3
        if not phaseB:
            expand = cnt > 1
            kinds["passes_A"] += 1
        else:
            expand = np.zeros(len(cnt), bool); expand[:C_front] = cnt[:C_front] > 1
            kinds["passes_B"] += 1
        ccnt = np.zeros((len(cnt), 4), np.int64)
        m = expand[node]
        np.add.at(ccnt, (node[m], q[m]), 1)
        nc = (ccnt > 0).sum(1)
        if phaseB:
            order = sorted(np.nonzero(expand)[0].tolist(), key=lambda p: (-cnt[p], p))     # count descending, list position ascending
            size, proc = prev_size, []
            for p in order:
                proc.append(p)
                size += nc[p] - 1
                if size >= N:
                    break
            if len(proc) < len(order):
                kinds["b_stop_mid"] += 1
                kinds["b_tie_at_stop"] += int(cnt[proc[-1]] == cnt[order[len(proc)]])
            kinds["b_tie_any"] += int(len(set(cnt[proc].tolist())) < len(proc))
            expand = np.zeros(len(cnt), bool); expand[proc] = True
        else:
            proc = np.nonzero(expand)[0].tolist()
        # the new list: the children in reverse order of creation (each was pushed to the front), then the nodes that were not expanded
        C = int(nc[proc].sum()) if proc else 0
        keepers = np.nonzero(~expand)[0]
        new_n = C + len(keepers)
        nx0 = np.zeros(new_n, np.int64); nx1 = nx0.copy(); ny0 = nx0.copy(); ny1 = nx0.copy(); ncnt = nx0.copy()
        newid_child = np.full((len(cnt), 4), -1, np.int64)
        cx0 = np.stack([x0, x0 + hx, x0, x0 + hx], 1); cx1 = np.stack([x0 + hx, x1, x0 + hx, x1], 1)
        cy0 = np.stack([y0, y0, y0 + hy, y0 + hy], 1); cy1 = np.stack([y0 + hy, y0 + hy, y1, y1], 1)
        pos = 0
        for p in proc:
            for c in range(4):
                if ccnt[p, c] > 0:
                    t = C - 1 - pos
                    newid_child[p, c] = t
                    nx0[t], nx1[t], ny0[t], ny1[t], ncnt[t] = cx0[p, c], cx1[p, c], cy0[p, c], cy1[p, c], ccnt[p, c]
                    pos += 1
        newid_keep = np.full(len(cnt), -1, np.int64)
        newid_keep[keepers] = C + np.arange(len(keepers))
        nx0[C:], nx1[C:], ny0[C:], ny1[C:], ncnt[C:] = x0[keepers], x1[keepers], y0[keepers], y1[keepers], cnt[keepers]
        node = np.where(expand[node], newid_child[node, q], newid_keep[node])
        x0, x1, y0, y1, cnt = nx0, nx1, ny0, ny1, ncnt
        C_front = C
        size = len(cnt)
        if size >= N:
            kinds["end_by_quota_B" if phaseB else "end_by_quota_A"] = 1
            break
        if size == prev_size:
            kinds["end_by_stall"] = 1
            break
        if not phaseB and size + 3 * int((cnt[:C] > 1).sum()) > N:
            phaseB = True
    # per node: the largest response, the first key in candidate order among equals
    o = np.lexsort((np.arange(n), -resp.astype(np.float64), node))
    first = np.ones(n, bool); first[1:] = node[o][1:] != node[o][:-1]
    sel = o[first]
    assert np.array_equal(node[sel], np.arange(len(cnt)))
    top = resp[sel][node]
    kinds["best_tie"] = int((np.bincount(node[resp == top], minlength=len(cnt)) > 1).sum())
    return sel, kinds


def distribute_level(cand, w, h, N):
    """The quadtree of one level from the oracle's candidates (x, y relative to the border 16, as the extractor holds them); returns (sel, kinds)."""
    return distribute(cand["x"], cand["y"], cand["response"], 16, w - 16, 16, h - 16, N)


def add_kinds(total, kinds):
    for k in KIND_NAMES:
        total[k] = total.get(k, 0) + kinds[k]
    return total
