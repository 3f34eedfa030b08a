"""What the three RANSAC routes share (Sim3Solver.cc:114-138 / :163-177, PnPsolver.cc:166-197 / :233-246, Initializer.cc:82-97), stated once in plain Python: the draw
rule of DUtils::Random::RandomInt over the shrinking vAvailableIndices, its literal list-with-pop emulation, the iteration cap of SetRansacParameters, and the scatter
of 64-bit inlier mask words into byte flags.  sim3solver_reference, pnpsolver_reference and initializer_reference import their draw functions from here; csrc/ransac_common.h
is the same text for the device and the host (tests/test_ransac_common_host.py holds the two equal)."""
import math
import numpy as np

f32, f64 = np.float32, np.float64
RAND_RANGE = 2 ** 31                          # RAND_MAX + 1


def draw_set(r, set_size, N):
    """set_size picks without replacement from 0 .. N-1: randi = int(rand() / (RAND_MAX + 1.0) * size), the pick replaced by the vector's back.  The vector is
    0 .. N-1 apart from the positions written so far, kept as (position, value) pairs"""
    pos, val, out = [], [], []
    for k in range(set_size):
        size = N - k
        randi = int(f64(int(r[k])) / f64(RAND_RANGE) * f64(size))
        v, back = randi, size - 1
        for j in range(k):
            if pos[j] == randi:
                v = val[j]
            if pos[j] == size - 1:
                back = val[j]
        out.append(v); pos.append(randi); val.append(back)
    return out


def draw_set_literal(r, set_size, N):
    avail = list(range(N)); out = []
    for k in range(set_size):
        randi = int((float(int(r[k])) / (float(RAND_RANGE - 1) + 1.0)) * len(avail))
        out.append(avail[randi])
        avail[randi] = avail[-1]; avail.pop()
    return out


def iteration_cap(N, n_min_inliers, epsilon, probability, max_iterations):
    """mRansacMaxIts from the adjusted nMinInliers and the float epsilon; 0 = iterate() sets bNoMore at once"""
    if N < n_min_inliers:
        return 0
    if n_min_inliers == N:
        nit = 1
    else:
        x = math.ceil(math.log(1 - probability) / math.log(1 - math.pow(float(f32(epsilon)), 3.0)))
        nit = max_iterations if not x < max_iterations else (1 if x < 1 else int(x))
    return max(1, min(nit, max_iterations))


def scatter_flags(mask_words, N, index, stride):
    """the byte flags of one event: bit k of the mask sets flag index[k] (k itself without an index), inside [0, stride) only"""
    fl = np.zeros(stride, np.uint8)
    for k in range(N):
        if (int(mask_words[k >> 6]) >> (k & 63)) & 1:
            f = k if index is None else int(index[k])
            if 0 <= f < stride:
                fl[f] = 1
    return fl
