"""Plain numpy restatement of the DTW call (cvx_dtw_f32 / ops.dtw) and of the metrics built on it, in fp32 with every operation
individually rounded (numpy rounds every array operation and never contracts), so that the kernel's result can be compared with ==.
Shared by test_dtw.py (CPU) and test_dtw_gpu.py; written from the header's description, not from the kernel.  Also: all warping
paths by brute force for tiny sizes, and the same DP in fp64."""
import math

import numpy as np

MAX_FRAMES = 4096       # CVX_DTW_MAX_FRAMES
MAX_DIM = 80            # CVX_DTW_MAX_DIM
MCD_CONST = 10.0 / math.log(10.0) * math.sqrt(2.0)
_BIG = np.int32(1 << 30)


def frame_distances(x, y, dtype=np.float32) -> np.ndarray:
    """c[i, j] = sqrt(sum_d (x[i, d] - y[j, d])^2), d ascending from +0, every operation rounded to `dtype`"""
    x, y = np.asarray(x, dtype=dtype), np.asarray(y, dtype=dtype)
    acc = np.zeros((x.shape[0], y.shape[0]), dtype=dtype)
    for d in range(x.shape[1]):
        diff = x[:, d, None] - y[None, :, d]
        acc = acc + diff * diff
    return np.sqrt(acc)


def dtw(x, y, dtype=np.float32):
    """(cost, steps) of the last cell: steps (i-1, j-1), (i-1, j), (i, j-1), a lexicographic minimum on (cost, steps) over the
    predecessors, anti-diagonal by anti-diagonal.  Cell (i, j) lives at [i + 1, j + 1]; row 0 and column 0 are +inf but for [0, 0] =
    (0, 0 steps), diagonally above cell (0, 0)."""
    x, y = np.asarray(x, dtype=dtype), np.asarray(y, dtype=dtype)
    Tx, Ty = x.shape[0], y.shape[0]
    if Tx == 0 or Ty == 0:
        return dtype(0), 0
    c = frame_distances(x, y, dtype)
    cost = np.full((Tx + 1, Ty + 1), np.inf, dtype=dtype)
    steps = np.zeros((Tx + 1, Ty + 1), dtype=np.int32)
    cost[0, 0] = 0
    for k in range(Tx + Ty - 1):
        i = np.arange(max(0, k - Ty + 1), min(k, Tx - 1) + 1)
        j = k - i
        cu, cl, cd = cost[i, j + 1], cost[i + 1, j], cost[i, j]
        su, sl, sd = steps[i, j + 1], steps[i + 1, j], steps[i, j]
        best = np.minimum(np.minimum(cu, cl), cd)
        s = np.minimum(np.minimum(np.where(cu == best, su, _BIG), np.where(cl == best, sl, _BIG)), np.where(cd == best, sd, _BIG))
        cost[i + 1, j + 1] = c[i, j] + best
        steps[i + 1, j + 1] = s + 1
    return cost[Tx, Ty], int(steps[Tx, Ty])


def dtw64(x, y) -> float:
    """the cost of the same DP in fp64 on the same (fp32) inputs"""
    return float(dtw(np.asarray(x, dtype=np.float32).astype(np.float64), np.asarray(y, dtype=np.float32).astype(np.float64), np.float64)[0])


def brute(x, y):
    """every warping path from (0, 0) to the last cell, for tiny sizes: (the smallest cost in fp64, the fewest cells among the paths of
    that cost).  Exact for integer-valued 1-D features."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    c = frame_distances(x, y, np.float64)
    Tx, Ty = c.shape
    best = [math.inf, 0]

    def walk(i, j, cost, n):
        cost, n = cost + c[i, j], n + 1
        if i == Tx - 1 and j == Ty - 1:
            if cost < best[0] or (cost == best[0] and n < best[1]):
                best[0], best[1] = cost, n
            return
        if i + 1 < Tx and j + 1 < Ty:
            walk(i + 1, j + 1, cost, n)
        if i + 1 < Tx:
            walk(i + 1, j, cost, n)
        if j + 1 < Ty:
            walk(i, j + 1, cost, n)
    walk(0, 0, 0.0, 0)
    return best[0], best[1]


def tables(lengths, pairs):
    """(items int32 [n, 2] = (first row, frames) of sequences packed back to back, pairs int32 [P, 2])"""
    items, row = [], 0
    for n in lengths:
        items.append((row, int(n)))
        row += int(n)
    return (np.asarray(items, dtype=np.int32).reshape(-1, 2), np.asarray([tuple(p) for p in pairs], dtype=np.int32).reshape(-1, 2))


def dtw_many(features, pairs, memo=None):
    """What ops.dtw returns: (cost float32 [P], steps int32 [P]); a pair met before (in either order: the rule is symmetric, which
    test_dtw.py checks on the restatement itself) is not computed again.  `memo` keeps results between calls on the same features."""
    seen = {} if memo is None else memo
    cost, steps = [], []
    for i, j in pairs:
        key = (min(i, j), max(i, j))
        if key not in seen:
            seen[key] = dtw(features[key[0]], features[key[1]])
        cost.append(seen[key][0])
        steps.append(seen[key][1])
    return np.asarray(cost, dtype=np.float32), np.asarray(steps, dtype=np.int32)


def dct_matrix(n_mels=80, n_coef=13) -> np.ndarray:
    """rows k = 1 ... n_coef of the orthonormal DCT-II, fp64"""
    k = np.arange(1, n_coef + 1, dtype=np.float64)[:, None]
    m = np.arange(n_mels, dtype=np.float64)[None, :]
    return math.sqrt(2.0 / n_mels) * np.cos(math.pi * k * (2 * m + 1) / (2 * n_mels))


def mcd(cost, steps) -> float:
    """mel-cepstral distortion in dB of a path; NaN without a path"""
    return MCD_CONST * float(cost) / steps if steps > 0 else math.nan
