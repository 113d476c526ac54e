"""Plain Python / numpy restatement of the edit-distance call and what is built on it: the unit-cost Levenshtein distance, the item and
pair tables of cvx_edit_distance_i64, consensus (minimum-Bayes-risk) selection and the token error rate.  Shared by
test_edit_distance.py (CPU) and test_edit_distance_gpu.py; written from the header's and the docstrings' descriptions, not from the
kernel."""
import math

import numpy as np

MAX_LEN = 4096          # CVX_EDIT_MAX_LEN


def naive(a, b) -> int:
    """The textbook matrix, cell by cell."""
    a, b = list(a), list(b)
    D = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(len(a) + 1):
        for j in range(len(b) + 1):
            if i == 0 or j == 0:
                D[i][j] = i + j
                continue
            best = None
            for cand in (D[i - 1][j] + 1, D[i][j - 1] + 1, D[i - 1][j - 1] + (a[i - 1] != b[j - 1])):
                best = cand if best is None or cand < best else best
            D[i][j] = best
    return D[len(a)][len(b)]


def distance(a, b) -> int:
    """Row by row; the insertion chain D[i][j] = min_k<=j (t[k] + j - k) of a row is one running minimum of t[k] - k."""
    a, b = np.asarray(a, dtype=np.int64).reshape(-1), np.asarray(b, dtype=np.int64).reshape(-1)
    n = b.size
    idx = np.arange(n + 1, dtype=np.int64)
    row = idx.copy()
    for x in a:
        t = np.empty(n + 1, dtype=np.int64)
        t[0] = row[0] + 1
        np.minimum(row[1:] + 1, row[:-1] + (b != x), out=t[1:])
        row = np.minimum.accumulate(t - idx) + idx
    return int(row[n])


def tables(lengths, pairs):
    """(items int32 [n, 2] = (offset, length) of sequences packed back to back, pairs int32 [P, 2])"""
    items, off = [], 0
    for n in lengths:
        items.append((off, int(n)))
        off += int(n)
    return (np.asarray(items, dtype=np.int32).reshape(-1, 2), np.asarray([tuple(p) for p in pairs], dtype=np.int32).reshape(-1, 2))


def distances(sequences, pairs) -> np.ndarray:
    """What ops.edit_distance returns: int32 [P]; a pair met before is not computed again."""
    seen, out = {}, []
    for i, j in pairs:
        key = (min(i, j), max(i, j))
        if key not in seen:
            a, b = sorted((sequences[i], sequences[j]), key=len)          # the row loop over the shorter one (the distance is symmetric)
            seen[key] = 0 if i == j else distance(a, b)
        out.append(seen[key])
    return np.asarray(out, dtype=np.int32)


def counted(stream, eos):
    """the tokens of one stream up to and including its first eos; all of them without one"""
    s = [int(x) for x in stream]
    return s[:s.index(eos) + 1] if eos in s else s


def consensus_risks(candidate_streams, eos, dist=distance):
    """candidate_streams: per candidate its streams [S][L] -> risk[c] = sum over c' != c and s of d(counted(c, s), counted(c', s))"""
    toks = [[counted(s, eos) for s in cand] for cand in candidate_streams]
    N = len(toks)
    risk = [0] * N
    for c in range(N):
        for c2 in range(N):
            if c2 != c:
                risk[c] += sum(dist(x, y) for x, y in zip(toks[c], toks[c2]))
    return risk


def best_candidate(scores) -> int:
    best = 0
    for c in range(1, len(scores)):
        if scores[c] > scores[best] or (math.isnan(scores[best]) and not math.isnan(scores[c])):
            best = c
    return best


def consensus_candidate(risks, scores) -> int:
    """smallest risk; then the larger score (a NaN loses against a number); then the lowest index"""
    low = min(risks)
    tied = [c for c in range(len(risks)) if risks[c] == low]
    return tied[best_candidate([scores[c] for c in tied])]


def token_error_rate(pred, ref, pad=501, dist=distance) -> float:
    pred, ref = [int(x) for x in pred], [int(x) for x in ref]
    L = max(len(pred), len(ref))
    if L == 0:
        return 0.0
    return dist(pred + [pad] * (L - len(pred)), ref + [pad] * (L - len(ref))) / L
