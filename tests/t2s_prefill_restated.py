"""Shared by tests/test_t2s_prefill.py (CPU) and tests/test_t2s_prefill_gpu.py: the packed attention of a text2semantic prefill pass
(include/covomix_hip.h, cvx_t2s_prefill_attention_f32) restated in fp32 torch from its plain description, the same through the fp64
math of oracle/t2s_oracle.py::attention, the inputs of the kernel test, and `prefill_rows` restated row by row."""
import torch

import t2s_oracle as orc

SEQ_LENS = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257)      # query rows per sequence of the one packed call
KEY_COUNTS = (1, 2, 14, 32, 33, 65, 130)                           # cross mode: key counts, cycled over the sequences
HEADS = (1, 3)
REL_L2 = 5e-6                    # per (sequence, head): the bound tests/test_kernels_gpu.py::test_attention holds the fp32 attention to
CTX_ROWS = 132                   # rows of a cross-attention record (>= the largest key count)
SCALE = 64 ** -0.5


def description(heads, seed=0):
    """The inputs of the kernel test as a plain description: q [M, I] with rows of norm sqrt(I) (so that the oracle's RMSNorm in front of
    to_q is the identity), self k / v [M, I] (sequence i's keys are its own rows: kbase = cu), cross records kv [n * CTX_ROWS, 2 I] of
    which sequence i reads the first nk[i] rows of record i - the rows behind are NaN."""
    g = torch.Generator().manual_seed(1234 + 17 * heads + seed)
    I, n = 64 * heads, len(SEQ_LENS)
    cu = [0]
    for L in SEQ_LENS:
        cu.append(cu[-1] + L)
    M = cu[-1]
    q = torch.randn(M, I, generator=g, dtype=torch.float64)
    q = (q / q.norm(dim=-1, keepdim=True) * I ** 0.5).float()
    k, v = torch.randn(M, I, generator=g), torch.randn(M, I, generator=g)
    nk = [KEY_COUNTS[i % len(KEY_COUNTS)] for i in range(n)]
    kv = torch.randn(n * CTX_ROWS, 2 * I, generator=g)
    for i in range(n):
        kv[i * CTX_ROWS + nk[i]:(i + 1) * CTX_ROWS] = float("nan")
    return dict(heads=heads, cu=cu, q=q, k=k, v=v, kv=kv, nk=nk, kbase_cross=[i * CTX_ROWS for i in range(n)])


def counts(cu, nk, causal):
    """per packed row: (sequence, keys it sees)"""
    out = []
    for i in range(len(cu) - 1):
        for p in range(cu[i + 1] - cu[i]):
            out.append((i, p + 1 if causal else nk[i]))
    return out


def restated(q, k, v, cu, kbase, nk, heads, scale, causal):
    """fp32 torch, straight from the definition: query row r of sequence i, p = r - cu[i], attends to the key rows kbase[i] + j for
    j < (p + 1 if causal else nk[i]); a row past the count is never touched."""
    out = torch.zeros(q.shape[0], heads * 64, dtype=q.dtype)
    for r, (i, c) in enumerate(counts(cu, nk, causal)):
        for h in range(heads):
            cols = slice(64 * h, 64 * h + 64)
            kk, vv = k[kbase[i]:kbase[i] + c, cols], v[kbase[i]:kbase[i] + c, cols]
            out[r, cols] = torch.softmax((kk @ q[r, cols]) * scale, dim=0) @ vv
    return out


def oracle(q, k, v, cu, kbase, nk, heads, causal):
    """The same through oracle/t2s_oracle.py::attention in fp64, sequence by sequence: its RMSNorm is the identity on q's rows (norm
    sqrt(I), gamma 1), to_q, to_kv and to_out are identities, the keys / values come in as the context (the rows up to the largest count
    of the sequence, NaN rows replaced by zeros and masked out - the oracle masks by a large negative number) and `causal` is its own."""
    I = heads * 64
    eye = torch.eye(I, dtype=torch.float64)
    sd = {"a.norm.gamma": torch.ones(I, dtype=torch.float64), "a.to_q.0.weight": eye, "a.to_kv.0.weight": torch.eye(2 * I, dtype=torch.float64),
          "a.to_out.weight": eye}
    outs = []
    for i in range(len(cu) - 1):
        L = cu[i + 1] - cu[i]
        c = L if causal else nk[i]
        ctx = torch.cat((k[kbase[i]:kbase[i] + c], v[kbase[i]:kbase[i] + c]), dim=-1).double()
        assert bool(torch.isfinite(ctx).all())
        o, _ = orc.attention(sd, "a", q[cu[i]:cu[i + 1]].double()[None], heads, context=ctx[None], causal=causal)
        outs.append(o[0])
    return torch.cat(outs)


def rel_l2(got, ref, cu, heads):
    """[n, heads] rel-L2 per (sequence, head)"""
    got, ref = got.double(), ref.double()
    out = torch.zeros(len(cu) - 1, heads, dtype=torch.float64)
    for i in range(len(cu) - 1):
        for h in range(heads):
            a, b = got[cu[i]:cu[i + 1], 64 * h:64 * h + 64], ref[cu[i]:cu[i + 1], 64 * h:64 * h + 64]
            out[i, h] = (a - b).norm() / b.norm().clamp_min(1e-30)
    return out


def rows_restated(seqs, streams, max_length, ctx_rows):
    """`t2s.prefill_rows` restated row by row in plain Python: per packed row (sequence, position, embedding ids, target ids, cache row)."""
    cu, rows, kbase, nk = [0], [], [], []
    for tok, record, ctx, slot in seqs:
        tok = [[int(x) for x in row] for row in tok.tolist()]
        L = len(tok[0])
        for p in range(L):
            rows.append(dict(pos=p, gather=[0 if p == 0 else tok[s][p - 1] for s in range(streams)], start=p == 0,
                             target=[tok[s][p] for s in range(streams)], cache=None if slot is None else slot * max_length + p))
        cu.append(cu[-1] + L)
        kbase.append(record * ctx_rows)
        nk.append(ctx)
    return dict(cu=cu, rows=rows, kbase=kbase, nk=nk)
