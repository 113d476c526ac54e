"""Shared by tests/test_t2s_logprobs.py (CPU) and tests/test_t2s_logprobs_gpu.py: the rows the stand-alone log-prob entry
(cvx_t2s_logprob_f32) is checked on, their fp64 log_softmax, an fp32 restatement of the epilogue and the error bound.

Bound: |lp - lp64| <= LOGP_TOL_ULPS * 2^-24 * (1 + |lp64|) with LOGP_TOL_ULPS = 256.  It does not come from the kernel: an fp32
restatement of the epilogue on the CPU - exp and log in fp32, the sum taken sequentially, pairwise and in the kernel's own order - reaches
17.2 of these units on the full row set of `rows_for` over every V of VOCABS (sequential sum, V = 1024; pairwise 1.8, kernel order 4.0),
below the 26 units measured earlier on a subset of these rows; the bound is ten times those 26 units - the margin
oracle/t2s_oracle.py LONG_LOGIT_TOL takes - and is not widened, because the full set's figure is not larger.
tests/test_t2s_logprobs.py asserts that the restatement stays within a tenth of the bound."""
import torch

VOCABS = (1, 3, 5, 502, 1023, 1024)
LOGP_TOL_ULPS = 256.0
EPS = 2.0 ** -24
ROWS_PER_KIND = 3


def rows_for(V: int, seed: int = 0):
    """(logits fp32 [rows, V], tokens int64 [rows]) for one vocabulary size: randn * s + o for s in {1, 8, 40} and o in {0, +-1e4} with
    a random token, the token at the row maximum and at the row minimum; all-equal rows; one entry 80 above the rest with the token
    there and elsewhere."""
    gen = torch.Generator().manual_seed(1000 * V + seed)
    rows, toks = [], []

    def add(r, t):
        rows.append(r.to(torch.float32))
        toks.append(int(t))
    for s in (1.0, 8.0, 40.0):
        for o in (0.0, 1.0e4, -1.0e4):
            for _ in range(ROWS_PER_KIND):
                r = (torch.randn(V, generator=gen) * s + o).to(torch.float32)
                add(r, torch.randint(0, V, (1,), generator=gen))
                add(r, r.argmax())
                add(r, r.argmin())
    for c in (0.0, 3.5, -1.0e4):
        add(torch.full((V,), c), torch.randint(0, V, (1,), generator=gen))
    for _ in range(ROWS_PER_KIND):
        r = torch.randn(V, generator=gen)
        hot = int(torch.randint(0, V, (1,), generator=gen))
        r[hot] += 80.0
        add(r, hot)
        add(r, (hot + 1) % V)
    return torch.stack(rows), torch.tensor(toks, dtype=torch.int64)


def reference(logits, tokens):
    """fp64 log_softmax gathered at the tokens"""
    return torch.log_softmax(logits.double(), dim=-1).gather(-1, tokens[:, None])[:, 0]


def bound(lp64):
    return LOGP_TOL_ULPS * EPS * (1.0 + lp64.abs())


def _sum_sequential(ex):
    acc = torch.zeros(ex.shape[0], dtype=torch.float32)
    for j in range(ex.shape[1]):
        acc = acc + ex[:, j]
    return acc


def _sum_pairwise(ex):
    n = 1
    while n < ex.shape[1]:
        n *= 2
    v = torch.zeros(ex.shape[0], n, dtype=torch.float32)
    v[:, :ex.shape[1]] = ex
    while v.shape[1] > 1:
        v = v[:, 0::2] + v[:, 1::2]
    return v[:, 0]


def _sum_kernel_order(ex):
    """the epilogue's order: lane t adds the entries t, t + 64, ..., t + 960 in ascending order (0 past V), then the xor butterfly
    32, 16, ..., 1 over the 64 lanes"""
    v = torch.zeros(ex.shape[0], 1024, dtype=torch.float32)
    v[:, :ex.shape[1]] = ex
    v = v.reshape(-1, 16, 64)
    acc = torch.zeros(ex.shape[0], 64, dtype=torch.float32)
    for i in range(16):
        acc = acc + v[:, i, :]
    lanes = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ o]
    return acc[:, 0]


SUMS = {"sequential": _sum_sequential, "pairwise": _sum_pairwise, "kernel order": _sum_kernel_order}


def restated(logits, tokens, order: str = "kernel order"):
    """the epilogue in fp32 on the CPU: lp = (l[tok] - m) - log(sum_j exp(l[j] - m)), every operation rounded to fp32"""
    l = logits.to(torch.float32)
    m = l.max(dim=-1, keepdim=True).values
    ex = torch.exp(l - m)
    return (l.gather(-1, tokens[:, None])[:, 0] - m[:, 0]) - torch.log(SUMS[order](ex))


def ulps(lp, lp64):
    """the error in units of 2^-24 * (1 + |lp64|)"""
    return (lp.double() - lp64).abs() / (EPS * (1.0 + lp64.abs()))
