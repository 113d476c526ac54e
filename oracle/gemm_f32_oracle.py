"""fp64 reference of the fp32 GEMM's contract (include/covomix_hip.h: cvx_gemm_bias_act_f32), a per-element error bound computed from
the reference side alone, and the table of launches the fp32 GEMM tests share.

TEST INFRASTRUCTURE ONLY: nothing under neurips2024-covomix_amd/ imports this file; only tests/ may, as the checker.

  CASES                    the launches, each with the kernel form it is meant to take (tests/test_gemm_f32_forms.py takes the forms
                           from the library, cvx_gemm_f32_form, so a retuned rule fails there instead of dropping a kernel from coverage)
  problem(case)            the operands of a case on the CPU (cached; never modified afterwards): allocations and the views the call takes
  reference(case)          C = epilogue([A | A2] W^T) in fp64:  bias -> act -> half-split RoPE on [0, rope_cols) -> + residual
  evaluate_f32(case)       the same in plain fp32 torch (torch.matmul + an fp32 epilogue): what a correct fp32 kernel looks like
  bound(case)              per-element bound on |C - reference| of ANY correct fp32 evaluation (derivation below)
  mutant(case, name)       deliberately wrong variants of the reference: how tests/test_gemm_f32_forms.py proves the bound can fail

The bound.  u = 2^-23 (one ulp of fp32 relative to the value: twice the unit roundoff, so that the bound does not depend on how the
matrix pipe rounds internally).  A K-term fp32 dot product in ANY summation order, fused or not, has the forward error
    |fl(a . w) - a . w| <= gamma_K (|a| . |w|),   gamma_K = K u' / (1 - K u')  <  (K + 2) u   for u' <= u, K u < 0.1,
so  e0 = (K + 2) u (|A| |W|^T)  bounds the accumulators.  The epilogue carries it on:
    bias add            e <- e + u |v|                                      (v = the value after the step, here and below)
    activation          e <- L e + u |v|,  L = 1.13 (GELU: max |gelu'| = 1.129) or 1.1 (SiLU: max |silu'| = 1.0998)
    RoPE (lo, hi)       e_lo, e_hi <- e_lo + e_hi + 2 u (|lo| + |hi|)       (|cos|, |sin| <= 1; two products, rounded, of lo and hi)
    residual add        e <- e + u |v|
    store               e <- e + u |v|
Derived, not measured: nothing here looks at what a kernel returns.
"""
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

U = 2.0 ** -23
TOL = 2e-6                                   # rel-L2 of the whole output against fp64: TOL of tests/test_kernels_gpu.py
ACT_NONE, ACT_GELU, ACT_SILU, ACT_TANH = 0, 1, 2, 3
LIPSCHITZ = {ACT_NONE: 1.0, ACT_GELU: 1.13, ACT_SILU: 1.1}
FORMS = ("T64", "T64_GENERIC", "T128_DMA", "T128_GENERIC")
MUTANTS = ("drop_k", "last_row_from_prev", "last_col_from_prev", "swap_a_a2", "rope_pos_off_by_one", "residual_twice")


@dataclass(frozen=True)
class Case:
    name: str
    M: int
    N: int
    K: int
    form: str
    reason: str
    lda: int = 0                 # row strides in floats; 0 = the width of the view (dense)
    lda2: int = 0
    ldw: int = 0
    ldc: int = 0
    ldr: int = 0
    K1: int = 0                  # > 0: columns [0, K1) come from A, [K1, K) from A2
    bias: bool = False
    act: int = ACT_NONE
    residual: bool = False
    alias: bool = False          # the residual IS the output buffer (in place)
    rope: Optional[str] = None   # "shared": cos / sin [rope_T][32], position = row % rope_T; "per_row": rope_T = M, one table row per row
    rope_T: int = 0
    rope_cols: int = 0
    overlap: bool = False        # A is an as_strided view of ONE flat buffer with lda < K: consecutive rows share columns
    nan_pad: bool = False        # the columns of the allocations past the views' widths hold NaN (a tail read instead of predicated poisons C)
    seed: int = 0

    def stride(self, which: str) -> int:
        dense = {"lda": self.K1 or self.K, "lda2": self.K - self.K1, "ldw": self.K, "ldc": self.N, "ldr": self.N}[which]
        return getattr(self, which) or dense


_T128 = [
    Case("dma-threshold-4096x1024x64", 4096, 1024, 64, "T128_DMA", "32 x 8 = 256 tiles of 128 x 128: the smallest launch on the 128-row kernels",
         seed=1),
    Case("dma-one-row-tile-3969x1000x96", 3969, 1000, 96, "T128_DMA",
         "last row tile holds 1 row (clamped sources), last column wave 40 columns: vector and scalar epilogue waves in one launch",
         bias=True, act=ACT_GELU, residual=True, seed=2),
    Case("dma-33-panels-4100x1056x32", 4100, 1056, 32, "T128_DMA",
         "33 row panels: grid_m = 40, 7 panels of blocks return; last tile 4 rows; last column tile 32 columns (its second wave is "
         "outside N); one K tile: the loop runs once with no next tile; out is a view, ldc = 1060",
         ldc=1060, bias=True, act=ACT_SILU, seed=3),
    Case("dma-scalar-epilogue-4033x1090x64", 4033, 1090, 64, "T128_DMA",
         "last row tile 65 rows, last column tile 66 columns (last wave: 2); ldc = 1090 (not a multiple of 4) puts every wave on the "
         "scalar epilogue; the residual is the output buffer",
         ldc=1090, ldr=1090, bias=True, residual=True, alias=True, seed=4),
    Case("dma-a2-switch-first-4096x1024x128-k1-32", 4096, 1024, 128, "T128_DMA",
         "K1 = 32 of 4 K tiles: the A -> A2 switch is the FIRST loop step's load; A2 is a column view of a wider tensor (lda2 = 160)",
         K1=32, lda2=160, bias=True, seed=5),
    Case("dma-a2-switch-last-4096x1024x128-k1-96", 4096, 1024, 128, "T128_DMA",
         "K1 = 96 of 4 K tiles: the switch is the LAST load of the loop; A2 is a column view of a wider tensor (lda2 = 96)",
         K1=96, lda2=96, residual=True, seed=6),
    Case("dma-rope-partial-tile-4158x1152x64", 4158, 1152, 64, "T128_DMA",
         "H = 6: N = 3 * 384, rope_cols = 768; Bt = 54 sequences of T = 77 frames: M = 4158, last row tile 62 rows, every tile "
         "straddles sequences", rope="shared", rope_T=77, rope_cols=768, seed=7),
    Case("dma-rope-per-row-4158x1152x64", 4158, 1152, 64, "T128_DMA",
         "the same launch with one table row per GEMM row (rope_T = M, cos / sin [M][32]): the ragged-batch form",
         rope="per_row", rope_T=4158, rope_cols=768, seed=8),
    Case("dma-overlap-hubert-8197x512x96", 8197, 512, 96, "T128_DMA",
         "HuBERT conv as a GEMM over overlapping channels-last rows: kernel 3, stride 2, 32 channels: K = 96, lda = 64 < K; 65 row "
         "panels, last tile 5 rows", lda=64, overlap=True, bias=True, act=ACT_GELU, seed=9),
    Case("dma-overlap-mel-8100x482x480", 8100, 482, 480, "T128_DMA",
         "mel DFT framing: hop 160, window 480: lda = 160 < K = 480 (15 K tiles), N = 482: last column wave 34 columns; 64 x 4 = 256 tiles",
         lda=160, overlap=True, seed=10),
    Case("gen128-k80-4100x1000", 4100, 1000, 80, "T128_GENERIC",
         "to_embed's K = 80: 2.5 K tiles, the tail predicated; 33 row panels, last tile 4 rows, last column wave 40 columns",
         lda=96, ldw=112, nan_pad=True, bias=True, seed=11),
    Case("gen128-k36-4100x1000", 4100, 1000, 36, "T128_GENERIC",
         "K = 36: one whole K tile and a 4-column tail (one 16-byte load per row of the second tile)",
         lda=40, ldw=44, nan_pad=True, bias=True, act=ACT_SILU, residual=True, ldc=1004, seed=12),
    Case("gen128-a2-tail-4100x1000x112-k1-32", 4100, 1000, 112, "T128_GENERIC",
         "K1 = 32: A2 carries 80 columns, so the predicated tail is A2's (limit K - K1), not A's",
         K1=32, lda=64, lda2=128, ldw=128, nan_pad=True, residual=True, seed=13),
]

_T64 = [
    Case("t64-below-threshold-3968x1024x64", 3968, 1024, 64, "T64", "31 x 8 = 248 tiles of 128 x 128: the largest neighbour below the threshold",
         bias=True, seed=20),
    Case("t64-1x8x32", 1, 8, 32, "T64", "one row, 8 columns, one K tile: every other row and column of the tile is clamped",
         bias=True, act=ACT_GELU, seed=21),
    Case("t64-64x128x64", 64, 128, 64, "T64", "exactly one full 64 x 128 tile (M = 64 is the last M that ignores the tile count)",
         residual=True, seed=22),
    Case("t64-65x200x96", 65, 200, 96, "T64", "second row tile holds 1 row; second column tile 72 columns: its last wave 8 columns (scalar)",
         bias=True, act=ACT_SILU, residual=True, ldc=204, seed=23),
    Case("gen64-130x66x80", 130, 66, 80, "T64_GENERIC", "three row tiles, the last with 2 rows; 66 columns: the second wave 2 columns; K tail 16",
         lda=96, ldw=96, nan_pad=True, bias=True, act=ACT_GELU, ldc=66, seed=24),
    Case("gen64-63x1090x36", 63, 1090, 36, "T64_GENERIC", "M < 64; nine column tiles, ldc = 1090: scalar epilogue; 4-column K tail; residual in place",
         lda=40, ldw=40, nan_pad=True, ldc=1090, ldr=1090, residual=True, alias=True, seed=25),
    Case("gen64-a2-257x384x112-k1-32", 257, 384, 112, "T64_GENERIC", "five row tiles, the last with 1 row; K1 = 32, A2's 80 columns carry the tail",
         K1=32, lda=32, lda2=96, ldw=112, nan_pad=True, bias=True, seed=26),
]

CASES: List[Case] = _T128 + _T64
BY_NAME: Dict[str, Case] = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# (M, N, K) on either side of the 256-tile threshold and of M = 64 -> the form the rule gives
THRESHOLDS = [((4096, 1024, 64), "T128_DMA"), ((3968, 1024, 64), "T64"), ((4096, 1024, 36), "T128_GENERIC"), ((3968, 1024, 36), "T64_GENERIC"),
              ((64, 128 * 256, 32), "T64"), ((65, 128 * 256, 32), "T128_DMA"), ((65, 128 * 255, 32), "T64")]

# calls the library refuses (CVX_EINVAL, nothing launched, C untouched): name -> the fields to change on a valid 128 x 128 x 64 call
REFUSALS = ("K%4", "lda%4", "ldw%4", "misaligned_A", "K1%32", "K1>=K", "rope_cols%64", "rope_cols>N", "act_tanh")


# ------------------------------------------------------------------------------------------------ operands
class Problem:
    """Operands of one case.  `alloc` holds the allocations (contiguous; what a test moves to the GPU), views(alloc) the tensors the
    call takes: a, a2, w, bias, res, cos, sin (None where the case has none).  `row_groups`: lists of rows that hold COPIES of one A
    (and A2, residual, table) row and share the RoPE position - their rows of C are equal bit for bit in a correct kernel;
    `col_pair`: (0, N - 1) where W rows, bias and residual columns 0 and N - 1 are copies (cases without RoPE), else None."""

    def __init__(self, case: Case):
        c = self.case = case
        g = torch.Generator().manual_seed(7919 * c.seed + c.M + 3 * c.N + 5 * c.K)
        rn = lambda *s: torch.randn(*s, generator=g)
        ka = c.K1 or c.K
        lda, ldw = c.stride("lda"), c.stride("ldw")
        al: Dict[str, torch.Tensor] = {}
        if c.overlap:
            assert lda < c.K and c.K1 == 0
            al["a"] = rn((c.M - 1) * lda + c.K)
        else:
            assert lda >= ka
            al["a"] = rn(c.M, lda)
        if c.K1:
            assert c.stride("lda2") >= c.K - c.K1
            al["a2"] = rn(c.M, c.stride("lda2"))
        assert ldw >= c.K
        al["w"] = rn(c.N, ldw) / math.sqrt(c.K)
        if c.bias:
            al["bias"] = rn(c.N) * 0.5
        if c.residual:
            assert c.stride("ldr") >= c.N
            al["res"] = rn(c.M, c.stride("ldr"))
        if c.rope:
            assert c.rope_cols % 64 == 0 and c.rope_cols <= c.N and c.rope_T == (c.M if c.rope == "per_row" else c.rope_T)
            inv = 1.0 / (10000 ** (torch.arange(0, 64, 2).float() / 64))
            pos = torch.arange(c.rope_T).float()
            if c.rope == "per_row":                              # a ragged batch: positions restart at every sequence
                pos = pos % 211
            ang = pos[:, None] * inv[None, :]
            al["cos"], al["sin"] = ang.cos().contiguous(), ang.sin().contiguous()
        self.alloc = al
        v = self.views(al)
        # ---- planted copies (written through the views, so overlapping rows and padded allocations are handled alike)
        M, N = c.M, c.N
        bm = 128 if c.form.startswith("T128") else 64
        mid = min((-(-M // bm) // 2) * bm + bm // 2 + 5, M - 1)           # a row of the second wave row of a middle tile
        if c.rope == "shared":
            T = c.rope_T
            assert M % T == 0 and M // T >= 3
            nseq = M // T
            groups = [[0, T * (nseq // 2), T * (nseq - 1)], [T - 1, T * (nseq // 2) + T - 1, M - 1]]
        else:
            groups = [sorted({0, mid, M - 1})]
        self.row_groups = [gr for gr in groups if len(gr) > 1]
        for gr in self.row_groups:
            for r in gr[1:]:
                v["a"][r] = v["a"][gr[0]]
                if c.K1:
                    v["a2"][r] = v["a2"][gr[0]]
                if c.residual:
                    v["res"][r] = v["res"][gr[0]]
                if c.rope == "per_row":
                    v["cos"][r], v["sin"][r] = v["cos"][gr[0]], v["sin"][gr[0]]
        self.col_pair = None
        if c.rope is None and N > 1:
            v["w"][N - 1] = v["w"][0]
            if c.bias:
                v["bias"][N - 1] = v["bias"][0]
            if c.residual:
                v["res"][:, N - 1] = v["res"][:, 0]
            self.col_pair = (0, N - 1)
        if c.nan_pad:                                                      # after the copies: the padding is never a copy's source
            assert not c.overlap
            al["a"][:, ka:] = float("nan")
            al["w"][:, c.K:] = float("nan")
            if c.K1:
                al["a2"][:, c.K - c.K1:] = float("nan")
        self.v = v

    def views(self, al: Dict[str, torch.Tensor]) -> Dict[str, Optional[torch.Tensor]]:
        c = self.case
        ka = c.K1 or c.K
        v: Dict[str, Optional[torch.Tensor]] = dict(a2=None, bias=al.get("bias"), res=None, cos=al.get("cos"), sin=al.get("sin"))
        v["a"] = al["a"].as_strided((c.M, c.K), (c.stride("lda"), 1)) if c.overlap else al["a"][:, :ka]
        if c.K1:
            v["a2"] = al["a2"][:, :c.K - c.K1]
        v["w"] = al["w"][:, :c.K]
        if c.residual:
            v["res"] = al["res"][:, :c.N]
        return v

    def a_cat(self, dtype, swap: bool = False) -> torch.Tensor:
        a = self.v["a"].to(dtype)
        if self.case.K1:
            a2 = self.v["a2"].to(dtype)
            return torch.cat([a2, a] if swap else [a, a2], 1)
        return a.contiguous()

    def positions(self) -> Optional[torch.Tensor]:
        return torch.arange(self.case.M) % self.case.rope_T if self.case.rope else None


# One case's problem, accumulators, reference and bound are kept (a few hundred MB at the largest shapes): the tests walk the table case
# by case, so everything a case needs is computed once and dropped when the next case asks.
_CACHE: Dict[Tuple[str, str], object] = {}


def _cached(kind: str, name: str, make):
    if (kind, name) not in _CACHE:
        for k in [k for k in _CACHE if k[1] != name]:
            del _CACHE[k]
        _CACHE[(kind, name)] = make()
    return _CACHE[(kind, name)]


def _problem(name: str) -> Problem:
    return _cached("problem", name, lambda: Problem(BY_NAME[name]))


def problem(case: Case) -> Problem:
    return _problem(case.name)


# ------------------------------------------------------------------------------------------------ reference
def _act(v: torch.Tensor, act: int) -> torch.Tensor:
    if act == ACT_GELU:
        return 0.5 * v * (1.0 + torch.erf(v * (1.0 / math.sqrt(2.0))))
    if act == ACT_SILU:
        return v * torch.sigmoid(v)
    assert act == ACT_NONE
    return v


def _split_heads(v: torch.Tensor, rope_cols: int) -> Tuple[torch.Tensor, torch.Tensor]:
    blk = v[:, :rope_cols].reshape(v.shape[0], rope_cols // 64, 2, 32)
    return blk[:, :, 0], blk[:, :, 1]


def epilogue(p: Problem, acc: torch.Tensor, rows: Optional[torch.Tensor] = None, pos: Optional[torch.Tensor] = None,
             res_times: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bias -> act -> half-split RoPE on [0, rope_cols) -> + residual, in acc's dtype.  rows: the GEMM rows acc's rows stand for
    (default all); pos: their RoPE positions (default row % rope_T); res_times: factor on the residual per element (mutants)."""
    c, dt = p.case, acc.dtype
    rows = torch.arange(c.M) if rows is None else rows
    v = acc.clone()
    if c.bias:
        v = v + p.v["bias"].to(dt)
    v = _act(v, c.act)
    if c.rope:
        pos = rows % c.rope_T if pos is None else pos
        cos, sin = p.v["cos"][pos].to(dt)[:, None, :], p.v["sin"][pos].to(dt)[:, None, :]
        lo, hi = _split_heads(v, c.rope_cols)
        rot = torch.stack((lo * cos - hi * sin, hi * cos + lo * sin), 2).reshape(v.shape[0], c.rope_cols)
        v = torch.cat((rot, v[:, c.rope_cols:]), 1)
    if c.residual:
        r = p.v["res"][rows].to(dt)
        v = v + (r if res_times is None else r * res_times)
    return v


def _accumulators(name: str) -> torch.Tensor:
    p = _problem(name)
    return _cached("acc", name, lambda: p.a_cat(torch.float64) @ p.v["w"].double().T)


def _reference(name: str) -> torch.Tensor:
    return _cached("ref", name, lambda: epilogue(_problem(name), _accumulators(name)))


def reference(case: Case) -> torch.Tensor:
    """[M, N] fp64.  Cached: do not modify."""
    return _reference(case.name)


def evaluate_f32(case: Case) -> torch.Tensor:
    """The contract in plain fp32 torch on the CPU."""
    p = problem(case)
    return epilogue(p, p.a_cat(torch.float32) @ p.v["w"].float().contiguous().T)


# ------------------------------------------------------------------------------------------------ the bound
def _bound(name: str) -> torch.Tensor:
    return _cached("bound", name, lambda: _make_bound(name))


def _make_bound(name: str) -> torch.Tensor:
    p = _problem(name)
    c = p.case
    acc = _accumulators(name)
    e = (c.K + 2) * U * (p.a_cat(torch.float64).abs() @ p.v["w"].double().abs().T)
    v = acc
    if c.bias:
        v = v + p.v["bias"].double()
        e = e + U * v.abs()
    if c.act != ACT_NONE:
        v = _act(v, c.act)
        e = LIPSCHITZ[c.act] * e + U * v.abs()
    if c.rope:
        lo, hi = _split_heads(v, c.rope_cols)
        elo, ehi = _split_heads(e, c.rope_cols)
        er = elo + ehi + 2.0 * U * (lo.abs() + hi.abs())
        e = torch.cat((torch.stack((er, er), 2).reshape(c.M, c.rope_cols), e[:, c.rope_cols:]), 1)
    v = _reference(name)
    if c.residual:
        e = e + U * v.abs()
    return e + U * v.abs()


def bound(case: Case) -> torch.Tensor:
    """[M, N] fp64: |C - reference(case)| <= bound(case) element by element for a correct fp32 kernel.  Cached: do not modify."""
    return _bound(case.name)


def rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def worst_ratio(out: torch.Tensor, case: Case) -> float:
    """max over elements of |out - reference| / bound (inf for a NaN)"""
    r = ((out.detach().double().cpu() - reference(case)).abs() / bound(case))
    return float("inf") if bool(torch.isnan(r).any()) else float(r.max())


# ------------------------------------------------------------------------------------------------ mutants
def mutants_of(case: Case) -> List[str]:
    """the mutants this case can express"""
    m = ["drop_k"]
    if case.M >= 2:
        m.append("last_row_from_prev")
    if case.N >= 2:
        m.append("last_col_from_prev")
    if case.K1:
        m.append("swap_a_a2")
    if case.rope:
        m.append("rope_pos_off_by_one")
    if case.residual:
        m.append("residual_twice")
    return m


def mutant(case: Case, name: str) -> torch.Tensor:
    """The reference with ONE deliberate fault, fp64 [M, N]:
      drop_k                one k-term (the largest in magnitude) missing from the dot product of element (M - 1, N - 1)
      last_row_from_prev    row M - 1 of C computed from row M - 2 of A (and A2): a clamp that is off by one
      last_col_from_prev    column N - 1 of C computed from row N - 2 of W
      swap_a_a2             the K columns read as [A2 | A] instead of [A | A2]
      rope_pos_off_by_one   the RoPE table row of the last GEMM row is the one before its own
      residual_twice        the residual added twice to element (M - 1, 0)"""
    assert name in mutants_of(case), (case.name, name)
    p, c = problem(case), case
    M, N = c.M, c.N
    acc = _accumulators(c.name)
    out = reference(case).clone()
    last = torch.tensor([M - 1])
    if name == "drop_k":
        terms = p.a_cat(torch.float64)[M - 1] * p.v["w"][N - 1].double()
        row = acc[M - 1:M].clone()
        row[0, N - 1] -= terms[terms.abs().argmax()]
        out[M - 1] = epilogue(p, row, last)[0]
    elif name == "last_row_from_prev":
        out[M - 1] = epilogue(p, acc[M - 2:M - 1], last)[0]
    elif name == "last_col_from_prev":
        a2 = acc.clone()
        a2[:, N - 1] = acc[:, N - 2]
        out = epilogue(p, a2)
    elif name == "swap_a_a2":
        out = epilogue(p, p.a_cat(torch.float64, swap=True) @ p.v["w"].double().T)
    elif name == "rope_pos_off_by_one":
        pos = torch.tensor([(M - 2) % c.rope_T])
        out[M - 1] = epilogue(p, acc[M - 1:M], last, pos=pos)[0]
    elif name == "residual_twice":
        t = torch.ones(1, N, dtype=torch.float64)
        t[0, 0] = 2.0
        out[M - 1] = epilogue(p, acc[M - 1:M], last, res_times=t)[0]
    return out
