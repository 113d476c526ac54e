"""Every kernel of the fp32 GEMM (cvx_gemm_bias_act_f32: T64 gemm_f32_kernel<1>, T64_GENERIC / T128_GENERIC gemm_f32_generic_kernel<1 / 2>,
T128_DMA gemm_f32_glds_kernel) against an fp64 reference at its tile edges, through ops.gemm, i.e. the C ABI.

The table of launches, the reference and the per-element bound live in oracle/gemm_f32_oracle.py; tests/test_gemm_f32_forms.py proves
on the CPU that every case takes the kernel it names (through the library's own launch rule, cvx_gemm_f32_form), that a plain fp32
evaluation stays inside the bound and that six deliberately wrong variants of the reference leave it.  Per case:

  output guard           C is a view of an allocation of M + 1 rows of ldc floats pre-filled with a sentinel bit pattern: row M and the
                         columns [N, ldc) hold it afterwards, the [M, N] block holds neither the sentinel nor a NaN;
  per-element error      |C - reference| <= bound for EVERY element (bound: (K + 2) 2^-23 |A| |W|^T pushed through the epilogue; derived
                         in the oracle, not measured);
  rel-L2                 below 2e-6, the TOL of tests/test_kernels_gpu.py;
  position independence  rows of C whose A (A2, residual) rows are copies and whose RoPE table rows agree - one in the first tile, one
                         in another wave of a middle tile, one in the last, partial tile - are equal bit for bit; without RoPE so are
                         columns 0 and N - 1 (copies of one W row, bias and residual column): a vector and a scalar epilogue wave;
  in-place residual      a case whose residual is the output buffer equals the run with a separate residual tensor bit for bit.
Different kernels are NOT compared bit for bit: the header does not promise it.

MEASURED (MI355X): worst |error| / bound over all elements, and rel-L2 against fp64 - a record, not a threshold:
  case                                       kernel        ratio    rel-L2
  dma-threshold-4096x1024x64                 T128_DMA      0.0426   1.437e-07
  dma-one-row-tile-3969x1000x96              T128_DMA      0.0350   1.101e-07
  dma-33-panels-4100x1056x32                 T128_DMA      0.0844   1.166e-07
  dma-scalar-epilogue-4033x1090x64           T128_DMA      0.0429   1.023e-07
  dma-a2-switch-first-4096x1024x128-k1-32    T128_DMA      0.0215   1.837e-07
  dma-a2-switch-last-4096x1024x128-k1-96     T128_DMA      0.0227   1.464e-07
  dma-rope-partial-tile-4158x1152x64         T128_DMA      0.0470   1.464e-07
  dma-rope-per-row-4158x1152x64              T128_DMA      0.0379   1.459e-07
  dma-overlap-hubert-8197x512x96             T128_DMA      0.0268   1.828e-07
  dma-overlap-mel-8100x482x480               T128_DMA      0.0069   3.924e-07
  gen128-k80-4100x1000                       T128_GENERIC  0.0351   1.475e-07
  gen128-k36-4100x1000                       T128_GENERIC  0.0706   7.370e-08
  gen128-a2-tail-4100x1000x112-k1-32         T128_GENERIC  0.0260   1.374e-07
  t64-below-threshold-3968x1024x64           T64           0.0445   1.309e-07
  t64-1x8x32                                 T64           0.0053   2.588e-08
  t64-64x128x64                              T64           0.0253   1.076e-07
  t64-65x200x96                              T64           0.0204   1.092e-07
  gen64-130x66x80                            T64_GENERIC   0.0167   1.614e-07
  gen64-63x1090x36                           T64_GENERIC   0.0509   8.116e-08
  gen64-a2-257x384x112-k1-32                 T64_GENERIC   0.0203   1.721e-07
"""
import ctypes as C

import pytest
import torch

import gemm_f32_oracle as go

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0DEAD      # a quiet NaN with a payload no kernel produces
CVX_EINVAL = -22


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import covomix_amd.ops as o
    return o


def dev():
    return torch.device("cuda:0")


def _guarded_out(case):
    """(allocation [M + 1, ldc] of sentinels, the [M, N] view the call writes)"""
    alloc = torch.full((case.M + 1, case.stride("ldc")), SENTINEL, dtype=torch.int32, device=dev()).view(torch.float32)
    return alloc, alloc[:case.M, :case.N]


def _run(ops, case, p, v, out, residual):
    rope = (v["cos"], v["sin"]) if case.rope else None
    ops.gemm(v["a"], v["w"], out, bias=v["bias"], act=case.act, residual=residual, a2=v["a2"], rope=rope, rope_cols=case.rope_cols)
    torch.cuda.synchronize()


def _check_guard(case, alloc):
    bits = alloc.view(torch.int32)
    assert bool((bits[case.M] == SENTINEL).all()), f"{case.name}: row M was written"
    assert bool((bits[:case.M, case.N:] == SENTINEL).all()), f"{case.name}: columns [N, ldc) were written"
    block = bits[:case.M, :case.N]
    assert not bool((block == SENTINEL).any()), f"{case.name}: an element of C was not written"
    assert not bool(torch.isnan(alloc[:case.M, :case.N]).any()), f"{case.name}: NaN in C"


@pytest.mark.parametrize("case", go.CASES, ids=lambda c: c.name)
def test_gemm_f32_form_against_fp64(ops, case):
    assert ops.gemm_f32_form(case.M, case.N, case.K) == case.form
    p = go.problem(case)
    v = p.views({k: t.to(dev()) for k, t in p.alloc.items()})
    for k, t in v.items():                                   # the call sees the strides the case names
        if t is not None and t.ndim == 2 and k in ("a", "a2", "w", "res"):
            assert t.stride(0) == case.stride({"a": "lda", "a2": "lda2", "w": "ldw", "res": "ldr"}[k]) and t.stride(1) == 1, (k, t.stride())
    alloc, out = _guarded_out(case)
    assert out.stride(0) == case.stride("ldc")
    if case.alias:                                           # in place: the output buffer holds the residual
        out.copy_(v["res"])
        _run(ops, case, p, v, out, out)
    else:
        _run(ops, case, p, v, out, v["res"])
    _check_guard(case, alloc)
    got = out.cpu()
    ref, bnd = go.reference(case), go.bound(case)
    err = (got.double() - ref).abs()
    ratio, l2 = float((err / bnd).max()), go.rel_l2(got, ref)
    print(f"GEMM_F32_FORMS {case.name} [{case.form}]: worst |error| / bound {ratio:.4f}, rel-L2 {l2:.3e}")
    over = int((err > bnd).sum())
    assert over == 0, (case.name, over, ratio)
    assert l2 < go.TOL, (case.name, l2)
    # position independence
    bits = got.view(torch.int32)
    for gr in p.row_groups:
        for r in gr[1:]:
            assert torch.equal(bits[r], bits[gr[0]]), f"{case.name}: rows {gr[0]} and {r} hold copies of one problem row and differ"
    if p.col_pair is not None:
        c0, c1 = p.col_pair
        assert torch.equal(bits[:, c0], bits[:, c1]), f"{case.name}: columns {c0} and {c1} hold copies of one problem column and differ"
    if case.alias:                                           # the same call with the residual in a tensor of its own
        alloc2, out2 = _guarded_out(case)
        _run(ops, case, p, v, out2, v["res"])
        _check_guard(case, alloc2)
        assert torch.equal(out2.cpu().view(torch.int32), bits), f"{case.name}: in place differs from out of place"


def test_all_four_kernels_are_in_the_table(ops):
    assert {ops.gemm_f32_form(c.M, c.N, c.K) for c in go.CASES} == set(ops.GEMM_F32_FORMS)


# ------------------------------------------------------------------------------------------------ refusals
def _valid_call(ops, M=128, N=128, K=64):
    """A call the library accepts (a 128 x 128 x 64 product with every optional operand present), as raw cvx_gemm_args, and what keeps
    its memory alive."""
    from covomix_amd._lib import GemmArgs
    g = torch.Generator().manual_seed(5)
    t = dict(a=torch.randn(M, K + 8, generator=g).to(dev()), a2=torch.randn(M, K, generator=g).to(dev()),
             w=torch.randn(N, K + 8, generator=g).to(dev()), cos=torch.ones(16, 32, device=dev()), sin=torch.zeros(16, 32, device=dev()))
    t["alloc"] = torch.full((M + 1, N), SENTINEL, dtype=torch.int32, device=dev())
    a = GemmArgs()
    a.A, a.lda = t["a"].data_ptr(), K + 8
    a.A2, a.lda2, a.K1 = None, 0, 0
    a.W, a.ldw = t["w"].data_ptr(), K + 8
    a.C, a.ldc = t["alloc"].data_ptr(), N
    a.bias, a.residual, a.ldr = None, None, 0
    a.M, a.N, a.K, a.act = M, N, K, go.ACT_NONE
    a.rope_cos, a.rope_sin, a.rope_T, a.rope_cols = None, None, 0, 0
    return a, t


def _with_a2(a, t, K1):
    a.A2, a.lda2, a.K1 = t["a2"].data_ptr(), t["a2"].stride(0), K1


def _with_rope(a, t, cols):
    a.rope_cos, a.rope_sin, a.rope_T, a.rope_cols = t["cos"].data_ptr(), t["sin"].data_ptr(), 16, cols


REFUSALS = {
    "K%4": lambda a, t: setattr(a, "K", 62),
    "lda%4": lambda a, t: setattr(a, "lda", 70),
    "ldw%4": lambda a, t: setattr(a, "ldw", 70),
    "misaligned_A": lambda a, t: setattr(a, "A", t["a"].data_ptr() + 4),
    "K1%32": lambda a, t: _with_a2(a, t, 16),
    "K1>=K": lambda a, t: _with_a2(a, t, 64),
    "rope_cols%64": lambda a, t: _with_rope(a, t, 32),
    "rope_cols>N": lambda a, t: _with_rope(a, t, 192),
    "act_tanh": lambda a, t: setattr(a, "act", go.ACT_TANH),
}
assert tuple(REFUSALS) == go.REFUSALS


@pytest.mark.parametrize("what", go.REFUSALS)
def test_gemm_f32_refuses_and_leaves_c_untouched(ops, what):
    from covomix_amd import _lib
    lib = _lib.load()
    a, t = _valid_call(ops)
    REFUSALS[what](a, t)
    rc = lib.cvx_gemm_bias_act_f32(C.byref(a), ops._stream())
    torch.cuda.synchronize()
    assert rc == CVX_EINVAL, (what, rc)
    assert bool((t["alloc"] == SENTINEL).all()), f"{what}: a refused call wrote to C"
    assert lib.cvx_last_error_string()


def test_gemm_f32_valid_twin_of_the_refusals_runs_and_m0_writes_nothing(ops):
    """The call the refusals are derived from is accepted (so each refusal is due to the one field it changes), and M = 0 is CVX_OK
    without a store."""
    from covomix_amd import _lib
    lib = _lib.load()
    a, t = _valid_call(ops)
    a.M = 0
    assert lib.cvx_gemm_bias_act_f32(C.byref(a), ops._stream()) == 0
    torch.cuda.synchronize()
    assert bool((t["alloc"] == SENTINEL).all())
    a.M = 128
    _with_a2(a, t, 32)
    _with_rope(a, t, 64)
    assert lib.cvx_gemm_bias_act_f32(C.byref(a), ops._stream()) == 0
    torch.cuda.synchronize()
    assert bool((t["alloc"][128] == SENTINEL).all()) and not bool((t["alloc"][:128] == SENTINEL).any())
    ref = torch.cat([t["a"][:, :32], t["a2"][:, :32]], 1).double() @ t["w"][:, :64].double().T        # cos = 1, sin = 0: RoPE is the identity
    assert go.rel_l2(t["alloc"][:128].view(torch.float32), ref) < go.TOL
