"""CPU: the fp32 GEMM's launch rule and the table of launches tests/test_gemm_f32_forms_gpu.py runs.

  * cvx_gemm_f32_form (host arithmetic; cvx_gemm_bias_act_f32 launches by the same function) against a restatement of the rule in this
    file's own Python, over a grid that holds M = 64 / 65, 255 / 256 tiles of 128 x 128 and K % 32 = 0 / 4; invalid shapes give -1;
  * every entry of oracle/gemm_f32_oracle.CASES sits on the kernel it names, and all four kernels occur;
  * the bound of the oracle is neither too tight nor vacuous: a plain fp32 CPU evaluation of every case stays inside it (and below the
    suite's rel-L2 constant), and each of six deliberately wrong variants of the fp64 reference leaves it on at least one element.
"""
import itertools

import pytest
import torch

import gemm_f32_oracle as go

T64, T64G, T128D, T128G = range(4)


def restated_form(M: int, N: int, K: int) -> int:
    """The rule as csrc/gemm_f32.hip's header comment states it, restated: not a copy of the C expression."""
    if M < 1 or N < 1 or K < 4 or K % 4 != 0:
        return -1
    tiles = len(range(0, M, 128)) * len(range(0, N, 128))
    tall = M > 64 and tiles >= 256
    whole_k_tiles = K % 32 == 0
    return {(False, True): T64, (False, False): T64G, (True, True): T128D, (True, False): T128G}[(tall, whole_k_tiles)]


@pytest.fixture(scope="module")
def lib():
    from covomix_amd import _lib
    return _lib.load()


def test_form_function_matches_the_restated_rule(lib):
    from covomix_amd import ops
    Ms = [1, 2, 63, 64, 65, 127, 128, 129, 255 * 128, 255 * 128 + 1, 256 * 128, 3968, 3969, 4096, 8100, 2 ** 31 - 1]
    Ns = [1, 8, 127, 128, 129, 1000, 1024, 1025, 255 * 128, 255 * 128 + 1, 256 * 128, 2 ** 31 - 1]
    Ks = [4, 28, 32, 36, 64, 68, 96, 100, 480, 484, 2 ** 31 - 4]
    seen = set()
    for M, N, K in itertools.product(Ms, Ns, Ks):
        want = restated_form(M, N, K)
        assert lib.cvx_gemm_f32_form(M, N, K) == want, (M, N, K)
        assert ops.gemm_f32_form(M, N, K) == go.FORMS[want] == ops.GEMM_F32_FORMS[want]
        seen.add(want)
    assert seen == {T64, T64G, T128D, T128G}
    # the edges by name: M = 64 / 65 at 256 tiles, 255 / 256 tiles at M > 64, K % 32 = 0 / 4
    for (M, N, K), form in go.THRESHOLDS:
        assert ops.gemm_f32_form(M, N, K) == form, (M, N, K)
    assert ops.gemm_f32_form(64, 128 * 1000, 64) == "T64" and ops.gemm_f32_form(65, 128 * 256, 68) == "T128_GENERIC"
    assert ops.gemm_f32_form(128 * 255, 128, 32) == "T64" and ops.gemm_f32_form(128 * 255 + 1, 128, 32) == "T128_DMA"


@pytest.mark.parametrize("shape", [(0, 8, 32), (-1, 8, 32), (8, 0, 32), (8, -5, 32), (8, 8, 0), (8, 8, 2), (8, 8, 3), (8, 8, 34),
                                   (8, 8, -32), (4096, 1024, 30)])
def test_form_function_refuses_shapes_no_launch_has(lib, shape):
    from covomix_amd import ops
    assert lib.cvx_gemm_f32_form(*shape) == -1 == restated_form(*shape)
    with pytest.raises(ValueError):
        ops.gemm_f32_form(*shape)


def test_every_case_sits_on_the_form_it_names():
    from covomix_amd import ops
    for c in go.CASES:
        assert ops.gemm_f32_form(c.M, c.N, c.K) == c.form, c.name
        assert c.reason and c.form in go.FORMS
        # the call is one the library accepts (validate_gemm_args)
        assert c.K % 4 == 0 and c.stride("lda") % 4 == 0 and c.stride("ldw") % 4 == 0
        assert c.K1 == 0 or (0 < c.K1 < c.K and c.K1 % 32 == 0 and c.stride("lda2") % 4 == 0)
        assert c.stride("ldc") >= c.N and (not c.alias or (c.residual and c.stride("ldr") == c.stride("ldc")))
    assert {c.form for c in go.CASES} == set(go.FORMS)
    # the features the table must hold somewhere on the 128-row kernels
    t128 = [c for c in go.CASES if c.form == "T128_DMA"]
    assert any(c.M % 128 == 1 for c in t128) and any(-(-c.M // 128) % 8 != 0 for c in t128) and any(c.N % 64 not in (0, 32) for c in t128)
    assert {c.K1 for c in t128 if c.K1} == {32, 96} and {c.rope for c in t128} == {None, "shared", "per_row"}
    assert sum(c.overlap for c in t128) == 2 and any(c.alias for c in t128) and any(c.stride("ldc") % 4 for c in t128)
    gen = [c for c in go.CASES if c.form == "T128_GENERIC"]
    assert {c.K for c in gen} == {80, 36, 112} and all(c.nan_pad for c in gen) and any(c.K1 for c in gen)


@pytest.mark.parametrize("case", go.CASES, ids=lambda c: c.name)
def test_bound_holds_a_plain_fp32_evaluation_and_rejects_every_mutant(case):
    p = go.problem(case)
    ref, bnd = go.reference(case), go.bound(case)
    assert ref.shape == (case.M, case.N) and bool(torch.isfinite(ref).all()) and bool((bnd > 0).all())
    # the planted copies the GPU test relies on: equal operand rows / columns (the fp64 reference's own rows agree to its rounding
    # only: a CPU BLAS is free to sum an edge row in another order)
    for gr in p.row_groups:
        for r in gr[1:]:
            assert all(torch.equal(p.v[k][r], p.v[k][gr[0]]) for k in ("a", "a2", "res") if p.v[k] is not None), (case.name, gr)
            assert case.rope is None or int(p.positions()[r]) == int(p.positions()[gr[0]]) or case.rope == "per_row"
            assert case.rope != "per_row" or (torch.equal(p.v["cos"][r], p.v["cos"][gr[0]]) and torch.equal(p.v["sin"][r], p.v["sin"][gr[0]]))
            assert float((ref[r] - ref[gr[0]]).abs().max()) <= 1e-12 * float(ref[r].abs().max()), (case.name, gr)
    if p.col_pair is not None:
        c0, c1 = p.col_pair
        assert torch.equal(p.v["w"][c0], p.v["w"][c1])
        assert float((ref[:, c0] - ref[:, c1]).abs().max()) <= 1e-12 * float(ref[:, c0].abs().max())
    assert p.row_groups or case.M == 1
    # not too tight: plain fp32 stays inside, everywhere
    out = go.evaluate_f32(case)
    ratio, l2 = go.worst_ratio(out, case), go.rel_l2(out, ref)
    print(f"fp32-cpu {case.name}: worst |error| / bound {ratio:.3f}, rel-L2 {l2:.2e}")
    assert ratio <= 1.0, (case.name, ratio)
    assert l2 < go.TOL, (case.name, l2)
    # not vacuous: every fault leaves the bound on at least one element
    for name in go.mutants_of(case):
        worst = float(((go.mutant(case, name) - ref).abs() / bnd).max())
        print(f"  mutant {name}: worst |difference| / bound {worst:.3g}")
        assert worst > 1.0, (case.name, name, worst)


def test_every_mutant_is_exercised_by_some_case():
    seen = set()
    for c in go.CASES:
        seen.update(go.mutants_of(c))
    assert seen == set(go.MUTANTS)
