"""CPU: the route table of tests/acoustic_routes.py against the package's published constants and against acoustic.route itself, field for
field, and the library's own host arithmetic for the split-K scratch (cvx_gemm_f16x3_workspace_floats).

The finding this file writes down: at exactly M = 2048 rows two rules meet that are not the same rule.  The walkers fuse the norms into
their producers for M < acoustic.FUSE_NORM_BELOW_ROWS = 2048; ops.gemm hands the split-K scratch over for M <=
ops.SPLITK_SCRATCH_MAX_ROWS = 2048; cvx_gemm_f16x3_workspace_floats counts the
medium-problem kernel's slices for M < 2048 only; and the launch code asks splitk_factor_p8m whenever the round rule picked the
medium-problem kernel and a scratch came with the call, without looking at M.  On 256 CUs the round rule gives every GEMM of a
dim = 512 or dim = 1024 layer to the medium-problem kernel at 2048 rows, so that one row count runs K slices on separate blocks, the
plain reduction kernel and a STAND-ALONE adarmsnorm: the launch code follows ops.gemm's rule, not workspace_floats'.  Nothing is read or
written past the scratch (the launch code compares the slices' floats with the size the caller passed, and ops.gemm passes 4 x 2048 x
4096 floats whatever the shape) and no norm is left undone (norm= is never passed at 2048 rows); a caller that sized its scratch by
workspace_floats would merely get one slice where ops.gemm's callers get two or four."""
import dataclasses
import operator

import pytest
from acoustic_routes import (DEFER_FLOOR_ROWS, FUSE_NORM_BELOW_ROWS, GRAPH_MAX_ROWS_DEFAULT, SCRATCH_UP_TO_ROWS, SPLIT_IO_ABOVE_ROWS, Route,
                             expected_record, gemm_kernel, layer_gemms, published, route)
from gemm_guarded import WORKSPACE_FLOATS, splitk_factor_p8m
from hubert_routes import splitk_factor


@pytest.fixture(scope="module")
def lib():
    from covomix_amd import _lib
    return _lib.load()


SWEEP_ROWS = tuple(range(1, 8201)) + (9216, 16000, 16384, 20480)
SWEEP_DIMS = (96, 128, 512, 520, 1024, 4096, 8192)          # 96 and 520: the % 32 (f16x3) and % 64 (f16, deferred) conditions


def _sweep(what):
    """acoustic.route == the restated route, field for field, over every row count, width, precision and batch kind"""
    from covomix_amd import acoustic as ac
    fields, consts = operator.attrgetter(*Route._fields), published()
    assert type(ac.route(1, 512, "f16x3")) is ac.Route and tuple(f.name for f in dataclasses.fields(ac.Route)) == Route._fields
    for p in ("f16x3", "fp32", "f16"):
        for dim in SWEEP_DIMS:
            for M in SWEEP_ROWS:
                for rr in (None, M):
                    got, want = ac.route(M, dim, p, rr), route(M, dim, p, rr, consts)
                    assert fields(got) == want, (what, M, dim, p, rr, got, want)


def test_published_constants_and_inline_rules(monkeypatch):
    """The constants the table reads, its restated literals against the library's named thresholds, and the library's route function
    against the restated one in the default environment: a change of either must come with a change of tests/acoustic_routes.py (and
    of the cases of the GPU file, which sit either side of these numbers)."""
    for k in ("CVX_DEFER_NORM", "CVX_GRAPH", "CVX_GRAPH_MAX_ROWS"):
        monkeypatch.delenv(k, raising=False)
    assert published() == (128, 8192, 1024, 8192, SPLIT_IO_ABOVE_ROWS, FUSE_NORM_BELOW_ROWS, SCRATCH_UP_TO_ROWS, GRAPH_MAX_ROWS_DEFAULT,
                           DEFER_FLOOR_ROWS)
    _sweep("defaults")


@pytest.mark.parametrize("name,value", [("CVX_DEFER_NORM", "0"), ("CVX_GRAPH", "0"), ("CVX_GRAPH_MAX_ROWS", "4096"), ("DEFER_MIN_ROWS", 2048),
                                        ("DEFER_MIN_ROWS", 1024)])
def test_route_function_under_a_setting(name, value, monkeypatch):
    """The same sweep with one switch moved.  DEFER_MIN_ROWS = 1024 pins the floor the deferred forms have at 2048 rows (the
    large-problem kernel takes no fewer): the setting acts as 2048."""
    from covomix_amd import acoustic as ac
    for k in ("CVX_DEFER_NORM", "CVX_GRAPH", "CVX_GRAPH_MAX_ROWS"):
        monkeypatch.delenv(k, raising=False)
    if name == "DEFER_MIN_ROWS":
        monkeypatch.setattr(ac.VectorField, name, value)
        assert [ac.route(M, 512, "f16x3").deferred for M in (value - 1, value, 2047, 2048)] == [False, value == 2048, False, True]
    else:
        monkeypatch.setenv(name, value)
    _sweep(f"{name}={value}")


def test_route_table_at_every_crossing():
    R = Route
    # dim = 512, f16x3:             split  il     fuse   scratch defer  graph
    want = {64: R(False, False, False, False, False, True, None), 65: R(True, False, True, True, False, True, None),
            66: R(True, False, True, True, False, True, None), 127: R(True, False, True, True, False, True, None),
            128: R(True, True, True, True, False, True, None), 129: R(True, True, True, True, False, True, None),
            2046: R(True, True, True, True, False, True, None), 2047: R(True, True, True, True, False, True, None),
            2048: R(True, True, False, True, False, True, None), 2049: R(True, True, False, False, False, True, None),
            8190: R(True, True, False, False, False, True, None), 8192: R(True, True, False, False, True, True, None),
            8194: R(True, True, False, False, True, False, None)}
    for M, r in want.items():
        assert route(M, 512, "f16x3") == r == route(M, 1024, "f16x3"), M
    # 'f16' keeps hi halves only: no interleaved pairs, so no deferred norms - and the same fuse_norm / scratch boundaries
    for M, r in want.items():
        assert route(M, 512, "f16") == r._replace(interleaved=False, deferred=False), M
        assert route(M, 512, "fp32") == R(False, False, False, False, False, r.graph, None), M
        assert route(M, 128, "f16x3") == r._replace(interleaved=False, deferred=False), M      # (what test_edge_shapes_vs_oracle can reach)
    # ragged: never a graph, capacity in steps of 1024 rows, everything else from the real row count
    for M, cap in ((64, 1024), (128, 1024), (2046, 2048), (2048, 2048), (2050, 3072), (2047, 2048), (2049, 3072), (8190, 8192),
                   (8192, 8192), (8194, 9216)):
        assert route(M, 512, "f16x3", ragged_rows=M) == route(M, 512, "f16x3")._replace(graph=False, ragged_capacity=cap), M
    # the one point where the two 2048-row rules part
    r = route(2048, 512, "f16x3")
    assert r.splitk_scratch and not r.fuse_norm
    assert all(route(M, 512, p).splitk_scratch == route(M, 512, p).fuse_norm for M in (65, 2047, 2049, 4000) for p in ("f16x3", "f16"))


def test_expected_record_counts():
    """The launch counts the GPU file holds the recorded calls to, on the two networks it runs (depth 4 with combiners in layers 2-3,
    depth 2 with one in layer 1) and on the full network (depth 8: the 15 deferred norms test_deferred_norm_is_scale_free counts)."""
    rec = expected_record(route(64, 512, "f16x3"), 4, [2, 3], 2)
    assert rec == dict(gemm_plain=1 + 2 * 20, gemm_pair=0, gemm_il=0, gemm_norm=0, gemm_rowsq=0, gemm_row_scale=0, attention=8,
                       attention_f16x3=0, adarmsnorm=18, rownorm_scale=0, scratch=0)
    rec = expected_record(route(65, 512, "f16x3"), 4, [2, 3], 2)
    assert (rec["gemm_plain"], rec["gemm_pair"], rec["gemm_il"], rec["gemm_norm"], rec["adarmsnorm"], rec["scratch"]) == (3, 38, 0, 16, 2, 30)
    rec = expected_record(route(2048, 512, "f16x3"), 4, [2, 3], 2)
    assert (rec["gemm_pair"], rec["gemm_il"], rec["gemm_norm"], rec["adarmsnorm"], rec["scratch"]) == (0, 38, 0, 18, 30)
    rec = expected_record(route(2049, 512, "f16x3"), 4, [2, 3], 2)
    assert (rec["gemm_il"], rec["gemm_norm"], rec["adarmsnorm"], rec["scratch"], rec["rownorm_scale"]) == (38, 0, 18, 0, 0)
    rec = expected_record(route(8192, 512, "f16x3"), 4, [2, 3], 2)
    assert (rec["gemm_il"], rec["gemm_rowsq"], rec["gemm_row_scale"], rec["rownorm_scale"], rec["adarmsnorm"]) == (38, 14, 14, 14, 4)
    assert expected_record(route(16000, 1024, "f16x3"), 8, [4, 5, 6, 7], 1)["rownorm_scale"] == 15
    rec = expected_record(route(2046, 1024, "f16x3"), 2, [1], 2)
    assert (rec["gemm_il"], rec["gemm_norm"], rec["adarmsnorm"], rec["scratch"]) == (20, 8, 2, 16)


@pytest.mark.parametrize("dim,heads", [(512, 8), (1024, 16)])
def test_splitk_scratch_rules_at_2048_rows(lib, dim, heads):
    """cvx_gemm_f16x3_workspace_floats against the two restated split-K rules for the GEMMs of one layer, one row either side of 2048,
    and what the launch code does with a scratch at exactly 2048 rows (see the module docstring)."""
    shapes = layer_gemms(dim, heads)
    for M in (2046, 2047, 2048, 2049):
        for name, (N, K, K1) in shapes.items():
            plain = splitk_factor(M, N, K)
            assert not K1 or plain == 1 or K1 % (K // plain) == 0                 # (A | A2 changes over at a slice boundary: the rule needs no second try)
            medium = splitk_factor_p8m(M, N, K, K1)
            # the library's figure: the larger of the plain rule and - BELOW 2048 rows only - the medium-problem kernel's
            f = max(plain, medium if M < 2048 else 1)
            assert lib.cvx_gemm_f16x3_workspace_floats(M, N, K, K1) == (f * M * N if f > 1 else 0), (M, name)
            # what ops.gemm passes covers every slice count the launch code can choose, at every row count it passes a scratch for
            if M <= SCRATCH_UP_TO_ROWS:
                assert max(plain, medium) * M * N <= WORKSPACE_FLOATS, (M, name)
    # 2046 / 2047 rows: the medium-problem kernel by row count; the K-split GEMMs are those whose norm evaluate() fuses - to_out, ff2 and
    # the combiner have N = dim, one of the widths splitk_reduce_norm_kernel<N / 256> exists for (<2> at 512, <4> at 1024)
    for M in (2046, 2047):
        r = route(M, dim, "f16x3")
        assert r.fuse_norm and r.splitk_scratch
        for name in ("out", "ff2", "skip"):
            N, K, K1 = shapes[name]
            assert gemm_kernel(M, N) == "medium" and splitk_factor_p8m(M, N, K, K1) > 1 and N % 256 == 0 and N <= 1024, (M, name)
    # 2048 rows: the round rule on 256 CUs keeps every GEMM of the layer on the medium-problem kernel, ops.gemm still hands the scratch
    # over, and the launch code splits K by the medium kernel's own rule - which workspace_floats no longer counts there.  evaluate()
    # passes no norm=: the reduction is the plain one and the norm a launch of its own.
    r = route(2048, dim, "f16x3")
    assert r.splitk_scratch and not r.fuse_norm
    launched = {name: (gemm_kernel(2048, N), splitk_factor_p8m(2048, N, K, K1) if name != "qkv" else 1) for name, (N, K, K1) in shapes.items()}
    want = {512: dict(qkv=("medium", 1), out=("medium", 2), ff1=("medium", 1), ff2=("medium", 4), skip=("medium", 4)),
            1024: dict(qkv=("medium", 1), out=("medium", 2), ff1=("medium", 1), ff2=("medium", 2), skip=("medium", 2))}[dim]
    assert launched == want                                                          # (to_qkv carries RoPE: never split)
    N, K, K1 = shapes["out"]
    floats = lib.cvx_gemm_f16x3_workspace_floats(2048, N, K, K1)
    # the disagreement itself: the launch code splits to_out in two; the size query reports the plain branch's figure for it
    assert floats == (0 if dim == 512 else 2 * 2048 * N) and launched["out"][1] == 2
    if dim == 512:
        assert floats < 2 * 2048 * N                           # sized by the query, the launch code's own size check keeps K whole: safe
    # 2049 rows: no scratch from ops.gemm, so no slices whatever either rule says; the round rule still prefers 128 x 128 tiles
    r = route(2049, dim, "f16x3")
    assert not r.splitk_scratch and not r.fuse_norm and all(gemm_kernel(2049, shapes[n][0]) == "medium" for n in ("qkv", "out", "ff2", "skip"))
    # the large-problem kernel takes over where its rounds come out shorter: the 16,000-row route of bench.py stays where it was
    assert gemm_kernel(16000, 1024) == "large" and gemm_kernel(16000, 4096) == "large" and gemm_kernel(4000, 1024) == "medium"
