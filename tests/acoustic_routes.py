"""Shared by tests/test_acoustic_routes.py (CPU) and tests/test_acoustic_routes_gpu.py: which kernels one evaluation of the acoustic
network launches, as a function of its row count M (B T without guidance, 2 B T with the null branch, the sum of the lengths - doubled
under guidance - for a ragged batch).  Restated from the rules of acoustic.route and ops.gemm, with no import of their logic: only the
constants the package publishes are read from it, and tests/test_acoustic_routes.py holds this function to acoustic.route field for field.

  M <= 64            fp32 GEMM, ops.attention, adarmsnorm into fp32 (split_io false)
  65 ... 127         split pipe on separate (hi, lo) tensors, norms fused into their producers (fuse_norm), split-K scratch handed over
  128 ... 2047       interleaved pairs (SplitIL) if dim >= 512 and the precision keeps lo halves; otherwise as above
  2048               fuse_norm off (FUSE_NORM_BELOW_ROWS: M < 2048), scratch still handed over (ops.SPLITK_SCRATCH_MAX_ROWS: M <= 2048)
  2049 ... 8191      no scratch, stand-alone norms
  >= DEFER_MIN_ROWS  deferred norms on the pair-only residual stream (f16x3, interleaved pairs, 512 <= dim <= 4096, dim % 64 == 0); the
                     large-problem kernel they need starts at 2048 rows, so a DEFER_MIN_ROWS below that acts as 2048
  > 8192             no captured graph (CVX_GRAPH_MAX_ROWS); a ragged batch never has one"""
import os
from collections import namedtuple

SPLIT_IO_ABOVE_ROWS = 64          # restates acoustic.SPLIT_IO_ABOVE_ROWS: the split pipe runs for M > 64
FUSE_NORM_BELOW_ROWS = 2048       # restates acoustic.FUSE_NORM_BELOW_ROWS: norms ride in their producers for M < 2048
SCRATCH_UP_TO_ROWS = 2048         # restates ops.SPLITK_SCRATCH_MAX_ROWS: ops.gemm hands the split-K scratch over for M <= 2048 without RoPE
GRAPH_MAX_ROWS_DEFAULT = 8192     # restates acoustic.GRAPH_MAX_ROWS: rows > CVX_GRAPH_MAX_ROWS (this by default) stay eager
DEFER_FLOOR_ROWS = 2048           # restates acoustic.LARGE_KERNEL_MIN_ROWS: the deferred forms need the large-problem kernel
MI355X_CUS = 256                  # what cvx_ctx_cus gives for a stream without a CU mask

Route = namedtuple("Route", "split_io interleaved fuse_norm splitk_scratch deferred graph ragged_capacity")


def published():
    """(il_min_rows, DEFER_MIN_ROWS, RAGGED_ROW_QUANTUM, graph row limit) and the five named thresholds (SPLIT_IO_ABOVE_ROWS,
    FUSE_NORM_BELOW_ROWS, SPLITK_SCRATCH_MAX_ROWS, GRAPH_MAX_ROWS, LARGE_KERNEL_MIN_ROWS): the constants the package publishes (host
    code only).  route() below reads the first four; the others are compared with its own literals by the CPU test."""
    from covomix_amd import acoustic as ac, ops
    return (ops.il_min_rows(), ac.VectorField.DEFER_MIN_ROWS, ac.VectorField.RAGGED_ROW_QUANTUM,
            int(os.environ.get("CVX_GRAPH_MAX_ROWS", str(GRAPH_MAX_ROWS_DEFAULT))),
            ac.SPLIT_IO_ABOVE_ROWS, ac.FUSE_NORM_BELOW_ROWS, ops.SPLITK_SCRATCH_MAX_ROWS, ac.GRAPH_MAX_ROWS, ac.LARGE_KERNEL_MIN_ROWS)


def route(M, dim, precision, ragged_rows=None, consts=None):
    """The route of one evaluation of M rows.  ragged_rows: the row count of a packed ragged batch (then equal to M), None for an
    equal-length batch.  consts: published(), read once by a caller that asks for many routes under the same settings."""
    assert precision in ("f16x3", "fp32", "f16") and (ragged_rows is None or ragged_rows == M)
    il_rows, defer_rows, quantum, graph_rows = (consts or published())[:4]
    if precision == "f16x3":
        split_io = M > SPLIT_IO_ABOVE_ROWS and dim % 32 == 0
    elif precision == "f16":
        split_io = M > SPLIT_IO_ABOVE_ROWS and dim % 64 == 0
    else:
        split_io = False
    # (interleaved weights exist in every f16x3 model: to_pred always gets a copy)
    interleaved = split_io and precision == "f16x3" and M >= il_rows and dim >= 512
    fuse_norm = split_io and M < FUSE_NORM_BELOW_ROWS
    splitk_scratch = split_io and M <= SCRATCH_UP_TO_ROWS
    deferred = interleaved and M >= max(defer_rows, DEFER_FLOOR_ROWS) and dim % 64 == 0 and 512 <= dim <= 4096 and os.environ.get("CVX_DEFER_NORM", "1") == "1"
    graph = ragged_rows is None and M <= graph_rows and os.environ.get("CVX_GRAPH", "1") != "0"
    capacity = None if ragged_rows is None else -(-ragged_rows // quantum) * quantum
    return Route(split_io, interleaved, fuse_norm, splitk_scratch, deferred, graph, capacity)


def layer_gemms(dim, heads):
    """name -> (N, K, K1) of the split-precision GEMMs of one transformer layer (skip: the combiner of the later layers, A | A2)"""
    inner = heads * 64
    return dict(qkv=(3 * inner, dim, 0), out=(dim, inner, 0), ff1=(4 * dim, dim, 0), ff2=(dim, 4 * dim, 0), skip=(dim, 2 * dim, dim))


def gemm_kernel(M, N, cus=MI355X_CUS):
    """'medium' or 'large': the kernel gemm_f16x3_impl picks for interleaved operands without a deferred norm (csrc/gemm_f16x3.hip, the
    round rule): below 2048 rows or 512 columns the medium-problem kernel, otherwise whichever finishes its rounds of one tile per CU
    sooner - 256- or 192-row tiles of the large kernel (a 192-row tile at 0.8 of the time) against 128 x 128 tiles at 0.31 each."""
    if M < 2048 or N < 512:
        return "medium"
    up = lambda a, b: -(-a // b)
    t256, t192, t128 = up(M, 256) * up(N, 256), up(M, 192) * up(N, 256), up(M, 128) * up(N, 128)
    large = min(float(up(t256, cus)), 0.8 * up(t192, cus))
    return "medium" if 0.31 * up(t128, cus) < 0.97 * large else "large"


def expected_record(r, depth, comb_layers, nfe, dim_out_mult16=True):
    """What the recording wrappers of the GPU file see over ONE pass (prepare + nfe evaluations) on route r, for a network of `depth`
    layers whose layers `comb_layers` start with a skip combiner (never layer 0): counts of ops.gemm calls by the type of a_split
    (none / plain pair / SplitIL) and by norm= / c_rowsq= / a_row_scale=, of the two attentions, of stand-alone norms, of factor-per-row
    launches and of split-K scratch hand-overs (ops._splitk_workspace: every pre-split GEMM without RoPE up to 2048 rows)."""
    L, C = depth, len(comb_layers)
    assert 0 not in comb_layers
    follows = sum(1 for i in range(L) if i + 1 < L and (i + 1) not in comb_layers)      # ff2 outputs the NEXT layer's attention norm reads
    rec = dict(gemm_plain=0, gemm_pair=0, gemm_il=0, gemm_norm=0, gemm_rowsq=0, gemm_row_scale=0, attention=0, attention_f16x3=0,
               adarmsnorm=0, rownorm_scale=0, scratch=0)
    split_gemms = 4 * L + C + 1                                   # per evaluation: to_qkv, to_out, ff1, ff2 per layer, the combiners, to_pred
    rec["gemm_plain"] = 1 + nfe * (1 if r.split_io else split_gemms + 1)      # to_embed's step-invariant columns once, its x columns per evaluation
    if not r.split_io:
        rec["attention"], rec["adarmsnorm"] = nfe * L, nfe * (2 * L + 1)
        return rec
    rec["gemm_il" if r.interleaved else "gemm_pair"] = nfe * split_gemms
    rec["attention_f16x3"] = nfe * L
    if r.splitk_scratch:
        rec["scratch"] = nfe * (split_gemms - L)                  # (to_qkv carries RoPE)
    if r.deferred:
        producers = C + L + follows                               # combiners, to_out, and ff2 where the next layer has no combiner
        rec["gemm_rowsq"] = rec["rownorm_scale"] = nfe * producers
        rec["gemm_row_scale"] = nfe * (2 * L - 1)                 # ff1 of every layer, to_qkv of every layer but the first
        rec["adarmsnorm"] = nfe * 2                               # the first attention norm and the final norm
    elif r.fuse_norm:
        rec["gemm_norm"] = nfe * (C + L + follows + 1)            # combiners, to_out, ff2 before a combiner-less layer, ff2 of the last layer
        rec["adarmsnorm"] = nfe * 1                               # the first layer's attention norm
    else:
        rec["adarmsnorm"] = nfe * (2 * L + 1)
    return rec
