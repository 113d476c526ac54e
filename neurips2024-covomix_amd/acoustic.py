"""VoMix / VoSingle vector field and ODE sampler on the MI355X kernels.

Host-side mirror of the reference classes on this path (paths relative to /root/reference):
  CoVoMix.forward / forward_with_cond_scale      covomix/covomix_model/acoustic.py:414-521
  Transformer / Attention / AdaptiveRMSNorm       acoustic.py:165-318
  ConditionalFlowMatcherWrapper.sample            acoustic.py:597-688   (torchdiffeq midpoint, :586-591)

MI355X-first restructuring (exact in real arithmetic; only fp32 rounding order changes):
  * both CFG branches run as ONE batch of 2B rows (the reference runs 2 sequential forwards);
  * the adaptive-norm projections depend only on t: all to_gamma/to_beta(time_emb) rows for the
    NFE time points are produced by two GEMMs per call instead of 32 GEMVs per forward (the
    reference re-reads 537 MB of weights per forward for them);
  * to_embed is linear in cat(x, phoneme_emb, cond): the 2208 step-invariant input columns are
    multiplied once per call, only the 80 x-columns every step;
  * RoPE is an epilogue of the to_qkv GEMM, attention never materialises T x T scores, GELU /
    bias / residual / skip-concat are GEMM epilogues or a K-split.
Python here only sequences kernel launches on torch's current stream and owns device buffers.
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass, field
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple, Union

import math
import os

import torch

from . import ops


def _dims_from_state(sd: Dict[str, torch.Tensor]) -> dict:
    dim, e_in = sd["to_embed.weight"].shape
    dim_cond = sd["null_cond"].shape[0]
    dim_emb = sd["to_phoneme_emb.weight"].shape[1]
    depth = 0
    while f"transformer.layers.{depth}.2.to_qkv.weight" in sd:
        depth += 1
    inner = sd["transformer.layers.0.2.to_qkv.weight"].shape[0] // 3
    dim_out = sd["to_pred.weight"].shape[0]
    streams = (e_in - dim_out - dim_cond) // dim_emb
    if dim_out + streams * dim_emb + dim_cond != e_in or inner % 64 != 0:
        raise ValueError("unsupported CoVoMix checkpoint geometry")
    return dict(dim=dim, e_in=e_in, dim_cond=dim_cond, dim_emb=dim_emb, depth=depth, heads=inner // 64,
                dim_head=64, dim_out=dim_out, streams=streams,
                null_id=sd["to_phoneme_emb.weight"].shape[0] - 1,
                time_hidden=sd["sinu_pos_emb.1.weight"].shape[0])


# ---------------------------------------------------------------------- which kernels a solve runs: a function of its row count
SPLIT_IO_ABOVE_ROWS = 64         # up to here the fp32 kernels; above, activations that only feed GEMMs live as split pairs
FUSE_NORM_BELOW_ROWS = 2048      # below: every norm rides in the GEMM that produces its input (the split-K path normalises inside its reduction)
LARGE_KERNEL_MIN_ROWS = 2048     # the deferred-norm forms exist in the large-problem GEMM only, which takes no fewer rows
GRAPH_MAX_ROWS = 8192            # default of CVX_GRAPH_MAX_ROWS: larger batches are GPU-bound and stay eager


@dataclass(frozen=True)
class Route:
    """What route() decided for one network evaluation of M rows; every consumer reads this record."""
    split_io: bool                   # the split pipe: (fp16 hi, lo) activations, f16x3 / f16 kernels on every consumer GEMM
    interleaved: bool                # GEMM A operands as ops.SplitIL (needs interleaved weights: f16x3, dim % 32 == 0)
    fuse_norm: bool                  # to_out / ff2 / combiner calls carry norm=
    splitk_scratch: bool             # ops.gemm hands its split-K scratch over (its own rule: SPLITK_SCRATCH_MAX_ROWS)
    deferred: bool                   # pair-only residual stream, norms deferred into the GEMMs (_layers_pair_stream)
    graph: bool                      # the solve is captured once per shape and replayed
    ragged_capacity: Optional[int]   # rows of a ragged batch's workspace (None: equal-length batch)


def route(M: int, dim: int, precision: str, ragged_rows: Optional[int] = None) -> Route:
    """The route of an evaluation of M rows (B T, doubled under guidance; ragged_rows = M for a packed ragged batch).  Pure: no tensor,
    no device; the environment and VectorField.DEFER_MIN_ROWS are read now."""
    env = os.environ.get
    # split activations need K % 32 == 0 on every consumer GEMM; the single-term kernel of 'f16' consumes 64 k per stage
    split_io = precision != "fp32" and M > SPLIT_IO_ABOVE_ROWS and dim % (64 if precision == "f16" else 32) == 0
    interleaved = split_io and precision == "f16x3" and M >= ops.il_min_rows() and dim >= 512
    deferred = (interleaved and M >= max(VectorField.DEFER_MIN_ROWS, LARGE_KERNEL_MIN_ROWS) and dim % 64 == 0 and dim <= 4096
                and env("CVX_DEFER_NORM", "1") == "1")
    graph = ragged_rows is None and env("CVX_GRAPH", "1") != "0" and M <= int(env("CVX_GRAPH_MAX_ROWS", GRAPH_MAX_ROWS))
    q = VectorField.RAGGED_ROW_QUANTUM
    return Route(split_io, interleaved, split_io and M < FUSE_NORM_BELOW_ROWS, split_io and M <= ops.SPLITK_SCRATCH_MAX_ROWS, deferred,
                 graph, None if ragged_rows is None else (ragged_rows + q - 1) // q * q)


def route_seq_times(M: int, dim: int, precision: str, ragged_rows: Optional[int] = None) -> Route:
    """The route of ONE evaluation with a time per sequence (VectorField.evaluate_seq_times): route()'s record with the three forms off
    that need one gamma / beta row for all rows (fuse_norm: the fused-norm GEMMs take one row), per-time weight copies (deferred: gamma(t)
    is baked into them) or a replay that would pay for itself (graph: one evaluation is launched once).  Pure, like route()."""
    return dataclasses.replace(route(M, dim, precision, ragged_rows), fuse_norm=False, deferred=False, graph=False)


class _Linear(NamedTuple):
    """One linear of the network: fp32 weight, bias (or None), its load-time (hi, lo, 1/scale) split and the interleaved copy of that."""
    w: torch.Tensor
    bias: Optional[torch.Tensor]
    split: Optional[tuple]
    il: Optional[tuple]
    plain: Optional[tuple]           # the w_split of a call without split I/O: none under 'f16' (VectorField.__init__)


class _Layer(NamedTuple):
    comb: Optional[_Linear]          # the skip combiner of the later layers (None: this layer pushes a skip)
    qkv: _Linear
    out: _Linear
    ff1: _Linear
    ff2: _Linear


class VectorField:
    """Device-resident weights of one CoVoMix network + the launch sequence of one evaluation."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], device: torch.device, precision: str = "f16x3"):
        """precision: 'f16x3' (default) runs the transformer GEMMs on the fp16 matrix pipe with every operand split
        into (hi, lo) fp16 halves and three MFMA products - fp32-class accuracy (kernel error 5.8e-7 vs 5.1e-7 for
        fp32 MFMA, tests/test_kernels_gpu.py) at 2x the rate; 'fp32' uses v_mfma_f32_32x32x2_f32 everywhere;
        'f16' (opt-in) keeps only the hi halves: plain fp16 GEMM / attention operands with fp32 accumulation,
        softmax, norms and residual stream - inside the 1e-3 rel-L2 budget of BASELINE.json, not fp32-class."""
        if precision not in ("f16x3", "fp32", "f16"):
            raise ValueError(f"precision must be 'f16x3', 'f16' or 'fp32', got {precision!r}")
        self.precision = precision
        if torch.device(device).type == "cuda":
            with torch.cuda.device(device):
                ops.saturation_reset()      # (allocates the device's saturation flag now, outside any stream capture)
        sd = {k: v.detach().to(device=device, dtype=torch.float32).contiguous() for k, v in state_dict.items()}
        self.device = device
        self.d = d = _dims_from_state(sd)
        if sd["conv_embed.dw_conv1d.0.weight"].shape[-1] != 31:
            raise ValueError("only conv_pos_embed_kernel_size == 31 is supported (reference default)")
        self.sd = sd
        # adaptive-norm projection weights packed [2*n_norms*dim, time_hidden]: (gamma, beta) per norm
        names = [f"transformer.layers.{i}.{n}.{nm}" for i in range(d["depth"]) for n in (1, 3) for nm in ("to_gamma", "to_beta")]
        self.ada_w = torch.cat([sd[k + ".weight"] for k in names], dim=0).contiguous()
        self.ada_b = torch.cat([sd[k + ".bias"] for k in names], dim=0).contiguous()
        for k in names:                      # the unpacked copies are never read again
            del sd[k + ".weight"], sd[k + ".bias"]
        self.dw_w = sd["conv_embed.dw_conv1d.0.weight"].reshape(d["dim"], 31).contiguous()
        inv_freq = sd.get("transformer.rotary_emb.inv_freq")
        if inv_freq is None:
            inv_freq = 1.0 / (10000 ** (torch.arange(0, 64, 2, device=device).float() / 64))
        self.inv_freq = inv_freq
        self._ws: Dict[tuple, dict] = {}
        self._dn_bufs: Dict[tuple, dict] = {}          # deferred norm: W diag(gamma(t)) pairs per (n, depth, solver grid)
        self._time_cache: Dict[tuple, dict] = {}       # solver grid (nfe, method) -> everything that depends on the evaluation times only
        def linear(name: str) -> Optional[_Linear]:
            """The record of one linear (None: the checkpoint has none of that name): load-time packing of the big GEMM weights as
            split (fp16 hi, fp16 lo, 1/scale) copies, and for the medium- and large-problem kernels an interleaved copy of those
            ([hi 32 | lo 32] per K-step: whole cache lines for the DMA)."""
            w, bias = sd.get(name + ".weight"), sd.get(name + ".bias")
            if w is None:
                return None
            sp = ops.split_f16(w, with_lo=(precision == "f16x3")) if precision != "fp32" and w.shape[1] % 32 == 0 else None
            il = ops.split_f16_interleaved(sp) if precision == "f16x3" and sp is not None and (w.shape[0] >= 512 or name == "to_pred") else None
            # a call without split I/O passes no w_split under 'f16': the single-term kernel needs a pre-split A, and ops.gemm would
            # otherwise take the f16x3 branch above SPLIT_IO_ABOVE_ROWS rows - the fp32 kernels run instead
            return _Linear(w, bias, sp, il, None if precision == "f16" else sp)
        self.layers = [_Layer(*(linear(f"transformer.layers.{i}.{n}") for n in ("0", "2.to_qkv", "2.to_out", "4.0", "4.2")))
                       for i in range(d["depth"])]
        self.to_pred = linear("to_pred")
        self.final_gamma = sd["transformer.final_norm.gamma"]
        self.embed_x = sd["to_embed.weight"][:, : d["dim_out"]]          # the x columns of to_embed: every evaluation
        # the step-invariant columns of to_embed (phoneme embeddings | conditioning mel: one [2BT, 2208] x [2208, 1024] product
        # per solve) - 0.74 ms on the fp32 pipe at the bench shape
        # the adaptive-norm table GEMM - [n evaluation times, dim] x the packed [4 depth dim, dim] matrix: pure weight
        # streaming at 32 rows - 1.35 ms per solve on the fp32 kernel inside the model (cold weights), 0.76 ms here
        # (rocprofv3).  Neither is close to the 134 MB / HBM rate = 30 us: DESIGN 4.4
        # (solves of more than 32 evaluation times build self.ada_split on demand: _time_tables)
        self.ada_split = None
        w_rest = sd["to_embed.weight"][:, d["dim_out"]:]
        pack = precision == "f16x3" and w_rest.shape[1] % 32 == 0
        w_rest = w_rest.contiguous() if pack else w_rest
        sp = ops.split_f16(w_rest) if pack else None
        self.embed_rest = _Linear(w_rest, sd["to_embed.bias"], sp, None, sp)
        self._init_gain_model()

    # ------------------------------------------------------------------ activation pre-scales (scale-free split pairs)
    # An (fp16 hi, fp16 lo) pair has full (22-bit) precision only while |x| is inside [2^-3, 2^16): below, `lo` falls into
    # fp16's subnormals (absolute floor 2^-25), above, `hi` saturates.  Every split ACTIVATION tensor is therefore written
    # times a power of two that puts its expected RMS at 2^4 (full precision for elements from 2^-7 to 2^12 times the RMS),
    # and the consuming kernel divides it out of its fp32 accumulators - exactly what load-time packing does for the
    # weights.  The powers come from a GAIN MODEL, not from the data: RMS of an AdaRMSNorm output = sqrt(mean(gamma^2) +
    # mean(beta^2)) of that evaluation time's table row (exact for RMS-normalised input), RMS after a Linear = input RMS
    # x ||W||_F / sqrt(N).  They are computed on the device by prepare() (no host round trip: the solve stays
    # graph-capturable), depend on the weights and the evaluation times only - never on the utterance - and sit in one
    # small tensor the kernels read through DEVICE pointers (cvx_gemm_split_io.a_scale_dev, ...).
    WORKSPACE_SHAPES = 4
    N_KINDS = 6          # per (evaluation, layer): normed->qkv, q|k, v, attention out, normed->ff1, ff hidden
    TARGET_RMS = 16.0

    def _init_gain_model(self) -> None:
        d, sd = self.d, self.sd
        inner = d["heads"] * 64

        def fro(w, rows=None):              # ||W||_F / sqrt(N): RMS gain of y = W x for x with unit per-element RMS
            w = w if rows is None else w[rows[0]:rows[1]]
            return float(w.double().square().sum().sqrt() / (w.shape[0] ** 0.5))
        g = dict(qk=[], v=[], o=[], f1=[], b1=[], f2=[], comb=[])
        for ly in self.layers:
            g["qk"].append(fro(ly.qkv.w, (0, 2 * inner))); g["v"].append(fro(ly.qkv.w, (2 * inner, 3 * inner)))
            g["o"].append(fro(ly.out.w))
            g["f1"].append(fro(ly.ff1.w)); g["b1"].append(float(ly.ff1.bias.double().square().mean()))
            g["f2"].append(fro(ly.ff2.w))
            g["comb"].append(fro(ly.comb.w) if ly.comb is not None else 0.0)
        dev = self.device
        self.gain = {k: torch.tensor(v, dtype=torch.float32, device=dev) for k, v in g.items()}
        # embedding output: x columns (x ~ N(0,1) at t = 0, O(1) later), phoneme-embedding columns (RMS of the table), cond
        # columns (log-mel prompt frames, |.| of a few units: taken as RMS 4), bias
        we = sd["to_embed.weight"].double()
        n_x, n_e = d["dim_out"], d["streams"] * d["dim_emb"]
        emb_ms = float(sd["to_phoneme_emb.weight"].double().square().mean())
        ms = lambda w: float(w.square().sum() / w.shape[0])
        self.embed_ms = (ms(we[:, :n_x]) + emb_ms * ms(we[:, n_x:n_x + n_e]) + 16.0 * ms(we[:, n_x + n_e:])
                         + float(sd["to_embed.bias"].double().square().mean()))
        gf = float(self.final_gamma.double().square().mean().sqrt())
        self.pred_scale = torch.tensor([self._pow2(self.TARGET_RMS / max(gf, 1e-30))], dtype=torch.float32, device=dev)

    @staticmethod
    def _pow2(x: float) -> float:
        return 2.0 ** max(-40, min(40, round(math.log2(x)))) if x > 0 and math.isfinite(x) else 1.0

    def _activation_scales(self, table: torch.Tensor) -> tuple:
        """(S [n_eval, depth, N_KINDS], H [1], HS [depth, 4]) power-of-two pre-scales from the gain model; device tensors, no host sync."""
        d, gn = self.d, self.gain
        n, L, dim = table.shape[0], d["depth"], d["dim"]
        tab = table.view(n, L, 4, dim)
        ms = tab.square().mean(dim=-1)                                  # [n, L, 4]: mean(gamma_a^2), mean(beta_a^2), gamma_f, beta_f
        rn_a = (ms[..., 0] + ms[..., 1]).sqrt()
        rn_f = (ms[..., 2] + ms[..., 3]).sqrt()
        qk, v = rn_a * gn["qk"], rn_a * gn["v"]
        att = v * 0.25                                                  # softmax averages values: between v_rms / sqrt(T) and v_rms
        ff = ((rn_f * gn["f1"]).square() + gn["b1"]).sqrt() * 0.5       # GELU(z) ~ z / 2 .. 0.6 z
        rms = torch.stack([rn_a, qk, v, att, rn_f, ff], dim=-1)         # [n, L, 6]
        tiny = torch.finfo(torch.float32).tiny
        S = torch.exp2(torch.round(torch.log2(self.TARGET_RMS / rms.clamp_min(tiny))).clamp(-40, 40)).contiguous()
        # residual stream (split twins of h feed the skip combiners; all of them share ONE scale because a combiner reads two
        # of them as the halves of its K range): embedding output, then every block adds its attention and FF output
        h2 = torch.full((), self.embed_ms * 2.25, dtype=torch.float32, device=table.device)   # x + GELU(conv(x)): up to 1.5 x
        hmax = h2
        att_o = (att * gn["o"]).square().amax(dim=0)                    # [L]: largest over the evaluation times
        ff_o = (ff * gn["f2"]).square().amax(dim=0)
        skips = []
        stages = []                          # mean squares of the stream per layer: at its input, behind its skip combiner, behind to_out, behind ff2
        for i in range(L):
            h_in = h2
            if self.layers[i].comb is not None:
                h2 = (h2 + skips.pop()) * gn["comb"][i].square()
            else:
                skips.append(h2)
            h_c = h2
            h_a = h2 + att_o[i]
            h2 = h_a + ff_o[i]
            stages.append(torch.stack([h_in, h_c, h_a, h2]))
            hmax = torch.maximum(hmax, h2)
        H = torch.exp2(torch.round(torch.log2(self.TARGET_RMS / hmax.sqrt().clamp_min(tiny))).clamp(-40, 40)).reshape(1).contiguous()
        # the pair-only residual stream of the deferred-norm path (section 4.1d) carries ONE pre-scale PER STAGE: the stream IS those
        # pairs there, and a stage far below the largest one would sit under the full-precision window of a shared scale
        HS = torch.exp2(torch.round(torch.log2(self.TARGET_RMS / torch.stack(stages).sqrt().clamp_min(tiny))).clamp(-40, 40)).contiguous()
        return S, H, HS

    # ------------------------------------------------------------------ workspace
    RAGGED_ROW_QUANTUM = 1024       # ragged batches: workspaces are sized in steps of this many rows and shared by every
                                    # batch composition that fits (a directory never repeats a composition)

    def route(self, M: int, ragged_rows: Optional[int] = None) -> Route:
        return route(M, self.d["dim"], self.precision, ragged_rows)

    def _workspace(self, Bt: int, T: int, ragged_rows: int = 0, r: Optional[Route] = None) -> dict:
        """Buffers of one batch shape.  Equal-length batch: Bt sequences of T frames.  Ragged batch (ragged_rows = M > 0):
        capacity rounded up to RAGGED_ROW_QUANTUM rows, ONE V^T row set per head over all packed rows, no RoPE table (it
        depends on the composition: prepare() builds it per call); callers use a row-cut view (_ws_cut)."""
        d, dev = self.d, self.device
        r = r or self.route(ragged_rows or Bt * T, ragged_rows or None)        # (prepare() passes the route it made for the batch)
        M = r.ragged_capacity or Bt * T
        key = ("ragged", M, ragged_rows >= ops.il_min_rows()) if ragged_rows else (Bt, T)  # (the pair layout depends on the real row count)
        ws = self._ws.pop(key, None)
        if ws is not None:
            self._ws[key] = ws                                   # most recently used last
            return ws
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        ws = dict(
            h=[f(M, d["dim"]) for _ in range(d["depth"] // 2 + 3)],
            normed=f(M, d["dim"]), qkv=f(M, 3 * d["heads"] * 64), att=f(M, d["heads"] * 64),
            ff=f(M, 4 * d["dim"]), base=f(M, d["dim"]), xin=f(M, d["dim_out"]), pred=f(M, d["dim_out"]),
            gathered=f(M, d["streams"] * d["dim_emb"] + d["dim_cond"]),
            rowsq=f(M, max(d["dim"] // 64, 1)), rs=f(M),           # deferred norm: row sums of squares per 64 columns, factor per row
        )
        if self.precision in ("f16x3", "f16"):      # activations that only feed GEMMs live as (fp16 hi, fp16 lo) pairs
            lo_too = self.precision == "f16x3"          # 'f16': (hi, None)
            h16 = lambda *s: (torch.empty(*s, dtype=torch.float16, device=dev),
                              torch.empty(*s, dtype=torch.float16, device=dev) if lo_too else None)
            # GEMM A operands: for the medium- and large-problem kernels (from ops.il_min_rows() rows, interleaved weights available)
            # as INTERLEAVED pairs ([hi 32 | lo 32] per K-step: whole cache lines for the DMA), otherwise as two separate fp16 tensors
            a16 = (lambda rows, cols: ops.SplitIL(rows, cols, dev)) if r.interleaved else h16
            ws["normed16"], ws["att16"], ws["ff16"] = a16(M, d["dim"]), a16(M, d["heads"] * 64), a16(M, 4 * d["dim"])
            # final norm -> to_pred (N = 80): the medium-problem kernel takes it (interleaved pair; K slices below 2048 rows)
            ws["pred16"] = a16(M, d["dim"]) if (a16 is not h16 and d["dim_out"] % 16 == 0) else h16(M, d["dim"])
            ws["qk16"] = h16(M, 2 * d["heads"] * 64)
            ws["h16"] = [a16(M, d["dim"]) for _ in ws["h"]]      # split twins of the residual-stream buffers (skip GEMMs)
            # V^T rows, zero (always finite) beyond the last frame: read by the last key tile with weight 0
            vt_rows, Tp = (d["heads"] * 64, M) if ragged_rows else (Bt * d["heads"] * 64, ((T + 31) // 32) * 32)
            ws["vt16"] = (torch.zeros(vt_rows, Tp, dtype=torch.float16, device=dev),
                          torch.zeros(vt_rows, Tp, dtype=torch.float16, device=dev) if lo_too else None)
        if not ragged_rows:
            ws["rope"] = self._rope_tables(torch.arange(T, device=dev, dtype=torch.float32))
        while len(self._ws) >= self.WORKSPACE_SHAPES:          # keep the most recent shapes resident (a directory of
            self._ws.pop(next(iter(self._ws)))                  # utterances alternates between a few lengths; ~0.4 GB per 1000 rows)
        self._ws[key] = ws
        return ws

    def stage_buffers(self, ctx: dict, n: int) -> List[torch.Tensor]:
        """n (<= 3) buffers [M1, dim_out] for the stored stages of a Runge-Kutta step (FlowMatchingSampler._integrate_stages).  They
        belong to the batch shape's workspace and are made when a solver first asks for them: midpoint and Euler never do."""
        ws, M1 = ctx["ws"], ctx["M1"]
        whole = ws.get("whole", ws)                             # ragged batch: the capacity-sized workspace behind the row views
        rows = whole["xin"].shape[0] if whole is not ws else M1
        ks = whole.setdefault("rk_k", [])
        assert 0 <= n <= 3
        while len(ks) < n:
            ks.append(torch.empty(rows, self.d["dim_out"], dtype=torch.float32, device=self.device))
        return [k[:M1] for k in ks[:n]]

    def _rope_tables(self, pos: torch.Tensor) -> tuple:
        """(cos, sin) [len(pos), 32] of the half-split rotary embedding at the given positions (acoustic.py:120-137)."""
        ang = pos[:, None] * self.inv_freq[None, :]
        return ang.cos().contiguous(), ang.sin().contiguous()

    # ------------------------------------------------------------------ per-call setup
    def prepare(self, phoneme_ids: torch.Tensor, cond: torch.Tensor, times: torch.Tensor, use_null: bool,
                lengths: Optional[List[int]] = None, times_key=None, seq_times: bool = False) -> dict:
        """Everything that does not depend on the ODE state x:
        time MLP + adaptive-norm tables for every evaluation time (_time_tables: computed once per solver grid `times_key` and
        model), and the step-invariant part of to_embed.
        lengths: ragged batch - phoneme_ids [M1(, S)] and cond [M1, C] hold the utterances back to back (M1 = sum(lengths));
        the null-branch rows repeat the same sequence structure behind them.
        seq_times: `times` holds one time PER UTTERANCE of a ragged batch for ONE evaluation (evaluate(ctx, 0)) instead of one per
        evaluation: the route is route_seq_times', the tables are built for these times and not cached, ctx["seq"] (the batch's
        Ragged) makes the layer walkers take every adaptive norm's gamma / beta row per sequence (_norm), and the activation
        pre-scales - one scalar per (layer, kind) for the whole evaluation - are the smallest over the utterances' times: the
        largest modelled RMS (H takes the maximum already)."""
        d, sd = self.d, self.sd
        rg = None
        if lengths is not None:
            B, T, M1 = len(lengths), None, int(sum(lengths))
            assert cond.ndim == 2 and cond.shape[0] == M1 and phoneme_ids.shape[0] == M1
            rg = ops.Ragged(lengths, self.device, repeat=2 if use_null else 1)
        else:
            B, T, _ = cond.shape
            M1 = B * T
        Bt, M = (2 * B, 2 * M1) if use_null else (B, M1)
        r = self.route(M, ragged_rows=None if rg is None else M)   # from the real row count: read here, by _workspace and by evaluate()
        if seq_times:
            assert rg is not None and times.numel() == B, "a time per utterance goes with a packed batch and one time for each"
            r = route_seq_times(M, d["dim"], self.precision, M)
        if rg is not None:
            full = self._workspace(0, 0, M, r)
            ws = self._ws_cut(full, 0, M, vt=None)               # row views of the capacity-sized buffers; V^T stays whole
            ws["whole"] = full
            ws["rope"] = self._rope_tables(rg.positions())       # per-ROW tables: the to_qkv epilogue then runs with rope_T = M
        else:
            ws = self._workspace(Bt, T, r=r)
        tt = self._time_tables(times, None if seq_times else times_key)
        if seq_times:
            tt = dict(tt, table=tt["table"].repeat(2, 1) if use_null else tt["table"])      # the null-branch sequences repeat the times
            if "S" in tt:
                S = tt["S"].amin(dim=0, keepdim=True).contiguous()
                p0, K = S.data_ptr(), self.N_KINDS
                tt.update(S=S, sp=[[[p0 + 4 * (i * K + k) for k in range(K)] for i in range(d["depth"])]])
        # step-invariant to_embed columns: rows [0, M1) conditional, rows [M1, 2*M1) null branch
        g = ws["gathered"]
        ids = phoneme_ids.to(torch.int64).contiguous()
        ops.embed_gather(ids, d["streams"], sd["to_phoneme_emb.weight"], cond.contiguous(), None, d["dim_cond"],
                         d["null_id"], g[:M1], M1)
        if use_null:
            ops.embed_gather(None, d["streams"], sd["to_phoneme_emb.weight"], None, sd["null_cond"], d["dim_cond"],
                             d["null_id"], g[M1:], M1)
        rest = self.embed_rest
        ops.gemm(g, rest.w, ws["base"], bias=rest.bias, w_split=rest.split)
        ctx = dict(ws=ws, table=tt["table"], B=B, T=T, Bt=Bt, M1=M1, use_null=use_null, M=M, ragged=rg, route=r, seq=rg if seq_times else None)
        if "S" in tt:
            ctx["scales"], ctx["h_scale"] = tt["S"], tt["H"]                   # keep the tensors alive as long as the pointers
            ctx["sp"], ctx["hp"] = tt["sp"], tt["H"].data_ptr()
            if r.deferred:
                if tt["dn"] is None:
                    # built by split-pair kernels (split_f16_colscale_il): cached only when the build itself stayed inside the window
                    # (_tables_clean) - a clamped table must not outlive the call that is flagged for it
                    clean0 = self._flag_clear()
                    dn = self._deferred_norm_tables(tt["table"], tt["HS"], times_key)
                    if tt.get("cached") and clean0 and self._flag_clear():
                        tt["dn"], tt["dn_ready"] = dn, self._ready_event()
                    ctx["dn"] = dn
                else:
                    self._wait(tt["dn_ready"])                                  # (built on another stream, maybe)
                    ctx["dn"] = tt["dn"]
        return ctx

    @staticmethod
    def _flag_clear():
        """Is the current stream's sticky saturation flag clear right now (one stream synchronisation)?  None when nothing can be
        said: inside a stream capture, or with the checks switched off (CVX_SAT_CHECK=0)."""
        if torch.cuda.is_current_stream_capturing() or os.environ.get("CVX_SAT_CHECK", "1") != "1":
            return None
        return ops.saturation_query(reset=False) == 0

    @staticmethod
    def _wait(ev) -> None:
        """the current stream waits for tables another stream may have built (not inside a capture: a capture starts after the
        capturing call's own eager run and a stream synchronisation - everything cached is complete by then)"""
        if not torch.cuda.is_current_stream_capturing():
            torch.cuda.current_stream().wait_event(ev)

    @staticmethod
    def _ready_event():
        ev = torch.cuda.Event()
        ev.record()
        return ev

    # ------------------------------------------------------------------ everything that depends on the evaluation times only
    TIME_CACHE = 2          # evaluation-time grids whose tables stay resident (each holds 0.22 GB per evaluation time once a batch deferred its norms)

    def _time_tables(self, times: torch.Tensor, key) -> dict:
        """Time MLP + adaptive-norm table for every evaluation time, the activation pre-scales of the gain model and (filled in by
        prepare() when a batch defers its norms) the deferred-norm weight tables.  All of it is a function of the CHECKPOINT and the
        evaluation times - gamma / beta are functions of the time embedding alone (reference acoustic.py:198-204) - never of the
        utterance, so a solver grid `key` = (nfe, method) computes it once per VectorField (= per set of weights: CoVoMixModel builds a
        new field when its weights change) and every later call reuses it: 15 split_colscale_il + 34 weight-streaming launches and
        ~30 torch launches less per call.  key = None: not cached.  At most TIME_CACHE grids stay resident; evicting one also
        drops the captured graphs (they hold addresses of its tables)."""
        d, sd = self.d, self.sd
        if key is not None and key in self._time_cache:
            ent = self._time_cache.pop(key)
            self._time_cache[key] = ent                                        # most recently used last
            self._wait(ent["ready"])                                           # (the tables may have been built on another stream)
            return ent
        # The tables are built by split-precision kernels that can raise the sticky saturation flag (split_act_f16(temb), the f16x3
        # GEMM of the table above 32 rows, the activation scales).  A call that builds them and is flagged is re-run in fp32 - but a
        # CACHED clamped table would be reused by later calls under a clean flag: silently wrong.  So an entry is cached only when
        # its build provably stayed inside the window: flag clear before AND after (two stream synchronisations per (model, grid)).
        clean0 = self._flag_clear() if key is not None else None
        n = times.numel()
        four = torch.empty(n, d["dim"], dtype=torch.float32, device=self.device)
        ops.time_fourier(times, sd["sinu_pos_emb.0.weights"], four)
        temb = torch.empty(n, d["time_hidden"], dtype=torch.float32, device=self.device)
        # products with n <= 32 rows are weight streaming: cvx_gemm_skinny_f32 (the table, 537 MB of weights: 1.35 ms on the tiled fp32
        # kernel, 0.79 on the split-precision one, 0.25 here)
        skinny = lambda w: n <= 32 and w.shape[1] % 8 == 0
        if skinny(sd["sinu_pos_emb.1.weight"]):
            ops.gemm_skinny(four, sd["sinu_pos_emb.1.weight"], temb, bias=sd["sinu_pos_emb.1.bias"], act=ops.ACT_SILU)
        else:
            ops.gemm(four, sd["sinu_pos_emb.1.weight"], temb, bias=sd["sinu_pos_emb.1.bias"], act=ops.ACT_SILU)
        table = torch.empty(n, self.ada_w.shape[0], dtype=torch.float32, device=self.device)
        if skinny(self.ada_w):
            ops.gemm_skinny(temb, self.ada_w, table, bias=self.ada_b)
        elif self.precision == "f16x3" and self.ada_w.shape[1] % 32 == 0:
            self.ada_split = self.ada_split or ops.split_f16(self.ada_w)
            ops.gemm(temb, self.ada_w, table, bias=self.ada_b, w_split=self.ada_split, a_split=ops.split_act_f16(temb))
        else:
            ops.gemm(temb, self.ada_w, table, bias=self.ada_b)
        ent = dict(table=table, dn=None)
        if self.precision in ("f16x3", "f16"):
            S, H, HS = self._activation_scales(table)
            p0, K = S.data_ptr(), self.N_KINDS
            ent.update(S=S, H=H, HS=HS, sp=[[[p0 + 4 * ((e * d["depth"] + i) * K + k) for k in range(K)] for i in range(d["depth"])] for e in range(n)])
        ent["ready"] = self._ready_event()
        if key is not None and clean0 and self._flag_clear():     # (None inside a capture: tables made there belong to that graph's pool)
            ent["cached"] = True
            while len(self._time_cache) >= self.TIME_CACHE:
                old = next(iter(self._time_cache))
                del self._time_cache[old]
                self._dn_bufs = {k: v for k, v in self._dn_bufs.items() if k[2] != old}
                self.__dict__.pop("_graphs", None)
            self._time_cache[key] = ent
        return ent

    # ------------------------------------------------------------------ deferred AdaptiveRMSNorm (large batches)
    DEFER_MIN_ROWS = int(os.environ.get("CVX_DEFER_NORM_ROWS", "8192"))      # (route() floors it at LARGE_KERNEL_MIN_ROWS)
    # The row count is the whole rule: round 4 kept batches whose 256-row rounds came out part-empty - 18,000 / 20,480 rows - off this path;
    # with the large-problem kernel's 192-row tiles, round 5, the path wins at every size from 8192 rows: tools/archive/defer_rows_bench.py,
    # 20,480 rows 448.7 vs 470.1 ms, 18,000 rows 404.2 vs 417.5, 9,300 rows 232.8 vs 242.1

    def _deferred_norm_tables(self, table: torch.Tensor, HS: torch.Tensor, times_key) -> dict:
        """Per (evaluation time, layer): W diag(gamma) for to_qkv (layers 1..) and ff1 as interleaved split pairs, beta W^T as their
        bias (ff1: b1 + beta_ff W1^T), and the power of two that keeps |gamma| <= 1 inside the weight pair (divided out on the
        accumulators through the consumer's a_scale).  A function of the weights and the evaluation times: built once per solver
        grid (_time_tables)."""
        d = self.d
        n, L, dim = table.shape[0], d["depth"], d["dim"]
        tab = table.view(n, L, 4, dim)
        tiny = torch.finfo(torch.float32).tiny
        gmax = tab[:, :, 0::2, :].abs().amax(dim=-1)                                     # [n, L, 2]: max |gamma_attn|, max |gamma_ff|
        gs = torch.exp2(-torch.ceil(torch.log2(gmax.clamp_min(tiny))).clamp(-40, 40)).contiguous()
        # HS [L, 4]: stream pre-scale at a layer's input / behind its combiner / to_out / ff2
        AS = (gs * HS[None, :, 1:3]).contiguous()                                        # pre-scale of the consumers' A pairs (stage scale) times the weights' gs

        def beta_w(beta_rows: torch.Tensor, w: torch.Tensor, bias) -> torch.Tensor:
            out = torch.empty(n, w.shape[0], dtype=torch.float32, device=self.device)
            for r0 in range(0, n, 32):                                                   # weight streaming: 32 rows at a time on the skinny kernel
                r1 = min(n, r0 + 32)
                ops.gemm_skinny(beta_rows[r0:r1], w, out[r0:r1], bias=bias)
            return out
        key = (n, L, times_key)
        bufs = self._dn_bufs.get(key)
        if bufs is None:                     # (0.22 GB per evaluation time; released with the grid's cache entry, _time_tables)
            mk = lambda N: torch.empty(n, N, 2 * dim, dtype=torch.float16, device=self.device)
            bufs = dict(wq=[None if i == 0 else mk(3 * d["heads"] * 64) for i in range(L)], w1=[mk(4 * dim) for _ in range(L)])
            self._dn_bufs[key] = bufs
        b1p, bq, wq, w1 = [], [], [], []
        for i, ly in enumerate(self.layers):
            b1p.append(beta_w(tab[:, i, 3, :], ly.ff1.w, ly.ff1.bias))
            inv1 = ly.ff1.il[1]
            ops.split_f16_colscale_il(ly.ff1.w, tab[:, i, 2, :], gs[:, i, 1], 1.0 / inv1, bufs["w1"][i])
            w1.append([(bufs["w1"][i][e], inv1) for e in range(n)])
            if i == 0:
                bq.append(None); wq.append(None)
                continue
            bq.append(beta_w(tab[:, i, 1, :], ly.qkv.w, None))
            invq = ly.qkv.il[1]
            ops.split_f16_colscale_il(ly.qkv.w, tab[:, i, 0, :], gs[:, i, 0], 1.0 / invq, bufs["wq"][i])
            wq.append([(bufs["wq"][i][e], invq) for e in range(n)])
        a0, h0 = AS.data_ptr(), HS.data_ptr()
        return dict(b1p=b1p, bq=bq, wq=wq, w1=w1, gs=gs, AS=AS, HS=HS, hsp=[[h0 + 4 * (4 * i + k) for k in range(4)] for i in range(L)],
                         asp=[[(a0 + 4 * ((e * L + i) * 2), a0 + 4 * ((e * L + i) * 2 + 1)) for i in range(L)] for e in range(n)])

    # ------------------------------------------------------------------ one evaluation (both CFG branches)
    @staticmethod
    def _ws_cut(ws: dict, r0: int, r1: int, vt) -> dict:
        """Views of every workspace buffer restricted to rows [r0, r1); vt = (lo, hi): the V^T rows that go with them
        (None: V^T is shared whole - ragged batches)."""

        def cut(v, lo=r0, hi=r1):
            if isinstance(v, ops.SplitIL):
                return v.rows_view(lo, hi)
            if isinstance(v, tuple):
                return tuple(None if t is None else t[lo:hi] for t in v)
            if isinstance(v, list):
                return [cut(t, lo, hi) for t in v]
            return v[lo:hi]
        out = {}
        for k, v in ws.items():
            if k == "rope":
                out[k] = v
            elif k == "vt16":
                out[k] = v if vt is None else cut(v, vt[0], vt[1])
            else:
                out[k] = cut(v)
        return out

    def evaluate(self, ctx: dict, step: int) -> torch.Tensor:
        """Run the network on ws['xin'] (rows: cond branch then null branch) at evaluation time #step.
        Returns ws['pred'] [Bt*T, dim_out].  The front runs here; the layers on the walker ctx['route'] names, then _head."""
        ws, r = ctx["ws"], ctx["route"]
        free: List[torch.Tensor] = list(ws["h"])
        h, h0 = free.pop(), free.pop()
        ops.gemm(ws["xin"], self.embed_x, h0, residual=ws["base"])
        ops.dwconv31_gelu_res(h0, self.dw_w, self.sd["conv_embed.dw_conv1d.0.bias"], h, ctx["Bt"], ctx["T"], ragged=ctx["ragged"])
        free.append(h0)
        if not r.split_io:
            return self._head(ctx, self._layers_fp32(ctx, step, h, free), False)
        # residual-stream tensors that later feed a skip combiner (as x or as the popped skip) also get a split
        # twin, so that GEMM takes both operands pre-split (all-DMA kernel) instead of splitting on the fly
        twin = {id(b): pr for b, pr in zip(ws["h"], ws["h16"])}
        tw = twin[id(h)]
        h0s = ctx["dn"]["hsp"][0][0] if r.deferred else ctx["hp"]      # (deferred-norm path: one pre-scale per stage of the stream)
        ops.split_act_f16(h, tw, scale=h0s) if isinstance(tw, ops.SplitIL) else ops.split_act_f16(h, *tw, scale=h0s)
        if r.deferred:
            return self._head(ctx, self._layers_pair_stream(ctx, step, h, twin, free), False)
        return self._head(ctx, *self._layers_split(ctx, step, h, twin, free, r.fuse_norm))

    def _norm_rows(self, ctx: dict, step: int) -> torch.Tensor:
        """The adaptive-norm rows of evaluation #step as [depth, 4, ...]: [dim] each - or, with a time per sequence (ctx["seq"]),
        [n sequences, dim] views of the [n, depth, 4, dim] table, a sequence's rows depth * 4 * dim floats apart."""
        d = self.d
        if ctx.get("seq") is None:
            return ctx["table"][step].view(d["depth"], 4, d["dim"])
        assert step == 0
        return ctx["table"].view(-1, d["depth"], 4, d["dim"]).permute(1, 2, 0, 3)

    @staticmethod
    def _norm(ctx: dict, h: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, out, **kw):
        """One adaptive norm of the layer walkers: one gamma / beta row for all rows, or one per sequence (ctx["seq"], _norm_rows)."""
        if ctx.get("seq") is None:
            return ops.adarmsnorm(h, gamma, beta, out, **kw)
        return ops.adarmsnorm_seq(h, gamma, beta, out, ctx["seq"], **kw)

    def xin_rows(self, lengths: Sequence[int], use_null: bool = False) -> torch.Tensor:
        """The conditional rows [sum(lengths), dim_out] of the input buffer evaluate_seq_times will run this batch on: a producer
        (ops.cfm_inputs) that writes them there saves the copy."""
        M1 = int(sum(lengths))
        M = 2 * M1 if use_null else M1
        return self._workspace(0, 0, M, route_seq_times(M, self.d["dim"], self.precision, M))["xin"][:M1]

    def evaluate_seq_times(self, phoneme_ids: torch.Tensor, cond: torch.Tensor, x: torch.Tensor, times: torch.Tensor, lengths: Sequence[int],
                           use_null: bool = False) -> torch.Tensor:
        """ONE evaluation of the network on a packed batch with a TIME PER UTTERANCE (what the flow-matching loss and the reference's
        sample_regression need, acoustic.py:768, :716): phoneme_ids [M1(, S)], cond [M1, C], x [M1, dim_out] hold the utterances back to
        back (an equal-length batch is a packed one), times fp32 [len(lengths)] on the device.  use_null: the null-conditioning branch
        runs behind the conditional rows at the same times.  Returns the workspace's pred [M1 or 2 M1, dim_out] (valid until the next
        call on this field).  Route: route_seq_times - stand-alone norms (ops.adarmsnorm_seq), never deferred, never captured."""
        lengths = [int(t) for t in lengths]
        if not 1 <= len(lengths) * (2 if use_null else 1) <= ops.SEQ_NORM_MAX_SEQS:
            raise ValueError(f"evaluate_seq_times: {len(lengths)} utterances{' and their null-branch twins' if use_null else ''} in one evaluation "
                             f"(1 ... {ops.SEQ_NORM_MAX_SEQS} sequences)")
        ctx = self.prepare(phoneme_ids, cond, times, use_null, lengths=lengths, seq_times=True)
        xin, M1 = ctx["ws"]["xin"], ctx["M1"]
        if x.data_ptr() != xin.data_ptr():
            xin[:M1].copy_(x.reshape(M1, -1))
        if use_null:
            xin[M1:].copy_(xin[:M1])
        return self.evaluate(ctx, 0)

    def _head(self, ctx: dict, h: torch.Tensor, normed_ahead: bool) -> torch.Tensor:
        """The final RMSNorm and to_pred.  normed_ahead: the last ff2 wrote the normed pair already (fuse_norm)."""
        ws = ctx["ws"]
        if not ctx["route"].split_io:
            ops.adarmsnorm(h, self.final_gamma, None, ws["normed"])
            return ops.gemm(ws["normed"], self.to_pred.w, ws["pred"], w_split=self.to_pred.plain)
        pp = self.pred_scale.data_ptr()
        if not normed_ahead:
            ops.adarmsnorm(h, self.final_gamma, None, None, out_split=ws["pred16"], split_scale=pp)
        lin = self.to_pred                   # (ops.gemm reads w_il only where pred16 is an interleaved pair)
        return ops.gemm(ws["normed"], lin.w, ws["pred"], w_split=lin.split, w_il=lin.il, a_split=ws["pred16"], a_scale=pp)

    def _layers_fp32(self, ctx: dict, step: int, h: torch.Tensor, free: list) -> torch.Tensor:
        """The layers on the fp32 residual stream with fp32 activations (no split I/O: up to SPLIT_IO_ABOVE_ROWS rows, 'fp32', odd widths)."""
        d, ws, Bt, T, rg = self.d, ctx["ws"], ctx["Bt"], ctx["T"], ctx["ragged"]
        tab = self._norm_rows(ctx, step)
        skips: List[torch.Tensor] = []
        for i, (cb, qkv, out, ff1, ff2) in enumerate(self.layers):
            g_attn, b_attn, g_ff, b_ff = tab[i].unbind(0)
            keep_input = cb is None              # this layer's input stays alive as a skip
            if keep_input:
                skips.append(h)
            else:
                s, comb = skips.pop(), free.pop()
                ops.gemm(h, cb.w, comb, bias=cb.bias, w_split=cb.plain, a2=s)
                free += [h, s]
                h = comb
            self._norm(ctx, h, g_attn, b_attn, ws["normed"])
            ops.gemm(ws["normed"], qkv.w, ws["qkv"], w_split=qkv.plain, rope=ws["rope"], rope_cols=2 * d["heads"] * 64)
            ops.attention(ws["qkv"], ws["att"], Bt, T, d["heads"], 64 ** -0.5, ragged=rg)
            h_in, h = h, (free.pop() if keep_input else h)
            ops.gemm(ws["att"], out.w, h, w_split=out.plain, residual=h_in)
            self._norm(ctx, h, g_ff, b_ff, ws["normed"])
            ops.gemm(ws["normed"], ff1.w, ws["ff"], bias=ff1.bias, w_split=ff1.plain, act=ops.ACT_GELU)
            ops.gemm(ws["ff"], ff2.w, h, bias=ff2.bias, w_split=ff2.plain, residual=h)
        return h

    def _layers_split(self, ctx: dict, step: int, h: torch.Tensor, twin: dict, free: list, fuse_norm: bool) -> tuple:
        """The layers on the fp32 residual stream with split-pair activations; returns (h, the final norm is done already).
        fuse_norm: every to_out / ff2 / skip-combiner product is followed by a norm of its output: one call (ops.gemm(norm=...)), so
        that problems on the split-K path (one utterance) normalise inside the reduction (FUSE_NORM_BELOW_ROWS rows and more never
        split K: the call would run the same two kernels, so it stays two calls there)."""
        d, ws, Bt, T, rg = self.d, ctx["ws"], ctx["Bt"], ctx["T"], ctx["ragged"]
        tab = self._norm_rows(ctx, step)
        sp_step, hp, pp = ctx["sp"][step], ctx["hp"], self.pred_scale.data_ptr()
        n16, a16, f16 = ws["normed16"], ws["att16"], ws["ff16"]
        normed_ahead = False                 # the attention norm of the layer about to start was produced by the previous GEMM
        skips: List[torch.Tensor] = []
        for i, (cb, qkv, out, ff1, ff2) in enumerate(self.layers):
            g_attn, b_attn, g_ff, b_ff = tab[i].unbind(0)
            # device pointers of this (evaluation, layer)'s activation pre-scales: normed, q|k, v, attention out, normed, ff
            s_na, s_qk, s_v, s_at, s_nf, s_ff = sp_step[i]
            keep_input = cb is None              # this layer's input stays alive as a skip
            if keep_input:
                skips.append(h)
            else:
                s, comb = skips.pop(), free.pop()
                ops.gemm(h, cb.w, comb, bias=cb.bias, w_split=cb.split, w_il=cb.il, a2=s, a_split=twin[id(h)], a2_split=twin[id(s)], a_scale=hp,
                         norm=dict(gamma=g_attn, beta=b_attn, out_split=n16, scale=s_na) if fuse_norm else None)
                normed_ahead = fuse_norm
                free += [h, s]
                h = comb
            if not normed_ahead:
                self._norm(ctx, h, g_attn, b_attn, None, out_split=n16, split_scale=s_na)
            # q | k split row-major, v split + transposed, straight into the f16x3 attention (any T: sequences whose
            # length is not a multiple of 4 store their v columns 2 bytes at a time)
            ops.gemm(ws["normed"], qkv.w, ws["qkv"], w_split=qkv.split, w_il=qkv.il, rope=ws["rope"], rope_cols=2 * d["heads"] * 64, a_split=n16,
                     out_split=ws["qk16"], vt_split=ws["vt16"], write_f32=False, a_scale=s_na, c_scale=s_qk, vt_scale=s_v)
            ops.attention_f16x3(ws["qk16"], ws["vt16"], None, Bt, T, d["heads"], 64 ** -0.5, out_split=a16,
                                qk_scale=s_qk, v_scale=s_v, out_scale=s_at, ragged=rg)
            h_in, h = h, (free.pop() if keep_input else h)
            ops.gemm(ws["att"], out.w, h, w_split=out.split, w_il=out.il, residual=h_in, a_split=a16, a_scale=s_at,
                     norm=dict(gamma=g_ff, beta=b_ff, out_split=n16, scale=s_nf) if fuse_norm else None)
            if not fuse_norm:
                self._norm(ctx, h, g_ff, b_ff, None, out_split=n16, split_scale=s_nf)
            ops.gemm(ws["normed"], ff1.w, ws["ff"], bias=ff1.bias, w_split=ff1.split, w_il=ff1.il, act=ops.ACT_GELU, a_split=n16, out_split=f16,
                     write_f32=False, a_scale=s_nf, c_scale=s_ff)
            last = i + 1 == d["depth"]
            nm = None
            if fuse_norm and last:                   # the final RMSNorm in front of to_pred
                nm = dict(gamma=self.final_gamma, beta=None, out_split=ws["pred16"], scale=pp)
            elif fuse_norm and self.layers[i + 1].comb is None:      # next layer starts with its attention norm
                nm = dict(gamma=tab[i + 1, 0], beta=tab[i + 1, 1], out_split=n16, scale=sp_step[i + 1][0])
            ops.gemm(ws["ff"], ff2.w, h, bias=ff2.bias, w_split=ff2.split, w_il=ff2.il, residual=h, a_split=f16,
                     out_split=None if last else twin[id(h)], a_scale=s_ff, c_scale=None if last else hp, norm=nm)
            normed_ahead = nm is not None
        return h, normed_ahead

    def _layers_pair_stream(self, ctx: dict, step: int, h: torch.Tensor, twin: dict, free: list) -> torch.Tensor:
        """The layers with the residual stream as split pairs only and WITHOUT the norm kernel (route.deferred).  h: the embedding
        output (fp32, its pair already in twin[id(h)]).  An AdaptiveRMSNorm is one gamma / beta row per evaluation for every frame
        (acoustic.py:198-204), so for the product that follows it (:306-318)
            norm(x) W^T = (sqrt(D) / ||x_row||) * (x (W diag(gamma))^T) + beta W^T :
        * the producing GEMM (to_out, ff2, skip combiner) writes its output ONLY as the split pair the skip combiners already
          needed (no fp32 store: it moves the bytes the fp32 form moved), reads its residual from that pair, and leaves the rows'
          sums of squares per 64 columns (cvx_gemm_split_io.R_hi / c_rowsq); cvx_rownorm_scale_f32 makes one factor per row;
        * the consuming GEMM (to_qkv, ff1) multiplies its accumulator rows by that factor, carries beta W^T in its bias and runs on
          W diag(gamma(t)) - split copies of the weights for every evaluation time of the solver grid, built ONCE per (model, grid)
          (_time_tables; cvx_split_f16_colscale_il: 7 GB for 32 evaluation times - capacity HBM3E has - written in ~2 ms).
        The norm kernel (131 MB of traffic per launch at the bench shape, 16 of 17 launches per evaluation) does not run and ff2 no
        longer writes its output twice.  Only the first layer's attention norm (input from the embedding, fp32) and the final norm
        stay.  Large-problem kernel only: batches of DEFER_MIN_ROWS rows and more (CVX_DEFER_NORM=0: off)."""
        d, ws, dn, Bt, T, M, rg = self.d, ctx["ws"], ctx["dn"], ctx["Bt"], ctx["T"], ctx["M"], ctx["ragged"]
        dim, L = d["dim"], d["depth"]
        tab = ctx["table"][step].view(L, 4, dim)
        sp_step, hsp = ctx["sp"][step], dn["hsp"]
        cur = hsp[0][0]                      # device pointer of the pre-scale the current h's pair carries (one per stage, _activation_scales)
        parts64, rt_dim, rowsq, rs = dim // 64, float(dim) ** 0.5, ws["rowsq"], ws["rs"]
        n16, a16, f16 = ws["normed16"], ws["att16"], ws["ff16"]
        def factor():                        # sqrt(D) / ||row|| from the producer's partial sums (computing it in the consumer's epilogue instead
            ops.rownorm_scale(rowsq, M, parts64, rs, rt_dim)       # was built and measured: + 5 ms per step against these 480 launches of 5 us)
        qkv_kw = dict(rope=ws["rope"], rope_cols=2 * d["heads"] * 64, out_split=ws["qk16"], vt_split=ws["vt16"], write_f32=False)
        skips: List[tuple] = []
        have_rs = False                      # rowsq holds the sums of squares of the current h's rows (per 64 columns)
        for i, (cb, qkv, out, ff1, ff2) in enumerate(self.layers):
            s_na, s_qk, s_v, s_at, s_nf, s_ff = sp_step[i]
            as_a, as_f = dn["asp"][step][i]
            last = i + 1 == L
            keep_input = cb is None              # this layer's input stays alive as a skip
            if keep_input:
                skips.append((h, cur))
            else:
                (s, s_scale), comb = skips.pop(), free.pop()
                ops.gemm(h, cb.w, comb, bias=cb.bias, w_split=cb.split, w_il=cb.il, a2=s, a_split=twin[id(h)], a2_split=twin[id(s)], a_scale=cur,
                         a2_scale=s_scale, out_split=twin[id(comb)], c_scale=hsp[i][1], c_rowsq=rowsq, write_f32=False)
                cur = hsp[i][1]
                factor()
                have_rs = True
                free += [h, s]
                h = comb
            if have_rs:
                ops.gemm(ws["normed"], qkv.w, ws["qkv"], w_split=qkv.split, w_il=dn["wq"][i][step], bias=dn["bq"][i][step], a_split=twin[id(h)],
                         a_scale=as_a, a_row_scale=rs, c_scale=s_qk, vt_scale=s_v, **qkv_kw)
            else:                            # first layer: the embedding output exists in fp32
                ops.adarmsnorm(h, tab[i, 0], tab[i, 1], None, out_split=n16, split_scale=s_na)
                ops.gemm(ws["normed"], qkv.w, ws["qkv"], w_split=qkv.split, w_il=qkv.il, a_split=n16, a_scale=s_na, c_scale=s_qk, vt_scale=s_v, **qkv_kw)
            ops.attention_f16x3(ws["qk16"], ws["vt16"], None, Bt, T, d["heads"], 64 ** -0.5, out_split=a16,
                                qk_scale=s_qk, v_scale=s_v, out_scale=s_at, ragged=rg)
            h_in, h = h, (free.pop() if keep_input else h)
            ops.gemm(ws["att"], out.w, h, w_split=out.split, w_il=out.il, a_split=a16, a_scale=s_at, res_split=twin[id(h_in)], res_scale=cur,
                     out_split=twin[id(h)], c_scale=hsp[i][2], c_rowsq=rowsq, write_f32=False)
            cur = hsp[i][2]
            factor()
            ops.gemm(ws["normed"], ff1.w, ws["ff"], w_split=ff1.split, w_il=dn["w1"][i][step], bias=dn["b1p"][i][step], act=ops.ACT_GELU,
                     a_split=twin[id(h)], out_split=f16, write_f32=False, a_scale=as_f, a_row_scale=rs, c_scale=s_ff)
            feeds_norm = (not last) and self.layers[i + 1].comb is None   # the next layer's attention norm reads THIS output's rows
            ops.gemm(ws["ff"], ff2.w, h, bias=ff2.bias, w_split=ff2.split, w_il=ff2.il, a_split=f16, a_scale=s_ff, res_split=twin[id(h)],
                     res_scale=cur, out_split=twin[id(h)], c_scale=hsp[i][3], c_rowsq=rowsq if feeds_norm else None,
                     write_f32=last)                                      # (the final norm reads fp32)
            cur = hsp[i][3]
            if feeds_norm:
                factor()
            have_rs = feeds_norm
        return h


@dataclass(frozen=True)
class Tableau:
    """Butcher tableau of an explicit Runge-Kutta method on the fixed grid: stage j evaluates the field at t0 + c[j] dt on
    y + dt sum_i a[j-1][i] k_i, the step ends at y + dt sum_j b[j] k_j.  `a` holds the strictly lower-triangular rows (row j - 1 of
    stage j: j entries), so a one-stage method has a = ().  At most MAX_STAGES stages (the stage kernel keeps three earlier ones).
    Frozen and hashable: it is part of the keys of the per-grid tables and of the captured graphs.
    b_err (optional): the weights of a LOWER-order solution on the same stages - an embedded pair.  dt sum_j (b[j] - b_err[j]) k_j is
    then the local error of that lower-order solution (FlowMatchingSampler.sample(return_error=True)).  It does not change the solve
    and takes no part in equality or the hash: the time tables and graphs of a tableau serve it with any b_err."""
    name: str
    a: Tuple[Tuple[float, ...], ...]
    b: Tuple[float, ...]
    c: Tuple[float, ...]
    b_err: Optional[Tuple[float, ...]] = field(default=None, compare=False)

    MAX_STAGES = 4

    def __post_init__(self):
        try:
            a = tuple(tuple(float(x) for x in row) for row in self.a)
            b, c = tuple(float(x) for x in self.b), tuple(float(x) for x in self.c)
        except TypeError as e:
            raise ValueError(f"tableau {self.name!r}: a must be rows of numbers, b and c sequences of numbers") from e
        for k, v in (("a", a), ("b", b), ("c", c)):
            object.__setattr__(self, k, v)
        n = len(b)
        if not 1 <= n <= self.MAX_STAGES:
            raise ValueError(f"tableau {self.name!r}: {n} stages, 1 to {self.MAX_STAGES} are supported")
        if len(c) != n or len(a) != n - 1 or any(len(row) != j + 1 for j, row in enumerate(a)):
            raise ValueError(f"tableau {self.name!r}: a must be the {n - 1} strictly lower-triangular rows (1, 2, ... entries) and c must have {n} entries")
        if not all(math.isfinite(x) for x in b + c + tuple(x for row in a for x in row)):
            raise ValueError(f"tableau {self.name!r}: non-finite entry")
        if abs(sum(b) - 1.0) > 1e-12:
            raise ValueError(f"tableau {self.name!r}: sum(b) = {sum(b)!r}, a consistent method needs 1")
        for j in range(n):
            row_sum = sum(a[j - 1]) if j else 0.0
            if abs(c[j] - row_sum) > 1e-12:
                raise ValueError(f"tableau {self.name!r}: c[{j}] = {c[j]!r} is not the sum of its row of a ({row_sum!r})")
        if self.b_err is not None:
            try:
                be = tuple(float(x) for x in self.b_err)
            except TypeError as e:
                raise ValueError(f"tableau {self.name!r}: b_err must be a sequence of numbers") from e
            object.__setattr__(self, "b_err", be)
            if len(be) != n or not all(math.isfinite(x) for x in be):
                raise ValueError(f"tableau {self.name!r}: b_err must have {n} finite entries")
            if abs(sum(be) - 1.0) > 1e-12:
                raise ValueError(f"tableau {self.name!r}: sum(b_err) = {sum(be)!r}, a consistent method needs 1")
            if be == b:
                raise ValueError(f"tableau {self.name!r}: b_err equals b - the estimate would be 0")

    @property
    def stages(self) -> int:
        return len(self.b)

    @property
    def err_order(self) -> Optional[int]:
        """Order q of the solution b_err gives (None without b_err): 1, 2 with sum b_err_j c_j = 1/2, 3 with the two third-order
        conditions on top.  The estimate of a step is O(dt^(q+1))."""
        if self.b_err is None:
            return None
        n, be, c = self.stages, self.b_err, self.c
        ac = [sum(self.a[j - 1][i] * c[i] for i in range(j)) if j else 0.0 for j in range(n)]
        dot = lambda u, v: sum(x * y for x, y in zip(u, v))
        if abs(dot(be, c) - 0.5) > 1e-12:
            return 1
        if abs(dot(be, [x * x for x in c]) - 1 / 3) > 1e-12 or abs(dot(be, ac) - 1 / 6) > 1e-12:
            return 2
        return 3


TABLEAUS = {t.name: t for t in (
    # b_err (last argument): Euler's step inside midpoint and Heun (order 1), a second-order rule on the stages of the others
    Tableau("euler", (), (1.0,), (0.0,)),
    Tableau("midpoint", ((0.5,),), (0.0, 1.0), (0.0, 0.5), (1.0, 0.0)),
    Tableau("heun2", ((1.0,),), (0.5, 0.5), (0.0, 1.0), (1.0, 0.0)),
    Tableau("heun3", ((1 / 3,), (0.0, 2 / 3)), (0.25, 0.0, 0.75), (0.0, 1 / 3, 2 / 3), (0.0, 0.5, 0.5)),
    # torchdiffeq's fixed-grid "rk4" is the 3/8 rule (the reference's torchdiffeq_ode_method, acoustic.py:560-591)
    Tableau("rk4", ((1 / 3,), (-1 / 3, 1.0), (1.0, -1.0, 1.0)), (1 / 8, 3 / 8, 3 / 8, 1 / 8), (0.0, 1 / 3, 2 / 3, 1.0), (0.0, 0.5, 0.5, 0.0)),
    Tableau("rk4_classic", ((0.5,), (0.0, 0.5), (0.0, 0.0, 1.0)), (1 / 6, 1 / 3, 1 / 3, 1 / 6), (0.0, 0.5, 0.5, 1.0), (0.0, 1.0, 0.0, 0.0)),
)}


def resolve_method(method) -> Tableau:
    """The tableau of a solver given by name or as a Tableau; ValueError for anything else (an unknown name used to run Euler)."""
    if isinstance(method, Tableau):
        return method
    if isinstance(method, str) and method in TABLEAUS:
        return TABLEAUS[method]
    raise ValueError(f"unknown ODE method {method!r}: one of {', '.join(TABLEAUS)} or a Tableau")


SWAY_MAX = 2.0 / (math.pi - 2.0)        # t' = u + s (cos(pi u / 2) - 1 + u) is monotone on [0, 1] for -1 <= s <= 2 / (pi - 2)


def _steps_of(nfe: int, tab: Tableau) -> int:
    n = tab.stages
    if int(nfe) != nfe or nfe < n or nfe % n:
        raise ValueError(f"nfe={nfe} is not valid for method={tab.name}: a positive multiple of its {n} stage(s)")
    return int(nfe) // n


def time_grid(spec, steps: int) -> Tuple[float, ...]:
    """The steps + 1 grid points of a solve on [0, 1] as python floats that fp32 holds exactly: 0.0 first, 1.0 last, strictly increasing.
    spec: 'uniform' (the reference's grid: arange(steps + 1) * fp32(1 / steps) in fp32, the last point set to 1), 'sway:<s>'
    (t' = u + s (cos(pi u / 2) - 1 + u) on u = j / steps, -1 <= s <= 2 / (pi - 2): s < 0 takes small steps first - F5-TTS's sway
    sampling), 'cosine' (t' = (1 - cos(pi u)) / 2: small steps at both ends), or an explicit sequence of steps + 1 numbers (rounded to
    fp32).  sway and cosine are computed in fp64 and rounded to fp32 ('sway:0' need not have the uniform grid's bits).  ValueError,
    naming the entry: wrong length, a non-finite value, ends other than 0 and 1, not strictly increasing."""
    if int(steps) != steps or steps < 1:
        raise ValueError(f"time grid: steps={steps!r}, a positive integer is needed")
    steps = int(steps)
    if isinstance(spec, str):
        if spec == "uniform":
            g = torch.arange(0, steps + 1, dtype=torch.float32) * torch.tensor(1.0 / steps, dtype=torch.float32)
            g[-1] = 1.0
            vals = g.tolist()
        elif spec == "cosine" or spec.startswith("sway:"):
            if spec == "cosine":
                fn = lambda u: (1.0 - math.cos(math.pi * u)) / 2.0
            else:
                try:
                    sw = float(spec[5:])
                except ValueError:
                    raise ValueError(f"time grid {spec!r}: sway:<s> needs a number") from None
                if not -1.0 <= sw <= SWAY_MAX:             # (NaN fails both comparisons)
                    raise ValueError(f"time grid {spec!r}: s must lie in [-1, 2 / (pi - 2) = {SWAY_MAX:.6f}], where the map is monotone")
                fn = lambda u: u + sw * (math.cos(math.pi * u / 2.0) - 1.0 + u)
            vals = [fn(j / steps) for j in range(steps + 1)]
            vals[0], vals[-1] = 0.0, 1.0
        else:
            raise ValueError(f"unknown time grid {spec!r}: uniform, cosine, sway:<s> or a sequence of steps + 1 numbers")
    else:
        try:
            vals = [float(x) for x in spec]
        except (TypeError, ValueError) as e:
            raise ValueError(f"time grid: {spec!r} is neither a grid's name nor a sequence of numbers") from e
        if len(vals) != steps + 1:
            raise ValueError(f"time grid: {len(vals)} points for {steps} steps, {steps + 1} are needed")
    for j, v in enumerate(vals):
        if not math.isfinite(v):
            raise ValueError(f"time grid: entry {j} is {v!r}")
    vals = torch.tensor(vals, dtype=torch.float64).to(torch.float32).tolist()
    if vals[0] != 0.0:
        raise ValueError(f"time grid: entry 0 is {vals[0]!r}, the grid starts at 0")
    if vals[-1] != 1.0:
        raise ValueError(f"time grid: entry {steps} is {vals[-1]!r}, the grid ends at 1")
    for j in range(steps):
        if not vals[j] < vals[j + 1]:
            raise ValueError(f"time grid: entry {j + 1} ({vals[j + 1]!r}) is not above entry {j} ({vals[j]!r}) in fp32")
    return tuple(vals)


def resolve_grid(grid, nfe: int, method) -> Optional[Tuple[float, ...]]:
    """None for the uniform grid (None, 'uniform', or its points given explicitly: existing callers keep their table and graph keys),
    otherwise the validated grid as a hashable tuple - with every refusal of time_grid and of evaluation_times."""
    if grid is None or (isinstance(grid, str) and grid == "uniform"):
        return None
    tab = resolve_method(method)
    g = time_grid(grid, _steps_of(nfe, tab))
    if g == time_grid("uniform", len(g) - 1):
        return None
    evaluation_times(nfe, tab, g)
    return g


def evaluation_times(nfe: int, method, grid=None):
    """Fixed grid of the reference solver (torchdiffeq fixed-grid, options.step_size) as python floats
    computed in fp32 exactly like the solver does: (t0, dt) per step, plus every time the field is evaluated at -
    t0 + fp32(c_j) dt per stage, the grid point t1 itself for a stage with c_j = 1 (as torchdiffeq's rk4 does).  One time per
    evaluation: the last stage of a step and the first of the next may repeat a time (the per-time tables are indexed by evaluation).
    grid: None / 'uniform', or anything time_grid takes - the same fp32 arithmetic on its points.  ValueError if a step of a given
    grid is so small that a stage time with 0 < c_j < 1 rounds onto t0 or t1."""
    tab = resolve_method(method)
    steps = _steps_of(nfe, tab)
    given = not (grid is None or (isinstance(grid, str) and grid == "uniform"))
    if given:
        grid = torch.tensor(time_grid(grid, steps), dtype=torch.float32)
    else:
        h = torch.tensor(1.0 / steps, dtype=torch.float32)
        grid = torch.arange(0, steps + 1, dtype=torch.float32) * h
        grid[-1] = 1.0
    times, dts = [], []
    for j, (a, b) in enumerate(zip(grid[:-1], grid[1:])):
        dt = b - a
        dts.append(float(dt))
        for c in tab.c:
            if c == 0.0:
                times.append(float(a))
            elif c == 1.0:
                times.append(float(b))
            else:
                t = float(a + torch.tensor(c, dtype=torch.float32) * dt)
                if given and 0.0 < c < 1.0 and not float(a) < t < float(b):
                    raise ValueError(f"time grid: entry {j + 1} ({float(b)!r}) is so close to entry {j} ({float(a)!r}) that the stage at "
                                     f"c = {c!r} of {tab.name} falls onto a grid point in fp32")
                times.append(t)
    return torch.tensor(times, dtype=torch.float32), dts


@dataclass(frozen=True)
class SolveError:
    """The embedded error estimate of one solve.  delta_rms[k, i]: root mean square over utterance i's elements of
    delta = dt_k sum_j (b_j - b_err_j) k_j at step k - the local error of the order-`order` solution on the method's stages,
    O(dt^(order + 1)); state_rms[k, i]: the same mean of the state after step k.  fp64 CPU tensors [steps, utterances]."""
    grid: Tuple[float, ...]
    method: Union[str, Tableau]
    order: int
    delta_rms: torch.Tensor
    state_rms: torch.Tensor


def fit_time_grid(error: SolveError, steps: int, reduce: str = "rms") -> Tuple[float, ...]:
    """A grid of `steps` steps that equidistributes the measured local error: with E_k the `reduce` ('rms', 'mean' or 'max') over the
    utterances of error.delta_rms[k], h_k the steps of error.grid and q = error.order, the density rho_k = E_k^(1 / (q + 1)) / h_k is
    constant on step k (a step of length h there has local error ~ (rho h)^(q + 1)); F is its integral and the new points are
    F^-1(j F(1) / steps), piecewise linear.  fp64 on the host, rounded to fp32, ends exactly 0 and 1, refused like an explicit grid.
    Equal E_k on a uniform grid give the uniform points (up to the fp32 rounding of j / steps)."""
    d = error.delta_rms.to(torch.float64)
    if d.ndim != 2 or d.shape[0] != len(error.grid) - 1 or d.shape[1] < 1 or not bool(torch.isfinite(d).all()):
        raise ValueError("fit_time_grid: delta_rms must be a finite [steps, utterances] table on error.grid")
    if reduce == "rms":
        E = d.square().mean(dim=1).sqrt()
    elif reduce == "mean":
        E = d.mean(dim=1)
    elif reduce == "max":
        E = d.amax(dim=1)
    else:
        raise ValueError(f"fit_time_grid: reduce={reduce!r}: rms, mean or max")
    old = [float(t) for t in error.grid]
    E = [max(float(e), 1e-300) for e in E]
    p = 1.0 / (int(error.order) + 1)
    F = [0.0]
    for e in E:
        F.append(F[-1] + e ** p)                       # rho_k h_k
    new, k = [], 0
    for j in range(steps + 1):
        tgt = j * F[-1] / steps
        while k + 1 < len(E) and F[k + 1] < tgt:
            k += 1
        new.append(old[k] + (old[k + 1] - old[k]) * min(max((tgt - F[k]) / (F[k + 1] - F[k]), 0.0), 1.0))
    new[0], new[-1] = 0.0, 1.0
    g = time_grid(new, steps)
    tab = resolve_method(error.method)
    evaluation_times(steps * tab.stages, tab, g)
    return g


class FlowMatchingSampler:
    """ConditionalFlowMatcherWrapper.sample (acoustic.py:597-688) on a VectorField.

    `nfe` counts CFG-combined field evaluations: the reference's ode_step_size=0.0625 midpoint
    setting is nfe=32 (16 steps x 2).  `method`: the name of a built-in tableau (TABLEAUS: the reference's torchdiffeq_ode_method;
    'euler' is an extra the reference lacks) or a Tableau; nfe must be a multiple of its stage count.  cond_scale may be one float
    per utterance (extension: the reference takes one scalar per call).  `grid`: the time grid (time_grid: 'uniform', 'sway:<s>',
    'cosine' or the points) - fixed before the solve starts, like everything that depends on the evaluation times."""

    def __init__(self, field: VectorField, nfe: int = 32, method: Union[str, Tableau] = "midpoint", grid="uniform"):
        self.field, self.nfe, self.method = field, nfe, method
        resolve_method(method)
        self.grid = resolve_grid(grid, nfe, method)      # None: uniform; otherwise a tuple - part of the table and graph keys

    # launch-bound regime (short / single utterances): the whole solve - ~2400 kernel launches for 32 NFE - is captured
    # once per input shape into a HIP graph and replayed (env CVX_GRAPH=0 disables, CVX_GRAPH_MAX_ROWS bounds the
    # batch size it applies to; large batches are GPU-bound and stay eager).
    GRAPH_CACHE = 4

    def _times_key(self) -> tuple:
        return (int(self.nfe), str(self.method)) + (() if self.grid is None else (self.grid,))

    def _integrate(self, phoneme_ids, cond, y, times_dev, dts, s: float, use_null: bool, lengths=None, row_scale=None, err=None) -> None:
        """prepare() + the fixed-grid loop; advances `y` in place (ragged batch: y, cond, ids packed, see prepare).
        row_scale: one guidance scale per row of y on the device (then `s` is not used).  err: the buffers of the embedded error
        estimate (_error_state) - the generic stage loop then runs for every method."""
        f = self.field
        ctx = f.prepare(phoneme_ids, cond, times_dev, use_null, lengths=lengths, times_key=self._times_key())
        ws, M1 = ctx["ws"], ctx["M1"]
        xin = ws["xin"]
        x_c = xin[:M1]
        x_n = xin[M1:] if use_null else None
        x_c.copy_(y.reshape(M1, -1))
        if use_null:
            x_n.copy_(x_c)
        if row_scale is not None or err is not None or self.method not in ("midpoint", "euler"):      # (an explicit Tableau is never equal to a name)
            self._integrate_stages(ctx, y.reshape(M1, -1), dts, s, resolve_method(self.method), row_scale, err)
            return ctx
        evaluate = f.evaluate
        e = 0
        for dt in dts:
            if self.method == "midpoint":
                pred = evaluate(ctx, e); e += 1
                ops.cfg_combine_axpy(pred[:M1], pred[M1:] if use_null else None, y, s, 0.5 * dt, x_c, x_n)
                pred = evaluate(ctx, e); e += 1
                ops.cfg_combine_axpy(pred[:M1], pred[M1:] if use_null else None, y, s, dt, y, x_c, x_n)
            else:
                pred = evaluate(ctx, e); e += 1
                ops.cfg_combine_axpy(pred[:M1], pred[M1:] if use_null else None, y, s, dt, y, x_c, x_n)
        return ctx

    def _integrate_stages(self, ctx: dict, y: torch.Tensor, dts, s: float, tab: Tableau, row_scale, err=None) -> None:
        """The fixed-grid loop of any explicit tableau: one field evaluation and one cvx_rk_stage_f32 launch per stage.  The launch
        after stage i combines the CFG branches into k_i and writes the next evaluation's input y + dt sum_l a[i+1][l] k_l - after
        the last stage the step's result y + dt sum_l b[l] k_l, in place.  k_i is stored only when a later launch reads it (its b
        or a later row of a is not 0): midpoint and Euler store nothing, Heun's third-order rule one stage, the fourth-order rules
        three - buffers of the workspace, made on first use.
        err: the last launch of every step is cvx_rk_stage_err_f32 (the same bits in y) with the weights dt (b_j - b_err_j); a stage
        those weights read is stored as well (midpoint's k_0), and one cvx_rk_err_finish_f32 launch ends the solve."""
        f = self.field
        ws, M1, use_null = ctx["ws"], ctx["M1"], ctx["use_null"]
        x_c = ws["xin"][:M1]
        x_n = ws["xin"][M1:] if use_null else None
        n = tab.stages
        rows = ((),) + tab.a + (tab.b,)          # rows[i + 1]: the weights the launch after stage i applies to k_0 .. k_i
        db = [b - be for b, be in zip(tab.b, tab.b_err)] if err is not None else [0.0] * n
        keep = [i + 1 < n and (db[i] != 0.0 or any(rows[j][i] != 0.0 for j in range(i + 2, n + 1))) for i in range(n)]
        bufs = iter(f.stage_buffers(ctx, sum(keep)))
        k = [next(bufs) if keep[i] else None for i in range(n)]
        e = 0
        for step, dt in enumerate(dts):
            for i in range(n):
                pred = f.evaluate(ctx, e); e += 1
                coef, last = rows[i + 1], i + 1 == n
                if last and err is not None:
                    ops.rk_stage_err(pred[:M1], pred[M1:] if use_null else None, y, s, [dt * c for c in coef], [dt * c for c in db], y,
                                     err["map"], err["partials"][step], k_prev=[k[l] if (coef[l] != 0.0 or db[l] != 0.0) else None for l in range(i)],
                                     row_scale=row_scale, out2=x_c, out3=x_n)
                    continue
                ops.rk_stage(pred[:M1], pred[M1:] if use_null else None, y, s, [dt * c for c in coef], y if last else x_c,
                             k_prev=[k[l] if coef[l] != 0.0 else None for l in range(i)], k_out=k[i], row_scale=row_scale,
                             out2=x_c if last else x_n, out3=x_n if last else None)
        if err is not None:
            ops.rk_err_finish(err["partials"], err["map"], err["sums"])

    def _error_state(self, lengths: List[int], return_error: bool) -> Optional[dict]:
        """The device buffers of the embedded error estimate for sequences of these lengths: the block map of the last-stage kernel,
        its partial sums per (step, block) and the sums per (step, sequence).  Made once per call - or once per captured graph, whose
        static state they are - before the loop starts."""
        if not return_error:
            return None
        tab = resolve_method(self.method)
        if tab.b_err is None:
            raise ValueError(f"return_error: method {tab.name!r} has no embedded pair (Tableau.b_err)")
        dev, steps = self.field.device, len(self._grid_points()) - 1
        emap = ops.RkErrMap(lengths, dev)
        return dict(map=emap, partials=torch.zeros(steps, emap.blocks, 2, dtype=torch.float32, device=dev),
                    sums=torch.zeros(steps, emap.n_seq, 2, dtype=torch.float32, device=dev))

    def _grid_points(self) -> Tuple[float, ...]:
        return self.grid if self.grid is not None else time_grid("uniform", _steps_of(self.nfe, resolve_method(self.method)))

    def _solve_error(self, err: dict, lengths: List[int]) -> SolveError:
        """the two tables of a finished solve on the host (one synchronising copy)"""
        tab = resolve_method(self.method)
        sums = err["sums"].cpu().double()                                           # [steps, sequences, 2]
        count = torch.tensor([L * self.field.d["dim_out"] for L in lengths], dtype=torch.float64)
        return SolveError(grid=self._grid_points(), method=self.method, order=tab.err_order,
                          delta_rms=(sums[..., 0] / count).sqrt(), state_rms=(sums[..., 1] / count).sqrt())

    @staticmethod
    def _scales(cond_scale, n: int):
        """(scalar, per-utterance list or None) of a cond_scale given as one number or as one number per utterance; equal values
        are the scalar."""
        if not (isinstance(cond_scale, (list, tuple)) or getattr(cond_scale, "ndim", 0) > 0):
            return float(cond_scale), None
        vals = [float(v) for v in cond_scale]
        if len(vals) != n:
            raise ValueError(f"cond_scale: {len(vals)} values for {n} utterances")
        if all(v == vals[0] for v in vals):
            return vals[0], None
        return 0.0, vals

    @ops.gated
    @torch.no_grad()
    def sample(self, *, phoneme_ids: torch.Tensor, cond: torch.Tensor, mask: Optional[torch.Tensor] = None,
               cond_scale: Union[float, Sequence[float]] = 1.0, y0: Optional[torch.Tensor] = None, return_error: bool = False):
        """return_error: also measure the embedded error estimate - the result is (y, SolveError), y with the bits of the plain call."""
        f, d = self.field, self.field.d
        dev = f.device
        if cond.ndim != 3 or cond.shape[-1] != d["dim_cond"]:
            raise AssertionError(f"cond must be [B,T,{d['dim_cond']}], got {tuple(cond.shape)}")
        expect_ids = cond.shape[:2] + ((d["streams"],) if d["streams"] > 1 else ())
        if tuple(phoneme_ids.shape) != tuple(expect_ids):
            raise AssertionError(f"phoneme_ids must be {tuple(expect_ids)}, got {tuple(phoneme_ids.shape)}")
        cond = cond.to(device=dev, dtype=torch.float32).contiguous()
        phoneme_ids = phoneme_ids.to(device=dev, dtype=torch.int64).contiguous()
        B, T, _ = cond.shape
        if y0 is None:                       # acoustic.py:647-650 (VoMix draws 80 channels)
            y0 = torch.randn(B, T, d["dim_out"], device=dev, dtype=torch.float32)
        if tuple(y0.shape) != (B, T, d["dim_out"]):
            raise AssertionError(f"y0 must be [B,T,{d['dim_out']}] = {(B, T, d['dim_out'])}, got {tuple(y0.shape)}")
        y = y0.to(device=dev, dtype=torch.float32).contiguous().clone()
        s, per = self._scales(cond_scale, B)
        use_null = s != 1.0 if per is None else True         # acoustic.py:423 (different scales: at least one is not 1)
        # per-utterance scales: one float per row, read by the stage kernel (a row at 1.0 takes its conditional branch there)
        row_scale = None if per is None else ops.h2d(torch.tensor(per, dtype=torch.float32).repeat_interleave(T), dev)
        times, dts = evaluation_times(self.nfe, self.method, self.grid)
        if not f.route((2 * B if use_null else B) * T).graph:
            err = self._error_state([T] * B, return_error)
            self._integrate(phoneme_ids, cond, y, ops.h2d(times, dev), dts, s, use_null, row_scale=row_scale, err=err)
            return (y, self._solve_error(err, [T] * B)) if return_error else y
        main = torch.cuda.current_stream()
        # (the saturation flag of the launching stream is a kernel argument of the captured launches: one graph per stream;
        #  per-utterance scales sit in a buffer the graph reads: one graph serves every mix of them)
        key = (B, T, use_null, s if per is None else "per-row", self.nfe, self.method, main.cuda_stream)
        if self.grid is not None:            # (the uniform grid keeps the key it always had)
            key += (self.grid,)
        if return_error:                     # (b_err takes no part in a Tableau's equality)
            key += ("error", resolve_method(self.method).b_err)
        cache = f.__dict__.setdefault("_graphs", {})
        ent = cache.get(key)
        if ent is None:
            st = dict(ids=phoneme_ids.clone(), cond=cond.clone(), y=y.clone(), times=ops.h2d(times, dev),
                      row_scale=None if row_scale is None else row_scale.clone(), err=self._error_state([T] * B, return_error))
            ctx = self._integrate(st["ids"], st["cond"], st["y"], st["times"], dts, s, use_null, row_scale=st["row_scale"], err=st["err"])   # eager warm-up
            st["ws"] = ctx["ws"]             # keep this shape's workspace alive for as long as the graph is
            # (thread-local capture mode + the package's capture gate: another host thread driving its own model on this device
            #  must not break this capture, nor be broken by it - HIP rejects its synchronisations while a capture is open even
            #  in thread-local mode, so the capture waits until the package's other entry points have left; ops._CaptureGate)
            with ops.CAPTURE_GATE.exclusive():
                main.synchronize()
                g = torch.cuda.CUDAGraph()
                if getattr(self, "_cap", None) is None:
                    self._cap = torch.cuda.Stream(device=dev)
                ops.saturation_share(main, self._cap)    # the captured launches report into the calling stream's flag
                with torch.cuda.graph(g, stream=self._cap, capture_error_mode="thread_local"):
                    self._integrate(st["ids"], st["cond"], st["y"], st["times"], dts, s, use_null, row_scale=st["row_scale"], err=st["err"])
            cache = f.__dict__.setdefault("_graphs", {})     # (the warm-up may have evicted a time grid and, with it, the cache)
            if len(cache) >= self.GRAPH_CACHE:
                cache.pop(next(iter(cache)))
            ent = cache[key] = (g, st)
        g, st = ent
        st["ids"].copy_(phoneme_ids)
        st["cond"].copy_(cond)
        st["y"].copy_(y)
        if row_scale is not None:
            st["row_scale"].copy_(row_scale)
        g.replay()
        if return_error:
            return st["y"].clone(), self._solve_error(st["err"], [T] * B)
        return st["y"].clone()

    @ops.gated
    @torch.no_grad()
    def sample_ragged(self, *, phoneme_ids: List[torch.Tensor], cond: List[torch.Tensor], cond_scale: Union[float, Sequence[float]] = 1.0,
                      y0: Optional[List[torch.Tensor]] = None, return_error: bool = False):
        """The same solve for several utterances of DIFFERENT length in one launch sequence: utterance i is
        phoneme_ids[i] [T_i(, streams)], cond[i] [T_i, dim_cond] (y0[i] [T_i, dim_out]); returns the list of [T_i, dim_out]
        results.  The reference runs such utterances one at a time (monologue_generation.py:259-304) and its network has
        no padding mask (acoustic.py:313), so they are PACKED back to back - M = sum T_i rows - and the three operators
        that look along time (attention, rotary positions, ConvPositionEmbed) work per sequence (include/covomix_hip.h,
        RAGGED BATCHES); every utterance gets the result of its own B = 1 run up to fp32 summation order.
        cond_scale: one float, or one per utterance.  return_error: the result is (list, SolveError), as in sample()."""
        f, d = self.field, self.field.d
        dev = f.device
        n = len(cond)
        if n == 0:
            if return_error:
                raise ValueError("return_error: no utterance to measure")
            return []
        lengths = [int(c.shape[0]) for c in cond]
        for i in range(n):
            if cond[i].ndim != 2 or cond[i].shape[1] != d["dim_cond"] or lengths[i] < 1:
                raise AssertionError(f"cond[{i}] must be [T,{d['dim_cond']}] with T >= 1, got {tuple(cond[i].shape)}")
            expect = (lengths[i],) + ((d["streams"],) if d["streams"] > 1 else ())
            if tuple(phoneme_ids[i].shape) != expect:
                raise AssertionError(f"phoneme_ids[{i}] must be {expect}, got {tuple(phoneme_ids[i].shape)}")
            if y0 is not None and tuple(y0[i].shape) != (lengths[i], d["dim_out"]):
                raise AssertionError(f"y0[{i}] must be {(lengths[i], d['dim_out'])}, got {tuple(y0[i].shape)}")
        cond_p = torch.cat([c.to(device=dev, dtype=torch.float32) for c in cond]).contiguous()
        ids_p = torch.cat([p.to(device=dev, dtype=torch.int64) for p in phoneme_ids]).contiguous()
        if y0 is None:                       # acoustic.py:647-650, one draw per utterance
            y = torch.randn(cond_p.shape[0], d["dim_out"], device=dev, dtype=torch.float32)
        else:
            y = torch.cat([t.to(device=dev, dtype=torch.float32) for t in y0]).contiguous().clone()
        s, per = self._scales(cond_scale, n)
        use_null = s != 1.0 if per is None else True         # acoustic.py:423
        row_scale = None if per is None else ops.h2d(torch.tensor(per, dtype=torch.float32).repeat_interleave(torch.tensor(lengths)), dev)
        times, dts = evaluation_times(self.nfe, self.method, self.grid)
        err = self._error_state(lengths, return_error)
        self._integrate(ids_p, cond_p, y, ops.h2d(times, dev), dts, s, use_null, lengths=lengths, row_scale=row_scale, err=err)
        out = list(torch.split(y, lengths))
        return (out, self._solve_error(err, lengths)) if return_error else out
