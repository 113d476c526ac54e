"""HiFi-GAN generator on the MI355X kernels - drop-in for the reference `Generator`.

Mirrors covomix/vocoder/models.py:75-125 (Generator), :11-48 (ResBlock1) and
covomix/vocoder/env.py:5-8 (AttrDict) of the reference:

    h = AttrDict(json.load(open('vocoder_config.json')))
    generator = Generator(h).to(device)
    generator.load_state_dict(torch.load(ckpt)['generator'])      # weight_g / weight_v / bias
    generator.eval(); generator.remove_weight_norm()
    wav = generator(mel)            # mel [B,80,T] -> [B,1,160T+32];  [80,T] -> [1,160T+32]

Only resblock == '1' (what config_covomix.json selects) is implemented.  Each conv launch
fuses the preceding leaky_relu, bias, the ResBlock residual add and the running
`xs += resblock(x)` / `xs / num_kernels` of Generator.forward (models.py:104-110).

precision (constructor argument or env CVX_VOCODER_PRECISION):
  'f16x3' (default)  the ResBlock convolutions (97 % of the FLOPs) and, where the whole configuration fits, the ConvTranspose1d
                     upsamplers run on the fp16 matrix pipe with split-precision operands on channels-last activations with zero
                     halos; conv_pre and conv_post stay on the fp32 kernels.  `plan()` says which kernels a configuration gets;
  'fp32'             everything on v_mfma_f32_32x32x2_f32 (cvx_hifigan_conv1d_f32).
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Dict, Optional, Tuple

import torch

from . import ops

LRELU_SLOPE = 0.1   # models.py:8
PRESCALE_TARGET = 1024.0    # a split stage's pairs hold leaky_relu(x) * zs, zs the power of two that brings the measured max|x| to 2^10


class AttrDict(dict):
    """dict with attribute access (reference env.py:5-8)."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.__dict__ = self


def get_padding(kernel_size: int, dilation: int = 1) -> int:
    return int((kernel_size * dilation - dilation) / 2)     # vocoder/utils.py:34-35


def fold_weight_norm(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """weight = weight_v * weight_g / ||weight_v|| with the norm over every dim but 0
    (torch._weight_norm, dim=0 - per INPUT channel for ConvTranspose1d).  Load-time plumbing."""
    out: Dict[str, torch.Tensor] = {}
    for k, v in sd.items():
        if k.endswith(".weight_g"):
            base = k[: -len(".weight_g")]
            wv = sd[base + ".weight_v"].float()
            nrm = wv.reshape(wv.shape[0], -1).norm(dim=1).reshape(-1, *([1] * (wv.ndim - 1)))
            out[base + ".weight"] = wv * (v.float() / nrm)
        elif not k.endswith(".weight_v"):
            out[k] = v
    return out


# ---- which kernels a generator runs ---------------------------------------------------------
@dataclass(frozen=True)
class Stage:
    """One upsampling rate: ConvTranspose1d, then the ResBlocks summed into xs (models.py:102-110)."""
    channels: int
    rate: int
    ksize: int
    upsampler: str                  # 'split' | 'polyphase' | 'stuffed'
    resblocks: str                  # 'grouped' | 'blocks' | 'fp32'
    blocks: Tuple[str, ...]         # per ResBlock 'call' | 'pairs' | 'convs' ('grouped': the calls that share launches; 'fp32': empty)
    np: Optional[int]               # width of the stage's channels-last buffers = the kernels' tile width; None on an fp32 stage
    wide: bool                      # the stage keeps split pairs in HBM (np > ops.HIFI_NARROW_NP)
    mul: int                        # an item of T mel frames has mul * T + add positions behind this stage's upsampler
    add: int


@dataclass(frozen=True)
class Plan:
    pipeline: str                   # 'channels_last' | 'channel_major'
    stages: Tuple[Stage, ...]
    cp_in: Optional[int]            # channels-last pipeline: channel width of the first upsampler's input pair


def plan(h, precision: str, group_stages: bool = True) -> Plan:
    """Every choice of kernels a generator of configuration h makes, decided once (host arithmetic: no GPU, no library, no tensors).

      configuration property                                                          what it decides
      precision 'fp32'                                                                channel-major flow, every stage 'fp32'
      stage channels <= 256, every (k - 1) * dilation of the ResBlocks even, <= 50    the stage's ResBlocks on the split pipe
      ... of EVERY stage; last stage <= 64 channels; rates <= 8; 3 dilations a block  channels-last pipeline, 'split' upsamplers
      otherwise                                                                       channel-major flow: 'polyphase' upsamplers
                                                                                      (rate 1: 'stuffed'), converters around a split stage
      stage tile width np > 64                                                        wide: split pairs in HBM
      wide, 2 or 3 ResBlocks of 3 dilations, group_stages                             'grouped': one call for the stage
      otherwise, per ResBlock: 3 dilations / other counts, narrow / wide              'call' / 'pairs' / 'convs'
    """
    split_pipe = precision == "f16x3"
    rates, ksizes = list(h["upsample_rates"]), list(h["upsample_kernel_sizes"])
    dils = [list(d) for _, d in zip(h["resblock_kernel_sizes"], h["resblock_dilation_sizes"])]
    chans = [h["upsample_initial_channel"] // 2 ** (i + 1) for i in range(len(rates))]
    # cvx_hifigan_conv1d_f16x3 (include/covomix_hip.h) takes its 'same' padding of (k - 1) * dil / 2 zeros a side from the buffers' zero
    # halos: (k - 1) * dil even, and <= 50 - the activation tile it stages has 64 rows beyond its positions.  convs2 has dilation 1.
    reaches = [(k - 1) * d for k, ds in zip(h["resblock_kernel_sizes"], dils) for d in ds + [1]]
    taps_fit = all(r <= 50 and r % 2 == 0 for r in reaches)
    split_res = [split_pipe and taps_fit and c <= 256 for c in chans]           # 256: the widest tile (ops.hifigan_tile)
    # the stride-1 form computes `rate` phases per input row over L_in + 1 rows at most (1 <= k - 2 pad <= 2 rate), in up to 8 column
    # tiles of a whole number of phases (rate <= 8), 256 columns a phase at most
    split_up = [split_pipe and c <= 256 and u <= 8 and 1 <= k - 2 * ((k - u) // 2) <= 2 * u for c, u, k in zip(chans, rates, ksizes)]
    # channels-last from conv_pre to the waveform needs every upsampler and ResBlock on the split pipe, a last stage conv_post's
    # channels-last kernel can read (one tile of <= 64 channels), and the three-dilation blocks it was built and measured with
    cl = all(split_up) and all(split_res) and chans[-1] <= ops.HIFI_NARROW_NP and all(len(d) == 3 for d in dils)
    stages, mul, add = [], 1, 0                 # conv_pre (7 taps, padding 3) keeps the length
    for c, u, k, split in zip(chans, rates, ksizes, split_res):
        mul, add = mul * u, (add - 1) * u + k - 2 * ((k - u) // 2)             # ConvTranspose1d(stride u, padding (k - u) // 2), models.py:85-88
        upsampler = "split" if cl else "polyphase" if u > 1 else "stuffed"      # polyphase: 1 / rate of the zero-stuffed form's work
        if not split:
            stages.append(Stage(c, u, k, upsampler, "fp32", (), None, False, mul, add))
            continue
        np_ = ops.hifigan_tile(c)
        wide = np_ > ops.HIFI_NARROW_NP
        # one C call runs a ResBlock of three conv pairs (narrow: three fused kernels; wide: six convolutions); other dilation
        # counts go pair by pair through the fused kernel, or convolution by convolution where the stage is too wide for it
        blocks = tuple("call" if len(d) == 3 else "convs" if wide else "pairs" for d in dils)
        # the ResBlocks of a wide stage are independent until xs sums them: 2 or 3 of them share launches (cvx_hifigan_resblock_stage_
        # f16x3 takes up to 3 three-pair blocks; a narrow block is three launches already), bit-identical to block after block
        grouped = group_stages and wide and 2 <= len(blocks) <= 3 and all(b == "call" for b in blocks)
        stages.append(Stage(c, u, k, upsampler, "grouped" if grouped else "blocks", blocks, np_, wide, mul, add))
    c0 = h["upsample_initial_channel"]
    cp_in = (ops.hifigan_tile(c0) if c0 <= 256 else (c0 + 31) // 32 * 32) if cl else None    # (only the first upsampler reads > 256 channels)
    return Plan("channels_last" if cl else "channel_major", tuple(stages), cp_in)


# ---- buffers of one call shape ------------------------------------------------------------------
@dataclass
class StageBuffers:
    """Channels-last buffers [B, ops.hifigan_cl_rows(L), np] of one split stage; None where a stage has no such buffer."""
    L: int
    x0: torch.Tensor                # fp32 stage input (the upsampler's output)
    xs: torch.Tensor                # fp32 sum of the ResBlocks / num_kernels
    zs: torch.Tensor                # fp32[1]: pre-scale of the stage's pairs
    amax: torch.Tensor              # int32[1]: bit pattern of a measured max|x|; zero between its producer and consumer pairs
    scratch: tuple                  # dict(r0, r1, t, rz0, rz1) as ops.hifigan_resblock_f16x3 takes it (narrow: the pairs t, rz0, rz1 are None)
    z0: Optional[tuple]             # wide: split(leaky_relu(x0) * zs)
    zn: Optional[tuple]             # channels-last pipeline, not the last stage: the next upsampler's input pair
    zs_next: Optional[torch.Tensor]


@dataclass
class Workspace:
    stages: Tuple[Optional[StageBuffers], ...]      # None: an fp32 stage
    zin: Optional[tuple]            # channels-last pipeline: the first upsampler's input pair split(leaky_relu(conv_pre(mel)) * zs_in)
    zs_in: Optional[torch.Tensor]
    amax_in: Optional[torch.Tensor]


def workspace(p: Plan, B: int, T_in: int, device) -> Workspace:
    """All buffers of a call of B mels of T_in frames, zero-initialised ONCE: the kernels only ever write valid rows (zeros behind
    a shorter item's end, zeros into the padded channels), so halos and padding stay zero from call to call."""
    f32 = lambda shape: torch.zeros(shape, dtype=torch.float32, device=device)
    pair = lambda shape: (torch.zeros(shape, dtype=torch.float16, device=device), torch.zeros(shape, dtype=torch.float16, device=device))
    scale = lambda: torch.ones(1, dtype=torch.float32, device=device)
    amax = lambda: torch.zeros(1, dtype=torch.int32, device=device)
    cl = p.pipeline == "channels_last"
    stages = []
    for i, st in enumerate(p.stages):
        L = st.mul * T_in + st.add
        if st.resblocks == "fp32":
            stages.append(None)
            continue
        shape = (B, ops.hifigan_cl_rows(L), st.np)
        pairs = lambda: {k: pair(shape) if st.wide else None for k in ("t", "rz0", "rz1")}
        # blocks that share launches need scratch of their OWN; block after block, one set serves all
        scratch = tuple(dict(r0=f32(shape), r1=f32(shape), **pairs()) for _ in range(len(st.blocks) if st.resblocks == "grouped" else 1))
        feeds_next = cl and i + 1 < len(p.stages)
        zn = None if not feeds_next else scratch[0]["t"] if st.wide else pair(shape)     # (t is free once xs is complete)
        stages.append(StageBuffers(L, f32(shape), f32(shape), scale(), amax(), scratch, pair(shape) if st.wide else None,
                                   zn, scale() if feeds_next else None))
    if not cl:
        return Workspace(tuple(stages), None, None, None)
    return Workspace(tuple(stages), pair((B, ops.hifigan_cl_rows(T_in), p.cp_in)), scale(), amax())


WORKSPACE_SHAPES = 3    # call shapes (B, T) whose buffers a generator keeps; one more clears them


class Generator:
    def __init__(self, h, precision: Optional[str] = None, group_stages: bool = True):
        if str(h["resblock"]) != "1":
            raise NotImplementedError("only ResBlock1 (resblock == '1') is supported, as in config_covomix.json")
        self.precision = precision or os.environ.get("CVX_VOCODER_PRECISION", "f16x3")
        if self.precision not in ("f16x3", "fp32"):
            raise ValueError(f"vocoder precision must be 'f16x3' or 'fp32', got {self.precision!r}")
        self.group_stages = group_stages     # False: the ResBlocks of a wide stage block after block (same bits; tests compare)
        self.plan: Optional[Plan] = None
        self._ws: Dict[tuple, Workspace] = {}
        self.h = h
        self.num_kernels = len(h["resblock_kernel_sizes"])
        self.num_upsamples = len(h["upsample_rates"])
        self.device = torch.device("cpu")
        self._sd: Optional[Dict[str, torch.Tensor]] = None
        self._has_weight_norm = False
        self._packed = None
        self._fp32_twin: Optional["Generator"] = None       # built only if a split-precision call ever saturates

    # ---- nn.Module-like surface used by the reference scripts -------------------------
    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True):
        self._sd = {k: v.detach().to("cpu") for k, v in sd.items()}
        self._has_weight_norm = any(k.endswith(".weight_g") for k in self._sd)
        self._packed = self._fp32_twin = None
        return self

    def state_dict(self):
        return dict(self._sd or {})

    def eval(self):
        return self

    def to(self, device):
        device = torch.device(device)
        if device != self.device:
            self.device = device
            self._packed = self._fp32_twin = None
            self._ws.clear()
        return self

    def remove_weight_norm(self):
        print('Removing weight norm...')
        if self._has_weight_norm:
            self._sd = fold_weight_norm(self._sd)
            self._has_weight_norm = False
            self._packed = self._fp32_twin = None
        return self

    # ---- weight packing -----------------------------------------------------------------
    def _conv(self, name: str, form: str, dil: int = 1, pad: int = 0, up: int = 1, cp_in: Optional[int] = None) -> SimpleNamespace:
        """Pack one convolution the way the plan names: 'fp32' / 'f16x3' (Conv1d), 'split' / 'polyphase' / 'stuffed' (ConvTranspose1d)."""
        w = self._sd[name + ".weight"].float()
        transposed = form in ("split", "polyphase", "stuffed")
        c = SimpleNamespace(cout=w.shape[1 if transposed else 0], k=w.shape[2], dil=dil, up=up, padding=pad)
        c.pad = c.k - 1 - pad if transposed else pad        # transposed: stride-1 conv over the zero-stuffed input, flipped kernel
        c.bias = self._sd[name + ".bias"].float().to(self.device).contiguous()
        if form in ("fp32", "stuffed"):
            c.wp = ops.hifigan_pack_weight(w, transposed).to(self.device)
        elif form == "polyphase":
            c.wp_poly = ops.hifigan_pack_conv_transpose1d(w, up, pad).to(self.device)
        elif form == "split":                # (input = the Np-wide buffers of the stage before)
            c.w16t = ops.hifigan_pack_conv_transpose1d_f16x3(w.to(self.device), c.bias, up, pad, cp_in)
        else:
            c.w16 = ops.hifigan_pack_weight_f16x3(w.to(self.device))
            c.bias16 = torch.zeros(c.w16[3], dtype=torch.float32, device=self.device)
            c.bias16[: c.cout] = c.bias
        return c

    def pack(self) -> "Generator":
        """Fold weight norm and lay the weights out for the kernels NOW (otherwise the first forward does it - with host-to-device
        copies that wait behind whatever the stream is still running, e.g. the solve whose mel this call is about to vocode)."""
        if self._packed is None:
            self._pack()
        return self

    def _pack(self):
        if self._sd is None:
            raise RuntimeError("Generator: load_state_dict() has not been called")
        if self._has_weight_norm:
            # the reference can run with weight norm still attached (same function); fold on the fly
            self._sd = fold_weight_norm(self._sd)
            self._has_weight_norm = False
        if self.device.type != "cuda":
            raise ops._lib.CovomixHipError("Generator must be moved to a GPU (`.to('cuda')`): covomix_amd has no CPU path")
        h = self.h
        self.plan = plan(h, self.precision, self.group_stages)
        pk = dict(pre=self._conv("conv_pre", "fp32", pad=3), ups=[], res=[])
        cp_in = self.plan.cp_in
        for i, st in enumerate(self.plan.stages):
            pk["ups"].append(self._conv(f"ups.{i}", st.upsampler, pad=(st.ksize - st.rate) // 2, up=st.rate, cp_in=cp_in))
            form, cp_in = "fp32" if st.resblocks == "fp32" else "f16x3", st.np
            blocks = []
            for j, (rk, dils) in enumerate(zip(h["resblock_kernel_sizes"], h["resblock_dilation_sizes"])):
                p = f"resblocks.{i * self.num_kernels + j}"
                blocks.append([(self._conv(f"{p}.convs1.{m}", form, dil=d, pad=get_padding(rk, d)),
                                self._conv(f"{p}.convs2.{m}", form, dil=1, pad=get_padding(rk, 1)))
                               for m, d in enumerate(dils)])
            pk["res"].append(blocks)
        pk["post_w"] = self._sd["conv_post.weight"].float().reshape(-1, 7).contiguous().to(self.device)
        pk["post_b"] = float(self._sd["conv_post.bias"].float().reshape(-1)[0])
        if pk["pre"].k != 7 or [(c.cout, c.k) for c in pk["ups"]] != [(st.channels, st.ksize) for st in self.plan.stages]:
            raise ValueError("Generator: the weights' channel counts or kernel sizes are not the configuration's (the plan's buffer sizes)")
        self._packed = pk

    # ---- forward ------------------------------------------------------------------------
    def _run(self, c, x: torch.Tensor, out: Optional[torch.Tensor] = None, *, in_slope=1.0, res=None,
             accum=None, out_scale=1.0, items=None) -> torch.Tensor:
        B, _, lin = x.shape
        lout = (lin - 1) * c.up + 1 + 2 * c.pad - (c.k - 1) * c.dil
        if out is None:
            out = torch.empty(B, c.cout, lout, dtype=torch.float32, device=x.device)
        return ops.hifigan_conv1d(x, c.wp, c.bias, out, cout=c.cout, ksize=c.k, dil=c.dil, pad=c.pad, up=c.up,
                                  in_slope=in_slope, res=res, accum=accum, out_scale=out_scale, items=items)

    def output_length(self, frames: int) -> int:
        """Samples the generator returns for a mel of `frames` frames."""
        last = self.pack().plan.stages[-1]
        return last.mul * frames + last.add

    @ops.gated
    @torch.no_grad()
    def __call__(self, mel: torch.Tensor, lengths=None) -> torch.Tensor:
        """mel [B, 80, T] -> [B, 1, L]  ([80, T] -> [1, L]), models.py:100-116.
        lengths (extension, ragged batch): item b only has lengths[b] <= T valid frames (the rest of its mel must be zero
        padding); its first output_length(lengths[b]) samples are then exactly what a B = 1 call on its own frames returns
        (every kernel writes zeros behind a shorter item's end - the zero padding the B = 1 run sees there), the samples
        behind them are unspecified.  `ragged()` wraps the padding and slicing.
        The split-precision stages keep their activations within 2^6 of the measured max|x| of the stage input; when a
        ResBlock intermediate outgrows that, the kernels clamp and raise the device's sticky saturation flag
        (include/covomix_hip.h).  One flag read per call; a flagged call is re-run on the all-fp32 kernels (or raises:
        CVX_ON_SATURATION=raise) - never returned as is."""
        checked = self.precision != "fp32" and ops.saturation_checked() and self.device.type == "cuda"
        if not checked:
            return self._forward(mel, lengths)
        with torch.cuda.device(self.device):
            ops.saturation_reset()
            y = self._forward(mel, lengths)
            if not ops.saturation_query():
                return y
        msg = ("covomix_amd: the split-precision vocoder stages saturated (an intermediate left the fp16 window around the "
               "measured stage input)")
        if os.environ.get("CVX_ON_SATURATION", "fp32") == "raise":
            raise ops._lib.CovomixHipError(msg + " (CVX_ON_SATURATION=raise)")
        import warnings
        warnings.warn(msg + "; re-running this call on the all-fp32 kernels")
        if self._fp32_twin is None:
            twin = Generator(self.h, precision="fp32").to(self.device)
            twin._sd, twin._has_weight_norm = self._sd, self._has_weight_norm
            self._fp32_twin = twin
        return self._fp32_twin._forward(mel, lengths)

    @torch.no_grad()
    def ragged(self, mels) -> list:
        """mels: list of [80, T_b] tensors of different length -> list of [1, L_b] waveforms from ONE batched call (each
        equal to generator(mels[b]) up to fp32 summation order)."""
        if not mels:
            return []
        T = [int(m.shape[-1]) for m in mels]
        pad = torch.zeros(len(mels), mels[0].shape[0], max(T), dtype=torch.float32, device=self.device)
        for b, m in enumerate(mels):
            pad[b, :, : T[b]] = m
        y = self(pad, lengths=T) if len(set(T)) > 1 else self(pad)
        return [y[b, :, : self.output_length(T[b])] for b in range(len(mels))]

    def _forward(self, mel: torch.Tensor, lengths=None) -> torch.Tensor:
        pk = self.pack()._packed
        unbatched = mel.ndim == 2
        x = mel.to(device=self.device, dtype=torch.float32)
        if unbatched:
            x = x.unsqueeze(0)
        x = x.contiguous()
        B, _, T = x.shape
        lens = None
        if lengths is not None:
            if len(lengths) != B or min(lengths) < 1 or max(lengths) > T:
                raise ValueError(f"lengths must hold one frame count in [1, {T}] per batch item")
            lens = ops.h2d(torch.tensor([int(t) for t in lengths], dtype=torch.int32), self.device)
        items = lambda mul, add: None if lens is None else (lens, mul, add)      # item b is valid on mul * lengths[b] + add positions
        ws = self._ws.get((B, T))
        if ws is None:
            if len(self._ws) >= WORKSPACE_SHAPES:
                self._ws.clear()
            ws = self._ws[(B, T)] = workspace(self.plan, B, T, self.device)
        x = self._run(pk["pre"], x, items=items(1, 0))
        run = self._channels_last if self.plan.pipeline == "channels_last" else self._channel_major
        y = run(pk, ws, x, [items(st.mul, st.add) for st in self.plan.stages])
        return y.squeeze(0) if unbatched else y

    forward = __call__

    def _channel_major(self, pk, ws: Workspace, x: torch.Tensor, items) -> torch.Tensor:
        """Upsamplers on the fp32 kernels, channel-major; a split stage sits between two layout converters, an fp32 stage stays
        channel-major throughout."""
        B, _, T = x.shape
        for i, (st, sb) in enumerate(zip(self.plan.stages, ws.stages)):
            up, split = pk["ups"][i], st.resblocks != "fp32"
            if st.upsampler == "polyphase":                                 # leaky_relu + ConvTranspose1d; leaves max|out| for a split stage
                y = torch.empty(B, st.channels, st.mul * T + st.add, dtype=torch.float32, device=x.device)
                x = ops.hifigan_conv_transpose1d(x, up.wp_poly, up.bias, y, cout=up.cout, ksize=up.k, stride=up.up, padding=up.padding,
                                                 in_slope=LRELU_SLOPE, amax_bits=sb.amax if split else None, items=items[i])
            else:
                x = self._run(up, x, in_slope=LRELU_SLOPE, items=items[i])
            if not split:
                x = self._resblocks_fp32(pk["res"][i], x, items[i])
                continue
            if st.upsampler == "polyphase":
                zs = ops.pow2_scale_from_amax(sb.amax, PRESCALE_TARGET, sb.zs)
            else:
                zs = ops.amax_pow2_scale(x, PRESCALE_TARGET, sb.zs, sb.amax)
            ops.hifigan_to_channels_last(x, sb.x0, sb.z0, LRELU_SLOPE, z_scale=zs)
            self._resblocks(st, pk["res"][i], sb, B, zs, items[i])
            x = ops.hifigan_from_channels_last(sb.xs, torch.empty_like(x))
        y = torch.empty(B, 1, x.shape[2], dtype=torch.float32, device=x.device)
        return ops.hifigan_post(x, pk["post_w"], pk["post_b"], y, slope=0.01)       # F.leaky_relu default slope (:112)

    def _channels_last(self, pk, ws: Workspace, x: torch.Tensor, items) -> torch.Tensor:
        """Everything behind conv_pre on channels-last buffers: per stage
            ConvTranspose1d on the split pipe (stride-1 form; leaves max|out| on the device) -> fp32 x0
            -> [wide stages] z0 = split(leaky_relu(x0) * zs)  -> the ResBlocks -> xs
            -> max|xs| -> the next upsampler's input pair split(leaky_relu(xs) * zs'),
        then conv_post + tanh straight from the last xs.  No channel-major tensor exists between conv_pre and the waveform."""
        B, _, lin = x.shape
        cur_z, cur_zs = ws.zin, ops.amax_pow2_scale(x, PRESCALE_TARGET, ws.zs_in, ws.amax_in)
        ops.hifigan_to_channels_last(x, None, cur_z, LRELU_SLOPE, z_scale=cur_zs)
        for i, (st, sb) in enumerate(zip(self.plan.stages, ws.stages)):
            ops.hifigan_conv_transpose1d_f16x3(cur_z, pk["ups"][i].w16t, B, lin, sb.x0, sb.L, z_scale=cur_zs, amax_bits=sb.amax, items=items[i])
            zs = ops.pow2_scale_from_amax(sb.amax, PRESCALE_TARGET, sb.zs)
            if st.wide:
                ops.hifigan_split_channels_last(sb.x0, sb.z0, LRELU_SLOPE, z_scale=zs)
            self._resblocks(st, pk["res"][i], sb, B, zs, items[i])
            if sb.zn is not None:
                cur_zs = ops.amax_pow2_scale(sb.xs, PRESCALE_TARGET, sb.zs_next, sb.amax)
                ops.hifigan_split_channels_last(sb.xs, sb.zn, LRELU_SLOPE, z_scale=cur_zs)
                cur_z, lin = sb.zn, sb.L
        y = torch.empty(B, 1, sb.L, dtype=torch.float32, device=x.device)
        return ops.hifigan_post_channels_last(sb.xs, st.channels, sb.L, pk["post_w"], pk["post_b"], y, slope=0.01)

    # ---- the ResBlocks of one stage: xs = sum_j ResBlock1_j(x) / num_kernels  (models.py:104-110, :35-42) ------------------
    def _fold(self, j: int, n: int, xs: torch.Tensor, last: bool = True) -> tuple:
        """(accum, out_scale) of a convolution of block j of n: the LAST one of a block adds to xs (from the second block on) and the
        last block's divides by num_kernels; the others write a block's intermediate."""
        return (xs if last and j > 0 else None), (1.0 / self.num_kernels if last and j == n - 1 else 1.0)

    def _resblocks_fp32(self, blocks, x: torch.Tensor, items) -> torch.Tensor:
        t, r, xs = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
        for j, block in enumerate(blocks):
            cur = x
            for m, (c1, c2) in enumerate(block):
                last = m + 1 == len(block)
                accum, out_scale = self._fold(j, len(blocks), xs, last)
                self._run(c1, cur, t, in_slope=LRELU_SLOPE, items=items)
                cur = self._run(c2, t, xs if last else r, in_slope=LRELU_SLOPE, res=cur, accum=accum, out_scale=out_scale, items=items)
        return xs

    def _resblocks(self, st: Stage, blocks, sb: StageBuffers, B: int, zs, items) -> None:
        """sb.xs from sb.x0 (fp32) and, on a wide stage, sb.z0 = split(leaky_relu(x0) * zs): all channels-last."""
        n, L = len(blocks), sb.L
        if st.resblocks == "grouped":           # 18 -> 8 launches per stage
            ops.hifigan_resblock_stage_f16x3(sb.x0, sb.z0, blocks, B, L, sb.scratch, sb.xs, out_scale=self._fold(n - 1, n, sb.xs)[1],
                                             z_scale=zs, items=items)
            return
        s = sb.scratch[0]
        for j, (form, block) in enumerate(zip(st.blocks, blocks)):
            if form == "call":                  # cvx_hifigan_resblock_f16x3: 6 launches, or 3 fused pairs
                accum, out_scale = self._fold(j, n, sb.xs)
                ops.hifigan_resblock_f16x3(sb.x0, sb.z0, block, B, L, s, accum=accum, out=sb.xs, out_scale=out_scale, z_scale=zs, items=items)
                continue
            cur_x, cur_z = sb.x0, sb.z0
            for m, (c1, c2) in enumerate(block):
                last = m + 1 == len(block)
                accum, out_scale = self._fold(j, n, sb.xs, last)
                out_x, out_z = (sb.xs, None) if last else (s["r0"], s["rz0"]) if m % 2 == 0 else (s["r1"], s["rz1"])
                if form == "pairs":
                    ops.hifigan_resblock_pair_f16x3(cur_x, c1, c2, B, L, out_x, accum=accum, out_scale=out_scale, z_scale=zs, items=items)
                else:
                    ops.hifigan_conv1d_f16x3(cur_z, c1.w16, c1.bias16, B, L, ksize=c1.k, dil=c1.dil, out_z=s["t"], z_slope=LRELU_SLOPE,
                                             z_scale=zs, items=items)
                    ops.hifigan_conv1d_f16x3(s["t"], c2.w16, c2.bias16, B, L, ksize=c2.k, dil=c2.dil, res=cur_x, accum=accum, out_x=out_x,
                                             out_scale=out_scale, out_z=out_z, z_slope=LRELU_SLOPE, z_scale=zs, items=items)
                cur_x, cur_z = out_x, out_z


def mel_decode_to_wav(generator: Generator, mel: torch.Tensor):
    """reference monologue_generation.py:52-59: generator(mel) -> squeeze -> *32768 -> int16 numpy."""
    y = generator(mel)
    pcm = ops.wav_to_int16(y.squeeze().contiguous())
    return pcm.cpu().numpy()
