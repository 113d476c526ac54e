"""Prompt mel extraction on the GPU - SURVEY.md section 8f row N3.

Host mirror of `extract_mel` / `mel_spectrogram` (monologue_generation.py:62-74, data_preparation/generate_mel.py:49-72 =
hifi-gan/meldataset.py:49-72), parameterised like the reference function by (sr, n_fft, hop, win, n_mels, fmin, fmax); the
defaults are the constants the generation scripts set (monologue_generation.py:349-357): 8 kHz, n_fft = win = 480,
hop 160, 80 mel bins, fmin 0, fmax 4000.

    mel = extract_mel(wav)          # wav float32 [n] in [-1, 1], or a wav file of any rate / sample type -> [80, n // 160]

The STFT is not an FFT here: with an n_fft-sample window and n_fft/2+1 bins it is a [T, n_fft] x [n_fft, 2*bins] matrix
product, i.e. one call of the fp32 MFMA GEMM on the reflect-padded signal viewed as overlapping rows (row stride = hop),
with the hann window folded into the cos | sin basis; magnitude, the mel projection (second GEMM) and log(clamp) follow.

The mel basis is `librosa.filters.mel` in the reference (third-party, not in this image): `slaney_mel_basis` restates its
published algorithm (Slaney scale, slaney normalisation).  PINNED: tests/golden/mel_ref_16k.npz holds two wav -> mel pairs
written by the reference's own function (16 kHz / 1024 / 256 / fmax 8000); this module reproduces them to <= 5e-5 on the
log-mel (tests/test_mel_gpu.py), the CPU oracle to 1e-6.  Files at another rate than `sr` are resampled on the GPU
(cvx_resample_fir_f32, windowed sinc; the reference calls librosa.load(sr=8000) - third-party, unpinned).

Many prompts of different lengths and source rates in ONE call (opt-in; the reference has no counterpart, and the functions above stay
the route for one prompt): mel_spectrogram_many / extract_mel_many through cvx_mel_spectrogram_many_f32 - one upload, one launch
sequence over a packed buffer, one download; every item bit-identical to extract_mel's (second half of this file).
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib, ops

SR, N_FFT, HOP, WIN, N_MELS, FMIN, FMAX = 8000, 480, 160, 480, 80, 0.0, 4000.0

def _hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    f_sp, min_log_hz, logstep = 200.0 / 3, 1000.0, math.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_hz / f_sp + np.log(np.maximum(f, 1e-10) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    f_sp, min_log_hz, logstep = 200.0 / 3, 1000.0, math.log(6.4) / 27.0
    min_log_mel = min_log_hz / f_sp
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def slaney_mel_basis(sr: int = SR, n_fft: int = N_FFT, n_mels: int = N_MELS, fmin: float = FMIN, fmax: float = FMAX) -> np.ndarray:
    """[n_mels, n_fft // 2 + 1] float32: librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax) with its defaults
    (Slaney mel scale, triangular filters on the FFT bin frequencies, norm='slaney')."""
    fftfreqs = np.linspace(0.0, sr / 2.0, n_fft // 2 + 1)
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fftfreqs[None, :]
    w = np.zeros((n_mels, n_fft // 2 + 1))
    for i in range(n_mels):
        w[i] = np.maximum(0.0, np.minimum(-ramps[i] / fdiff[i], ramps[i + 2] / fdiff[i + 1]))
    return (w * (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]).astype(np.float32)


_CONST: Dict[tuple, tuple] = {}


def _constants(device: torch.device, sr: int, n_fft: int, win: int, n_mels: int, fmin: float, fmax: float):
    key = (device, sr, n_fft, win, n_mels, float(fmin), float(fmax))
    c = _CONST.get(key)
    if c is None:
        if win != n_fft:
            raise NotImplementedError("mel_spectrogram: win_size must equal n_fft (every caller of the reference does)")
        nb = n_fft // 2 + 1
        nbp = (nb + 3) // 4 * 4                                        # K of the mel GEMM padded to a multiple of 4
        n = torch.arange(n_fft, dtype=torch.float64)
        k = torch.arange(nb, dtype=torch.float64)
        ang = (2.0 * math.pi / n_fft) * k[:, None] * n[None, :]
        w = torch.hann_window(win, dtype=torch.float64)
        dft = torch.cat((torch.cos(ang) * w, torch.sin(ang) * w), dim=0).float().contiguous().to(device)      # [2*nb, n_fft]
        basis = torch.zeros(n_mels, nbp, dtype=torch.float32)
        basis[:, :nb] = torch.from_numpy(slaney_mel_basis(sr, n_fft, n_mels, fmin, fmax))
        if len(_CONST) >= 8:
            _CONST.clear()
        c = _CONST[key] = (dft, basis.to(device), nb, nbp)
    return c


@torch.no_grad()
def mel_spectrogram(y: torch.Tensor, n_fft: int = N_FFT, num_mels: int = N_MELS, sampling_rate: int = SR, hop_size: int = HOP,
                    win_size: int = WIN, fmin: float = FMIN, fmax: float = FMAX, center: bool = False) -> torch.Tensor:
    """y [B, n] or [n] float32 in [-1, 1] on the GPU -> [B, num_mels, T] (or [num_mels, T]) log-mel, T = n // hop_size.
    Argument names and order follow the reference function (generate_mel.py:49)."""
    if y.device.type != "cuda":
        raise _lib.CovomixHipError("mel_spectrogram needs the waveform on a GPU: covomix_amd has no CPU path")
    if center:
        raise NotImplementedError("center=True is not used by the reference's callers")
    if n_fft % 4 or (n_fft - hop_size) % 2 or hop_size % 4:
        raise ValueError("mel_spectrogram: n_fft and hop_size must be multiples of 4 (16-byte aligned overlapping rows)")
    single = y.ndim == 1
    y = (y[None] if single else y).to(torch.float32)
    dft, basis, nb, nbp = _constants(y.device, int(sampling_rate), int(n_fft), int(win_size), int(num_mels), fmin, fmax)
    pad = int((n_fft - hop_size) / 2)
    yr = torch.nn.functional.pad(y[:, None], (pad, pad), mode="reflect")[:, 0]                    # index plumbing only
    yp = torch.zeros(yr.shape[0], (yr.shape[1] + 3) // 4 * 4, dtype=torch.float32, device=y.device)      # 16-byte aligned rows
    yp[:, : yr.shape[1]] = yr
    n_pad = yr.shape[1]
    out = []
    st = ops._stream()
    for b in range(yp.shape[0]):
        sig = yp[b]
        T = (n_pad - n_fft) // hop_size + 1
        frames = sig.as_strided((T, n_fft), (hop_size, 1))             # overlapping rows: frame t = sig[hop t : hop t + n_fft]
        spec = torch.empty(T, 2 * nb, dtype=torch.float32, device=y.device)
        ops.gemm(frames, dft, spec)
        mag = torch.empty(T, nbp, dtype=torch.float32, device=y.device)
        _lib.check(_lib.load().cvx_mel_magnitude_f32(spec.data_ptr(), mag.data_ptr(), T, nb, nbp, st), "cvx_mel_magnitude_f32")
        proj = torch.empty(T, num_mels, dtype=torch.float32, device=y.device)
        ops.gemm(mag, basis, proj)
        mel = torch.empty(num_mels, T, dtype=torch.float32, device=y.device)
        _lib.check(_lib.load().cvx_mel_log_transpose_f32(proj.data_ptr(), mel.data_ptr(), T, num_mels, st), "cvx_mel_log_transpose_f32")
        out.append(mel)
    return out[0] if single else torch.stack(out)


def extract_mel(x: Union[str, np.ndarray, torch.Tensor], device: Union[str, torch.device] = "cuda", channel_idx=None,
                sr: int = SR, **mel_kw) -> torch.Tensor:
    """monologue_generation.py:62-74: wav -> (mono, `sr` Hz) -> clip to [-1, 1] -> mel_spectrogram -> [80, T] on the CPU.
    A path may be a wav file of any sample rate and PCM type: samples are converted to float by their stored type, the
    channel is selected (channel_idx) or the channels averaged (librosa.load's mono=True), and other rates are resampled
    to `sr` on the GPU with the windowed-sinc FIR the HuBERT reader uses."""
    if isinstance(x, str):
        from .audio import read_wav
        file_sr, data = read_wav(x)
        if data.ndim == 2:
            data = data[:, channel_idx] if channel_idx is not None else data.mean(axis=1, dtype=np.float32)
        wav = torch.from_numpy(np.ascontiguousarray(data, dtype=np.float32)).to(device)
        if file_sr != sr:
            from .hubert import resample
            wav = resample(wav, file_sr, sr)
    else:
        wav = x.detach() if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x, dtype=np.float32))
        wav = wav.to(device=device, dtype=torch.float32)
    return mel_spectrogram(wav.clamp(-1.0, 1.0), sampling_rate=sr, **mel_kw).cpu()


# ---------------------------------------------------------------------------------------------------------------------------
# Many prompts of different lengths (and source rates) in ONE call - opt-in; the functions above are the route for one prompt.
# cvx_mel_spectrogram_many_f32 (include/covomix_hip.h, "MANY PROMPTS IN ONE CALL"): the reflect-padded, clamped signals are packed
# into one buffer by one launch (which also resamples the items that name a filter bank), the DFT and the mel projection run once
# over all rows, and the items' own frames are gathered into one packed output.  An item's mel is bit for bit extract_mel's.

DEFAULT_MAX_BATCH_SAMPLES = 2_560_000       # packed floats of one ragged call: thirty-two 10-s prompts at 8 kHz (extract_mel_many)
MAX_BANKS = 16                              # source rates other than `sr` in one call (cvx_mel_items_fill)

_WS: Dict[torch.device, torch.Tensor] = {}          # workspace of the ragged call per device, grown on demand
_BANKS: Dict[tuple, object] = {}                    # (rates, sr) -> (geometry int32 [n, 3], taps); (device, rates, sr) -> taps on the device
_STAGE: Dict[str, torch.Tensor] = {}                # the pinned staging buffer of extract_mel_many's uploads


class MelItemTable:
    """The item table of a ragged mel call: int32 words filled by cvx_mel_items_fill on the host, with named views.
    Host arithmetic only - no GPU needed."""

    HEADER, ITEM, BANK = 16, 8, 4

    def __init__(self, words: np.ndarray):
        self.words = words
        (_magic, self.n, self.n_fft, self.hop, self.pad, self.rows, self.M, self.max_T, self.packed_floats, self.raw_floats,
         self.n_banks, self.bank_floats) = (int(v) for v in words[:12])
        end = self.HEADER + self.ITEM * self.n
        assert words.size == end + self.BANK * self.n_banks
        items = words[self.HEADER:end].reshape(self.n, self.ITEM)
        self.raw_off, self.n_raw, self.samples, self.slot, self.frames, self.cu, self.bank = (items[:, i] for i in range(7))
        self.banks = words[end:].reshape(self.n_banks, self.BANK)           # up, down, width, offset into the taps
        self.offsets = self.slot.astype(np.int64) * self.hop                # S_b, in floats of the packed buffer


def mel_item_table(n_raw: Sequence[int], bank: Optional[Sequence[int]] = None, bank_geom: Optional[Sequence[Sequence[int]]] = None,
                   n_fft: int = N_FFT, hop: int = HOP) -> MelItemTable:
    """Item table for stored signals of `n_raw` samples; bank[b] >= 0 names the (up, down, width) triple of `bank_geom` item b is
    resampled with (-1 / bank=None: the samples are at the target rate).  Raises CovomixHipError for an illegal batch (no items,
    a geometry mel_spectrogram refuses, an item of at most (n_fft - hop) / 2 samples at the target rate, sizes beyond int32)."""
    lib = _lib.load()
    n = len(n_raw)
    ns = np.ascontiguousarray(n_raw, dtype=np.int64)
    bk = np.ascontiguousarray(bank if bank is not None else [-1] * n, dtype=np.int32)
    geom = np.ascontiguousarray(bank_geom if bank_geom is not None else np.zeros((0, 3)), dtype=np.int32).reshape(-1, 3)
    assert bk.size == n
    args = (int(n_fft), int(hop), ns.ctypes.data, bk.ctypes.data, geom.ctypes.data if len(geom) else None, len(geom), n)
    words = int(lib.cvx_mel_items_words(*args)) if n else -1
    if words < 0:
        raise _lib.CovomixHipError(f"cvx_mel_items_words: {n} items of {list(n_raw)[:8]}{'...' if n > 8 else ''} samples are not a legal "
                                   f"batch for n_fft {n_fft}, hop {hop}")
    table = np.zeros(words, dtype=np.int32)
    _lib.check(lib.cvx_mel_items_fill(*args, table.ctypes.data, words), "cvx_mel_items_fill")
    return MelItemTable(table)


def split_batches(lengths: Sequence[int], max_batch_samples: int, n_fft: int = N_FFT, hop: int = HOP) -> List[List[int]]:
    """Indices of `lengths` (samples at the target rate) in order, cut into consecutive groups whose PACKED size (every item reflect
    padded and rounded up to the hop) stays within max_batch_samples; an item larger than the budget forms a group of its own."""
    pad = (n_fft - hop) // 2
    groups, cur, used = [], [], 0
    for i, n in enumerate(lengths):
        size = -(-(int(n) + 2 * pad) // hop) * hop
        if cur and used + size > max_batch_samples:
            groups.append(cur)
            cur, used = [], 0
        cur.append(i)
        used += size
    if cur:
        groups.append(cur)
    return groups


def _check_geometry(n_fft: int, hop_size: int, win_size: int, center: bool):
    if center:
        raise NotImplementedError("center=True is not used by the reference's callers")
    if win_size != n_fft:
        raise NotImplementedError("mel_spectrogram: win_size must equal n_fft (every caller of the reference does)")
    if n_fft % 4 or (n_fft - hop_size) % 2 or hop_size % 4 or hop_size > n_fft or hop_size <= 0:
        raise ValueError("mel_spectrogram: n_fft and hop_size must be multiples of 4 (16-byte aligned overlapping rows)")


def _check_lengths(lengths: Sequence[int], pad: int, what: str, names=None):
    for b, n in enumerate(lengths):
        if n <= pad:
            who = f"item {b}" + (f" ({names[b]})" if names is not None and isinstance(names[b], str) else "")
            raise ValueError(f"{what}: {who} has {n} samples at the target rate, the reflect padding of {pad} needs more")


def _cuda_device(device) -> torch.device:
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.CovomixHipError("the prompt mel needs a GPU: covomix_amd has no CPU path")
    return device if device.index is not None else torch.device("cuda", torch.cuda.current_device())


def _run_many(tab: MelItemTable, items_dev: torch.Tensor, raw_dev: torch.Tensor, banks_dev: Optional[torch.Tensor], device: torch.device,
              n_fft: int, num_mels: int, sampling_rate: int, win_size: int, fmin: float, fmax: float) -> torch.Tensor:
    """The C call on uploaded operands -> the packed output [num_mels * M] on the device."""
    lib = _lib.load()
    dft, basis, _nb, _nbp = _constants(device, int(sampling_rate), int(n_fft), int(win_size), int(num_mels), fmin, fmax)
    out = torch.empty(num_mels * tab.M, dtype=torch.float32, device=device)
    need = int(lib.cvx_mel_workspace_bytes_many(tab.words.ctypes.data, tab.words.size, tab.n, num_mels))
    if need < 0:
        _lib.check(-22, "cvx_mel_workspace_bytes_many")
    ws = _WS.get(device)
    if ws is None or ws.numel() < need:
        _WS.pop(device, None)                                       # release before growing
        ws = _WS[device] = torch.empty(max(need, 256), dtype=torch.uint8, device=device)
    _lib.check(lib.cvx_mel_spectrogram_many_f32(raw_dev.data_ptr(), None if banks_dev is None else banks_dev.data_ptr(), dft.data_ptr(),
                                                basis.data_ptr(), num_mels, tab.words.ctypes.data, items_dev.data_ptr(), tab.words.size,
                                                tab.n, out.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream()),
               "cvx_mel_spectrogram_many_f32")
    return out


def _views(out: torch.Tensor, tab: MelItemTable, num_mels: int) -> List[torch.Tensor]:
    return [out[num_mels * int(tab.cu[b]): num_mels * (int(tab.cu[b]) + int(tab.frames[b]))].view(num_mels, int(tab.frames[b]))
            for b in range(tab.n)]


@torch.no_grad()
def mel_spectrogram_many(wavs: Sequence[torch.Tensor], n_fft: int = N_FFT, num_mels: int = N_MELS, sampling_rate: int = SR,
                         hop_size: int = HOP, win_size: int = WIN, fmin: float = FMIN, fmax: float = FMAX,
                         center: bool = False) -> List[torch.Tensor]:
    """mel_spectrogram of every 1-D float32 GPU waveform in `wavs` (any lengths) from ONE C call -> list of [num_mels, T_b] GPU
    tensors in input order, views of one packed output, each bit-identical to mel_spectrogram(wav_b) for wav_b in [-1, 1] (the
    packing clamps to that range, as extract_mel does in front of mel_spectrogram).  T_b = 0 for a padded item shorter than
    n_fft; ValueError for an item of at most (n_fft - hop_size) / 2 samples (its reflection is undefined)."""
    wavs = list(wavs)
    _check_geometry(n_fft, hop_size, win_size, center)
    if not wavs:
        return []
    for b, w in enumerate(wavs):
        if not isinstance(w, torch.Tensor) or w.device.type != "cuda":
            raise _lib.CovomixHipError(f"mel_spectrogram_many needs every waveform on a GPU (item {b}): covomix_amd has no CPU path")
        if w.ndim != 1:
            raise ValueError(f"mel_spectrogram_many: item {b} is not 1-D")
    device = wavs[0].device
    _check_lengths([w.numel() for w in wavs], (n_fft - hop_size) // 2, "mel_spectrogram_many")
    tab = mel_item_table([w.numel() for w in wavs], n_fft=n_fft, hop=hop_size)
    raw = torch.empty(tab.raw_floats, dtype=torch.float32, device=device)
    for w, o in zip(wavs, tab.raw_off):
        raw[int(o):int(o) + w.numel()] = w.to(device=device, dtype=torch.float32)
    items_dev = ops.h2d(torch.from_numpy(tab.words), device)
    out = _run_many(tab, items_dev, raw, None, device, n_fft, num_mels, sampling_rate, win_size, fmin, fmax)
    return _views(out, tab, num_mels)


def _banks_host(rates: tuple, sr: int):
    """Filter banks of the source rates `rates` -> (geometry int32 [n, 3] = up, down, width per rate; their taps one after the other).
    Cached: a run's prompts come at a handful of rates."""
    key = (rates, sr)
    c = _BANKS.get(key)
    if c is None:
        from .hubert import sinc_resample_kernel
        geom, taps = [], []
        for r in rates:
            kern, width, orig, new = sinc_resample_kernel(r, sr)
            geom.append((new, orig, width))
            taps.append(kern.reshape(-1))
        if len(_BANKS) >= 16:
            _BANKS.clear()
        c = _BANKS[key] = (np.asarray(geom, dtype=np.int32).reshape(-1, 3), np.concatenate(taps))
    return c


def _banks_dev(device: torch.device, rates: tuple, sr: int) -> torch.Tensor:
    key = (device, rates, sr)
    c = _BANKS.get(key)
    if c is None:
        c = _BANKS[key] = ops.h2d(torch.from_numpy(_banks_host(rates, sr)[1]), device)
    return c


def _staging(words: int) -> torch.Tensor:
    """`words` int32 of PINNED host memory for an upload, cut from one buffer that is kept and grown on demand (pinning costs more than
    the copy).  The caller is done with it before it returns: every call ends in a blocking copy of its result."""
    buf = _STAGE.get("host")
    if buf is None or buf.numel() < words:
        _STAGE.pop("host", None)
        buf = _STAGE["host"] = torch.empty(max(words, 1 << 16), dtype=torch.int32, pin_memory=True)
    return buf[:words]


def _load_source(x, channel_idx, sr: int):
    """extract_mel's host side: -> (float32 samples [n], their rate)."""
    if isinstance(x, str):
        from .audio import read_wav
        file_sr, data = read_wav(x)
        if data.ndim == 2:
            data = data[:, channel_idx] if channel_idx is not None else data.mean(axis=1, dtype=np.float32)
        return np.ascontiguousarray(data, dtype=np.float32), int(file_sr)
    data = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return np.ascontiguousarray(data, dtype=np.float32).reshape(-1), int(sr)


@torch.no_grad()
def extract_mel_many(sources: Sequence[Union[str, np.ndarray, torch.Tensor]], device: Union[str, torch.device] = "cuda", channel_idx=None,
                     sr: int = SR, max_batch_samples: int = DEFAULT_MAX_BATCH_SAMPLES, **mel_kw) -> List[torch.Tensor]:
    """extract_mel of every entry of `sources` (wav paths of any rate / sample type, or arrays at `sr`) -> list of [num_mels, T_b] CPU
    tensors in input order, each bit-identical to extract_mel(entry).  channel_idx: one value for all entries or one per entry.
    File handling is extract_mel's (read_wav, channel select or mean on the host); the raw samples of up to max_batch_samples
    packed floats go up in ONE copy together with the item table, files at another rate are resampled inside the packing launch,
    and all mels of a call come back in ONE copy (views of it are returned).  Longer lists are cut by split_batches."""
    sources = list(sources)
    kw = dict(n_fft=N_FFT, num_mels=N_MELS, hop_size=HOP, win_size=WIN, fmin=FMIN, fmax=FMAX, center=False)
    unknown = set(mel_kw) - set(kw)
    if unknown:
        raise TypeError(f"extract_mel_many: unexpected keyword(s) {sorted(unknown)}")
    kw.update(mel_kw)
    n_fft, hop, num_mels = int(kw["n_fft"]), int(kw["hop_size"]), int(kw["num_mels"])
    _check_geometry(n_fft, hop, int(kw["win_size"]), bool(kw["center"]))
    if not sources:
        return []
    if torch.device(device).type != "cuda":
        raise _lib.CovomixHipError("extract_mel_many needs a GPU: covomix_amd has no CPU path")
    per_entry = isinstance(channel_idx, (list, tuple, np.ndarray))
    if per_entry and len(channel_idx) != len(sources):
        raise ValueError(f"extract_mel_many: {len(channel_idx)} channel indices for {len(sources)} sources")
    loaded = [_load_source(x, channel_idx[i] if per_entry else channel_idx, sr) for i, x in enumerate(sources)]
    rates = tuple(dict.fromkeys(r for _, r in loaded if r != sr))
    if len(rates) > MAX_BANKS:
        raise ValueError(f"extract_mel_many: {len(rates)} different source rates in one list (at most {MAX_BANKS})")
    geom = _banks_host(rates, sr)[0] if rates else None
    bank = [rates.index(r) if r != sr else -1 for _, r in loaded]
    lengths = [len(d) if k < 0 else -(-int(geom[k][0]) * len(d) // int(geom[k][1])) for (d, _), k in zip(loaded, bank)]
    _check_lengths(lengths, (n_fft - hop) // 2, "extract_mel_many", sources)
    device = _cuda_device(device)
    taps_dev = _banks_dev(device, rates, sr) if rates else None
    result: List[Optional[torch.Tensor]] = [None] * len(sources)
    for group in split_batches(lengths, max_batch_samples, n_fft, hop):
        tab = mel_item_table([len(loaded[i][0]) for i in group], [bank[i] for i in group], geom, n_fft, hop)
        head = (tab.words.size + 3) // 4 * 4                        # table | samples in one staging buffer: one upload
        stage = _staging(head + tab.raw_floats)
        sn = stage.numpy()
        sn[:tab.words.size] = tab.words
        sf = sn[head:].view(np.float32)
        for i, o in zip(group, tab.raw_off):
            sf[int(o):int(o) + len(loaded[i][0])] = loaded[i][0]
        dev = stage.to(device, non_blocking=True)
        out = _run_many(tab, dev[:tab.words.size], dev[head:].view(torch.float32), taps_dev, device, n_fft, num_mels, sr,
                        int(kw["win_size"]), kw["fmin"], kw["fmax"])
        for i, m in zip(group, _views(out.cpu(), tab, num_mels)):
            result[i] = m
    return result
