"""Python / numpy restatement of the ragged prompt-mel call's host side (include/covomix_hip.h, "MANY PROMPTS IN ONE CALL"):
the item table cvx_mel_items_fill writes, and the packed buffer cvx_mel_pack_f32 writes.  Shared by test_mel_many.py (CPU) and
test_mel_many_gpu.py; written from the header's description, not from the C code."""
import math

import numpy as np

MAGIC = 0x4D454C31
HEADER, ITEM, BANK = 16, 8, 4
INT32 = 1 << 31


def bank_geometry(orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99):
    """(up, down, width) of the polyphase filter bank that converts orig_freq to new_freq."""
    g = math.gcd(int(orig_freq), int(new_freq))
    orig, new = int(orig_freq) // g, int(new_freq) // g
    return new, orig, math.ceil(lowpass_filter_width * orig / (min(orig, new) * rolloff))


def frames(n, n_fft, hop):
    """T_b of an item of n samples at the target rate."""
    pad = (n_fft - hop) // 2
    return max(0, math.floor((n + 2 * pad - n_fft) / hop) + 1)


def item_table(n_raw, n_fft, hop, bank=None, geoms=()):
    """The int32 words of the table, or None where the header says the batch is refused."""
    n = len(n_raw)
    bank = [-1] * n if bank is None else list(bank)
    if n <= 0 or n_fft <= 0 or hop <= 0 or n_fft % 4 or hop % 4 or hop > n_fft or (n_fft - hop) % 2 or len(geoms) > 16:
        return None
    pad = (n_fft - hop) // 2
    items, raw_off, slot, cu = [], 0, 0, 0
    for nr, bk in zip(n_raw, bank):
        if nr < 0 or bk < -1 or bk >= len(geoms):
            return None
        nb = nr if bk < 0 else -(-geoms[bk][0] * nr // geoms[bk][1])
        if nb <= pad:
            return None
        T = frames(nb, n_fft, hop)
        items.append([raw_off, nr, nb, slot, T, cu, bk, 0])
        raw_off = -(-(raw_off + nr) // 4) * 4
        slot += -(-(nb + 2 * pad) // hop)
        cu += T
    packed = -(-(slot * hop + n_fft - hop) // 4) * 4
    banks, off = [], 0
    for up, down, width in geoms:
        banks.append([up, down, width, off])
        off += up * (2 * width + down)
    if packed + hop >= INT32 or raw_off >= INT32 or off >= INT32 or cu >= (1 << 24):
        return None
    head = [MAGIC, n, n_fft, hop, pad, slot, cu, max(i[4] for i in items), packed, raw_off, len(geoms), off] + [0] * 4
    return np.asarray(head + [w for i in items for w in i] + [w for b in banks for w in b], dtype=np.int64).astype(np.int32)


def pack(raws, n_fft, hop, rates=None, sr=8000):
    """The packed buffer: per item (resample where its rate differs from sr ->) clamp to [-1, 1] -> np.pad(mode="reflect") by
    (n_fft - hop) / 2 -> placed at its slot; everything else zero.  raws: float32 arrays; rates: their sample rates (None: all sr)."""
    import hubert_oracle
    pad = (n_fft - hop) // 2
    rates = [sr] * len(raws) if rates is None else rates
    sigs = []
    for x, r in zip(raws, rates):
        x = np.asarray(x, dtype=np.float32)
        if r != sr:
            x = np.asarray(hubert_oracle.sinc_resample(x, r, sr), dtype=np.float32)
        sigs.append(np.pad(np.clip(x, -1.0, 1.0), (pad, pad), mode="reflect"))
    slots = [-(-len(s) // hop) for s in sigs]
    total = sum(slots) * hop + n_fft - hop
    out = np.zeros(-(-total // 4) * 4, dtype=np.float32)
    at = 0
    for s, k in zip(sigs, slots):
        out[at:at + len(s)] = s
        at += k * hop
    return out
