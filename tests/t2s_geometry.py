"""Shared by tests/test_t2s_geometry.py (CPU) and tests/test_t2s_geometry_gpu.py: small depth-1 text2semantic models whose GEOMETRY
(target width, heads, vocab, feed-forward width, outputs) sits at the edges that t2s_validate admits and the four fixture geometries
(cosingle_small, comix_small, cosingle, comix) never reach, and the launch arithmetic of one token step restated from
csrc/t2s_decode.hip (t2s_decode_run, launch_gemv, launch_gemv_b, gemv_kernel, pair_rows, load_chunk, stage_chunk), so that the GPU
file's cases can say which kernel paths they launch and the CPU file can hold the table to it."""
import math
from collections import OrderedDict

import torch

T2S_MAX_DIM = 4096                       # t2s_decode.hip: floats of the staged input vector
SOURCE = dict(dim=64, source_depth=1, target_depth=1, num_text=50)
TEXT_TOKENS, STEPS, MAX_LENGTH, MAX_SOURCE = 7, 48, 64, 16
SLOT_FORMS = (1, 2, 3, 5, 9)             # BQ = 1, 2, 4, 8 and two slot groups

# name -> outputs, target width, heads, vocab, feed-forward width (None: the model's own int(8 d / 3))
CASES = OrderedDict([
    ("k4-v5", dict(outputs=1, dim_target=4, heads=1, vocab=5, ff=None)),                  # ff 10 (12)
    ("k260-h3-v501", dict(outputs=1, dim_target=260, heads=3, vocab=501, ff=None)),       # ff 693 (696)
    ("k1020-h2-v1023", dict(outputs=1, dim_target=1020, heads=2, vocab=1023, ff=None)),   # ff 2720 (2720)
    ("k1028-h1-v1024", dict(outputs=1, dim_target=1028, heads=1, vocab=1024, ff=None)),   # ff 2741 (2744)
    ("k1536-ff4096", dict(outputs=1, dim_target=1536, heads=1, vocab=65, ff=None)),       # ff 4096 (4096)
    ("k4096-v65", dict(outputs=1, dim_target=4096, heads=1, vocab=65, ff=1001)),          # ff 1001 (1004)
    ("k64-ff4095", dict(outputs=1, dim_target=64, heads=1, vocab=130, ff=4095)),          # ff 4095 (4096)
    ("two-k520-v333", dict(outputs=2, dim_target=520, heads=2, vocab=333, ff=None)),      # ff 1386 (1388)
    ("two-k8-v9", dict(outputs=2, dim_target=8, heads=1, vocab=9, ff=None)),              # ff 21 (24)
])
# the geometries of every other GPU test of the decode (the KW tables of tests/test_t2s_long_gpu.py and tests/golden/make_golden_t2s.py)
EXISTING = OrderedDict([
    ("cosingle_small", dict(outputs=1, dim_target=64, heads=1, vocab=502, ff=None)),
    ("comix_small", dict(outputs=2, dim_target=128, heads=1, vocab=502, ff=None)),
    ("cosingle", dict(outputs=1, dim_target=512, heads=8, vocab=502, ff=None)),
    ("comix", dict(outputs=2, dim_target=1024, heads=8, vocab=502, ff=None)),
])


def dims(outputs, dim_target, heads, vocab, ff=None):
    """the descriptor fields t2s.py derives from a state dict of that geometry"""
    ff = int(dim_target * 4 * 2 / 3) if ff is None else ff
    return dict(dim=dim_target, inner=64 * heads, heads=heads, streams=outputs, dim_emb=dim_target // outputs, vocab=vocab,
                ff_inner=ff, ff_inner_pad=(ff + 3) // 4 * 4)


def admitted(d):
    """t2s_validate's geometry conditions"""
    return (d["dim"] > 0 and d["dim"] % 4 == 0 and d["dim"] <= T2S_MAX_DIM and d["streams"] in (1, 2) and d["dim_emb"] * d["streams"] == d["dim"]
            and d["dim_emb"] % 4 == 0 and (d["streams"] == 1 or d["dim"] <= 1024) and 0 < d["vocab"] <= 1024
            and d["ff_inner"] > 0 and d["ff_inner_pad"] >= d["ff_inner"] and d["ff_inner_pad"] % 4 == 0 and d["ff_inner_pad"] <= T2S_MAX_DIM)


def state_dict(name, seed=0):
    """synthetic weights of case `name` as torch tensors"""
    import covomix_amd.synthetic as syn
    c = CASES[name]
    shapes = syn.t2s_param_shapes(two_output=c["outputs"] == 2, dim_target=c["dim_target"], heads=c["heads"], num_semantic=c["vocab"] - 1, **SOURCE)
    if c["ff"] is not None:                              # the one width t2s_param_shapes does not parametrise
        p, dt, di = "target_transformer.layers.0.2", c["dim_target"], c["ff"]
        shapes[p + ".1.weight"], shapes[p + ".1.bias"], shapes[p + ".4.weight"] = (2 * di, dt), (2 * di,), (dt, di)
    return {k: torch.from_numpy(v) for k, v in syn.t2s_state_dict(shapes, seed=seed).items()}


def text(n=TEXT_TOKENS, seed=7):
    """n text ids in 1 .. num_text - 1 (0 is the pad id, the last row of the text embedding the text eos)"""
    return torch.randint(1, SOURCE["num_text"], (1, n), generator=torch.Generator().manual_seed(seed))


def draws(steps, S, V, seed):
    return torch.rand(steps, S, V, generator=torch.Generator().manual_seed(seed))


def forced_tokens(name, L=STEPS, seed=11):
    """random forced tokens [S, L] of case `name`"""
    c = CASES[name]
    return torch.randint(0, c["vocab"], (c["outputs"], L), generator=torch.Generator().manual_seed(seed))


# ---------------------------------------------------------------- the GEMV launches of one token step
def _strips(K, c):
    """load_chunk / dot_chunk: the four 256-float strips of chunk c of a row of K floats: "whole", ("partial", lanes that load) or "absent" """
    out = []
    for i in range(4):
        kb = 1024 * c + 256 * i
        out.append("whole" if kb + 256 <= K else (("partial", (K - kb) // 4) if kb < K else "absent"))
    return tuple(out)


def gemv_launches(d, slots):
    """The launch_gemv calls of one token step of a depth-1 decoder (t2s_decode_run: six per layer and the logits) at `slots` decode
    slots.  Per launch:
    mode, N, K (row length the strips are classified by), Kin (staged floats per slot), gamma (normalised input), pairs, row_blocks, BQ,
    groups (slot groups = blocks per row block), chunks (per chunk the class of its four strips), no_second_row (a pair whose second row
    does not exist), zero_fill (GEGLU entries written as zeros), idle_waves (waves of the last block without a pair; under GEGLU the
    zero-filling waves are not idle), exit_blocks (row blocks of the padded grid that return at once; gy > 1 only)."""
    D, I, S, V, F, Fp = d["dim"], d["inner"], d["streams"], d["vocab"], d["ff_inner"], d["ff_inner_pad"]
    bq = 1 if slots <= 1 else 2 if slots <= 2 else 4 if slots <= 4 else 8
    groups = (slots + 7) // 8 if slots > 4 else 1
    rows = [("qkv_s", "QKV", 3 * I, D, D, True, 3 * I // 2), ("wo_s", "RES", D, I, I, False, (D + 1) // 2),
            ("wq_c", "PLAIN", I, D, D, True, I // 2), ("wo_c", "RES", D, I, I, False, (D + 1) // 2),
            ("w1", "GEGLU", 2 * F, D, D, True, Fp), ("w2", "RES", D, Fp, Fp, False, (D + 1) // 2),
            ("logits", "LOGITS", V, d["dim_emb"], d["dim_emb"] * S, True, S * ((V + 1) // 2))]
    out = []
    for name, mode, N, K, Kin, gamma, pairs in rows:
        nb = (pairs + 3) // 4
        out.append(dict(name=name, mode=mode, N=N, K=K, Kin=Kin, gamma=gamma, pairs=pairs, row_blocks=nb, BQ=bq, groups=groups,
                        chunks=tuple(_strips(K, c) for c in range((Kin + 1023) // 1024)),
                        no_second_row=mode in ("RES", "PLAIN", "LOGITS") and N % 2 == 1,
                        zero_fill=Fp - F if mode == "GEGLU" else 0,
                        idle_waves=4 * nb - pairs,
                        exit_blocks=(nb + 7) // 8 * 8 - nb if groups > 1 else 0,
                        streams=S if mode == "LOGITS" else 1))
    return out


def paths(launches):
    """the named path classes a list of launches reaches (PATHS lists all of them)"""
    p = set()
    for l in launches:
        m, ch = l["mode"], l["chunks"]
        flat = [s for c in ch for s in c]
        part = [s[1] for s in flat if isinstance(s, tuple)]
        if l["gamma"]:
            if any("whole" in c and any(isinstance(s, tuple) for s in c) for c in ch): p.add(f"norm-whole-then-partial-strip:{m}")
            if len(ch) > 1: p.add(f"norm-second-chunk:{m}")
            if len(ch) > 1 and ch[-1] == (("partial", 1), "absent", "absent", "absent"): p.add(f"norm-second-chunk-one-vector:{m}")
            if l["K"] == T2S_MAX_DIM: p.add(f"norm-K-max:{m}")
            if 1 in part: p.add("norm-one-lane-strip")
            if 63 in part: p.add("norm-strip-one-lane-short")
        if m == "LOGITS":
            if l["no_second_row"]: p.add("logits-odd-vocab")
            if l["streams"] == 1 and l["K"] > 1024: p.add("logits-multi-chunk")
            if l["streams"] == 2 and l["K"] % 64: p.add("logits-slice-offset-unaligned")       # (the fixtures' second slices start at 64 and 512)
            if l["N"] == 1024: p.add("sample-V-1024")
            if l["N"] == 1023: p.add("sample-V-1023")
            if l["N"] < 64: p.add("sample-V-below-a-wave")
        if m in ("RES", "PLAIN", "QKV"):
            if l["idle_waves"]: p.add(f"idle-waves:{m}")
            if l["exit_blocks"]: p.add(f"exit-blocks:{m}")
        if m == "GEGLU":
            if l["zero_fill"] in (0, 1): p.add(f"geglu-zero-fill-{l['zero_fill']}")
            if l["N"] // 2 + l["zero_fill"] == T2S_MAX_DIM: p.add("geglu-ff-pad-max")
    return p


NORM_MODES = ("QKV", "PLAIN", "GEGLU", "LOGITS")
# every class `paths` can name that a valid geometry can reach.  (PLAIN and QKV launch 32 and 96 pairs per head - 8 and 24 whole row
# blocks - so of the three residual-free modes only RES can have idle waves or exiting row blocks.)
PATHS = frozenset([f"{k}:{m}" for k in ("norm-whole-then-partial-strip", "norm-second-chunk", "norm-second-chunk-one-vector", "norm-K-max")
                   for m in NORM_MODES] +
                  ["norm-one-lane-strip", "norm-strip-one-lane-short", "logits-odd-vocab", "logits-multi-chunk", "logits-slice-offset-unaligned",
                   "sample-V-1024", "sample-V-1023", "sample-V-below-a-wave", "idle-waves:RES", "exit-blocks:RES",
                   "geglu-zero-fill-0", "geglu-zero-fill-1", "geglu-ff-pad-max"])


def case_paths(c):
    """the path classes of geometry c over every slot form"""
    return set().union(*(paths(gemv_launches(dims(**c), s)) for s in SLOT_FORMS))


def top_k(V):
    return math.ceil(0.1 * V)
