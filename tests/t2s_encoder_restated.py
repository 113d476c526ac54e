"""Shared by tests/test_t2s_encoder.py (CPU) and tests/test_t2s_encoder_gpu.py: the cases, packings, fp64 expectations, metrics and bounds
of the checks of TextToSemanticDecoder.encode_many and of the context records _contexts / _guided_contexts write (t2s.py), and plain
torch restatements of both with the defects the checks have to resolve (MUTANTS; used by the CPU file only).  No GPU needed.

Cases: the committed cosingle_small fixture (source width 64, 1 head, source depth 2) and two synthetic depth-1 models built the way
tests/t2s_geometry.py::state_dict builds its models (seed 0, num_text 50, a small target side): d260-h3 (K % 32 != 0: the GENERIC fp32
GEMM forms; feed-forward 693, padded to 696) and d512-h8.  max_source = 272 for all three.

Packings (token counts; a text's rows are one more, the text eos):
  EDGES           row counts 2, 31, 32, 33, 127, 128, 129, 257 (the 32-key tile and the 128-query block of csrc/attention_f32.hip), the
                  text of no tokens (its eos row alone) and 270 tokens;
  EDGES_REVERSED  the same texts in reverse order: same M, same kernel forms, every text at another offset;
  MANY            32-token texts, as many as it takes for ops.gemm_f32_form to name another form than under EDGES for at least one of the
                  encoder's four GEMMs (many_count); a case that cannot get there under MAX_ROWS is named in MANY_UNREACHABLE.

Expectation: oracle/t2s_oracle.py::encode on the state dict cast to float64, one text per call; context rows: that times the layer's
to_kv weight in fp64.  Metrics: per_text = rel-L2 of a text's rows, per_row = the largest row-wise rel-L2; nothing is pooled over texts
and no row is left out.  Bounds: FACTOR x the distance of the fp32 CPU oracle (the same code on the float32 state dict; for the context
rows the fp32 CPU product behind it) from the fp64 one, the largest over the packing's texts - derived from the reference alone.  The
factor 4 covers one difference: the kernels sum in another order than torch's CPU GEMM (MFMA tiles, online softmax); both are fp32-class."""
import os
from collections import OrderedDict

import numpy as np
import torch

import t2s_oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAX_SOURCE = 272
MAX_ROWS = 4096                      # packed rows of the largest packing a test may run
FACTOR = 4.0                         # bound = FACTOR x the fp32 CPU oracle's own distance from fp64
REFERENCE_ALONE_MAX = 1e-5           # ... which stays under this (tests/test_t2s_encoder.py): a bound can never silently grow
EDGES = (1, 30, 31, 32, 126, 127, 128, 256, 0, 270)
PACKINGS = ("EDGES", "EDGES_REVERSED", "MANY")
MANY_TOKENS = 32

# name -> source width, heads (None: the committed fixture)
CASES = OrderedDict([("cosingle_small", None), ("d260-h3", dict(dim=260, heads=3)), ("d512-h8", dict(dim=512, heads=8))])
SYNTHETIC = dict(two_output=False, dim_target=64, source_depth=1, target_depth=1, num_text=50, num_semantic=64)
# cases whose four encoder GEMMs keep their EDGES forms up to MAX_ROWS packed rows: no MANY packing (test_t2s_encoder.py holds the list to
# gemm_f32_form).  Width 64: the widest GEMM has 3 column tiles, 256 tiles of 128 x 128 would take 10881 rows.
MANY_UNREACHABLE = {"cosingle_small": "no encoder GEMM of width 64 changes its form under 4096 packed rows (256 tiles of 128 x 128 need 10881)"}

_SD, _TEXTS, _EXPECT, _BOUNDS = {}, {}, {}, {}


def state_dict(name):
    """float32 weights of a case (built once; do not modify)"""
    if name not in _SD:
        if CASES[name] is None:
            g = np.load(os.path.join(GOLDEN, f"t2s_{name}.npz"))
            _SD[name] = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w::")}
        else:
            import covomix_amd.synthetic as syn
            shapes = syn.t2s_param_shapes(**SYNTHETIC, **CASES[name])
            _SD[name] = {k: torch.from_numpy(v) for k, v in syn.t2s_state_dict(shapes, seed=0).items()}
    return _SD[name]


def cast(sd, dtype):
    return {k: v.to(dtype) if v.is_floating_point() else v for k, v in sd.items()}


def encoder_gemms(name):
    """(N, K) of the four GEMMs of an encoder layer as encode_many launches them: to_qkv, to_out, the feed-forward's two"""
    d = orc.t2s_dims(state_dict(name))
    D, I = d["dim"], d["heads"] * 64
    F_ = state_dict(name)["source_transformer.layers.0.2.4.weight"].shape[1]
    return ((3 * I, D), (D, I), (2 * F_, D), (D, (F_ + 3) // 4 * 4))


def forms(name, M):
    """ops.gemm_f32_form of the four encoder GEMMs at M packed rows"""
    from covomix_amd import ops
    return tuple(ops.gemm_f32_form(M, N, K) for N, K in encoder_gemms(name))


def rows_of(tokens):
    return sum(t + 1 for t in tokens)


def many_count(name):
    """texts of MANY: the fewest MANY_TOKENS-token texts whose packed row count moves one of the four GEMMs to another form than under EDGES;
    None when MAX_ROWS rows do not get there"""
    edges = forms(name, rows_of(EDGES))
    for n in range(1, MAX_ROWS // (MANY_TOKENS + 1) + 1):
        if forms(name, n * (MANY_TOKENS + 1)) != edges:
            return n
    return None


def token_counts(name, packing):
    if packing == "EDGES":
        return EDGES
    if packing == "EDGES_REVERSED":
        return EDGES[::-1]
    assert packing == "MANY" and name not in MANY_UNREACHABLE, (name, packing)
    return (MANY_TOKENS,) * many_count(name)


def texts(name, packing):
    """the texts of a packing: int64 [1, t] ids in [1, num_text), seeded per text - never 0 (the pad id), never the text eos"""
    if packing == "EDGES_REVERSED":
        return texts(name, "EDGES")[::-1]
    if (name, packing) not in _TEXTS:
        num_text = state_dict(name)["token_emb.text.weight"].shape[0] - 1
        base = 0 if packing == "EDGES" else 1000
        _TEXTS[(name, packing)] = [torch.randint(1, num_text, (1, t), generator=torch.Generator().manual_seed(base + i))
                                   for i, t in enumerate(token_counts(name, packing))]
    return list(_TEXTS[(name, packing)])


# ---------------------------------------------------------------- metrics
def per_text(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def row_errors(a, b):
    a, b = a.double().cpu().reshape(b.shape), b.double().cpu()
    return (a - b).norm(dim=-1) / b.norm(dim=-1).clamp_min(1e-30)


def per_row(a, b):
    return float(row_errors(a, b).max())


def pooled(parts, refs):
    """the measure the older encoder check uses: rel-L2 over all rows of all texts"""
    return per_text(torch.cat([p.double().cpu() for p in parts]), torch.cat([r.double().cpu() for r in refs]))


# ---------------------------------------------------------------- expectations and bounds
def kv_weights(name):
    """the to_kv weights of the decoder layers' cross-attention, [2 inner, source width] each"""
    sd, d = state_dict(name), orc.t2s_dims(state_dict(name))
    return [sd[f"target_transformer.layers.{i}.1.to_kv.0.weight"] for i in range(d["target_depth"])]


def expectation(name, packing):
    """(enc64, enc32): per text the oracle's encoder rows [t + 1, dim] in fp64 and in fp32.  Computed once; do not modify."""
    if packing == "EDGES_REVERSED":
        e64, e32 = expectation(name, "EDGES")
        return e64[::-1], e32[::-1]
    if (name, packing) not in _EXPECT:
        sd32, sd64 = state_dict(name), cast(state_dict(name), torch.float64)
        with torch.no_grad():
            e64 = [orc.encode(sd64, t)[0][0] for t in texts(name, packing)]
            e32 = [orc.encode(sd32, t)[0][0] for t in texts(name, packing)]
        _EXPECT[(name, packing)] = (e64, e32)
    e64, e32 = _EXPECT[(name, packing)]
    return list(e64), list(e32)


def bounds(name, packing):
    """dict(ref_text, ref_row, bound_text, bound_row, ctx_ref_text, ctx_ref_row, ctx_bound_text, ctx_bound_row): the fp32 CPU oracle's
    largest per-text and per-row distance from the fp64 one over the packing's texts (encoder rows; context rows = the fp32 product of
    the fp32 rows against the fp64 product of the fp64 rows, over the decoder layers), and FACTOR times each."""
    key = (name, "EDGES" if packing == "EDGES_REVERSED" else packing)
    if key not in _BOUNDS:
        e64, e32 = expectation(*key)
        b = dict(ref_text=max(per_text(a, r) for a, r in zip(e32, e64)), ref_row=max(per_row(a, r) for a, r in zip(e32, e64)),
                 ctx_ref_text=0.0, ctx_ref_row=0.0)
        for W in kv_weights(name):
            for a, r in zip(e32, e64):
                kv32, kv64 = a @ W.T, r @ W.double().T
                b["ctx_ref_text"], b["ctx_ref_row"] = max(b["ctx_ref_text"], per_text(kv32, kv64)), max(b["ctx_ref_row"], per_row(kv32, kv64))
        for k in ("text", "row"):
            b["bound_" + k], b["ctx_bound_" + k] = FACTOR * b["ref_" + k], FACTOR * b["ctx_ref_" + k]
        _BOUNDS[key] = b
    return dict(_BOUNDS[key])


def split_rows(enc, lengths):
    """the packed rows [M, width] of encode_many cut into texts"""
    assert enc.shape[0] == sum(lengths), (enc.shape, lengths)
    return list(enc.split(list(lengths), dim=0))


# ---------------------------------------------------------------- restatements (CPU test only)
MUTANTS = ("leak", "eos", "late", "packed", "scatter")     # (a) .. (e) of the CPU file's docstring


def late_row(rows):
    """the row of a text of `rows` rows whose rotary angle mutant (c) takes one position late (texts of one row are not touched: one
    query and its own key, rotated alike)"""
    return rows // 2 if rows >= 2 else None


def restated_encode_many(sd, sources, dtype=torch.float64, mutant=None):
    """encode_many (t2s.py) in plain torch at `dtype`: the texts packed, the eos appended, attention and rotary positions per text.
    -> list of [t + 1, dim] rows per text.  mutant: None, or
      "leak"    the last key of the preceding text is visible to a text's queries (every text but the first);
      "eos"     the eos row is embedded with the neighbouring id (every text);
      "late"    the rotary angle of one row per text (late_row) is taken one position late (texts of two rows and more);
      "packed"  the rotary tables are taken at the packed row index (every text but the first)."""
    assert mutant in (None, "leak", "eos", "late", "packed")
    sd = cast(sd, dtype)
    d = orc.t2s_dims(sd)
    H, eos = d["heads"], d["text_eos_id"]
    ids = [torch.cat((s.reshape(-1).long(), torch.tensor([eos - 1 if mutant == "eos" else eos]))) for s in sources]
    lengths = [i.numel() for i in ids]
    cu = [0]
    for t in lengths:
        cu.append(cu[-1] + t)
    x = sd["token_emb.text.weight"][torch.cat(ids)]
    pos = torch.cat([torch.arange(t, dtype=torch.float32) for t in lengths])
    if mutant == "late":
        for i, t in enumerate(lengths):
            if late_row(t) is not None:
                pos[cu[i] + late_row(t)] += 1
    if mutant == "packed":
        pos = torch.arange(cu[-1], dtype=torch.float32)
    freqs = sd["source_transformer.layers.0.0.rotary_emb.freqs"]
    M = cu[-1]
    for l in range(d["source_depth"]):
        p = f"source_transformer.layers.{l}"
        xn = orc.rmsnorm(x, sd[p + ".0.norm.gamma"])
        q = (xn @ sd[p + ".0.to_q.0.weight"].T).reshape(M, H, 64).transpose(0, 1)
        k, v = [t.reshape(M, H, 64).transpose(0, 1) for t in (xn @ sd[p + ".0.to_kv.0.weight"].T).chunk(2, dim=-1)]
        q, k = orc.rotate_interleaved(q, pos, freqs), orc.rotate_interleaved(k, pos, freqs)
        out = torch.empty(M, H * 64, dtype=dtype)
        for i in range(len(lengths)):
            keys = list(range(cu[i], cu[i + 1]))
            if mutant == "leak" and i > 0:
                keys = [cu[i] - 1] + keys
            prob = ((q[:, cu[i]:cu[i + 1]] @ k[:, keys].transpose(-1, -2)) * 64 ** -0.5).softmax(dim=-1)
            out[cu[i]:cu[i + 1]] = (prob @ v[:, keys]).transpose(0, 1).reshape(lengths[i], H * 64)
        x = out @ sd[p + ".0.to_out.weight"].T + x
        x = orc.feedforward(sd, p + ".2", x) + x
    return split_rows(orc.rmsnorm(x, sd["source_transformer.final_norm.gamma"]), lengths)


def restated_contexts(enc, W, null, records, n_records, sentinel, mutant=None):
    """_contexts' scatter of one decoder layer in plain torch: enc = the encoder rows per text, W the layer's to_kv weight, null its null
    row [2 inner] -> records [n_records, MAX_SOURCE + 2, 2 inner] pre-filled with `sentinel`, record records[i] holding
    [null | enc[i] @ W.T].  mutant "scatter": everything one row late - the null row at index 1, the text rows behind it."""
    assert mutant in (None, "scatter")
    off = 1 if mutant == "scatter" else 0
    out = torch.full((n_records, MAX_SOURCE + 2, W.shape[0]), float(sentinel), dtype=enc[0].dtype)
    for e, r in zip(enc, records):
        out[r, off] = null.to(e.dtype)
        out[r, off + 1:off + 1 + e.shape[0]] = e @ W.to(e.dtype).T
    return out


def check_records(kv_c, W, null, records, enc64, sentinel):
    """One layer's context records kv_c [n_records, MAX_SOURCE + 2, 2 inner] (CPU) after a scatter of the texts whose fp64 encoder rows are
    enc64 into `records`, everything else pre-filled with `sentinel` -> dict(text, row: the worst per-text / per-row distance of rows
    1 .. t from enc64 @ W^T in fp64; rows: per text the row-wise distances; null_exact: row 0 of every named record equals `null` bit for
    bit; untouched: every element outside rows [0, t] of the named records still holds the sentinel; last: per text the last index that
    does not hold the sentinel).  No bound is applied here: the callers assert."""
    assert kv_c.shape[1] == MAX_SOURCE + 2 and len(set(records)) == len(records)
    written = torch.zeros(kv_c.shape[:2], dtype=torch.bool)
    res = dict(text=0.0, row=0.0, rows=[], null_exact=True, last=[])
    for e, r in zip(enc64, records):
        t = e.shape[0]
        written[r, :t + 1] = True
        want = e @ W.double().T
        res["rows"].append(row_errors(kv_c[r, 1:t + 1], want))
        res["text"], res["row"] = max(res["text"], per_text(kv_c[r, 1:t + 1], want)), max(res["row"], float(res["rows"][-1].max()))
        res["null_exact"] &= torch.equal(kv_c[r, 0], null.to(kv_c.dtype))
        touched = (kv_c[r] != sentinel).any(dim=-1).nonzero()
        res["last"].append(int(touched.max()) if touched.numel() else -1)
    res["untouched"] = bool((kv_c[~written] == sentinel).all())
    return res
