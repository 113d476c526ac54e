"""CPU: the C-ABI library loads and exports every declared symbol; host-side logic (time grid,
checkpoint loader incl. EMA + stub unpickling, DP sharding + gloo broadcast, loud failure without GPU)."""
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import ROOT


def test_library_exports_every_header_symbol():
    from covomix_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "covomix_hip.h")).read()
    declared = set(re.findall(r"\b(cvx_[a-z0-9_]+)\s*\(", hdr))
    assert declared, "no symbols parsed from the header"
    assert declared == set(_lib.SIGNATURES), (declared ^ set(_lib.SIGNATURES))
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.cvx_version() >= 100
    assert lib.cvx_hifigan_packed_weight_floats(250, 250, 11) == 4 * 16 * 11 * 64 * 16


def test_pack_weight_layout_cpu():
    """cvx_hifigan_pack_weight_f32 is host code: check the documented layout, incl. the transposed flip."""
    from covomix_amd import ops
    w = torch.arange(3 * 5 * 4, dtype=torch.float32).reshape(3, 5, 4)          # [Cout=3, Cin=5, k=4]
    wp = ops.hifigan_pack_weight(w, False).reshape(1, 1, 4, 32, 16)
    for co in range(3):
        for ci in range(5):
            for k in range(4):
                assert wp[0, 0, k, co, ci] == w[co, ci, k]
    assert wp[0, 0, :, 3:, :].abs().sum() == 0 and wp[0, 0, :, :, 5:].abs().sum() == 0
    wt = torch.arange(5 * 3 * 4, dtype=torch.float32).reshape(5, 3, 4)          # ConvT [Cin=5, Cout=3, k=4]
    wpt = ops.hifigan_pack_weight(wt, True).reshape(1, 1, 4, 32, 16)
    for co in range(3):
        for ci in range(5):
            for k in range(4):
                assert wpt[0, 0, k, co, ci] == wt[ci, co, 3 - k]


def test_ops_fail_loudly_without_gpu():
    from covomix_amd import _lib, ops
    from covomix_amd.conditional_model import CoVoMixModel
    from covomix_amd.vocoder import AttrDict, Generator
    import covomix_amd.synthetic as syn
    a = torch.zeros(4, 4)
    with pytest.raises(_lib.CovomixHipError):
        ops.gemm(a, a, a.clone())
    shapes = syn.acoustic_param_shapes(dim=128, dim_cond=160, dim_emb=64, depth=2, heads=2, streams=2)
    sd = {k: torch.from_numpy(v) for k, v in syn.synth_state_dict(shapes).items()}
    m = CoVoMixModel.from_state_dict(sd).eval()
    with pytest.raises(_lib.CovomixHipError):
        m.synthesis_sample(torch.zeros(1, 8, 2, dtype=torch.long), torch.zeros(1, 8, 160), None, 0.7)
    h = dict(syn.HIFIGAN_COVOMIX_CONFIG); h["upsample_initial_channel"] = 32
    g = Generator(AttrDict(h))
    g.load_state_dict({k: torch.from_numpy(v) for k, v in syn.synth_state_dict(syn.hifigan_param_shapes(h)).items()})
    g.remove_weight_norm()
    with pytest.raises(_lib.CovomixHipError):
        g(torch.zeros(80, 10))


def test_missing_library_message(tmp_path, monkeypatch):
    from covomix_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_lib.CovomixHipError, match="no CPU"):
        _lib.load()


def test_evaluation_times_match_oracle_grid():
    import covomix_oracle as orc
    from covomix_amd.acoustic import evaluation_times
    t, dts = evaluation_times(32, "midpoint")
    g = orc.fixed_grid(0.0625)
    assert len(dts) == 16 and all(d == 0.0625 for d in dts)
    exp = []
    for a, b in zip(g[:-1], g[1:]):
        exp += [float(a), float(a + 0.5 * (b - a))]
    assert t.tolist() == exp
    t, dts = evaluation_times(10, "euler")
    assert t.numel() == 10 and abs(sum(dts) - 1.0) < 1e-6
    with pytest.raises(ValueError):
        evaluation_times(7, "midpoint")


def _fake_ckpt(path, with_ema=True):
    import covomix_amd.synthetic as syn
    shapes = syn.acoustic_param_shapes(dim=128, dim_cond=80, dim_emb=64, depth=2, heads=2, streams=1)
    sd = {k: torch.from_numpy(v) for k, v in syn.synth_state_dict(shapes, seed=0).items()}
    full = {"cfm_wrapper.CoVoMix." + k: v for k, v in sd.items()}
    full["cfm_wrapper.CoVoMix.transformer.rotary_emb.inv_freq"] = torch.from_numpy(syn.rotary_inv_freq(64))
    ema = {k: torch.from_numpy(v) for k, v in syn.synth_state_dict(shapes, seed=7).items()}

    # a hyper_parameters entry that references a class from a module that is NOT importable here,
    # like Lightning's save_hyperparameters does with data_module_cls (conditional_model.py:150)
    import types
    fake = types.ModuleType("covomix_fake_data_module")
    class SpecsDataModule:  # noqa: E306
        pass
    SpecsDataModule.__module__ = "covomix_fake_data_module"
    SpecsDataModule.__qualname__ = "SpecsDataModule"
    fake.SpecsDataModule = SpecsDataModule
    sys.modules["covomix_fake_data_module"] = fake
    ckpt = {"state_dict": full,
            "hyper_parameters": {"CoVoMix_dim": 80, "CoVoMix_depth": 2, "text2semantic": False,
                                 "twocondition_oneoutput": False, "data_module_cls": SpecsDataModule}}
    if with_ema:
        ckpt["ema"] = {"decay": 0.999, "num_updates": 10, "shadow_params": list(ema.values()), "collected_params": None}
    torch.save(ckpt, path)
    del sys.modules["covomix_fake_data_module"]
    return sd, ema


def test_checkpoint_loader_ema_and_stub_unpickle(tmp_path):
    from covomix_amd.conditional_model import CoVoMixModel
    p = str(tmp_path / "last.ckpt")
    sd, ema = _fake_ckpt(p, with_ema=True)
    m = CoVoMixModel.load_from_checkpoint(p, base_dir='', batch_size=16, num_workers=0)
    assert m.hparams["CoVoMix_depth"] == 2 and "data_module_cls" not in m.hparams
    m.eval()
    act = m.active_state_dict()
    for k in ema:
        assert torch.equal(act[k], ema[k])                      # EMA weights are what run
    assert "transformer.rotary_emb.inv_freq" in act
    m.eval(no_ema=True)
    assert torch.equal(m.active_state_dict()["null_cond"], sd["null_cond"])
    m.train(True)
    assert torch.equal(m.active_state_dict()["null_cond"], sd["null_cond"])
    p2 = str(tmp_path / "noema.ckpt")
    sd2, _ = _fake_ckpt(p2, with_ema=False)
    with pytest.warns(UserWarning, match="EMA"):
        m2 = CoVoMixModel.load_from_checkpoint(p2)
    assert torch.equal(m2.eval().active_state_dict()["null_cond"], sd2["null_cond"])
    with pytest.raises(AssertionError):
        CoVoMixModel.load_from_checkpoint(str(tmp_path / "missing.ckpt"))


def test_vocoder_fold_matches_oracle_and_api():
    import covomix_oracle as orc
    import covomix_amd.synthetic as syn
    from covomix_amd.vocoder import AttrDict, Generator, fold_weight_norm, get_padding
    h = dict(syn.HIFIGAN_COVOMIX_CONFIG); h["upsample_initial_channel"] = 32
    sd = {k: torch.from_numpy(v) for k, v in syn.synth_state_dict(syn.hifigan_param_shapes(h)).items()}
    a, b = fold_weight_norm(sd), orc.fold_weight_norm(sd)
    assert a.keys() == b.keys() and all(torch.allclose(a[k], b[k], rtol=1e-6, atol=0) for k in a)
    assert get_padding(11, 5) == 25 and get_padding(3, 1) == 1
    g = Generator(AttrDict(h))
    g.load_state_dict(sd)
    assert g.eval() is g and len(g.state_dict()) == 234
    g.remove_weight_norm()
    assert not any(k.endswith("weight_g") for k in g.state_dict())
    assert AttrDict(h).upsample_rates == [5, 4, 4, 2]


def test_sharding_plan():
    from covomix_amd.dp import batch_equal_length, shard_utterances
    lengths = [1000] * 64
    plan = shard_utterances(lengths, 8)
    assert sorted(sum(plan, [])) == list(range(64)) and all(len(p) == 8 for p in plan)
    ragged = [500, 120, 977, 33, 500, 500, 64, 800, 120]
    plan = shard_utterances(ragged, 3)
    assert sorted(sum(plan, [])) == list(range(9))
    loads = [sum(ragged[i] for i in p) for p in plan]
    assert max(loads) - min(loads) <= max(ragged)
    assert shard_utterances([], 4) == [[], [], [], []]
    batches = batch_equal_length([0, 4, 5, 1, 8], ragged, max_batch=2)
    assert batches == [[0, 4], [5], [1, 8]]
    # ragged batches: in the given order, bounded by utterance count and by frames; an over-long utterance runs alone
    from covomix_amd.dp import batch_by_frames
    assert batch_by_frames([2, 7, 0, 4, 5, 1, 8, 6, 3], ragged, max_batch=3, max_frames=1500) == [[2], [7, 0], [4, 5, 1], [8, 6, 3]]
    assert batch_by_frames([2, 7], ragged, max_batch=8, max_frames=100) == [[2], [7]]
    assert batch_by_frames([], ragged, 8, 1000) == []
    every = batch_by_frames(list(range(9)), ragged, max_batch=8, max_frames=10 ** 9)
    assert every == [list(range(8)), [8]]
    # first-fit decreasing into bins of max_frames (what the CLI uses): bins are filled, every index exactly once, deterministic
    from covomix_amd.dp import pack_by_frames
    bins = pack_by_frames(list(range(9)), ragged, max_frames=1000, max_batch=32)
    assert sorted(sum(bins, [])) == list(range(9)) and all(sum(ragged[i] for i in b) <= 1000 for b in bins)
    assert bins == [[2], [7, 1, 6], [0, 4], [5, 8, 3]] and bins == pack_by_frames(list(range(9))[::-1], ragged, 1000, 32)
    assert pack_by_frames([2, 7], ragged, max_frames=100, max_batch=32) == [[2], [7]]         # longer than a bin: alone
    assert pack_by_frames(list(range(9)), ragged, max_frames=10 ** 9, max_batch=4) == [[2, 7, 0, 4], [5, 1, 8, 6], [3]]
    # vocoder sub-groups of a bin: padding to the group's longest item stays below 25 % of its real frames (round-3 advisor
    # finding: an 8000-frame item with 31 short fillers was vocoded as 32 x 8000 frames)
    from covomix_amd.dp import group_by_padding
    tg = [8000] + [150 + 3 * i for i in range(31)]
    groups = group_by_padding(tg)
    assert sorted(i for g_ in groups for i in g_) == list(range(32)) and groups[0] == [0]
    for g_ in groups:
        assert len(g_) * max(tg[i] for i in g_) <= 1.25 * sum(tg[i] for i in g_)
    assert sum(len(g_) * max(tg[i] for i in g_) for g_ in groups) < 1.25 * sum(tg)
    assert group_by_padding([600, 600, 600]) == [[0, 1, 2]] and group_by_padding([]) == []
    lens16 = [400, 1200, 451, 1149, 503, 1097, 555, 1044, 607, 993, 659, 941, 711, 889, 763, 837]
    b16 = pack_by_frames(list(range(16)), lens16, 8192, 32)
    assert len(b16) == 2 and sum(lens16[i] for i in b16[0]) >= 8000


def test_two_rank_gloo_broadcast_and_shard(tmp_path):
    """world_size-2 CPU run of the DP plumbing: weight broadcast (rank 1 starts from garbage),
    disjoint utterance shards, metric reduction."""
    script = tmp_path / "w.py"
    script.write_text(f"""
import os, sys, torch
sys.path.insert(0, {ROOT!r})
from covomix_amd import dp
import covomix_amd.synthetic as syn
rank, world, local = dp.init_from_env("gloo")
shapes = syn.acoustic_param_shapes(dim=128, dim_cond=80, dim_emb=64, depth=2, heads=2, streams=1)
good = {{k: torch.from_numpy(v) for k, v in syn.synth_state_dict(shapes, seed=0).items()}}
mine = good if rank == 0 else {{k: torch.full_like(v, float('nan')) for k, v in good.items()}}
got = dp.broadcast_state_dict(mine, torch.device('cpu'), src=0, bucket_bytes=1 << 18)
assert all(torch.equal(got[k], good[k]) for k in good), rank
plan = dp.shard_utterances([100, 200, 300, 400, 500], world)
frames, secs = dp.reduce_metric(float(sum([100, 200, 300, 400, 500][i] for i in plan[rank])), 1.0 + rank, torch.device('cpu'))
assert frames == 1500.0 and secs == 2.0
torch.distributed.barrier()
torch.distributed.destroy_process_group()
print('RANK_OK', rank, flush=True)
""")
    from covomix_amd import dp
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(dp.free_port()))
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = [p.communicate(timeout=240)[0] for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and f"RANK_OK {r}" in o, o


def test_text2semantic_checkpoint_layout_and_ema_order(tmp_path):
    """A text2semantic .ckpt as Lightning writes it for TextToSemanticWrapper: prefix cfm_wrapper.model., tied / shared
    tensors under several names, EMA shadow params in parameters() order (aliases excluded)."""
    import covomix_amd.synthetic as syn
    from covomix_amd.conditional_model import CoVoMixModel, t2s_parameter_order
    shapes = syn.t2s_param_shapes(two_output=True, dim=64, dim_target=128, source_depth=2, target_depth=2, heads=1, num_text=50)
    sd = {k: torch.from_numpy(v) for k, v in syn.t2s_state_dict(shapes, seed=0).items()}
    ema = {k: torch.from_numpy(v) for k, v in syn.t2s_state_dict(shapes, seed=3).items()}
    full = {}
    for k, v in sd.items():                                     # state_dict order of the reference module
        full["cfm_wrapper.model." + k] = v
        if k == "semantic_token_emb.weight":
            full["cfm_wrapper.model.token_emb.speech.weight"] = v
        if k == "start_token.text":
            full["cfm_wrapper.model.to_logits.speech.weight"] = sd["semantic_token_emb.weight"]
            full["cfm_wrapper.model.to_logits.text.weight"] = sd["token_emb.text.weight"]
        if k.endswith(".0.norm.gamma") and ".layers.0.0." not in k:
            pre = k[: -len("norm.gamma")]
            full["cfm_wrapper.model." + pre + "rotary_emb.freqs"] = sd[k.split(".layers.")[0] + ".layers.0.0.rotary_emb.freqs"]
    names = t2s_parameter_order([k[len("cfm_wrapper.model."):] for k in full])
    assert names == list(shapes.keys())                         # == reference named_parameters() order (make_golden_t2s.py)
    p = str(tmp_path / "t2s.ckpt")
    torch.save({"state_dict": full, "hyper_parameters": {"text2semantic": True, "text2semantic_two_output": True},
                "ema": {"decay": 0.999, "num_updates": 1, "shadow_params": [ema[k] for k in shapes], "collected_params": None}}, p)
    m = CoVoMixModel.load_from_checkpoint(p).eval()
    assert m.is_text2semantic
    assert torch.equal(m.active_state_dict()["start_token.speech"], ema["start_token.speech"])
    assert torch.equal(m.eval(no_ema=True).active_state_dict()["start_token.speech"], sd["start_token.speech"])
    with pytest.raises(TypeError):
        m.synthesis_sample(None, None, None, 0.7)
    with pytest.raises(AssertionError):
        m.synthesis_sample_text2semantic(torch.tensor([[1, 2]]), cond_scale=3.0)
    from covomix_amd._lib import CovomixHipError
    with pytest.raises(CovomixHipError):                        # no CPU fallback
        m.synthesis_sample_text2semantic(torch.tensor([[1, 2]]))


def test_tokenizer_cli_shards_files_by_rank(monkeypatch, tmp_path):
    """fairseq-hubert/get_fisher_semantic_tokens.py drop-in: files are dealt round-robin over RANK / WORLD_SIZE (host logic
    only - the encoder is stubbed, no GPU)."""
    import numpy as np
    import covomix_amd.hubert as hb
    for n in ("a", "b", "c", "d", "e"):
        open(tmp_path / f"{n}.wav", "wb").close()

    class Fake:
        def __init__(self, **kw):
            pass

        def wav2code(self, path, channel_id=1):
            return "1 2 3"
    monkeypatch.setattr(hb, "HubertTokenizer", Fake)
    monkeypatch.setattr(hb.torch.cuda, "set_device", lambda d: None)
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "1")
    monkeypatch.setenv("LOCAL_RANK", "1")
    out = tmp_path / "codes"
    assert hb.tokenize_directory(str(tmp_path), str(out), "x.pt", "km.bin") == 2
    import os
    assert sorted(os.listdir(out)) == ["b.hubert_code.npy", "d.hubert_code.npy"]
    assert np.load(out / "b.hubert_code.npy").tolist() == ["1", "2", "3"]


def test_generation_plan_is_rank_invariant_and_turn_aware(tmp_path):
    """The sharding plan of the generation driver is built from file names and sizes only (per-rank sampled
    lengths made ranks disagree): every rank computes the same partition, every utterance appears exactly once, turns of
    a dialogue stay on one rank, and the per-utterance RNG seeds do not depend on the rank."""
    import numpy as np
    from covomix_amd import generation as g
    tdir = str(tmp_path)
    rs = np.random.RandomState(0)
    for i in range(7):
        np.save(os.path.join(tdir, f"utt{i}.semantic.npy"), rs.randint(0, 500, size=20 + 13 * i))
    for k in range(3):
        np.save(os.path.join(tdir, f"dlg.turn{k}.semantic.npy"), rs.randint(0, 500, size=30 + k))
    with open(os.path.join(tdir, "spoken.txt"), "w") as f:
        f.write("hello there [spkchange] general kenobi [spkchange] bye")
    names, sources, plan = g.utterance_plan(tdir, True, "covosingle", True, 3)
    assert names == sorted(["dlg", "spoken"] + [f"utt{i}" for i in range(7)])
    assert len(sources["dlg"]) == 3 and [s[0] for s in sources["dlg"]] == ["sem"] * 3
    assert [s[0] for s in sources["spoken"]] == ["txt"] * 3 and sources["spoken"][1][1].strip() == "general kenobi"
    assert sorted(n for r in plan for n in r) == names and all(len(r) >= 2 for r in plan)
    assert g.utterance_plan(tdir, True, "covosingle", True, 3)[2] == plan                  # deterministic
    # monologue / covomix: the whole text is one turn; without text2semantic text files are not utterances
    mono = g.utterance_plan(tdir, False, "covosingle", True, 1)
    assert len(mono[1]["spoken"]) == 1 and "dlg.turn1" in mono[0] and "dlg" not in mono[0]
    assert "spoken" not in g.utterance_plan(tdir, True, "covosingle", False, 1)[0]
    assert g._stable_seed(30, "utt1", 0, 1) == g._stable_seed(30, "utt1", 0, 1) != g._stable_seed(30, "utt1", 1, 1)
    assert g._stable_seed(30, "utt1", 0, 1) != g._stable_seed(31, "utt1", 0, 1)
    import pytest
    with pytest.raises(FileNotFoundError):
        g.utterance_plan(os.path.join(tdir, "nothing_here"), False, "covosingle", False, 1)


def test_workspace_queries():
    """Section 8(b): caller-owned workspaces come with a size query (no GPU needed to ask)."""
    from covomix_amd import _lib
    lib = _lib.load()
    assert lib.cvx_gemm_f16x3_workspace_floats(1000, 1024, 4096, 0) == 4 * 1000 * 1024          # one utterance, long K: 4 slices
    assert lib.cvx_gemm_f16x3_workspace_floats(1000, 1024, 2048, 1024) == 4 * 1000 * 1024       # skip combiner: slices end at A | A2
    assert lib.cvx_gemm_f16x3_workspace_floats(16000, 1024, 4096, 0) == 0                       # large grids never split K
    assert lib.cvx_gemm_f16x3_workspace_floats(1000, 80, 1024, 0) == 8 * 1000 * 80              # to_pred on the medium-problem kernel: 8 slices
    assert lib.cvx_gemm_f16x3_workspace_floats(1000, 1024, 1024, 0) == 4 * 1000 * 1024          # to_out: 64 tiles x 4 slices fill the chip
    assert lib.cvx_rope_attention_workspace_floats(2, 130, 4) == 2 * 130 * 3 * 4 * 64
    assert lib.cvx_rope_attention_workspace_floats(0, 130, 4) == 0


def test_launch_ranks_self_spawns_two_gloo_ranks(tmp_path):
    """dp.launch_ranks (what `bench.py --gpus N` and the generation scripts use from a plain shell): N ranks under
    torch.distributed.run on a free port; init_from_env refuses WORLD_SIZE > 1 without a launcher-provided MASTER_PORT."""
    from covomix_amd import dp
    script = tmp_path / "ranks.py"
    script.write_text(f"""
import sys, os, torch
sys.path.insert(0, {ROOT!r})
from covomix_amd import dp
rank, world, local = dp.init_from_env("gloo")
assert world == 2 and os.environ["MASTER_ADDR"] == "127.0.0.1"
allv = dp.gather_floats([float(rank), 10.0 + rank], torch.device("cpu"))
assert allv == [[0.0, 10.0], [1.0, 11.0]], allv
open(os.path.join({str(tmp_path)!r}, f"rank{{rank}}.ok"), "w").write(sys.argv[1])
torch.distributed.destroy_process_group()
""")
    assert dp.launch_ranks(str(script), ["hello"], 2) == 0
    assert (tmp_path / "rank0.ok").read_text() == "hello" and (tmp_path / "rank1.ok").read_text() == "hello"
    env = {k: v for k, v in os.environ.items() if k not in ("MASTER_PORT", "MASTER_ADDR")}
    r = subprocess.run([sys.executable, "-c", f"import sys; sys.path.insert(0, {ROOT!r}); from covomix_amd import dp; dp.init_from_env('gloo')"],
                       env=dict(env, WORLD_SIZE="2", RANK="0"), capture_output=True, text=True)
    assert r.returncode != 0 and "MASTER_PORT" in r.stderr


def test_launch_cost_model_and_frames_per_launch():
    """dp.launch_cost: rounds of GEMM tiles of a packed launch (one tile per CU and round; 256-row tiles, or 192-row ones at 0.8 where
    they give fewer / shorter rounds) - the model behind dp.choose_max_frames.  Whole rounds cost least per frame; the cap is chosen from
    the directory's lengths, deterministically, and scales with the CUs the acoustic stage owns."""
    from covomix_amd import dp
    full = dp.launch_cost(8192)                    # 16384 rows = 64 row panels: qkv 3 + out 1 + ff1 4 + ff2 4 + skip 1 rounds
    assert full == 13.0
    assert dp.launch_cost(8150) == 13.0            # (the last panel is ragged: same rounds)
    # 9,298 rows: to_qkv 37 x 12 tiles = 2 rounds of 256-row tiles; N = 1024 products on 192-row tiles: one round at 0.75 (K = dim) / 0.8 (K > dim);
    # ff1 (16 column tiles): 3 rounds of 256-row tiles, 4 of 192-row ones at 0.75 - the same; the mixed form pays its launch boundary
    assert dp.launch_cost(4649) == pytest.approx(2 + 0.75 + 3 + 4 * 0.8 + 0.8)
    assert dp.launch_cost(4649) / 4649 > full / 8192                               # a part-empty launch costs more per frame
    assert dp.launch_cost(7168, cus=224) == 13.0                                   # the same whole rounds on 224 CUs
    lengths = [400, 1200, 451, 1149, 503, 1097, 555, 1044, 607, 993, 659, 941, 711, 889, 763, 837]      # the ragged test directory
    assert dp.choose_max_frames(lengths, 32) == 8192
    assert dp.choose_max_frames(lengths, 32, cus=224) in (7168, 10752, 14336, 21504)
    assert dp.choose_max_frames([1000] * 24, 32) == 8192                           # 24,000 frames: three whole-round launches tie any bigger one: smallest cap
    assert dp.choose_max_frames(lengths, 32) == dp.choose_max_frames(list(lengths), 32)


def test_launch_ranks_reports_the_rank_that_failed(tmp_path, capfd):
    """A rank that dies takes the job down; launch_ranks then prints every rank's stderr tail so that the first multi-GPU run is
    diagnosable from its log (round-4 review item 8) - and a healthy rank's stdout stays untouched (rank 0's JSON line is ONE bare line)."""
    from covomix_amd import dp
    script = tmp_path / "ranks_fail.py"
    script.write_text(f"""
import sys, os
sys.path.insert(0, {ROOT!r})
rank = int(os.environ["RANK"])
if rank == 0:
    print('{{"n_gpus": 2}}', flush=True)
if rank == 1:
    print("rank one could not bring its communicator up: simulated", file=sys.stderr, flush=True)
    os._exit(17)                     # (an abort, not a Python exception)
import time; time.sleep(1.0)
""")
    rc = dp.launch_ranks(str(script), [], 2)
    out, err = capfd.readouterr()
    assert rc != 0
    assert '{"n_gpus": 2}' in out.splitlines()
    assert "--- rank 1 ---" in err and "rank one could not bring its communicator up: simulated" in err.split("--- rank 1 ---")[1]


def test_every_python_source_compiles():
    """Host modules that only run on a GPU box (t2s, hubert, generation, tools) are still byte-compiled here, so a syntax
    error cannot reach the GPU tier unnoticed."""
    import compileall
    for sub in ("neurips2024-covomix_amd", "tools", "tests", "oracle"):
        assert compileall.compile_dir(os.path.join(ROOT, sub), quiet=1, force=False, maxlevels=2), sub
    for f in ("bench.py", "__graft_entry__.py", "monologue_generation.py", "dialogue_generation.py", "covomix_amd.py"):
        assert compileall.compile_file(os.path.join(ROOT, f), quiet=1), f
    import covomix_amd.t2s, covomix_amd.generation, covomix_amd.hubert, covomix_amd.mel, covomix_amd.vocoder  # noqa: F401,E401


def test_capture_gate_shared_entries_overlap_and_a_capture_is_alone():
    """ops._CaptureGate (host threads vs stream capture on HIP): shared holders run together, an exclusive holder runs alone,
    a thread that holds the gate shared can take it exclusive (two such threads at once: no deadlock), nested entries are free,
    and a waiting capture is not starved by a stream of new shared entries."""
    import threading
    import time
    import covomix_amd.ops as ops
    gate = ops._CaptureGate()
    state = dict(shared=0, excl=0, max_shared=0, bad=0, captures=0)
    lock = threading.Lock()

    def entry(i):
        for k in range(40):
            with gate.shared():
                with lock:
                    state["shared"] += 1
                    state["max_shared"] = max(state["max_shared"], state["shared"])
                    state["bad"] += state["excl"] != 0
                with gate.shared():                      # nested (sample inside synthesis_sample)
                    time.sleep(0.0005)
                if k % 10 == i:                          # "first call of a shape": capture from inside the entry point
                    with lock:
                        state["shared"] -= 1
                    with gate.exclusive():
                        with lock:
                            state["excl"] += 1
                            state["bad"] += (state["excl"] != 1) + (state["shared"] != 0)
                        with gate.shared(), gate.exclusive():
                            time.sleep(0.001)
                        with lock:
                            state["excl"] -= 1
                            state["captures"] += 1
                    with lock:
                        state["shared"] += 1
                with lock:
                    state["shared"] -= 1
    ts = [threading.Thread(target=entry, args=(i,)) for i in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(60)
    assert not any(t.is_alive() for t in ts), "deadlock"
    assert state["bad"] == 0 and state["captures"] == 16 and state["max_shared"] >= 2, state
    assert gate._readers == 0 and not gate._writer and gate._waiting == 0


@pytest.mark.parametrize("nb", [8, 64])
def test_t2s_uniform_buffer_covers_every_position_a_chunked_decode_reads(nb):
    """text2semantic host sizing (no kernel runs): a lock-step decode replays whole chunks of CHUNK steps and its sampling kernel
    reads the uniform draws of every position it reaches (up to the decoder's max_length); with the dialogue capacity equal to the
    batch, the last dialogue's last read must stay inside the buffer whatever the call's max_length."""
    import numpy as np
    from conftest import GOLDEN
    from covomix_amd.t2s import CHUNK, TextToSemanticDecoder
    g = np.load(os.path.join(GOLDEN, "t2s_cosingle_small.npz"))
    sd = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w::")}
    model = TextToSemanticDecoder(sd, torch.device("cpu"), max_length=2048)
    S, V = model.d["streams"], model.d["vocab"]
    for m in (1, 15, 17, 20, 33, 2047):
        model._ensure(nb, nb, m)
        steps = model._descriptor(1.0, nb).uniform_steps
        last = min(-(-m // CHUNK) * CHUNK, model.max_length) - 1                 # the last position the chunks reach
        assert model._dialogues == nb and steps >= -(-m // CHUNK) * CHUNK, (m, steps)
        assert model.buf["uniforms"].numel() >= model._dialogues * steps * S * V
        assert (((nb - 1) * steps + last) * S + S - 1) * V + V - 1 < model.buf["uniforms"].numel()
        assert model._uniform_view(nb).shape == (nb, steps, S, V)
