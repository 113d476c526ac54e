#!/usr/bin/env python3
"""Dev: the ragged HuBERT tokeniser call (HubertEncoder.extract_features_many) against a loop of one-utterance calls.

  MODE=loop | many   N in {1, 2, 4, 8, 16, 32} prompts, all 10 s long and lengths mixed 3 - 10 s (seeded), layer 12, synthetic
                     HuBERT-Base weights, waveforms resident on the device: ms per prompt between two device synchronisations and the
                     effective shader clock of each timed region (ops.clock_stamps).  One mode per process, so that runs can alternate.
  MODE=cli           generation.run in dialogue mode (covomix, tokens from files) on DIALOGUES dialogues whose 2 x DIALOGUES prompts are
                     16 kHz wav files tokenised through --hubert_ckpt, with --hubert_batch HUBERT_BATCH; wall seconds of PASSES passes
                     after one warm-up pass.
Env: MODE, PROMPTS (default 128: each N is timed over about that many prompts), DIALOGUES=16, HUBERT_BATCH=1, PASSES=3, OUT=/tmp/hubert_many."""
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import covomix_amd.synthetic as syn
from covomix_amd import ops

MODE = os.environ.get("MODE", "many")
NS = (1, 2, 4, 8, 16, 32)


def wave(n, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n) / 16000.0
    return 0.1 * torch.sin(2 * np.pi * 220 * t) + 0.05 * torch.sin(2 * np.pi * 1710 * t + 0.3) + 0.02 * torch.randn(n, generator=g) + 0.01


def clock(c0, c1):
    r = ops.clock_from_stamps(c0, c1)
    return round(r["mhz"]) if r else None


def extract_bench():
    from covomix_amd.hubert import HubertEncoder
    enc = HubertEncoder(syn.hubert_state_dict(seed=0))
    mixed = np.random.default_rng(0).integers(48000, 160001, size=max(NS)).tolist()
    total = int(os.environ.get("PROMPTS", "128"))
    for tag, lengths in (("10s", [160000] * max(NS)), ("3-10s", mixed)):
        waves = [wave(n, 100 + i).cuda() for i, n in enumerate(lengths)]
        for N in NS:
            batch = waves[:N]
            call = (lambda: enc.extract_features_many(batch, 12)) if MODE == "many" else (lambda: [enc.extract_features(w, 12) for w in batch])
            call(); call()
            reps = max(3, total // N)
            torch.cuda.synchronize(); c0 = ops.clock_stamps(); torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                call()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            c1 = ops.clock_stamps(); torch.cuda.synchronize()
            print(json.dumps({"mode": MODE, "lengths": tag, "N": N, "seconds_of_audio": round(sum(lengths[:N]) / 16000, 1), "reps": reps,
                              "ms_per_call": round(dt / reps * 1e3, 3), "ms_per_prompt": round(dt / reps / N * 1e3, 3),
                              "sclk_eff_mhz": clock(c0, c1)}), flush=True)


def cli_bench():
    import contextlib
    import io
    import types
    import joblib
    from scipy.io.wavfile import write
    from covomix_amd import generation
    tmp = os.environ.get("OUT", "/tmp/hubert_many")
    os.makedirs(tmp, exist_ok=True)
    sd = {k: torch.from_numpy(v) for k, v in syn.synth_state_dict(syn.acoustic_param_shapes(), seed=0).items()}
    torch.save({"state_dict": {"cfm_wrapper.CoVoMix." + k: v for k, v in sd.items()}, "hyper_parameters": {"twocondition_oneoutput": True}},
               os.path.join(tmp, "acous.ckpt"))
    h = dict(syn.HIFIGAN_COVOMIX_CONFIG)
    vsd = {k: torch.from_numpy(v) for k, v in syn.synth_state_dict(syn.hifigan_param_shapes(h), seed=0).items()}
    os.makedirs(os.path.join(tmp, "voc"), exist_ok=True)
    torch.save({"generator": vsd}, os.path.join(tmp, "voc", "g_00000001"))
    json.dump(h, open(os.path.join(tmp, "voc", "vocoder_config.json"), "w"))
    hub = os.path.join(tmp, "hubert.pt")
    torch.save({"cfg": {"model": {"_name": "hubert", "extractor_mode": "default", "layer_norm_first": False},
                        "task": {"_name": "hubert_pretraining", "sample_rate": 16000, "normalize": False}},
                "model": {k: torch.from_numpy(v) for k, v in syn.hubert_state_dict(seed=0).items()}}, hub)
    km = os.path.join(tmp, "km.bin")
    joblib.dump(types.SimpleNamespace(cluster_centers_=syn.hubert_kmeans_centers(seed=0)), km)
    tdir, pdir, sdir = (os.path.join(tmp, d) for d in ("text", "prompt", "out"))
    os.makedirs(tdir, exist_ok=True); os.makedirs(pdir, exist_ok=True)
    g = np.random.RandomState(7)
    T, P = 1008, 400                       # 1008-frame dialogues, 8-s prompts (400 frames of 20 ms)
    for i in range(int(os.environ.get("DIALOGUES", "16"))):
        for suf in ("_1", "_2"):
            pcm = np.clip(np.round(wave(320 * (P - 1) + 400, 10 * i + len(suf) + (suf == "_2")).numpy() * 32768.0), -32768, 32767).astype(np.int16)
            write(os.path.join(pdir, f"u{i:02d}{suf}.wav"), 16000, pcm)
            np.save(os.path.join(pdir, f"u{i:02d}{suf}.mel.npy"), (g.randn(80, P) * 2 - 6).astype(np.float32))
        np.save(os.path.join(tdir, f"u{i:02d}.semantic.npy"), g.randint(0, 500, size=(2, T - P)))
    argv = ["--acous_ckpt", os.path.join(tmp, "acous.ckpt"), "--hifigan_ckpt", os.path.join(tmp, "voc", "g_00000001"),
            "--text_dir", tdir, "--prompt_dir", pdir, "--saved_dir", sdir, "--mode", "covomix", "--seed", "1",
            "--hubert_ckpt", hub, "--km_path", km, "--hubert_batch", os.environ.get("HUBERT_BATCH", "1")]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for k in range(int(os.environ.get("PASSES", "3")) + 1):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                generation.run(True, argv)
            torch.cuda.synchronize(); dt = time.perf_counter() - t0
            st = generation.run.last_stats
            if k:
                print(json.dumps({"mode": "cli", "hubert_batch": int(os.environ.get("HUBERT_BATCH", "1")), "pass": k, "wall_s": round(dt, 4),
                                  "prepass_s": round(st["hubert_prepass_seconds"], 4), "run_s": round(st["seconds"], 4),
                                  "load_s": round(st["load_seconds"], 4)}), flush=True)


if __name__ == "__main__":
    cli_bench() if MODE == "cli" else extract_bench()
