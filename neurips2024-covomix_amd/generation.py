"""Driver behind monologue_generation.py / dialogue_generation.py at the repo root.

Keeps the reference CLI (monologue_generation.py:324-333: --t2s_ckpt --acous_ckpt --hifigan_ckpt --text_dir
--prompt_dir --saved_dir --seed --mode) and the per-utterance flow of covosingle()/covosinx()/covomix()
(monologue_generation.py:146-304, dialogue_generation.py:145-329) for the stages this build covers:
token/prompt assembly -> synthesis_sample (cond_scale 0.7) -> frame selection -> HiFi-GAN -> int16 wav.

Upstream stages:
  * text2semantic (N1, built: t2s.py): with --t2s_ckpt, `<text_dir>/<name>.text_ids.npy` (the BERT token ids of the
      cleaned text, what tokenizer(...).input_ids holds in cosingle_pred / comix_pred, :179-186, :307-319) or
      `<name>.txt` (needs the bert-base-uncased vocabulary in the local transformers cache - a third-party asset
      this repo does not ship) is decoded on the GPU; otherwise `<text_dir>/<name>.semantic.npy` holds already
      predicted tokens (covosingle / covosinx: int array [n]; covomix: [2, n] or flat [2n], split at half).
  * prompt mel extraction (N3, built: mel.py): `<prompt_dir>/<name>.mel.npy` ([80, T] log-mel) if present, else the
      log-mel of `<prompt_dir>/<name>.wav` (8 kHz) computed on the GPU (--mel_batch N > 1: all such prompts of the run
      up front, N per ragged call, instead of one call per prompt; the same mels bit for bit)
  * prompt tokens (N4, built: hubert.py): `<prompt_dir>/<name>.hubert_code.npy` if present (what
      fairseq-hubert/get_fisher_semantic_tokens.py wrote offline), else, with --hubert_ckpt and --km_path, the HuBERT
      layer-12 + k-means codes of `<prompt_dir>/<name>.wav` computed on the GPU (resampled to the checkpoint's rate;
      --hubert_batch N > 1: all such prompts of the run up front, N per ragged call, instead of one call per prompt);
      dialogue mode uses `<name>_1.*` and `<name>_2.*` (dialogue_generation.py:285-286)
Dialogue covosingle / covosinx decode the text turn by turn (split at "[spkchange]") with alternating prompts / streams
exactly as dialogue_generation.py:145-193, :205-272 do; pre-tokenised turns are `<name>.turn<k>.semantic.npy` /
`<name>.turn<k>.text_ids.npy`.
New relative to the reference: utterances are sharded over ranks (torchrun; the plan is built from file names and sizes
only, so every rank computes the same one and decodes only its own utterances), batched by equal length through the
acoustic model and by equal generated length through the vocoder; the sampled tokens and the ODE noise of an utterance
are seeded from (--seed, name, turn) and therefore do not depend on the number of ranks.
"""
from __future__ import annotations

import glob
import json
import os
import random
from argparse import ArgumentParser

import numpy as np
import torch

from . import assembly, dp
from .acoustic import evaluation_times, resolve_grid, resolve_method
from .conditional_model import CoVoMixModel
from .vocoder import AttrDict, Generator

COND_SCALE = 0.7    # every shipped caller (monologue_generation.py:171,238,298)


def build_parser() -> ArgumentParser:
    p = ArgumentParser()
    p.add_argument("--t2s_ckpt", type=str, default=None, help="text2semantic checkpoint (CoSingle / CoMix); without it "
                   "<name>.semantic.npy files are read from --text_dir")
    p.add_argument("--acous_ckpt", type=str, default="/pretrained_models/comix.ckpt", help="acoustic model checkpoint")
    p.add_argument("--hifigan_ckpt", type=str, default="/pretrained_models/vocoder.ckpt", help="vocoder checkpoint")
    p.add_argument("--text_dir", type=str, default="test/test_dir", help="directory with <name>.semantic.npy")
    p.add_argument("--prompt_dir", type=str, default="test/monologue_prompt_dir", help="directory with acoustic prompts")
    p.add_argument("--saved_dir", type=str, default=".saved_dir", help="target directory")
    p.add_argument("--seed", type=int, default=30, help="random seed")
    p.add_argument("--mode", type=str, choices=["covosingle", "covosinx", "covomix"], default="covosingle")
    p.add_argument("--max_batch", type=int, default=32, help="utterances per launch at most (any lengths: they are packed back to back)")
    p.add_argument("--max_frames", type=int, default=None, help="frames per launch (sum over its utterances); default: chosen from the "
                   "directory's lengths among 8192 / 12288 / 16384 / 24576 by the cost of the packing in rounds of GEMM tiles "
                   "(dp.choose_max_frames); 14336 under --pipeline on (two rounds on the 224 CUs the acoustic stage owns)")
    p.add_argument("--pipeline", type=str, choices=["auto", "batch", "on", "serial", "off"], default="auto",
                   help="extension: how text2semantic (--t2s_ckpt) and the acoustic stage share the GPU.  batch (= auto when there is text "
                        "to decode): ALL turns first, through 64 continuously refilled decode slots on the whole chip, then one global packing "
                        "of the acoustic work - the fastest schedule measured (bench.py `c5`: the decode costs 4.7 ms per dialogue at 64 "
                        "slots against 89 ms of solve; hiding it on a CU partition costs the solve 12.5 %% of the chip).  on: decode the "
                        "NEXT utterances on a CU-masked side stream while the acoustic model and the vocoder work on the current batch "
                        "(covomix_amd/pipeline.py: first audio sooner); serial = the batches of `on` on the same two streams one after "
                        "the other (bit-identical output, for comparison); off = batch with the decode outside the timed region")
    p.add_argument("--hubert_ckpt", type=str, default=None, help="HuBERT checkpoint (fairseq layout): tokenise <name>.wav prompts "
                   "that have no <name>.hubert_code.npy (fairseq-hubert/get_fisher_semantic_tokens.py:23-24)")
    p.add_argument("--km_path", type=str, default=None, help="k-means model (joblib) for --hubert_ckpt")
    p.add_argument("--hubert_batch", type=int, default=1, help="with --hubert_ckpt: N > 1 tokenises the run's wav prompts up front, N per "
                   "ragged call (HubertTokenizer.wav2code_many; 16 is the measured recommendation); 1 = one call per prompt as it is needed")
    p.add_argument("--mel_batch", type=int, default=1, help="extension: N > 1 extracts the mels of the run's wav prompts that have no "
                   "<name>.mel.npy up front, N per ragged call (mel.extract_mel_many; bit-identical mels); 1 = one extract_mel call per "
                   "prompt as it is needed")
    p.add_argument("--nfe", type=int, default=32, help="extension: CFG-combined field evaluations of the midpoint solver (32 = the "
                   "reference's ode_step_size 0.0625, acoustic.py:586-591; 64 = BASELINE config 5's 64-step setting)")
    p.add_argument("--ode_method", type=str, default="midpoint", help="extension: the fixed-grid solver (the reference's "
                   "torchdiffeq_ode_method, acoustic.py:560-591): euler, midpoint, heun2, heun3, rk4 (torchdiffeq's 3/8 rule) or rk4_classic; "
                   "--nfe must be a multiple of its stages (1, 2, 2, 3, 4, 4)")
    p.add_argument("--ode_grid", type=str, default="uniform", help="extension: the time grid of the solve - uniform (the reference's), "
                   "cosine, sway:<s> (-1 <= s <= 1.75: s < 0 steps finely first), or the path of a JSON list of nfe / stages + 1 points as "
                   "tools/fit_time_grid.py writes it")
    p.add_argument("--ode_error_json", type=str, default=None, help="extension: also measure the method's embedded error estimate and "
                   "write, per utterance, the grid and the delta_rms / state_rms tables per step (acoustic.SolveError) to this file; the "
                   "audio is the same bit for bit (ranks other than 0 append .rank<r>)")
    p.add_argument("--t2s_temperature", type=float, default=None, help="extension: sampling temperature of the text2semantic decode "
                   "(default: the reference's 1.0)")
    p.add_argument("--t2s_cond_scale", type=float, default=None, help="extension: classifier-free guidance of the text2semantic decode "
                   "(> 1 needs a checkpoint trained with cond_drop_prob > 0, one-output models; default: the reference's 1.0 = off)")
    p.add_argument("--t2s_filter", type=str, choices=["top_k", "top_p"], default=None, help="extension: logit filter of the text2semantic "
                   "decode (text2semantic.py:118-132; default: the reference's top_k)")
    p.add_argument("--t2s_filter_thres", type=float, default=None, help="extension: the filter's thres (top_k: k = ceil(thres * vocab), "
                   "reference default 0.1; top_p: the nucleus mass, reference default 0.9, inside (0, 1))")
    p.add_argument("--t2s_top_k", type=int, default=None, help="extension: an explicit k for --t2s_filter top_k (overrides the thres)")
    p.add_argument("--t2s_repetition_penalty", type=float, default=None, help="extension: history rule of the text2semantic decode - every "
                   "token id a stream has already emitted (inside --t2s_repetition_window) is penalised once before the filter: "
                   "l > 0 ? l / penalty : l * penalty; > 0, 1 is off")
    p.add_argument("--t2s_repetition_window", type=int, default=None, help="extension: the last W tokens of a stream the repetition penalty "
                   "looks at (0, the default: all of them)")
    p.add_argument("--t2s_no_repeat_ngram", type=int, default=None, help="extension: history rule - no n-gram of this size occurs twice in a "
                   "stream (0..8; 0 is off)")
    p.add_argument("--t2s_min_length", type=int, default=None, help="extension: history rule - the eos cannot be selected below this many "
                   "steps")
    p.add_argument("--t2s_best_of", type=int, default=1, help="extension: decode this many candidates per turn through the continuously "
                   "refilled slots and keep the one the model finds most likely (largest mean token log-probability; 1 = off: today's files)")
    p.add_argument("--t2s_best_of_select", choices=("logprob", "mbr"), default="logprob", help="extension: the rule --t2s_best_of keeps a "
                   "candidate by - logprob: the largest mean token log-probability (today's files); mbr: consensus (minimum Bayes risk) - the "
                   "candidate with the smallest total edit distance to the turn's other candidates, ties to the larger log-probability; "
                   "needs --t2s_best_of > 1 or --t2s_best_of_temperatures")
    p.add_argument("--t2s_best_of_temperatures", type=str, default=None, help="extension: T1,T2,... - --t2s_best_of with one temperature per "
                   "candidate: candidate c of every turn is decoded at temperature c (implies --t2s_best_of = their number)")
    p.add_argument("--t2s_mixed_guidance", action="store_true", help="extension: turns whose side files make some of them guided and "
                   "others not are decoded in ONE call through one slot pool instead of two calls (the same files either way)")
    p.add_argument("--t2s_prefill", action="store_true", help="extension: turns with a <name>.prefix.semantic.npy take their prefix through one "
                   "causal full-sequence pass instead of one decode step per prefix token (fp32-class, not bit-identical to the steps; such "
                   "turns decode in windows of as many turns as the slots hold; not with --t2s_mixed_guidance); other turns are unaffected")
    p.add_argument("--t2s_beam_size", type=int, default=0, help="extension: beam search with this many hypotheses per turn (1..16) instead of "
                   "sampling - deterministic: no draws, temperature and filter unused; not together with --t2s_best_of > 1 or guidance "
                   "(0 = off: sampling, today's files)")
    p.add_argument("--t2s_beam_rules", action="store_true", help="extension: lets --t2s_beam_size run under the history rules "
                   "--t2s_no_repeat_ngram and --t2s_min_length (and those two keys of a turn's <name>.t2s.json): candidates are removed along "
                   "every hypothesis' own history, scores stay the model's log-probabilities; --t2s_repetition_penalty stays refused")
    p.add_argument("--t2s_beam_guided", action="store_true", help="extension: lets --t2s_beam_size run under guidance (--t2s_cond_scale > 1): "
                   "every hypothesis takes a slot pair, so a wave holds half as many turns (one-output models)")
    p.add_argument("--gpus", type=int, default=1, help="extension: from a plain shell, start this many ranks (one per GPU, "
                   "utterances sharded; under torch.distributed.run the launcher's WORLD_SIZE is used instead)")
    return p


HEAD_START = 16     # utterances read before the first launch of a large directory (generation.run, --pipeline off)
_HUBERT = None      # HubertTokenizer, built by main() when --hubert_ckpt / --km_path are given
_HUBERT_CODES: dict = {}   # (prompt_dir, prompt name) -> code string, filled by the --hubert_batch pre-pass
_PROMPT_MELS: dict = {}    # (prompt_dir, prompt name) -> [80, T] log-mel, filled by the --mel_batch pre-pass


def _load_prompt(prompt_dir: str, name: str):
    code = os.path.join(prompt_dir, name + ".hubert_code.npy")
    if os.path.isfile(code) or _HUBERT is None:
        tok = torch.from_numpy(np.load(code).astype(np.int64))
    elif (prompt_dir, name) in _HUBERT_CODES:              # tokenised by the --hubert_batch pre-pass
        tok = torch.tensor([int(c) for c in _HUBERT_CODES[(prompt_dir, name)].split(" ")], dtype=torch.int64)
    else:                                                # encoder.wav2code(file, 1) (get_fisher_semantic_tokens.py:35-37, row N4)
        tok = torch.tensor([int(c) for c in _HUBERT.wav2code(os.path.join(prompt_dir, name + ".wav"), 1).split(" ")], dtype=torch.int64)
    npy = os.path.join(prompt_dir, name + ".mel.npy")
    if os.path.isfile(npy):
        mel = torch.from_numpy(np.load(npy).astype(np.float32))
    elif (prompt_dir, name) in _PROMPT_MELS:               # extracted by the --mel_batch pre-pass
        mel = _PROMPT_MELS[(prompt_dir, name)]
    else:                                                  # extract_mel(prompt wav), monologue_generation.py:62-74 (row N3)
        from .mel import extract_mel
        mel = extract_mel(os.path.join(prompt_dir, name + ".wav"))
    return assembly.truncate_prompt(tok, mel)            # -> tokens [Tp], mel [Tp, 80]


def prompt_names(names, dialogue: bool):
    """The prompt files `_build_items` will ask `_load_prompt` for: <name> for a monologue, <name>_1 and <name>_2 for a dialogue."""
    return [n + suffix for n in names for suffix in (("_1", "_2") if dialogue else ("",))]


def pretokenise_prompts(prompt_dir: str, names, batch: int) -> int:
    """--hubert_batch N > 1: tokenise every prompt of the run that has no <name>.hubert_code.npy in groups of N
    (HubertTokenizer.wav2code_many) and keep the codes for `_load_prompt`.  -> number of prompts tokenised."""
    todo = [n for n in dict.fromkeys(names) if not os.path.isfile(os.path.join(prompt_dir, n + ".hubert_code.npy"))]
    for i in range(0, len(todo), batch):
        group = todo[i:i + batch]
        for n, code in zip(group, _HUBERT.wav2code_many([os.path.join(prompt_dir, n + ".wav") for n in group], 1)):
            _HUBERT_CODES[(prompt_dir, n)] = code
    return len(todo)


def preextract_prompt_mels(prompt_dir: str, names, batch: int) -> int:
    """--mel_batch N > 1: extract the mel of every prompt of the run that has no <name>.mel.npy in groups of N (mel.extract_mel_many:
    what extract_mel returns for the file, bit for bit) and keep them for `_load_prompt`.  -> number of prompts extracted."""
    from .mel import extract_mel_many
    todo = [n for n in dict.fromkeys(names) if not os.path.isfile(os.path.join(prompt_dir, n + ".mel.npy"))]
    for i in range(0, len(todo), batch):
        group = todo[i:i + batch]
        for n, mel in zip(group, extract_mel_many([os.path.join(prompt_dir, n + ".wav") for n in group])):
            _PROMPT_MELS[(prompt_dir, n)] = mel
    return len(todo)


def remove_punctuation(text: str) -> str:
    """monologue_generation.py:108-114."""
    punctuation = '''!()-{};:'"\\,<>./?@#$%^&*_~'''
    text = text.lower()
    for x in text:
        if x in punctuation:
            text = text.replace(x, "")
    return text


_TOKENIZER = None


def _stable_seed(seed: int, name: str, turn: int, salt: int) -> int:
    """Per-utterance RNG seed that depends only on (--seed, utterance name, turn): the sampled tokens and the ODE noise of an
    utterance are the same whatever the number of ranks, the sharding or the batching."""
    import zlib
    return (zlib.crc32(f"{name}|{turn}|{salt}".encode()) ^ (int(seed) * 0x9E3779B1)) & 0x7FFFFFFF


def _turn_sources(text_dir: str, name: str, multi_turn: bool, have_t2s: bool):
    """The text turns of one utterance as a list of ("sem", path) / ("ids", path) / ("txt", string) sources.
    Multi-turn (dialogue covosingle / covosinx: the reference splits the text at "[spkchange]" and decodes every turn on its
    own, dialogue_generation.py:160-165, :243-247): `<name>.turn<k>.semantic.npy` or `<name>.turn<k>.text_ids.npy`, k = 0, 1,
    ..., else `<name>.txt` split at "[spkchange]".  Otherwise (or when no turn files exist) the whole utterance is one turn:
    `<name>.semantic.npy`, `<name>.text_ids.npy` or `<name>.txt`."""
    j = lambda suffix: os.path.join(text_dir, name + suffix)
    if multi_turn:
        turns, k = [], 0
        while True:
            if os.path.isfile(j(f".turn{k}.semantic.npy")):
                turns.append(("sem", j(f".turn{k}.semantic.npy")))
            elif have_t2s and os.path.isfile(j(f".turn{k}.text_ids.npy")):
                turns.append(("ids", j(f".turn{k}.text_ids.npy")))
            else:
                break
            k += 1
        if turns:
            return turns
        if have_t2s and os.path.isfile(j(".txt")) and not os.path.isfile(j(".semantic.npy")) and not os.path.isfile(j(".text_ids.npy")):
            with open(j(".txt"), "r", encoding="utf-8") as f:
                return [("txt", t) for t in f.read().split("[spkchange]")]
    if os.path.isfile(j(".semantic.npy")):
        return [("sem", j(".semantic.npy"))]
    if have_t2s and os.path.isfile(j(".text_ids.npy")):
        return [("ids", j(".text_ids.npy"))]
    if have_t2s and os.path.isfile(j(".txt")):
        with open(j(".txt"), "r", encoding="utf-8") as f:
            return [("txt", f.read())]
    raise FileNotFoundError(f"{name}: no .semantic.npy" + (" / .text_ids.npy / .txt" if have_t2s else " (and no --t2s_ckpt)") + f" in {text_dir}")


def _source_cost(src) -> int:
    """Rank-independent size of a turn (bytes of its file or characters of its text): what the sharding plan is built on."""
    kind, v = src
    return len(v) if kind == "txt" else os.path.getsize(v)


def _tokenize(txt: str) -> torch.Tensor:
    global _TOKENIZER
    if _TOKENIZER is None:
        from transformers import BertTokenizer
        tok = BertTokenizer.from_pretrained("bert-base-uncased", local_files_only=True)
        for t in ("[laughter]", "[spkchange]", "[spka]", "[spkb]", "[partialoverlap]", "[backchannel]"):
            tok.add_tokens([t])
        _TOKENIZER = tok
    return _TOKENIZER([remove_punctuation(txt).lower()], padding=True, truncation=True, return_tensors="pt").input_ids


def t2s_sampling_kwargs(args) -> dict:
    """The --t2s_* flags as keywords of CoVoMixModel.synthesis_sample_text2semantic; a flag that was not given adds nothing (the
    facade's defaults are the reference's behaviour)."""
    kw = {}
    if args.t2s_temperature is not None:
        kw["temprature"] = float(args.t2s_temperature)
    if args.t2s_cond_scale is not None:
        kw["cond_scale"] = float(args.t2s_cond_scale)
    if args.t2s_filter is not None:
        kw["filter_logits_fn"] = args.t2s_filter
    fkw = {}
    if args.t2s_filter_thres is not None:
        fkw["thres"] = float(args.t2s_filter_thres)
    if args.t2s_top_k is not None:
        if (args.t2s_filter or "top_k") != "top_k":
            raise ValueError("--t2s_top_k goes with --t2s_filter top_k")
        fkw["k"] = int(args.t2s_top_k)
    if fkw:
        kw["filter_fn_kwargs"] = fkw
    best_of = int(getattr(args, "t2s_best_of", 1))
    if best_of < 1:
        raise ValueError(f"--t2s_best_of {best_of}: at least 1")
    if best_of > 1:
        kw["best_of"] = best_of
    if getattr(args, "t2s_best_of_temperatures", None):
        temps = tuple(float(t) for t in str(args.t2s_best_of_temperatures).split(",") if t.strip())
        if not temps or any(not t >= 0.0 for t in temps):
            raise ValueError(f"--t2s_best_of_temperatures {args.t2s_best_of_temperatures}: a comma-separated list of temperatures >= 0")
        if best_of > 1 and best_of != len(temps):
            raise ValueError(f"--t2s_best_of {best_of} disagrees with the {len(temps)} --t2s_best_of_temperatures")
        kw["best_of_temperatures"] = temps
        best_of = len(temps)
    select = getattr(args, "t2s_best_of_select", None) or "logprob"
    if select not in ("logprob", "mbr"):
        raise ValueError(f"--t2s_best_of_select {select}: logprob or mbr")
    beam = int(getattr(args, "t2s_beam_size", 0))
    if select == "mbr":
        if beam:
            raise ValueError("--t2s_best_of_select mbr does not combine with --t2s_beam_size (consensus is over sampled candidates)")
        if best_of < 2:
            raise ValueError("--t2s_best_of_select mbr needs candidates to choose among: --t2s_best_of > 1 or --t2s_best_of_temperatures")
        kw["best_of_select"] = "mbr"
    if beam:
        if not 1 <= beam <= 16:
            raise ValueError(f"--t2s_beam_size {beam}: 0 (sampling) or 1..16")
        guided_beam = bool(getattr(args, "t2s_beam_guided", False))
        if best_of > 1 or (kw.get("cond_scale", 1.0) > 1.0 and not guided_beam):
            raise ValueError("--t2s_beam_size does not combine with --t2s_best_of > 1 or, without --t2s_beam_guided, guidance "
                             "(--t2s_cond_scale > 1)")
        kw["beam_search_decode"], kw["beam_size"] = True, beam
        if guided_beam:
            kw["guided_beam"] = True
        if getattr(args, "t2s_beam_rules", False):
            kw["beam_rules"] = True
    if getattr(args, "t2s_mixed_guidance", False):
        kw["mixed_guidance"] = True
    if getattr(args, "t2s_prefill", False):
        if kw.get("mixed_guidance"):
            raise ValueError("--t2s_prefill does not combine with --t2s_mixed_guidance (the mixed pool's slots are armed on the device)")
        kw["prefill"] = True
    for flag, key, conv in T2S_RULE_FLAGS:
        if getattr(args, "t2s_" + flag, None) is not None:
            if beam and not (kw.get("beam_rules") and flag in T2S_BEAM_RULE_FLAGS):
                raise ValueError(f"--t2s_beam_size does not combine with the history rules (--t2s_{flag})" if not kw.get("beam_rules") else
                                 f"--t2s_beam_size with --t2s_beam_rules runs --t2s_no_repeat_ngram and --t2s_min_length, not --t2s_{flag}")
            kw[key] = conv(getattr(args, "t2s_" + flag))
    return kw


# the history rules: (flag without --t2s_ = key of <name>.t2s.json, facade keyword, conversion)
T2S_RULE_FLAGS = (("repetition_penalty", "repetition_penalty", float), ("repetition_window", "repetition_window", int),
                  ("no_repeat_ngram", "no_repeat_ngram_size", int), ("min_length", "min_length", int))
T2S_RULE_KEYWORDS = tuple(key for _, key, _ in T2S_RULE_FLAGS)
T2S_BEAM_RULE_FLAGS = ("no_repeat_ngram", "min_length")     # the history rules beam search runs (--t2s_beam_rules)


def _candidate_salt(c: int) -> int:
    """The salt of candidate c of a turn's text2semantic draws (--t2s_best_of): candidate 0 keeps the salt the single decode always had
    (1: the same files with --t2s_best_of 1); candidate c > 0 takes one that depends on c only (2 is the acoustic noise's)."""
    return 1 if c == 0 else 0x100 + int(c)


T2S_SIDE_FIELDS = ("temperature", "filter", "filter_thres", "top_k", "cond_scale") + tuple(flag for flag, _, _ in T2S_RULE_FLAGS)


def _turn_side_files(text_dir, name: str, k: int, src):
    """The optional side files of one text turn -> (settings dict or None, prefix tokens or None).
    `<stem>.t2s.json`: any of temperature, filter ("top_k" / "top_p"), filter_thres, top_k, cond_scale, repetition_penalty,
    repetition_window, no_repeat_ngram, min_length for this turn - they override the --t2s_* flags.  `<stem>.prefix.semantic.npy`: tokens the turn's decode continues from, in the layout of `<name>.semantic.npy` (flat:
    stream 1 then stream 2 on a two-output model, equally long).  <stem> is the turn's own file stem - `<name>.turn<k>` for a turn file,
    `<name>` for a whole-utterance file; the turns of a `<name>.txt` look for `<name>.turn<k>.*` and then take the utterance's
    `<name>.t2s.json` (the prefix `<name>.prefix.semantic.npy` goes to turn 0 only)."""
    kind, v = src
    if kind == "ids":
        stems = [(v[:-len(".text_ids.npy")], True)]
    elif text_dir is None:
        return None, None
    else:
        stems = [(os.path.join(text_dir, f"{name}.turn{k}"), True), (os.path.join(text_dir, name), k == 0)]
    settings = prefix = None
    for stem, with_prefix in stems:
        if settings is None and os.path.isfile(stem + ".t2s.json"):
            with open(stem + ".t2s.json", "r", encoding="utf-8") as f:
                settings = json.load(f)
            unknown = sorted(set(settings) - set(T2S_SIDE_FIELDS)) if isinstance(settings, dict) else ["(not an object)"]
            if unknown:
                raise ValueError(f"{stem}.t2s.json: unknown fields {unknown}; known: {list(T2S_SIDE_FIELDS)}")
        if prefix is None and with_prefix and os.path.isfile(stem + ".prefix.semantic.npy"):
            prefix = np.load(stem + ".prefix.semantic.npy").astype(np.int64)
    return settings, prefix


def _turn_sampling(sampling: dict, side) -> dict:
    """The facade keywords of ONE turn: the --t2s_* flags (t2s_sampling_kwargs) overridden by the turn's `.t2s.json`.  A filter named in
    the side file drops the flags' thres / k of ANOTHER filter."""
    kw = {k: sampling[k] for k in ("temprature", "cond_scale", "filter_logits_fn", "filter_fn_kwargs") + T2S_RULE_KEYWORDS if k in sampling}
    side = side or {}
    for flag, key, conv in T2S_RULE_FLAGS:
        if flag in side:
            kw[key] = conv(side[flag])
    if "temperature" in side:
        kw["temprature"] = float(side["temperature"])
    if "cond_scale" in side:
        kw["cond_scale"] = float(side["cond_scale"])
    fkw = dict(kw.get("filter_fn_kwargs") or {})
    if "filter" in side:
        if side["filter"] not in ("top_k", "top_p"):
            raise ValueError(f"t2s.json: filter must be 'top_k' or 'top_p', got {side['filter']!r}")
        if side["filter"] != kw.get("filter_logits_fn", "top_k"):
            fkw = {}
        kw["filter_logits_fn"] = side["filter"]
    if "filter_thres" in side:
        fkw["thres"] = float(side["filter_thres"])
    if "top_k" in side:
        if kw.get("filter_logits_fn", "top_k") != "top_k":
            raise ValueError("t2s.json: top_k goes with filter top_k")
        fkw["k"] = int(side["top_k"])
    kw["filter_fn_kwargs"] = fkw or None
    return kw


def _predict_turns(work, t2s, device, seed: int, slots: int = 64, sampling=None, text_dir=None) -> dict:
    """(name, turn) -> predicted semantic tokens (int64 numpy).  work: list of (name, turn, source).  Sources that are
    already tokens are read; the others are decoded by text2semantic on the GPU through `slots` decode slots, every turn
    with its OWN stream of uniforms (seeded from (--seed, name, turn)): the tokens do not depend on batching or ranks.
    sampling: the --t2s_* flags as keywords (t2s_sampling_kwargs).  text_dir: where the turns' optional side files live
    (_turn_side_files): per-turn settings and prefixes - the turns still share the slots (t2s.generate_many(settings=, prefixes=));
    guided and unguided turns run as two calls, or as one with --t2s_mixed_guidance.  Without side files nothing changes."""
    out, todo, side = {}, [], {}
    for name, k, (kind, v) in work:
        if kind == "sem":
            out[(name, k)] = np.load(v).astype(np.int64)
        else:
            ids = torch.from_numpy(np.load(v).astype(np.int64)).reshape(1, -1) if kind == "ids" else _tokenize(v)
            todo.append((name, k, ids))
            st, pre = _turn_side_files(text_dir, name, k, (kind, v))
            if st is not None or pre is not None:
                side[(name, k)] = (st, pre)
    if todo and t2s is None:
        raise RuntimeError("text sources need --t2s_ckpt")
    if todo:
        # ALL turns through t2s.generate_many: 64 continuously refilled decode slots - a turn that has sampled its eos frees its slot for
        # the next one on the device (the reference decodes turn by turn, dialogue_generation.py:297-304).  In windows of 256 turns: the
        # uniform draws of a window (8 MB per turn at 2048 steps) and its context k/v are resident while it decodes.
        # --t2s_best_of N: N candidates per turn, each with its own draws ([N, L, S, V] per turn), in windows of WINDOW / N turns - the
        # draws are made window by window, so the resident memory stays that of WINDOW records.
        from .t2s import WINDOW
        dec = t2s._get_t2s()
        S, V, L = dec.d["streams"], dec.d["vocab"], dec.max_length
        best_of = int((sampling or {}).get("best_of", 1))
        if (sampling or {}).get("best_of_temperatures"):
            best_of = len(sampling["best_of_temperatures"])
        win = max(1, WINDOW // best_of)
        for w in range(0, len(todo), win):
            part = todo[w:w + win]
            if (sampling or {}).get("beam_search_decode"):          # --t2s_beam_size: no draws, lock-step waves of 64 // beam_size turns
                bkw = dict(sampling)
                if sampling.get("beam_rules"):                      # --t2s_beam_rules: the two rules per turn, side files over flags
                    for flag, key, conv in T2S_RULE_FLAGS:
                        if flag in T2S_BEAM_RULE_FLAGS:
                            bkw[key] = [conv((side.get((name, k), (None, None))[0] or {}).get(flag, sampling.get(key, 0))) for name, k, _ in part]
                toks = t2s.synthesis_sample_text2semantic([ids.to(device) for _, _, ids in part], **bkw)
                for (name, k, _), t in zip(part, toks):
                    out[(name, k)] = t.cpu().numpy().astype(np.int64)
                continue
            uniforms = []
            for name, k, _ in part:
                draws = []
                for c in range(best_of):
                    g = torch.Generator(device=device).manual_seed(_stable_seed(seed, name, k, _candidate_salt(c)))
                    draws.append(torch.rand(L, S, V, device=device, generator=g))
                uniforms.append(draws[0] if best_of == 1 else torch.stack(draws))
            if not any((name, k) in side for name, k, _ in part):
                toks = t2s.synthesis_sample_text2semantic([ids.to(device) for _, _, ids in part], uniforms=uniforms, slots=slots,
                                                          **(sampling or {}))
                for (name, k, _), t in zip(part, toks):
                    out[(name, k)] = t.cpu().numpy().astype(np.int64)
                continue
            # turns with side files: every turn's own keywords as lists; guided and unguided turns do not share a launch - two calls -
            # unless --t2s_mixed_guidance puts them into one slot pool (one call, the same tokens)
            per = [_turn_sampling(sampling or {}, side.get((name, k), (None, None))[0]) for name, k, _ in part]
            rest = {k_: v for k_, v in (sampling or {}).items()
                    if k_ not in ("temprature", "cond_scale", "filter_logits_fn", "filter_fn_kwargs") + T2S_RULE_KEYWORDS}
            rule_off = dict(repetition_penalty=1.0, repetition_window=0, no_repeat_ngram_size=0, min_length=0)
            one_call = bool((sampling or {}).get("mixed_guidance"))
            for guided in ((None,) if one_call else (False, True)):
                sel = [i for i, kw_ in enumerate(per) if one_call or (kw_.get("cond_scale", 1.0) > 1.0) == guided]
                if not sel:
                    continue
                pres = []
                for i in sel:
                    pre = side.get((part[i][0], part[i][1]), (None, None))[1]
                    if pre is not None and (pre.ndim > 2 or pre.size == 0 or pre.size % S or (pre.ndim == 2 and pre.shape[0] != S)):
                        raise ValueError(f"{part[i][0]} turn {part[i][1]}: the prefix holds {pre.shape} tokens for {S} stream(s) of equal length")
                    pres.append(None if pre is None else torch.from_numpy(pre.reshape(S, -1)))
                toks = t2s.synthesis_sample_text2semantic([part[i][2].to(device) for i in sel], uniforms=[uniforms[i] for i in sel], slots=slots,
                                                          temprature=[per[i].get("temprature", 1.0) for i in sel],
                                                          cond_scale=[per[i].get("cond_scale", 1.0) for i in sel],
                                                          filter_logits_fn=[per[i].get("filter_logits_fn", "top_k") for i in sel],
                                                          filter_fn_kwargs=[per[i]["filter_fn_kwargs"] for i in sel],
                                                          prefix=pres if any(p_ is not None for p_ in pres) else None, **rest,
                                                          **{key: [per[i].get(key, rule_off[key]) for i in sel] for key in T2S_RULE_KEYWORDS
                                                             if any(key in per[i] for i in sel)})
                for i, t in zip(sel, toks):
                    out[(part[i][0], part[i][1])] = t.cpu().numpy().astype(np.int64)
    return out


def _build_items(mode: str, dialogue: bool, prompt_dir: str, name: str, preds):
    """One utterance -> list of (phoneme_ids, cond, mask) network inputs (one per OUTPUT SEGMENT; the segments' audio is
    concatenated).  preds: the predicted tokens of its turns, in order."""
    if mode == "covosingle":
        if not dialogue:                                                # monologue_generation.py:146-176
            sem, mel = _load_prompt(prompt_dir, name)
            return [assembly.build_monologue_inputs(sem, torch.from_numpy(preds[0].reshape(-1)), mel)]
        prompts = [_load_prompt(prompt_dir, name + "_1"), _load_prompt(prompt_dir, name + "_2")]
        return [assembly.build_monologue_inputs(prompts[k % 2][0], torch.from_numpy(p.reshape(-1)), prompts[k % 2][1])
                for k, p in enumerate(preds)]                           # dialogue_generation.py:145-193: turn k speaks with prompt k % 2
    if dialogue:
        sa, ma = _load_prompt(prompt_dir, name + "_1")
        sb, mb = _load_prompt(prompt_dir, name + "_2")
    else:
        sa, ma = _load_prompt(prompt_dir, name)
        sb, mb = sa, ma
    if mode == "covosinx":                # every turn on one stream, the other filled with 157; streams alternate per turn
        pa, pb = [], []                   # (dialogue_generation.py:243-259; one turn, stream A: monologue_generation.py:222-226)
        for k, p in enumerate(preds):
            t = torch.from_numpy(p.reshape(-1))
            sil = torch.ones_like(t) * assembly.SILENT_TOKEN
            pa.append(t if k % 2 == 0 else sil)
            pb.append(sil if k % 2 == 0 else t)
        pa, pb = torch.cat(pa), torch.cat(pb)
    else:                                 # covomix: one decode yields both streams, split at half (comix_pred, :316-320)
        flat = preds[0].reshape(-1)
        half = flat.shape[0] // 2
        pa, pb = torch.from_numpy(flat[:half].copy()), torch.from_numpy(flat[half:].copy())
    return [assembly.build_dialogue_inputs(sa, sb, pa, pb, ma, mb)]


def utterance_plan(text_dir: str, dialogue: bool, mode: str, have_t2s: bool, world: int):
    """(names, sources, plan): the sorted utterance names, their text turns, and plan[r] = the names rank r generates.
    RANK-INVARIANT by construction: built from file names and sizes only, before anything is sampled, so every rank
    computes the same plan, every utterance is generated exactly once, and a rank decodes only its own text."""
    stems = set()
    multi_turn = dialogue and mode in ("covosingle", "covosinx")
    for ext in (".semantic.npy",) + ((".text_ids.npy", ".txt") if have_t2s else ()):
        for p in glob.glob(os.path.join(text_dir, "*" + ext)):
            stem = os.path.basename(p)[: -len(ext)]
            if ext == ".semantic.npy" and stem.endswith(".prefix"):      # a turn's prefix (_turn_side_files), not an utterance
                continue
            if multi_turn and ".turn" in stem and stem.rsplit(".turn", 1)[1].isdigit():
                stem = stem.rsplit(".turn", 1)[0]
            stems.add(stem)
    names = sorted(stems)
    if not names:
        raise FileNotFoundError(f"no utterances in --text_dir {text_dir} (looked for *.semantic.npy"
                                + (", *.text_ids.npy, *.txt" if have_t2s else "; text sources need --t2s_ckpt") + ")")
    sources = {n: _turn_sources(text_dir, n, multi_turn, have_t2s) for n in names}
    cost = [sum(_source_cost(s) for s in sources[n]) for n in names]
    plan = [[names[i] for i in sorted(idx)] for idx in dp.shard_utterances(cost, world)]
    return names, sources, plan


def ode_grid_argument(spec: str):
    """--ode_grid: a grid's name as it is, the JSON list of a file otherwise"""
    if spec in ("uniform", "cosine") or spec.startswith("sway:"):
        return spec
    if not os.path.isfile(spec):
        raise ValueError(f"--ode_grid {spec!r}: neither uniform, cosine, sway:<s> nor a file")
    with open(spec) as f:
        pts = json.load(f)
    if not isinstance(pts, list):
        raise ValueError(f"--ode_grid {spec!r}: the file must hold one JSON list of grid points")
    return tuple(pts)


def run(dialogue: bool, argv=None) -> int:
    import time
    from scipy.io.wavfile import write
    from . import ops
    import sys
    args = build_parser().parse_args(argv)
    evaluation_times(int(args.nfe), args.ode_method)              # (ValueError before anything loads: unknown method, nfe no multiple of its stages)
    ode_grid = resolve_grid(ode_grid_argument(args.ode_grid), int(args.nfe), args.ode_method) or "uniform"
    if args.ode_error_json and resolve_method(args.ode_method).b_err is None:
        raise ValueError(f"--ode_error_json: --ode_method {args.ode_method} has no embedded error estimate")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:          # spawn our own ranks (hifi-gan/train.py:268-278 does the same)
        rc = dp.launch_ranks(os.path.abspath(sys.argv[0]), list(sys.argv[1:] if argv is None else argv), args.gpus)
        if rc:
            raise SystemExit(rc)
        return 0
    print(args)
    os.makedirs(args.saved_dir, exist_ok=True)
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    random.seed(args.seed)
    rank, world, local = dp.init_from_env()
    if not torch.cuda.is_available():
        from ._lib import CovomixHipError
        raise CovomixHipError("generation needs an MI355X: covomix_amd has no CPU path")
    torch.cuda.set_device(local)
    torch.cuda.manual_seed(args.seed)
    device = torch.device("cuda", local)

    config_file = os.path.join(os.path.split(args.hifigan_ckpt)[0], "vocoder_config.json")   # :368
    with open(config_file) as f:
        h = AttrDict(json.loads(f.read()))
    generator = Generator(h).to(device)
    assert os.path.isfile(args.hifigan_ckpt)
    state_dict_g = torch.load(args.hifigan_ckpt, map_location="cpu", weights_only=False)
    generator.load_state_dict(state_dict_g["generator"])
    generator.eval()
    generator.remove_weight_norm()
    generator.pack()                           # (part of loading the model, not of the first batch)
    model = CoVoMixModel.load_from_checkpoint(args.acous_ckpt, base_dir="", batch_size=16, num_workers=0)
    model.eval()
    model = model.to(device)
    model.nfe, model.ode_method = int(args.nfe), args.ode_method
    model.ode_grid, model.ode_error = ode_grid, bool(args.ode_error_json)
    solve_errors: dict = {}                  # --ode_error_json: utterance -> segment -> tables
    t2s_kw = t2s_sampling_kwargs(args)
    if rank == 0:
        with open(os.path.join(args.saved_dir, "config.txt"), "w") as f:
            f.write("Vocoder: " + str(dict(h)) + "\n")
            f.write("t2s_ckpt: " + str(args.t2s_ckpt) + "\n")
            f.write("acoustic model: " + args.acous_ckpt + "\n")

    t2s = None
    if args.t2s_ckpt:
        assert os.path.isfile(args.t2s_ckpt), f"--t2s_ckpt {args.t2s_ckpt}: no such file (monologue_generation.py:46)"
        t2s = CoVoMixModel.load_from_checkpoint(args.t2s_ckpt, base_dir="", batch_size=16, num_workers=0)   # :93-96
        t2s.eval()
        t2s = t2s.to(device)
    global _HUBERT
    _HUBERT = None
    if args.hubert_ckpt or args.km_path:
        assert args.hubert_ckpt and args.km_path and os.path.isfile(args.hubert_ckpt) and os.path.isfile(args.km_path), \
            "--hubert_ckpt and --km_path must both name existing files"
        from .hubert import HubertTokenizer
        _HUBERT = HubertTokenizer(hubert_path=args.hubert_ckpt, hubert_layer=12, km_path=args.km_path)   # get_fisher_semantic_tokens.py:30-32

    names, sources, plan = utterance_plan(args.text_dir, dialogue, args.mode, t2s is not None, world)
    mine = plan[rank]
    _HUBERT_CODES.clear()
    prepass_s = 0.0                                               # (added to `seconds` below, and reported on its own in last_stats)
    if _HUBERT is not None and args.hubert_batch > 1:
        t_pre = time.perf_counter()
        pretokenise_prompts(args.prompt_dir, prompt_names(mine, dialogue), int(args.hubert_batch))
        prepass_s = time.perf_counter() - t_pre
    _PROMPT_MELS.clear()
    mel_prepass_s = 0.0                                           # (the same for the --mel_batch pre-pass)
    if args.mel_batch > 1:
        t_pre = time.perf_counter()
        preextract_prompt_mels(args.prompt_dir, prompt_names(mine, dialogue), int(args.mel_batch))
        mel_prepass_s = time.perf_counter() - t_pre
    work = [(n, k, s) for n in mine for k, s in enumerate(sources[n])]
    to_decode = sum(1 for _, _, (kind, _) in work if kind != "sem")
    mode = args.pipeline
    if mode == "auto":
        mode = "batch" if (t2s is not None and to_decode > 0) else "off"
    if mode != "off" and t2s is None:
        mode = "off"                                              # nothing to decode: tokens come from files
    two_stage = mode in ("on", "serial")
    from . import pipeline as pl
    # frames per launch: pipelined - two rounds of the N = 1024 products' tiles on the acoustic stage's CUs (the batches form while the
    # text is still being decoded: the lengths are not known up front); otherwise chosen from the directory's lengths below
    max_frames = args.max_frames or (2 * pl.frames_per_launch(device) if two_stage else None)
    segments = {n: {} for n in mine}
    n_out = model._get_field().d["dim_out"]       # acoustic.py:647-650: 80 channels (twocondition_oneoutput) or as wide as cond

    # The reference generates one utterance at a time (monologue_generation.py:259-304); here up to --max_batch utterances
    # of ANY lengths share a launch sequence: packed back to back (no padding), every utterance attending to itself only
    # (sample_ragged), so each gets the result of its own B = 1 run.  Batches are FILLED to --max_frames (first-fit decreasing,
    # dp.pack_by_frames): the frames of a launch decide how many whole rounds of GEMM tiles it runs.
    def one_batch(batch, y0, defer=False):
        """acoustic solve + vocoder of one packed batch of (inputs, (name, segment)) -> parts, generated frames.  parts: one
        (int16 PCM [items, samples] on the HOST, [(name, segment, samples of that item)]) per vocoder call; defer: the PCM travels by
        an asynchronous copy into pinned memory - valid once the stream has got there (_finish)."""
        its = [it for it, _ in batch]
        lens = [int(it[0].shape[0]) for it in its]
        up = lambda t: ops.h2d(t, device)          # (through pinned memory: a pageable copy would make the host wait for the stream)
        if len(set(lens)) == 1:                                                          # equal lengths: the plain [B, T, .] call
            sampled = list(model.synthesis_sample(phoneme_ids=up(torch.stack([it[0] for it in its])),
                                                  cond=up(torch.stack([it[1] for it in its])),
                                                  mask=torch.stack([it[2] for it in its]),
                                                  cond_scale=COND_SCALE, y0=torch.stack(y0)))
        else:
            sampled = model.synthesis_sample(phoneme_ids=[up(it[0]) for it in its], cond=[up(it[1]) for it in its],
                                             mask=[it[2] for it in its], cond_scale=COND_SCALE, y0=y0)
        if model.ode_error:                   # (one column per utterance of the batch, in the batch's order)
            se = model.last_solve_error
            for j, (_, (n, seg)) in enumerate(batch):
                solve_errors.setdefault(n, {})[seg] = dict(grid=list(se.grid), method=str(args.ode_method), order=se.order,
                                                           delta_rms=se.delta_rms[:, j].tolist(), state_rms=se.state_rms[:, j].tolist())
        # vocoder: the generated frames of every utterance of the batch (:299-300: mask is a suffix) go through HiFi-GAN in
        # ONE ragged call (zero-padded to the longest, per-item lengths: every item gets its B = 1 waveform); one int16 cast
        # and one device-to-host copy per batch, sliced per utterance on the host
        n_prompt = [int((~it[2]).sum()) for it in its]
        js = [j for j in range(len(its)) if lens[j] - n_prompt[j] > 0]
        # (items of similar length only: the ragged vocoder call pads to its longest item and skips no work behind a short
        #  one, dp.group_by_padding keeps that padding below 25 % of the real frames)
        tg_all = [lens[j] - n_prompt[j] for j in js]
        parts, nfr = [], 0
        for grp in dp.group_by_padding(tg_all):
            gj = [js[k] for k in grp]
            tgen = [tg_all[k] for k in grp]
            mel = torch.zeros(len(gj), n_out, max(tgen), dtype=torch.float32, device=device)
            for r, j in enumerate(gj):
                mel[r, :, : tgen[r]] = sampled[j][n_prompt[j]:, :].T
            wav = generator(mel, lengths=tgen) if len(set(tgen)) > 1 else generator(mel)
            pcm_dev = ops.wav_to_int16(wav.squeeze(1).contiguous())                        # mel_decode_to_wav (:52-59), batched
            if defer:
                pcm = torch.empty(pcm_dev.shape, dtype=pcm_dev.dtype, pin_memory=True)
                pcm.copy_(pcm_dev, non_blocking=True)
            else:
                pcm = pcm_dev.cpu()
            nfr += sum(tgen)
            parts.append((pcm, [(batch[j][1][0], batch[j][1][1], generator.output_length(tgen[r])) for r, j in enumerate(gj)]))
        return parts, nfr

    def _store(parts):
        for pcm, owners in parts:
            pcm = pcm.numpy()
            for r, (n, seg, ns) in enumerate(owners):
                segments[n][seg] = pcm[r, :ns].copy()

    # The host runs ONE BATCH AHEAD of the device: solve() enqueues a batch - inputs through pinned memory, the solve, the vocoder, the
    # PCM and the saturation flag into pinned memory, an event - and only then waits for the batch BEFORE it.  File-to-tensor work,
    # packing, the per-utterance copies around the vocoder and the Python between the launches (7 % of the device's time on a directory
    # of 16 utterances when every batch ended in a blocking copy) then happen under the previous batch's kernels.
    pending: list = []

    def _finish(entry):
        batch, y0, parts, flag, ev, nfr, st = entry
        ev.synchronize()
        if flag is not None and int(flag[0]) != 0:
            # a flagged batch is repeated with the per-call checks (the stage that saturated warns and re-runs in fp32, or raises
            # under CVX_ON_SATURATION=raise) ON THE STREAM IT WAS ENQUEUED ON: the last batch of a two-stage run is collected after
            # the runner has left its main stream - another stream owns other CUs, picks other GEMM kernels and does not own y0
            with torch.cuda.stream(st):
                parts, nfr = one_batch(batch, y0)
        _store(parts)
        now = time.perf_counter()
        batch_log.append((len(batch), sum(int(it[0].shape[0]) for it, _ in batch), nfr, now - batch_log_t[0]))
        batch_log_t[0] = now

    def solve(batch):
        """one packed batch on the current stream: noise, solve, vocoder, saturation flag -> generated frames (its PCM is collected when
        the NEXT batch has been enqueued, or by drain())"""
        y0 = [torch.randn(int(it[0].shape[0]), n_out, device=device, generator=torch.Generator(device=device).manual_seed(
            _stable_seed(args.seed, own[0], own[1], 2))) for it, own in batch]             # acoustic.py:647-650, per utterance
        with ops.saturation_deferred(read=False):          # one flag read per batch instead of one blocking read per call
            parts, nfr = one_batch(batch, y0, defer=True)
        flag = ops.saturation_snapshot()
        ev = torch.cuda.Event()
        ev.record()
        pending.append((batch, y0, parts, flag, ev, nfr, torch.cuda.current_stream()))
        while len(pending) > 1:
            _finish(pending.pop(0))
        return nfr

    def drain():
        while pending:
            _finish(pending.pop(0))

    def items_of(n, pred):
        return [(it, (n, seg)) for seg, it in enumerate(_build_items(args.mode, dialogue, args.prompt_dir, n,
                                                                     [pred[(n, k)] for k in range(len(sources[n]))]))]

    done, frames = 0, 0
    batch_log_t = [0.0]
    batch_log: list = []                     # (utterances, frames in the launch, generated frames, seconds) per batch -> last_stats
    load_s = 0.0
    if mode == "off":       # ---- text2semantic for this rank's utterances first (not timed, as in round 4), then ONE global packing
        pred = _predict_turns(work, t2s, device, args.seed, sampling=t2s_kw, text_dir=args.text_dir)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    batch_log_t[0] = t0
    if mode == "batch":     # ---- every turn of this rank through the continuously batched decode (timed), then ONE global packing
        pred = _predict_turns(work, t2s, device, args.seed, sampling=t2s_kw, text_dir=args.text_dir)
    head_start = not two_stage and len(mine) >= 2 * HEAD_START
    if head_start:
        # ---- a large directory: the model inputs of the first HEAD_START utterances are read, their fullest first-fit-decreasing bin
        # is ENQUEUED, and the rest of the directory is read while the device works on it (reading is Python + numpy, ~0.7 ms per
        # utterance: 2-3 % of the run when it all happens before the first launch; a reader THREAD was tried first and fought the
        # enqueueing thread for the interpreter lock - 40 utterances in 224-295 ms instead of 40, the first launch enqueued in
        # 200-390 ms instead of 60); then one global packing of everything that is left.  Every batch is a function of the
        # utterance list alone.
        if max_frames is None:
            max_frames = max(256, 32 * ops.stream_cus())          # two rounds of the N = 1024 products' tiles (8192 on 256 CUs)
        head = [x for n in mine[:HEAD_START] for x in items_of(n, pred)]
        load_s = time.perf_counter() - t0
        lengths = [int(it[0].shape[0]) for it, _ in head]
        bins = dp.pack_by_frames(list(range(len(head))), lengths, max_frames, args.max_batch)
        first = max(range(len(bins)), key=lambda b: (sum(lengths[i] for i in bins[b]), -b))
        frames += solve([head[i] for i in bins[first]])
        taken = set(bins[first])
        pool = [x for i, x in enumerate(head) if i not in taken] + [x for n in mine[HEAD_START:] for x in items_of(n, pred)]
        lengths = [int(it[0].shape[0]) for it, _ in pool]
        for b in dp.pack_by_frames(list(range(len(pool))), lengths, max_frames, args.max_batch):
            frames += solve([pool[i] for i in b])
    elif not two_stage:
        pool = [x for n in mine for x in items_of(n, pred)]
        load_s = time.perf_counter() - t0                         # prompt files -> model inputs (host only)
        lengths = [int(it[0].shape[0]) for it, _ in pool]
        if max_frames is None:               # the cap whose packing costs least in rounds of GEMM tiles (dp.choose_max_frames)
            max_frames = dp.choose_max_frames(lengths, args.max_batch, ops.stream_cus())
        for b in dp.pack_by_frames(list(range(len(pool))), lengths, max_frames, args.max_batch):
            frames += solve([pool[i] for i in b])
    else:
        # ---- two-stage pipeline: stage 1 decodes the turns 8 at a time (side stream, worker thread), the collate step assembles
        # the utterances whose turns are all there and packs them; stage 2 = solve() on the main stream.  A bin is launched when it
        # is (nearly) full; the rest waits for more utterances - every batch is a function of the utterance list alone, so
        # `--pipeline serial` runs exactly the same batches (bit-identical PCM).
        groups = [work[i:i + 8] for i in range(0, len(work), 8)]

        def collate(results):
            pred, pool, pending = {}, [], list(mine)
            for part_pred in results:
                pred.update(part_pred)
                while pending and all((pending[0], k) in pred for k in range(len(sources[pending[0]]))):
                    pool.extend(items_of(pending.pop(0), pred))
                last = not pending
                lengths = [int(it[0].shape[0]) for it, _ in pool]
                bins = dp.pack_by_frames(list(range(len(pool))), lengths, max_frames, args.max_batch)
                keep = []
                for b in bins:
                    full = sum(lengths[i] for i in b) >= 0.9 * max_frames or len(b) >= args.max_batch
                    if full or last:
                        yield [pool[i] for i in b]
                    else:
                        keep += b
                pool = [pool[i] for i in sorted(keep)]
        nfr = pl.run_two_stage(groups, lambda g: _predict_turns(g, t2s, device, args.seed, sampling=t2s_kw, text_dir=args.text_dir), solve, device,
                               overlap=(mode == "on"), collate=collate)
        frames = sum(nfr)
    drain()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0 + prepass_s + mel_prepass_s     # (--hubert_batch 1 / --mel_batch 1 work inside the loop: both forms are counted)
    for n in mine:
        if not segments[n]:
            continue
        audio = np.concatenate([segments[n][k] for k in sorted(segments[n])])           # dialogue covosingle: turns in order (:190)
        out = os.path.join(args.saved_dir, n + ".wav")
        write(out, 8000, audio)
        print("Saved wavfile", out)
        done += 1
    if args.ode_error_json:
        with open(args.ode_error_json + (f".rank{rank}" if rank else ""), "w") as f:
            json.dump({n: [segs[k] for k in sorted(segs)] for n, segs in sorted(solve_errors.items())}, f, indent=1)
    print(f"rank {rank}: {done} utterances, {frames} generated frames in {elapsed:.3f} s ({frames / max(elapsed, 1e-9):.1f} frames/s, "
          f"{'text2semantic + ' if mode != 'off' else ''}sampling + vocoder, excluding model load; --pipeline {mode}"
          + (f"; of that {prepass_s:.3f} s in the --hubert_batch pre-pass" if prepass_s else "")
          + (f"; of that {mel_prepass_s:.3f} s in the --mel_batch pre-pass" if mel_prepass_s else "") + ")")
    run.last_stats = dict(utterances=done, frames=frames, seconds=elapsed, pipeline=mode, load_seconds=load_s, batches=batch_log,
                          max_frames=max_frames, head_start=bool(head_start), hubert_prepass_seconds=prepass_s,
                          mel_prepass_seconds=mel_prepass_s)
    return done
