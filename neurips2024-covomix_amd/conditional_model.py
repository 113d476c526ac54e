"""`CoVoMixModel` facade - the Python-level drop-in boundary.

Mirrors the inference surface of the reference LightningModule
(covomix/conditional_model.py:38-321) without Lightning / torch_ema / diffusers:

    model = CoVoMixModel.load_from_checkpoint(ckpt, base_dir='', batch_size=16, num_workers=0)
    model.eval()                  # swaps in the EMA shadow weights (conditional_model.py:203-217)
    model = model.to(device)
    mel = model.synthesis_sample(phoneme_ids=..., cond=..., mask=..., cond_scale=0.7)   # :295-302
    tok = t2s_model.synthesis_sample_text2semantic(grapheme_token_ids)                  # :313-321 (text2semantic ckpt)

Checkpoint layout accepted (what Lightning's ModelCheckpoint + on_save_checkpoint write, :150,:200-201):
    ckpt['state_dict']        keys 'cfm_wrapper.CoVoMix.<param>' (acoustic) or 'cfm_wrapper.model.<param>' (text2semantic:
                              TextToSemanticWrapper.model, text2semantic.py:1205-1213; tied / shared tensors appear
                              under several names - token_emb.speech.*, to_logits.*, per-layer rotary_emb.freqs)
    ckpt['hyper_parameters']  dict (may reference classes such as covomix.data_module.SpecsDataModule
                              that do not exist here -> unpickled as inert stubs)
    ckpt['ema']               torch_ema state: {'decay','num_updates','shadow_params': [...], 'collected_params'}
                              with shadow_params in nn.Module.parameters() order
If 'ema' is missing the plain state_dict is used, with a warning (:192-198).
"""
from __future__ import annotations

import os
import pickle
import types
import warnings
from collections import OrderedDict
from typing import Dict, Optional

import torch

from . import ops
from .acoustic import FlowMatchingSampler, VectorField, resolve_grid, resolve_method

_PREFIX = "cfm_wrapper.CoVoMix."
_PREFIX_T2S = "cfm_wrapper.model."


class _StubUnpickler(pickle.Unpickler):
    """Unpickler that turns references to classes/functions of modules that are not installed here
    (pytorch_lightning callbacks, covomix.data_module.SpecsDataModule, ...) into inert placeholders."""

    def find_class(self, module, name):
        try:
            return super().find_class(module, name)
        except Exception:
            return type(name, (), {"__module__": module, "__init__": lambda self, *a, **k: None,
                                   "__setstate__": lambda self, s: None})


_stub_pickle = types.SimpleNamespace(Unpickler=_StubUnpickler, load=lambda f, **kw: _StubUnpickler(f, **kw).load(),
                                     __name__="covomix_amd_stub_pickle")


def _torch_load(path: str):
    return torch.load(path, map_location="cpu", weights_only=False, pickle_module=_stub_pickle)


def parameter_order(sd_keys) -> list:
    """Names in nn.Module.parameters() order for the reference CoVoMix (buffers such as
    rotary_emb.inv_freq are not parameters)."""
    return [k for k in sd_keys if not k.endswith("rotary_emb.inv_freq")]


def t2s_parameter_order(sd_keys) -> list:
    """nn.Module.parameters() order of the reference TextToSemantic: state_dict order minus the aliases of tied /
    shared parameters (to_logits.* and token_emb.speech.* are the embedding tables, text2semantic.py:524-552; one
    RotaryEmbedding per transformer is shared by its layers, :291-299)."""
    return [k for k in sd_keys if not (k.startswith("token_emb.speech.") or k.startswith("to_logits.")
                                       or (k.endswith("rotary_emb.freqs") and ".layers.0.0." not in k))]


class CoVoMixModel:
    def __init__(self, state_dict: Dict[str, torch.Tensor], hparams: Optional[dict] = None,
                 ema_shadow: Optional[list] = None, nfe: int = 32, ode_method="midpoint",
                 precision: Optional[str] = None, ode_grid="uniform", ode_error: bool = False):
        """state_dict: un-prefixed CoVoMix parameter names (acoustic.py:326-406).
        ode_method: the reference's torchdiffeq_ode_method (acoustic.py:560-591) - the name of a built-in tableau (acoustic.TABLEAUS:
        euler, midpoint, heun2, heun3, rk4 = torchdiffeq's 3/8 rule, rk4_classic) or an acoustic.Tableau; nfe counts field evaluations
        and must be a multiple of the method's stages.
        ode_grid: the time grid of the solve (acoustic.time_grid: 'uniform', 'sway:<s>', 'cosine' or nfe / stages + 1 points).
        ode_error: every synthesis_sample also measures the method's embedded error estimate and leaves it in last_solve_error
        (acoustic.SolveError); the result is the same, bit for bit."""
        resolve_method(ode_method)
        resolve_grid(ode_grid, nfe, ode_method)
        self.hparams = dict(hparams or {})
        self.is_text2semantic = "token_emb.text.weight" in state_dict
        if bool(self.hparams.get("text2semantic", self.is_text2semantic)) != self.is_text2semantic:
            raise ValueError("hyper_parameters['text2semantic'] disagrees with the parameter names of the state_dict")
        self._raw = OrderedDict((k, v.detach().cpu()) for k, v in state_dict.items())
        self._ema = None
        if ema_shadow is not None:
            names = (t2s_parameter_order if self.is_text2semantic else parameter_order)(self._raw.keys())
            if len(names) != len(ema_shadow):
                raise ValueError(f"EMA has {len(ema_shadow)} shadow params, model has {len(names)} parameters")
            self._ema = OrderedDict(self._raw)
            for n, t in zip(names, ema_shadow):
                if tuple(t.shape) != tuple(self._raw[n].shape):
                    raise ValueError(f"EMA shadow param shape mismatch at {n}")
                self._ema[n] = t.detach().cpu()
        self._error_loading_ema = ema_shadow is None
        self._use_ema = False
        self.device = torch.device("cpu")
        self.nfe, self.ode_method = nfe, ode_method
        self.ode_grid, self.ode_error = ode_grid, bool(ode_error)
        self.last_solve_error = None
        self.precision = precision or os.environ.get("CVX_PRECISION", "f16x3")
        self._field: Optional[VectorField] = None
        self._field_fp32: Optional[VectorField] = None      # built only if a split-precision call ever saturates
        self._t2s = None

    # ---- construction ---------------------------------------------------------------------
    @classmethod
    def load_from_checkpoint(cls, checkpoint_path, base_dir='', batch_size=16, num_workers=0, **kwargs):
        assert os.path.isfile(checkpoint_path), checkpoint_path      # mirrors monologue_generation.py:46
        ckpt = _torch_load(checkpoint_path)
        sd = OrderedDict((k[len(_PREFIX):], v) for k, v in ckpt["state_dict"].items() if k.startswith(_PREFIX))
        if not sd:                                                   # text2semantic checkpoint (CoSingle / CoMix)
            sd = OrderedDict((k[len(_PREFIX_T2S):], v) for k, v in ckpt["state_dict"].items() if k.startswith(_PREFIX_T2S))
        if not sd:
            raise KeyError(f"no '{_PREFIX}*' or '{_PREFIX_T2S}*' entries in checkpoint state_dict")
        ema = ckpt.get("ema")
        shadow = None
        if ema is not None:
            shadow = ema["shadow_params"]
        else:
            warnings.warn("EMA state_dict not found in checkpoint!")
        hp = ckpt.get("hyper_parameters", {})
        hp = {k: v for k, v in dict(hp).items() if isinstance(v, (int, float, str, bool, type(None)))}
        return cls(sd, hparams=hp, ema_shadow=shadow, **kwargs)

    @classmethod
    def from_state_dict(cls, state_dict, **kwargs):
        return cls(state_dict, **kwargs)

    # ---- nn.Module-like surface -------------------------------------------------------------
    def train(self, mode: bool = True, no_ema: bool = False):
        use = (not mode) and (not no_ema) and (not self._error_loading_ema)
        if use != self._use_ema:
            self._use_ema = use
            self._field = None
            self._field_fp32 = None
            self._t2s = None
        return self

    def eval(self, no_ema: bool = False):
        return self.train(False, no_ema=no_ema)

    def to(self, device):
        device = torch.device(device)
        if device != self.device:
            self.device = device
            self._field = None
            self._field_fp32 = None
            self._t2s = None
        return self

    def active_state_dict(self) -> Dict[str, torch.Tensor]:
        return self._ema if (self._use_ema and self._ema is not None) else self._raw

    def _get_field(self) -> VectorField:
        if self.is_text2semantic:
            raise TypeError("this checkpoint is a text2semantic model: use synthesis_sample_text2semantic")
        if self._field is None:
            if self.device.type != "cuda":
                from ._lib import CovomixHipError
                raise CovomixHipError("CoVoMixModel must be on a GPU (`.to('cuda')`): covomix_amd has no CPU path")
            self._field = VectorField(self.active_state_dict(), self.device, precision=self.precision)
        return self._field

    # ---- sampling -----------------------------------------------------------------------------
    @ops.gated
    @torch.no_grad()
    def synthesis_sample(self, phoneme_ids, cond, mask, cond_scale, y0=None):
        """reference conditional_model.py:295-302 -> ConditionalFlowMatcherWrapper.sample.
        `mask` is accepted and unused, exactly as in the reference (acoustic.py:597-688).
        `y0` (optional) fixes the initial noise; parity is defined given y0.
        Extension: LISTS of per-utterance tensors (phoneme_ids[i] [T_i(, streams)], cond[i] [T_i, C], y0[i] [T_i, dim_out],
        lengths may differ) run as one packed ragged batch and return a list; each result equals that utterance's B = 1
        call up to fp32 summation order (the reference loops over utterances, monologue_generation.py:259-304).
        Extension: cond_scale may be a sequence of one float per utterance (batched or ragged); an utterance at exactly 1.0 takes its
        conditional branch alone, as a scalar call at 1.0 does (acoustic.py:423)."""
        from . import ops
        field = self._get_field()
        ragged = isinstance(cond, (list, tuple))     # extension: utterances of different length in one packed launch

        def run(f):
            sampler = FlowMatchingSampler(f, nfe=self.nfe, method=self.ode_method, grid=self.ode_grid)
            if ragged:
                res = sampler.sample_ragged(phoneme_ids=list(phoneme_ids), cond=list(cond), cond_scale=cond_scale,
                                            y0=None if y0 is None else list(y0), return_error=self.ode_error)
            else:
                res = sampler.sample(phoneme_ids=phoneme_ids, cond=cond, mask=mask, cond_scale=cond_scale, y0=y0, return_error=self.ode_error)
            if self.ode_error:
                res, self.last_solve_error = res
            return res
        # Split-precision activations live in a window of 2^12 around the RMS the gain model predicts (acoustic.py,
        # _activation_scales).  A checkpoint with an outlier row / channel can leave it: the kernels then clamp and raise the
        # device's sticky saturation flag (include/covomix_hip.h).  One flag read per call (the only host synchronisation of
        # the solve); a flagged call is re-run on the exact-fp32 kernels (or raises: CVX_ON_SATURATION=raise) - never
        # returned as is.
        checked = field.precision != "fp32" and ops.saturation_checked() and (not ragged or len(cond) > 0)
        if ragged and y0 is None and checked:       # a re-run must see the same noise
            y0 = [torch.randn(c.shape[0], field.d["dim_out"], device=self.device) for c in cond]
        elif not ragged and y0 is None and checked:
            y0 = torch.randn(cond.shape[0], cond.shape[1], field.d["dim_out"], device=self.device)
        if checked:
            ops.saturation_reset()
        out = run(field)
        if checked and ops.saturation_query():
            out = run(self._saturated(field.precision))
        if ragged:
            return [o.to(c.device) if c.device != o.device else o for o, c in zip(out, cond)]
        return out.to(cond.device) if cond.device != out.device else out

    def _saturated(self, precision: str) -> VectorField:
        """Called when a split-precision solve raised the saturation flag: warn (or raise) and hand back the exact-fp32
        field (built on first use: one more device copy of the weights)."""
        msg = (f"covomix_amd: split-precision ('{precision}') activations left the fp16 window (saturating store): this "
               "checkpoint has outlier weights the gain model does not predict")
        if os.environ.get("CVX_ON_SATURATION", "fp32") == "raise":
            from ._lib import CovomixHipError
            raise CovomixHipError(msg + " (CVX_ON_SATURATION=raise)")
        warnings.warn(msg + "; re-running this call on the exact-fp32 kernels (construct the model with precision='fp32' to avoid the double work)")
        if self._field_fp32 is None:
            self._field_fp32 = VectorField(self.active_state_dict(), self.device, precision="fp32")
        return self._field_fp32

    def _get_t2s(self):
        """The device-resident text2semantic decoder (built on first use)."""
        if not self.is_text2semantic:
            raise TypeError("this checkpoint is an acoustic model: use synthesis_sample")
        if self._t2s is None:
            if self.device.type != "cuda":
                from ._lib import CovomixHipError
                raise CovomixHipError("CoVoMixModel must be on a GPU (`.to('cuda')`): covomix_amd has no CPU path")
            from .t2s import TextToSemanticDecoder
            self._t2s = TextToSemanticDecoder(self.active_state_dict(), self.device)
        return self._t2s

    @ops.gated
    @torch.no_grad()
    def synthesis_sample_text2semantic(self, grapheme_token_ids, temprature=1.0, cond_scale=1.0, beam_search_decode=False,
                                       prompt_mel=None, uniforms=None, generator=None, max_length=None, slots=64,
                                       filter_logits_fn="top_k", filter_fn_kwargs=None, return_logprobs=False, best_of=1,
                                       beam_size=10, length_penalty=1.0, prefix=None, best_of_temperatures=None, mixed_guidance=False,
                                       guided_beam=False, repetition_penalty=1.0, repetition_window=0, no_repeat_ngram_size=0, min_length=0,
                                       beam_rules=False, prefill=False, best_of_select="logprob"):
        """reference conditional_model.py:313-321 -> TextToSemanticWrapper.sample (text2semantic.py:1237-1251): the
        sampled semantic tokens as one flat int64 tensor (two-output models: stream 1 then stream 2) on the input's
        device.  (`temprature` is the reference's spelling.)  `uniforms` / `generator` (optional) fix the U(0,1) draws
        behind the Gumbel noise; parity is defined given them.  A LIST of id tensors (any number) is decoded through `slots`
        continuously refilled decode slots (t2s.generate_many), guided calls (slot pairs) included, and returns a list (the
        reference decodes utterances one by one; the tokens are the same).  filter_logits_fn / filter_fn_kwargs (extension: the
        reference's wrapper does not pass them on): the logit filter of TextToSemantic.generate, "top_k" (thres, k) or "top_p"
        (thres) - t2s.filter_setting; the default is the reference's.
        return_logprobs (extension): returns (tokens, streams [S, L], logprobs float32 [S, L]) per utterance instead of the tokens alone -
        the log-probability the model gave every sampled token (t2s.generate_batch); `t2s.sequence_logprob(logprobs, streams, eos)` is the
        utterance's mean log-probability per token.
        best_of = N > 1 (extension): N candidates per utterance are decoded through the continuously refilled slots (N * n dialogues, or
        record pairs under guidance) and the one with the largest sequence_logprob is returned; the lowest candidate index wins ties.
        Caller-supplied `uniforms` of an utterance are then [N, steps, S, V].  best_of = 1 is the call without it, bit for bit.
        beam_search_decode=True (the flag the reference's generate accepts and never implements, text2semantic.py:673-677): beam search
        with `beam_size` hypotheses (default 10, the reference's; 1..16) - t2s.generate_beam: deterministic, so `temprature` and
        `filter_*` are unused, and `uniforms`, `generator` or best_of > 1 with it are a ValueError; returns the tokens of the hypothesis with
        the largest cumulative log-probability / (tokens scored) ** length_penalty (or the tuple under return_logprobs; lists run in
        lock-step waves of 64 // beam_size utterances).  Beam search under guidance (cond_scale > 1) is opt-in: guided_beam=True (default
        False) runs t2s.generate_beam(cond_scale=...) - every hypothesis a slot pair, waves of 64 // (2 * beam_size) utterances, one-output
        models - and without the switch the combination stays a NotImplementedError; guided_beam=True with cond_scale == 1 is the plain
        beam call.
        Per-utterance settings (extension; t2s.generate_many(settings=...)): with a LIST of texts, `temprature`, `cond_scale`,
        `filter_logits_fn` and `filter_fn_kwargs` may each be a list of the same length - utterance j then decodes with entry j, in the same
        slots and the same captured graph as the others, and gets what it gets alone with those values (lists whose entries are all equal
        take the scalar path).  Guided and unguided utterances do not share a call (ValueError) - unless mixed_guidance=True (default
        False): a list of cond_scale values may then hold 1 (unguided) beside values > 1 (guided), and all of them run through one slot
        pool in one call (t2s.generate_many(mixed_guidance=True)) with the results they get one by one.
        prefix (extension): int64 [S, P] tokens the decode continues from (a list, None where an utterance has none, for a list of texts):
        the result starts with them (t2s.generate_many(prefixes=...)).  prefill=True (default False; without a prefix it changes nothing):
        the prefix positions come from one causal full-sequence pass instead of one decode step per token
        (t2s.generate_many(prefill=True): fp32-class, not bit-identical to the steps; windows of as many utterances as the slots hold;
        a ValueError with mixed_guidance).
        best_of_temperatures (extension): a sequence of N temperatures - best_of = N with candidate c of every utterance decoded at
        temperature c, all in the one generate_many call of best_of; a best_of other than 1 or N is a ValueError.
        repetition_penalty / repetition_window / no_repeat_ngram_size / min_length (extension; t2s.generate_batch, t2s.check_rules): the
        history rules of the decode - a penalty on every id a stream has emitted in its last `repetition_window` tokens (0: all), no
        n-gram twice in a stream, no eos below min_length.  Scalars, or - with a list of texts - lists of the same length (per-utterance
        settings, as above).  All off by default: the call is then what it was.  Log-probs stay those of the model's unmodified rows.
        None of these combines with beam search (ValueError) - unless beam_rules=True (default False): no_repeat_ngram_size and min_length,
        scalars or lists as above, then run under beam search (t2s.generate_beam(beam_rules=True): candidates are removed along every
        hypothesis' own ancestry, scores and log-probs stay the model's); a repetition_penalty other than 1 and a repetition_window other than 0 stay a ValueError.
        best_of_select (extension): the rule best_of keeps a candidate by.  "logprob" (default: the call as it was, no edit-distance call is
        made) - the largest sequence_logprob.  "mbr" - consensus (minimum Bayes risk): the candidate with the smallest total edit distance to
        the utterance's other candidates over the counted tokens of every stream (t2s.consensus_risks: all utterances of the call in one
        ops.edit_distance launch), ties to the larger sequence_logprob, then to the lowest index (t2s.consensus_candidate).  "mbr" without
        best_of > 1 or best_of_temperatures, with beam search, or an unknown name: ValueError."""
        if not self.is_text2semantic:
            raise TypeError("this checkpoint is an acoustic model: use synthesis_sample")
        if best_of_select not in ("logprob", "mbr"):
            raise ValueError(f"best_of_select must be 'logprob' or 'mbr', got {best_of_select!r}")
        if best_of_select == "mbr":
            if beam_search_decode:
                raise ValueError("best_of_select='mbr' does not combine with beam search (consensus is over sampled candidates)")
            if best_of_temperatures is None and not (isinstance(best_of, int) and not isinstance(best_of, bool) and best_of > 1):
                raise ValueError("best_of_select='mbr' needs candidates to choose among: best_of > 1 or best_of_temperatures")
        ids = grapheme_token_ids
        many = isinstance(ids, (list, tuple))
        lists = {k: list(v) for k, v in (("temperature", temprature), ("cond_scale", cond_scale), ("filter_logits_fn", filter_logits_fn),
                                         ("filter_fn_kwargs", filter_fn_kwargs), ("repetition_penalty", repetition_penalty),
                                         ("repetition_window", repetition_window), ("no_repeat_ngram_size", no_repeat_ngram_size),
                                         ("min_length", min_length)) if isinstance(v, (list, tuple))}
        for k, v in lists.items():
            if not many or len(v) != len(ids):
                raise ValueError(f"a list of {k} values goes with a list of texts of the same length ({len(v)} values, "
                                 f"{len(ids) if many else 'one'} text{'s' if many else ''})")
        scales = [float(c) for c in lists.get("cond_scale", [cond_scale])]
        assert all(c >= 1. for c in scales), "cond_scale >= 1 (text2semantic.py:683)"
        # text2semantic.py:684: guidance needs a model trained with condition dropping - the checkpoint's `cond_drop_prob`
        # hyper-parameter (conditional_model.py:52, :78, :114); checkpoints without the key were built with the default 0
        assert not (any(c > 1 for c in scales) and float(self.hparams.get("cond_drop_prob", 0.0)) == 0.0), \
            ("you need to train with conditional drop probability greater than 0 to use classifier free guidance at inference "
             "(text2semantic.py:684): this checkpoint's hyper_parameters['cond_drop_prob'] is 0 or absent")
        if lists.get("temperature") and all(x == lists["temperature"][0] for x in lists["temperature"]):
            temprature = lists.pop("temperature")[0]
        if lists.get("cond_scale") and all(x == lists["cond_scale"][0] for x in lists["cond_scale"]):
            cond_scale = lists.pop("cond_scale")[0]
        if lists.get("filter_logits_fn") and all(x == lists["filter_logits_fn"][0] for x in lists["filter_logits_fn"]):
            filter_logits_fn = lists.pop("filter_logits_fn")[0]
        if lists.get("filter_fn_kwargs") and all(x == lists["filter_fn_kwargs"][0] for x in lists["filter_fn_kwargs"]):
            filter_fn_kwargs = lists.pop("filter_fn_kwargs")[0]
        # the history rules: a list whose entries are all equal is its scalar; a scalar that is off is not passed on (the call as it was)
        rule_kw = dict(repetition_penalty=repetition_penalty, repetition_window=repetition_window, no_repeat_ngram_size=no_repeat_ngram_size,
                       min_length=min_length)
        for k in list(rule_kw):
            if lists.get(k) and all(x == lists[k][0] for x in lists[k]):
                rule_kw[k] = lists.pop(k)[0]
        from .t2s import RULE_FIELDS, RULES_OFF, check_beam_size, check_best_of, check_rules
        rule_kw = {k: v for k, v in rule_kw.items() if k not in lists}
        check_rules(None, 1, 1 << 30, **rule_kw)
        rule_kw = {k: v for k, v in rule_kw.items() if v != RULES_OFF[RULE_FIELDS.index(k)]}
        per = bool(lists) or prefix is not None or best_of_temperatures is not None
        beam_kw = {}
        if beam_search_decode and beam_rules:
            # the two rules of the beam chain leave the per-utterance lists; t2s.check_beam_rules validates them and refuses a penalty
            pens = lists.get("repetition_penalty") or [rule_kw.get("repetition_penalty", 1.0)]    # (a list of equal entries is its scalar)
            if any(float(x) != 1.0 for x in pens):
                raise ValueError("beam search takes no repetition_penalty (it would make the search score something other than the model's "
                                 "log-probability): leave it at 1")
            beam_kw = dict(beam_rules=True, no_repeat_ngram_size=lists.pop("no_repeat_ngram_size", rule_kw.get("no_repeat_ngram_size", 0)),
                           min_length=lists.pop("min_length", rule_kw.get("min_length", 0)))
            if any(int(x) != 0 for x in (lists.get("repetition_window") or [rule_kw.get("repetition_window", 0)])):
                raise ValueError("beam search takes no repetition_window: it is the window of the repetition penalty, which beam search does "
                                 "not run")
            lists.pop("repetition_penalty", None)
            lists.pop("repetition_window", None)       # (lists of 1s and 0s: off)
            rule_kw = {}
            per = bool(lists) or prefix is not None or best_of_temperatures is not None
        if beam_search_decode:
            if rule_kw or any(k in lists for k in RULE_FIELDS):
                raise ValueError("beam search does not run the history rules (repetition_penalty, repetition_window, no_repeat_ngram_size, "
                                 "min_length): leave them off, or sample")
            if per:
                raise ValueError("beam search takes no per-utterance settings, no prefix and no best_of_temperatures")
            if uniforms is not None or generator is not None:
                raise ValueError("beam search is deterministic: it takes no uniforms and no generator")
            if not (isinstance(best_of, int) and not isinstance(best_of, bool) and best_of == 1):
                raise ValueError("beam search already keeps beam_size hypotheses: best_of > 1 does not combine with it")
            check_beam_size(beam_size)
            if cond_scale > 1 and not guided_beam:
                raise NotImplementedError("beam search under guidance (cond_scale > 1) is opt-in: pass guided_beam=True (every hypothesis "
                                          "then takes a slot pair, text context / null context, sharing one ancestry)")
            if cond_scale > 1:
                from .t2s import _dims
                if _dims(self.active_state_dict())["streams"] != 1:          # (from the weights: refused whatever the device)
                    raise NotImplementedError("guidance (cond_scale > 1) on a two-output model: the reference cannot run it")
                res = self._get_t2s().generate_beam(list(ids) if many else ids, beam_size, max_length, float(length_penalty),
                                                    cond_scale=float(cond_scale), **beam_kw)
            else:
                res = self._get_t2s().generate_beam(list(ids) if many else ids, beam_size, max_length, float(length_penalty), **beam_kw)
            pick = (lambda r, i: tuple(t.to(i.device) for t in r[:3])) if return_logprobs else (lambda r, i: r[0].to(i.device))
            return [pick(r, i) for r, i in zip(res, ids)] if many else pick(res, ids)
        if best_of_temperatures is not None:
            temps = [float(t) for t in best_of_temperatures]
            if not temps or (best_of != 1 and best_of != len(temps)):
                raise ValueError(f"best_of_temperatures holds {len(temps)} temperatures: best_of = {best_of!r} disagrees (leave it out)")
            best_of = len(temps)
        best_of = check_best_of(best_of, len(ids) if many else None, uniforms)
        self._get_t2s()
        if per:
            # one generate_many call: dialogue j * N + c is candidate c of utterance j, every dialogue with its own row of settings
            N, ids_l = best_of, list(ids) if many else [ids]
            n = len(ids_l)
            if prefix is None:
                pres = None
            elif many != isinstance(prefix, (list, tuple)) or (many and len(prefix) != n):
                raise ValueError("prefix: one [S, P] tensor for one text, or a list (None: no prefix) as long as the list of texts")
            else:
                pres = [p for p in (list(prefix) if many else [prefix]) for _ in range(N)]
            sets = [{k: v[j] for k, v in lists.items()} for j in range(n)]
            if "filter_logits_fn" in lists and "filter_fn_kwargs" not in lists and filter_fn_kwargs is not None:
                sets = [dict(s_, filter_fn_kwargs=filter_fn_kwargs) for s_ in sets]      # (one kwargs dict for every utterance's filter)
            if best_of_temperatures is not None:
                sets = [dict(s_, temperature=t) for s_ in sets for t in temps]
            else:
                sets = [s_ for s_ in sets for _ in range(N)]
            us = None
            if uniforms is not None:
                us = list(uniforms) if many else [uniforms]
                us = [u[c] for u in us for c in range(N)] if N > 1 else us
            res = self._t2s.generate_many([i for i in ids_l for _ in range(N)], us, max_length,
                                          1.0 if "temperature" in lists else float(temprature), generator, slots=slots,
                                          cond_scale=max(scales) if "cond_scale" in lists else float(cond_scale),
                                          filter_logits_fn="top_k" if "filter_logits_fn" in lists else filter_logits_fn,
                                          filter_fn_kwargs=None if "filter_logits_fn" in lists or "filter_fn_kwargs" in lists else filter_fn_kwargs,
                                          return_logprobs=bool(return_logprobs) or N > 1, settings=sets, prefixes=pres,
                                          **({"mixed_guidance": True} if mixed_guidance else {}), **({"prefill": True} if prefill else {}),
                                          **rule_kw)
            eos = self._t2s.d["vocab"] - 1
            chosen = self._select_candidates(res, N, eos, best_of_select) if N > 1 else [0] * n
            out = []
            for j, i in enumerate(ids_l):
                r = res[j * N + chosen[j]]
                out.append(tuple(t.to(i.device) for t in r) if return_logprobs else r[0].to(i.device))
            return out if many else out[0]
        if best_of > 1:
            # candidate c of utterance j is dialogue j * N + c of one generate_many call: its own draws, the slots shared by all of them
            N, ids_l = best_of, list(ids) if many else [ids]
            us = None
            if uniforms is not None:
                us = [u[c] for u in (list(uniforms) if many else [uniforms]) for c in range(N)]
            res = self._t2s.generate_many([i for i in ids_l for _ in range(N)], us, max_length, float(temprature), generator, slots=slots,
                                          cond_scale=float(cond_scale), filter_logits_fn=filter_logits_fn, filter_fn_kwargs=filter_fn_kwargs,
                                          return_logprobs=True, **rule_kw)
            eos = self._t2s.d["vocab"] - 1
            chosen = self._select_candidates(res, N, eos, best_of_select)
            out = []
            for j, i in enumerate(ids_l):
                r = res[j * N + chosen[j]]
                out.append(tuple(t.to(i.device) for t in r) if return_logprobs else r[0].to(i.device))
            return out if many else out[0]
        if many:                                    # extension: several utterances decoded together (bit-identical tokens)
            ids = list(ids)
            # any number of utterances through 64 continuously refilled decode slots (guidance: 32 slot pairs)
            if return_logprobs:
                res = self._t2s.generate_many(ids, uniforms, max_length, float(temprature), generator, slots=slots, cond_scale=float(cond_scale),
                                              filter_logits_fn=filter_logits_fn, filter_fn_kwargs=filter_fn_kwargs, return_logprobs=True, **rule_kw)
                return [tuple(t.to(i.device) for t in r) for r, i in zip(res, ids)]
            res = self._t2s.generate_many(ids, uniforms, max_length, float(temprature), generator, slots=slots, cond_scale=float(cond_scale),
                                          filter_logits_fn=filter_logits_fn, filter_fn_kwargs=filter_fn_kwargs, **rule_kw)
            return [r[0].to(i.device) for r, i in zip(res, ids)]
        if return_logprobs:
            res = self._t2s.generate(ids, uniforms=uniforms, max_length=max_length, temperature=float(temprature), generator=generator,
                                     cond_scale=float(cond_scale), filter_logits_fn=filter_logits_fn, filter_fn_kwargs=filter_fn_kwargs,
                                     return_logprobs=True, **rule_kw)
            return tuple(t.to(ids.device) for t in res)
        out = self._t2s.generate(ids, uniforms=uniforms, max_length=max_length, temperature=float(temprature), generator=generator,
                                 cond_scale=float(cond_scale), filter_logits_fn=filter_logits_fn, filter_fn_kwargs=filter_fn_kwargs, **rule_kw)
        return out.to(ids.device) if ids.device != out.device else out

    @staticmethod
    def _select_candidates(res, N: int, eos: int, select: str) -> list:
        """Per utterance the index best-of-N keeps among its N candidates res[j * N : (j + 1) * N] ((flat, streams, logprobs) tuples)."""
        from .t2s import best_candidate, consensus_candidate, consensus_risks, sequence_logprob
        groups = [res[j:j + N] for j in range(0, len(res), N)]
        scores = [[sequence_logprob(c[2], c[1], eos) for c in cand] for cand in groups]
        if select == "logprob":
            return [best_candidate(sc) for sc in scores]
        return [consensus_candidate(r, sc) for r, sc in zip(consensus_risks(groups, eos), scores)]

    @ops.gated
    @torch.no_grad()
    def evaluate_text2semantic(self, grapheme_token_ids, gt_tokens, **sampling_kw):
        """reference covomix/util/inference.py:287-358 (evaluate_text2semantic) on texts and ground-truth tokens that are already loaded:
        LISTS of id tensors and of 1-D int64 token tensors -> (0.0, mean token error rate) - the reference's return shape, its accuracy
        being the constant 0.  Every text is decoded through t2s.generate_many (synthesis_sample_text2semantic with a list;
        **sampling_kw are its keywords); a two-output model's prediction is the first half of the flat result (len // 2, as the
        reference cuts it); t2s.token_error_rate runs all pairs in one launch and the mean is taken in fp64 on the host."""
        from .t2s import _dims, token_error_rate
        if not self.is_text2semantic:
            raise TypeError("this checkpoint is an acoustic model")
        if not isinstance(grapheme_token_ids, (list, tuple)) or not isinstance(gt_tokens, (list, tuple)) or \
                len(grapheme_token_ids) != len(gt_tokens) or not grapheme_token_ids:
            raise ValueError("evaluate_text2semantic: a non-empty list of texts and an equally long list of ground-truth token tensors")
        if sampling_kw.get("return_logprobs"):
            raise ValueError("evaluate_text2semantic: return_logprobs is not a sampling setting of the metric")
        preds = self.synthesis_sample_text2semantic(list(grapheme_token_ids), **sampling_kw)
        if _dims(self.active_state_dict())["streams"] == 2:
            preds = [p[:p.shape[0] // 2] for p in preds]
        rates = token_error_rate([p.reshape(-1) for p in preds], [torch.as_tensor(g).reshape(-1) for g in gt_tokens])
        return 0.0, float(torch.tensor(rates, dtype=torch.float64).mean())

    @ops.gated
    @torch.no_grad()
    def evaluate_acoustic(self, phoneme_ids, cond_mels, gt_mels=None, region=("head", 0.7), cond_scale=0.7, y0=None, mcd=False):
        """reference covomix/util/inference.py:32-75 (evaluate_acoustic_predictor_hubert) and :151-227 (..._2input_1output, without
        repeat_prompt) on utterances that are already loaded: LISTS of token tensors [T_i(, streams)], of conditioning mels [T_i, C] and
        (optional; default = cond_mels) of ground-truth mels [T_i, dim_out], of any lengths -> (0.0, mean MSE) - the reference's return
        shape, its accuracy being the constant 0.  The split index of an utterance is int(T_i * fraction), as the reference computes it.
        region = ("head", f): the first part is generated and the rest stays as the prompt (:55-68, f = 0.7); ("tail", f): the rest
        is generated and the first part stays (:191-220, f = 0.5, gt_mels = the mix mel).  The conditioning is the mel with the
        generated part zeroed; ONE ragged synthesis_sample call runs all utterances (y0, a list, is passed through); the MSE of an
        utterance is F.mse_loss over its generated part, the mean over utterances is taken in fp64 on the host.  mcd=True: a third
        value, the per-utterance mel-cepstral distortion of the generated part without alignment (float64 [n] in dB,
        metrics.mel_cepstral_distortion(align="none"): this project's definition, see metrics.py)."""
        from .metrics import mel_cepstral_distortion, mel_mse
        if self.is_text2semantic:
            raise TypeError("this checkpoint is a text2semantic model")
        lists = [phoneme_ids, cond_mels] + ([gt_mels] if gt_mels is not None else []) + ([y0] if y0 is not None else [])
        if not all(isinstance(x, (list, tuple)) for x in lists) or len(set(len(x) for x in lists)) != 1 or not phoneme_ids:
            raise ValueError("evaluate_acoustic: non-empty, equally long lists of token tensors, conditioning mels (and ground-truth mels, y0)")
        if not (isinstance(region, (list, tuple)) and len(region) == 2 and region[0] in ("head", "tail") and 0.0 <= float(region[1]) <= 1.0):
            raise ValueError(f"evaluate_acoustic: region = {region!r} (('head' | 'tail', a fraction in [0, 1]))")
        head, frac = region[0] == "head", float(region[1])
        gts = list(cond_mels) if gt_mels is None else list(gt_mels)
        conds, parts = [], []
        for i, (ids, c, g) in enumerate(zip(phoneme_ids, cond_mels, gts)):
            if c.shape[0] != ids.shape[0] or g.shape[0] != ids.shape[0]:
                raise ValueError(f"evaluate_acoustic: utterance {i} has {ids.shape[0]} tokens, {c.shape[0]} and {g.shape[0]} mel frames")
            k = int(len(ids) * frac)
            parts.append(slice(0, k) if head else slice(k, ids.shape[0]))
            c = c.clone()
            c[parts[-1]] = 0
            conds.append(c.to(self.device))
        preds = self.synthesis_sample([p.to(self.device) for p in phoneme_ids], conds, None, cond_scale, y0=y0)
        gen = [p[s] for p, s in zip(preds, parts)]
        want = [g[s].to(p.device) for g, p, s in zip(gts, preds, parts)]
        for i, (a, b) in enumerate(zip(gen, want)):
            if a.shape != b.shape:
                raise ValueError(f"evaluate_acoustic: utterance {i} generates {tuple(a.shape)} against a ground truth of {tuple(b.shape)}")
        mse = float(torch.stack([m.double().cpu() for m in mel_mse(gen, want)]).mean())
        if not mcd:
            return 0.0, mse
        return 0.0, mse, mel_cepstral_distortion([a.contiguous() for a in gen], [b.contiguous() for b in want], align="none")[0]

    def _acoustic_dims(self) -> dict:
        from .acoustic import _dims_from_state
        if self.is_text2semantic:
            raise TypeError("this checkpoint is a text2semantic model")
        return _dims_from_state(self.active_state_dict())

    def _run_unsaturated(self, run):
        """run(field) under the saturation contract of synthesis_sample: one flag read per call; a flagged call on a split-precision field is
        repeated on the exact-fp32 field (or raises: CVX_ON_SATURATION=raise) - run must be repeatable with the same draws."""
        field = self._get_field()
        checked = field.precision != "fp32" and ops.saturation_checked()
        if checked:
            ops.saturation_reset()
        out = run(field)
        if checked and ops.saturation_query():
            out = run(self._saturated(field.precision))
        return out

    @ops.gated
    @torch.no_grad()
    def flow_matching_loss(self, phoneme_ids, mels, cond_mels=None, masks=None, times=None, x0=None, cond_drop=None, sigma=0.0, seed=None,
                           max_rows=8192, return_pred=False):
        """The conditional-flow-matching loss of held-out mels: the reference's `valid_loss` (conditional_model.py:229-271 ->
        ConditionalFlowMatcherWrapper.forward, acoustic.py:732-791, on CoVoMix.forward(..., target = flow), :430-538) - ONE network
        evaluation per utterance, at a time of its own.  LISTS of per-utterance tensors of any lengths: phoneme_ids[i] [T_i(, streams)],
        mels[i] [T_i, dim_out] (x1), cond_mels[i] [T_i, dim_cond] (default: mels, as VoSingle trains), masks[i] bool [T_i] (True: the frame
        is hidden from the conditioning and counted by the loss), times [n] in [0, 1], x0[i] [T_i, dim_out] (the noise), cond_drop [n] bools
        (True: the utterance runs on the null phoneme id and null_cond, acoustic.py:473-494; default none - the reference's default
        cond_drop_prob is 0), sigma (the wrapper's, default 0).  -> flow_loss.FlowLoss.
        PER-UTTERANCE semantics: every utterance gets the reference's result at B = 1 (acoustic.py:527-538: the masked mean over its own
        frames) and `loss` is the mean of those in fp64 - the reference pads a batch to its longest item without a padding mask, which
        this project reproduces nowhere.  The caller's order is cut into packed launches of at most max_rows rows; per launch
        ops.cfm_inputs, one VectorField.evaluate_seq_times and ops.masked_mse.
        What is not passed is drawn from a CPU torch.Generator seeded with `seed`, utterance by utterance: time ~ U[0, 1), x0 ~ N(0, 1),
        the mask of acoustic.py:460-465 (flow_loss.draw documents the order) - the reference's distributions, not its device RNG stream.
        A mask without a True frame is no error: that utterance's loss is 0 through the clamp, as in the reference.
        Saturation: as synthesis_sample - a flagged call on a split-precision field is repeated on the fp32 field with the same draws.
        ValueError: unequal list lengths, an empty list, token / mel / mask / x0 shapes that disagree, a time outside [0, 1];
        TypeError: a text2semantic checkpoint."""
        from . import flow_loss as fl
        d = self._acoustic_dims()
        chk = fl.check_inputs(d, phoneme_ids, mels, cond_mels, masks, times, x0, cond_drop, sigma)
        n, lengths, drop = chk["n"], chk["lengths"], chk["drop"]
        launches = fl.cut_launches(lengths, max_rows, ops.SEQ_NORM_MAX_SEQS)
        drawn = fl.draw(lengths, d["dim_out"], seed, need_times=times is None, need_x0=x0 is None, need_masks=masks is None)
        tv = chk["times"] if times is not None else torch.tensor(drawn["times"], dtype=torch.float32)
        x0 = list(x0) if x0 is not None else drawn["x0"]
        masks = [m.cpu() for m in masks] if masks is not None else drawn["masks"]
        f32 = lambda ts: torch.cat([t.detach().to(dtype=torch.float32).cpu().reshape(t.shape[0], -1) for t in ts]).contiguous()

        def run(field):
            dev = field.device
            res = []
            for rng in launches:
                lens = [lengths[i] for i in rng]
                ids = torch.cat([torch.full_like(phoneme_ids[i].cpu(), d["null_id"]) if drop[i] else phoneme_ids[i].cpu() for i in rng])
                x1_d, x0_d, c_d = (ops.h2d(f32([src[i] for i in rng]), dev) for src in (mels, x0, chk["conds"]))
                m_d = ops.h2d(torch.cat([masks[i] for i in rng]).to(torch.uint8), dev)
                t_d = ops.h2d(tv[rng.start:rng.stop].contiguous(), dev)
                rg = ops.Ragged(lens, dev)
                _, flow, cond_in = ops.cfm_inputs(x1_d, x0_d, c_d, m_d, t_d, rg, float(sigma), field.xin_rows(lens))
                for k, i in enumerate(rng):              # the null conditioning replaces the (already masked) one, acoustic.py:476
                    if drop[i]:
                        cond_in[rg.cu_host[k]:rg.cu_host[k + 1]] = field.sd["null_cond"]
                pred = field.evaluate_seq_times(ops.h2d(ids.to(torch.int64), dev), cond_in, field.xin_rows(lens), t_d, lens)
                loss, count, err = ops.masked_mse(pred, flow, m_d, rg)
                res.append((loss.cpu(), count.cpu(), err.cpu(), pred.cpu() if return_pred else None, lens))
            return res
        res = self._run_unsaturated(run)
        per = torch.cat([r[0] for r in res]).double()
        err_rows, preds = [], []
        for _, _, err, pred, lens in res:
            err_rows += list(torch.split(err, lens))
            if return_pred:
                preds += list(torch.split(pred, lens))
        return fl.FlowLoss(loss=float(per.mean()), per_utterance=per, frames=torch.cat([r[1] for r in res]).to(torch.int64), times=tv,
                           masks=masks, err_rows=err_rows, pred=preds if return_pred else None)

    @ops.gated
    @torch.no_grad()
    def synthesis_regression_duration(self, phoneme_ids, cond, mask, cond_scale, y0=None, times=None):
        """The reference's one-shot regression sample (conditional_model.py synthesis_regression_duration ->
        ConditionalFlowMatcherWrapper.sample_regression, acoustic.py:690-727): ONE guided evaluation f_c (1 + s) - s f_null of the network
        on noise at a random time per utterance.  A batch (phoneme_ids [B, T(, streams)], cond [B, T, C]; -> [B, T, dim_out]) or LISTS of
        per-utterance tensors of any lengths (-> a list); `mask` is accepted and unused, as in the reference.  y0 (the noise, default
        randn) and times ([B] in [0, 1], default U[0, 1)) fix the draws; parity is defined given them.  One call holds at most
        ops.SEQ_NORM_MAX_SEQS utterances, half as many under guidance (ValueError).  cond_scale == 1 runs the
        conditional branch alone (acoustic.py:423).  One VectorField.evaluate_seq_times call on the packed batch, the branches combined
        by the solve's combine kernel."""
        d = self._acoustic_dims()
        many = isinstance(cond, (list, tuple))
        conds = list(cond) if many else list(cond.unbind(0))
        idsl = list(phoneme_ids) if many else list(phoneme_ids.unbind(0))
        n = len(conds)
        if n == 0 or len(idsl) != n:
            raise ValueError("synthesis_regression_duration: a non-empty batch of tokens and conditioning mels of the same size")
        lengths = [int(c.shape[0]) for c in conds]
        for i in range(n):
            if conds[i].dim() != 2 or conds[i].shape[1] != d["dim_cond"] or lengths[i] < 1:
                raise ValueError(f"synthesis_regression_duration: cond[{i}] must be [T >= 1, {d['dim_cond']}], got {tuple(conds[i].shape)}")
            expect = (lengths[i],) + ((d["streams"],) if d["streams"] > 1 else ())
            if tuple(idsl[i].shape) != expect:
                raise ValueError(f"synthesis_regression_duration: phoneme_ids[{i}] must be {expect}, got {tuple(idsl[i].shape)}")
        if y0 is None:
            y0l = [torch.randn(T, d["dim_out"]) for T in lengths]
        else:
            y0l = list(y0) if many else list(y0.unbind(0))
            if len(y0l) != n or any(tuple(y.shape) != (T, d["dim_out"]) for y, T in zip(y0l, lengths)):
                raise ValueError(f"synthesis_regression_duration: y0 must hold one [T, {d['dim_out']}] per utterance")
        tv = torch.rand(n) if times is None else torch.tensor([float(t) for t in times], dtype=torch.float64).to(torch.float32)
        if tv.numel() != n or not bool(((tv >= 0) & (tv <= 1)).all()):
            raise ValueError("synthesis_regression_duration: one time in [0, 1] per utterance")
        s = float(cond_scale)
        use_null = s != 1.0
        if n * (2 if use_null else 1) > ops.SEQ_NORM_MAX_SEQS:      # (the null branch doubles the sequences of the one evaluation)
            raise ValueError(f"synthesis_regression_duration: {n} utterances in one call, at most {ops.SEQ_NORM_MAX_SEQS // (2 if use_null else 1)}"
                             f"{' under guidance (cond_scale != 1)' if use_null else ''}")

        def run(field):
            dev = field.device
            ids_p = torch.cat([p.to(device=dev, dtype=torch.int64) for p in idsl]).contiguous()
            cond_p = torch.cat([c.to(device=dev, dtype=torch.float32) for c in conds]).contiguous()
            y = torch.cat([t.to(device=dev, dtype=torch.float32) for t in y0l]).contiguous()
            pred = field.evaluate_seq_times(ids_p, cond_p, y, ops.h2d(tv, dev), lengths, use_null=use_null)
            M1 = y.shape[0]
            if not use_null:
                return pred[:M1].clone()
            out = torch.empty_like(y)
            ops.cfg_combine_axpy(pred[:M1], pred[M1:], torch.zeros_like(y), s, 1.0, out)      # 0 + 1 * (f_c (1 + s) - s f_null)
            return out
        out = self._run_unsaturated(run)
        ref = conds[0]
        outs = [o.to(ref.device) if ref.device != o.device else o for o in torch.split(out, lengths)]
        return outs if many else torch.stack(outs)

    @ops.gated
    @torch.no_grad()
    def score_text2semantic(self, grapheme_token_ids, streams, cond_scale=1.0, mixed_guidance=False, prefill=False):
        """Teacher-forced scoring (extension; what the reference's evaluate_text2semantic measures through
        TextToSemantic.forward(..., return_loss=True)): the log-probability of every token of `streams` - int64 [S, L], the streams a
        sampling call returned - under the text: float32 [S, L] (t2s.score_many).  One utterance, or LISTS of texts and streams (-> a
        list).  cond_scale > 1 scores under the guidance-combined logits and needs what sampling with it needs.  mixed_guidance=True with
        lists: cond_scale may be a list as long as the texts, 1 (unguided) beside values > 1 (guided), scored in one call.
        prefill=True (default False): the log-probs come from causal full-sequence passes over the streams instead of one decode step per
        token (t2s.score_many(prefill=True)): much faster for few utterances, fp32-class, not bit-identical to the default."""
        if not self.is_text2semantic:
            raise TypeError("this checkpoint is an acoustic model")
        scales = [float(c) for c in cond_scale] if isinstance(cond_scale, (list, tuple)) else [float(cond_scale)]
        if isinstance(cond_scale, (list, tuple)) and not mixed_guidance:
            raise ValueError("score_text2semantic: a list of cond_scale values needs mixed_guidance=True")
        assert all(c >= 1. for c in scales), "cond_scale >= 1 (text2semantic.py:683)"
        assert not (any(c > 1 for c in scales) and float(self.hparams.get("cond_drop_prob", 0.0)) == 0.0), \
            ("you need to train with conditional drop probability greater than 0 to use classifier free guidance at inference "
             "(text2semantic.py:684): this checkpoint's hyper_parameters['cond_drop_prob'] is 0 or absent")
        many = isinstance(grapheme_token_ids, (list, tuple))
        if many != isinstance(streams, (list, tuple)):
            raise ValueError("score_text2semantic: one utterance and its streams, or a list of each")
        dec = self._get_t2s()
        if mixed_guidance:
            if isinstance(cond_scale, (list, tuple)) and (not many or len(scales) != len(grapheme_token_ids)):
                raise ValueError("score_text2semantic: a list of cond_scale values goes with a list of texts of the same length")
            res = dec.score_many(list(grapheme_token_ids) if many else [grapheme_token_ids], list(streams) if many else [streams],
                                 cond_scale=scales if isinstance(cond_scale, (list, tuple)) else scales[0], mixed_guidance=True,
                                 **({"prefill": True} if prefill else {}))
            return res if many else res[0]
        res = dec.score_many(list(grapheme_token_ids) if many else [grapheme_token_ids], list(streams) if many else [streams],
                             cond_scale=float(cond_scale), **({"prefill": True} if prefill else {}))
        return res if many else res[0]
