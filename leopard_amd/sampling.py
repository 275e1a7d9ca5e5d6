"""HF-style decoding arguments of the generate() surfaces (compat, idefics2_compat, reference_shim) -> LeopardEngine's SamplingParams.

HF semantics: ``do_sample`` False or absent = greedy (bit-identical to the greedy path); with ``do_sample=True`` an argument left unset
takes the checkpoint's generation_config.json value, else HF's default (temperature 1.0, top_k 50, top_p 1.0); ``temperature <= 0``
with sampling raises ValueError.  The per-call seed comes from torch's default CPU generator (``torch.manual_seed(s)`` makes a run
reproducible) unless ``seed=`` is passed.  ``min_p``, ``typical_p``, ``epsilon_cutoff`` and ``eta_cutoff`` are HF's warpers after top-p, in HF's order (lmi_decode_sample_ex): call
arguments over generation_config.json over "off"; ignored, as ``temperature``, without ``do_sample``.  Options this library does not
implement (``penalty_alpha``, ``num_return_sequences``, ...) produce one warning naming them instead of being ignored silently.  ``repetition_penalty``, ``no_repeat_ngram_size`` and ``min_new_tokens`` are
implemented (LeopardEngine's LogitsRules): call arguments over generation_config.json over "off" (``resolve_rules``)."""
from __future__ import annotations

import json
import os
import warnings
from dataclasses import dataclass
from typing import List, Optional

import torch

from .engine import GenerateOutput, LogitsRules, SamplingParams

HF_DEFAULTS = {"temperature": 1.0, "top_k": 50, "top_p": 1.0}
WARPER_OFF = {"min_p": 0.0, "typical_p": 1.0, "epsilon_cutoff": 0.0, "eta_cutoff": 0.0}     # lmi_decode_sample_ex: implemented; the value = off
SAMPLING_KEYS = ("do_sample", "temperature", "top_k", "top_p") + tuple(WARPER_OFF)
RULE_KEYS = ("repetition_penalty", "no_repeat_ngram_size", "min_new_tokens")       # LogitsRules: implemented (lmi_decode_rules)
BEAM_KEYS = ("num_beams", "length_penalty", "early_stopping")                     # generate_beams: implemented (lmi_beam_step)
BEAM_DEFAULTS = {"num_beams": 1, "length_penalty": 1.0, "early_stopping": False}  # HF's
# generate() options that change the decoding rule and are not implemented, with the value that means "off".  The three RULE_KEYS and the
# four warpers of WARPER_OFF are still listed — warn_unsupported names whatever it is handed — but the generate() surfaces take them as
# named parameters (``resolve_rules``, ``resolve``), so they never reach it from there and no longer warn
UNSUPPORTED = {"num_beams": 1, "num_beam_groups": 1, "penalty_alpha": None, "repetition_penalty": 1.0, "encoder_repetition_penalty": 1.0,
               "length_penalty": 1.0, "no_repeat_ngram_size": 0, "min_p": None, "typical_p": 1.0, "epsilon_cutoff": 0.0,
               "eta_cutoff": 0.0, "num_return_sequences": 1, "diversity_penalty": 0.0, "sequence_bias": None, "guidance_scale": None,
               "low_memory": None, "prompt_lookup_num_tokens": None, "assistant_model": None, "logits_processor": None,
               "min_new_tokens": None, "min_length": None, "renormalize_logits": False, "force_words_ids": None,
               "constraints": None,
               # whole vocabulary rows (or attention maps) per step are not kept: ``logprobs=k`` returns the chosen token's and the top-k
               # log-probabilities instead
               "output_scores": False, "output_logits": False, "output_attentions": False}


def read_generation_defaults(path: str):
    """(sampling and logits-rule keys, beam-search keys) of ``<path>/generation_config.json``, read once: what ``generate*`` and
    ``generate_beams`` take when a call leaves them unset (both empty when the file is absent)."""
    gpath = os.path.join(str(path), "generation_config.json")
    if not os.path.exists(gpath):
        return {}, {}
    with open(gpath) as f:
        g = json.load(f)
    return tuple({k: g[k] for k in keys if g.get(k) is not None} for keys in (SAMPLING_KEYS + RULE_KEYS, BEAM_KEYS))


def read_generation_config(path: str, beams: bool = False) -> dict:
    """The sampling and logits-rule keys of ``<path>/generation_config.json`` (empty when the file or the keys are absent); with ``beams``
    the beam-search keys instead (BEAM_KEYS)."""
    return read_generation_defaults(path)[1 if beams else 0]


def warn_unsupported(where: str, kwargs: dict) -> None:
    bad = sorted(k for k, off in UNSUPPORTED.items() if k in kwargs and kwargs[k] is not None and kwargs[k] != off)
    if bad:
        hint = "; for beam search use generate_beams()" if "num_beams" in bad and where != "generate_beams" else ""
        warnings.warn(f"{where}: {', '.join(bad)} {'is' if len(bad) == 1 else 'are'} not supported by leopard_amd and ignored "
                      f"(decoding is greedy or temperature / top-k / top-p sampling{hint})", UserWarning, stacklevel=3)


def resolve(defaults: Optional[dict] = None, do_sample=None, temperature=None, top_k=None, top_p=None,
            seed: Optional[int] = None, min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None) -> Optional[SamplingParams]:
    """None = greedy; otherwise the SamplingParams of this call (call arguments over ``defaults`` over HF's defaults; the four warpers after
    top-p: over "off").  Values outside their ranges raise ValueError (SamplingParams)."""
    d = defaults or {}
    if not bool(do_sample if do_sample is not None else d.get("do_sample", False)):
        return None
    t = temperature if temperature is not None else d.get("temperature", HF_DEFAULTS["temperature"])
    k = top_k if top_k is not None else d.get("top_k", HF_DEFAULTS["top_k"])
    p = top_p if top_p is not None else d.get("top_p", HF_DEFAULTS["top_p"])
    if not float(t) > 0:
        raise ValueError(f"`temperature` (={t}) has to be a strictly positive float when sampling")
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())        # torch's default CPU generator: torch.manual_seed(s) reproduces the run
    more = {"min_p": min_p, "typical_p": typical_p, "epsilon_cutoff": epsilon_cutoff, "eta_cutoff": eta_cutoff}
    more = {key: v if v is not None else (d[key] if d.get(key) is not None else off) for (key, off), v in zip(WARPER_OFF.items(), more.values())}
    return SamplingParams(float(t), int(k), float(p), int(seed), **more)


def resolve_rules(defaults: Optional[dict] = None, repetition_penalty=None, no_repeat_ngram_size=None,
                  min_new_tokens=None) -> Optional[LogitsRules]:
    """None = no rule; otherwise the LogitsRules of this call (call arguments over ``defaults`` — generation_config.json — over "off")."""
    d = defaults or {}
    pick = lambda v, key, off: v if v is not None else (d.get(key) if d.get(key) is not None else off)
    rules = LogitsRules(float(pick(repetition_penalty, "repetition_penalty", 1.0)), int(pick(no_repeat_ngram_size, "no_repeat_ngram_size", 0)),
                        int(pick(min_new_tokens, "min_new_tokens", 0)))
    return rules if rules.active else None


def resolve_beams(defaults: Optional[dict] = None, num_beams=None, length_penalty=None, early_stopping=None):
    """(num_beams, length_penalty, early_stopping) of a ``generate_beams`` call: call arguments over ``defaults`` (generation_config.json)
    over HF's defaults (1, 1.0, False)."""
    d = defaults or {}
    pick = lambda v, key: v if v is not None else (d[key] if d.get(key) is not None else BEAM_DEFAULTS[key])
    return int(pick(num_beams, "num_beams")), float(pick(length_penalty, "length_penalty")), pick(early_stopping, "early_stopping")


def describe_beams(num_beams: int, length_penalty: float, early_stopping=False) -> str:
    """``beam(4, length_penalty=1.0)``, with ``early_stopping`` appended when it is not HF's default."""
    return f"beam({num_beams}, length_penalty={length_penalty}" + ("" if early_stopping is False else f", early_stopping={early_stopping!r}") + ")"


def beam_outputs(out, num_return_sequences: int, device):
    """An engine ``BeamOutput`` as the surfaces return it: the best sequence [1, n], or the list when ``num_return_sequences`` > 1."""
    seqs = [s.to(device) for s in out.sequences]
    return seqs[0] if int(num_return_sequences) == 1 else seqs


@dataclass
class GenerationLogprobs:
    """What a generate() surface returns for one request with ``logprobs=k``: log-softmax values of the raw logits row each token was
    chosen from — comparable with ``loglikelihood`` / ``forward(labels=)``; under sampling or ``suppress_tokens`` the chosen token need not
    be ``top_token_ids[t, 0]``."""
    sequences: torch.Tensor                      # LongTensor [1, S_in + T]: what the call returns without ``logprobs``
    token_logprobs: torch.Tensor                 # fp32 [T]
    top_token_ids: torch.Tensor                  # int64 [T, k] (value descending, lower id first on ties; -1 = no such entry)
    top_logprobs: torch.Tensor                   # fp32 [T, k]

    @property
    def sequence_logprob(self) -> float:
        """log p(generated tokens | prompt): the float64 sum of ``token_logprobs``."""
        return float(self.token_logprobs.to(torch.float64).sum())


def logprob_outputs(out: GenerateOutput) -> List[GenerationLogprobs]:
    """One GenerationLogprobs per request of an engine call made with ``logprobs=k``."""
    seqs = out.sequences if isinstance(out.sequences, list) else [out.sequences]
    return [GenerationLogprobs(s, lp, ti, tl) for s, lp, ti, tl in zip(seqs, out.token_logprobs, out.top_ids, out.top_logprobs)]


def describe(params: Optional[SamplingParams], rules: Optional[LogitsRules] = None) -> str:
    """``greedy`` / ``sample(...)``, with the active rules appended (``greedy + repetition_penalty=1.2``)."""
    base = "greedy" if params is None else params.describe()
    return base if rules is None or not rules.active else base + " + " + rules.describe()
