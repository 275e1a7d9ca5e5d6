"""The model object the reference's evaluation script drives (evaluations/models/llava_multiimg_siglip_anyres.py,
"EVAL"), backed by the HIP engine.

EVAL:373-375   llava = myLlavaForConditionalGeneration.from_pretrained(ckpt, torch_dtype=torch.float32); .eval(); .to('cuda:0')
EVAL:405,445   images.to(llava.device), input_ids.to(llava.device)
EVAL:448-452   llava.generate(input_ids, pixel_values=, attention_mask=, pad_token_id=, eos_token_id=[128001,128009],
                              max_new_tokens=128, use_cache=True) -> LongTensor [1, S_in + T]
EVAL:201-361   forward(input_ids=, pixel_values=, attention_mask=, ..., return_dict=) -> .logits [1,S,V], .past_key_values

``LeopardForConditionalGeneration`` honours exactly that surface (same argument names, same return shapes/devices,
ValueError on an image-token / feature-count mismatch as transformers 4.38's merge raises).  ``torch_dtype`` is the
dtype the caller's tensors use (fp32 in EVAL); the MFMA compute type is ``compute_dtype`` (fp16 by default: closest to
the reference's fp32 results at the full matrix-core rate).  Batch is 1 per call, like the reference.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import os

import torch

from .checkpoint import CheckpointSource, load_config
from .config import LeopardConfig
from .engine import DecodeBatchLimitOption, KVCache, LeopardEngine
from .ops import Ops
from .weights import EngineWeights
from . import sampling


@dataclass
class LlavaCausalLMOutputWithPast:
    """Field-compatible with transformers.models.llava.modeling_llava.LlavaCausalLMOutputWithPast (EVAL:355-361)."""
    loss: Optional[torch.Tensor] = None
    logits: Optional[torch.Tensor] = None
    past_key_values: Optional[object] = None
    hidden_states: Optional[Tuple] = None
    attentions: Optional[Tuple] = None

    def __getitem__(self, i):
        return [v for v in (self.loss, self.logits, self.past_key_values, self.hidden_states, self.attentions)
                if v is not None][i]


def resolve_precision(requested_dtype, compute_dtype, precision: Optional[str] = None, tp_size: int = 1) -> str:
    """Schedule of the prefill (LeopardEngine.precision).  ``LEOPARD_AMD_PRECISION`` = fast | lo4 | split overrides everything; an explicit
    ``precision`` argument comes next; otherwise a caller that asks for ``torch_dtype=torch.float32`` — the reference script does, EVAL:373 —
    gets the mode that meets the stated tolerance against fp32 arithmetic (lo4: fp16 operands + the fp4 correction phase, full-depth logits
    within 1e-3), and a caller that asks for a 16-bit type gets the fast schedule of that type.  Tensor-parallel engines run fast or lo4."""
    env = os.environ.get("LEOPARD_AMD_PRECISION", "").lower()
    mode = env or precision or ("lo4" if requested_dtype in (None, torch.float32) and compute_dtype == torch.float16 else "fast")
    if mode not in ("fast", "lo4", "split"):
        raise ValueError(f"precision must be fast, lo4 or split, not {mode!r}")
    return "fast" if (tp_size > 1 and mode == "split") else mode


class LeopardForConditionalGeneration(DecodeBatchLimitOption):
    def __init__(self, config: LeopardConfig, source_factory, compute_dtype=torch.float16, ops: Optional[Ops] = None,
                 torch_dtype=torch.float32, precision: Optional[str] = None, tp_rank: int = 0, tp_size: int = 1):
        self.config = config
        self._source_factory = source_factory            # (device, dtype) -> parameter source with .get(name)
        self.compute_dtype = compute_dtype
        self.requested_dtype = torch_dtype
        self.precision = resolve_precision(torch_dtype, compute_dtype, precision, tp_size)
        self.tp_rank, self.tp_size = int(tp_rank), int(tp_size)
        self._ops = ops
        self._engine: Optional[LeopardEngine] = None
        self.device = torch.device("cpu")
        self.generation_defaults: dict = {}              # do_sample / temperature / top_k / top_p / the logits rules of the checkpoint's generation_config.json
        self.last_decoding = "greedy"                    # the decoding rule of the last generate* call (leopard_amd.sampling.describe)
        self.beam_defaults: dict = {}                    # num_beams / length_penalty / early_stopping of generation_config.json (generate_beams)

    # ---- loading ---------------------------------------------------------------------------------------------
    @classmethod
    def from_pretrained(cls, path: str, torch_dtype=torch.float32, compute_dtype=torch.float16, ops: Optional[Ops] = None,
                        precision: Optional[str] = None, tp_rank: int = 0, tp_size: int = 1, decode_batch_limit: Optional[int] = None,
                        decode_pair_limit: Optional[int] = None):
        """``precision``: see resolve_precision.  ``decode_pair_limit`` (also a settable attribute): the most sequences a precision mode decodes on
        the pair step (LeopardEngine.decode_pair_limit; 8 .. 32, default 8).  ``decode_batch_limit`` (also a settable attribute): the most sequences generate_stream /
        generate_batch decode in one step (LeopardEngine.decode_batch_limit; default 16).  ``tp_size`` > 1 (SURVEY.md 8 f1 "optional TP pre-sharding on load"): this process holds
        tensor-parallel shard ``tp_rank`` of the LLM — the checkpoint's tensors are sliced while they stream to the device
        (EngineWeights.build) — and needs an initialised process group of that size (leopard_amd.dist.init) by the time ``.to(device)`` runs."""
        cfg = load_config(path)
        m = cls(cfg, lambda dev, dt: CheckpointSource(path, dev, dt), compute_dtype, ops, torch_dtype=torch_dtype, precision=precision,
                tp_rank=tp_rank, tp_size=tp_size)
        m.generation_defaults, m.beam_defaults = sampling.read_generation_defaults(path)
        if decode_batch_limit is not None:
            m.decode_batch_limit = decode_batch_limit
        if decode_pair_limit is not None:
            m.decode_pair_limit = decode_pair_limit
        return m

    def eval(self):
        return self

    def to(self, device):
        device = torch.device(device)
        if self._engine is None or device != self.device:
            ops = self._ops if self._ops is not None else Ops()
            source = self._source_factory(device, self.compute_dtype)
            W = EngineWeights.build(self.config, source, self.compute_dtype, tp_rank=self.tp_rank, tp_size=self.tp_size)
            stats = getattr(source, "cast_stats", None)              # checkpoint.CheckpointSource: what the cast to the compute type cost
            self.weight_cast_stats = dict(stats) if stats else None
            if stats and stats["inexact_elements"] > 0.05 * max(stats["elements"], 1):     # (a bf16-trained checkpoint: only its few values below 2^-17)
                import warnings
                warnings.warn("leopard_amd: " + source.cast_report(), UserWarning, stacklevel=2)
            self._engine = LeopardEngine(self.config, W, ops=ops, device=device)
            if self.precision == "lo4" and not self._engine.lo4_supported():
                # a model shape the lo4 schedule does not cover: the 2 K mode meets the same figure on one rank; tensor-parallel engines only
                # run fast / lo4 (resolve_precision's rule for an explicit "split" request)
                self.precision = "split" if self.tp_size == 1 else "fast"
            self._engine.precision = self.precision
            self._apply_decode_batch_limit()
            self.device = device
        return self

    @property
    def engine(self) -> LeopardEngine:
        if self._engine is None:
            raise RuntimeError("call .to(device) first (the HIP engine is built on the target device)")
        return self._engine

    def _as_tiles(self, pixel_values):
        """``pixel_values``: the reference's normalised fp32 [N,3,S,S], or the GPU tiler's u8 [N,S,S,3] tile stack (the
        normalisation then happens in lmi_preprocess_tiles)."""
        if pixel_values is None:
            return None
        if pixel_values.dtype == torch.uint8:
            return pixel_values.to(self.device).contiguous()
        return pixel_values.to(device=self.device, dtype=torch.float32).contiguous()

    # ---- EVAL:201-361 ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, input_ids=None, pixel_values=None, attention_mask=None, position_ids=None, past_key_values=None,
                inputs_embeds=None, vision_feature_layer=None, vision_feature_select_strategy=None, labels=None,
                use_cache=None, output_attentions=None, output_hidden_states=None, return_dict=None):
        if inputs_embeds is not None or output_attentions or output_hidden_states:
            raise NotImplementedError("input_ids (+ pixel_values, labels) only: no inputs_embeds / attentions / hidden states")
        if input_ids.shape[0] != 1:
            raise NotImplementedError("batch 1 per call, as in the reference harness (EVAL:381-452)")
        if attention_mask is not None and not bool(attention_mask.to(torch.bool).all()):
            raise NotImplementedError("padded prompts are not produced by the reference harness (batch 1)")
        eng = self.engine
        if past_key_values is not None and input_ids.shape[1] == 1:          # decode branch, EVAL:291-320
            logits = eng.decode_step(int(input_ids[0, 0]), past_key_values)
            return LlavaCausalLMOutputWithPast(logits=logits.view(1, 1, -1), past_key_values=past_key_values)
        if past_key_values is not None and input_ids.shape[1] > 1 and labels is None:
            # multi-turn (HF semantics: append n rows to the cache): the n new ids run against the cached rows (LeopardEngine.append);
            # pixel_values are ignored here as in the decode branch — images belong to the call that built the cache
            logits = eng.append(past_key_values, input_ids.to(self.device))
            return LlavaCausalLMOutputWithPast(logits=logits.unsqueeze(0), past_key_values=past_key_values)
        if labels is not None:
            if past_key_values is not None:
                raise NotImplementedError("labels score a whole prompt: no past_key_values")
            rows, targets, _ = eng.score_targets(input_ids, labels)          # ValueError on bad labels, before any launch
        tiles = self._as_tiles(pixel_values)
        cache = KVCache(self.config, eng.merged_len(input_ids) + 256, self.compute_dtype, self.device) if use_cache else None
        res = eng.prefill(input_ids.to(self.device), tiles, cache=cache, all_logits=True)
        loss = None
        if labels is not None:
            # EVAL:333-348: the mean cross-entropy of the shifted labels over their non-ignored targets (nan when there are none), from the
            # logits just computed (lmi_token_logprobs on the scored rows: no second head pass)
            lp, _ = eng.logits_logprobs(res.logits_all, rows, targets)
            loss = (-lp.to(torch.float64).mean()).to(torch.float32) if len(rows) else torch.full((), float("nan"), device=self.device)
        return LlavaCausalLMOutputWithPast(loss=loss, logits=res.logits_all.unsqueeze(0), past_key_values=cache)

    __call__ = forward

    @torch.no_grad()
    def loglikelihood(self, requests: Sequence[Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]], batch_size: int = 8,
                      share_prefix: bool = False) -> List[Tuple[float, bool]]:
        """The ``loglikelihood`` contract of VLM evaluation harnesses: [(context_ids [1, S_c], continuation_ids [1, S_t], pixel_values)] ->
        [(sum of log p(continuation | images + context), is_greedy)].  The continuation is appended to the context, the context labelled -100,
        and the requests are scored ``batch_size`` at a time in one packed prefill each (LeopardEngine.score_batch); is_greedy = every
        continuation token is its row's argmax.
        ``share_prefix`` (default False: the path and the bits above): consecutive requests whose ``pixel_values`` are THE SAME OBJECT form a
        group; the longest common prefix of the group's context ids — cut so that every request keeps at least one context id as its tail —
        is prefilled once and the group goes through ``loglikelihood_shared``.  A group of one request, or one whose tails would hold an
        image token, is scored as without the flag.  The results come back in request order."""
        if not share_prefix:
            return score_loglikelihood(self.engine, [(c, t, self._as_tiles(p)) for c, t, p in requests], batch_size, self.device)
        out: List[Tuple[float, bool]] = []
        i = 0
        while i < len(requests):
            j = i + 1
            while j < len(requests) and requests[j][2] is requests[i][2] and requests[i][2] is not None:
                j += 1
            group = requests[i:j]
            split = shared_context_split([g[0] for g in group], self.config.image_token_index) if len(group) > 1 else None
            if split is None:
                out += score_loglikelihood(self.engine, [(c, t, self._as_tiles(p)) for c, t, p in group], batch_size, self.device)
            else:
                head, tails = split
                out += self.loglikelihood_shared(head, group[0][2], [(t, g[1]) for t, g in zip(tails, group)])
            i = j
        return out

    @torch.no_grad()
    def loglikelihood_shared(self, prefix_ids, pixel_values, requests: Sequence[Tuple[torch.Tensor, torch.Tensor]],
                             attention: Optional[str] = None) -> List[Tuple[float, bool]]:
        """Rank N continuations over one set of images: ``prefix_ids`` [1, S_p] with ``pixel_values`` is prefilled ONCE (the vision tower runs
        once), then [(tail_ids [1, t_j >= 0], continuation_ids [1, m_j >= 1])] are scored from its cache together
        (LeopardEngine.score_shared) -> [(sum of log p(continuation | images + prefix + tail), is_greedy)], what ``loglikelihood`` gives for
        the concatenated prompts within the tolerances of ``extend``.  ``attention``: "ranges" / "rows" (LeopardEngine.extend); None = the
        engine's default."""
        as_ids = lambda t: torch.as_tensor(t).reshape(1, -1).to(torch.int64)
        res = self.engine.score_shared(as_ids(prefix_ids).to(self.device), self._as_tiles(pixel_values), [(as_ids(t), as_ids(c)) for t, c in requests],
                                       attention=attention)
        # one read-back for all requests (every continuation has at least one id, so no result is empty)
        sums = torch.stack([r.token_logprobs.to(torch.float64).sum() for r in res]).tolist()
        greedy = torch.stack([(r.argmax == r.target_ids).all() for r in res]).tolist()
        return [(float(s), bool(g)) for s, g in zip(sums, greedy)]

    # ---- EVAL:448-452 ------------------------------------------------------------------------------------------
    def _sampling(self, where: str, unused: dict, do_sample, temperature, top_k, top_p, seed, repetition_penalty=None,
                  no_repeat_ngram_size=None, min_new_tokens=None, **warpers):
        """HF decoding arguments -> (SamplingParams (None = greedy), LogitsRules (None = no rule)); unsupported options warn
        (leopard_amd.sampling).  ``warpers``: min_p / typical_p / epsilon_cutoff / eta_cutoff of the call."""
        sampling.warn_unsupported(where, unused)
        sp = sampling.resolve(self.generation_defaults, do_sample, temperature, top_k, top_p, seed, **warpers)
        rules = sampling.resolve_rules(self.generation_defaults, repetition_penalty, no_repeat_ngram_size, min_new_tokens)
        self.last_decoding = sampling.describe(sp, rules)
        return sp, rules

    @torch.no_grad()
    def generate(self, input_ids, pixel_values=None, attention_mask=None, pad_token_id=None, eos_token_id=None,
                 max_new_tokens: int = 128, use_cache: bool = True, do_sample=None, temperature=None, top_k=None, top_p=None,
                 seed: Optional[int] = None, logprobs: Optional[int] = None, repetition_penalty=None, no_repeat_ngram_size=None,
                 min_new_tokens=None, min_p=None, typical_p=None, epsilon_cutoff=None,
                 eta_cutoff=None, **unused):
        """Greedy (EVAL:448-452), or sampled with ``do_sample=True`` (temperature / top_k / top_p, then min_p / typical_p / epsilon_cutoff /
        eta_cutoff, HF semantics and order: leopard_amd.sampling).
        ``repetition_penalty`` / ``no_repeat_ngram_size`` / ``min_new_tokens``: HF's logits processors over the ids of ``input_ids`` and the
        generated tokens, inside the decode step (LeopardEngine's LogitsRules); not together with ``logprobs``.
        ``logprobs`` = k in 0 .. 8: returns a ``sampling.GenerationLogprobs`` (.sequences, .token_logprobs, .top_token_ids, .top_logprobs,
        .sequence_logprob) instead of the tensor — computed inside the decode step (LeopardEngine.generate)."""
        sp, rules = self._sampling("generate", unused, do_sample, temperature, top_k, top_p, seed, repetition_penalty, no_repeat_ngram_size,
                                   min_new_tokens, min_p=min_p, typical_p=typical_p,
                                   epsilon_cutoff=epsilon_cutoff, eta_cutoff=eta_cutoff)
        if input_ids.shape[0] != 1:
            raise NotImplementedError("batch 1 per call, as in the reference harness")
        tiles = self._as_tiles(pixel_values)
        out = self.engine.generate(input_ids.to(self.device), tiles, max_new_tokens=max_new_tokens, eos_token_id=_eos_list(eos_token_id), sampling=sp,
                                   logprobs=logprobs, rules=rules)
        return _with_logprobs(out, logprobs, one=True)

    @torch.no_grad()
    def generate_beams(self, input_ids, pixel_values=None, num_beams=None, max_new_tokens: int = 128, eos_token_id=None, length_penalty=None,
                       early_stopping=None, num_return_sequences: int = 1, repetition_penalty=None, no_repeat_ngram_size=None,
                       min_new_tokens=None, **unused):
        """Beam search (HF's ``generate(num_beams=K, do_sample=False)``: LeopardEngine.generate_beams) with the prompt's K / V rows stored
        once for all beams (``decode`` = "shared").  ``repetition_penalty`` / ``no_repeat_ngram_size`` / ``min_new_tokens``: HF's logits
        processors on every beam's log-softmax scores (call arguments over generation_config.json over "off").  ``num_beams`` / ``length_penalty`` / ``early_stopping`` left unset take the
        checkpoint's generation_config.json value, else HF's default (1, 1.0, False).  Returns the best sequence [1, n], or the list of
        the ``num_return_sequences`` best, best first.  ``generate(num_beams=)`` itself still warns and decodes greedily."""
        sampling.warn_unsupported("generate_beams", unused)
        K, lp, es = sampling.resolve_beams(self.beam_defaults, num_beams, length_penalty, early_stopping)
        rules = sampling.resolve_rules(self.generation_defaults, repetition_penalty, no_repeat_ngram_size, min_new_tokens)
        if input_ids.shape[0] != 1:
            raise NotImplementedError("batch 1 per call, as in the reference harness")
        out = self.engine.generate_beams(input_ids.to(self.device), self._as_tiles(pixel_values), K, max_new_tokens=max_new_tokens,
                                         eos_token_id=_eos_list(eos_token_id), length_penalty=lp, early_stopping=es,
                                         num_return_sequences=num_return_sequences, decode="shared", rules=rules)
        self.last_decoding = sampling.describe_beams(K, lp, es) + ("" if rules is None else " + " + rules.describe())
        return sampling.beam_outputs(out, num_return_sequences, input_ids.device)

    @torch.no_grad()
    def generate_batch(self, requests: Sequence[Tuple[torch.Tensor, Optional[torch.Tensor]]], eos_token_id=None,
                       max_new_tokens: int = 128, do_sample=None, temperature=None, top_k=None, top_p=None, seed: Optional[int] = None,
                       logprobs: Optional[int] = None, repetition_penalty=None, no_repeat_ngram_size=None, min_new_tokens=None,
                       min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None, **unused):
        """[(input_ids [1, S_in], pixel_values)] -> [LongTensor [1, S_in + T]]: the batched form of ``generate`` (one packed prefill
        for all requests, LeopardEngine.generate_batch).  Not a surface of the reference script — its loop is batch 1 — but of
        leopard_amd.harness.run_inference(batch_size=...).  Sampling: request i draws with its own seed (SamplingParams.for_request).
        ``logprobs`` = k: a list of ``sampling.GenerationLogprobs``, one per request, instead of the tensors."""
        sp, rules = self._sampling("generate_batch", unused, do_sample, temperature, top_k, top_p, seed, repetition_penalty,
                                   no_repeat_ngram_size, min_new_tokens, min_p=min_p, typical_p=typical_p,
                                   epsilon_cutoff=epsilon_cutoff, eta_cutoff=eta_cutoff)
        samples = [(ids.to(self.device), self._as_tiles(pix)) for ids, pix in requests]
        out = self.engine.generate_batch(samples, max_new_tokens=max_new_tokens, eos_token_id=_eos_list(eos_token_id), sampling=sp,
                                         logprobs=logprobs, rules=rules)
        return _with_logprobs(out, logprobs)


    @torch.no_grad()
    def generate_shared(self, prefix_ids, pixel_values, suffix_ids_list: Sequence[torch.Tensor], eos_token_id=None, max_new_tokens: int = 128,
                        do_sample=None, temperature=None, top_k=None, top_p=None, seed: Optional[int] = None, decode: str = "copy",
                        logprobs: Optional[int] = None, repetition_penalty=None, no_repeat_ngram_size=None, min_new_tokens=None,
                        min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None, **unused):
        """Many questions about one set of images: ``prefix_ids`` [1, S_p] (the chat head and every image group, with ``pixel_values``) is
        prefilled ONCE — the vision tower runs once — and the text-only ``suffix_ids_list`` ([1, s_j] each: question, instruction, tail)
        continue from its cache together (LeopardEngine.generate_shared).  Returns [LongTensor [1, S_p + s_j + T]], each what ``generate``
        returns for the concatenated prompt.  Decoding kwargs as ``generate_batch``; request i draws with its own seed.  Memory: with
        ``decode`` = "copy" (the default) every decode slot holds its own copy of the prefix rows, B x (P + s + T) rows per layer; with
        ``decode`` = "shared" the prefix is stored once and read once per step for the whole batch — about P + B x (s + T) rows per layer
        (head_dim 128 and 4 query heads per KV head; NotImplementedError otherwise).  ``logprobs`` = k: a list of
        ``sampling.GenerationLogprobs`` instead of the tensors (ranking the N answers by ``sequence_logprob`` needs no second pass)."""
        sp, rules = self._sampling("generate_shared", unused, do_sample, temperature, top_k, top_p, seed, repetition_penalty,
                                   no_repeat_ngram_size, min_new_tokens, min_p=min_p, typical_p=typical_p,
                                   epsilon_cutoff=epsilon_cutoff, eta_cutoff=eta_cutoff)
        out = self.engine.generate_shared(prefix_ids.to(self.device), self._as_tiles(pixel_values), [s.to(self.device) for s in suffix_ids_list],
                                          max_new_tokens=max_new_tokens, eos_token_id=_eos_list(eos_token_id), sampling=sp, decode=decode,
                                          logprobs=logprobs, rules=rules)
        return _with_logprobs(out, logprobs)

    @torch.no_grad()
    def generate_stream(self, requests: Sequence[Tuple[torch.Tensor, Optional[torch.Tensor]]], batch_size: int = 8, eos_token_id=None,
                        max_new_tokens: int = 128, stats: Optional[dict] = None, do_sample=None, temperature=None, top_k=None, top_p=None,
                        seed: Optional[int] = None, logprobs: Optional[int] = None, repetition_penalty=None, no_repeat_ngram_size=None,
                        min_new_tokens=None, min_p=None, typical_p=None, epsilon_cutoff=None,
                        eta_cutoff=None, **unused):
        """Continuous batching over a list of requests: ``batch_size`` decode slots kept busy (LeopardEngine.generate_stream); the outputs
        come back in request order, each what ``generate`` returns for that request.  Sampling: request i draws with its own seed
        (SamplingParams.for_request), so its tokens do not depend on ``batch_size``.  ``logprobs`` = k: a list of
        ``sampling.GenerationLogprobs`` instead of the tensors."""
        sp, rules = self._sampling("generate_stream", unused, do_sample, temperature, top_k, top_p, seed, repetition_penalty,
                                   no_repeat_ngram_size, min_new_tokens, min_p=min_p, typical_p=typical_p,
                                   epsilon_cutoff=epsilon_cutoff, eta_cutoff=eta_cutoff)
        # a callable in place of the pixels is called when a slot admits the request (leopard_amd.harness: bounded memory over a shard)
        samples = [(ids.to(self.device), (lambda f=pix: self._as_tiles(f())) if callable(pix) else self._as_tiles(pix)) for ids, pix in requests]
        out = self.engine.generate_stream(samples, batch_size=batch_size, max_new_tokens=max_new_tokens, eos_token_id=_eos_list(eos_token_id),
                                          stats=stats, sampling=sp, logprobs=logprobs, rules=rules)
        return _with_logprobs(out, logprobs)


def _eos_list(eos_token_id) -> list:
    """HF's ``eos_token_id`` (None, one id, or a list / tuple of ids) as the engine's sequence of ids."""
    return eos_token_id if isinstance(eos_token_id, (list, tuple)) else ([] if eos_token_id is None else [eos_token_id])


def _with_logprobs(out, logprobs, one: bool = False):
    """An engine generation call's return value as the surface returns it: unchanged without ``logprobs``, else one
    ``sampling.GenerationLogprobs`` per request (``one``: that of the only request)."""
    if logprobs is None:
        return out
    res = sampling.logprob_outputs(out)
    return res[0] if one else res


def shared_context_split(contexts, image_token_index: int):
    """(head ids [1, h], [tail ids [1, t_j >= 1]]) of the context ids of one group: the longest common prefix, cut so that every context keeps at
    least one id as its tail.  None when there is no common head or a tail would hold an image token (images belong to the prefix)."""
    ctx = [torch.as_tensor(c).reshape(-1).to("cpu", torch.int64) for c in contexts]
    n = min(int(c.numel()) for c in ctx) - 1
    differ = (torch.stack([c[:n] for c in ctx]) != ctx[0][:n]).any(dim=0).nonzero() if n > 0 else torch.zeros(0, 1)
    h = int(differ[0]) if differ.numel() else max(n, 0)
    if h < 1 or any(bool((c[h:] == image_token_index).any()) for c in ctx):
        return None
    return ctx[0][:h].reshape(1, -1), [c[h:].reshape(1, -1) for c in ctx]


def score_loglikelihood(engine: LeopardEngine, requests, batch_size: int, device) -> List[Tuple[float, bool]]:
    """loglikelihood() of the model surfaces: requests [(context_ids, continuation_ids, tiles / images)] through engine.score_batch."""
    if batch_size < 1:
        raise ValueError(f"batch_size must be >= 1, got {batch_size}")
    packed = []
    for ctx, cont, vis in requests:
        ctx, cont = torch.as_tensor(ctx).reshape(1, -1).to(torch.int64), torch.as_tensor(cont).reshape(1, -1).to(torch.int64)
        ids = torch.cat([ctx.cpu(), cont.cpu()], dim=1)
        labels = torch.cat([torch.full_like(ctx.cpu(), LeopardEngine.IGNORE_INDEX), cont.cpu()], dim=1)
        packed.append((ids.to(device), vis, labels))
    out = []
    for i in range(0, len(packed), batch_size):
        for r in engine.score_batch(packed[i:i + batch_size]):
            out.append((float(r.token_logprobs.to(torch.float64).sum()), bool((r.argmax == r.target_ids).all())))
    return out


def from_pretrained(path: str, torch_dtype=torch.float32, **kw) -> LeopardForConditionalGeneration:
    """Drop-in for ``myLlavaForConditionalGeneration.from_pretrained``."""
    return LeopardForConditionalGeneration.from_pretrained(path, torch_dtype=torch_dtype, **kw)
