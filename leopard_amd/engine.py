"""Prefill / decode orchestration of the Leopard-LLaVA hot path on one MI355X.

Host Python only sequences kernel launches on the current HIP stream; every arithmetic step is a call into
libleopard_amd.so (see leopard_amd/ops.py).  The data path mirrors the reference forward
(evaluations/models/llava_multiimg_siglip_anyres.py:261-333, "EVAL"):

    u8 tiles / pixel_values --lmi_preprocess_tiles--> im2col rows
      --GEMM(+bias +pos-emb)--> fp32 ViT stream --27x[LN, QKV GEMM, varlen attention (one 676-token sequence per
      tile), out-proj GEMM(+residual), LN, fc1 GEMM(+gelu_tanh), fc2 GEMM(+residual)]--> post-LN           (EVAL:268-273)
      --GEMM(pixel-shuffle gather, +gelu_erf)--GEMM--> visual tokens [N*169, 4096] fp32                      (EVAL:283)
      --lmi_embed_merge (host-planned index map)--> fp32 LLM stream [S, 4096]                                (EVAL:263,285)
      --32x[RMSNorm, QKV GEMM, RoPE(+KV cache), causal GQA attention, o GEMM(+residual), RMSNorm,
            gate/up GEMM(+SwiGLU), down GEMM(+residual)]--> final RMSNorm --> lm_head                        (EVAL:322-333)

HBM residency: the residual streams are fp32 (ViT [N*676,1152], LLM [S,4096]); GEMM operands and activations
between kernels are the 16-bit compute type; weights are converted once at load (leopard_amd/weights.py).
"""
from __future__ import annotations

import contextlib
import gc
import math
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .config import LeopardConfig
from .ops import Ops
from .weights import EngineWeights


def llama3_inv_freq(head_dim: int, theta: float, scaling) -> torch.Tensor:
    """Inverse RoPE frequencies with the llama3.1 wavelength-dependent scaling
    (Megatron-LM-240603/megatron/core/models/common/embeddings/rotary_pos_embedding.py:48-83)."""
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float32) / head_dim))
    if scaling is None:
        return inv
    lo_wl = scaling.original_max_position_embeddings / scaling.low_freq_factor
    hi_wl = scaling.original_max_position_embeddings / scaling.high_freq_factor
    wl = 2 * math.pi / inv
    scaled = torch.where(wl > lo_wl, inv / scaling.factor, inv)
    smooth = (scaling.original_max_position_embeddings / wl - scaling.low_freq_factor) / (
        scaling.high_freq_factor - scaling.low_freq_factor)
    mid = (1 - smooth) * scaled / scaling.factor + smooth * scaled
    return torch.where(~(wl < hi_wl) & ~(wl > lo_wl), mid, scaled)


def plan_merge(input_ids: np.ndarray, image_token_index: int, n_feature_rows: int, tokens_per_tile: int) -> np.ndarray:
    """Index map of the merged sequence (transformers-4.38 ``_merge_input_ids_with_image_features`` semantics for
    one unpadded sample, EVAL:284-287): ``src[s] >= 0`` -> text embedding of input position ``src[s]``;
    ``src[s] < 0`` -> visual token row ``-src[s]-1``.  Raises ValueError on an image-token / feature count
    mismatch, before any kernel is launched."""
    ids = np.asarray(input_ids, dtype=np.int64).reshape(-1)
    is_img = ids == image_token_index
    n_img = int(is_img.sum())
    if n_img * tokens_per_tile != n_feature_rows:
        raise ValueError(
            f"The input provided to the model are wrong. The number of image tokens is {n_img} while the number of "
            f"image given to the model is {n_feature_rows // max(tokens_per_tile, 1)}. This prevents correct indexing "
            "and breaks batch generation.")
    width = np.where(is_img, tokens_per_tile, 1)
    start = np.cumsum(width) - width
    S = int(width.sum())
    src = np.empty(S, dtype=np.int64)
    text_pos = np.nonzero(~is_img)[0]
    src[start[text_pos]] = text_pos
    img_pos = np.nonzero(is_img)[0]
    if n_img:
        rows = (start[img_pos][:, None] + np.arange(tokens_per_tile)[None, :]).reshape(-1)
        src[rows] = -(np.arange(n_img * tokens_per_tile) + 1)
    return src


@dataclass
class PrefillResult:
    logits_last: torch.Tensor                    # fp32 [vocab]
    seq_len: int
    n_tiles: int
    logits_all: Optional[torch.Tensor] = None    # fp32 [S, vocab] when requested (what the reference computes)
    parts: Optional[Dict[str, torch.Tensor]] = None


@dataclass
class ScoreResult:
    """LeopardEngine.score: the labelled tokens of one request under the model (EVAL:333-348 semantics over merged rows)."""
    loss: torch.Tensor                           # fp32 0-dim (device): mean of -token_logprobs; nan when nothing is labelled
    token_logprobs: torch.Tensor                 # fp32 [n]: log p(target | rows <= row)
    argmax: torch.Tensor                         # int64 [n]: the most likely token of the row (lowest index on ties)
    target_ids: torch.Tensor                     # int64 [n]
    rows: torch.Tensor                           # int64 [n]: merged rows that predict the targets (row s predicts merged label s + 1)
    seq_len: int


@dataclass
class ExtendResult:
    """LeopardEngine.extend: N text suffixes continued from one cached prefix."""
    logits: torch.Tensor                         # fp32 [N, vocab]: the last row of every suffix
    seq_lens: List[int]                          # the suffix lengths s_j (rows; suffixes are text only)
    prefix_len: int                              # P: suffix j's rows sit at positions P .. P + s_j - 1
    kv_out: Optional["KVCache"] = None           # the suffixes' K / V at packed row offsets (sum of the earlier s_j), when asked for


@dataclass
class GenerateOutput:
    """What generate / generate_batch / generate_stream / generate_shared return with ``logprobs=k``: the call's usual return value and, per
    request, the log-probability of every generated token (the one from the prefill logits included) and the k most likely tokens of each
    step.  All numbers are log-softmax values of the RAW logits row the token was chosen from (lmi_decode_logprobs: no temperature, no
    suppress list) — what ``score`` / ``loglikelihood`` report on those logits; under sampling or ``suppress_tokens`` the chosen token need
    not be ``top_ids[t, 0]``."""
    sequences: object                            # the return value of the call without ``logprobs`` (a tensor, or a list of tensors)
    token_logprobs: List[torch.Tensor]           # per request fp32 [T]
    top_ids: List[torch.Tensor]                  # per request int64 [T, k]: value descending, lower id first on ties; -1 = no such entry
    top_logprobs: List[torch.Tensor]             # per request fp32 [T, k]

    @staticmethod
    def join(parts: Sequence["GenerateOutput"]) -> "GenerateOutput":
        """One output of several calls, in order (``sequences`` becomes the list of all their sequences)."""
        seqs: List[torch.Tensor] = []
        for p in parts:
            seqs += p.sequences if isinstance(p.sequences, list) else [p.sequences]
        return GenerateOutput(seqs, [t for p in parts for t in p.token_logprobs], [t for p in parts for t in p.top_ids],
                              [t for p in parts for t in p.top_logprobs])


@dataclass
class BeamOutput:
    """What ``generate_beams`` returns: the ``num_return_sequences`` best finished hypotheses, best first."""
    sequences: List[torch.Tensor]                # LongTensor [1, S_in + T_i] each, on the input's device
    scores: List[float]                          # accumulated log-probability / T_i ** length_penalty (fp32 arithmetic, as transformers)


class _LogprobRows:
    """Host side of one request's logprob rows: slices of the rings as they are drained, in token order."""
    def __init__(self, k: int):
        self.k, self.lp, self.ti, self.tl = k, [], [], []

    def add(self, lp: torch.Tensor, ti: torch.Tensor, tl: torch.Tensor) -> None:
        """n more tokens: lp [n], ti / tl [n, 8]."""
        self.lp.append(lp.reshape(-1)); self.ti.append(ti.reshape(-1, ti.shape[-1])); self.tl.append(tl.reshape(-1, tl.shape[-1]))

    def result(self, T: int):
        """(token_logprobs [T], top_ids [T, k], top_logprobs [T, k]) of the request's T generated tokens."""
        k = self.k
        if not self.lp:
            return torch.zeros(0), torch.zeros(0, k, dtype=torch.int64), torch.zeros(0, k)
        lp, ti, tl = torch.cat(self.lp)[:T], torch.cat(self.ti)[:T, :k], torch.cat(self.tl)[:T, :k]
        assert lp.numel() == T, (lp.numel(), T)
        return lp.clone(), ti.to(torch.int64), tl.clone()


class KVCache:
    def __init__(self, cfg: LeopardConfig, capacity: int, dtype, device, tp_size: int = 1):
        tc = cfg.text_config
        w = tc.num_key_value_heads // tp_size * tc.head_dim          # a tensor-parallel rank caches its own kv heads
        self.k = [torch.zeros(capacity, w, dtype=dtype, device=device) for _ in range(tc.num_hidden_layers)]
        self.v = [torch.zeros(capacity, w, dtype=dtype, device=device) for _ in range(tc.num_hidden_layers)]
        self.capacity, self.length = capacity, 0
        self._decode_state = None                # the DecodeState of the batch-1 step over this cache (LeopardEngine._decode_state)


@dataclass
class SamplingParams:
    """Sampled decoding (lmi_decode_sample, csrc/sample.h): temperature, then top-k (0 = off), then top-p (1.0 = off); the draws of a
    request are Philox4x32-10 keyed by ``seed``, one counter step per produced token (step 0 = the token from the prefill's logits).
    Then HF's remaining warpers, in HF's order, each over what the earlier ones left (lmi_decode_sample_ex): ``min_p`` in (0, 1] (0 = off),
    ``typical_p`` in (0, 1) (1.0 = off), ``epsilon_cutoff`` and ``eta_cutoff`` in (0, 1) (0 = off).  A call with all four off runs
    lmi_decode_sample."""
    temperature: float = 1.0
    top_k: int = 50
    top_p: float = 1.0
    seed: int = 0
    min_p: float = 0.0
    typical_p: float = 1.0
    epsilon_cutoff: float = 0.0
    eta_cutoff: float = 0.0

    def __post_init__(self):
        self.min_p = 0.0 if self.min_p is None else float(self.min_p)
        if not 0.0 <= self.min_p <= 1.0:
            raise ValueError(f"min_p must be in [0, 1], got {self.min_p}")
        self.typical_p = float(self.typical_p)
        if not 0.0 < self.typical_p <= 1.0:
            raise ValueError(f"typical_p must be in (0, 1], got {self.typical_p}")
        self.epsilon_cutoff, self.eta_cutoff = float(self.epsilon_cutoff), float(self.eta_cutoff)
        if not 0.0 <= self.epsilon_cutoff < 1.0:
            raise ValueError(f"epsilon_cutoff must be in [0, 1), got {self.epsilon_cutoff}")
        if not 0.0 <= self.eta_cutoff < 1.0:
            raise ValueError(f"eta_cutoff must be in [0, 1), got {self.eta_cutoff}")
        if not self.temperature > 0:
            raise ValueError(f"temperature must be > 0 when sampling, got {self.temperature}")
        if int(self.top_k) < 0:
            raise ValueError(f"top_k must be >= 0, got {self.top_k}")
        if not 0.0 <= float(self.top_p) <= 1.0:
            raise ValueError(f"top_p must be in [0, 1], got {self.top_p}")
        self.seed = int(self.seed) & ((1 << 64) - 1)

    def for_request(self, i: int) -> "SamplingParams":
        """The parameters of request i of a call: its seed depends on the call's seed and i only (not on batch size or admission order)."""
        return SamplingParams(self.temperature, self.top_k, self.top_p, (self.seed + i * 0x9E3779B97F4A7C15) & ((1 << 64) - 1),
                              self.min_p, self.typical_p, self.epsilon_cutoff, self.eta_cutoff)

    @property
    def extended(self) -> bool:
        """Any of min_p / typical_p / epsilon_cutoff / eta_cutoff is on: the step draws with lmi_decode_sample_ex."""
        return self.min_p > 0.0 or self.typical_p < 1.0 or self.epsilon_cutoff > 0.0 or self.eta_cutoff > 0.0

    def describe(self) -> str:
        more = "".join(f", {name}={v:g}" for name, v, off in (("min_p", self.min_p, 0.0), ("typical_p", self.typical_p, 1.0),
                                                             ("epsilon_cutoff", self.epsilon_cutoff, 0.0),
                                                             ("eta_cutoff", self.eta_cutoff, 0.0)) if v != off)
        return f"sample(temperature={self.temperature:g}, top_k={int(self.top_k)}, top_p={self.top_p:g}{more})"


@dataclass(frozen=True)
class LogitsRules:
    """Logits processors of a generation call (lmi_decode_rules, csrc/decode_rules.h), applied inside the decode step before the choice, in
    HF's order: ``repetition_penalty`` (1.0 = off) over every id of the prompt and of the tokens generated so far, ``no_repeat_ngram_size``
    (0 = off) over the same ids, ``min_new_tokens`` (0 = off): the call's eos ids cannot be chosen before that many new tokens exist."""
    repetition_penalty: float = 1.0
    no_repeat_ngram_size: int = 0
    min_new_tokens: int = 0

    def __post_init__(self):
        if not float(self.repetition_penalty) > 0:
            raise ValueError(f"repetition_penalty must be > 0, got {self.repetition_penalty}")
        if int(self.no_repeat_ngram_size) < 0:
            raise ValueError(f"no_repeat_ngram_size must be >= 0, got {self.no_repeat_ngram_size}")
        if int(self.min_new_tokens) < 0:
            raise ValueError(f"min_new_tokens must be >= 0, got {self.min_new_tokens}")

    @property
    def active(self) -> bool:
        return float(self.repetition_penalty) != 1.0 or int(self.no_repeat_ngram_size) > 0 or int(self.min_new_tokens) > 0

    def describe(self) -> str:
        parts = []
        if float(self.repetition_penalty) != 1.0:
            parts.append(f"repetition_penalty={float(self.repetition_penalty):g}")
        if int(self.no_repeat_ngram_size) > 0:
            parts.append(f"no_repeat_ngram_size={int(self.no_repeat_ngram_size)}")
        if int(self.min_new_tokens) > 0:
            parts.append(f"min_new_tokens={int(self.min_new_tokens)}")
        return " + ".join(parts)


@contextlib.contextmanager
def _capture_safe():
    """Hold off Python's cyclic garbage collector while a HIP graph is captured.  A collection that starts inside the capture runs the
    finalizers of whatever dead cycle it finds there — an engine left by an earlier caller, with its own captured graphs and events — and
    releasing those is not allowed on a capturing stream: the process aborts.  The garbage is collected after the capture instead."""
    was = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


def _signed64(v: int) -> int:
    return v - (1 << 64) if v >= (1 << 63) else v


@dataclass(eq=False)
class DecodeState:
    """Static buffers, device counters and captured graphs of one decode step over B rows: the batch-1 step of one KVCache
    (LeopardEngine._decode_state, kept on the cache) or the B slots of a pooled cache (LeopardEngine._batch_state)."""
    B: int
    capacity: int                                # KV rows per sequence the step's launch geometry is built for
    mode: tuple                                  # (precision, decode_precision) the buffers and launches belong to: another mode rebuilds the state
    layout: bool                                 # llm_packed at construction: a captured step replays the launches of that weight layout
    hl: bool                                     # operand buffers hold [hi rows; lo rows] pairs (decode precision mode, decode_hl)
    tok: torch.Tensor                            # int64 [B]: the token each row consumes; the step leaves the next one here
    src: torch.Tensor                            # int64 [B] = 0 .. B-1: row b of the stream is the embedding of tok[b] (lmi_embed_merge)
    pos: torch.Tensor                            # int32 [B]
    cu_q: torch.Tensor                           # int32 [B + 1]: one query row per sequence
    k_begin: torch.Tensor                        # int32 [B]: first cache row of each sequence, b * capacity
    x: torch.Tensor                              # fp32 [B, D] residual rows
    h: torch.Tensor
    qkv: torch.Tensor
    att: torch.Tensor
    gu: torch.Tensor
    hf32: Optional[torch.Tensor]                 # fp32 [B, D] (hl only): a norm's output before it is split into a pair
    cos: torch.Tensor
    sin: torch.Tensor
    ws: torch.Tensor                             # decode attention workspace (lmi_decode_workspace_elems)
    # per-row sampling parameters in device memory: written before a replay, read by the captured step, so new parameters never need a
    # new capture.  ``sampling`` selects which captured step runs (``graphs``)
    temp: torch.Tensor
    topk: torch.Tensor
    topp: torch.Tensor
    seed: torch.Tensor
    step: torch.Tensor
    ext: torch.Tensor                            # fp32 [4, B]: min_p, typical_p, epsilon_cutoff, eta_cutoff (lmi_decode_sample_ex), one buffer
    # generate(logprobs=k): the rings lmi_decode_logprobs writes after the choice kernel — ONE buffer of 4-byte words, so that the host
    # drains all three with one copy: lp fp32 [ring, B], top_id int32 [ring, B, 8], top_lp fp32 [ring, B, 8] are views of it.  ring = HIST
    # for the pooled states (slot = the step's place in the token history ring), 1 for the batch-1 state (read every step, with the token).
    # Allocated by the first call with ``logprobs`` (_set_logprobs): a state that never sees one holds what it held before
    sampling: bool = False
    sample_ex: bool = False                      # the running call has one of the four warpers of ``ext`` on: the step draws with _ex
    lp_buf: Optional[torch.Tensor] = None
    lp: Optional[torch.Tensor] = None
    top_id: Optional[torch.Tensor] = None
    top_lp: Optional[torch.Tensor] = None
    logprobs: Optional[int] = None               # k of the running call: the step also launches lmi_decode_logprobs
    # generate(rules=...): the device side of lmi_decode_rules — per slot the ids seen so far (the prompt as the caller passed it, then one
    # id per step, appended by the kernel), its parameters and the steps eos stays banned; the eos ids of the running call.  4 bytes x
    # (prefix_capacity + capacity) per slot.  Allocated by the first call with ``rules`` (_set_rules): a state that never sees one holds
    # what it held before.  The parameters are device values: other values never capture again
    rules: bool = False                          # the running call has rules: the step launches lmi_decode_rules before the choice
    seq: Optional[torch.Tensor] = None           # int32 [B, prefix_capacity + capacity]
    seq_len: Optional[torch.Tensor] = None       # int32 [B]
    rule_pen: Optional[torch.Tensor] = None      # fp32 [B]
    rule_ngram: Optional[torch.Tensor] = None    # int32 [B]
    rule_min_left: Optional[torch.Tensor] = None  # int32 [B]
    rule_eos: Optional[torch.Tensor] = None      # int64 [MAX_EOS], -1 = unused
    # generate_beams: K = ``beams`` > 0 makes the step's tail lmi_beam_step + lmi_beam_reorder instead of the choice kernel.  All device
    # memory, allocated by the first beam search on the state (_set_beams); the eos ids, the first row that can differ between slots and
    # the rows held are device values, so another prompt or eos list never captures again
    beams: int = 0
    beam_score: Optional[torch.Tensor] = None    # fp32 [8]: the beams' accumulated log-probabilities
    beam_parent: Optional[torch.Tensor] = None   # int32 [8]: the slot each new beam descends from
    beam_walk: Optional[torch.Tensor] = None     # int32 [LMI_BEAM_WALK_WORDS]: the step's walk list, the ONE buffer the host reads per step
    beam_rows: Optional[tuple] = None            # the row launch's outputs: (row_lse, row_id, row_lp, row_eos_lp)
    beam_eos: Optional[torch.Tensor] = None      # int64 [4], -1 = unused
    beam_row0: Optional[torch.Tensor] = None     # int32 [1]: 0 in a shared-prefix state, the prompt length in a copy state
    beam_held: Optional[torch.Tensor] = None     # int32 [1]: the rows every slot holds
    beam_ptrs: Optional[torch.Tensor] = None     # int64 [2 L]: the base pointers of st.k and st.v
    beam_max_rows: int = 0                       # host bound on the divergent rows (a multiple of 256): the reorder launch's grid
    # generate_beams(rules=...): the step's tail is lmi_beam_step_rules over ``seq`` and the rule parameters above (every slot starts with
    # the prompt's ids), then one more lmi_beam_reorder over ``seq`` in 16-byte chunks of four ids — 4 bytes x the slot's id capacity x K
    beam_id_ptr: Optional[torch.Tensor] = None   # int64 [1]: the base pointer of ``seq``
    beam_id_chunks: Optional[torch.Tensor] = None  # int32 [2]: the chunk that holds the first generated id, the chunks a finished call holds
    # the captured steps (LeopardEngine._run_step), keyed by (sampling, with logprobs): greedy / sampled, each without and with the logprobs
    # launch — the latter two with top_k = lp_k — and by (sampling, False, True) for the steps with the rules launch; a beam step adds
    # ("beams", K, reorder bound) to its key, without and with rules; a sampled step that draws with lmi_decode_sample_ex adds "ex"
    graphs: dict = field(default_factory=dict)
    lp_k: Optional[int] = None                   # the top_k the two logprobs graphs were captured with (another k captures them again)
    graph_failed: bool = False                   # tensor parallel: the capture failed once, the step runs eagerly (_decode_run)
    graph_comm_bytes: int = 0                    # tensor parallel: what one replay puts on the links
    sq_a: Optional[torch.Tensor] = None          # folded-norm partials: feeding gate/up ...
    sq_b: Optional[torch.Tensor] = None          # ... and the next layer's q|k|v
    logits: Optional[torch.Tensor] = None        # fp32 [Vp] (batch-1 step) / [B, Vp]
    # the batch-1 step of one KVCache only
    cu_k: Optional[torch.Tensor] = None          # int32 [2]: [0, key count]
    part: Optional[torch.Tensor] = None          # tensor parallel: partial o_proj / down_proj row
    # the pooled step only: B slots of capacity rows per layer (slot b = rows [b * capacity, (b + 1) * capacity)) and the device side of
    # continuous batching (_batch_state)
    k: Optional[List[torch.Tensor]] = None
    v: Optional[List[torch.Tensor]] = None
    k_len: Optional[torch.Tensor] = None
    # the shared-prefix pooled step only (_shared_state): ONE copy of the prefix K / V per layer, owned by the state (the captured step holds
    # no pointer into caller memory); the slots above then hold a sequence's OWN rows (capacity = own rows) and positions start at prefix_len
    kp: Optional[List[torch.Tensor]] = None      # [prefix_capacity, KV hd] per layer
    vp: Optional[List[torch.Tensor]] = None
    prefix_capacity: int = 0
    prefix_len: Optional[torch.Tensor] = None    # int32 [1], device: the attention's prefix length AND the append's row bias
    live: Optional[torch.Tensor] = None
    budget: Optional[torch.Tensor] = None
    eos: Optional[torch.Tensor] = None
    hist: Optional[torch.Tensor] = None
    hist_pos: Optional[torch.Tensor] = None


class LeopardEngine:
    def __init__(self, cfg: LeopardConfig, weights: EngineWeights, ops: Optional[Ops] = None, device=None,
                 use_tr: bool = True, comm=None, pack_llm_weights: Optional[bool] = None):
        self.cfg, self.W = cfg, weights
        self.ops = ops if ops is not None else Ops()
        self.dtype = weights.dtype
        self.device = torch.device(device) if device is not None else weights.embed.device
        self.use_tr = use_tr
        self.use_graphs = True         # capture the decode step in a HIP graph (cuda devices only)
        # tensor parallel (weights built with tp_size > 1): the communicator of the one-sample-on-all-ranks path (leopard_amd.dist)
        self.comm = comm
        if getattr(weights, "tp_size", 1) > 1 and comm is None:
            from . import dist as D
            self.comm = D.get_comm(self.device if self.device.type == "cuda" else None, getattr(self.ops, "lib", None))
            if self.comm is None or self.comm.world != weights.tp_size:
                raise RuntimeError(f"tensor-parallel weights (tp_size {weights.tp_size}) need an initialised process group of that size")
        self.tp_chunks = 2             # row chunks per layer under TP: chunk c's collectives overlap chunk c+1's GEMMs
        # dtype of the reduce-scattered partial products.  torch.float32 (default since round 5) = exact partial sums: at C2 full depth two ranks
        # with fp32 sums sit at 1.18e-3 of the logit scale against the fp32 reference — the one-rank fast schedule's 1.14e-3 — while the
        # 16-bit exchange (None = the compute type: half the reduce-scatter bytes) adds a rounding per partial product and half layer, 1.74e-3
        # (tests/test_gpu_dist.py, profiles/r05_tp_parity.txt).  LMI_TP_COMM_DTYPE=16 selects the 16-bit exchange.
        self.tp_comm_dtype = None if os.environ.get("LMI_TP_COMM_DTYPE", "32") == "16" else torch.float32
        # TP decode: capture the step (with its RCCL all-reduces) in a HIP graph when the communicator is RcclComm.  OFF by default: capture and
        # replay of a multi-rank RCCL step has only ever run on a one-rank communicator (tests/test_gpu_dist.py) — LMI_TP_DECODE_GRAPH=1 /
        # this flag opt in, and a failed capture falls back to the eager step (``_decode_run``)
        self.tp_decode_graph = os.environ.get("LMI_TP_DECODE_GRAPH", "0") == "1"
        # all-gather of the projected visual tokens: None = fp32 (bit-identical to one rank: the rows are merged into the fp32 residual stream,
        # which carries them unrounded through every layer); the 16-bit compute type halves the bytes (58 MB at C3) at one extra rounding
        self._comm_stream = None
        self._workspaces: Dict[tuple, torch.Tensor] = {}   # caller-owned scratch per (stage, launch stream) (lmi_llm_prefill_workspace_bytes / lmi_vit_workspace_bytes)
        self.graph_encode = False      # capture the vision encode per ViT-input count in a HIP graph (BASELINE config 5)
        self._encode_graphs: Dict[tuple, tuple] = {}   # (ViT-input count, stream) -> (graph, static in, static out)
        self._private_scratch = False  # True while an encode graph is warmed up / captured: _carve hands out fresh allocations the graph owns
        self.fuse_norm_rope = True     # Llama layers: RMSNorm + RoPE + KV append inside the GEMM epilogues (lmi_rmsnorm_rope / lmi_gemm_ex)
        # Last Llama / Mistral layer of a single-sequence prefill: "read" = everything after its k | v projection runs only on a
        # trailing row window that holds the row whose logits are read (nothing else of that layer is read afterwards: K / V need every row
        # of the layer's INPUT, the rest only feeds the head); "all" = every row (A/B; LMI_LAST_LAYER_ROWS).  Same bits either way.
        self.last_layer_rows = os.environ.get("LMI_LAST_LAYER_ROWS", "read")
        if self.last_layer_rows not in ("read", "all"):
            raise ValueError(f"LMI_LAST_LAYER_ROWS must be 'read' or 'all', not {self.last_layer_rows!r}")
        self.suppress_tokens = None    # optional int64 device tensor of token ids that greedy decoding may never emit (HF bad_words_ids)
        self.trace = None              # optional callable(name, fp32 residual stream) after the embeddings / every layer (tests)
        # Split-operand precision mode: every A operand of every ViT / LLM layer linear is handed over as a hi + lo pair of
        # 16-bit values (lmi_split_hi_lo) and multiplied against [W | W] — the GEMMs run at 2 K, the hand-over roundings that make up the
        # distance to the fp32 reference are gone (full-depth logits within north_star's 1e-3; ~1.8x the prefill time).  Prefill only.
        self.split_operands = False
        # Low-bit correction mode (round 5): the same goal at + 25 % matrix time instead of + 100 %.  Every producer of a layer-
        # linear A operand also hands over an MX fp4 image of the rounding residual x - T(x) (lmi_norm_lo4, lmi_split_lo4, the GELU / SwiGLU /
        # folded-norm GEMM epilogues), every layer linear has an fp4 weight image (+ 0.5 B per parameter), and the GEMMs run a second k-loop
        # phase of v_mfma_scale_f32_32x32x64_f8f6f4 on the two images into the accumulators of the 16-bit pass (lmi_gemm_lo4).  Prefill only;
        # one rank.  ``precision`` = "fast" | "lo4" | "split" selects between the three schedules.
        self.lo4 = False
        # lo4 corrects the LLM layer linears; ``lo4_vit`` (LMI_LO4_VIT=1) extends it to the SigLIP layer linears.  Off by default: measured at
        # full depth, the tower's correction moves the logits of the benchmarked C3 sample by < 1 % (2.35e-4 vs 2.37e-4 of the logit scale) and
        # those of the hardest case — C1: one ViT input, S = 228 — from 7.3e-4 to 6.1e-4, for + 6 % of the step (1.20 x vs 1.27 x the fast schedule)
        # Round 6: "auto" (default) = the tower is corrected too for the samples whose LLM sequence is short (<= LO4_FULL_BELOW rows: C1-like, where
        # the rounding noise of ONE realisation lands anywhere between 7e-4 and 1e-3 without it) — a per-SAMPLE decision carried to the tower's rows
        # by the same row selection as the LLM's (the tiles of a long sample in a packed batch stay on the fast tower: packed == separate).
        env_vit = os.environ.get("LMI_LO4_VIT", "auto")
        self.lo4_vit = "auto" if env_vit == "auto" else env_vit == "1"
        self._lo4_w = {}               # tower -> fp4 weight images (built when the mode is selected / on first use; dropped by invalidate_lo4_weights)
        # WHICH ROWS carry the correction (round 6; DESIGN.md 2.1 "row selection", tools/lo4_policy_study.py).  The logits of a row are dominated by
        # the hand-over roundings on that row's OWN path through the 32 layers; the roundings of the other rows reach it only through the softmax
        # average over the keys, i.e. attenuated by ~sqrt(S) (emulating oracle, C1: correcting ONLY the last row removes 90 % of what correcting all
        # 228 rows removes).  The rows whose logits are read are the last rows of each sequence, so by default ("auto") a sequence longer than
        # LO4_FULL_BELOW rows carries the correction on its last LO4_TAIL_ROWS rows only; shorter sequences on every row.  "all" = every row (round
        # 5's schedule); an int = that many trailing rows.  A property of the ROW (its distance from the end of its sequence), not of where the row
        # lands in a tile: packed == separate stays bit for bit.  LMI_LO4_ROWS overrides.
        env_rows = os.environ.get("LMI_LO4_ROWS", "auto")
        self.lo4_rows = env_rows if env_rows in ("auto", "all") else int(env_rows)
        self.decode_precision = os.environ.get("LMI_DECODE_PRECISION", "1") == "1"   # lo4 / split also cover the decode steps (decode_hl); 0 = fast decode (A/B)
        self._lo4_sel_cache: Dict[tuple, tuple] = {}
        self._score_sel_cache: Dict[tuple, tuple] = {}   # lo4 selections that include scored rows (_lo4_selection with extra rows)
        self.last_lo4_ranges = None    # [n, 2] int32 [begin, end) packed rows the last lo4 LLM pass corrected (None: no lo4 pass ran)
        self.score_chunk_rows = 1024   # score(): rows per head GEMM into the reusable fp32 chunk (525 MB at V = 128 256)
        self.skinny_fold_norm = True   # batched decode: RMSNorms folded into the projections (lmi_gemm_skinny_ex producer / consumer); False: norm launches
        self.skinny_packed = True      # batched decode over nn.Linear-layout weights (TP, pack_llm_weights=False): stream a packed second copy
        self.fp8_fused = True          # fp8 schedule: attention writes the fp8 o_proj operand, q|k|v GEMM does RoPE + KV append (False: separate launches)
        self.fp8_attention = os.environ.get("LMI_FP8_ATTENTION", "0") == "1"   # fp8 schedule: QK^T and PV of the Llama layers on the fp8 pipe too (attention_fp8.h)
        self._fp8 = None               # leopard_amd.fp8.Fp8Plan: fp8 operands for the ViT / LLM layer linears (enable_fp8; configs[4])
        self._rec = None               # calibration recorder callable((tower, layer, site), operand tensor)
        tc = cfg.text_config
        self._inv_freq = llama3_inv_freq(tc.head_dim, tc.rope_theta, tc.rope_scaling).to(self.device)
        self._geom_cache: Dict[tuple, tuple] = {}      # seq_lens -> (cu, cos, sin, last_rows) device tensors
        self._vit_cu_cache: Dict[int, torch.Tensor] = {}
        self._window_sel: Dict[tuple, tuple] = {}         # (row_sel pointer, w0) -> the lo4 selection tables of that row window (_window_selection)
        self._window_cu: Dict[tuple, torch.Tensor] = {}   # (S, w0) -> cu_seqlens_q of the last layer's row window (_last_layer_window)
        self._split_w = None           # [W | W] weight copies of the split-operand mode (_split_weights)
        self._gen_cache = None         # the KV cache generate() reuses (_generation_cache)
        self._stream_cache = None      # the KV cache generate_stream prefills a newcomer into before its rows move to a slot
        self._batch_states: Dict[int, DecodeState] = {}   # B -> state of the batched decode step (_batch_state)
        self._decode_batch_limit = self.MAX_DECODE_BATCH   # decode_batch_limit: sequences per captured step of generate_stream / generate_batch
        self._decode_pair_limit = self.PAIR_DECODE_BATCH   # decode_pair_limit: the most sequences a precision mode decodes on the pair (hl) step
        self._skinny_pack = None       # second copy of the LLM weights in the skinny-M operand order (_skinny_weights)
        self._head_pack = None         # lm_head in the packed order (_skinny_head)
        # ONE copy of the LLM weights (default; LMI_PACK_LLM_WEIGHTS=0 / pack_llm_weights=False keep the nn.Linear layout): see pack_llm_weights
        if pack_llm_weights is None:
            pack_llm_weights = os.environ.get("LMI_PACK_LLM_WEIGHTS", "1") == "1"
        if pack_llm_weights:
            self.pack_llm_weights()

    # ------------------------------------------------------------------------------------------------
    @property
    def fp8(self):
        return self._fp8

    @fp8.setter
    def fp8(self, plan):
        """Switching the schedule invalidates the captured vision-encode graphs (they replay the launches of the old one)."""
        self._fp8 = plan
        self._encode_graphs.clear()

    @property
    def tp_size(self) -> int:
        return getattr(self.W, "tp_size", 1)

    @property
    def precision(self) -> str:
        """"fast" (one rounding per operand hand-over: the benchmarked schedule up to round 4), "lo4" (+ the fp4 correction phase: meets
        north_star's 1e-3 at full depth), "split" (hi + lo 16-bit operand pairs at 2 K: the most exact, ~1.9 x the time)."""
        return "split" if self.split_operands else ("lo4" if self.lo4 else "fast")

    def lo4_supported(self) -> bool:
        """The lo4 schedule rides on the fused Llama / Mistral layer (head_dim 128, rope-ordered q|k|v rows, hidden % 256 == 0) and on
        32-element blocks along every contraction axis (hidden sizes and FFN widths % 32 == 0); 16-bit compute type.  Tensor-parallel
        engines run it too (round 5): the sequence-parallel norms hand over Lo4 pairs and the all-gathers move the images with the rows."""
        tc, vc, W = self.cfg.text_config, self.cfg.vision_config, self.W
        return bool(self.dtype in (torch.float16, torch.bfloat16) and tc.head_dim == 128 and tc.hidden_size % 256 == 0
                    and W.llm_layers and W.llm_layers[0].qkv_w_rope is not None and (tc.intermediate_size // self.tp_size) % 32 == 0
                    and tc.intermediate_size // self.tp_size >= 128 and vc.hidden_size % 32 == 0)

    @precision.setter
    def precision(self, mode: str):
        if mode not in ("fast", "lo4", "split"):
            raise ValueError(f"precision must be 'fast', 'lo4' or 'split', not {mode!r}")
        if mode == "split" and self.tp_size > 1:
            raise ValueError("the split-operand mode runs on one rank (tensor-parallel engines: 'fast' or 'lo4')")
        if mode == "lo4" and not self.lo4_supported():
            raise ValueError("precision 'lo4' needs the fused Llama / Mistral layer shape (head_dim 128, hidden % 256 == 0): use 'split'")
        self.split_operands, self.lo4 = mode == "split", mode == "lo4"
        self._encode_graphs.clear()                           # captured encodes replay the launches of the old schedule
        if self.lo4 and self.device.type == "cuda":
            self._lo4_weights("llm")                          # the multi-GB quantisation happens HERE, not inside the first (timed) prefill

    def decode_hl(self, B: int = 1, pair_limit: Optional[int] = None) -> bool:
        """Decode precision mode (round 6): with ``precision`` = "lo4" / "split" the captured decode step hands every projection operand over as a
        pair of 16-bit rows — T(x) and T(x - T(x)) — through the M <= 16 kernels (lmi_gemm_skinny_hl ...): the hand-over roundings of the token's
        own path through the layers, which are what its logits' error is made of, are gone, at no extra weight traffic.  Needs the packed one-copy
        weight layout (the default on one rank), the folded norms and B <= decode_pair_limit (8 pairs are the 16 rows of those kernels; above, the
        step runs on lmi_gemm_skinny_wide_hl ...: M <= 32 pairs); otherwise the step is the fast one.  ``pair_limit``: a caller's own cap
        (generate_shared keeps the 8-pair step)."""
        D = self.cfg.text_config.hidden_size
        limit = self._decode_pair_limit if pair_limit is None else min(self._decode_pair_limit, pair_limit)
        return bool((self.lo4 or self.split_operands) and self.decode_precision and self.tp_size == 1 and self.llm_packed and B <= limit
                    and self.skinny_fold_norm and D % 16 == 0 and self.cfg.text_config.head_dim == 128
                    and all(L.qkv_w_rope is not None for L in self.W.llm_layers))

    def _llm_heads(self) -> Tuple[int, int]:
        """(query heads, kv heads) this rank computes."""
        tc = self.cfg.text_config
        return (getattr(self.W, "llm_heads", 0) or tc.num_attention_heads, getattr(self.W, "llm_kv_heads", 0) or tc.num_key_value_heads)

    # ---- one copy of the LLM weights ----------------------------------------------------------------------------------------------
    @property
    def llm_packed(self) -> bool:
        """True when the layer linears are stored in the packed order.  The layout of a tensor is a mark on the tensor object
        (weights.mark_packed), which a copy (.clone() / .to()) does not carry: the engine remembers what it packed and refuses to run on a
        weight set whose marks disagree with that, instead of reading a packed matrix as row-major."""
        from .weights import is_packed
        L0 = self.W.llm_layers[0] if self.W.llm_layers else None
        marked = L0 is not None and is_packed(L0.o_w)
        want = getattr(self.W, "_llm_packed", None)
        if want is not None and any(is_packed(getattr(L, n)) != want for L in self.W.llm_layers for n in ("qkv_w_rope", "o_w", "gu_w", "down_w")
                                    if getattr(L, n) is not None):                # every layer, every linear (128 attribute reads per pass)
            raise RuntimeError("LLM layer weights were replaced by copies that lost their layout mark (weights.mark_packed); "
                               "call engine.pack_llm_weights() / unpack_llm_weights() instead of copying packed tensors")
        return marked

    def pack_llm_weights(self) -> bool:
        """Store the Llama / Mistral layer linears ONCE, in the operand order the decode kernels stream (weights.skinny_pack), in place.
        The prefill GEMM stages its LDS image from that order too (ldw = LMI_LDW_PACKED(K): the packed order is a permutation of the
        16-byte pieces an LDS-DMA lane picks anyway — same image, same MFMA order, same bits, csrc/gemm.h GemmStager), the batch-1 decode
        step runs on lmi_gemm_skinny with one row, and the natural-order duplicate of q|k|v (1.6 GB for Llama-3.1-8B) is dropped:
        16.1 GB of layer weights are resident instead of 17.7 GB + a 15 GB second copy for batched decoding.  Single rank, head_dim 128,
        K % 128 == 0 (the conditions of the batched decode); returns False (and changes nothing) otherwise.  lm_head, embeddings and the
        vision side keep the nn.Linear layout."""
        from .weights import as_packed
        W = self.W
        if self.llm_packed:
            return True
        if not (self.tp_size == 1 and W.llm_layers and all(L.qkv_w_rope is not None for L in W.llm_layers) and self._batch_decode_supported()
                and self.dtype in (torch.float16, torch.bfloat16)):
            return False
        for L in W.llm_layers:
            for name in ("qkv_w_rope", "o_w", "gu_w", "down_w"):
                setattr(L, name, as_packed(getattr(L, name)))
            L.qkv_w = None
        W._llm_packed = True
        self._skinny_pack = None
        self._batch_states = {}                               # steps captured over a second copy of the weights
        return True

    def pack_vit_weights(self, packed: bool = True) -> int:
        """A/B knob (default: not applied): the SigLIP layer linears in the packed order as well — the GEMM's W staging reads 2-KiB-contiguous
        row groups instead of 128-byte row segments 2.3 / 8.7 KiB apart (the effect that made the Llama GEMMs 0.7 % faster).  Same bits.  Returns
        the number of tensors converted.  The fp8 plan and the split-operand copies are built from row-major views either way."""
        from .weights import as_packed, as_row_major, is_packed, packable
        n = 0
        for L in self.W.vit_layers:
            for name in ("qkv_w", "o_w", "fc1_w", "fc2_w"):
                w = getattr(L, name)
                if packed and not is_packed(w) and packable(w) and w.shape[0] % 128 == 0:
                    setattr(L, name, as_packed(w)); n += 1
                elif not packed and is_packed(w):
                    setattr(L, name, as_row_major(w)); n += 1
        if n:
            self._encode_graphs.clear()                       # captured encodes replay the launches of the old layout
        return n

    def unpack_llm_weights(self) -> None:
        """Back to the nn.Linear layout (A/B runs, tools that read the weights)."""
        from .weights import as_row_major
        if not self.llm_packed:
            return
        self.W._llm_packed = None                             # in transition
        for L in self.W.llm_layers:
            L.qkv_w = self._qkv_natural(L)
            for name in ("qkv_w_rope", "o_w", "gu_w", "down_w"):
                setattr(L, name, as_row_major(getattr(L, name)))
        self.W._llm_packed = False
        self._batch_states = {}                               # captured steps hold the packed tensors' launches (batch-1 states re-capture: _decode_run)
        self._head_pack = None

    def _qkv_natural(self, L) -> torch.Tensor:
        """q | k | v projection rows in their natural (checkpoint) order, row-major — kept beside the rope-ordered rows only while the
        weights are unpacked; rebuilt from them otherwise (rope_permute_rows is its own inverse)."""
        if L.qkv_w is not None:
            return L.qkv_w
        from .weights import as_row_major, rope_permute_rows
        (H, KV), hd = self._llm_heads(), self.cfg.text_config.head_dim
        w = as_row_major(L.qkv_w_rope)
        return torch.cat([rope_permute_rows(w[:(H + KV) * hd], hd), w[(H + KV) * hd:]], dim=0).contiguous()

    def _row_parallel(self, a: torch.Tensor, w: torch.Tensor, x: torch.Tensor, tmp: Optional[torch.Tensor]):
        """x += a @ w.T for o_proj / down_proj.  Single rank: fused in the GEMM's fp32 residual epilogue.  Tensor parallel: the
        rank's partial product goes to ``tmp`` (fp32), ONE all-reduce sums it over the ranks (RCCL over xGMI), then it is added."""
        if self.tp_size == 1:
            self.ops.gemm(a, w, x, epilogue=_lib.EPI_RESIDUAL)
            return
        self.ops.gemm(a, w, tmp, epilogue=_lib.EPI_STORE_F32)
        self.comm.all_reduce(tmp)
        x.add_(tmp)

    def _empty(self, *shape, dtype=None):
        return torch.empty(*shape, dtype=dtype or self.dtype, device=self.device)

    def _carve(self, which: str, total: int, offsets, specs):
        """Views into the engine's caller-owned workspace of stage ``which`` ("llm" / "vit"; SURVEY.md 8b: sized by the library's
        lmi_*_workspace_bytes, owned by the caller): ONE uint8 allocation per stage AND LAUNCH STREAM, grown when a larger pass arrives and
        reused by every later one on that stream, carved at the byte offsets the library returned.  specs: [(rows, cols, dtype)] in LMI_WS_*
        order.  Per stream because passes on different HIP streams are not ordered against each other (bench.py --inflight > 1, a graph
        capture beside eager work): they must not share scratch.  A workspace is allocated while its stream is current, so the caching
        allocator's own stream bookkeeping covers its release."""
        if self._private_scratch:
            # warm-up and capture of a vision-encode graph (_encode_images_graph): inside capture the current stream is torch's capture stream,
            # whatever stream the graph is later launched on — a table keyed by it would hand every captured graph the SAME scratch, and
            # replays of two graphs on two launch streams (bench.py --inflight 2 --graph-encode) would race on it.  A graph therefore OWNS its
            # scratch: allocated here, inside the capture, from the graph's private pool; it lives and dies with the graph (round 6, advisor).
            ws = torch.empty(max(total, 256), dtype=torch.uint8, device=self.device)
        else:
            sid = torch.cuda.current_stream(self.device).cuda_stream if self.device.type == "cuda" else 0
            key = (which, sid)
            ws = self._workspaces.get(key)
            if ws is None or ws.numel() < total:
                if ws is None and len(self._workspaces) >= 16:          # streams come and go: bound the table.  An evicted workspace was allocated on
                    self._workspaces.pop(next(iter(self._workspaces)))  # ITS stream and only ever used there, so the allocator's reuse is ordered; no
                ws = self._workspaces[key] = torch.empty(max(total, 256), dtype=torch.uint8, device=self.device)   # graph points into the table
        out = []
        for off, (r, c, dt) in zip(offsets, specs):
            nbytes = r * c * torch.empty(0, dtype=dt).element_size()
            out.append(ws[off:off + nbytes].view(dt).view(r, c))
        return out

    def _pinned_to_device(self, t: torch.Tensor) -> torch.Tensor:
        """Host tensor -> device without blocking the host on the stream (pinned staging + async copy)."""
        if self.device.type != "cuda":
            return t.to(self.device)
        staged = t.pin_memory()
        out = staged.to(self.device, non_blocking=True)
        out._lmi_staging = staged                       # keep the pinned source alive until the copy has run
        return out

    def sequence_geometry(self, seq_lens: Sequence[int]):
        """cu_seqlens / RoPE tables / last-row indices for a tuple of packed sequence lengths (cached: the same
        prompt geometry recurs, and rebuilding would cost a blocking host->device copy per call)."""
        key = tuple(int(l) for l in seq_lens)
        hit = self._geom_cache.get(key)
        if hit is None:
            cu_list = [0]
            for l in key:
                cu_list.append(cu_list[-1] + l)
            cu = torch.tensor(cu_list, dtype=torch.int32, device=self.device)
            pos = torch.cat([torch.arange(l) for l in key])
            cos, sin = self.rope_tables(pos)
            last_rows = torch.tensor([c - 1 for c in cu_list[1:]], device=self.device)
            if len(self._geom_cache) > 64:
                self._geom_cache.clear()
            hit = self._geom_cache[key] = (cu, cos, sin, last_rows, cu_list)
        return hit

    def rope_tables(self, positions: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """cos/sin [S, head_dim/2] fp32 on device (tiny; torch used as plumbing for a table build)."""
        f = positions.to(device=self.device, dtype=torch.float32).reshape(-1, 1) * self._inv_freq.reshape(1, -1)
        return f.cos().contiguous(), f.sin().contiguous()

    # ------------------------------------------------------------------------------------------------
    # a5 + a7: vision tower
    # ------------------------------------------------------------------------------------------------
    def lo4_vit_tiles(self, tiles_per_sample: Sequence[int], seq_lens: Sequence[int]) -> Optional[Tuple[bool, ...]]:
        """Per ViT input: does the lo4 schedule correct the SigLIP layer linears for it (``lo4_vit``: True / False / "auto" = the inputs of the
        samples whose LLM sequence has at most LO4_FULL_BELOW rows)?  None = no input is corrected (the fast tower)."""
        if not self.lo4 or self.lo4_vit is False:
            return None
        flags: List[bool] = []
        for n, S in zip(tiles_per_sample, seq_lens):
            flags += [bool(self.lo4_vit is True or int(S) <= self.LO4_FULL_BELOW)] * int(n)
        return tuple(flags) if any(flags) else None

    def vision_tower(self, tiles: torch.Tensor, lo4_tiles: Optional[Sequence[bool]] = None) -> torch.Tensor:
        """tiles: u8 [N,S,S,3] (HWC) or fp32 pixel_values [N,3,S,S].  Returns post-LN features T [N*T, D].  ``lo4_tiles``: per ViT input, whether
        the lo4 schedule corrects the tower's linears for it (lo4_vit_tiles; None = none)."""
        ops, W, vc = self.ops, self.W, self.cfg.vision_config
        n = tiles.shape[0]
        T, D = vc.num_patches, vc.hidden_size
        M = n * T
        x = self._empty(M, D, dtype=torch.float32)
        # normalise + im2col + patch conv + bias + position embedding: one launch, no im2col matrix in HBM (lmi_patch_embed)
        ops.patch_embed(tiles, W.patch_w_fused, W.patch_b, W.pos_emb, x, vc.image_size, vc.patch_size)
        if n not in self._vit_cu_cache:          # cu_seqlens of the layers' attention: one T-token sequence per ViT input
            self._vit_cu_cache[n] = torch.arange(0, (n + 1) * T, T, dtype=torch.int32, device=self.device)
        if self.trace:
            self.trace("vit.embed", x)
        if self.fp8 is not None:
            self._vit_layers_fp8(x, n)
        elif self.split_operands:
            self._vit_layers_split(x, n)
        elif self.lo4 and lo4_tiles is not None and any(lo4_tiles):
            self._vit_layers(x, self._vit_cu_cache[n], T, self._vit_operands_lo4(M, lo4_tiles), self._lo4_weights("vit"), trace=self.trace)
        else:
            self._vit_layers(x, self._vit_cu_cache[n], T, self._vit_operands_fast(M), rec=self._rec, trace=self.trace)
        out = self._empty(M, D)                 # a result, not scratch: the caller may hold it across later passes that reuse the workspace
        ops.layernorm(x, W.post_ln_w, W.post_ln_b, out, vc.layer_norm_eps)
        return out

    def _vit_operands_fast(self, M: int):
        """(h, qkv, att, ff) of the fast SigLIP layers: 16-bit tensors on the caller-owned workspace."""
        W, D = self.W, self.cfg.vision_config.hidden_size
        qkv_w = W.vit_layers[0].qkv_w.shape[0] if W.vit_layers else 3 * D
        total, offs = self.ops.vit_workspace(M, D, qkv_w, W.vit_ff, self.dtype)
        return self._carve("vit", total, offs, [(M, D, self.dtype), (M, qkv_w, self.dtype), (M, D, self.dtype), (M, W.vit_ff, self.dtype)])

    def _vit_layers(self, x: torch.Tensor, cu: torch.Tensor, max_len: int, operands, w4s=None, rec=None, trace=None) -> None:
        """The SigLIP layers of the fast and of the lo4 schedule over the packed sequences ``cu``; like its siblings below, updates the fp32
        stream ``x`` in place.  ``operands`` = (h, qkv, att, ff) choose the schedule (ops.linear): 16-bit tensors = fast, one rounding per
        operand hand-over; h / att / ff as Lo4Acts with ``w4s`` (_lo4_weights("vit")) = the low-bit correction phase: the LayerNorms and fc1's
        GELU epilogue hand over T(y) + the fp4 image of y - T(y) directly, and so does the attention kernel (lmi_attn_varlen_fwd_lo4: every
        head padded to 96 slots in the image, out_proj's weight image laid out to match).  q / k / v and the attention arithmetic stay 16-bit.
        ``rec`` / ``trace``: the calibration and trace hooks of the caller, if it has any."""
        ops, W, vc = self.ops, self.W, self.cfg.vision_config
        D, H, hd = vc.hidden_size, vc.num_attention_heads, vc.head_dim
        h, qkv, att, ff = operands
        scale = hd ** -0.5
        for li, (L, (qkv4, o4, fc14, fc24)) in enumerate(zip(W.vit_layers, w4s or [(None,) * 4] * len(W.vit_layers))):
            ops.norm(x, L.ln1_w, L.ln1_b, h, vc.layer_norm_eps)
            rec and rec(("vit", li, "h1"), h)
            ops.linear(h, L.qkv_w, qkv, qkv4, bias=L.qkv_b)
            ops.attend(qkv[:, 0:D], qkv[:, D:2 * D], qkv[:, 2 * D:3 * D], att, cu, cu, max_len, H, H, hd, scale, False, self.use_tr)
            rec and rec(("vit", li, "att"), att)
            ops.linear(att, L.o_w, x, o4, bias=L.o_b, epilogue=_lib.EPI_RESIDUAL)
            ops.norm(x, L.ln2_w, L.ln2_b, h, vc.layer_norm_eps)
            rec and rec(("vit", li, "h2"), h)
            ops.linear(h, L.fc1_w, ff, fc14, bias=L.fc1_b, act=_lib.ACT_GELU_TANH)
            rec and rec(("vit", li, "ff"), ff)
            ops.linear(ff, L.fc2_w, x, fc24, bias=L.fc2_b, epilogue=_lib.EPI_RESIDUAL)
            if trace:
                trace(f"vit.{li}", x)

    def _vit_layers_fp8(self, x: torch.Tensor, n: int) -> None:
        """The SigLIP layers with fp8 linears (leopard_amd.fp8): LayerNorm -> fp8 operand in one launch, fc1's GELU epilogue
        writes fc2's fp8 operand; q|k|v and the attention stay 16-bit, the residual stream fp32."""
        ops, W, vc, P = self.ops, self.W, self.cfg.vision_config, self.fp8
        T, D, H, hd = vc.num_patches, vc.hidden_size, vc.num_attention_heads, vc.head_dim
        M = n * T
        u8 = torch.uint8
        h8 = self._empty(M, D, dtype=u8)
        att8 = self._empty(M, D, dtype=u8)
        ff8 = self._empty(M, W.vit_ff, dtype=u8)
        qkv = self._empty(M, W.vit_layers[0].qkv_w.shape[0])
        att = self._empty(M, D)
        cu = self._vit_cu_cache[n]
        scale = hd ** -0.5
        fused = self.fp8_fused and self.use_tr          # (the fp8-output attention lives in the LDS-DMA kernel, the production one)
        for li, (L, Q) in enumerate(zip(W.vit_layers, P.vit)):
            ops.norm_fp8(x, L.ln1_w, L.ln1_b, h8, vc.layer_norm_eps, 2.0 ** Q.act["h1"])
            ops.gemm_fp8(h8, Q.lin["qkv"].w8, qkv, bias=L.qkv_b, scale_exp=Q.out_exp("h1", "qkv"))
            if fused:
                ops.attention_fp8out(qkv[:, 0:D], qkv[:, D:2 * D], qkv[:, 2 * D:3 * D], att8, 2.0 ** Q.act["att"], cu, cu, T, H, H, hd, scale, False)
            else:
                ops.attention(qkv[:, 0:D], qkv[:, D:2 * D], qkv[:, 2 * D:3 * D], att, cu, cu, T, H, H, hd, scale, False,
                              self.use_tr)
                ops.quantize_fp8(att, att8, 2.0 ** Q.act["att"])
            ops.gemm_fp8(att8, Q.lin["o"].w8, x, bias=L.o_b, epilogue=_lib.EPI_RESIDUAL, scale_exp=Q.out_exp("att", "o"))
            ops.norm_fp8(x, L.ln2_w, L.ln2_b, h8, vc.layer_norm_eps, 2.0 ** Q.act["h2"])
            ops.gemm_fp8(h8, Q.lin["fc1"].w8, ff8, bias=L.fc1_b, act=_lib.ACT_GELU_TANH, scale_exp=Q.out_exp("h2", "fc1"),
                         out_scale=2.0 ** Q.act["ff"])
            ops.gemm_fp8(ff8, Q.lin["fc2"].w8, x, bias=L.fc2_b, epilogue=_lib.EPI_RESIDUAL, scale_exp=Q.out_exp("ff", "fc2"))
            if self.trace:
                self.trace(f"vit.{li}", x)

    # ---- split-operand precision mode -------------------------------------------------------------------------------------------
    def _split_weights(self):
        """[W | W] copies of the layer-linear weights (K doubled), built on first use: +0.8 GB (SigLIP) + 14 GB (Llama-3.1-8B)."""
        sw = self._split_w
        if sw is None:
            from .weights import as_row_major
            dup = lambda w: (lambda r: torch.cat([r, r], dim=1).contiguous())(as_row_major(w))
            W = self.W
            sw = self._split_w = {
                "vit": [(dup(L.qkv_w), dup(L.o_w), dup(L.fc1_w), dup(L.fc2_w)) for L in W.vit_layers],
                "llm": [(dup(L.qkv_w_rope if L.qkv_w_rope is not None else L.qkv_w), dup(L.o_w), dup(L.gu_w), dup(L.down_w)) for L in W.llm_layers]}
        return sw

    def _vit_layers_split(self, x: torch.Tensor, n: int) -> None:
        """The SigLIP layers with split (hi + lo) A operands: LayerNorm -> fp32 -> [hi | lo]; attention output and GELU output in fp32 ->
        [hi | lo]; every linear at 2 K against [W | W].  q / k / v and the attention arithmetic stay 16-bit."""
        ops, W, vc = self.ops, self.W, self.cfg.vision_config
        T, D, H, hd = vc.num_patches, vc.hidden_size, vc.num_attention_heads, vc.head_dim
        M = n * T
        f32 = torch.float32
        h32, h2 = self._empty(M, D, dtype=f32), self._empty(M, 2 * D)
        qkv = self._empty(M, W.vit_layers[0].qkv_w.shape[0])
        ff32, ff2 = self._empty(M, W.vit_ff, dtype=f32), self._empty(M, 2 * W.vit_ff)
        cu = self._vit_cu_cache[n]
        scale = hd ** -0.5
        for li, (L, (qkv_w2, o_w2, fc1_w2, fc2_w2)) in enumerate(zip(W.vit_layers, self._split_weights()["vit"])):
            ops.layernorm(x, L.ln1_w, L.ln1_b, h32, vc.layer_norm_eps)
            ops.split_hi_lo(h32, h2)
            ops.gemm(h2, qkv_w2, qkv, bias=L.qkv_b)
            ops.attention_f32out(qkv[:, 0:D], qkv[:, D:2 * D], qkv[:, 2 * D:3 * D], h32, cu, cu, T, H, H, hd, scale, False)
            ops.split_hi_lo(h32, h2)
            ops.gemm(h2, o_w2, x, bias=L.o_b, epilogue=_lib.EPI_RESIDUAL)
            ops.layernorm(x, L.ln2_w, L.ln2_b, h32, vc.layer_norm_eps)
            ops.split_hi_lo(h32, h2)
            ops.gemm(h2, fc1_w2, ff32, bias=L.fc1_b, act=_lib.ACT_GELU_TANH, epilogue=_lib.EPI_STORE_F32)
            ops.split_hi_lo(ff32, ff2)
            ops.gemm(ff2, fc2_w2, x, bias=L.fc2_b, epilogue=_lib.EPI_RESIDUAL)
            if self.trace:
                self.trace(f"vit.{li}", x)

    def _llm_layers_split(self, x, cache, cu, cos, sin, max_len):
        """The Llama / Mistral layers with split (hi + lo) A operands (see _vit_layers_split); q|k|v + RoPE + KV append stay one launch
        (lmi_rmsnorm_rope on the 2 K operand), the attention hands over fp32."""
        ops, W, tc = self.ops, self.W, self.cfg.text_config
        S, D = x.shape
        (H, KV), hd = self._llm_heads(), tc.head_dim
        qw, kw = H * hd, KV * hd
        f32 = torch.float32
        h32, h2 = self._empty(S, D, dtype=f32), self._empty(S, 2 * D)
        a32, a2 = (h32, h2) if qw == D else (self._empty(S, qw, dtype=f32), self._empty(S, 2 * qw))
        qkv = self._empty(S, qw + 2 * kw)
        gu32, gu2 = self._empty(S, W.llm_ff, dtype=f32), self._empty(S, 2 * W.llm_ff)
        scale = hd ** -0.5
        for i, (L, (qkv_w2, o_w2, gu_w2, down_w2)) in enumerate(zip(W.llm_layers, self._split_weights()["llm"])):
            ops.rmsnorm(x, L.in_norm, h32, tc.rms_norm_eps)
            ops.split_hi_lo(h32, h2)
            if L.qkv_w_rope is not None and hd == 128:
                ops.rmsnorm_rope(h2, qkv_w2, qkv, None, tc.rms_norm_eps, cos, sin, cache.k[i] if cache else None, cache.v[i] if cache else None,
                                 0, H, KV, hd)
            else:
                ops.gemm(h2, qkv_w2, qkv)
                ops.rope_qk(qkv, H, KV, hd, cos, sin, cache.k[i] if cache else None, cache.v[i] if cache else None, 0)
            ops.attention_f32out(qkv[:, :qw], qkv[:, qw:qw + kw], qkv[:, qw + kw:], a32, cu, cu, max_len, H, KV, hd, scale, True,
                                 window=tc.sliding_window or 0)
            ops.split_hi_lo(a32, a2)
            ops.gemm(a2, o_w2, x, epilogue=_lib.EPI_RESIDUAL)
            ops.rmsnorm(x, L.post_norm, h32, tc.rms_norm_eps)
            ops.split_hi_lo(h32, h2)
            ops.gemm(h2, gu_w2, gu32, epilogue=_lib.EPI_SWIGLU_F32)
            ops.split_hi_lo(gu32, gu2)
            ops.gemm(gu2, down_w2, x, epilogue=_lib.EPI_RESIDUAL)
            if self.trace:
                self.trace(f"llm.{i}", x)

    # ---- low-bit correction mode --------------------------------------------------------------------------------------------------------
    LO4_FULL_BELOW = 1024              # "auto": sequences up to this length carry the correction on every row ...
    LO4_TAIL_ROWS = 16                 # ... longer ones on their last LO4_TAIL_ROWS rows: the row whose logits are read + a margin of 15 (tools/lo4_policy_study.py,
                                       # profiles/r06_lo4_policy_study_*.txt; on the device the last 1 / 16 / 64 / 256 / 1024 rows and every row all land at 2.4 - 2.8e-4 on
                                       # C3 and 3.7 - 4.1e-4 on C2).  16 rows sit in ONE 256-row tile 15 times out of 16, so one row tile per sequence runs the fp4 k-tiles;
                                       # 256 rows always straddled two (C2: 32.7 -> 31.6 ms, C3: 137.4 -> 137.0 ms on one box, profiles/r06_lo4_tail_rows_ab.txt)

    def _lo4_weights(self, tower: str = "llm"):
        """fp4 images (+ one E8M0 scale per row) of one tower's layer-linear weights, built from the row-major order of each weight when the
        mode is selected (or on first use): + 0.5 B per parameter (3.5 GB Llama-3.1-8B; 0.2 GB SigLIP, only with ``lo4_vit``)."""
        lw = self._lo4_w.get(tower)
        if lw is None:
            from .weights import as_row_major
            q = lambda w, head_pad=None: self.ops.quantize_w4(as_row_major(w).contiguous(), head_pad=head_pad)
            W, vc = self.W, self.cfg.vision_config
            if tower == "vit":
                vhp = (vc.num_attention_heads, vc.head_dim)      # out_proj's image in the per-head padded k order of the attention's residual image
                lw = [(q(L.qkv_w), q(L.o_w, vhp), q(L.fc1_w), q(L.fc2_w)) for L in W.vit_layers]
            else:
                lw = [(q(L.qkv_w_rope if L.qkv_w_rope is not None else L.qkv_w), q(L.o_w), q(L.gu_w), q(L.down_w)) for L in W.llm_layers]
            self._lo4_w[tower] = lw
        return lw

    def invalidate_lo4_weights(self) -> None:
        """Drop the fp4 weight images: call after replacing or changing the VALUES of layer weights (the images are a function of the values; a
        change of layout — pack / unpack — keeps them valid)."""
        self._lo4_w = {}

    def lo4_tail_rows(self, seq_len: int) -> int:
        """How many trailing rows of a ``seq_len``-row sequence carry the correction under ``lo4_rows``."""
        r = self.lo4_rows
        if r == "all":
            return seq_len
        if r == "auto":
            return seq_len if seq_len <= self.LO4_FULL_BELOW else min(self.LO4_TAIL_ROWS, seq_len)
        return max(1, min(int(r), seq_len))

    def _selection_tables(self, row: np.ndarray, pinned: bool):
        """uint8 row mask [S] -> (row_sel [S], unit_sel [ceil(S / 64)]) device tensors + the host [n, 2] int32 array of the selected row
        ranges (the maximal runs of ones: the tile-order hint of lmi_lo4.sel_ranges).  ``pinned``: staged through pinned memory and copied
        asynchronously (tables cached per geometry and read on whatever stream the pass runs); otherwise a synchronous copy, ready before
        any stream reads them (tables cached per launch stream)."""
        S = len(row)
        unit = np.zeros((S + 63) // 64 * 64, dtype=np.uint8)
        unit[:S] = row
        unit = unit.reshape(-1, 64).max(axis=1)
        ranges = np.flatnonzero(np.diff(np.concatenate([[0], row.astype(np.int8), [0]]))).reshape(-1, 2)
        to_device = self._pinned_to_device if pinned else (lambda t: t.to(self.device))
        return to_device(torch.from_numpy(row)), to_device(torch.from_numpy(unit)), np.ascontiguousarray(ranges.astype(np.int32))

    def _lo4_selection(self, seq_lens: Sequence[int], extra_rows: Optional[np.ndarray] = None):
        """(row_sel uint8 [S], unit_sel uint8 [ceil(S / 64)]) device tensors + the host [n, 2] int32 array of the selected row ranges (the
        tile-order hint of lmi_lo4.sel_ranges) for the packed rows of ``seq_lens``, or None when every row is selected.  ``extra_rows``:
        packed rows whose logits are read besides the tails (the scored rows of score / score_batch): selected as well."""
        lens = tuple(int(l) for l in seq_lens)
        tails = tuple(self.lo4_tail_rows(l) for l in lens)
        if tails == lens:
            return None
        if extra_rows is not None and len(extra_rows):
            # the tails united with the scored rows.  The tables are built with a synchronous copy (ready before any stream reads them) and
            # cached per launch stream, under a key that holds the extra rows themselves
            extra = np.asarray(extra_rows, dtype=np.int64)
            sid = torch.cuda.current_stream(self.device).cuda_stream if self.device.type == "cuda" else 0
            cache, bound, key = self._score_sel_cache, 16, (sid, lens, tails, extra.tobytes())
        else:
            extra = None
            cache, bound, key = self._lo4_sel_cache, 64, (lens, tails)
        hit = cache.get(key)
        if hit is None:
            row = np.zeros(sum(lens), dtype=np.uint8)
            end = 0
            for l, t in zip(lens, tails):
                end += l
                row[end - t:end] = 1
            if extra is not None:
                row[extra] = 1
                if row.all():
                    return None
            if len(cache) >= bound:
                cache.pop(next(iter(cache)))
            hit = cache[key] = self._selection_tables(row, pinned=extra is None)
        return hit

    def _lo4_act(self, rows: int, width: int, heads: Optional[tuple] = None, sel: Optional[tuple] = None):
        """Operand pair buffers; ``heads`` = (n_heads, head_dim): an attention output (image in the per-head padded k order); ``sel``: the row
        selection of the pass (_lo4_selection) — the images then start out zero and only selected rows are ever written."""
        from .ops import Lo4Act, lo4_head_k4
        return Lo4Act.empty(rows, width, self.dtype, self.device, k4=lo4_head_k4(*heads) if heads else None, sel=sel)

    def _vit_operands_lo4(self, M: int, flags: Optional[Sequence[bool]] = None):
        """(h, qkv, att, ff) of the SigLIP layers with the low-bit correction phase (_vit_layers): h / att / ff as operand pairs.  ``flags``:
        per ViT input of the tile tower, whether it is corrected (None = every row)."""
        W, vc = self.W, self.cfg.vision_config
        D, H, hd = vc.hidden_size, vc.num_attention_heads, vc.head_dim
        # (a packed batch whose samples differ: the row selection of the correction phase carries the per-input decision — every row of a selected
        # ViT input, none of the others: _lo4_selection with "sequences" = the inputs)
        sel = None
        if flags is not None and not all(flags):
            key = ("vit", tuple(bool(f) for f in flags))
            sel = self._lo4_sel_cache.get(key)
            if sel is None:
                sel = self._lo4_sel_cache[key] = self._selection_tables(np.repeat(np.array(flags, dtype=np.uint8), vc.num_patches), pinned=True)
        h, att, ff = self._lo4_act(M, D, sel=sel), self._lo4_act(M, D, heads=(H, hd), sel=sel), self._lo4_act(M, W.vit_ff, sel=sel)
        return h, self._empty(M, W.vit_layers[0].qkv_w.shape[0]), att, ff

    def enable_fp8(self, calibration_samples, headroom: float = 2.0):
        """Switch the ViT / LLM layer linears to fp8 operands (BASELINE configs[4]): quantise the weights once, take the static
        activation scales from a 16-bit prefill of ``calibration_samples`` [(input_ids, tiles)].  ``engine.fp8 = None`` reverts."""
        from . import fp8 as F8
        self.fp8 = F8.calibrate(self, calibration_samples, headroom)
        return self.fp8

    # ------------------------------------------------------------------------------------------------
    # a8 + a9: pixel shuffle + projector
    # ------------------------------------------------------------------------------------------------
    def project(self, vit_out: torch.Tensor, n_tiles: int) -> torch.Tensor:
        """T [N*T, Dv] -> visual tokens fp32 [N*T/4, Dt] (pixel shuffle folded into linear_1's A gather)."""
        ops, W, cfg = self.ops, self.W, self.cfg
        rows = n_tiles * cfg.tokens_per_tile
        Dt = cfg.text_config.hidden_size
        h1 = self._empty(rows, Dt)
        ops.gemm(vit_out, W.proj1_w, h1, bias=W.proj1_b, act=_lib.ACT_GELU_ERF, a_mode=_lib.A_PIXEL_SHUFFLE,
                 ps_grid=cfg.vision_config.grid, M=rows)
        vis = self._empty(rows, Dt, dtype=torch.float32)
        ops.gemm(h1, W.proj2_w, vis, bias=W.proj2_b, epilogue=_lib.EPI_STORE_F32)
        return vis

    def _warm_up(self, body, restore: Sequence[torch.Tensor] = ()) -> List[torch.Tensor]:
        """First half of a graph capture: ``body`` runs once outside capture (first-use attribute calls, allocator) on a side stream that
        waits on the current one, then the device counters ``restore`` get their values back.  Returns those values for ``_capture``."""
        keep = [t.clone() for t in restore]
        cur = torch.cuda.current_stream(self.device)
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            body()
        cur.wait_stream(side)
        for t, v in zip(restore, keep):
            t.copy_(v)
        return keep

    def _capture(self, body, restore: Sequence[torch.Tensor] = (), keep: Sequence[torch.Tensor] = ()):
        """Second half: ``body`` captured into a HIP graph; ``restore`` is put back to ``keep`` afterwards as well (capture does not execute).
        Returns (graph, what the captured call of the body returned).  ``body`` is called as given, so a caller that wants a method looked
        up when the step runs passes a lambda."""
        g = torch.cuda.CUDAGraph()
        with _capture_safe(), torch.cuda.graph(g):
            out = body()
        for t, v in zip(restore, keep):
            t.copy_(v)
        return g, out

    def _capture_graph(self, body, restore: Sequence[torch.Tensor] = ()):
        """Warm up and capture ``body`` (two calls of it), leaving the device tensors ``restore`` as they were."""
        return self._capture(body, restore, self._warm_up(body, restore))

    def encode_images(self, tiles: torch.Tensor, lo4_tiles: Optional[Sequence[bool]] = None) -> torch.Tensor:
        if self.graph_encode and self.device.type == "cuda" and not self.ops.emulated and tiles.dtype == torch.uint8:
            return self._encode_images_graph(tiles, lo4_tiles)
        return self.project(self.vision_tower(tiles, lo4_tiles), tiles.shape[0])

    def _encode_images_graph(self, tiles: torch.Tensor, lo4_tiles: Optional[Sequence[bool]] = None) -> torch.Tensor:
        """BASELINE config 5 ("hipGraph-captured encode"): the vision tower + projector for N ViT inputs is ~200 launches whose
        shapes depend on N only, so they are captured ONCE per N into a HIP graph over static buffers (u8 tiles in, fp32 visual
        tokens out) and replayed: one graph launch instead of ~200 stream launches, no per-launch host work.  Results are those
        of the eager path bit for bit (same kernels, same order).  The returned tensor is the graph's static output buffer:
        it is overwritten by the next encode of the same N (callers here consume it immediately in embed_merge)."""
        n = tiles.shape[0]
        # one graph + static buffers per (N, launch stream): replays of one graph from two streams (bench.py --inflight > 1) would
        # share the static buffers with nothing ordering them
        key = (n, torch.cuda.current_stream(self.device).cuda_stream, None if lo4_tiles is None else tuple(bool(f) for f in lo4_tiles))
        ent = self._encode_graphs.get(key)
        if ent is None:
            static_in = torch.empty_like(tiles)
            static_in.copy_(tiles)
            self._private_scratch = True                                       # the graph owns its tower scratch (see _carve)
            try:
                g, static_out = self._capture_graph(lambda: self.project(self.vision_tower(static_in, lo4_tiles), n))
            finally:
                self._private_scratch = False
            if len(self._encode_graphs) >= 8:                                  # a handful of distinct N per workload; bound the pools
                self._encode_graphs.pop(next(iter(self._encode_graphs)))
            ent = self._encode_graphs[key] = (g, static_in, static_out)
        g, static_in, static_out = ent
        static_in.copy_(tiles)
        g.replay()
        return static_out

    # ------------------------------------------------------------------------------------------------
    # a10: embedding gather + merge
    # ------------------------------------------------------------------------------------------------
    def embed_merge(self, input_ids: torch.Tensor, visual_tokens: Optional[torch.Tensor]) -> torch.Tensor:
        cfg = self.cfg
        # the index map is planned on the host from the token ids; ids that are already host-side (the tokenizer's
        # output, EVAL:443) cost no device sync at all
        ids_host_t = input_ids.detach().reshape(-1).to("cpu", torch.int64)
        n_rows = 0 if visual_tokens is None else visual_tokens.shape[0]
        src = plan_merge(ids_host_t.numpy(), cfg.image_token_index, n_rows, cfg.tokens_per_tile)
        if input_ids.device == self.device:
            ids_dev = input_ids.reshape(-1).to(torch.int64).contiguous()
        else:
            ids_dev = self._pinned_to_device(ids_host_t.contiguous())
        src_dev = self._pinned_to_device(torch.from_numpy(src))
        x = self._empty(len(src), cfg.text_config.hidden_size, dtype=torch.float32)
        self.ops.embed_merge(ids_dev, src_dev, self.W.embed, visual_tokens, x)
        return x

    # ------------------------------------------------------------------------------------------------
    # a11: LLM prefill over one or several packed causal sequences
    # ------------------------------------------------------------------------------------------------
    def llm_prefill(self, x: torch.Tensor, seq_lens: Sequence[int], cache: Optional[KVCache] = None,
                    all_logits: bool = False, score_rows: Optional[np.ndarray] = None):
        """x: fp32 [sum(seq_lens), D] residual stream (updated in place).  Returns (logits_last [n_seq, V],
        logits_all or None).  ``cache`` (single sequence only) receives rotated K and V.  ``score_rows`` (score / score_batch): the packed
        rows whose logits are read — the lo4 schedule corrects them as well — and no head runs here: returns (None, None).
        One sequence whose last-row logits are all that is read (``last_layer_rows`` = "read"): the last layer updates only a trailing window
        of ``x``; the rows before it keep that layer's input."""
        S = x.shape[0]
        cu, cos, sin, last_rows, cu_list = self.sequence_geometry(seq_lens)
        assert cu_list[-1] == S
        self.llm_packed                                   # raises when a packed weight was replaced by a copy without its layout mark
        if cache is not None:       # one sequence, or a pool holding the packed rows of several (generate_batch splits it afterwards)
            assert cache.length == 0 and cache.capacity >= S
        max_len = max(int(l) for l in seq_lens)
        self.last_lo4_ranges = None
        # nothing but the last row's logits (and the KV cache) leaves this call: the last layer may skip the other rows (_last_layer_window)
        last_only = (self.last_layer_rows == "read" and len(seq_lens) == 1 and not all_logits and score_rows is None and self.trace is None
                     and self._rec is None)
        if self.trace:
            self.trace("llm.embed", x)
        if self.fp8 is not None:
            self._llm_layers_fp8(x, cache, cu, cos, sin, max_len, seq_lens)
        elif self.split_operands and self.tp_size == 1 and not self.lo4:
            self._llm_layers_split(x, cache, cu, cos, sin, max_len)
        else:
            self._llm_layers(x, cache, cu, cos, sin, max_len, seq_lens, all_rows=all_logits, extra_rows=score_rows, last_only=last_only)
        if cache is not None:
            cache.length = S
        return (None, None) if score_rows is not None else self._lm_head(x, last_rows, all_logits)

    def _attend(self, i, qkv, att, cu, max_len, cache, prefix, cu_k, window=None, rows_att=None):
        """The attention launch of layer i over the packed q|k|v rows.  ``att``: the 16-bit output rows, or the Lo4Act of the lo4 schedule.
        Default: causal self-attention of the packed sequences.  ``prefix`` (extend): every sequence's keys are [the P cached rows of
        ``prefix`` ; its own rows] — the two-range launch, the prefix read in place.  ``cu_k`` (append): the keys are the rows of ``cache``
        itself, which the q|k|v epilogue has just extended.  ``window`` = (w0, cu_w) (_last_layer_window; one sequence): the queries are
        the rows w0.. of ``qkv`` (``att``: their output rows), the keys every row — cu_q = cu_w != cu_k = cu, bottom-right causal.
        ``rows_att`` (with ``prefix``; _rows_attention): the row-packed launch instead of the two-range one — under lo4 its merge also hands
        over the fp32 rows and lmi_split_lo4 makes T(o) and the residual image of them (every row selected: _rows_attention_guard)."""
        from .ops import Lo4Act
        ops, tc = self.ops, self.cfg.text_config
        (H, KV), hd = self._llm_heads(), tc.head_dim
        qw, kw = H * hd, KV * hd
        q, k, v = qkv[:, :qw], qkv[:, qw:qw + kw], qkv[:, qw + kw:]
        if prefix is not None:
            assert window is None
            P = prefix.length
            if rows_att is not None:
                k_begin, k_len, max_k, ws, o32 = rows_att
                pair = isinstance(att, Lo4Act)
                assert not pair or att.row_sel is None
                ops.attention_prefix_rows(q, prefix.k[i][:P], prefix.v[i][:P], P, k, v, att.hi if pair else att, k_begin, k_len, max_k, H, KV, hd,
                                          hd ** -0.5, ws, out_f32=o32 if pair else None)
                if pair:
                    ops.split_lo4(o32, att)
                return
            ops.attend_prefix(q, k, v, prefix.k[i][:P], prefix.v[i][:P], P, att, cu, max_len, H, KV, hd, hd ** -0.5)
            return
        # (queries, cu_seqlens_q, cu_seqlens_k, longest query sequence) per mode; k / v: the packed rows, or the cache (append)
        if window is not None:
            assert cu_k is None
            w0, cu_w = window
            q, cu_q, cu_keys, max_q = q[w0:], cu_w, cu, max_len - w0
        elif cu_k is not None:
            k, v = cache.k[i], cache.v[i]
            cu_q, cu_keys, max_q = cu, cu_k, max_len
        else:
            cu_q, cu_keys, max_q = cu, cu, max_len
        ops.attend(q, k, v, att, cu_q, cu_keys, max_q, H, KV, hd, hd ** -0.5, True, self.use_tr, window=tc.sliding_window or 0)

    def _last_layer_window(self, S: int, first_needed: int):
        """(w0, cu_w) of the trailing row window [w0, S) the last layer of a one-sequence prefill runs on after its k | v projection, or None
        when that is the whole sequence.  ``first_needed``: the first row that must be in it (the read row; under lo4 the first selected
        row).  w0 is a multiple of ATT_BQ = 128 rows from the sequence start: the attention decides its deferred rescale per 32-row wave of a
        128-row query block, so a row's bits depend on its wave-mates — an aligned window keeps the blocks of the full launch — and the
        64-row units of the lo4 selection can be sliced.  cu_w: the window's cu_seqlens_q (cached: building one is a host-to-device copy)."""
        w0 = min(int(first_needed), S - 1) // 128 * 128
        if w0 <= 0:
            return None
        cu_w = self._window_cu.get((S, w0))
        if cu_w is None:
            if len(self._window_cu) >= 64:                       # one entry per sequence length served: bounded, oldest out first
                self._window_cu.pop(next(iter(self._window_cu)))
            cu_w = self._window_cu[(S, w0)] = torch.tensor([0, S - w0], dtype=torch.int32, device=self.device)
        return w0, cu_w

    def _window_selection(self, sel: tuple, w0: int) -> tuple:
        """The selection tables of _lo4_selection for the rows w0.. (w0 % 64 == 0; every selected row at or after w0): row_sel / unit_sel
        views and the host ranges relative to w0.  Cached beside the tables they are cut from (which the views keep alive)."""
        key = (sel[0].data_ptr(), w0)
        hit = self._window_sel.get(key)
        if hit is None:
            if len(self._window_sel) >= 64:
                self._window_sel.pop(next(iter(self._window_sel)))
            hit = self._window_sel[key] = (sel[0][w0:], sel[1][w0 // 64:], np.ascontiguousarray(sel[2] - w0, dtype=np.int32))
        return hit

    @staticmethod
    def _qkv_weight_parts(w_rope: torch.Tensor, q_rows: int):
        """(q rows, k | v rows) of a rope-ordered q|k|v weight as views: row slices of the nn.Linear layout, and of the packed order too (its
        16-row groups are contiguous; the layout mark is a property of the tensor object, so the views get their own)."""
        from .weights import is_packed, mark_packed
        wq, wkv = w_rope[:q_rows], w_rope[q_rows:]
        if is_packed(w_rope):
            assert q_rows % 16 == 0
            mark_packed(wq), mark_packed(wkv)
        return wq, wkv

    def _llm_layers(self, x, cache, cu, cos, sin, max_len, seq_lens=None, all_rows=False, extra_rows=None, prefix=None, cache_pos0=0,
                    cu_k=None, last_only=False, rows_att=None):
        """The Llama / Mistral layers of the fast and of the lo4 schedule: the buffers, the row selection and the weight images are set up per
        schedule, then ONE layer body serves both — the operands choose the entries (ops.linear; fast: 16-bit tensors on the caller-owned
        workspace, lo4: Lo4Acts).  That body is the FUSED schedule: the RMSNorms ride in the GEMM epilogues (under lo4 the producers o_proj /
        down_proj also write the fp4 image of the residual of T(x gamma)), q|k|v + RoPE + KV append is one launch, gate/up's SwiGLU epilogue
        writes down_proj's operand (pair), the attention kernel o_proj's: lo4 adds no launch to the fast schedule.  Where the shapes do not
        allow the fusion the fast schedule runs launch by launch (_llm_layers_unfused); lo4 needs it.
        ``prefix`` / ``cache_pos0`` / ``cu_k`` / ``rows_att``: continuing from cached rows (extend / append; _attend).  ``last_only`` (llm_prefill; fused
        schedule): only the last row of the one sequence is read afterwards — the last layer projects k | v for every row (the cache needs
        them) and runs q, the attention, o_proj, gate/up and down_proj on the rows of _last_layer_window alone; under lo4 the window also
        holds every selected row, so the selection tables are sliced with the rows.  ``seq_lens`` / ``all_rows`` / ``extra_rows``: what
        the lo4 row selection is made from (below)."""
        from .ops import Lo4Weight, rows_from
        ops, W, tc = self.ops, self.W, self.cfg.text_config
        S, D = x.shape
        (H, KV), hd = self._llm_heads(), tc.head_dim
        qw, kw = H * hd, KV * hd
        parts = (D + 63) // 64
        lo4 = self.lo4 and self.tp_size == 1
        # Fused schedule (one rank, head_dim 128): the RMSNorms and the RoPE ride in the GEMM epilogues.  Each residual GEMM
        # (o_proj, down_proj) also emits T(x * gamma_next) and per-row partial sums of squares; the GEMM that consumes them
        # (gate/up, next layer's qkv) applies rstd to its accumulator rows; the qkv GEMM rotates q / k and appends K / V to the
        # cache in its epilogue.  Only the very first norm of the stack is a launch of its own.
        fused = (self.tp_size == 1 and hd == 128 and D % 256 == 0 and W.llm_layers and W.llm_layers[0].qkv_w_rope is not None)
        first_needed = S - 1                                         # first row the last layer's window must hold: the read row ...
        if lo4:
            if not fused:
                raise RuntimeError("precision 'lo4' needs head_dim 128 and the rope-ordered q|k|v weights (the fused Llama / Mistral schedule)")
            # row selection (lo4_rows): only the trailing rows of each sequence hand over residual images; the other rows' images stay zero and the
            # tiles without a selected row skip the fp4 k-tiles (csrc/gemm.h GemmArgs::row_sel)
            # (``all_rows``: the caller reads the logits of EVERY row — all_logits — so every row is a logits row)
            # (``extra_rows``: packed rows whose logits are read besides the tails — score / score_batch: corrected too)
            sel = None if all_rows else self._lo4_selection(seq_lens if seq_lens is not None else [S], extra_rows)
            self.last_lo4_ranges = np.array([[0, S]], dtype=np.int32) if sel is None else sel[2].copy()
            h, att, gu = self._lo4_act(S, D, sel=sel), self._lo4_act(S, qw, heads=(H, hd), sel=sel), self._lo4_act(S, W.llm_ff, sel=sel)
            qkv = self._empty(S, qw + 2 * kw)
            sq_a, sq_b = self._empty(S, parts, dtype=torch.float32), self._empty(S, parts, dtype=torch.float32)
            w4s = self._lo4_weights("llm")
            first_needed = 0 if sel is None else int(sel[2][0, 0])   # ... under lo4 every selected row (sel None = all of them: no window)
            assert not last_only or sel is None or (len(sel[2]) == 1 and int(sel[2][0, 1]) == S)   # one sequence, no scored rows: its tail, one range
        else:
            sel, w4s = None, [(None,) * 4] * len(W.llm_layers)
            total, offs = ops.llm_prefill_workspace(S, D, H, KV, hd, W.llm_ff, self.dtype)
            h, qkv, att, gu, sq_a, sq_b = self._carve("llm", total, offs, [(S, D, self.dtype), (S, qw + 2 * kw, self.dtype), (S, qw, self.dtype),
                                                                             (S, W.llm_ff, self.dtype), (S, parts, torch.float32), (S, parts, torch.float32)])
            if not (fused and self.fuse_norm_rope):
                return self._llm_layers_unfused(x, cache, cu, cos, sin, max_len, (h, qkv, att, gu), prefix, cache_pos0, cu_k, rows_att)
        win = self._last_layer_window(S, first_needed) if last_only and prefix is None and cu_k is None else None
        n_layers = len(W.llm_layers)                            # sq_a: partials feeding gate/up; sq_b: feeding the next layer's qkv
        for i, (L, (qkv4, o4, gu4, down4)) in enumerate(zip(W.llm_layers, w4s)):
            kc, vc = (cache.k[i], cache.v[i]) if cache else (None, None)
            if i == 0:
                ops.norm(x, L.in_norm, None, h, tc.rms_norm_eps)
            if win is not None and i == n_layers - 1:
                w0 = win[0]
                wq, wkv = self._qkv_weight_parts(L.qkv_w_rope, qw)
                q4, kv4 = (Lo4Weight(qkv4.img[:qw], qkv4.sc[:qw]), Lo4Weight(qkv4.img[qw:], qkv4.sc[qw:])) if qkv4 is not None else (None, None)
                wsel = self._window_selection(sel, w0) if sel is not None else None
                hw, attw, guw = (rows_from(a, w0, wsel) for a in (h, att, gu))
                ops.qkv_rope(h, wkv, qkv[:, qw:], None if i == 0 else sq_b, tc.rms_norm_eps, cos, sin, kc, vc, cache_pos0, 0, KV, hd, kv4)
                ops.qkv_rope(hw, wq, qkv[w0:, :qw], None if i == 0 else sq_b[w0:], tc.rms_norm_eps, cos[w0:], sin[w0:], None, None, 0, H, 0, hd, q4)
                self._attend(i, qkv, attw, cu, max_len, cache, None, None, window=win)
                ops.linear(attw, L.o_w, x[w0:], o4, epilogue=_lib.EPI_RESIDUAL, norm_out=hw, norm_gamma=L.post_norm, rowsq_out=sq_a[w0:])
                ops.linear(hw, L.gu_w, guw, gu4, epilogue=_lib.EPI_SWIGLU, rowsq_in=sq_a[w0:], norm_dim=D, norm_eps=tc.rms_norm_eps)
                ops.linear(guw, L.down_w, x[w0:], down4, epilogue=_lib.EPI_RESIDUAL)
                break
            ops.qkv_rope(h, L.qkv_w_rope, qkv, None if i == 0 else sq_b, tc.rms_norm_eps, cos, sin, kc, vc, cache_pos0, H, KV, hd, qkv4)
            self._attend(i, qkv, att, cu, max_len, cache, prefix, cu_k, rows_att=rows_att)
            ops.linear(att, L.o_w, x, o4, epilogue=_lib.EPI_RESIDUAL, norm_out=h, norm_gamma=L.post_norm, rowsq_out=sq_a)
            ops.linear(h, L.gu_w, gu, gu4, epilogue=_lib.EPI_SWIGLU, rowsq_in=sq_a, norm_dim=D, norm_eps=tc.rms_norm_eps)
            if i + 1 < n_layers:
                ops.linear(gu, L.down_w, x, down4, epilogue=_lib.EPI_RESIDUAL, norm_out=h, norm_gamma=W.llm_layers[i + 1].in_norm, rowsq_out=sq_b)
            else:
                ops.linear(gu, L.down_w, x, down4, epilogue=_lib.EPI_RESIDUAL)
            if self.trace:
                self.trace(f"llm.{i}", x)

    def _llm_layers_unfused(self, x, cache, cu, cos, sin, max_len, bufs, prefix=None, cache_pos0=0, cu_k=None, rows_att=None):
        """The Llama / Mistral layers of the fast schedule launch by launch, on the workspace buffers ``bufs`` = (h, qkv, att, gu): where the
        shapes do not allow the fused schedule, the tensor-parallel packed prefill and the calibration pass (``_rec``)."""
        ops, W, tc = self.ops, self.W, self.cfg.text_config
        S, D = x.shape
        (H, KV), hd = self._llm_heads(), tc.head_dim
        qw, kw = H * hd, KV * hd
        h, qkv, att, gu = bufs
        tmp = self._empty(S, D, dtype=torch.float32) if self.tp_size > 1 else None
        rec = self._rec
        for i, L in enumerate(W.llm_layers):
            ops.rmsnorm(x, L.in_norm, h, tc.rms_norm_eps)
            rec and rec(("llm", i, "h1"), h)
            if L.qkv_w is not None:
                ops.gemm(h, L.qkv_w, qkv)
                ops.rope_qk(qkv, H, KV, hd, cos, sin, cache.k[i] if cache else None, cache.v[i] if cache else None, cache_pos0)
            else:                                    # packed weights keep the rope-ordered rows only: projection + RoPE + KV append on the normalised rows
                ops.rmsnorm_rope(h, L.qkv_w_rope, qkv, None, tc.rms_norm_eps, cos, sin, cache.k[i] if cache else None,
                                 cache.v[i] if cache else None, cache_pos0, H, KV, hd)
            if rec:                                  # operands of the fp8 attention arithmetic (rotated q / k, v)
                rec(("llm", i, "q"), qkv[:, :qw]); rec(("llm", i, "k"), qkv[:, qw:qw + kw]); rec(("llm", i, "v"), qkv[:, qw + kw:])
            self._attend(i, qkv, att, cu, max_len, cache, prefix, cu_k, rows_att=rows_att)
            rec and rec(("llm", i, "att"), att)
            self._row_parallel(att, L.o_w, x, tmp)
            ops.rmsnorm(x, L.post_norm, h, tc.rms_norm_eps)
            rec and rec(("llm", i, "h2"), h)
            ops.gemm(h, L.gu_w, gu, epilogue=_lib.EPI_SWIGLU)
            rec and rec(("llm", i, "gu"), gu)
            self._row_parallel(gu, L.down_w, x, tmp)
            if self.trace:
                self.trace(f"llm.{i}", x)

    def _llm_layers_fp8(self, x, cache, cu, cos, sin, max_len, seq_lens=None):
        """The Llama layers with fp8 linears (leopard_amd.fp8): RMSNorm -> fp8 operand in one launch, the SwiGLU epilogue of
        gate/up writes down_proj's fp8 operand; q|k|v, RoPE and the KV cache stay 16-bit, the stream fp32.  ``fp8_attention``: the
        attention's two products run on the fp8 matrix pipe as well (lmi_attn_prep_fp8 + lmi_attn_fp8_fwd: e4m3 q, k, v and P with the
        static scales of the plan; the cache keeps the 16-bit K / V for the decode)."""
        ops, W, tc, P = self.ops, self.W, self.cfg.text_config, self.fp8
        S, D = x.shape
        (H, KV), hd = self._llm_heads(), tc.head_dim
        qw, kw = H * hd, KV * hd
        u8 = torch.uint8
        h8 = self._empty(S, D, dtype=u8)
        att8 = self._empty(S, qw, dtype=u8)
        gu8 = self._empty(S, W.llm_ff, dtype=u8)
        qkv = self._empty(S, qw + 2 * kw)
        att = self._empty(S, qw)
        scale = hd ** -0.5
        fused = self.fp8_fused and self.use_tr          # (the fp8-output attention lives in the LDS-DMA kernel, the production one)
        a8 = (self.fp8_attention and fused and hd == 128 and seq_lens is not None and not (tc.sliding_window or 0)
              and all(k in Q.act for Q in P.llm for k in ("q", "k", "v")))
        if a8:
            tiles = [(int(l) + 63) // 64 for l in seq_lens]
            key = ("a8", tuple(int(l) for l in seq_lens))
            tb = self._geom_cache.get(key)
            if tb is None:
                tb = self._geom_cache[key] = self._pinned_to_device(torch.tensor([0] + list(np.cumsum(tiles)), dtype=torch.int32))
            n_tiles = sum(tiles)
            q8 = self._empty(S, qw, dtype=u8)
            k_img, v_img = self._empty(KV * n_tiles * 8192, dtype=u8), self._empty(KV * n_tiles * 8192, dtype=u8)
        for i, (L, Q) in enumerate(zip(W.llm_layers, P.llm)):
            ops.norm_fp8(x, L.in_norm, None, h8, tc.rms_norm_eps, 2.0 ** Q.act["h1"])
            if fused and hd == 128 and "qkv_rope" in Q.lin:
                ops.rope_qkv_fp8(h8, Q.lin["qkv_rope"].w8, qkv, Q.out_exp("h1", "qkv"), cos, sin, cache.k[i] if cache else None,
                                 cache.v[i] if cache else None, 0, H, KV, hd)
            else:
                ops.gemm_fp8(h8, Q.lin["qkv"].w8, qkv, scale_exp=Q.out_exp("h1", "qkv"))
                ops.rope_qk(qkv, H, KV, hd, cos, sin, cache.k[i] if cache else None, cache.v[i] if cache else None, 0)
            if a8:
                sq, sk, sv = 2.0 ** Q.act["q"], 2.0 ** Q.act["k"], 2.0 ** Q.act["v"]
                ops.attn_prep_fp8(qkv, cu, tb, n_tiles, H, KV, hd, sq, sk, sv, q8, k_img, v_img)
                ops.attention_fp8(q8, k_img, v_img, att8, cu, tb, n_tiles, max_len, H, KV, hd, scale, sq, sk, sv, causal=True,
                                  out_fp8_scale=2.0 ** Q.act["att"], dtype=self.dtype)
            elif fused:
                ops.attention_fp8out(qkv[:, :qw], qkv[:, qw:qw + kw], qkv[:, qw + kw:], att8, 2.0 ** Q.act["att"], cu, cu, max_len, H, KV, hd, scale,
                                     True, window=tc.sliding_window or 0)
            else:
                ops.attention(qkv[:, :qw], qkv[:, qw:qw + kw], qkv[:, qw + kw:], att, cu, cu, max_len, H, KV, hd, scale,
                              True, self.use_tr, window=tc.sliding_window or 0)
                ops.quantize_fp8(att, att8, 2.0 ** Q.act["att"])
            ops.gemm_fp8(att8, Q.lin["o"].w8, x, epilogue=_lib.EPI_RESIDUAL, scale_exp=Q.out_exp("att", "o"))
            ops.norm_fp8(x, L.post_norm, None, h8, tc.rms_norm_eps, 2.0 ** Q.act["h2"])
            ops.gemm_fp8(h8, Q.lin["gu"].w8, gu8, epilogue=_lib.EPI_SWIGLU, scale_exp=Q.out_exp("h2", "gu"),
                         out_scale=2.0 ** Q.act["gu"])
            ops.gemm_fp8(gu8, Q.lin["down"].w8, x, epilogue=_lib.EPI_RESIDUAL, scale_exp=Q.out_exp("gu", "down"))
            if self.trace:
                self.trace(f"llm.{i}", x)

    def _lm_head(self, x, last_rows, all_logits):
        ops, W, tc = self.ops, self.W, self.cfg.text_config
        V = tc.vocab_size
        # last position of every packed sequence: final RMSNorm + head in ONE launch over the fp32 rows (no 16-bit
        # rounding of the normalised row: lmi_lm_head_last)
        logits_last = self._empty(last_rows.numel(), W.lm_head.shape[0], dtype=torch.float32)
        ops.lm_head_last(W.lm_head, x, last_rows, W.final_norm, tc.rms_norm_eps, logits_last)
        logits_all = None
        if all_logits:
            hall = self._empty(*x.shape)
            ops.rmsnorm(x, W.final_norm, hall, tc.rms_norm_eps)
            logits_all = self._empty(x.shape[0], W.lm_head.shape[0], dtype=torch.float32)
            ops.gemm(hall, W.lm_head, logits_all, epilogue=_lib.EPI_STORE_F32)
            logits_all = logits_all[:, :V]
        return logits_last[:, :V], logits_all

    # ------------------------------------------------------------------------------------------------
    # the whole prefill for one sample (EVAL:261-333)
    # ------------------------------------------------------------------------------------------------
    def merged_len(self, input_ids: torch.Tensor, n_img: Optional[int] = None) -> int:
        """Rows of a prompt's merged sequence: every image token stands for ``tokens_per_tile`` rows.  ``n_img``: the number of image tokens
        where the caller knows it (its ViT-input count); counted from the ids otherwise."""
        if n_img is None:
            n_img = int((input_ids == self.cfg.image_token_index).sum())
        return input_ids.numel() + n_img * (self.cfg.tokens_per_tile - 1)

    @torch.no_grad()
    def prefill(self, input_ids: torch.Tensor, tiles: Optional[torch.Tensor], cache: Optional[KVCache] = None,
                all_logits: bool = False, keep_parts: bool = False, visual_tokens: Optional[torch.Tensor] = None
                ) -> PrefillResult:
        if self.tp_size > 1:
            if all_logits or keep_parts:
                raise NotImplementedError("all_logits / keep_parts are single-rank diagnostics")
            return self._prefill_tp(input_ids, tiles, cache, visual_tokens)
        parts = {} if keep_parts else None
        n_tiles = 0
        if visual_tokens is None and tiles is not None and tiles.shape[0] > 0:
            n_tiles = tiles.shape[0]
            vflags = self.lo4_vit_tiles([n_tiles], [self.merged_len(input_ids, n_tiles)])
            if keep_parts:
                vit = self.vision_tower(tiles, vflags)
                visual_tokens = self.project(vit, n_tiles)
                parts["vit"] = vit
            else:
                visual_tokens = self.encode_images(tiles, vflags)
        elif visual_tokens is not None:
            n_tiles = visual_tokens.shape[0] // self.cfg.tokens_per_tile
        if keep_parts and visual_tokens is not None:
            parts["visual_tokens"] = visual_tokens
        x = self.embed_merge(input_ids, visual_tokens)
        if keep_parts:
            parts["inputs_embeds"] = x.clone()
        S = x.shape[0]
        last, all_ = self.llm_prefill(x, [S], cache=cache, all_logits=all_logits)
        return PrefillResult(logits_last=last[0], seq_len=S, n_tiles=n_tiles, logits_all=all_, parts=parts)


    # ------------------------------------------------------------------------------------------------
    # ONE sample on all ranks (SURVEY.md 8e phases A + B): tile-sharded vision encode + one all-gather, then the
    # LLM tensor-parallel with sequence-parallel norms.  The fp32 residual stream is sharded by rows: with R ranks and NC row
    # chunks, chunk c holds global rows [c*R*Sl, (c+1)*R*Sl) and rank r owns rows [c*R*Sl + r*Sl, +Sl) of it.  Per half layer
    # and chunk:  RMSNorm(own rows) -> all-gather (16-bit, [R*Sl, D]) -> column-parallel GEMM(s) on all rows of the chunk for
    # this rank's heads / FFN slice -> row-parallel GEMM -> reduce-scatter (16-bit) -> residual add on the own rows.
    # Collectives go to a side stream; chunk c's exchange runs under chunk c+1's GEMMs.  Causal attention makes the row chunks
    # independent in the right order: chunk c attends to the K/V rows of chunks <= c, which the cache already holds.
    # ------------------------------------------------------------------------------------------------
    def _tp_geometry(self, S: int):
        R, NC = self.tp_size, max(1, int(self.tp_chunks))
        Sl = -(-S // (R * NC))
        Sl = (Sl + 7) // 8 * 8                                  # 16-byte aligned row blocks for the collectives
        return R, NC, Sl, R * Sl

    def tp_padded_len(self, S: int) -> int:
        """KV-cache rows a tensor-parallel prefill of S tokens writes (the row chunks are padded to equal size)."""
        R, NC, Sl, Sc = self._tp_geometry(S)
        return NC * Sc

    @torch.no_grad()
    def _prefill_tp(self, input_ids, tiles, cache, visual_tokens):
        from . import dist as D
        cfg, ops, W, tc = self.cfg, self.ops, self.W, self.cfg.text_config
        comm, dev = self.comm, self.device
        if visual_tokens is None and tiles is not None and tiles.shape[0] > 0:
            visual_tokens = D.encode_images_sharded(self, tiles)
        n_tiles = 0 if visual_tokens is None else visual_tokens.shape[0] // cfg.tokens_per_tile
        ids_host = input_ids.detach().reshape(-1).to("cpu", torch.int64)
        n_rows = 0 if visual_tokens is None else visual_tokens.shape[0]
        src = plan_merge(ids_host.numpy(), cfg.image_token_index, n_rows, cfg.tokens_per_tile)
        S = len(src)
        R, NC, Sl, Sc = self._tp_geometry(S)
        rank = comm.rank
        if cache is None:
            cache = KVCache(cfg, NC * Sc, self.dtype, dev, tp_size=R)
        assert cache.length == 0 and cache.capacity >= NC * Sc, "tensor-parallel prefill needs cache capacity >= tp_padded_len(S)"
        # merged embeddings of the rows this rank owns, chunk by chunk (rows past S: any text row, finite and never used)
        ids_dev = self._pinned_to_device(ids_host.contiguous()) if input_ids.device != dev else input_ids.reshape(-1).to(torch.int64).contiguous()
        pad_src = int(np.nonzero(src >= 0)[0][0]) if (src >= 0).any() else 0
        D_ = tc.hidden_size
        xs = []
        for c in range(NC):
            g0 = c * Sc + rank * Sl
            loc = np.full(Sl, src[pad_src], dtype=np.int64)
            n_real = max(0, min(Sl, S - g0))
            loc[:n_real] = src[g0:g0 + n_real]
            x = self._empty(Sl, D_, dtype=torch.float32)
            ops.embed_merge(ids_dev, self._pinned_to_device(torch.from_numpy(loc)), W.embed, visual_tokens, x)
            xs.append(x)
        self._llm_layers_tp(xs, S, cache)
        cache.length = S
        # last real row -> every rank (fp32, 16 KB), then the column-parallel head: rank r computes its slice of the vocabulary
        last = S - 1
        c_l, r_l, l_l = last // Sc, (last % Sc) // Sl, last % Sl
        xrow = xs[c_l][l_l:l_l + 1].clone() if rank == r_l else self._empty(1, D_, dtype=torch.float32)
        comm.broadcast(xrow, r_l)
        Vp = W.lm_head.shape[0]
        Vl = -(-Vp // R)
        lo, hi = min(Vp, rank * Vl), min(Vp, (rank + 1) * Vl)
        mine = torch.zeros(1, Vl, dtype=torch.float32, device=dev)
        if hi > lo:
            ops.lm_head_last(W.lm_head[lo:hi], xrow, None, W.final_norm, tc.rms_norm_eps, mine[:, :hi - lo])
        full = self._empty(R * Vl, dtype=torch.float32)
        comm.all_gather(full, mine.reshape(-1))
        return PrefillResult(logits_last=full[:tc.vocab_size], seq_len=S, n_tiles=n_tiles)

    def _llm_layers_tp(self, xs, S: int, cache: KVCache):
        """The sequence-parallel layer loop over the row chunks ``xs`` (fp32 [Sl, D] each, updated in place)."""
        ops, W, tc, comm = self.ops, self.W, self.cfg.text_config, self.comm
        R, NC, Sl, Sc = self._tp_geometry(S)
        (H, KV), hd, D_ = self._llm_heads(), tc.head_dim, tc.hidden_size
        qw, kw = H * hd, KV * hd
        dev, T = self.device, self.dtype
        cdt = self.tp_comm_dtype or T
        on_gpu = dev.type == "cuda" and not ops.emulated
        if on_gpu and self._comm_stream is None:
            self._comm_stream = torch.cuda.Stream(device=dev)
        cs = self._comm_stream if on_gpu else None
        ms = torch.cuda.current_stream(dev) if on_gpu else None

        def to_comm():                 # everything enqueued on the compute stream so far happens-before what follows on the comm stream
            if on_gpu:
                cs.wait_stream(ms)

        def done():                    # marker on the comm stream for the compute stream to wait on
            if not on_gpu:
                return None
            e = torch.cuda.Event()
            e.record(cs)
            return e

        def wait(e):
            if e is not None:
                ms.wait_event(e)
        pos = torch.arange(NC * Sc)
        cos, sin = self.rope_tables(pos)
        lo4, L4 = self.lo4, [(None,) * 4] * len(W.llm_layers)
        if lo4:
            # precision "lo4" under tensor parallelism: the rank's normalised rows are Lo4 pairs (16-bit rows + fp4 image of their rounding
            # residual + block scales; image and scales in ONE buffer so that one more all-gather moves both: + 27 % all-gather bytes), the
            # column-parallel GEMMs run the correction phase on the gathered pair against the image of THIS rank's weight shard, the
            # attention and the SwiGLU epilogue hand their images to the row-parallel GEMMs.  The partial products are exchanged as before.
            from .ops import lo4_packed_act
            if not (hd == 128 and W.llm_layers and W.llm_layers[0].qkv_w_rope is not None):
                raise RuntimeError("precision 'lo4' needs head_dim 128 and the rope-ordered q|k|v weights")
            L4 = self._lo4_weights("llm")
            h_loc = [lo4_packed_act(Sl, D_, T, dev) for _ in range(NC)]
            h_full = [lo4_packed_act(Sc, D_, T, dev) for _ in range(NC)]
            att, gu = self._lo4_act(Sc, qw, heads=(H, hd)), self._lo4_act(Sc, W.llm_ff)
        else:
            h_loc = [self._empty(Sl, D_) for _ in range(NC)]
            h_full = [self._empty(Sc, D_) for _ in range(NC)]
            att = self._empty(Sc, qw)
            gu = self._empty(Sc, W.llm_ff)
        part = [self._empty(Sc, D_, dtype=cdt) for _ in range(NC)]
        red = [self._empty(Sl, D_, dtype=cdt) for _ in range(NC)]
        qkv = self._empty(Sc, qw + 2 * kw)
        cu_q = torch.tensor([0, Sc], dtype=torch.int32, device=dev)
        cu_k = [torch.tensor([0, (c + 1) * Sc], dtype=torch.int32, device=dev) for c in range(NC)]
        scale = hd ** -0.5
        epi_part = _lib.EPI_STORE if cdt == T else _lib.EPI_STORE_F32
        fused_rope = lo4 or (self.fuse_norm_rope and hd == 128 and W.llm_layers and W.llm_layers[0].qkv_w_rope is not None)
        hi = lambda a: getattr(a, "hi", a)        # the 16-bit rows of an operand of either kind
        n_layers = len(W.llm_layers)
        ev = [None] * NC

        def gather(c):
            """all-gather of chunk c's normalised rows (and, under lo4, of their residual images) on the comm stream."""
            to_comm()
            comm.all_gather(hi(h_full[c]), hi(h_loc[c]), cs)
            if lo4:
                comm.all_gather(h_full[c].buf.view(torch.float16), h_loc[c].buf.view(torch.float16), cs)
            ev[c] = done()

        def add_norm(c, delta, w):              # (w None: the add alone, after the last layer)
            ops.add_norm(xs[c], delta, w, None if w is None else h_loc[c], tc.rms_norm_eps)
        for li, (L, (qkv4, o4, gu4, down4)) in enumerate(zip(W.llm_layers, L4)):
            # ---- attention half ----------------------------------------------------------------------------------------
            for c in range(NC):
                if li == 0:
                    ops.norm(xs[c], L.in_norm, None, h_loc[c], tc.rms_norm_eps)
                gather(c)
            for c in range(NC):
                wait(ev[c])
                kc, vc = cache.k[li], cache.v[li]
                if fused_rope:
                    ops.qkv_rope(h_full[c], L.qkv_w_rope, qkv, None, tc.rms_norm_eps, cos[c * Sc:(c + 1) * Sc], sin[c * Sc:(c + 1) * Sc],
                                 kc, vc, c * Sc, H, KV, hd, qkv4)
                else:
                    ops.gemm(h_full[c], L.qkv_w, qkv)
                    ops.rope_qk(qkv, H, KV, hd, cos[c * Sc:(c + 1) * Sc], sin[c * Sc:(c + 1) * Sc], kc, vc, c * Sc)
                ops.attend(qkv[:, :qw], kc[:(c + 1) * Sc], vc[:(c + 1) * Sc], att, cu_q, cu_k[c], Sc, H, KV, hd, scale, True,
                           self.use_tr, window=tc.sliding_window or 0)
                ops.linear(att, L.o_w, part[c], o4, epilogue=epi_part)
                to_comm()
                comm.reduce_scatter(red[c], part[c], cs)
                ev[c] = done()
            # ---- MLP half ----------------------------------------------------------------------------------------------
            for c in range(NC):
                wait(ev[c])
                add_norm(c, red[c], L.post_norm)
                gather(c)
            for c in range(NC):
                wait(ev[c])
                ops.linear(h_full[c], L.gu_w, gu, gu4, epilogue=_lib.EPI_SWIGLU)
                ops.linear(gu, L.down_w, part[c], down4, epilogue=epi_part)
                to_comm()
                comm.reduce_scatter(red[c], part[c], cs)
                ev[c] = done()
            for c in range(NC):
                wait(ev[c])
                add_norm(c, red[c], W.llm_layers[li + 1].in_norm if li + 1 < n_layers else None)
            if self.trace:
                self.trace(f"llm.{li}", xs)
        if on_gpu:
            ms.wait_stream(cs)

    @torch.no_grad()
    def prefill_batch(self, samples: Sequence[Tuple[torch.Tensor, Optional[torch.Tensor]]]):
        """Several samples in ONE pass (BASELINE config C5: a batch of multi-image samples): all ViT inputs go through the
        vision tower and the projector together, every sample's merged sequence is packed into one varlen causal batch
        (``cu_seqlens`` keeps the samples apart).  samples: [(input_ids [1, S_in], tiles u8 [N_i, S, S, 3] or None)].
        Returns (logits_last [n_samples, vocab], seq_lens).  The reference runs one sample per ``generate`` call
        (EVAL:448-454); results are identical to per-sample ``prefill`` calls."""
        x, seq_lens = self._pack_requests(samples)
        last, _ = self.llm_prefill(x, seq_lens)
        return last, seq_lens

    # ------------------------------------------------------------------------------------------------
    # scoring: log-likelihoods of labelled tokens (EVAL:333-348, forward(labels=)) with the head over the scored rows only
    # ------------------------------------------------------------------------------------------------
    IGNORE_INDEX = -100                # LlavaConfig.ignore_index / nn.CrossEntropyLoss's default

    def _host_labels(self, input_ids: torch.Tensor, labels) -> np.ndarray:
        """labels -> host int64 [S_in] after the checks that must fail before any launch: the shape of input_ids, ids in [0, V) or -100."""
        if labels is None:
            raise ValueError("score needs labels (the shape of input_ids; -100 = not scored)")
        lab = torch.as_tensor(labels).detach()
        if tuple(lab.shape) != tuple(input_ids.shape):
            raise ValueError(f"labels must have the shape of input_ids {tuple(input_ids.shape)}, got {tuple(lab.shape)}")
        lab = lab.to("cpu", torch.int64).reshape(-1).numpy()
        V = self.cfg.text_config.vocab_size
        bad = np.nonzero((lab != self.IGNORE_INDEX) & ((lab < 0) | (lab >= V)))[0]
        if len(bad):
            raise ValueError(f"labels must be token ids in [0, {V}) or {self.IGNORE_INDEX}: labels[{int(bad[0])}] = {int(lab[bad[0]])}")
        return lab

    def _merged_labels(self, ids: np.ndarray, labels: np.ndarray) -> np.ndarray:
        """transformers-4.38 ``_merge_input_ids_with_image_features`` with labels: every visual row gets the ignore index, each text label
        goes to its merged row (the rows plan_merge gives the text positions)."""
        is_img = ids == self.cfg.image_token_index
        width = np.where(is_img, self.cfg.tokens_per_tile, 1)
        start = np.cumsum(width) - width
        merged = np.full(int(width.sum()), self.IGNORE_INDEX, dtype=np.int64)
        merged[start[~is_img]] = labels[~is_img]
        return merged

    def score_targets(self, input_ids: torch.Tensor, labels) -> Tuple[np.ndarray, np.ndarray, int]:
        """(rows, targets, S) on the host: merged row s is scored against merged label s + 1 (EVAL:337-343's shift) wherever that label is
        not the ignore index.  Raises ValueError on bad labels (nothing is launched)."""
        lab = self._host_labels(input_ids, labels)
        merged = self._merged_labels(input_ids.detach().reshape(-1).to("cpu", torch.int64).numpy(), lab)
        tgt = merged[1:]
        rows = np.nonzero(tgt != self.IGNORE_INDEX)[0].astype(np.int64)
        return rows, tgt[rows], len(merged)

    def _request_visual(self, samples) -> List[Optional[torch.Tensor]]:
        """Visual tokens of every (input_ids, tiles[, visual_tokens]) request: the tiles of all requests through ONE vision encode (the
        graph-captured one when ``graph_encode`` is set)."""
        tpt = self.cfg.tokens_per_tile
        need = [(s[0], s[1]) for s in samples if (len(s) < 3 or s[2] is None) and s[1] is not None and s[1].shape[0] > 0]
        visual = None
        if need:
            vflags = self.lo4_vit_tiles([t.shape[0] for _, t in need], [self.merged_len(ids, t.shape[0]) for ids, t in need])
            visual = self.encode_images(torch.cat([t for _, t in need], dim=0), vflags)
        out, row = [], 0
        for s in samples:
            if len(s) > 2 and s[2] is not None:
                out.append(s[2])
            elif s[1] is not None and s[1].shape[0] > 0:
                n = s[1].shape[0]
                out.append(visual[row * tpt:(row + n) * tpt])
                row += n
            else:
                out.append(None)
        return out

    def _pack_requests(self, samples) -> Tuple[torch.Tensor, List[int]]:
        """(input_ids, tiles[, visual_tokens]) requests -> (fp32 residual stream of their merged sequences, packed [sum(seq_lens), D],
        seq_lens): all ViT inputs go through the tower and the projector together (_request_visual), ``cu_seqlens`` keeps the sequences
        apart in the LLM pass."""
        xs = [self.embed_merge(s[0], v) for s, v in zip(samples, self._request_visual(samples))]
        return (torch.cat(xs, dim=0) if len(xs) > 1 else xs[0]), [x.shape[0] for x in xs]

    def _move_kv(self, src: KVCache, begin: int, S: int, k_dst: List[torch.Tensor], v_dst: List[torch.Tensor], row0: int) -> None:
        """Rows [begin, begin + S) of every layer of ``src`` -> rows [row0, row0 + S) of the per-layer caches ``k_dst`` / ``v_dst``."""
        for i in range(len(src.k)):
            self.ops.kv_append(src.k[i][begin:begin + S], src.v[i][begin:begin + S], k_dst[i], v_dst[i], row0)

    def _load_rows(self, pieces: Sequence[Tuple[KVCache, int, int]], k_dst: List[torch.Tensor], v_dst: List[torch.Tensor], row0: int) -> None:
        """Fill a decode slot: the row ranges ``pieces`` = [(cache, begin, n)] copied back to back from row ``row0`` of ``k_dst`` / ``v_dst``
        on (a shared prefix's rows, then the request's own)."""
        for src, begin, n in pieces:
            self._move_kv(src, begin, n, k_dst, v_dst, row0)
            row0 += n

    def _score_head(self, x: torch.Tensor, rows: torch.Tensor, targets: torch.Tensor):
        """Final RMSNorm of the gathered rows (lmi_rmsnorm_rows: the bits lmi_rmsnorm gives them in a stream of more than 32 rows; a shorter stream
        goes through lmi_rmsnorm's few-rows kernel, which may differ in the last bit) -> head GEMM into ONE reusable fp32 chunk of at most
        ``score_chunk_rows`` rows -> lmi_token_logprobs.  Peak extra memory: about one chunk, whatever the number of rows."""
        ops, W, tc = self.ops, self.W, self.cfg.text_config
        n, D, Vp = rows.numel(), x.shape[1], W.lm_head.shape[0]
        C = max(1, min(int(self.score_chunk_rows), n))
        h = self._empty(C, D)
        buf = self._empty(C, Vp, dtype=torch.float32)
        lp, lse = self._empty(n, dtype=torch.float32), self._empty(n, dtype=torch.float32)
        am = self._empty(n, dtype=torch.int64)
        for c0 in range(0, n, C):
            m = min(C, n - c0)
            ops.rmsnorm_rows(x, rows[c0:c0 + m], W.final_norm, h[:m], tc.rms_norm_eps)
            ops.gemm(h[:m], W.lm_head, buf[:m], epilogue=_lib.EPI_STORE_F32)
            ops.token_logprobs(buf[:m], tc.vocab_size, targets[c0:c0 + m], lp[c0:c0 + m], lse[c0:c0 + m], am[c0:c0 + m])
        return lp, am

    @torch.no_grad()
    def score(self, input_ids: torch.Tensor, tiles, labels, visual_tokens: Optional[torch.Tensor] = None) -> ScoreResult:
        """Log-likelihoods of the labelled tokens of one request: ``labels`` [1, S_in] as input_ids, -100 = not scored (LlavaForConditional-
        Generation.forward(labels=) semantics, EVAL:333-348: the 4.38 merge with labels, then merged row s predicts merged label s + 1).  The
        head runs over the scored rows only, in chunks; under precision "lo4" the pass also corrects the scored rows.  No targets: loss nan
        and no head launch."""
        return self.score_batch([(input_ids, tiles, labels)], visual_tokens=[visual_tokens])[0]

    @torch.no_grad()
    def score_batch(self, requests: Sequence[tuple], visual_tokens: Optional[Sequence[Optional[torch.Tensor]]] = None) -> List[ScoreResult]:
        """score() for several requests [(input_ids [1, S_in], tiles, labels)] in ONE packed varlen prefill (as prefill_batch); request i's
        results are those of its own score() call, bit for bit.  All labels are checked before anything is launched."""
        if self.tp_size > 1:
            raise NotImplementedError("scoring runs on one rank (tensor-parallel engines: out of scope, as all_logits)")
        plans = [self.score_targets(r[0], r[2]) for r in requests]
        if not any(len(p[0]) for p in plans):                        # nothing labelled: nothing to compute (nn.CrossEntropyLoss gives nan)
            return [self._empty_score(S) for _, _, S in plans]
        x, seq_lens = self._pack_requests([(r[0], r[1], None if visual_tokens is None else visual_tokens[i]) for i, r in enumerate(requests)])
        for (_, _, S), l in zip(plans, seq_lens):
            assert S == l
        offs = np.cumsum([0] + seq_lens[:-1])
        rows_all = np.concatenate([p[0] + o for p, o in zip(plans, offs)])
        tgt_all = np.concatenate([p[1] for p in plans])
        self.llm_prefill(x, seq_lens, score_rows=rows_all)
        rows_dev = torch.from_numpy(rows_all).to(self.device)
        tgt_dev = torch.from_numpy(tgt_all).to(self.device)
        lp, am = self._score_head(x, rows_dev, tgt_dev)
        out, k = [], 0
        for (rows, _, S), o in zip(plans, offs):
            m = len(rows)
            if m:
                loss = (-lp[k:k + m].to(torch.float64).mean()).to(torch.float32)      # the mean over the request's targets (fp64 sum)
                out.append(ScoreResult(loss, lp[k:k + m], am[k:k + m], tgt_dev[k:k + m], rows_dev[k:k + m] - int(o), S))
            else:
                out.append(self._empty_score(S))
            k += m
        return out

    def logits_logprobs(self, logits: torch.Tensor, rows: np.ndarray, targets: np.ndarray):
        """lmi_token_logprobs on rows of already computed fp32 logits [S, >= V] (forward(labels=): no second head pass).  Returns (token
        logprobs fp32 [n], argmax int64 [n]) on the device."""
        n = len(rows)
        lp, lse = self._empty(n, dtype=torch.float32), self._empty(n, dtype=torch.float32)
        am = self._empty(n, dtype=torch.int64)
        if n:
            self.ops.token_logprobs(logits, self.cfg.text_config.vocab_size, torch.from_numpy(np.ascontiguousarray(targets)).to(self.device), lp, lse,
                                    am, rows=torch.from_numpy(np.ascontiguousarray(rows)).to(self.device))
        return lp, am

    def _empty_score(self, S: int) -> ScoreResult:
        e = lambda dt: self._empty(0, dtype=dt)
        return ScoreResult(torch.full((), float("nan"), dtype=torch.float32, device=self.device), e(torch.float32), e(torch.int64),
                           e(torch.int64), e(torch.int64), S)

    # ------------------------------------------------------------------------------------------------
    # a12: decode.  One step = ~290 launches of memory-bound kernels, so the step is captured once per KV cache into a
    # HIP graph over static buffers; the token id and the position live in device memory (lmi_rope_qk_at, device
    # cu_seqlens), the graph itself takes the argmax and advances the position, and the host only reads the new token.
    # ------------------------------------------------------------------------------------------------
    def _decode_buffers(self, B: int, capacity: int, prefix_capacity: int = 0, pair_limit: Optional[int] = None) -> DecodeState:
        """What the batch-1 and the pooled decode state allocate alike: a function of (B, capacity) under the engine's current mode
        (``prefix_capacity`` > 0: the shared-prefix step — positions run to prefix_capacity + capacity, the workspace is that launch's)."""
        W, tc, dev = self.W, self.cfg.text_config, self.device
        (H, KV), hd, D = self._llm_heads(), tc.head_dim, tc.hidden_size
        hl = self.decode_hl(B, pair_limit)
        R = 2 * B if hl else B
        cos, sin = self.rope_tables(torch.arange(prefix_capacity + capacity))
        ws_elems = (self.ops.decode_shared_workspace_elems(B, H, hd, prefix_capacity, capacity) if prefix_capacity
                    else self.ops.decode_workspace_elems(B, H, hd, capacity))
        return DecodeState(
            B=B, capacity=capacity, mode=(self.precision, self.decode_precision), layout=self.llm_packed, hl=hl,
            tok=torch.zeros(B, dtype=torch.int64, device=dev), src=torch.arange(B, dtype=torch.int64, device=dev),
            pos=torch.zeros(B, dtype=torch.int32, device=dev), cu_q=torch.arange(B + 1, dtype=torch.int32, device=dev),
            k_begin=(torch.arange(B, dtype=torch.int32) * capacity).to(dev),
            x=self._empty(B, D, dtype=torch.float32), h=self._empty(R, D), qkv=self._empty(B, (H + 2 * KV) * hd), att=self._empty(R, H * hd),
            gu=self._empty(R, W.llm_ff), hf32=self._empty(B, D, dtype=torch.float32) if hl else None, cos=cos, sin=sin,
            ws=torch.empty(ws_elems, dtype=torch.float32, device=dev),
            temp=torch.ones(B, dtype=torch.float32, device=dev), topk=torch.zeros(B, dtype=torch.int32, device=dev),
            topp=torch.ones(B, dtype=torch.float32, device=dev), seed=torch.zeros(B, dtype=torch.int64, device=dev),
            step=torch.zeros(B, dtype=torch.int32, device=dev),
            ext=torch.tensor([0.0, 1.0, 0.0, 0.0], dtype=torch.float32).repeat(B, 1).t().contiguous().to(dev))

    def _decode_state(self, cache: KVCache) -> DecodeState:
        st = cache._decode_state
        if st is not None and st.mode == (self.precision, self.decode_precision):
            return st                                                 # (a state built under another precision mode is rebuilt: other buffers, other launches)
        D, dev = self.cfg.text_config.hidden_size, self.device
        st = self._decode_buffers(1, cache.capacity)
        st.cu_k = torch.tensor([0, 1], dtype=torch.int32, device=dev)
        st.part = torch.zeros(D, dtype=torch.float32, device=dev)
        st.sq_a, st.sq_b = self._empty(1, max(D // 16, 1), dtype=torch.float32), self._empty(1, max(D // 16, 1), dtype=torch.float32)
        st.logits = self._empty(self.W.lm_head.shape[0], dtype=torch.float32)
        cache._decode_state = st
        return st

    def _decode_body(self, st, cache: KVCache):
        """Everything of one decode step that does not depend on host values."""
        ops, W, tc = self.ops, self.W, self.cfg.text_config
        (H, KV), hd = self._llm_heads(), tc.head_dim
        qw = H * hd
        tp = self.tp_size > 1

        def row_parallel(w, a):
            if not tp:
                ops.gemv(w, a, st.x[0], epilogue=2)
                return
            ops.gemv(w, a, st.part, epilogue=0)
            self.comm.all_reduce(st.part)
            st.x[0].add_(st.part)
        ops.embed_merge(st.tok, st.src, W.embed, None, st.x)
        if self.llm_packed:
            # one copy of the weights, in the operand order of lmi_gemm_skinny: the batch-1 step is the batched step with one row (measured:
            # 3.10 ms per step at B = 2 against 3.12 ms for the GEMV step), its KV rows go to this cache, the head keeps the fp32 row
            self._skinny_layers(st, cache.k, cache.v, cache.capacity,
                                lambda i: ops.attention_decode(st.qkv[:, :qw], cache.k[i], cache.v[i], st.att, st.cu_q, st.cu_k, 1, cache.capacity, H, KV,
                                                               hd, hd ** -0.5, st.ws, window=tc.sliding_window or 0, hl=st.hl))
            ops.lm_head_last(W.lm_head, st.x, None, W.final_norm, tc.rms_norm_eps, st.logits.view(1, -1))
            self._choose(st, st.logits.view(1, -1), k_len=st.cu_k[1:])
            return
        fuse = tc.hidden_size == 4096                 # lmi_gemv_rmsnorm: the norm rides in the projection's launch
        for i, L in enumerate(W.llm_layers):
            if fuse and hd == 128 and L.qkv_w_rope is not None:   # norm + projection + RoPE + KV append: one launch
                ops.gemv_rmsnorm_rope(L.qkv_w_rope, st.x[0], L.in_norm, tc.rms_norm_eps, st.qkv[0], H, KV, hd, st.cos, st.sin,
                                      cache.k[i], cache.v[i], st.pos)
            else:
                if fuse:
                    ops.gemv_rmsnorm(L.qkv_w, st.x[0], L.in_norm, tc.rms_norm_eps, st.qkv[0], epilogue=1)
                else:
                    ops.rmsnorm(st.x, L.in_norm, st.h, tc.rms_norm_eps)
                    ops.gemv(L.qkv_w, st.h[0], st.qkv[0], epilogue=1)
                ops.rope_qk_at(st.qkv, H, KV, hd, st.cos, st.sin, cache.k[i], cache.v[i], st.pos)
            ops.attention_decode(st.qkv[:, :qw], cache.k[i], cache.v[i], st.att, st.cu_q, st.cu_k, 1, cache.capacity, H, KV, hd,
                                 hd ** -0.5, st.ws, window=tc.sliding_window or 0)
            row_parallel(L.o_w, st.att[0])
            if fuse:
                ops.gemv_rmsnorm(L.gu_w, st.x[0], L.post_norm, tc.rms_norm_eps, st.gu[0], epilogue=3)
            else:
                ops.rmsnorm(st.x, L.post_norm, st.h, tc.rms_norm_eps)
                ops.gemv(L.gu_w, st.h[0], st.gu[0], epilogue=3)
            row_parallel(L.down_w, st.gu[0])
        ops.lm_head_last(W.lm_head, st.x, None, W.final_norm, tc.rms_norm_eps, st.logits.view(1, -1))
        # greedy (or sampled) choice and position / key-count advance stay on the device, one launch (lmi_decode_advance /
        # lmi_decode_sample; capturable)
        self._choose(st, st.logits.view(1, -1), k_len=st.cu_k[1:])

    def _set_sampling(self, st, j: int, sp: "SamplingParams", step: int = 1) -> None:
        """Row j of a decode state draws with ``sp`` from counter ``step`` on (the token from the prefill was step 0)."""
        vals = torch.tensor([float(sp.temperature), float(sp.top_p)], dtype=torch.float32)
        ints = torch.tensor([int(sp.top_k), int(step)], dtype=torch.int32)
        st.temp[j:j + 1].copy_(vals[0:1]); st.topp[j:j + 1].copy_(vals[1:2])
        st.topk[j:j + 1].copy_(ints[0:1]); st.step[j:j + 1].copy_(ints[1:2])
        st.seed[j:j + 1].copy_(torch.tensor([_signed64(sp.seed)], dtype=torch.int64))
        if st.sample_ex:                                              # (a call without the four warpers never reads them: nothing more is written)
            st.ext[:, j:j + 1].copy_(torch.tensor([[sp.min_p], [sp.typical_p], [sp.epsilon_cutoff], [sp.eta_cutoff]], dtype=torch.float32))

    def _choose(self, st, logits, **kw) -> None:
        """The tail of a decode step: lmi_decode_advance (greedy) or lmi_decode_sample (st.sampling) — the only difference between the two
        captured steps — after lmi_decode_rules when the call has rules (HF's order: processors, then suppress list, then warpers)."""
        V = self.cfg.text_config.vocab_size
        if st.beams:                                                  # generate_beams: the beams choose jointly, then every slot's K / V rows follow
            if st.rules:                                              # ... from the processed rows, and every slot's id list follows too
                self.ops.beam_step_rules(logits, V, st.beams, st.beam_eos, st.beam_score, st.tok, st.beam_parent, st.beam_walk, *st.beam_rows,
                                         st.seq, st.seq_len, st.rule_pen, st.rule_ngram, st.rule_min_left, append=st.tok,
                                         suppress=self.suppress_tokens, pos=st.pos, k_len=kw.get("k_len"), rows_held=st.beam_held)
            else:
                self.ops.beam_step(logits, V, st.beams, st.beam_eos, st.beam_score, st.tok, st.beam_parent, st.beam_walk, *st.beam_rows,
                                   suppress=self.suppress_tokens, pos=st.pos, k_len=kw.get("k_len"), rows_held=st.beam_held)
            self.ops.beam_reorder(st.beam_ptrs, st.beam_parent, st.beams, st.beam_row0, st.beam_held, st.k[0].stride(0) * st.k[0].element_size(),
                                  st.capacity, st.beam_max_rows)
            if st.rules:                                              # the id lists: 16-byte "rows" of four ids, from the prompt's last chunk on
                self.ops.beam_reorder(st.beam_id_ptr, st.beam_parent, st.beams, st.beam_id_chunks[:1], st.beam_id_chunks[1:], 16,
                                      st.seq.shape[1] // 4, st.beam_max_rows)
            return
        if st.rules:                                                  # generate(rules=...): one more launch, before the choice (it rewrites the rows)
            self.ops.decode_rules(logits, V, st.seq, st.seq_len, st.rule_pen, st.rule_ngram, st.rule_min_left, tok=st.tok, live=kw.get("live"),
                                  eos=st.rule_eos)
        if st.sampling and st.sample_ex:                              # min_p / typical_p / epsilon_cutoff / eta_cutoff after top-p
            self.ops.decode_sample_ex(logits, V, st.temp, st.topk, st.topp, st.seed, st.step, st.tok, st.pos, *st.ext,
                                      suppress=self.suppress_tokens, **kw)
        elif st.sampling:
            self.ops.decode_sample(logits, V, st.temp, st.topk, st.topp, st.seed, st.step, st.tok, st.pos, suppress=self.suppress_tokens, **kw)
        else:
            self.ops.decode_advance(logits, V, st.tok, st.pos, suppress=self.suppress_tokens, **kw)
        if st.logprobs is not None:                                   # generate(logprobs=k): one more launch, after the choice (it reads st.tok)
            self.ops.decode_logprobs(logits, V, st.tok, st.logprobs, st.lp, st.top_id, st.top_lp, hist_pos=kw.get("hist_pos"))

    # ---- generate(rules=...): the host side ----
    def _rules_arg(self, what: str, rules: Optional[LogitsRules], logprobs: Optional[int], eos_token_id) -> Optional[LogitsRules]:
        """Validate ``rules`` before anything is launched: None when absent or with everything off."""
        if rules is None:
            return None
        if not isinstance(rules, LogitsRules):
            raise TypeError(f"{what}: rules must be a LogitsRules, got {type(rules).__name__}")
        if not rules.active:
            return None
        if logprobs is not None:
            raise NotImplementedError(f"{what}: rules with logprobs is not supported (the logprob rings promise values of the RAW logits row, "
                                      "and lmi_decode_rules rewrites the row in place before the choice)")
        if self.tp_size > 1:
            raise NotImplementedError(f"{what}: rules are not supported on tensor-parallel engines (the rules launch and its per-slot state belong "
                                      "to the single-rank decode step)")
        if int(rules.min_new_tokens) > 0 and len(set(int(e) for e in eos_token_id)) > self.MAX_EOS:
            raise NotImplementedError(f"{what}: min_new_tokens with more than {self.MAX_EOS} eos ids is not supported (the device holds "
                                      f"{self.MAX_EOS})")
        V = self.cfg.text_config.vocab_size
        if V > self.ops.RULES_MAX_VOCAB:
            raise NotImplementedError(f"{what}: rules need a vocabulary of at most {self.ops.RULES_MAX_VOCAB} ids (this model: {V})")
        return rules

    def _rule_eos(self, rules: LogitsRules, eos) -> torch.Tensor:
        """The eos ids the minimum-length rule bans, int64 [MAX_EOS] on the host (-1 = unused; all unused without that rule)."""
        ids = sorted(set(int(e) for e in eos)) if int(rules.min_new_tokens) > 0 else []
        return torch.tensor(ids + [-1] * (self.MAX_EOS - len(ids)), dtype=torch.int64)

    def _set_rules(self, st, rules: Optional[LogitsRules], eos=()) -> None:
        """The state runs the step with (or without) the rules launch; the first call with rules allocates their buffers."""
        st.rules = rules is not None
        if rules is None:
            return
        if st.seq is None:
            dev, B = self.device, st.B
            st.seq = torch.zeros(B, st.prefix_capacity + st.capacity, dtype=torch.int32, device=dev)
            st.seq_len = torch.zeros(B, dtype=torch.int32, device=dev)
            st.rule_pen = torch.ones(B, dtype=torch.float32, device=dev)
            st.rule_ngram = torch.zeros(B, dtype=torch.int32, device=dev)
            st.rule_min_left = torch.zeros(B, dtype=torch.int32, device=dev)
            st.rule_eos = torch.full((self.MAX_EOS,), -1, dtype=torch.int64, device=dev)
        st.rule_eos.copy_(self._rule_eos(rules, eos))

    def _fill_rules(self, st, j: int, prompt: Sequence[int], rules: LogitsRules) -> None:
        """Slot j starts a request under ``rules``: its ids so far are the prompt's (the first token is appended by step 1's kernel, from
        st.tok), and eos stays banned for min_new_tokens - 1 more steps (the first token was chosen under the rule already)."""
        n = len(prompt)
        if n >= st.seq.shape[1]:
            raise ValueError(f"rules: a prompt of {n} ids does not fit the {st.seq.shape[1]} ids a decode slot holds")
        st.seq[j, :n].copy_(torch.tensor(list(prompt), dtype=torch.int32))
        ints = torch.tensor([n, int(rules.no_repeat_ngram_size), max(int(rules.min_new_tokens) - 1, 0)], dtype=torch.int32)
        st.seq_len[j:j + 1].copy_(ints[0:1]); st.rule_ngram[j:j + 1].copy_(ints[1:2]); st.rule_min_left[j:j + 1].copy_(ints[2:3])
        st.rule_pen[j:j + 1].copy_(torch.tensor([float(rules.repetition_penalty)], dtype=torch.float32))

    def first_rules(self, logits: torch.Tensor, prompts: Sequence[Sequence[int]], rules: LogitsRules, eos) -> torch.Tensor:
        """The prefill / extend logits rows ([n, >= vocab] or [vocab]) after the rules, for the FIRST token of each request: the same kernel
        as inside the step, run eagerly on a COPY of the rows (the caller's logits are never modified), nothing appended (the ids seen are
        the prompt's), eos banned when min_new_tokens > 0."""
        rows = logits.reshape(-1, logits.shape[-1]).to(torch.float32).clone().contiguous()
        n, dev = rows.shape[0], rows.device
        assert len(prompts) == n
        seq = torch.zeros(n, max(max(len(p) for p in prompts), 1), dtype=torch.int32)
        for j, p in enumerate(prompts):
            seq[j, :len(p)] = torch.tensor(list(p), dtype=torch.int32)
        full = lambda v, dt: torch.full((n,), v, dtype=dt).to(dev)
        self.ops.decode_rules(rows, min(self.cfg.text_config.vocab_size, rows.shape[1]), seq.to(dev),
                              torch.tensor([len(p) for p in prompts], dtype=torch.int32).to(dev), full(float(rules.repetition_penalty), torch.float32),
                              full(int(rules.no_repeat_ngram_size), torch.int32), full(int(rules.min_new_tokens), torch.int32),
                              eos=self._rule_eos(rules, eos).to(dev))
        return rows

    # ---- generate(logprobs=k): the host side ----
    def _sampling_arg(self, what: str, sampling: Optional["SamplingParams"]) -> Optional["SamplingParams"]:
        """Validate ``sampling`` before anything is launched: the four warpers of lmi_decode_sample_ex need a single-rank engine."""
        if sampling is not None and sampling.extended and self.tp_size > 1:
            raise NotImplementedError(f"{what}: min_p / typical_p / epsilon_cutoff / eta_cutoff are not supported on tensor-parallel engines "
                                      f"(got {sampling.describe()})")
        return sampling

    def _logprobs_arg(self, what: str, logprobs: Optional[int]) -> Optional[int]:
        """Validate ``logprobs`` before anything is launched: None, or k in 0 .. 8 on a single-rank engine."""
        if logprobs is None:
            return None
        K = self.ops.MAX_TOP_LOGPROBS
        if isinstance(logprobs, bool) or not isinstance(logprobs, (int, np.integer)) or not 0 <= int(logprobs) <= K:
            raise ValueError(f"{what}: logprobs must be None or an int in 0 .. {K}, got {logprobs!r}")
        if self.tp_size > 1:
            raise NotImplementedError(f"{what}: logprobs is not supported on tensor-parallel engines (the logprobs launch and its rings belong to "
                                      "the single-rank decode step; the tensor-parallel step has no captured form with it)")
        return int(logprobs)

    def _set_logprobs(self, st, k: Optional[int]) -> None:
        st.logprobs = k
        if k is not None and st.lp_buf is None:                       # the rings: HIST slots beside a token history ring, else one
            K, ring = self.ops.MAX_TOP_LOGPROBS, (self.HIST if st.hist is not None else 1)
            n = ring * st.B
            st.lp_buf = torch.zeros(n * (1 + 2 * K), dtype=torch.int32, device=self.device)
            st.lp, st.top_id = st.lp_buf[:n].view(torch.float32).view(ring, st.B), st.lp_buf[n:n * (1 + K)].view(ring, st.B, K)
            st.top_lp = st.lp_buf[n * (1 + K):].view(torch.float32).view(ring, st.B, K)
        if k is not None and st.lp_k != k:                            # top_k is a launch argument: the captured logprobs steps hold one value
            st.graphs.pop((False, True), None); st.graphs.pop((True, True), None)      # (the steps with rules never hold the logprobs launch)
            st.lp_k = k

    def _rings_to_host(self, st):
        """(lp [ring, B], top_id [ring, B, 8], top_lp [ring, B, 8]) on the host: ONE copy of the state's ring buffer."""
        buf, n, K = st.lp_buf.to("cpu", copy=True), st.lp.numel(), self.ops.MAX_TOP_LOGPROBS
        return (buf[:n].view(torch.float32).view(st.lp.shape), buf[n:n * (1 + K)].view(st.top_id.shape),
                buf[n * (1 + K):].view(torch.float32).view(st.top_lp.shape))

    def first_logprobs(self, logits: torch.Tensor, toks: Sequence[int], k: int):
        """The logprob rows of the FIRST token of each request, from its prefill / extend logits row ([n, >= vocab] or [vocab]): the same
        kernel as inside the step, run eagerly (ring of one slot).  Returns host (lp [n], top_id [n, 8], top_lp [n, 8])."""
        rows = logits.reshape(-1, logits.shape[-1]).float()
        n, dev, K = rows.shape[0], rows.device, self.ops.MAX_TOP_LOGPROBS
        V = min(self.cfg.text_config.vocab_size, rows.shape[1])
        if rows.stride(1) != 1 or rows.stride(0) % 4 or rows.data_ptr() % 16:    # the kernel reads 16-byte aligned rows
            pad = torch.zeros(n, (rows.shape[1] + 3) // 4 * 4, dtype=torch.float32, device=dev)
            pad[:, :rows.shape[1]] = rows
            rows = pad
        tok = torch.tensor([int(t) for t in toks], dtype=torch.int64).to(dev)
        lp = torch.zeros(1, n, dtype=torch.float32, device=dev)
        ti = torch.full((1, n, K), -1, dtype=torch.int32, device=dev)
        tl = torch.full((1, n, K), float("-inf"), dtype=torch.float32, device=dev)
        self.ops.decode_logprobs(rows, V, tok, k, lp, ti, tl)
        return lp[0].cpu(), ti[0].cpu(), tl[0].cpu()

    @staticmethod
    def _outputs(toks: Sequence[List[int]], like: Sequence[torch.Tensor], lpr: Optional[Sequence[_LogprobRows]], n_prompt: Sequence[int],
                 one: bool = False):
        """What a generation call returns for its requests: each token list as a LongTensor [1, n] on the device of the request's ids
        (``like``) — the list of them, or (``one``) the tensor of the only request — and, with ``logprobs`` (``lpr``), the GenerateOutput
        around that with the rows of the tokens after the n_prompt ids."""
        seqs = [torch.tensor([t], dtype=torch.long, device=ids.device) for t, ids in zip(toks, like)]
        seqs = seqs[0] if one else seqs
        if lpr is None:
            return seqs
        res = [r.result(len(t) - int(p)) for r, t, p in zip(lpr, toks, n_prompt)]
        return GenerateOutput(seqs, [r[0] for r in res], [r[1] for r in res], [r[2] for r in res])

    def _first_tokens(self, logits: torch.Tensor, params: Optional[Sequence["SamplingParams"]], k: Optional[int],
                      rules: Optional[LogitsRules] = None, prompts: Optional[Sequence[Sequence[int]]] = None, eos=()):
        """The first token of each of n requests from its prefill / extend logits row ([n, >= vocab] or [vocab]): greedy (``params`` None) or
        drawn with its SamplingParams at step 0, then — ``logprobs`` = k — one eager logprobs launch for all of them.  With ``rules`` the
        choice is made from a copy of the rows that lmi_decode_rules has rewritten over ``prompts`` (first_rules).  Returns (first
        [n], the requests' _LogprobRows holding that first row, or None)."""
        rows = logits.reshape(-1, logits.shape[-1])
        if rules is not None:
            rows = self.first_rules(rows, prompts, rules, eos)
        first = [self.first_token(r) for r in rows] if params is None else self.sample_first(rows, params)
        if k is None:
            return first, None
        lpr = [_LogprobRows(k) for _ in first]
        for r, row in zip(lpr, zip(*self.first_logprobs(rows, first, k))):
            r.add(*row)
        return first, lpr

    def sample_first(self, logits: torch.Tensor, params: Sequence["SamplingParams"]) -> List[int]:
        """The first token of each request from its prefill logits row ([n, >= vocab] or [vocab]) through lmi_decode_sample at step 0
        (the sampled counterpart of ``first_token``), through lmi_decode_sample_ex when a request has one of its four warpers on."""
        rows = logits.reshape(-1, logits.shape[-1]).float()
        n, dev = rows.shape[0], rows.device
        temp = torch.tensor([float(p.temperature) for p in params], dtype=torch.float32).to(dev)
        topk = torch.tensor([int(p.top_k) for p in params], dtype=torch.int32).to(dev)
        topp = torch.tensor([float(p.top_p) for p in params], dtype=torch.float32).to(dev)
        seed = torch.tensor([_signed64(p.seed) for p in params], dtype=torch.int64).to(dev)
        step = torch.zeros(n, dtype=torch.int32, device=dev)
        tok = torch.zeros(n, dtype=torch.int64, device=dev)
        pos = torch.zeros(n, dtype=torch.int32, device=dev)
        V = min(self.cfg.text_config.vocab_size, rows.shape[1])
        if any(p.extended for p in params):
            ext = torch.tensor([[p.min_p for p in params], [p.typical_p for p in params], [p.epsilon_cutoff for p in params],
                                [p.eta_cutoff for p in params]], dtype=torch.float32).to(dev)
            self.ops.decode_sample_ex(rows, V, temp, topk, topp, seed, step, tok, pos, *ext, suppress=self.suppress_tokens)
        else:
            self.ops.decode_sample(rows, V, temp, topk, topp, seed, step, tok, pos, suppress=self.suppress_tokens)
        return [int(t) for t in tok.tolist()]

    def _run_step(self, st, body, restore: tuple, capturable: bool = True) -> None:
        """One decode step of ``st``.  ``body`` runs eagerly on the emulator, off a device, with graphs off or when the step is not
        ``capturable``; otherwise the captured step of (st.sampling, with logprobs[, with rules]) is replayed — warmed up and captured on its
        first use (two Python runs of ``body``), after each of which the device state the step advances (``restore``, the logprob rings, the
        rules' sequence length and eos countdown; the id the rules launch appended lands in the same cell again) is put back."""
        if self.ops.emulated or self.device.type != "cuda" or not self.use_graphs or not capturable:
            body()
            return
        key = (st.sampling, st.logprobs is not None) + ((True,) if st.rules else ()) + (("ex",) if st.sampling and st.sample_ex else ()) + ((("beams", st.beams, st.beam_max_rows),) if st.beams else ())
        if key not in st.graphs:
            # (a beam step is first captured at the first step of a call, where no slot holds a row that can differ yet: the one row the
            # warm-up run appends and permutes is written again by the replay)
            st.graphs[key], _ = self._capture_graph(body, restore + (() if st.logprobs is None else (st.lp_buf,)) +
                                                    ((st.seq_len, st.rule_min_left) if st.rules else ()) +
                                                    ((st.beam_score, st.beam_parent, st.beam_walk, st.beam_held) if st.beams else ()))
        st.graphs[key].replay()

    def _decode_run(self, st, cache: KVCache):
        if st.layout != self.llm_packed:                                   # pack_llm_weights / unpack_llm_weights since the capture
            st.graphs.clear()
            st.layout = self.llm_packed
        restore = (st.tok, st.pos, st.cu_k, st.step)
        if self.tp_size == 1:
            self._run_step(st, lambda: self._decode_body(st, cache), restore)
            return
        # Tensor parallel: the step holds 2 all-reduces per layer.  Through RcclComm they are plain stream-ordered RCCL launches, which
        # HIP graph capture records like any kernel (RCCL supports capture; tests/test_gpu_dist.py captures and replays
        # lmi_allreduce on the device), so the step stays ONE graph replay per token; over a torch.distributed group (gloo in the
        # CPU tests, host-staged) it cannot be captured and runs eagerly.
        from .dist import RcclComm
        comm = self.comm
        capturable = isinstance(comm, RcclComm) and self.tp_decode_graph and not st.graph_failed
        sent, keep = [], []                # comm.sent_bytes before each Python run of the body: none = a replay, two = warm-up, then capture

        def body():
            if capturable and not sent:
                keep.extend(t.clone() for t in restore)
            sent.append(comm.sent_bytes)
            self._decode_body(st, cache)
        try:
            self._run_step(st, body, restore, capturable)
        except Exception as exc:           # a communicator that cannot be captured: run the step eagerly from now on
            if len(sent) < 2:              # (not the capture: the warm-up or an eager step failed)
                raise
            import warnings
            warnings.warn(f"tensor-parallel decode step could not be captured in a HIP graph ({exc}); running it eagerly")
            st.graph_failed = True
            torch.cuda.synchronize(self.device)
            for t, v in zip(restore, keep):
                t.copy_(v)
            self._decode_body(st, cache)
            return
        if len(sent) == 2:                 # captured now: what the capture counted is what one replay puts on the links — the replay that followed
            st.graph_comm_bytes = comm.sent_bytes - sent[1]
        elif not sent:
            comm.sent_bytes += st.graph_comm_bytes

    def _decode_seed(self, st, cache: KVCache, token_id: int):
        if cache.length >= cache.capacity:
            raise RuntimeError("KV cache is full")
        st.tok.fill_(int(token_id))
        st.pos.fill_(cache.length)
        st.cu_k[1:].fill_(cache.length + 1)

    @torch.no_grad()
    def decode_step(self, token_id: int, cache: KVCache) -> torch.Tensor:
        """Append one token: returns its logits [vocab] (fp32, a view of a static buffer) and advances the cache."""
        st = self._decode_state(cache)
        st.sampling, st.sample_ex, st.logprobs, st.rules, st.beams = False, False, None, False, 0      # raw logits: never rules
        self._decode_seed(st, cache, token_id)
        self._decode_run(st, cache)
        cache.length += 1
        return st.logits[:self.cfg.text_config.vocab_size]

    def _generation_cache(self, need: int) -> KVCache:
        """ONE KV cache (with its decode state and captured graph) per engine, reused across generate() calls: the eval loop is
        batch 1 with at most 128 new tokens, and a fresh cache per sample would pay an eager warm-up step, a graph capture and new
        static buffers every time.  The graph reads the position and the key count from device memory and its launch geometry
        depends only on the capacity, so resetting ``length`` is all a new prompt needs; a longer prompt grows the cache."""
        c = self._gen_cache
        if c is None or c.capacity < need:
            c = self._gen_cache = KVCache(self.cfg, (need + 2047) // 2048 * 2048, self.dtype, self.device, tp_size=self.tp_size)
        c.length = 0
        return c

    def first_token(self, logits_last: torch.Tensor) -> int:
        """Greedy choice from prefill logits, honouring ``suppress_tokens``."""
        if self.suppress_tokens is not None:
            logits_last = logits_last.clone()
            logits_last.index_fill_(0, self.suppress_tokens, float("-inf"))
        return int(logits_last.argmax())

    def _greedy_loop(self, prompt_ids: List[int], first: int, cache: KVCache, max_new_tokens: int, eos,
                     sampling: Optional[SamplingParams] = None, lpr: Optional[_LogprobRows] = None,
                     rules: Optional[LogitsRules] = None) -> List[int]:
        """EVAL:448-452 after the prefill: greedy tokens until eos / max_new_tokens; one captured decode step per token.  With ``sampling``
        the step draws instead (the sampled graph; ``first`` was drawn at step 0).  ``lpr`` (generate(logprobs=k)): the step also writes the
        token's logprob row, read with one more small copy next to the token's."""
        out, nxt = list(prompt_ids), int(first)
        st = self._decode_state(cache)
        st.sampling, st.beams = sampling is not None, 0
        st.sample_ex = sampling is not None and sampling.extended
        self._set_logprobs(st, None if lpr is None else lpr.k)
        self._set_rules(st, rules, eos)
        if rules is not None:
            self._fill_rules(st, 0, prompt_ids, rules)
        if sampling is not None:
            self._set_sampling(st, 0, sampling)
        self._decode_seed(st, cache, nxt)
        for step in range(max_new_tokens):
            out.append(nxt)
            if nxt in eos or step == max_new_tokens - 1:
                break
            self._decode_run(st, cache)              # consumes st.tok at st.pos, leaves the next token / position on the device
            cache.length += 1
            nxt = int(st.tok.item())
            if lpr is not None:
                lp, ti, tl = self._rings_to_host(st)
                lpr.add(lp[0], ti[0], tl[0])
        return out

    def _continue_single(self, prompt: List[int], first: int, pieces, max_new_tokens: int, eos, sampling: Optional[SamplingParams],
                         lpr: Optional[_LogprobRows], rules: Optional[LogitsRules] = None) -> List[int]:
        """One request whose K / V rows are ``pieces`` (_load_rows) continued on the engine's ONE generation cache and its captured batch-1
        step: a chunk of one suffix, or the requests of a call one after another where the shape has no batched decode (toy configurations
        the skinny-M kernels do not cover)."""
        S = sum(n for _, _, n in pieces)
        cache = self._generation_cache(S + max_new_tokens)
        self._load_rows(pieces, cache.k, cache.v, 0)
        cache.length = S
        return self._greedy_loop(prompt, first, cache, max_new_tokens, eos, sampling, lpr, rules)

    @torch.no_grad()
    def generate(self, input_ids: torch.Tensor, tiles: Optional[torch.Tensor], max_new_tokens: int = 128,
                 eos_token_id: Sequence[int] = (128001, 128009), sampling: Optional[SamplingParams] = None,
                 logprobs: Optional[int] = None, rules: Optional[LogitsRules] = None):
        """Greedy generation (EVAL:448-452), or sampled with ``sampling``: returns LongTensor [1, S_in + T] on the input device.
        ``logprobs`` = k in 0 .. 8: returns a ``GenerateOutput`` — that tensor as ``sequences`` plus, for each of the T generated tokens, its
        log-probability and the k most likely tokens of its step (lmi_decode_logprobs inside the captured step).
        ``rules``: repetition penalty / no-repeat n-gram ban / min_new_tokens over the ids of ``input_ids`` (as passed: an image placeholder
        counts as its id) and the generated tokens, applied inside the step before the choice (lmi_decode_rules), the first token included.
        Not with ``logprobs``, not on tensor-parallel engines (NotImplementedError, before anything is launched)."""
        k = self._logprobs_arg("generate", logprobs)
        sampling = self._sampling_arg("generate", sampling)
        rules = self._rules_arg("generate", rules, k, eos_token_id)
        ids = input_ids.reshape(1, -1)
        S = self.merged_len(ids)
        cache = self._generation_cache((self.tp_padded_len(S) if self.tp_size > 1 else S) + max_new_tokens)
        res = self.prefill(ids, tiles, cache=cache)
        prompt, eos = [int(t) for t in ids.reshape(-1).tolist()], set(int(e) for e in eos_token_id)
        first, lpr = self._first_tokens(res.logits_last, None if sampling is None else [sampling], k, rules, [prompt], eos)
        out = self._greedy_loop(prompt, first[0], cache, max_new_tokens, eos, sampling, lpr and lpr[0], rules)
        return self._outputs([out], [input_ids], lpr, [ids.numel()], one=True)

    # ------------------------------------------------------------------------------------------------
    # f4: batched decode.  B sequences advance together: ONE pass over the weights per step serves B tokens (lmi_gemm_skinny),
    # their KV caches are slots of one pooled buffer per layer (slot b = rows [b * capacity, (b + 1) * capacity)), positions and
    # key counts live in device memory, and the whole step is ONE captured HIP graph per (B, capacity).
    # ------------------------------------------------------------------------------------------------
    MAX_DECODE_BATCH = 16              # rows of one lmi_gemm_skinny launch (one 16x16x32 MFMA column block)
    HIST = 8                           # continuous batching: decode steps between two host looks at the produced tokens
    MAX_EOS = 4                        # eos ids held on the device
    WIDE_DECODE_BATCH = 64             # rows of one lmi_gemm_skinny_wide launch (four column blocks): the most decode_batch_limit admits
    PAIR_DECODE_BATCH = 8              # hi + lo pairs of one lmi_gemm_skinny_hl launch (2 M <= 16 rows): the default decode_pair_limit
    WIDE_PAIR_DECODE_BATCH = 32        # pairs of one lmi_gemm_skinny_wide_hl launch (four column blocks): the most decode_pair_limit admits

    @property
    def decode_batch_limit(self) -> int:
        """The most sequences generate_stream / generate_batch decode in ONE captured step (default MAX_DECODE_BATCH).  Above 16 the step's
        projections and head run on the wide kernels (lmi_gemm_skinny_wide, lmi_rope_qkv_skinny_wide: M <= 64), which give every row the
        bits the 16-row kernels give it, so a request decodes to the same tokens at any width; a precision mode ("lo4" / "split") decodes
        more than decode_pair_limit sequences (default 8) on the fast step, as it does 9 .. 16.  The pooled KV cache is B x capacity rows per
        layer, and the pools of the two most recent batch sizes are kept: size the limit to the memory left beside the weights."""
        return self._decode_batch_limit

    @decode_batch_limit.setter
    def decode_batch_limit(self, value) -> None:
        if isinstance(value, bool) or not isinstance(value, int) or not 1 <= value <= self.WIDE_DECODE_BATCH:
            raise ValueError(f"decode_batch_limit must be an integer in 1 .. {self.WIDE_DECODE_BATCH}, got {value!r}")
        self._decode_batch_limit = value

    @property
    def decode_pair_limit(self) -> int:
        """The most sequences a precision mode ("lo4" / "split") decodes on the pair step (decode_hl) in generate_stream / generate_batch: 8 ..
        32, default 8 — the pairs of the 16-row kernels, with which every call launches and replays what it always did.  Above 8 sequences the
        step's projections and head run on lmi_gemm_skinny_wide_hl / lmi_rope_qkv_skinny_wide_hl (M <= 32 pairs), which give every pair the bits
        the 8-pair entries give it: a request decodes to the same tokens and log-probs at any width up to the limit.  More sequences than the
        limit (and 33 .. 64 always: 64 pairs would be 128 batch rows) decode on the fast step.  generate_shared and generate_beams keep the
        8-pair step.  Setting another value drops the pooled decode states: a step captured under one limit is never replayed under another."""
        return self._decode_pair_limit

    @decode_pair_limit.setter
    def decode_pair_limit(self, value) -> None:
        _check_pair_limit(value)
        if value != self._decode_pair_limit:
            self._batch_states = {}
        self._decode_pair_limit = value

    def _batch_decode_supported(self) -> bool:
        """lmi_gemm_skinny needs K % 128 == 0 and N % 16 == 0 (gate/up: % 64); the pooled decode attention head_dim 128."""
        W, tc = self.W, self.cfg.text_config
        (H, KV), hd, D = self._llm_heads(), tc.head_dim, tc.hidden_size
        return (hd == 128 and D % 128 == 0 and W.llm_ff % 128 == 0 and (2 * W.llm_ff) % 64 == 0 and ((H + 2 * KV) * hd) % 16 == 0 and
                W.lm_head.shape[0] % 16 == 0 and D % 16 == 0)

    def _pooled_state(self, key, fits, build, hl: bool) -> DecodeState:
        """The pooled decode state kept under ``key``: reused when it ``fits``, belongs to the current precision mode and is the pair (``hl``) or
        the fast step as the caller gets it now (decode_pair_limit, a caller's own cap), else built anew (``build``).  Bounded: a serving
        process that sees many batch sizes keeps the pools of the two most recent ones (each is B x capacity KV rows)."""
        states = self._batch_states
        st = states.get(key)
        if st is not None and fits(st) and st.mode == (self.precision, self.decode_precision) and st.hl == hl:
            return st
        st = build()
        while len(states) >= 2:
            states.pop(next(iter(states)))
        states[key] = st
        return st

    def _batch_state(self, B: int, need: int, pair_limit: Optional[int] = None) -> DecodeState:
        """Static buffers + pooled KV cache + captured graph of a B-sequence decode step (kept per engine and reused: the graph reads
        positions / key counts from device memory and its launch geometry depends on (B, capacity) only)."""
        def build():
            st = self._decode_buffers(B, (need + 1023) // 1024 * 1024, pair_limit=pair_limit)
            self._pool_buffers(st)
            return st
        return self._pooled_state(B, lambda st: st.capacity >= need, build, self.decode_hl(B, pair_limit))

    SHARED_OWN_ROWS = 256              # shared-prefix decode: a slot's own rows (question + new tokens) are rounded up to this ...
    SHARED_PREFIX_ROWS = 1024          # ... and the one prefix copy to this, so that calls of about the same shape reuse one captured step

    def _shared_decode_guard(self, B: int) -> None:
        """generate_shared(decode="shared"): the shapes lmi_attn_decode_shared serves — anything else is an error, never another path."""
        tc = self.cfg.text_config
        H, KV = self._llm_heads()
        if tc.head_dim != 128:
            raise NotImplementedError(f"generate_shared(decode='shared'): head_dim {tc.head_dim} is not supported (the shared-prefix decode attention needs 128)")
        if H != 4 * KV:
            raise NotImplementedError(f"generate_shared(decode='shared'): {H} query / {KV} KV heads are not supported (the prefix pass packs the 4 "
                                      "query heads of one KV head into a workgroup: the ratio must be 4)")
        if not self._batch_decode_supported():
            raise NotImplementedError("generate_shared(decode='shared'): this shape has no batched decode (lmi_gemm_skinny needs hidden and "
                                      "feed-forward widths that are multiples of 128)")
        if B > 32:
            raise NotImplementedError(f"generate_shared(decode='shared'): {B} sequences in one step (at most 32: one row of a 32-row tile each)")

    def _shared_state(self, B: int, need_own: int, need_prefix: int) -> DecodeState:
        """The pooled decode state of ``_batch_state`` with the prefix stored ONCE: B slots of own_capacity rows (a sequence's suffix and new
        tokens) + one prefix buffer of prefix_capacity rows per layer.  Kept per (B, own capacity, prefix capacity) next to the copy states,
        under the same bound of two retained pools; a later call whose own rows and prefix fit reuses the buffers and the captured step
        (the prefix length is a device int)."""
        def build():
            tc, dev = self.cfg.text_config, self.device
            KV, hd = self._llm_heads()[1], tc.head_dim
            own = (need_own + self.SHARED_OWN_ROWS - 1) // self.SHARED_OWN_ROWS * self.SHARED_OWN_ROWS
            pcap = (need_prefix + self.SHARED_PREFIX_ROWS - 1) // self.SHARED_PREFIX_ROWS * self.SHARED_PREFIX_ROWS
            self._batch_states.pop(("shared", B), None)                # the pool it replaces goes first: never two of one batch size
            st = self._decode_buffers(B, own, prefix_capacity=pcap, pair_limit=self.PAIR_DECODE_BATCH)
            self._pool_buffers(st)
            n_layers = len(self.W.llm_layers)
            st.kp = [torch.zeros(pcap, KV * hd, dtype=self.dtype, device=dev) for _ in range(n_layers)]
            st.vp = [torch.zeros(pcap, KV * hd, dtype=self.dtype, device=dev) for _ in range(n_layers)]
            st.prefix_capacity = pcap
            st.prefix_len = torch.ones(1, dtype=torch.int32, device=dev)
            return st
        return self._pooled_state(("shared", B), lambda st: st.capacity >= need_own and st.prefix_capacity >= need_prefix, build,
                                  self.decode_hl(B, self.PAIR_DECODE_BATCH))

    def _pool_buffers(self, st: DecodeState) -> None:
        """The pooled KV slots and the device side of continuous batching of a B-sequence decode state."""
        W, tc, dev = self.W, self.cfg.text_config, self.device
        (H, KV), hd, D = self._llm_heads(), tc.head_dim, tc.hidden_size
        B, cap = st.B, st.capacity
        n_layers = len(W.llm_layers)
        st.k = [torch.zeros(B * cap, KV * hd, dtype=self.dtype, device=dev) for _ in range(n_layers)]
        st.v = [torch.zeros(B * cap, KV * hd, dtype=self.dtype, device=dev) for _ in range(n_layers)]
        st.k_len = torch.ones(B, dtype=torch.int32, device=dev)
        st.sq_a, st.sq_b = self._empty(B, D // 16, dtype=torch.float32), self._empty(B, D // 16, dtype=torch.float32)   # folded-norm partials
        st.logits = self._empty(B, W.lm_head.shape[0], dtype=torch.float32)
        # continuous batching (generate_stream): which slots hold a running sequence, how many more tokens each may produce, the eos ids,
        # and a ring of the last HIST steps' tokens — all in device memory, so that slots are admitted / retired between replays of ONE
        # captured step and the host looks at the tokens only every HIST steps
        st.live = torch.ones(B, dtype=torch.int32, device=dev)
        st.budget = torch.full((B,), 1 << 30, dtype=torch.int32, device=dev)
        st.eos = torch.full((self.MAX_EOS,), -1, dtype=torch.int64, device=dev)
        st.hist = torch.zeros(self.HIST, B, dtype=torch.int64, device=dev)
        st.hist_pos = torch.zeros(B, dtype=torch.int32, device=dev)

    def _skinny_weights(self):
        """The decode projections + the head in lmi_gemm_skinny's packed (MFMA operand) order — a second copy of the 16-bit LLM weights
        (15 GB for Llama-3.1-8B), built on the first batched decode and shared by every batch size.  Only engines whose weights stay in
        the nn.Linear layout (tensor parallel, pack_llm_weights=False) need it: the default layout IS this order (pack_llm_weights)."""
        pk = self._skinny_pack
        if pk is None:
            from .weights import skinny_pack
            W = self.W
            # q|k|v: the rope-permuted rows when they exist (RoPE + KV append then ride in the projection's epilogue: lmi_rope_qkv_skinny)
            pk = self._skinny_pack = {"layers": [(skinny_pack(L.qkv_w_rope if L.qkv_w_rope is not None else L.qkv_w), skinny_pack(L.o_w),
                                                  skinny_pack(L.gu_w), skinny_pack(L.down_w)) for L in W.llm_layers],
                                      "head": self._skinny_head()}
        return pk

    def _skinny_layers(self, st, k_list, v_list, capacity: int, attend):
        """The layer stack of a decode step on the M <= 16 kernels (lmi_gemm_skinny*): st.x (fp32 rows) in, st.x out.  K / V rows are appended
        to k_list[i] / v_list[i] at row m * capacity + pos[m] (a shared-prefix state: minus *st.prefix_len — the slots hold own rows only);
        ``attend(i)`` runs layer i's attention from st.qkv into st.att."""
        ops, W, tc = self.ops, self.W, self.cfg.text_config
        (H, KV), hd = self._llm_heads(), tc.head_dim
        eps = tc.rms_norm_eps
        pk = None if self.llm_packed or not self.skinny_packed else self._skinny_weights()
        D, n_layers = tc.hidden_size, len(W.llm_layers)
        # folded RMSNorms (as the prefill's fused schedule): every residual projection (o_proj, down_proj) also emits T(x * gamma_next) and
        # per-row partial sums of squares, the projection that consumes them scales its accumulator rows by rstd — only the first
        # layer's norm and the final one stay launches of their own
        fold = self.skinny_fold_norm and D % 16 == 0 and all(L.qkv_w_rope is not None for L in W.llm_layers) and hd == 128
        hl = st.hl                                                    # decode precision mode: operands are [hi rows; lo rows] pairs (decode_hl)
        assert not hl or fold
        # a wide step (decode_batch_limit > 16; a pair step of more than 8, decode_pair_limit): launch for launch the same step on the
        # M <= 64 entries (pairs: M <= 32), which give every row the bits of the 16-row kernels and have no row_bias form (the shared-prefix step
        # keeps its own limits)
        wide = st.B > (self.PAIR_DECODE_BATCH if hl else self.MAX_DECODE_BATCH)
        assert not wide or st.prefix_len is None
        gemm, hlk = ((ops.gemm_skinny_wide_hl if hl else ops.gemm_skinny_wide), {}) if wide else (ops.gemm_skinny, {"hl": hl})
        norm = self._rmsnorm_rows32 if wide else ops.rmsnorm
        for i, L in enumerate(W.llm_layers):
            rope_fused = L.qkv_w_rope is not None and hd == 128
            qkv_w, o_w, gu_w, down_w = pk["layers"][i] if pk else (L.qkv_w_rope if rope_fused else L.qkv_w, L.o_w, L.gu_w, L.down_w)
            packed = None if pk is None else True            # None: as the weight is marked (weights.is_packed)
            if hl and i == 0:
                ops.rmsnorm(st.x, L.in_norm, st.hf32, eps)            # the first norm in fp32, handed over as a pair
                ops.split_rows_hl(st.hf32, st.h)
            elif not fold or i == 0:
                norm(st.x, L.in_norm, st.h, eps)
            if rope_fused and wide:
                rope_wide = ops.rope_qkv_skinny_wide_hl if hl else ops.rope_qkv_skinny_wide
                rope_wide(qkv_w, st.h, st.qkv, H, KV, hd, st.cos, st.sin, k_list[i], v_list[i], capacity, st.pos, packed,
                          rowsq_in=st.sq_b if fold and i > 0 else None, norm_eps=eps)
            elif rope_fused:
                ops.rope_qkv_skinny(qkv_w, st.h, st.qkv, H, KV, hd, st.cos, st.sin, k_list[i], v_list[i], capacity, st.pos, packed,
                                    rowsq_in=st.sq_b if fold and i > 0 else None, norm_eps=eps, hl=hl, row_bias=st.prefix_len)
            else:
                gemm(qkv_w, st.h, st.qkv, 0, packed)
                ops.rope_qk_rows(st.qkv, H, KV, hd, st.cos, st.sin, k_list[i], v_list[i], capacity, st.pos, row_bias=st.prefix_len)
            attend(i)
            if fold:
                gemm(o_w, st.att, st.x, 1, packed, norm_out=st.h, norm_gamma=L.post_norm, rowsq_out=st.sq_a, **hlk)
                gemm(gu_w, st.h, st.gu, 2, packed, rowsq_in=st.sq_a, norm_dim=D, norm_eps=eps, **hlk)
                if i + 1 < n_layers:
                    gemm(down_w, st.gu, st.x, 1, packed, norm_out=st.h, norm_gamma=W.llm_layers[i + 1].in_norm, rowsq_out=st.sq_b, **hlk)
                else:
                    gemm(down_w, st.gu, st.x, 1, packed, **hlk)
            else:
                gemm(o_w, st.att, st.x, 1, packed)
                norm(st.x, L.post_norm, st.h, eps)
                gemm(gu_w, st.h, st.gu, 2, packed)
                gemm(down_w, st.gu, st.x, 1, packed)

    def _rmsnorm_rows32(self, x, gamma, out, eps) -> None:
        """lmi_rmsnorm over the rows of a wide step, at most 32 per launch: up to 32 rows it takes its few-rows kernel, above them one
        wave per row, which adds the squares in another order — in chunks a slot keeps the bits it has in a step of at most 16."""
        for r0 in range(0, x.shape[0], 32):
            self.ops.rmsnorm(x[r0:r0 + 32], gamma, out[r0:r0 + 32], eps)

    def _skinny_head(self):
        """lm_head in the packed order for the batched step (shared with _skinny_weights' second copy when there is one)."""
        h = self._head_pack
        if h is None:
            from .weights import as_packed
            pk = self._skinny_pack
            h = self._head_pack = as_packed(pk["head"]) if pk else as_packed(self.W.lm_head)
        return h

    def _batch_decode_body(self, st):
        """One decode step for the B sequences of ``st`` (everything here is host-value free: graph-capturable)."""
        ops, W, tc = self.ops, self.W, self.cfg.text_config
        (H, KV), hd = self._llm_heads(), tc.head_dim
        qw, eps = H * hd, tc.rms_norm_eps
        ops.embed_merge(st.tok, st.src, W.embed, None, st.x)
        if st.kp is not None:                                         # shared prefix: one walk over the prefix rows serves all B rows
            attend = lambda i: ops.attention_decode_shared(st.qkv[:, :qw], st.kp[i], st.vp[i], st.prefix_len, st.prefix_capacity, st.k[i], st.v[i],
                                                           st.att, st.k_begin, st.k_len, st.capacity, H, KV, hd, hd ** -0.5, st.ws, n_seq=st.B,
                                                           hl=st.hl)
        else:
            attend = lambda i: ops.attention_decode_pool(st.qkv[:, :qw], st.k[i], st.v[i], st.att, st.cu_q, st.k_begin, st.k_len, st.capacity,
                                                         H, KV, hd, hd ** -0.5, st.ws, window=tc.sliding_window or 0, hl=st.hl)
        self._skinny_layers(st, st.k, st.v, st.capacity, attend)
        # head: one pass over lm_head for all B rows (lmi_lm_head_last streams the 1 GB head once PER row), from a packed copy of the head
        # (1 GB, built on the first batched step: the prefill's and the batch-1 step's head kernels read the nn.Linear layout; B = 8 step
        # 3.29 ms against 3.37 ms from the row-major head in the coalescing lane order)
        if st.hl:                                                     # decode precision mode: the head's operand as a pair too (the batch-1 step's head reads the fp32 row)
            ops.rmsnorm(st.x, W.final_norm, st.hf32, eps)
            ops.split_rows_hl(st.hf32, st.h)
            head = self._skinny_head() if self.skinny_packed else W.lm_head
            if st.B > self.PAIR_DECODE_BATCH:                         # a wide pair step (decode_pair_limit): the head on the M <= 32 pair entry
                ops.gemm_skinny_wide_hl(head, st.h, st.logits, 3)
            else:
                ops.gemm_skinny(head, st.h, st.logits, 3, hl=True)
        elif st.B > self.MAX_DECODE_BATCH:                            # a wide step: the final norm in chunks, the head on the M <= 64 entry
            self._rmsnorm_rows32(st.x, W.final_norm, st.h, eps)
            ops.gemm_skinny_wide(self._skinny_head() if self.skinny_packed else W.lm_head, st.h, st.logits, 3)
        else:
            ops.rmsnorm(st.x, W.final_norm, st.h, eps)
            ops.gemm_skinny(self._skinny_head() if self.skinny_packed else W.lm_head, st.h, st.logits, 3)
        # greedy choice, history ring, stop rule (eos ids / token budget) and position advance of all B slots: ONE launch, device memory only —
        # a slot that stopped freezes (live = 0) and what it produces afterwards is ignored (lmi_decode_advance)
        self._choose(st, st.logits, k_len=st.k_len, live=st.live, budget=st.budget, eos=st.eos, hist=st.hist, hist_pos=st.hist_pos)

    def _batch_decode_run(self, st):
        self._run_step(st, lambda: self._batch_decode_body(st), (st.tok, st.pos, st.k_len, st.live, st.budget, st.hist, st.hist_pos, st.step))

    def _greedy_loop_batch(self, st, prompts: List[List[int]], first: List[int], seq_lens: List[int], max_new_tokens: int, eos,
                           sampling: Optional[Sequence[SamplingParams]] = None, own_lens: Optional[List[int]] = None,
                           lpr: Optional[Sequence[_LogprobRows]] = None, rules: Optional[LogitsRules] = None) -> List[List[int]]:
        """EVAL:448-452 for B sequences at once: every sequence follows exactly the batch-1 rule (emit, stop at eos / max_new_tokens);
        finished sequences keep riding along in the batch (their slots are private) and are ignored.  ``own_lens`` (a shared-prefix state):
        the rows each slot holds — the key count starts there, the position at seq_lens.  ``lpr`` (logprobs=k): the steps also fill the
        logprob rings, drained once per HIST steps (step n writes slot n % HIST); a stopped slot keeps writing and its rows are dropped by
        the rule that drops its tokens (``_LogprobRows.result`` keeps a request's first T rows)."""
        B = st.B
        outs = [list(p) for p in prompts]
        nxt = [int(f) for f in first]
        done = [False] * B
        st.tok.copy_(torch.tensor(nxt, dtype=torch.int64))
        st.pos.copy_(torch.tensor(seq_lens, dtype=torch.int32))
        st.k_len.copy_(torch.tensor([s + 1 for s in (own_lens or seq_lens)], dtype=torch.int32))
        st.live.fill_(1); st.budget.fill_(1 << 30); st.eos.fill_(-1); st.hist_pos.zero_()      # the host applies the stop rule here
        st.sampling, st.beams = sampling is not None, 0
        st.sample_ex = any(sp.extended for sp in sampling or ())
        self._set_logprobs(st, None if lpr is None else lpr[0].k)
        self._set_rules(st, rules, eos)
        if rules is not None:
            for j, p in enumerate(prompts):
                self._fill_rules(st, j, p, rules)
        for j, sp in enumerate(sampling or ()):
            self._set_sampling(st, j, sp)
        undrained = 0                                                 # steps whose ring slots 0 .. undrained - 1 the host has not read yet

        def drain():
            lp, ti, tl = self._rings_to_host(st)
            for j in range(B):
                lpr[j].add(lp[:undrained, j], ti[:undrained, j], tl[:undrained, j])
        for step in range(max_new_tokens):
            for j in range(B):
                if not done[j]:
                    outs[j].append(nxt[j])
                    if nxt[j] in eos or step == max_new_tokens - 1:
                        done[j] = True
            if all(done):
                break
            self._batch_decode_run(st)
            nxt = [int(t) for t in st.tok.tolist()]
            if lpr is not None:
                undrained += 1
                if undrained == self.HIST:
                    drain()
                    undrained = 0
        if lpr is not None and undrained:
            drain()
        return outs

    def release_batch_state(self) -> None:
        """Free the pooled KV caches / captured graphs of the batched decode and — for engines that keep the nn.Linear layout (tensor
        parallel, pack_llm_weights=False) — the second copy of the LLM weights in the skinny-M operand order (15 GB for Llama-3.1-8B;
        rebuilt on the next batched call).  The default layout has no second copy: prefill, batch-1 and batched decode read the same
        packed tensors (pack_llm_weights)."""
        self._batch_states = {}
        self._skinny_pack = None
        self._head_pack = None
        if self.device.type == "cuda":
            torch.cuda.empty_cache()

    @torch.no_grad()
    def generate_stream(self, samples: Sequence[Tuple[torch.Tensor, Optional[torch.Tensor]]], batch_size: int = 8, max_new_tokens: int = 128,
                        eos_token_id: Sequence[int] = (128001, 128009), stats: Optional[dict] = None,
                        sampling: Optional[SamplingParams] = None, logprobs: Optional[int] = None, rules: Optional[LogitsRules] = None):
        """CONTINUOUS batching (the reference loop EVAL:381-452 is one generate() per record): ``batch_size`` decode slots,
        ONE captured step per token for all of them, and a slot that finishes (eos / max_new_tokens) is handed to the next pending sample
        — prefill of the newcomer, its K / V rows copied into the slot of the pooled cache, five small device writes — without
        re-capturing anything: positions, key counts, the live mask, the token budget and the eos ids all live in device memory, and the
        stop rule runs on the device.  The host reads the produced tokens every HIST steps (one copy of a [HIST, B] table) instead of
        one blocking read per token; a slot that stopped inside the window idles until the window ends (its state is frozen).
        Returns the outputs in input order, each exactly what ``generate`` returns for that sample (same rule; the batched projections sum
        in a different order than the batch-1 GEMVs, so a token can differ only on a near tie of the top two logits).
        ``stats`` (optional dict) receives steps / slot-steps / live slot-steps for occupancy accounting.
        ``sampling``: sampled decoding; request i draws with ``sampling.for_request(i)``, so its tokens do not depend on ``batch_size``.
        ``logprobs`` = k in 0 .. 8: returns a ``GenerateOutput`` (``sequences`` = that list); the logprob rings are read once per window, with
        the token table.  ``rules``: as ``generate``, one value for every request of the call; a slot's ids and countdown are set when it
        admits a request."""
        k = self._logprobs_arg("generate_stream", logprobs)
        sampling = self._sampling_arg("generate_stream", sampling)
        rules = self._rules_arg("generate_stream", rules, k, eos_token_id)
        assert self.tp_size == 1, "batched generation is a single-rank feature (replicas scale it out)"
        B = max(1, min(int(batch_size), self.decode_batch_limit, len(samples)))
        eos = [int(e) for e in eos_token_id]
        req = (lambda i: None) if sampling is None else sampling.for_request
        if B == 1 or not self._batch_decode_supported() or len(eos) > self.MAX_EOS:
            one = [self.generate(ids, t() if callable(t) else t, max_new_tokens, eos, sampling=req(i), logprobs=k, rules=rules)
                   for i, (ids, t) in enumerate(samples)]
            return one if k is None else GenerateOutput.join(one)
        need = max(self.merged_len(ids) for ids, _ in samples) + max_new_tokens
        st = self._batch_state(B, need)
        st.eos.fill_(-1)
        if eos:
            st.eos[:len(eos)].copy_(torch.tensor(eos, dtype=torch.int64))
        st.live.zero_(); st.budget.zero_(); st.pos.zero_(); st.k_len.fill_(1); st.tok.zero_(); st.hist_pos.zero_()
        st.sampling, st.beams = sampling is not None, 0
        st.sample_ex = sampling is not None and sampling.extended
        self._set_logprobs(st, k)
        self._set_rules(st, rules, eos)
        lpr = None if k is None else [None] * len(samples)          # a request's rows start with its first token's (admit)
        eos_set = set(eos)
        outs: List[Optional[List[int]]] = [None] * len(samples)
        slot_sample = [-1] * B                                       # which sample a slot runs (-1: free)
        h_budget = [0] * B                                           # host mirror of the device stop rule
        pending = list(range(len(samples)))
        n_steps = slot_steps = live_steps = 0
        scratch = self._stream_cache

        def admit(j: int) -> bool:
            """Next pending sample into slot j; False when nothing is pending.  Samples that end with their first token never take a slot."""
            nonlocal scratch
            while pending:
                i = pending.pop(0)
                ids, tiles = samples[i]
                if callable(tiles):                                   # lazy pixels: prepared when the sample is admitted, dropped after its prefill
                    tiles = tiles()
                S = self.merged_len(ids)
                if scratch is None or scratch.capacity < S:
                    scratch = self._stream_cache = KVCache(self.cfg, (S + 1023) // 1024 * 1024, self.dtype, self.device)
                scratch.length = 0
                res = self.prefill(ids.reshape(1, -1), tiles, cache=scratch)
                prompt = [int(t) for t in ids.reshape(-1).tolist()]
                (first,), rows = self._first_tokens(res.logits_last, None if sampling is None else [req(i)], k, rules, [prompt], eos_set)
                outs[i] = prompt + [first]
                if lpr is not None:
                    lpr[i] = rows[0]
                if first in eos_set or max_new_tokens <= 1:
                    continue                                          # finished by the prefill alone
                self._move_kv(scratch, 0, S, st.k, st.v, j * st.capacity)
                dev = self.device
                st.tok[j:j + 1].copy_(torch.tensor([first], dtype=torch.int64, device=dev))
                st.pos[j:j + 1].copy_(torch.tensor([S], dtype=torch.int32, device=dev))
                st.k_len[j:j + 1].copy_(torch.tensor([S + 1], dtype=torch.int32, device=dev))
                st.budget[j:j + 1].copy_(torch.tensor([max_new_tokens - 1], dtype=torch.int32, device=dev))
                st.live[j:j + 1].fill_(1)
                if sampling is not None:
                    self._set_sampling(st, j, req(i))
                if rules is not None:
                    self._fill_rules(st, j, prompt, rules)
                slot_sample[j], h_budget[j] = i, max_new_tokens - 1
                return True
            return False

        for j in range(B):
            admit(j)
        while any(i >= 0 for i in slot_sample):
            window = self.HIST
            st.hist_pos.zero_()
            for _ in range(window):
                self._batch_decode_run(st)
            toks = st.hist.tolist()                                   # ONE host read per window: [HIST][B]
            if lpr is not None:                                       # ... and one of the logprob rings, filled slot for slot with it
                r_lp, r_ti, r_tl = self._rings_to_host(st)
            n_steps += window
            for w in range(window):
                for j in range(B):
                    i = slot_sample[j]
                    slot_steps += 1
                    if i < 0:
                        continue
                    live_steps += 1
                    t = int(toks[w][j])
                    outs[i].append(t)
                    if lpr is not None:
                        lpr[i].add(r_lp[w, j], r_ti[w, j], r_tl[w, j])
                    h_budget[j] -= 1
                    if t in eos_set or h_budget[j] <= 0:
                        slot_sample[j] = -1                           # retired: the device froze it at this very step
            for j in range(B):
                if slot_sample[j] < 0:
                    admit(j)
        if stats is not None:
            stats.update(steps=n_steps, slot_steps=slot_steps, live_slot_steps=live_steps, batch_size=B)
        return self._outputs(outs, [ids for ids, _ in samples], lpr, [ids.numel() for ids, _ in samples])

    @torch.no_grad()
    def generate_batch(self, samples: Sequence[Tuple[torch.Tensor, Optional[torch.Tensor]]], max_new_tokens: int = 128,
                       eos_token_id: Sequence[int] = (128001, 128009), sampling: Optional[SamplingParams] = None,
                       _first_request: int = 0, logprobs: Optional[int] = None, rules: Optional[LogitsRules] = None):
        """Several samples per call (batching with per-sample cu_seqlens instead of one sample per generate()):
        ONE packed prefill — all ViT inputs through the tower together, all merged sequences in one varlen causal pass that also
        writes every sample's K/V into a packed cache — then each sample's K/V rows move to its slot of the pooled decode cache (a
        device copy) and ALL samples continue greedily together, one captured decode step per token for the whole batch
        (``_batch_decode_body``: the weight stream of a step is shared by the batch).  Same RULE as per-sample ``generate`` and numerically
        equivalent, not bit-identical: the first new token comes from the same prefill, the continuation's projections are MFMA tiles with folded
        norms instead of the batch-1 FMA chains, so a greedy choice can differ where the top two logits are within the 16-bit noise (the GPU
        tests assert equality and, where it fails, exactly such a near tie).
        ``sampling``: sampled decoding, request i with ``sampling.for_request(i)`` (as generate_stream).
        ``logprobs`` = k in 0 .. 8: returns a ``GenerateOutput`` (``sequences`` = that list); the rings are drained once per HIST steps.
        ``rules``: as ``generate``, one value for every request of the call."""
        k = self._logprobs_arg("generate_batch", logprobs)
        sampling = self._sampling_arg("generate_batch", sampling)
        rules = self._rules_arg("generate_batch", rules, k, eos_token_id)
        assert self.tp_size == 1, "batched generation is a single-rank feature (replicas scale it out)"
        # more samples than one step decodes (decode_batch_limit; 16 where the shape has no batched decode): one call per group
        limit = self.decode_batch_limit if self._batch_decode_supported() else self.MAX_DECODE_BATCH
        if len(samples) > limit:
            outs = [self.generate_batch(samples[i:i + limit], max_new_tokens, eos_token_id, sampling, _first_request + i, k, rules)
                    for i in range(0, len(samples), limit)]
            return [o for part in outs for o in part] if k is None else GenerateOutput.join(outs)
        req = (lambda i: None) if sampling is None else (lambda i: sampling.for_request(_first_request + i))
        if len(samples) > self.MAX_DECODE_BATCH:
            return self._generate_batch_wide(samples, max_new_tokens, eos_token_id, sampling, req, k, rules)
        if len(samples) == 1:
            ids, t = samples[0]
            one = self.generate(ids, t, max_new_tokens, eos_token_id, sampling=req(0), logprobs=k, rules=rules)
            return [one] if k is None else GenerateOutput.join([one])
        x, seq_lens = self._pack_requests(samples)
        packed = KVCache(self.cfg, sum(seq_lens), self.dtype, self.device)
        last, _ = self.llm_prefill(x, seq_lens, cache=packed)
        prompts = [[int(t) for t in ids.reshape(-1).tolist()] for ids, _ in samples]
        eos = set(int(e) for e in eos_token_id)
        first, lpr = self._first_tokens(last, None if sampling is None else [req(j) for j in range(last.shape[0])], k, rules, prompts, eos)
        offs = [0] + [int(c) for c in np.cumsum(seq_lens)]
        if not self._batch_decode_supported():
            outs = [self._continue_single(prompts[j], first[j], [(packed, offs[j], S)], max_new_tokens, eos, req(j), lpr and lpr[j], rules)
                    for j, S in enumerate(seq_lens)]
        else:
            st = self._batch_state(len(samples), max(seq_lens) + max_new_tokens)
            for j, S in enumerate(seq_lens):
                self._load_rows([(packed, offs[j], S)], st.k, st.v, j * st.capacity)
            del packed
            outs = self._greedy_loop_batch(st, prompts, first, seq_lens, max_new_tokens, eos,
                                           None if sampling is None else [req(j) for j in range(len(samples))], lpr=lpr, rules=rules)
        return self._outputs(outs, [ids for ids, _ in samples], lpr, [len(p) for p in prompts])

    def _generate_batch_wide(self, samples, max_new_tokens: int, eos_token_id, sampling, req, k, rules):
        """generate_batch for 17 .. decode_batch_limit samples: ONE pooled decode state for all of them.  The packed prefill still runs in
        groups of at most MAX_DECODE_BATCH samples (its workspace grows with the packed rows: 64 prompts of the C3 size would need tens of
        GB), each group's K / V rows move to their slots of the one pool, and all samples decode together."""
        G = self.MAX_DECODE_BATCH
        seq_all = [self.merged_len(ids) for ids, _ in samples]
        st = self._batch_state(len(samples), max(seq_all) + max_new_tokens)
        prompts = [[int(t) for t in ids.reshape(-1).tolist()] for ids, _ in samples]
        eos = set(int(e) for e in eos_token_id)
        first: List[int] = []
        lpr = None if k is None else []
        for g0 in range(0, len(samples), G):
            group = samples[g0:g0 + G]
            x, seq_lens = self._pack_requests(group)
            packed = KVCache(self.cfg, sum(seq_lens), self.dtype, self.device)
            last, _ = self.llm_prefill(x, seq_lens, cache=packed)
            f, rows = self._first_tokens(last, None if sampling is None else [req(g0 + j) for j in range(len(group))], k, rules,
                                         prompts[g0:g0 + G], eos)
            first += f
            if lpr is not None:
                lpr += rows
            offs = [0] + [int(c) for c in np.cumsum(seq_lens)]
            for j, S in enumerate(seq_lens):
                self._load_rows([(packed, offs[j], S)], st.k, st.v, (g0 + j) * st.capacity)
            del packed
        outs = self._greedy_loop_batch(st, prompts, first, seq_all, max_new_tokens, eos,
                                       None if sampling is None else [req(j) for j in range(len(samples))], lpr=lpr, rules=rules)
        return self._outputs(outs, [ids for ids, _ in samples], lpr, [len(p) for p in prompts])

    # ------------------------------------------------------------------------------------------------
    # Continuing from a cached prefix: N new row ranges against rows that are already in a KV cache.  ``extend`` fans one read-only prefix
    # out to N packed text suffixes (the two-range attention launch, csrc/attention.h PREFIX: the prefix K / V are read in place, never
    # copied per suffix); ``append`` grows one cache in place by n rows (multi-turn); ``generate_shared`` = one prefill of the shared
    # prompt head (the vision tower runs once) + extend + the unchanged batched decode.
    # ------------------------------------------------------------------------------------------------
    def _continuation_guard(self, what: str) -> None:
        tc = self.cfg.text_config
        if self.tp_size > 1:
            raise NotImplementedError(f"{what}: tensor-parallel engines are not supported (the two-range attention launch runs on one rank)")
        if self.fp8 is not None:
            raise NotImplementedError(f"{what}: the fp8 schedule is not supported (its attention operands have no prefix form); use 'fast' or 'lo4'")
        if self.split_operands:
            raise NotImplementedError(f"{what}: precision 'split' is not supported (its attention hands over fp32 rows); use 'fast' or 'lo4'")
        if (tc.sliding_window or 0) > 0:
            raise NotImplementedError(f"{what}: sliding_window = {tc.sliding_window} is not supported (the prefix range has no window)")

    def _text_suffixes(self, what: str, suffixes) -> List[torch.Tensor]:
        out = []
        for j, ids in enumerate(suffixes):
            ids = ids.reshape(1, -1)
            if ids.numel() == 0:
                raise ValueError(f"{what}: suffix {j} is empty")
            if bool((ids == self.cfg.image_token_index).any()):
                raise ValueError(f"{what}: suffix {j} holds an image token (images belong to the prefix)")
            out.append(ids)
        if not out:
            raise ValueError(f"{what}: no suffix")
        return out

    def _continuation_geometry(self, P: int, lens: Sequence[int]):
        """sequence_geometry for rows that start at position P of their sequence: cu_seqlens, RoPE tables of positions P .. P + l - 1, last rows."""
        key = ("ext", int(P), tuple(int(l) for l in lens))
        hit = self._geom_cache.get(key)
        if hit is None:
            cu_list = [0] + [int(c) for c in np.cumsum(key[2])]
            cu = torch.tensor(cu_list, dtype=torch.int32, device=self.device)
            cos, sin = self.rope_tables(torch.cat([torch.arange(P, P + l) for l in key[2]]))
            last_rows = torch.tensor([c - 1 for c in cu_list[1:]], device=self.device)
            if len(self._geom_cache) > 64:
                self._geom_cache.clear()
            hit = self._geom_cache[key] = (cu, cos, sin, last_rows, cu_list)
        return hit

    ATTENTION_MODES = ("ranges", "rows")
    # score_shared / loglikelihood_shared with attention=None: "rows" wherever lmi_attn_prefix_rows serves the request, "ranges" elsewhere.  Measured
    # (profiles/score_shared.json; README "Scoring from a cached prefix"): "rows" is ahead of "ranges" by 2.0 - 3.9 ms at N = 4 and at N = 16, more
    # than the 0.3 - 0.8 ms round-to-round spread of "ranges" there
    SCORE_SHARED_ATTENTION = "rows"

    def _attention_mode(self, what: str, attention: str) -> None:
        if attention not in self.ATTENTION_MODES:
            raise ValueError(f"{what}: attention must be 'ranges' or 'rows', got {attention!r}")

    def _rows_attention_refusal(self, lens: Sequence[int]) -> Optional[str]:
        """Why lmi_attn_prefix_rows cannot serve suffixes of these lengths on this model, or None."""
        (H, KV), hd = self._llm_heads(), self.cfg.text_config.head_dim
        if hd != 128:
            return f"attention='rows' needs head_dim 128 (this model: {hd})"
        if H != 4 * KV:
            return (f"attention='rows' packs the 4 query heads of one KV head into a workgroup — the ratio must be 4 (this model: {H} query / "
                    f"{KV} KV heads)")
        if self.lo4 and any(self.lo4_tail_rows(l) != l for l in lens):
            return (f"attention='rows' under precision 'lo4' hands its fp32 rows to lmi_split_lo4, which has no row selection: every suffix must "
                    f"be corrected whole (<= LO4_FULL_BELOW = {self.LO4_FULL_BELOW} rows under lo4_rows = 'auto'); the suffix lengths are {list(lens)}")
        return None

    def _rows_attention_guard(self, what: str, lens: Sequence[int]) -> None:
        """attention="rows": the shapes lmi_attn_prefix_rows serves — anything else is an error, never another launch."""
        why = self._rows_attention_refusal(lens)
        if why is not None:
            raise NotImplementedError(f"{what}: {why}")

    def _rows_attention(self, P: int, lens: Sequence[int]):
        """(k_begin, k_len, max_k_len, workspace, fp32 rows or None) of the row-packed launch over the packed suffix rows: row i of suffix j
        sees the own rows cu[j] .. cu[j] + i — causality as a key count.  The own pass re-reads a suffix's keys once per row: O(s^2)."""
        key = ("rows", tuple(int(l) for l in lens))
        hit = self._geom_cache.get(key)
        if hit is None:
            starts = np.cumsum([0] + list(key[1][:-1]))
            k_begin = np.concatenate([np.full(l, b, dtype=np.int32) for l, b in zip(key[1], starts)])
            k_len = np.concatenate([np.arange(1, l + 1, dtype=np.int32) for l in key[1]])
            if len(self._geom_cache) > 64:
                self._geom_cache.clear()
            hit = self._geom_cache[key] = (torch.from_numpy(k_begin).to(self.device), torch.from_numpy(k_len).to(self.device))
        (H, _), hd = self._llm_heads(), self.cfg.text_config.head_dim
        S, max_k = sum(key[1]), max(key[1])
        ws = self._empty(self.ops.prefix_rows_workspace_elems(S, H, hd, P, max_k), dtype=torch.float32)
        o32 = self._empty(S, H * hd, dtype=torch.float32) if self.lo4 else None
        return hit[0], hit[1], max_k, ws, o32

    def _suffix_targets(self, what: str, sfx: List[torch.Tensor], targets) -> List[np.ndarray]:
        """Host int64 targets per suffix after the checks that must fail before any launch: one per suffix row, ids in [0, V) or -100."""
        V, out = self.cfg.text_config.vocab_size, []
        for j, (ids, t) in enumerate(zip(sfx, targets)):
            t = torch.as_tensor(t).detach().to("cpu", torch.int64).reshape(-1).numpy()
            if len(t) != ids.numel():
                raise ValueError(f"{what}: request {j} has {ids.numel()} suffix ids and {len(t)} targets (one target per suffix row; "
                                 f"{self.IGNORE_INDEX} = not scored)")
            bad = np.nonzero((t != self.IGNORE_INDEX) & ((t < 0) | (t >= V)))[0]
            if len(bad):
                raise ValueError(f"{what}: targets must be token ids in [0, {V}) or {self.IGNORE_INDEX}: request {j}, targets[{int(bad[0])}] = "
                                 f"{int(t[bad[0]])}")
            out.append(t)
        return out

    def _extend_score_plan(self, what: str, requests, attention: str):
        """Everything extend_score refuses, checked on the host: (suffixes, their lengths, targets)."""
        self._attention_mode(what, attention)
        self._continuation_guard(what)
        sfx = self._text_suffixes(what, [r[0] for r in requests])
        tgts = self._suffix_targets(what, sfx, [r[1] for r in requests])
        lens = [int(t.numel()) for t in sfx]
        if self.cfg.text_config.head_dim != 128:
            raise NotImplementedError(f"{what}: the two-range attention launch needs head_dim 128")
        if attention == "rows":
            self._rows_attention_guard(what, lens)
        return sfx, lens, tgts

    @torch.no_grad()
    def extend_score(self, prefix: KVCache, requests: Sequence[tuple], attention: str = "ranges", _plan=None) -> List[ScoreResult]:
        """Score rows that continue ONE cached prefix: ``requests`` = [(suffix_ids [1, s_j], targets [1, s_j])], text ids only.  The suffix
        rows run as in ``extend`` (positions P .. P + s_j - 1, the prefix read in place and never written — the call can be repeated on the
        same cache); ``targets[i]`` is the id that suffix row i PREDICTS — already shifted, unlike the ``labels`` of ``score``, which are
        aligned with the ids and shifted inside — and -100 marks a row that is not scored.  The scored rows go through the chunked head of
        ``score`` (no [rows, V] tensor beyond one chunk); under lo4 they are in the row selection.  ScoreResult.rows are suffix-relative,
        seq_len is s_j; a request without a scored row gives the empty result of ``score``.  ``attention``: as ``extend``.  Every error is
        raised before anything is launched."""
        sfx, lens, tgts = self._extend_score_plan("extend_score", requests, attention) if _plan is None else _plan
        P = int(prefix.length)
        if P < 1:
            raise ValueError("extend_score: the prefix cache is empty (prefill it first)")
        rows = [np.nonzero(t != self.IGNORE_INDEX)[0].astype(np.int64) for t in tgts]
        if not any(len(r) for r in rows):
            return [self._empty_score(l) for l in lens]
        offs = np.cumsum([0] + lens[:-1])
        rows_all = np.concatenate([r + o for r, o in zip(rows, offs)])
        tgt_all = np.concatenate([t[r] for t, r in zip(tgts, rows)])
        x = self.embed_merge(torch.cat(sfx, dim=1) if len(sfx) > 1 else sfx[0], None)       # text ids only: one row per id, the suffixes packed
        cu, cos, sin, _, _ = self._continuation_geometry(P, lens)
        self.llm_packed
        self.last_lo4_ranges = None
        self._llm_layers(x, None, cu, cos, sin, max(lens), lens, extra_rows=rows_all, prefix=prefix,
                         rows_att=self._rows_attention(P, lens) if attention == "rows" else None)
        rows_dev = torch.from_numpy(rows_all).to(self.device)
        tgt_dev = torch.from_numpy(tgt_all).to(self.device)
        lp, am = self._score_head(x, rows_dev, tgt_dev)
        out, k = [], 0
        for r, o, l in zip(rows, offs, lens):
            m = len(r)
            if m:
                loss = (-lp[k:k + m].to(torch.float64).mean()).to(torch.float32)
                out.append(ScoreResult(loss, lp[k:k + m], am[k:k + m], tgt_dev[k:k + m], rows_dev[k:k + m] - int(o), l))
            else:
                out.append(self._empty_score(l))
            k += m
        return out

    @torch.no_grad()
    def score_shared(self, prefix_ids: torch.Tensor, tiles: Optional[torch.Tensor], requests: Sequence[tuple], prefix: Optional[KVCache] = None,
                     attention: Optional[str] = None) -> List[ScoreResult]:
        """Rank N continuations of one prompt head: ``prefix_ids`` (with all the images, ``tiles``) is prefilled ONCE — or ``prefix`` is a
        cache a ``prefill(prefix_ids, tiles, cache=prefix)`` filled, as in ``generate_shared`` — then ONE ``extend_score`` scores
        ``requests`` = [(tail_ids [1, t_j >= 0], continuation_ids [1, m_j >= 1])]: suffix j is [tail_j ; c_0 .. c_{m-2}], its targets are
        -100 on every tail row but the last, then c_0 .. c_{m-1} (the last tail row predicts c_0).  When some tail is empty, the last prefix
        id moves into every suffix and the prefix is prefilled one row shorter (it must be a text token); with ``prefix`` given that row
        cannot be produced: ValueError.  ``attention``: as ``extend``; None = SCORE_SHARED_ATTENTION ("rows") where that launch serves the model
        and the suffix lengths, "ranges" where it does not — an explicit "rows" is never replaced.  ScoreResult.rows are suffix-relative."""
        what = "score_shared"
        if attention is not None:
            self._attention_mode(what, attention)
        self._continuation_guard(what)
        pids = prefix_ids.reshape(1, -1)
        if pids.numel() == 0:
            raise ValueError("score_shared: the prefix is empty")
        if not len(requests):
            raise ValueError("score_shared: no request")
        # the request ids are a few each and every check reads them: they stay on the host until the one embedding launch
        tails = [torch.as_tensor(r[0]).reshape(1, -1).to("cpu", torch.int64) for r in requests]
        conts = [torch.as_tensor(r[1]).reshape(1, -1).to("cpu", torch.int64) for r in requests]
        for j, c in enumerate(conts):
            if c.numel() == 0:
                raise ValueError(f"score_shared: request {j} has an empty continuation")
        if any(t.numel() == 0 for t in tails):
            if prefix is not None:
                raise ValueError("score_shared: an empty tail needs the row of the last prefix id, which a given prefix cache no longer "
                                 "provides (pass that id as the tail and a cache of the shorter prefix)")
            moved = pids[:, -1:].to("cpu", torch.int64)
            if int(moved) == self.cfg.image_token_index:
                raise ValueError("score_shared: with an empty tail the last prefix id moves into the suffixes — it must be a text token")
            pids = pids[:, :-1]
            if pids.numel() == 0:
                raise ValueError("score_shared: the prefix is empty once its last id has moved into the suffixes")
            tails = [torch.cat([moved, t], dim=1) for t in tails]
        ext = []
        for t, c in zip(tails, conts):
            ign = torch.full((1, t.numel() - 1), self.IGNORE_INDEX, dtype=torch.int64)
            ext.append((torch.cat([t, c[:, :-1]], dim=1), torch.cat([ign, c], dim=1)))
        if attention is None:
            refused = self._rows_attention_refusal([int(e[0].numel()) for e in ext]) if self.SCORE_SHARED_ATTENTION == "rows" else None
            attention = self.SCORE_SHARED_ATTENTION if refused is None else "ranges"
        plan = self._extend_score_plan(what, ext, attention)
        P = self.merged_len(pids)
        if prefix is None:
            prefix = KVCache(self.cfg, P, self.dtype, self.device)
            self.prefill(pids, tiles, cache=prefix)
        elif prefix.length != P:
            raise ValueError(f"score_shared: the prefix cache holds {prefix.length} rows, prefix_ids merge to {P}")
        return self.extend_score(prefix, ext, attention=attention, _plan=plan)

    @torch.no_grad()
    def extend(self, prefix: KVCache, suffixes: Sequence[torch.Tensor], kv_out: Optional[KVCache] = None, attention: str = "ranges") -> ExtendResult:
        """Run N text-only suffixes ([1, s_j] ids, s_j >= 1) against ONE cached prefix: ``prefix`` is any cache a ``prefill(ids, tiles,
        cache=...)`` filled (P = prefix.length rows).  The suffix rows are embedded, packed, rotated at positions P .. P + s_j - 1 and run
        through the layers of the current precision ("fast" or "lo4"); their attention sees [the P prefix rows ; their own rows] through the
        two-range launch, so the prefix K / V are read in place once per layer whatever N is.  ``kv_out`` receives the suffixes' K / V at
        packed row offsets (kv_out.length = sum s_j).  ``prefix`` is never written: it can be extended any number of times.  Under lo4 the
        row selection applies to the suffix lengths (a suffix of <= LO4_FULL_BELOW rows is corrected whole); the prefix rows keep the
        schedule of their own prefill.  Not bit-identical to a from-scratch prefill of [prefix ; suffix] (another key-tile partition unless
        P % 64 == 0, and another row selection); held to the same tolerances against the fp32 oracle.
        ``attention``: "ranges" (the default) is that two-range launch; "rows" the row-packed one (lmi_attn_prefix_rows; _rows_attention_guard:
        NotImplementedError for a shape it cannot serve, never another launch silently) — meant for many SHORT suffixes."""
        self._attention_mode("extend", attention)
        self._continuation_guard("extend")
        P = int(prefix.length)
        if P < 1:
            raise ValueError("extend: the prefix cache is empty (prefill it first)")
        sfx = self._text_suffixes("extend", suffixes)
        lens = [int(t.numel()) for t in sfx]
        S = sum(lens)
        if kv_out is not None:
            if kv_out is prefix:
                raise ValueError("extend: kv_out must not be the prefix cache (extend never writes into the prefix; see append)")
            if kv_out.capacity < S:
                raise ValueError(f"extend: kv_out holds {kv_out.capacity} rows, the suffixes have {S}")
        if self.cfg.text_config.head_dim != 128:
            raise NotImplementedError("extend: the two-range attention launch needs head_dim 128")
        if attention == "rows":
            self._rows_attention_guard("extend", lens)
        xs = [self.embed_merge(t, None) for t in sfx]
        x = torch.cat(xs, dim=0) if len(xs) > 1 else xs[0]
        cu, cos, sin, last_rows, _ = self._continuation_geometry(P, lens)
        self.llm_packed
        self.last_lo4_ranges = None
        self._llm_layers(x, kv_out, cu, cos, sin, max(lens), lens, prefix=prefix, rows_att=self._rows_attention(P, lens) if attention == "rows" else None)
        if kv_out is not None:
            kv_out.length = S
        last, _ = self._lm_head(x, last_rows, False)
        return ExtendResult(logits=last, seq_lens=lens, prefix_len=P, kv_out=kv_out)

    @torch.no_grad()
    def append(self, cache: KVCache, ids: torch.Tensor) -> torch.Tensor:
        """Multi-turn: n more text ids onto ``cache`` IN PLACE.  Their K / V go to rows P .. P + n - 1 (P = cache.length), their attention is the
        existing varlen kernel over the cache rows (cu_q = [0, n], cu_k = [0, P + n], bottom-right causal), cache.length advances by n and
        the logits of the n new rows come back, fp32 [n, vocab].  The batch-1 decode state of the cache reads its position and key count
        from cache.length at every step, so it stays valid."""
        self._continuation_guard("append")
        P = int(cache.length)
        if P < 1:
            raise ValueError("append: the cache is empty (prefill it first)")
        ids = self._text_suffixes("append", [ids])[0]
        n = int(ids.numel())
        if P + n > cache.capacity:
            raise ValueError(f"append: {P} + {n} rows exceed the cache capacity {cache.capacity}")
        x = self.embed_merge(ids, None)
        cu, cos, sin, last_rows, _ = self._continuation_geometry(P, [n])
        ck = ("ext_k", P, n)
        cu_k = self._geom_cache.get(ck)
        if cu_k is None:
            cu_k = self._geom_cache[ck] = torch.tensor([0, P + n], dtype=torch.int32, device=self.device)
        self.llm_packed
        self.last_lo4_ranges = None
        self._llm_layers(x, cache, cu, cos, sin, n, [n], all_rows=True, cache_pos0=P, cu_k=cu_k)
        cache.length = P + n
        _, logits = self._lm_head(x, last_rows, True)
        return logits

    @torch.no_grad()
    def generate_shared(self, prefix_ids: torch.Tensor, tiles: Optional[torch.Tensor], suffixes: Sequence[torch.Tensor],
                        max_new_tokens: int = 128, eos_token_id: Sequence[int] = (128001, 128009),
                        sampling: Optional[SamplingParams] = None, prefix: Optional[KVCache] = None, decode: str = "copy",
                        logprobs: Optional[int] = None, rules: Optional[LogitsRules] = None):
        """N prompts that share their head — ``prefix_ids`` with all the images (``tiles``) — and differ in a text suffix (the question):
        ONE prefill of the prefix (the vision tower runs once) into a cache of exactly P rows, ONE ``extend`` of the N suffixes, then request
        j's rows — the P prefix rows and its own s_j — are copied into decode slot j and the batch continues through the unchanged batched
        decode (N = 1 and shapes without batched-decode support: the batch-1 cache).  More than MAX_DECODE_BATCH suffixes run in chunks that
        share the one prefix prefill.  Request i samples with ``sampling.for_request(i)``.  Each output is [1, len(prefix_ids) + len(suffix_j)
        + T]: what ``generate`` returns for the concatenated prompt (same rule; tokens can differ on a near tie of the top two logits).
        ``decode`` = "copy" (the default): the decode slots do NOT share the prefix — each holds its own copy, so the decode pool is
        B x (P + s + T) rows per layer and every step streams the prefix rows once per slot; what is saved is the prefill — tower and LLM rows
        fall from N x (P + s) to P + N x s.  ``decode`` = "shared": the prefix K / V are stored ONCE in the decode state (one copy out of the
        caller's cache, which stays untouched) and every step reads them once for the whole chunk (lmi_attn_decode_shared); the slots hold
        own rows only — prefix_capacity + B x own_capacity rows per layer.  Needs head_dim 128, 4 query heads per KV head and the batched
        decode (NotImplementedError otherwise: there is no silent fallback); a chunk of one suffix keeps the batch-1 path; under "lo4" /
        "split" the pair (hl) step serves B <= 8 as it does for "copy", larger chunks decode on the fast step.
        ``prefix``: a cache that a ``prefill(prefix_ids, tiles, cache=prefix)`` has already filled — the prefill is skipped (``tiles`` is not
        read) and, as with ``extend``, the cache is left untouched.
        ``logprobs`` = k in 0 .. 8: returns a ``GenerateOutput`` (``sequences`` = that list), in both ``decode`` modes; a request's T counts
        the tokens after its suffix.
        ``rules``: as ``generate``, in both ``decode`` modes and on the batch-1 paths; a request's ids are ``prefix_ids`` + its suffix."""
        k = self._logprobs_arg("generate_shared", logprobs)
        sampling = self._sampling_arg("generate_shared", sampling)
        rules = self._rules_arg("generate_shared", rules, k, eos_token_id)
        if decode not in ("copy", "shared"):
            raise ValueError(f"generate_shared: decode must be 'copy' or 'shared', got {decode!r}")
        self._continuation_guard("generate_shared")
        sfx = self._text_suffixes("generate_shared", suffixes)
        if decode == "shared":
            self._shared_decode_guard(min(len(sfx), self.MAX_DECODE_BATCH))
        pids = prefix_ids.reshape(1, -1)
        if pids.numel() == 0:
            raise ValueError("generate_shared: the prefix is empty")
        P = self.merged_len(pids)
        if prefix is None:
            prefix = KVCache(self.cfg, P, self.dtype, self.device)
            self.prefill(pids, tiles, cache=prefix)
        elif prefix.length != P:
            raise ValueError(f"generate_shared: the prefix cache holds {prefix.length} rows, prefix_ids merge to {P}")
        eos = set(int(e) for e in eos_token_id)
        head = [int(t) for t in pids.reshape(-1).tolist()]
        toks: List[List[int]] = []
        rows_all: Optional[List[_LogprobRows]] = None if k is None else []
        for c0 in range(0, len(sfx), self.MAX_DECODE_BATCH):
            chunk = sfx[c0:c0 + self.MAX_DECODE_BATCH]
            req = [None if sampling is None else sampling.for_request(c0 + j) for j in range(len(chunk))]
            lens = [int(t.numel()) for t in chunk]
            stepping = max_new_tokens > 1
            kv = KVCache(self.cfg, sum(lens), self.dtype, self.device) if stepping else None
            res = self.extend(prefix, chunk, kv_out=kv)
            prompts = [head + [int(t) for t in ids.reshape(-1).tolist()] for ids in chunk]
            first, lpr = self._first_tokens(res.logits, None if sampling is None else req, k, rules, prompts, eos)
            if lpr is not None:
                rows_all += lpr
            offs = [0] + [int(c) for c in np.cumsum(lens)]
            own = [[(kv, offs[j], s)] for j, s in enumerate(lens)]       # a request's own rows ...
            whole = [[(prefix, 0, P)] + o for o in own]                  # ... and all of them: the prefix rows first
            if not stepping:
                toks += [p + [f] for p, f in zip(prompts, first)] if max_new_tokens == 1 else prompts
            elif len(chunk) == 1 or not self._batch_decode_supported():
                toks += [self._continue_single(prompts[j], first[j], whole[j], max_new_tokens, eos, req[j], lpr and lpr[j], rules)
                         for j in range(len(chunk))]
            else:
                if decode == "shared":
                    st = self._shared_state(len(chunk), max(lens) + max_new_tokens, P)
                    self._load_rows([(prefix, 0, P)], st.kp, st.vp, 0)   # the one prefix copy (the captured step reads state-owned memory only)
                    st.prefix_len.fill_(P)
                else:
                    st = self._batch_state(len(chunk), P + max(lens) + max_new_tokens, pair_limit=self.PAIR_DECODE_BATCH)
                for j in range(len(chunk)):
                    self._load_rows(own[j] if decode == "shared" else whole[j], st.k, st.v, j * st.capacity)
                toks += self._greedy_loop_batch(st, prompts, first, [P + s for s in lens], max_new_tokens, eos, None if sampling is None else req,
                                                own_lens=lens if decode == "shared" else None, lpr=lpr, rules=rules)
        return self._outputs(toks, sfx, rows_all, [len(head) + int(t.numel()) for t in sfx])

    # ------------------------------------------------------------------------------------------------
    # Beam search: K hypotheses about one prompt are the K slots of a pooled decode state.  The step's tail chooses jointly over the K x V
    # candidates (lmi_beam_step) and makes slot b continue from the K / V rows of the beam it descends from (lmi_beam_reorder: an in-place
    # permutation of the rows that can differ); the host reads one small buffer per step — the walk list — and runs what transformers does
    # after candidate selection (leopard_amd/beams.py).
    # ------------------------------------------------------------------------------------------------
    BEAMS_LO4 = "served"               # precision "lo4": the pair step serves B <= 8, and num_beams <= 8 always

    def _set_beams(self, st, K: int, eos, row0: int, max_new_tokens: int, rules: Optional[LogitsRules] = None,
                   prompt: Sequence[int] = ()) -> None:
        """Make ``st`` the state of a beam search of K = st.B beams whose slots agree on rows [0, row0).  With ``rules`` every slot's id
        list starts as ``prompt`` and the step's tail is lmi_beam_step_rules + the id reorder (one more captured graph of the state)."""
        ops, dev = self.ops, self.device
        if st.beam_walk is None:
            st.beam_score = torch.zeros(ops.MAX_BEAMS, dtype=torch.float32, device=dev)
            st.beam_parent = torch.zeros(ops.MAX_BEAMS, dtype=torch.int32, device=dev)
            st.beam_walk = torch.zeros(ops.BEAM_WALK_WORDS, dtype=torch.int32, device=dev)
            st.beam_rows = (torch.zeros(K, dtype=torch.float32, device=dev), torch.zeros(K, ops.MAX_BEAMS, dtype=torch.int32, device=dev),
                            torch.zeros(K, ops.MAX_BEAMS, dtype=torch.float32, device=dev),
                            torch.zeros(K, ops.BEAM_MAX_EOS, dtype=torch.float32, device=dev))
            st.beam_eos = torch.full((ops.BEAM_MAX_EOS,), -1, dtype=torch.int64, device=dev)
            st.beam_row0 = torch.zeros(1, dtype=torch.int32, device=dev)
            st.beam_held = torch.zeros(1, dtype=torch.int32, device=dev)
            st.beam_ptrs = torch.tensor([t.data_ptr() for t in st.k + st.v], dtype=torch.int64).to(dev)
        st.beams, st.sampling, st.sample_ex = K, False, False
        st.beam_max_rows = (max_new_tokens + 255) // 256 * 256
        self._set_logprobs(st, None)
        self._set_rules(st, rules, eos)
        if rules is not None:
            if st.seq.shape[1] % 4 or st.seq.data_ptr() % 16:
                raise NotImplementedError(f"generate_beams: rules need id lists of a multiple of four ids (this state: {st.seq.shape[1]})")
            if st.beam_id_ptr is None:
                st.beam_id_ptr = torch.tensor([st.seq.data_ptr()], dtype=torch.int64).to(dev)
                st.beam_id_chunks = torch.zeros(2, dtype=torch.int32, device=dev)
            for j in range(K):
                self._fill_rules(st, j, prompt, rules)
            n = len(prompt)
            st.beam_id_chunks.copy_(torch.tensor([n // 4, (n + max_new_tokens + 3) // 4], dtype=torch.int32))
        ids = sorted(eos)
        st.beam_eos.copy_(torch.tensor(ids + [-1] * (ops.BEAM_MAX_EOS - len(ids)), dtype=torch.int64))
        st.beam_score.zero_(); st.beam_parent.zero_()
        st.beam_row0.fill_(row0); st.beam_held.fill_(row0)
        st.live.fill_(1); st.budget.fill_(1 << 30); st.eos.fill_(-1); st.hist_pos.zero_()

    @torch.no_grad()
    def generate_beams(self, input_ids: torch.Tensor, tiles: Optional[torch.Tensor], num_beams: int, max_new_tokens: int = 128,
                       eos_token_id: Sequence[int] = (128001, 128009), length_penalty: float = 1.0, early_stopping=False,
                       num_return_sequences: int = 1, decode: str = "shared", rules: Optional[LogitsRules] = None) -> BeamOutput:
        """Beam search with ``num_beams`` = K beams (1 .. 8): transformers' ``generate(num_beams=K, do_sample=False)`` — its candidate
        selection, its finished-hypothesis bookkeeping, ``length_penalty``, the three ``early_stopping`` values (False, True, "never") and
        ``num_return_sequences`` <= K.  Among EXACT ties of the accumulated log-probability, which torch.topk leaves open, the order here
        is beam ascending, then id ascending.  ``suppress_tokens`` applies as in HF's processors: the log-probabilities are those of the
        raw row and a suppressed id is never a candidate.  ``rules``: repetition penalty / no-repeat n-gram ban / min_new_tokens as
        transformers applies them in beam search — to the log-softmax scores of every beam, before its accumulated score is added, each
        beam judged against ``input_ids`` (as passed) + its own tokens (lmi_beam_step_rules; the id lists follow the beams); refused as
        ``generate(rules=)`` refuses.  K = 1 with a repetition penalty is NOT greedy ``generate(rules=)``: beams penalise logit - lse, greedy
        penalises the logit (HF's behaviour too).
        One prefill of the prompt into a cache of P rows; the first K beams come from its last logits row; the steps run on a pooled decode
        state of K slots, one captured step per token.  ``decode`` = "shared" (the default): the prompt's K / V rows are stored ONCE in the
        state and read once per step for all beams (lmi_attn_decode_shared), the slots hold the generated rows only — needs what
        ``generate_shared(decode="shared")`` needs (NotImplementedError otherwise; never a silent switch).  ``decode`` = "copy": every slot
        holds the prompt rows too — K x (P + max_new_tokens) rows per layer — and the pooled attention runs, sliding window included.
        Precision "lo4": served (the pair step, as for every batch of at most 8).  Refused before anything is launched: K outside 1 .. 8,
        ``num_return_sequences`` > K, more than MAX_EOS eos ids, a vocabulary below (1 + n_eos) K, tensor-parallel, fp8 and "split" engines,
        shapes without batched decode.  Returns a ``BeamOutput``."""
        from .beams import BeamSearch, decode_walk
        what, ops = "generate_beams", self.ops
        if isinstance(num_beams, bool) or not isinstance(num_beams, (int, np.integer)) or not 1 <= int(num_beams) <= ops.MAX_BEAMS:
            raise ValueError(f"{what}: num_beams must be an int in 1 .. {ops.MAX_BEAMS}, got {num_beams!r}")
        K = int(num_beams)
        if isinstance(num_return_sequences, bool) or not isinstance(num_return_sequences, (int, np.integer)) or not 1 <= int(num_return_sequences) <= K:
            raise ValueError(f"{what}: num_return_sequences must be in 1 .. num_beams = {K}, got {num_return_sequences!r}")
        if decode not in ("copy", "shared"):
            raise ValueError(f"{what}: decode must be 'copy' or 'shared', got {decode!r}")
        if isinstance(max_new_tokens, bool) or int(max_new_tokens) < 1:
            raise ValueError(f"{what}: max_new_tokens must be at least 1, got {max_new_tokens!r}")
        if early_stopping not in (False, True, "never"):
            raise ValueError(f"{what}: early_stopping must be False, True or 'never', got {early_stopping!r}")
        rules = self._rules_arg(what, rules, None, eos_token_id)
        V = self.cfg.text_config.vocab_size
        eos = set(int(e) for e in eos_token_id if 0 <= int(e) < V)
        if len(eos) > ops.BEAM_MAX_EOS or len(eos) > self.MAX_EOS:
            raise ValueError(f"{what}: {len(eos)} eos ids (at most {min(ops.BEAM_MAX_EOS, self.MAX_EOS)} are held on the device)")
        n_sup = 0 if self.suppress_tokens is None else int(self.suppress_tokens.numel())
        if V - n_sup < (1 + len(eos)) * K:
            raise ValueError(f"{what}: a vocabulary of {V} ids ({n_sup} suppressed) is below (1 + {len(eos)} eos ids) x {K} beams")
        if self.tp_size > 1:
            raise NotImplementedError(f"{what}: tensor-parallel engines are not supported (the beam launches and the pooled K / V slots belong to "
                                      "the single-rank batched decode step)")
        if self.fp8 is not None:
            raise NotImplementedError(f"{what}: the fp8 schedule is not supported (the batched decode step has no fp8 form); use 'fast' or 'lo4'")
        if self.split_operands:
            raise NotImplementedError(f"{what}: precision 'split' is not supported (its attention hands over fp32 rows); use 'fast' or 'lo4'")
        if decode == "shared":
            self._continuation_guard(f"{what}(decode='shared')")
            self._shared_decode_guard(K)
        elif not self._batch_decode_supported():
            raise NotImplementedError(f"{what}: this shape has no batched decode (lmi_gemm_skinny needs hidden and feed-forward widths that are "
                                      "multiples of 128, the pooled decode attention head_dim 128)")
        ids = input_ids.reshape(1, -1)
        if ids.numel() == 0:
            raise ValueError(f"{what}: the prompt is empty")
        T = int(max_new_tokens)
        P = self.merged_len(ids)
        prefix = KVCache(self.cfg, P, self.dtype, self.device)
        res = self.prefill(ids, tiles, cache=prefix)
        if decode == "shared":
            st = self._shared_state(K, T, P)
            self._load_rows([(prefix, 0, P)], st.kp, st.vp, 0)        # the one prompt copy: the slots start with ZERO own rows
            st.prefix_len.fill_(P)
            row0 = 0
        else:
            st = self._batch_state(K, P + T)
            for j in range(K):
                self._load_rows([(prefix, 0, P)], st.k, st.v, j * st.capacity)
            row0 = P
        del prefix
        prompt = [int(t) for t in ids.reshape(-1).tolist()]
        self._set_beams(st, K, eos, row0, T, rules, prompt)
        st.pos.fill_(P); st.k_len.fill_(row0 + 1)
        # the first token: the same entry, run eagerly on the ONE prefill row (score 0, K outputs) — HF's initial scores [0, -1e9, ..]
        row = res.logits_last.reshape(1, -1).float()
        if row.stride(1) != 1 or row.stride(0) % 4 or row.data_ptr() % 16:       # the kernel reads 16-byte aligned rows
            pad = torch.zeros(1, (row.shape[1] + 3) // 4 * 4, dtype=torch.float32, device=row.device)
            pad[:, :row.shape[1]] = row
            row = pad
        if rules is None:
            ops.beam_step(row, min(V, row.shape[1]), K, st.beam_eos, st.beam_score, st.tok, st.beam_parent, st.beam_walk,
                          *(t[:1] for t in st.beam_rows), suppress=self.suppress_tokens)
        else:                                                         # nothing appended, eos banned when min_new_tokens > 0, the row untouched
            dev = self.device
            ints = torch.tensor([len(prompt), int(rules.no_repeat_ngram_size), int(rules.min_new_tokens)], dtype=torch.int32).to(dev)
            ops.beam_step_rules(row, min(V, row.shape[1]), K, st.beam_eos, st.beam_score, st.tok, st.beam_parent, st.beam_walk,
                                *(t[:1] for t in st.beam_rows), st.seq[:1], ints[0:1], st.rule_pen[:1], ints[1:2], ints[2:3],
                                suppress=self.suppress_tokens)
        search = BeamSearch(K, T, length_penalty, early_stopping, int(num_return_sequences))
        try:
            while search.step(decode_walk(st.beam_walk.cpu().numpy())):
                self._batch_decode_run(st)
        finally:
            st.beams, st.rules = 0, False                             # the pooled state serves the other calls again, whatever happened
        best = search.results()
        return BeamOutput(sequences=[torch.tensor([prompt + seq], dtype=torch.int64, device=input_ids.device) for _, seq in best],
                          scores=[float(sc) for sc, _ in best])



class DecodeBatchLimitOption:
    """``decode_batch_limit`` of a model object (leopard_amd.compat / idefics2_compat): kept until ``.to(device)`` builds the engine, then the
    engine's (LeopardEngine.decode_batch_limit, which also checks the value).  The object names its engine ``_engine``."""
    _decode_batch_limit: Optional[int] = None                       # None: the engine's default

    @property
    def decode_batch_limit(self) -> int:
        eng = getattr(self, "_engine", None)
        if eng is not None:
            return eng.decode_batch_limit
        return LeopardEngine.MAX_DECODE_BATCH if self._decode_batch_limit is None else self._decode_batch_limit

    @decode_batch_limit.setter
    def decode_batch_limit(self, value) -> None:
        if isinstance(value, bool) or not isinstance(value, int) or not 1 <= value <= LeopardEngine.WIDE_DECODE_BATCH:
            raise ValueError(f"decode_batch_limit must be an integer in 1 .. {LeopardEngine.WIDE_DECODE_BATCH}, got {value!r}")
        self._decode_batch_limit = value
        if getattr(self, "_engine", None) is not None:
            self._engine.decode_batch_limit = value

    _decode_pair_limit: Optional[int] = None                        # ``decode_pair_limit`` (LeopardEngine.decode_pair_limit), kept the same way

    @property
    def decode_pair_limit(self) -> int:
        eng = getattr(self, "_engine", None)
        if eng is not None:
            return eng.decode_pair_limit
        return LeopardEngine.PAIR_DECODE_BATCH if self._decode_pair_limit is None else self._decode_pair_limit

    @decode_pair_limit.setter
    def decode_pair_limit(self, value) -> None:
        _check_pair_limit(value)
        self._decode_pair_limit = value
        if getattr(self, "_engine", None) is not None:
            self._engine.decode_pair_limit = value

    def _apply_decode_batch_limit(self) -> None:
        """Called by ``.to`` once the engine exists."""
        if self._decode_batch_limit is not None:
            self._engine.decode_batch_limit = self._decode_batch_limit
        if self._decode_pair_limit is not None:
            self._engine.decode_pair_limit = self._decode_pair_limit


def _check_pair_limit(value) -> None:
    lo, hi = LeopardEngine.PAIR_DECODE_BATCH, LeopardEngine.WIDE_PAIR_DECODE_BATCH
    if isinstance(value, bool) or not isinstance(value, int) or not lo <= value <= hi:
        raise ValueError(f"decode_pair_limit must be an integer in {lo} .. {hi}, got {value!r}")
