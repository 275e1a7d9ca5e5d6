"""The contract of lmi_beam_step_rules pinned to transformers (CPU, no kernel): a tiny random LlamaForCausalLM in float64,
``generate(num_beams=K, repetition_penalty=, no_repeat_ngram_size=, min_new_tokens=)`` against the restatement the kernel tests are held to —
``tests.logits_rules_ref.apply`` on the fp32 log-softmax row over ``prompt + that beam's tokens`` (eos banned while fewer than
``min_new_tokens`` tokens exist), then ``beams.walk_of`` and ``beams.BeamSearch``.  In beam search transformers runs the processors on the
log-softmax scores, not on the logits, and adds the running score afterwards; the restatement does exactly that, so sequences agree exactly
and scores to rounding of the float64 forward (1e-9)."""
import itertools

import numpy as np
import pytest
import torch

from leopard_amd import beams
from tests import logits_rules_ref as L

transformers = pytest.importorskip("transformers")
if not hasattr(transformers.GenerationMixin, "_beam_search"):
    pytest.skip("this transformers has no GenerationMixin._beam_search", allow_module_level=True)

T_NEW, PROMPT, PAD = 8, [5, 17, 3, 60, 41, 9, 17, 3], 1
RULES = ((1.3, 0, 0), (1.0, 2, 0), (1.0, 0, 5), (1.3, 2, 5), (0.8, 1, 3))          # (repetition_penalty, no_repeat_ngram_size, min_new_tokens)
CASES = list(itertools.product((2, 4), (False, True), (0.0, 1.0), RULES)) + [(1, False, 1.0, r) for r in RULES]
OFF = (1.0, 0, 0)


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(7)
    cfg = transformers.LlamaConfig(vocab_size=96, hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=4,
                                   num_key_value_heads=2, max_position_embeddings=64, initializer_range=0.35, tie_word_embeddings=False)
    return transformers.LlamaForCausalLM(cfg).double().eval()


def hf_generate(model, K, es, lp, rules, eos):
    """K = 1 runs ``_beam_search`` too: the mode is pinned to BEAM_SEARCH for the call (tests/test_beam_hf_pin.py)."""
    from transformers.generation.configuration_utils import GenerationConfig, GenerationMode
    mode = GenerationConfig.get_generation_mode
    if K == 1:
        GenerationConfig.get_generation_mode = lambda self, *a, **k: GenerationMode.BEAM_SEARCH
    p, n, m = rules
    kw = dict(repetition_penalty=p) if p != 1.0 else {}
    kw.update(dict(no_repeat_ngram_size=n) if n else {})
    kw.update(dict(min_new_tokens=m) if m else {})
    try:
        with torch.no_grad():
            return model.generate(torch.tensor([PROMPT]), num_beams=K, max_new_tokens=T_NEW, length_penalty=lp, early_stopping=es,
                                  num_return_sequences=K, eos_token_id=list(eos) if eos else None, pad_token_id=PAD, do_sample=False,
                                  return_dict_in_generate=True, output_scores=True, **kw)
    finally:
        GenerationConfig.get_generation_mode = mode


def restated(model, K, es, lp, rules, eos):
    p, n, m = rules
    search = beams.BeamSearch(K, T_NEW, lp, es, K)
    seqs, scores = [[]], [0.0]
    while True:
        with torch.no_grad():
            logits = model(torch.tensor([PROMPT + s for s in seqs])).logits[:, -1, :].to(torch.float32)
        rows = torch.log_softmax(logits, dim=-1)
        left = max(m - search.generated, 0)
        rows = torch.stack([L.apply(rows[b], PROMPT + seqs[b], p, n, left, eos) for b in range(len(seqs))]).numpy()
        if not search.step(beams.walk_of(rows, np.asarray(scores, dtype=np.float32), K, eos)):
            return search.results()
        seqs, scores = search.beams, search.scores


@pytest.fixture(scope="module")
def eos_ids(model):
    """Two ids the free 4-beam run emits: the third token of its best hypothesis and a later, different one of another."""
    out = hf_generate(model, 4, False, 1.0, OFF, ())
    gen = out.sequences[:, len(PROMPT):].tolist()
    a = gen[0][2]
    b = next(t for row in gen[1:] for t in row[3:] if t != a)
    return (a, b)


@pytest.fixture(scope="module")
def hf_runs(model, eos_ids):
    return {c: hf_generate(model, *c, eos_ids) for c in CASES}


@pytest.mark.parametrize("K,es,lp,rules", CASES)
def test_restatement_equals_transformers(model, eos_ids, hf_runs, K, es, lp, rules):
    out = hf_runs[(K, es, lp, rules)]
    want = restated(model, K, es, lp, rules, eos_ids)
    assert type(out).__name__ == "GenerateBeamDecoderOnlyOutput"       # _beam_search ran, for K = 1 too
    assert len(want) == K == out.sequences.shape[0]
    for i, (score, seq) in enumerate(want):
        got = out.sequences[i, len(PROMPT):].tolist()
        assert got[:len(seq)] == seq and all(t == PAD for t in got[len(seq):]), (i, got, seq)
        hf = float(out.sequences_scores[i])
        assert abs(score - hf) <= 1e-9 * max(abs(hf), 1e-30), (i, score, hf)


def test_the_rules_change_the_result(model, eos_ids, hf_runs):
    """About transformers' outputs alone: in at least half of the cases the rules change what the same call returns without them."""
    free = {}
    changed = 0
    for (K, es, lp, rules), out in hf_runs.items():
        if (K, es, lp) not in free:
            free[(K, es, lp)] = hf_generate(model, K, es, lp, OFF, eos_ids).sequences.tolist()
        changed += out.sequences.tolist() != free[(K, es, lp)]
    assert changed * 2 >= len(CASES), (changed, len(CASES))
