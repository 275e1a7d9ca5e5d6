"""leopard_amd.beams pinned to transformers (CPU, no kernel): a tiny random LlamaForCausalLM in float64, ``generate(num_beams=K)`` against
``beams.walk_of`` + ``beams.BeamSearch`` driven by the same model's logits.  transformers casts the last logits row to fp32, takes
log_softmax in fp32 and adds the running score in fp32; the restatement does exactly that, so the hypothesis scores agree to rounding of the
float64 forward (1e-9), not to fp32's."""
import itertools

import numpy as np
import pytest
import torch

from leopard_amd import beams

transformers = pytest.importorskip("transformers")
if not hasattr(transformers.GenerationMixin, "_beam_search"):
    pytest.skip("this transformers has no GenerationMixin._beam_search", allow_module_level=True)

T_NEW, PROMPT, PAD = 8, [5, 17, 3, 60, 41, 9], 1      # (a pad id of 0 is falsy: transformers would fill with the first eos id)
CASES = list(itertools.product((1, 2, 4), (False, True, "never"), (0.0, 1.0, 2.0)))


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(7)
    cfg = transformers.LlamaConfig(vocab_size=96, hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=4,
                                   num_key_value_heads=2, max_position_embeddings=64, initializer_range=0.35, tie_word_embeddings=False)
    return transformers.LlamaForCausalLM(cfg).double().eval()


def hf_generate(model, K, es, lp, eos):
    """``generate`` routes num_beams = 1 to its greedy search, which reads neither early_stopping nor length_penalty; for K = 1 the mode is
    therefore pinned to BEAM_SEARCH for the call, so that ``_beam_search`` itself runs with one beam."""
    from transformers.generation.configuration_utils import GenerationConfig, GenerationMode
    mode = GenerationConfig.get_generation_mode
    if K == 1:
        GenerationConfig.get_generation_mode = lambda self, *a, **k: GenerationMode.BEAM_SEARCH
    try:
        with torch.no_grad():
            return model.generate(torch.tensor([PROMPT]), num_beams=K, max_new_tokens=T_NEW, length_penalty=lp, early_stopping=es,
                                  num_return_sequences=K, eos_token_id=list(eos) if eos else None, pad_token_id=PAD, do_sample=False,
                                  return_dict_in_generate=True, output_scores=True)
    finally:
        GenerationConfig.get_generation_mode = mode


def restated(model, K, es, lp, eos):
    search = beams.BeamSearch(K, T_NEW, lp, es, K)
    seqs, scores = [[]], [0.0]
    while True:
        with torch.no_grad():
            logits = model(torch.tensor([PROMPT + s for s in seqs])).logits[:, -1, :].to(torch.float32)
        lp_rows = torch.log_softmax(logits, dim=-1).numpy()
        if not search.step(beams.walk_of(lp_rows, np.asarray(scores, dtype=np.float32), K, eos)):
            return search.results()
        seqs, scores = search.beams, search.scores


@pytest.fixture(scope="module")
def eos_ids(model):
    """Two ids the unconstrained 4-beam run emits: the third token of its best hypothesis and a later, different one of another."""
    out = hf_generate(model, 4, False, 1.0, ())
    gen = out.sequences[:, len(PROMPT):].tolist()
    a = gen[0][2]
    b = next(t for row in gen[1:] for t in row[3:] if t != a)
    return (a, b)


@pytest.fixture(scope="module")
def hf_runs(model, eos_ids):
    return {c: hf_generate(model, *c, eos_ids) for c in CASES}


@pytest.mark.parametrize("K,es,lp", CASES)
def test_restatement_equals_transformers(model, eos_ids, hf_runs, K, es, lp):
    out = hf_runs[(K, es, lp)]
    want = restated(model, K, es, lp, eos_ids)
    assert type(out).__name__ == "GenerateBeamDecoderOnlyOutput"       # _beam_search ran, for K = 1 too
    assert len(want) == K == out.sequences.shape[0]
    for i, (score, seq) in enumerate(want):
        got = out.sequences[i, len(PROMPT):].tolist()
        assert got[:len(seq)] == seq and all(t == PAD for t in got[len(seq):]), (i, got, seq)
        hf = float(out.sequences_scores[i])
        assert abs(score - hf) <= 1e-9 * max(abs(hf), 1e-30), (i, score, hf)


def test_the_cases_finish_early(hf_runs, eos_ids):
    """About transformers' outputs alone: at least half of the cases return a sequence shorter than max_new_tokens, and every
    early_stopping value has one such case."""
    def short(out):
        gen = out.sequences[:, len(PROMPT):]
        return any((row[-1] == PAD and PAD not in eos_ids) or any(int(t) in eos_ids for t in row[:-1]) for row in gen.tolist())
    hits = {c: short(o) for c, o in hf_runs.items()}
    assert sum(hits.values()) * 2 >= len(CASES), hits
    for es in (False, True, "never"):
        assert any(h for (K, e, lp), h in hits.items() if e is es or e == es and type(e) is type(es)), es


def test_walks_and_arguments():
    """walk_of on a hand-made step, decode_walk's layout, BeamSearch's argument checks."""
    lp = np.log(np.array([[0.5, 0.3, 0.15, 0.05], [0.4, 0.4, 0.1, 0.1]]))
    w = beams.walk_of(lp, [0.0, -0.1], 2, eos=[1])
    assert [(c.rank, c.parent, c.id, c.is_eos) for c in w] == [(0, 0, 0, False), (1, 1, 0, False)]
    w = beams.walk_of(lp, [0.0, 0.0], 2, eos=[0])
    assert [(c.parent, c.id, c.is_eos) for c in w] == [(0, 0, True), (1, 0, True), (1, 1, False), (0, 1, False)]
    assert [(c.parent, c.id) for c in beams.walk_of(lp, [0.0, 0.0], 2, suppress=[0])] == [(1, 1), (0, 1)]
    words = np.zeros(1 + 40 * 5, dtype=np.int32)
    words[:11] = [2, 0, np.float32(-0.5).view(np.int32), 1, 7, 0, 1, np.float32(-1.25).view(np.int32), 0, 3, 1]
    assert beams.decode_walk(words) == [beams.Cand(0, -0.5, 1, 7, False), beams.Cand(1, -1.25, 0, 3, True)]
    for kw in (dict(early_stopping="sometimes"), dict(num_return_sequences=3), dict(max_new_tokens=0)):
        with pytest.raises(ValueError):
            beams.BeamSearch(**dict(dict(num_beams=2, max_new_tokens=4), **kw))
