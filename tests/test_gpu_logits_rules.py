"""-m gpu: generate(rules=...) on the MI355X — lmi_decode_rules on the cases of tests/logits_rules_ref.py (shared with
tests/test_emu_logits_rules.py; bit for bit against the torch-fp32 restatement: what the device adds is the LDS atomicOr ownership across
sixteen waves, the device's fp32 divide and the production vocabulary), and the engine's generation calls with ``rules`` on the mid model
through the captured decode step, recomputed token for token by a host loop over ``decode_step``'s raw logits."""
import warnings

import numpy as np
import pytest
import torch

from tests import logits_rules_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = 12


@pytest.fixture(scope="module")
def ops():
    from leopard_amd.ops import Ops
    assert torch.cuda.is_available()
    return Ops()


# ---- the kernel ----------------------------------------------------------------------------------------------------------------------
def test_kernel_lengths(ops):
    R.check_lengths(ops, DEV)


def test_kernel_batches_and_the_row_with_everything_off(ops):
    R.check_batches(ops, DEV)


def test_kernel_without_append(ops):
    R.check_no_append(ops, DEV)


def test_kernel_one_id_repeated(ops):
    R.check_one_id_repeated(ops, DEV)


def test_kernel_ngram_pins(ops):
    R.check_ngram_pins(ops, DEV)


def test_kernel_min_left(ops):
    R.check_min_left(ops, DEV)


def test_kernel_frozen_and_full_rows(ops):
    R.check_frozen_and_full(ops, DEV)


def test_kernel_production_vocab(ops):
    R.check_production_vocab(ops, DEV)


def test_kernel_rejects_bad_arguments(ops):
    R.check_rejects(ops, DEV)


# ---- the engine, mid model -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mid():
    from leopard_amd import compat
    from leopard_amd.config import mid_config
    from leopard_amd.ops import Ops
    from leopard_amd.weights import SynthSource
    cfg, ops = mid_config(), Ops()
    m = compat.LeopardForConditionalGeneration(cfg, lambda dev, dt: SynthSource(cfg, ops, dev, dt), torch.float16, ops, torch_dtype=torch.float16)
    return m.to(DEV)


def mid_sample(cfg, seed=0):
    from tools.gen_fulldepth_fixtures import sample_inputs
    u8, ids = sample_inputs(cfg, 1, 336, 336, seed=seed)[:2]
    return torch.from_numpy(u8).to(DEV), ids.to(DEV)


def text_requests(n, seed):
    g = np.random.default_rng(seed)
    return [(torch.from_numpy(g.integers(3, 7900, 33 + 5 * j)).reshape(1, -1).to(DEV), None) for j in range(n)]


def rules_of(**kw):
    from leopard_amd.engine import LogitsRules
    return LogitsRules(**kw)


def host_loop(eng, cfg, ids, tiles, n_new, rules, eos=(), follow=None):
    """generate(rules=...) recomputed on the host: prefill, then decode_step's RAW logits, logits_rules_ref.apply, argmax.  Returns (ids,
    [processed row of every step], [raw row of every step]); ``follow``: consume these new tokens instead of the host's own choices."""
    from leopard_amd.engine import KVCache
    V = cfg.text_config.vocab_size
    cache = KVCache(cfg, eng.merged_len(ids) + n_new, eng.dtype, DEV)
    row = eng.prefill(ids.reshape(1, -1), tiles, cache=cache).logits_last.clone()
    seq, new, rows, raws = [int(t) for t in ids.reshape(-1).tolist()], [], [], []
    while True:
        raw = row[:V].float().cpu()
        r = R.apply(raw, seq, rules.repetition_penalty, rules.no_repeat_ngram_size, 1 if len(new) < rules.min_new_tokens else 0, eos)
        rows.append(r); raws.append(raw)
        tok = int(r.argmax()) if follow is None else int(follow[len(new)])
        new.append(tok); seq.append(tok)
        if tok in eos or len(new) == n_new:
            return seq, rows, raws
        row = eng.decode_step(tok, cache).clone()


def assert_equal_or_near_tie(eng, cfg, ids, tiles, one, got, rules, eos=()):
    """As tests/test_gpu_shared_decode.py, on the PROCESSED logits: equal, or differing first where the top two processed logits of the
    reference run (``one``, replayed through the batch-1 step) are within the 16-bit noise of the row."""
    if one.shape == got.shape and torch.equal(one, got):
        return True
    n = ids.shape[1]
    a, b = one[0].tolist(), got[0].tolist()
    j = next(i for i in range(min(len(a), len(b))) if a[i] != b[i])
    assert j >= n, (j, n)
    _, rows, raws = host_loop(eng, cfg, ids, tiles, j - n + 1, rules, eos, follow=a[n:])
    top2 = rows[j - n].topk(2).values
    scale = float(raws[j - n][torch.isfinite(raws[j - n])].abs().max())
    assert float(top2[0] - top2[1]) <= 2e-3 * scale, (j, top2, scale)
    return False


def test_generate_through_the_captured_step_equals_the_host_loop(mid):
    cfg, eng = mid.config, mid.engine
    tiles, img_ids = mid_sample(cfg, seed=4)
    txt = text_requests(1, seed=1)[0][0]
    greedy = eng.generate(txt, None, max_new_tokens=T, eos_token_id=())
    eos = (int(greedy[0, txt.shape[1]]),)                               # an eos the model would choose at once
    assert eng.generate(txt, None, max_new_tokens=T, eos_token_id=eos).shape[1] == txt.shape[1] + 1
    cases = [("penalty", rules_of(repetition_penalty=1.3), ()), ("ngram", rules_of(no_repeat_ngram_size=2), ()),
             ("min_new", rules_of(min_new_tokens=5), eos),
             ("all", rules_of(repetition_penalty=1.3, no_repeat_ngram_size=3, min_new_tokens=5), eos)]
    for name, rules, e in cases:
        for ids, tl in ((txt, None), (img_ids, tiles), (half_vocabulary_prompt(9), None)):     # (the last: a prompt on which the penalty bites)
            want, _, _ = host_loop(eng, cfg, ids, tl, T, rules, e)
            got = eng.generate(ids, tl, max_new_tokens=T, eos_token_id=e, rules=rules)
            assert got[0].tolist() == want, (name, got[0, ids.shape[1]:].tolist(), want[ids.shape[1]:])
            if rules.min_new_tokens:
                assert got.shape[1] - ids.shape[1] >= rules.min_new_tokens
    st = eng._gen_cache._decode_state
    assert st.graphs.get((False, False, True)) is not None and st.seq is not None      # the steps with rules were replays of their own graph
    # other values replay that graph; a call without rules replays the greedy one and returns what it returned before
    g = st.graphs[(False, False, True)]
    eng.generate(txt, None, max_new_tokens=T, eos_token_id=(), rules=rules_of(repetition_penalty=1.7, no_repeat_ngram_size=4))
    assert st.graphs[(False, False, True)] is g and eng._gen_cache._decode_state is st
    assert torch.equal(eng.generate(txt, None, max_new_tokens=T, eos_token_id=()), greedy)
    # the sampled step with one kept token makes the greedy choice
    from leopard_amd.engine import SamplingParams
    rules = cases[3][1]
    want, _, _ = host_loop(eng, cfg, txt, None, T, rules, eos)
    assert eng.generate(txt, None, max_new_tokens=T, eos_token_id=eos, rules=rules, sampling=SamplingParams(top_k=1, seed=5))[0].tolist() == want


def test_batch_stream_and_shared_agree_with_generate(mid):
    cfg, eng = mid.config, mid.engine
    rules = rules_of(repetition_penalty=1.3, no_repeat_ngram_size=3, min_new_tokens=4)
    reqs = text_requests(5, seed=2)
    first = eng.generate(reqs[0][0], None, max_new_tokens=2, eos_token_id=())
    eos = (int(first[0, -1]),)
    try:
        singles = [eng.generate(i, t, max_new_tokens=T, eos_token_id=eos, rules=rules) for i, t in reqs]
        same = [assert_equal_or_near_tie(eng, cfg, r[0], None, s, g, rules, eos)
                for r, s, g in zip(reqs[:3], singles, eng.generate_batch(reqs[:3], max_new_tokens=T, eos_token_id=eos, rules=rules))]
        same += [assert_equal_or_near_tie(eng, cfg, r[0], None, s, g, rules, eos)
                 for r, s, g in zip(reqs, singles, eng.generate_stream(reqs, batch_size=2, max_new_tokens=T, eos_token_id=eos, rules=rules))]
        print(f"[rules: generate_batch / generate_stream] {sum(same)} / {len(same)} outputs identical to generate()")
        tiles, ids = mid_sample(cfg, seed=4)
        head = ids[:, :-40]
        sfx = [ids[:, -40:]] + [r[0] for r in text_requests(2, seed=3)]
        copy = eng.generate_shared(head, tiles, sfx, max_new_tokens=T, eos_token_id=eos, decode="copy", rules=rules)
        shared = eng.generate_shared(head, tiles, sfx, max_new_tokens=T, eos_token_id=eos, decode="shared", rules=rules)
        same = [assert_equal_or_near_tie(eng, cfg, torch.cat([head, s], dim=1), tiles, c, g, rules, eos) for s, c, g in zip(sfx, copy, shared)]
        print(f"[rules: generate_shared] {sum(same)} / {len(same)} outputs of decode='shared' identical to decode='copy'")
        st = eng._batch_states[("shared", 3)]
        assert st.seq is not None and st.seq.shape == (3, st.prefix_capacity + st.capacity)
    finally:
        eng.release_batch_state()


def half_vocabulary_prompt(seed, n=3900):
    """A prompt built so that the penalty bites: n distinct ids, about half of the mid model's vocabulary in random order.  The synthetic
    model does not fall into a loop by itself within a dozen tokens, so the repetition the penalty acts on is put into the prompt: at
    every step the raw top token is a seen id about every second time, while its runner-up is about as often not."""
    g = np.random.default_rng(seed)
    return torch.from_numpy(g.permutation(np.arange(3, 7900))[:n].copy()).reshape(1, -1).to(DEV)


def test_compat_surface(mid):
    cfg, eng = mid.config, mid.engine
    found = None
    for seed in range(6):
        ids = half_vocabulary_prompt(seed)
        with warnings.catch_warnings():
            warnings.simplefilter("error")                              # implemented arguments: no warning
            plain = mid.generate(ids, max_new_tokens=T, eos_token_id=[])
            assert mid.last_decoding == "greedy"
            pen = mid.generate(ids, max_new_tokens=T, eos_token_id=[], repetition_penalty=1.3)
        assert mid.last_decoding == "greedy + repetition_penalty=1.3"
        want, _, _ = host_loop(eng, cfg, ids, None, T, rules_of(repetition_penalty=1.3))
        assert pen[0].tolist() == want
        if not torch.equal(pen, plain):
            found = seed
            break
    assert found is not None, "repetition_penalty=1.3 never changed the greedy tokens"
    print(f"[rules: compat surface] prompt {found}: greedy {plain[0, ids.shape[1]:].tolist()} -> penalised {pen[0, ids.shape[1]:].tolist()}")
    with pytest.warns(UserWarning, match="num_beams"):
        mid.generate(ids, max_new_tokens=2, eos_token_id=[], num_beams=4)
    with pytest.raises(NotImplementedError, match="logprobs"):
        mid.generate(ids, max_new_tokens=2, eos_token_id=[], repetition_penalty=1.3, logprobs=2)
