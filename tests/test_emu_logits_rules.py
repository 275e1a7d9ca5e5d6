"""generate(rules=...) on the CPU: lmi_decode_rules through the kernel-logic emulator — the cases of tests/logits_rules_ref.py, shared with
tests/test_gpu_logits_rules.py, bit for bit against the torch-fp32 restatement — and the engine's generation calls with ``rules`` on a
micro configuration, recomputed token for token by a host loop over ``decode_step``'s raw logits."""
import pytest
import torch

from tests import logits_rules_ref as R
from tests.emu_util import emu_ops

DEV = "cpu"


@pytest.fixture(scope="module")
def ops():
    return emu_ops()


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


# ---- the engine ----------------------------------------------------------------------------------------------------------------------
from leopard_amd.engine import KVCache, LogitsRules, SamplingParams  # noqa: E402

PEN, NGRAM, MINNEW = LogitsRules(repetition_penalty=1.3), LogitsRules(no_repeat_ngram_size=2), LogitsRules(min_new_tokens=4)
ALL = LogitsRules(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=4)


@pytest.fixture(scope="module")
def micro(ops):
    from tests.test_emu_shared_decode import _engine_setup
    cfg, eng, u8, ids = _engine_setup(ops, torch.float16)               # hidden 512, 4 query heads on 1 KV head: every decode path exists
    assert eng._batch_decode_supported()
    return cfg, eng, u8, ids


def text_requests(n=4, seed=17):
    """Short text-only requests (the emulated vision tower is the slow part of a request)."""
    g = torch.Generator().manual_seed(seed)
    return [(torch.randint(3, 240, (1, 9 + 3 * j), generator=g), None) for j in range(n)]


def host_loop(eng, cfg, ids, tiles, T, rules, eos=()):
    """generate(rules=...) recomputed on the host: prefill, then decode_step's RAW logits, logits_rules_ref.apply, argmax."""
    V = cfg.text_config.vocab_size
    cache = KVCache(cfg, eng.merged_len(ids) + T, eng.dtype, "cpu")
    row = eng.prefill(ids.reshape(1, -1), tiles, cache=cache).logits_last.clone()
    seq, new = [int(t) for t in ids.reshape(-1).tolist()], []
    while True:
        r = R.apply(row[:V].float(), seq, rules.repetition_penalty, rules.no_repeat_ngram_size, 1 if len(new) < rules.min_new_tokens else 0, eos)
        tok = int(r.argmax())
        new.append(tok); seq.append(tok)
        if tok in eos or len(new) == T:
            return seq
        row = eng.decode_step(tok, cache).clone()


@pytest.fixture(scope="module")
def greedy_loop_id(micro):
    """The id the micro model repeats under greedy decoding of the first text request (its tokens are one repeated id)."""
    cfg, eng, u8, ids = micro
    req = text_requests()[0][0]
    out = eng.generate(req, None, max_new_tokens=6, eos_token_id=())[0, req.shape[1]:].tolist()
    assert len(set(out[1:])) == 1, out
    return out[-1]


@pytest.mark.parametrize("rules", [PEN, NGRAM, MINNEW, ALL], ids=["penalty", "ngram", "min_new", "all"])
def test_generate_equals_the_host_loop(micro, greedy_loop_id, rules):
    cfg, eng, u8, ids = micro
    req, T = text_requests()[0][0], 7
    eos = (greedy_loop_id,) if rules.min_new_tokens else ()
    want = host_loop(eng, cfg, req, None, T, rules, eos)
    got = eng.generate(req, None, max_new_tokens=T, eos_token_id=eos, rules=rules)
    assert got[0].tolist() == want, (got[0].tolist(), want)
    top1 = eng.generate(req, None, max_new_tokens=T, eos_token_id=eos, rules=rules, sampling=SamplingParams(top_k=1, seed=3))
    assert top1[0].tolist() == want                                     # the sampled step with one kept token: the same choice
    if rules is not MINNEW:
        assert got[0].tolist() != eng.generate(req, None, max_new_tokens=T, eos_token_id=())[0].tolist()


def test_generate_with_an_image_prompt(micro):
    """The prompt ids as passed: the image placeholders (id 250) count as seen ids and are never a write target problem."""
    cfg, eng, u8, ids = micro
    want = host_loop(eng, cfg, ids, u8, 4, ALL, ())
    assert eng.generate(ids, u8, max_new_tokens=4, eos_token_id=(), rules=ALL)[0].tolist() == want


def test_no_repeat_unigram_and_min_new_tokens(micro, greedy_loop_id):
    cfg, eng, u8, ids = micro
    req = text_requests()[1][0]
    n = req.shape[1]
    out = eng.generate(req, None, max_new_tokens=9, eos_token_id=(), rules=LogitsRules(no_repeat_ngram_size=1))[0].tolist()
    assert len(set(out[n:])) == 9 and not set(out[n:]) & set(out[:n])  # no token repeats, no prompt id is produced
    first = eng.generate(req, None, max_new_tokens=9, eos_token_id=())[0, n:].tolist()
    eos = (first[0],)                                                   # an eos the model would choose at once
    assert eng.generate(req, None, max_new_tokens=9, eos_token_id=eos).shape[1] == n + 1
    for m in (1, 3, 9):
        new = eng.generate(req, None, max_new_tokens=9, eos_token_id=eos, rules=LogitsRules(min_new_tokens=m))[0, n:].tolist()
        assert len(new) >= m and eos[0] not in new[:m], (m, new)


def test_generate_batch_and_stream_equal_generate(micro, greedy_loop_id, rules=ALL):
    cfg, eng, u8, ids = micro
    reqs, T = text_requests(), 7
    eos = (greedy_loop_id,) if rules.min_new_tokens else ()
    singles = [eng.generate(i, t, max_new_tokens=T, eos_token_id=eos, rules=rules) for i, t in reqs]
    got = eng.generate_batch(reqs[:3], max_new_tokens=T, eos_token_id=eos, rules=rules)
    for g, s in zip(got, singles):
        assert torch.equal(g, s), (g.tolist(), s.tolist())
    hist = type(eng).HIST
    type(eng).HIST = 2
    try:
        for bs in (1, 3):
            got = eng.generate_stream(reqs, batch_size=bs, max_new_tokens=T, eos_token_id=eos, rules=rules)
            for g, s in zip(got, singles):
                assert torch.equal(g, s), (bs, g.tolist(), s.tolist())
    finally:
        type(eng).HIST = hist
        eng.release_batch_state()


@pytest.mark.parametrize("decode", ["copy", "shared"])
def test_generate_shared_equals_generate(micro, decode):
    """As tests/test_emu_shared_decode.py asserts it without rules: strict equality with generate() on [prefix ; suffix]."""
    cfg, eng, u8, ids = micro
    head = ids[:, :-48]
    sfx = [ids[:, -48:], ids[:, -48:-20], torch.tensor([[9, 8, 7, 6, 5]])]
    singles = [eng.generate(torch.cat([head, s], dim=1), u8, max_new_tokens=4, eos_token_id=(), rules=ALL) for s in sfx]
    got = eng.generate_shared(head, u8, sfx, max_new_tokens=4, eos_token_id=(), decode=decode, rules=ALL)
    for g, s in zip(got, singles):
        assert torch.equal(g, s), (g.tolist(), s.tolist())
    one = eng.generate_shared(head, u8, sfx[:1], max_new_tokens=4, eos_token_id=(), decode=decode, rules=ALL)       # the batch-1 path
    assert torch.equal(one[0], singles[0])
    eng.release_batch_state()


class Recorder:
    """A thin wrapper over Ops that records the name of every method called through it."""
    def __init__(self, ops):
        self._ops, self.calls = ops, []

    def __getattr__(self, name):
        v = getattr(self._ops, name)
        if callable(v) and not name.startswith("_"):
            def f(*a, **kw):
                self.calls.append(name)
                return v(*a, **kw)
            return f
        return v


def test_calls_without_rules_are_unchanged_and_values_never_recapture(micro, ops):
    cfg, eng, u8, ids = micro
    req, T = text_requests()[2][0], 5
    rec = Recorder(ops)
    eng.ops = rec
    eng._gen_cache = None                                               # a fresh generation cache and decode state
    try:
        eng.generate(req, None, max_new_tokens=T, eos_token_id=())      # (builds the state)
        st = eng._gen_cache._decode_state
        assert st.seq is None and st.rule_pen is None                  # a state that never saw rules holds what it held before
        del rec.calls[:]
        before = eng.generate(req, None, max_new_tokens=T, eos_token_id=())
        plain_calls = list(rec.calls)
        assert "decode_rules" not in plain_calls
        del rec.calls[:]
        eng.generate(req, None, max_new_tokens=T, eos_token_id=(), rules=PEN)
        assert rec.calls.count("decode_rules") == T                     # one eager launch for the first token + one per step
        assert sorted(c for c in rec.calls if c != "decode_rules") == sorted(plain_calls)
        seq = st.seq
        assert seq is not None and seq.shape == (1, st.capacity) and int(st.seq_len[0]) == req.shape[1] + T - 1
        del rec.calls[:]
        eng.generate(req, None, max_new_tokens=T, eos_token_id=(), rules=LogitsRules(repetition_penalty=1.7, no_repeat_ngram_size=3))
        assert st.seq is seq and eng._gen_cache._decode_state is st     # other values: the same buffers, the same state
        del rec.calls[:]
        after = eng.generate(req, None, max_new_tokens=T, eos_token_id=())
        assert rec.calls == plain_calls and torch.equal(after, before) and not st.rules
        off = eng.generate(req, None, max_new_tokens=T, eos_token_id=(), rules=LogitsRules())      # everything off: treated as None
        assert torch.equal(off, before) and "decode_rules" not in rec.calls
        raw = eng.decode_step(5, KVCache(cfg, 8, eng.dtype, "cpu"))     # decode_step never applies rules
        assert "decode_rules" not in rec.calls and torch.isfinite(raw).all()
    finally:
        eng.ops = ops


def test_first_rules_leaves_the_callers_logits_alone(micro):
    cfg, eng, u8, ids = micro
    V = cfg.text_config.vocab_size
    x = R.random_rows(2, V, V, seed=2)
    keep = x.clone()
    out = eng.first_rules(x, [[1, 2, 3, 2], [250, 7]], ALL, (5, 9))
    assert torch.equal(x, keep) and out.data_ptr() != x.data_ptr()
    for b, p in enumerate([[1, 2, 3, 2], [250, 7]]):
        assert R.same_bits(out[b], R.apply(x[b], p, 1.3, 2, 4, (5, 9)))


def test_rules_validation_and_refusals_before_any_launch(micro, ops):
    cfg, eng, u8, ids = micro
    for bad in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(no_repeat_ngram_size=-1), dict(min_new_tokens=-2)):
        with pytest.raises(ValueError):
            LogitsRules(**bad)
    assert not LogitsRules().active and LogitsRules().describe() == ""
    assert ALL.describe() == "repetition_penalty=1.3 + no_repeat_ngram_size=2 + min_new_tokens=4"
    head, sfx = ids[:, :-48], [ids[:, -48:], ids[:, -48:-20]]
    calls = [lambda **kw: eng.generate(ids, u8, max_new_tokens=2, **kw),
             lambda **kw: eng.generate_batch([(ids, u8), (ids, u8)], max_new_tokens=2, **kw),
             lambda **kw: eng.generate_stream([(ids, u8), (ids, u8)], batch_size=2, max_new_tokens=2, **kw),
             lambda **kw: eng.generate_shared(head, u8, sfx, max_new_tokens=2, **kw)]
    n = []
    check = ops._check
    ops._check = lambda rc: (n.append(1), check(rc))[1]
    try:
        for call in calls:
            with pytest.raises(NotImplementedError, match="logprobs"):
                call(rules=PEN, logprobs=2)
            with pytest.raises(NotImplementedError, match="eos ids"):
                call(rules=MINNEW, eos_token_id=(1, 2, 3, 4, 5))
            with pytest.raises(TypeError):
                call(rules={"repetition_penalty": 1.2})
            eng.W.tp_size = 2
            try:
                with pytest.raises(NotImplementedError, match="tensor-parallel"):
                    call(rules=PEN)
            finally:
                eng.W.tp_size = 1
    finally:
        ops._check = check
    assert n == []


# ---- the surfaces --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(ops):
    from leopard_amd import compat
    from leopard_amd.weights import SynthSource
    from tests.test_emu_engine import micro_config
    cfg = micro_config()
    m = compat.LeopardForConditionalGeneration(cfg, lambda dev, dt: SynthSource(cfg, ops, dev, dt), torch.float16, ops, torch_dtype=torch.float16)
    return m.to("cpu").eval()


def test_compat_surface_arguments(model, tmp_path, recwarn):
    import json
    import warnings
    from leopard_amd import sampling
    ids = text_requests()[0][0]
    eng = model.engine
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                  # the three arguments are implemented: no warning
        out = model.generate(ids, max_new_tokens=5, eos_token_id=[], repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=2)
    assert model.last_decoding == "greedy + repetition_penalty=1.3 + no_repeat_ngram_size=2 + min_new_tokens=2"
    want = eng.generate(ids, None, max_new_tokens=5, eos_token_id=(), rules=LogitsRules(1.3, 2, 2))
    assert torch.equal(out, want)
    plain = model.generate(ids, max_new_tokens=5, eos_token_id=[])
    assert model.last_decoding == "greedy" and not torch.equal(plain, out)
    assert torch.equal(model.generate(ids, max_new_tokens=5, eos_token_id=[], repetition_penalty=1.0, no_repeat_ngram_size=0), plain)
    reqs = [(ids, None), (text_requests()[1][0], None)]
    singles = [model.generate(i, max_new_tokens=4, eos_token_id=[], repetition_penalty=1.3) for i, _ in reqs]
    for got in (model.generate_batch(reqs, max_new_tokens=4, eos_token_id=[], repetition_penalty=1.3),
                model.generate_stream(reqs, batch_size=2, max_new_tokens=4, eos_token_id=[], repetition_penalty=1.3)):
        assert all(torch.equal(g, s) for g, s in zip(got, singles))
    model.generate(ids, max_new_tokens=2, eos_token_id=[], do_sample=True, seed=1, repetition_penalty=1.2)
    assert model.last_decoding.startswith("sample(") and model.last_decoding.endswith(" + repetition_penalty=1.2")
    with pytest.warns(UserWarning, match="num_beams"):                  # what is not implemented keeps warning
        model.generate(ids, max_new_tokens=2, eos_token_id=[], num_beams=4, repetition_penalty=1.2)
    with pytest.raises(ValueError, match="repetition_penalty"):
        model.generate(ids, max_new_tokens=2, repetition_penalty=0.0)
    # generation_config.json: call arguments over the file over "off"
    (tmp_path / "generation_config.json").write_text(json.dumps({"repetition_penalty": 1.3, "min_new_tokens": 2, "top_k": 40, "num_beams": 1}))
    d = sampling.read_generation_config(str(tmp_path))
    assert d == {"top_k": 40, "repetition_penalty": 1.3, "min_new_tokens": 2}
    assert sampling.resolve_rules(d) == LogitsRules(1.3, 0, 2)
    assert sampling.resolve_rules(d, repetition_penalty=1.0, min_new_tokens=0) is None
    assert sampling.resolve_rules(d, no_repeat_ngram_size=3) == LogitsRules(1.3, 3, 2)
    assert sampling.resolve_rules({}) is None and sampling.resolve_rules(None, min_new_tokens=1) == LogitsRules(min_new_tokens=1)
    was = model.generation_defaults
    model.generation_defaults = d
    try:
        model.generate(ids, max_new_tokens=2, eos_token_id=[])
        assert model.last_decoding == "greedy + repetition_penalty=1.3 + min_new_tokens=2"
    finally:
        model.generation_defaults = was
    eng.release_batch_state()
