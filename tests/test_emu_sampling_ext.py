"""min_p, typical_p, epsilon_cutoff and eta_cutoff on the CPU: lmi_decode_sample_ex through the kernel-logic emulator (the kept set is the
set of the draws, chi-square, all four off = lmi_decode_sample, rows independent of slot and batch) on the case list shared with
tests/test_gpu_sampling_ext.py, the generate() surfaces' arguments without a kernel launch, and the engine over the emulated kernels."""
import json
import warnings

import pytest
import torch

from tests.emu_util import emu_ops
from tests import sampling_ext_ref as X
from tests.row_kernels_ref import HEAD, gapped_row


@pytest.fixture(scope="module")
def ops():
    return emu_ops()


# ---- the kernel ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(X.GAPPED_CASES)))
def test_kept_set_is_the_set_of_draws_fewer_tokens_than_threads(ops, case):
    V = 1000                                                          # ld = 1024, 100.0 behind the vocabulary: never drawn
    X.check_kept_set_equals_draws(ops, gapped_row(V, HEAD, seed=1, ld=1024), V, X.GAPPED_CASES[case], 64, 16)


@pytest.mark.parametrize("case", [0, 4, 7, 9, 14])                    # each warper alone and all four: the scalar path
def test_kept_set_on_rows_that_are_not_16_byte_aligned(ops, case):
    V = 1003
    row = gapped_row(V, HEAD, seed=2)
    X.check_kept_set_equals_draws(ops, row, V, X.GAPPED_CASES[case], 64, 16, logits=X.unaligned_rows(row, 64, "cpu"))


@pytest.mark.parametrize("case", range(len(X.BROAD_CASES)))
def test_kept_set_on_the_broad_row_where_typical_p_removes_the_top_token(ops, case):
    row = X.broad_row()
    kept, notes = X.check_kept_set_equals_draws(ops, row, row.numel(), X.BROAD_CASES[case], 128, 16)
    if case < 3:
        assert notes["top_removed"] and int(row.argmax()) not in kept


@pytest.mark.parametrize("case", range(len(X.TIE_CASES)))
def test_tie_groups_on_the_boundaries_are_kept_whole(ops, case):
    row = X.tie_row()
    _, notes = X.check_kept_set_equals_draws(ops, row, row.numel(), X.TIE_CASES[case], 64, 8)
    assert max(notes.get(key, 0) for key in ("typ_group", "eps_group", "eta_group")) >= 2


def test_one_allowed_token_suppressed_ids_and_rows_without_a_drawable_token(ops):
    X.check_special_rows(ops, "cpu")


def test_distribution_chi_square(ops):
    X.check_chi_square(ops, "cpu", 1000, n_rows=64, n_steps=10)


def test_all_four_off_is_decode_sample(ops):
    X.check_all_off_equals_decode_sample(ops, "cpu", 300)


def test_rows_with_different_parameters_match_their_solo_launches(ops):
    X.check_rows_are_independent(ops, "cpu", 300)


def test_values_outside_their_ranges_act_as_off_and_never_fault(ops):
    V, n = 300, 4
    logits = torch.randn(n, V, generator=torch.Generator().manual_seed(4)) * 2.0
    temp, k, p, _ = X.ext_tensors(n, X.params(k=20, p=0.9), "cpu")
    a, b = X._state(n, "cpu"), X._state(n, "cpu")
    bad = dict(min_p=torch.tensor([-1.0, float("nan"), 0.0, -0.0]), typical_p=torch.tensor([0.0, -3.0, float("nan"), 7.0]),
               epsilon_cutoff=torch.tensor([1.0, -1.0, float("inf"), float("nan")]), eta_cutoff=torch.tensor([1.5, -0.1, float("nan"), 1.0]))
    ops.decode_sample(logits, V, temp, k, p, a["seed"], a["step"], a["tok"], a["pos"])
    ops.decode_sample_ex(logits, V, temp, k, p, b["seed"], b["step"], b["tok"], b["pos"], **bad)
    assert torch.equal(a["tok"], b["tok"])
    ops.decode_sample_ex(logits, V, temp, k, p, b["seed"], b["step"], b["tok"], b["pos"], min_p=torch.full((n,), 9.0))     # acts as 1.0
    assert torch.equal(b["tok"], logits.argmax(1))
    with pytest.raises(TypeError):
        ops.decode_sample_ex(logits, V, temp, k, p, b["seed"], b["step"], b["tok"], b["pos"], min_p=torch.zeros(n, dtype=torch.float64))
    with pytest.raises(RuntimeError):                                 # LMI_EINVAL for the host arguments, as lmi_decode_sample
        ops.decode_sample_ex(logits, V + 1, temp, k, p, b["seed"], b["step"], b["tok"], b["pos"])


# ---- SamplingParams and the generate() surfaces' arguments (no kernel launch) --------------------------------------------------------------
def test_sampling_params_fields_ranges_and_descriptions():
    from leopard_amd.engine import SamplingParams
    sp = SamplingParams(0.8, 1, 1.0, 5)                               # the positional construction of before
    assert (sp.min_p, sp.typical_p, sp.epsilon_cutoff, sp.eta_cutoff) == (0.0, 1.0, 0.0, 0.0) and not sp.extended
    assert sp.describe() == "sample(temperature=0.8, top_k=1, top_p=1)"
    sp = SamplingParams(1.0, 50, 0.9, 7, 0.05, 0.9, 3e-4, 2e-3)
    assert sp.extended and sp.describe() == "sample(temperature=1, top_k=50, top_p=0.9, min_p=0.05, typical_p=0.9, epsilon_cutoff=0.0003, eta_cutoff=0.002)"
    assert SamplingParams(min_p=0.1).describe() == "sample(temperature=1, top_k=50, top_p=1, min_p=0.1)"
    r = sp.for_request(3)
    assert (r.min_p, r.typical_p, r.epsilon_cutoff, r.eta_cutoff) == (0.05, 0.9, 3e-4, 2e-3) and r.seed != sp.seed
    assert SamplingParams(min_p=None).min_p == 0.0 and SamplingParams(min_p=1.0).extended
    for bad in (dict(min_p=-0.1), dict(min_p=1.5), dict(typical_p=0.0), dict(typical_p=1.2), dict(epsilon_cutoff=1.0), dict(epsilon_cutoff=-1e-3),
                dict(eta_cutoff=1.0), dict(eta_cutoff=-0.5), dict(min_p=float("nan")), dict(typical_p=float("nan"))):
        with pytest.raises(ValueError):
            SamplingParams(**bad)


def test_resolve_takes_call_arguments_over_generation_config_over_off():
    from leopard_amd import sampling
    assert set(sampling.WARPER_OFF) <= set(sampling.SAMPLING_KEYS) and set(sampling.WARPER_OFF) <= set(sampling.UNSUPPORTED)
    cfg = {"do_sample": True, "min_p": 0.05, "eta_cutoff": 2e-3}
    sp = sampling.resolve(cfg, None, seed=1)
    assert (sp.min_p, sp.typical_p, sp.epsilon_cutoff, sp.eta_cutoff) == (0.05, 1.0, 0.0, 2e-3)
    sp = sampling.resolve(cfg, None, seed=1, min_p=0.2, typical_p=0.9)
    assert (sp.min_p, sp.typical_p, sp.eta_cutoff) == (0.2, 0.9, 2e-3)
    assert sampling.resolve(cfg, None, seed=1, min_p=0.0, eta_cutoff=0.0).extended is False          # an explicit "off" wins over the file
    assert sampling.resolve(cfg, False, min_p=0.3) is None and sampling.resolve({}, None, min_p=7.0) is None     # greedy: ignored, as temperature
    sp = sampling.resolve({}, True, seed=1)
    assert not sp.extended and sampling.describe(sp) == "sample(temperature=1, top_k=50, top_p=1)"
    for kw in (dict(min_p=1.5), dict(typical_p=0.0), dict(epsilon_cutoff=1.0), dict(eta_cutoff=-1.0)):
        with pytest.raises(ValueError):
            sampling.resolve({}, True, seed=1, **kw)


def _llava(tmp_path, gen=None):
    from leopard_amd import compat
    from leopard_amd.checkpoint import save_synthetic_checkpoint
    from tests.test_emu_engine import micro_config
    d = tmp_path / "llava"
    save_synthetic_checkpoint(str(d), micro_config())
    if gen is not None:
        (d / "generation_config.json").write_text(json.dumps(gen))
    return compat.from_pretrained(str(d))


def test_generation_config_values_reach_the_surfaces_without_a_warning(tmp_path):
    m = _llava(tmp_path, {"do_sample": True, "temperature": 0.6, "min_p": 0.05, "typical_p": 0.95, "eos_token_id": 1})
    assert m.generation_defaults == {"do_sample": True, "temperature": 0.6, "min_p": 0.05, "typical_p": 0.95}
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                # the four no longer reach warn_unsupported from the surfaces
        sp, _ = m._sampling("generate", {}, None, None, None, None, 3, min_p=None, typical_p=None, epsilon_cutoff=1e-3, eta_cutoff=None)
    assert (sp.temperature, sp.min_p, sp.typical_p, sp.epsilon_cutoff, sp.eta_cutoff) == (0.6, 0.05, 0.95, 1e-3, 0.0)
    assert m.last_decoding == "sample(temperature=0.6, top_k=50, top_p=1, min_p=0.05, typical_p=0.95, epsilon_cutoff=0.001)"
    import inspect
    from leopard_amd import idefics2_compat as IC
    for fn in (m.generate, m.generate_batch, m.generate_stream, m.generate_shared, IC.Idefics2ForConditionalGeneration.generate):
        assert {"min_p", "typical_p", "epsilon_cutoff", "eta_cutoff"} <= set(inspect.signature(fn).parameters), fn
    assert "min_p" not in inspect.signature(m.generate_beams).parameters


# ---- the engine over the emulated kernels -------------------------------------------------------------------------------------------------
class _Spy:
    """Counts the choice launches of an Ops without changing them."""

    def __init__(self, ops):
        self.ops, self.calls = ops, []
        self._saved = {name: getattr(ops, name) for name in ("decode_sample", "decode_sample_ex", "decode_advance")}

    def __enter__(self):
        for name, fn in self._saved.items():
            setattr(self.ops, name, (lambda *a, _n=name, _f=fn, **kw: (self.calls.append(_n), _f(*a, **kw))[1]))
        return self

    def __exit__(self, *exc):
        for name in self._saved:
            delattr(self.ops, name)


def _micro_engine(ops):
    from leopard_amd.engine import LeopardEngine
    from leopard_amd.weights import EngineWeights, SynthSource
    from tests.test_emu_engine import micro_config
    cfg = micro_config()
    W = EngineWeights.build(cfg, SynthSource(cfg, ops, "cpu", torch.float16), torch.float16)
    return LeopardEngine(cfg, W, ops=ops, device="cpu")


def test_engine_uses_the_new_entry_only_for_calls_with_a_warper_on(ops):
    from leopard_amd.engine import SamplingParams
    eng = _micro_engine(ops)
    ids = torch.tensor([[7, 8, 9, 10]])
    gen = lambda sp: eng.generate(ids, None, max_new_tokens=5, eos_token_id=(), sampling=sp)
    hot = SamplingParams(temperature=50.0, top_k=0, top_p=1.0, seed=11)
    with _Spy(ops) as spy:
        before = gen(hot)
        assert set(spy.calls) == {"decode_sample"}
        del spy.calls[:]
        ext = gen(SamplingParams(50.0, 0, 1.0, 11, min_p=0.5, typical_p=0.9))
        assert set(spy.calls) == {"decode_sample_ex"} and len(spy.calls) == 5
        assert torch.equal(gen(SamplingParams(50.0, 0, 1.0, 11, min_p=0.5, typical_p=0.9)), ext) and not torch.equal(ext, before)
        del spy.calls[:]
        assert torch.equal(gen(hot), before) and set(spy.calls) == {"decode_sample"}
        greedy = eng.generate(ids, None, max_new_tokens=5, eos_token_id=())
        assert torch.equal(gen(SamplingParams(50.0, 0, 1.0, 3, min_p=1.0)), greedy)                   # only the top token passes min_p = 1
        assert torch.equal(gen(SamplingParams(50.0, 0, 1.0, 3, epsilon_cutoff=0.99)), greedy)
    eng.W.tp_size = 2                                                 # (what a tensor-parallel rank's weights say)
    with _Spy(ops) as spy:
        with pytest.raises(NotImplementedError):
            gen(SamplingParams(1.0, 0, 1.0, 3, eta_cutoff=0.1))
        assert spy.calls == []                                        # refused before anything is launched


def test_engine_stream_and_batch_with_warpers_do_not_depend_on_batch_size(ops):
    from leopard_amd.engine import LogitsRules, SamplingParams
    eng = _micro_engine(ops)
    eng.HIST = 2
    samples = [(torch.tensor([[5, 6, 7]]), None), (torch.tensor([[9, 3]]), None), (torch.tensor([[11, 12, 13, 14]]), None)]
    sp = SamplingParams(temperature=50.0, top_k=0, top_p=1.0, seed=99, min_p=0.4, typical_p=0.8, eta_cutoff=0.01)
    one = eng.generate_stream(samples, batch_size=1, max_new_tokens=4, eos_token_id=(), sampling=sp)
    three = eng.generate_stream(samples, batch_size=3, max_new_tokens=4, eos_token_id=(), sampling=sp)
    assert all(torch.equal(x, y) for x, y in zip(one, three)), ([o.tolist() for o in one], [t.tolist() for t in three])
    batch = eng.generate_batch(samples, max_new_tokens=4, eos_token_id=(), sampling=sp)
    assert all(torch.equal(x, y) for x, y in zip(one, batch))
    plain = eng.generate_stream(samples, batch_size=3, max_new_tokens=4, eos_token_id=(), sampling=SamplingParams(50.0, 0, 1.0, 99))
    assert any(not torch.equal(x, y) for x, y in zip(plain, three))
    # with rules and with logprobs (of the raw row): the calls run, reproducibly
    a = eng.generate(samples[0][0], None, max_new_tokens=4, eos_token_id=(), sampling=sp, rules=LogitsRules(repetition_penalty=1.3))
    b = eng.generate(samples[0][0], None, max_new_tokens=4, eos_token_id=(), sampling=sp, rules=LogitsRules(repetition_penalty=1.3))
    assert torch.equal(a, b)
    out = eng.generate(samples[0][0], None, max_new_tokens=4, eos_token_id=(), sampling=sp, logprobs=2)
    assert torch.equal(out.sequences, one[0]) and out.token_logprobs[0].numel() == 4
