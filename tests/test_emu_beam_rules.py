"""Beam search with logits processors on the CPU: lmi_beam_step_rules and the id reorder through the kernel-logic emulator on the cases of
tests/beam_rules_ref.py, the argument checks, and ``generate_beams(rules=)`` on the micro configuration against a host loop that keeps one
batch-1 cache per beam and processes whole float64 rows (tests/beam_rules_ref.HostLoop)."""
import json
import warnings

import numpy as np
import pytest
import torch

from tests import beam_ref as R
from tests import beam_rules_ref as B
from tests.emu_util import emu_ops

DEV = "cpu"
STEP_CASES = B.step_cases()
T_NEW = 6
PROMPT_SEED = 5                        # tests/beam_ref.engine_prompt: the host loop has a near-tie step in 1 of the 8 cases with this draw
#                                        (seeds 0 .. 11 give 3, 2, 5, 3, 3, 1, 3, 2, 1, 3, 1, 1); if a run exceeds the cap, another seed


@pytest.fixture(scope="module")
def ops():
    return emu_ops()


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", STEP_CASES, ids=[c["name"] for c in STEP_CASES])
def test_beam_step_rules(ops, case):
    B.check_step(ops, DEV, case)


def test_beam_step_rules_production_vocabulary(ops):
    B.check_step(ops, DEV, B.big_case())


def test_cases_cover_what_they_claim():
    """About the cases alone (the float64 restatement): each named situation happens."""
    by = {c["name"]: c for c in STEP_CASES}
    top = lambda c, b: [int(i) for i in np.argsort(-np.where(np.isnan(B.processed(c)[b]), -np.inf, B.processed(c)[b]), kind="stable")
                        if i not in set(c["eos"]) | set(c["suppress"])][:c["K"]]
    c = by["penalty-moves-out"]
    assert all(B.raw_order(c, b)[c["K"] - 1] in B.seen_ids(c, b) and B.raw_order(c, b)[c["K"] - 1] not in top(c, b) for b in range(c["K"]))
    c = by["half-penalty-lifts-in"]
    assert all(B.raw_order(c, b)[c["K"]] in top(c, b) for b in range(c["K"]))
    c = by["bigram-bans-best"]
    assert all(B.processed(c)[b, B.raw_order(c, b)[0]] == -np.inf for b in range(c["K"])) and c["rules"][1] == 2
    c = by["all-best-banned"]
    assert all((B.processed(c)[b, B.raw_order(c, b)[:c["K"]]] == -np.inf).all() for b in range(c["K"])) and c["rules"][1] == 1
    c = by["seen-eos-and-suppressed"]
    e, s = c["eos"][0], c["suppress"][0]
    x64 = c["logits"][:, :c["V"]].double().numpy()
    plain = x64 - R.lse64(x64)[:, None]
    assert all(e in B.seen_ids(c, b) and s in B.seen_ids(c, b) for b in range(c["K"]))
    assert all(B.processed(c)[b, e] == plain[b, e] * 1.3 and np.isfinite(plain[b, e]) for b in range(c["K"]))   # log-probabilities are negative
    c = by["seen-eos-min-left"]
    assert all(B.processed(c)[b, e] == -np.inf for b in range(c["K"]) for e in c["eos"]) and c["rules"][2] > 0
    assert {len(B.seen_ids(c, 0)) for c in STEP_CASES} >= set(B.L.LENGTHS)
    assert any(t >= c["V"] for c in STEP_CASES for t in B.seen_ids(c, 0))
    assert {c["K"] for c in STEP_CASES} >= {1, 2, 4, 8} and {c["logits"].shape[0] for c in STEP_CASES} >= {1, 2, 4, 8}
    # the rules change the walk in most cases
    changed = sum([(w.parent, w.id) for w in B.ref_walk(c)] != [(w.parent, w.id) for w in B.ref_walk(dict(c, rules=(1.0, 0, 0)))] for c in STEP_CASES)
    assert changed >= len(STEP_CASES) // 2


def test_rules64_is_apply_in_float64():
    """The float64 restatement has apply's structure: the same -inf pattern, and apply's values to fp32 rounding."""
    g = torch.Generator().manual_seed(0)
    for p, n, ml in B.RULESETS:
        s = -torch.rand(200, generator=g) * 9
        seq = B.L.heavy_seq(50, 200, seed=n, extra=(3, 250))
        a, b = B.L.apply(s, seq, p, n, ml, [3, 7]).double().numpy(), B.rules64(s.double().numpy(), seq, p, n, ml, [3, 7])
        assert np.array_equal(np.isinf(a), np.isinf(b)) and np.allclose(a[np.isfinite(a)], b[np.isfinite(b)], rtol=1e-6)


def test_id_lists_follow_any_parent(ops):
    for K in (2, 4, 8):
        for name, parent in R.permutations_of(K).items():
            for first, held in ((0, 0), (0, 1), (3, 4), (2, 16), (5, 3)):
                B.check_id_reorder(ops, DEV, K, parent, first, held)


def test_beam_step_rules_refuses_bad_arguments(ops):
    B.check_rejects(ops, DEV)


# ---- the engine --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def micro(ops):
    from tests.test_emu_shared_decode import _engine_setup
    cfg, eng, u8, ids = _engine_setup(ops, torch.float16)
    ids = R.engine_prompt(cfg, ids, PROMPT_SEED)
    host = B.HostLoop(eng, cfg, ids, u8, torch.float16, DEV)
    return cfg, eng, u8, ids, host, R.pick_eos(host, 4, T_NEW)


def test_generate_beams_with_rules_against_the_host_loop(micro):
    cfg, eng, u8, ids, host, eos = micro
    cases, rules = B.engine_cases(), B.engine_rules()
    full, cuts, differ, held_back = 0, 0, 0, 0
    for K, decode, es, lp, name in cases:
        ok, cut, want, got = B.compare_with_host(eng, host, K, decode, es, lp, T_NEW, eos, rules[name])
        full += ok
        cuts += cut is not None
        held_back += host.held_back > 0
        plain = eng.generate_beams(ids, u8, K, max_new_tokens=T_NEW, eos_token_id=eos, length_penalty=lp, early_stopping=es, decode=decode)
        differ += ok and not torch.equal(plain.sequences[0], got.sequences[0])
    print(f"[generate_beams rules emulator] {full} / {len(cases)} cases identical at full length; host-loop near-tie steps in {cuts} cases; "
          f"{differ} cases differ from the call without rules; min_new_tokens held an eos back in {held_back}")
    assert cuts <= len(cases) // 8 and len(cases) - full <= len(cases) // 8
    assert differ >= 1                                                 # the rules change the best sequence
    assert held_back >= 1                                              # a hypothesis that min_new_tokens kept from ending early


def test_one_beam_with_ngram_and_minimum_is_greedy_with_rules(micro):
    from leopard_amd.engine import LogitsRules
    cfg, eng, u8, ids, host, eos = micro
    rules = LogitsRules(no_repeat_ngram_size=2, min_new_tokens=4)
    want = eng.generate(ids, u8, max_new_tokens=T_NEW, eos_token_id=eos, rules=rules)
    for decode in ("shared", "copy"):
        got = eng.generate_beams(ids, u8, 1, max_new_tokens=T_NEW, eos_token_id=eos, decode=decode, rules=rules)
        assert torch.equal(got.sequences[0], want), (decode, got.sequences[0].tolist(), want.tolist())


def test_a_call_without_rules_is_unchanged_after_one_with_rules(micro):
    from leopard_amd.engine import LogitsRules
    cfg, eng, u8, ids, host, eos = micro
    before = eng.generate_beams(ids, u8, 2, max_new_tokens=T_NEW, eos_token_id=eos, num_return_sequences=2)
    eng.generate_beams(ids, u8, 2, max_new_tokens=T_NEW, eos_token_id=eos, rules=LogitsRules(repetition_penalty=1.3, no_repeat_ngram_size=2))
    st = eng._batch_states[("shared", 2)]
    assert st.seq is not None and st.rules is False and st.beams == 0
    after = eng.generate_beams(ids, u8, 2, max_new_tokens=T_NEW, eos_token_id=eos, num_return_sequences=2)
    assert all(torch.equal(a, b) for a, b in zip(before.sequences, after.sequences)) and before.scores == after.scores
    off = eng.generate_beams(ids, u8, 2, max_new_tokens=T_NEW, eos_token_id=eos, num_return_sequences=2, rules=LogitsRules())
    assert all(torch.equal(a, b) for a, b in zip(before.sequences, off.sequences)) and before.scores == off.scores   # everything off is no rule


def test_refusals(micro):
    from leopard_amd.engine import LogitsRules
    cfg, eng, u8, ids, host, eos = micro
    launches = []
    was = eng.prefill
    eng.prefill = lambda *a, **k: launches.append(1) or was(*a, **k)
    rules = LogitsRules(repetition_penalty=1.3, min_new_tokens=2)
    try:
        with pytest.raises(TypeError, match="LogitsRules"):
            eng.generate_beams(ids, u8, 2, rules=dict(repetition_penalty=1.3))
        with pytest.raises(NotImplementedError, match="eos ids"):
            eng.generate_beams(ids, u8, 2, eos_token_id=tuple(range(5, 5 + eng.MAX_EOS + 1)), rules=rules)
        was_max = eng.ops.RULES_MAX_VOCAB
        eng.ops.RULES_MAX_VOCAB = 8
        try:
            with pytest.raises(NotImplementedError, match="vocabulary"):
                eng.generate_beams(ids, u8, 2, rules=rules)
        finally:
            del eng.ops.RULES_MAX_VOCAB
            assert eng.ops.RULES_MAX_VOCAB == was_max
        for attr, obj, val, match in (("tp_size", eng.W, 2, "tensor-parallel"), ("_fp8", eng, object(), "fp8"), ("split_operands", eng, True, "split")):
            had, old = hasattr(obj, attr), getattr(obj, attr, None)
            setattr(obj, attr, val)
            try:
                for decode in ("shared", "copy"):
                    with pytest.raises(NotImplementedError, match=match):
                        eng.generate_beams(ids, u8, 2, decode=decode, rules=rules)
            finally:
                setattr(obj, attr, old) if had else delattr(obj, attr)
        assert not launches
    finally:
        eng.prefill = was


# ---- the surfaces --------------------------------------------------------------------------------------------------------------------
def test_model_object_surface(micro, ops, tmp_path):
    from leopard_amd import compat, sampling
    from leopard_amd.engine import LogitsRules
    from leopard_amd.weights import SynthSource
    cfg, eng, u8, ids, host, eos = micro
    m = compat.LeopardForConditionalGeneration(cfg, lambda dev, dt: SynthSource(cfg, ops, dev, dt), torch.float16, ops, torch_dtype=torch.float16)
    m = m.to("cpu").eval()
    rules = LogitsRules(repetition_penalty=1.3, no_repeat_ngram_size=2)
    want = eng.generate_beams(ids, u8, 2, max_new_tokens=4, eos_token_id=eos, decode="shared", rules=rules)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = m.generate_beams(ids, u8, num_beams=2, max_new_tokens=4, eos_token_id=list(eos), repetition_penalty=1.3, no_repeat_ngram_size=2)
    assert torch.equal(got, want.sequences[0])
    assert m.last_decoding == "beam(2, length_penalty=1.0) + repetition_penalty=1.3 + no_repeat_ngram_size=2"
    # a generation_config.json with beam keys and rule keys: what the explicit call gives
    (tmp_path / "generation_config.json").write_text(json.dumps({"num_beams": 2, "repetition_penalty": 1.3, "no_repeat_ngram_size": 2}))
    m.generation_defaults, m.beam_defaults = sampling.read_generation_defaults(str(tmp_path))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert torch.equal(m.generate_beams(ids, u8, max_new_tokens=4, eos_token_id=list(eos)), want.sequences[0])
    assert m.last_decoding == "beam(2, length_penalty=1.0) + repetition_penalty=1.3 + no_repeat_ngram_size=2"
    # a call argument wins over the file; everything off is no rule and the plain description
    plain = eng.generate_beams(ids, u8, 2, max_new_tokens=4, eos_token_id=eos, decode="shared")
    assert torch.equal(m.generate_beams(ids, u8, max_new_tokens=4, eos_token_id=list(eos), repetition_penalty=1.0, no_repeat_ngram_size=0),
                       plain.sequences[0])
    assert m.last_decoding == "beam(2, length_penalty=1.0)"
    with pytest.warns(UserWarning, match="diversity_penalty"):
        m.generate_beams(ids, u8, num_beams=2, max_new_tokens=2, eos_token_id=[], diversity_penalty=0.5, min_new_tokens=1)
