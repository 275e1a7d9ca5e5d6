"""-m gpu: beam search with logits processors on the MI355X — lmi_beam_step_rules and the id reorder on the cases of
tests/beam_rules_ref.py (the production vocabulary included), both captured in one graph and replayed with other device values, and
``generate_beams(rules=)`` on the 2 + 2-layer mid model against a host loop that keeps one batch-1 cache per beam."""
import json
import warnings

import pytest
import torch

from tests import beam_ref as R
from tests import beam_rules_ref as B

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEP_CASES = B.step_cases()
T_NEW = 6
PROMPT_SEED = 8                         # tests/beam_ref.engine_prompt: the host loop has a near-tie step in 0 of the 8 cases with this draw
#                                         (seeds 0 .. 11 give 4, 6, 3, 2, 4, 5, 3, 3, 0, 3, 3, 3); if a run exceeds the cap, another seed — never another cap


@pytest.fixture(scope="module")
def ops():
    from leopard_amd.ops import Ops
    return Ops()


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", STEP_CASES, ids=[c["name"] for c in STEP_CASES])
def test_beam_step_rules(ops, case):
    B.check_step(ops, DEV, case)


def test_beam_step_rules_production_vocabulary(ops):
    B.check_step(ops, DEV, B.big_case())


def test_id_lists_follow_any_parent(ops):
    for K in (2, 4, 8):
        for name, parent in R.permutations_of(K).items():
            for first, held in ((0, 0), (0, 1), (3, 4), (2, 16), (5, 3)):
                B.check_id_reorder(ops, DEV, K, parent, first, held)


def test_beam_step_rules_refuses_bad_arguments(ops):
    B.check_rejects(ops, DEV)


def test_entry_and_id_reorder_replay_from_a_graph(ops):
    """The entry and the id reorder captured in one HIP graph, replayed with other device values (penalty, n, min_left, lengths, ids, eos,
    scores): what the eager launches give."""
    from leopard_amd.engine import _capture_safe
    first = next(c for c in STEP_CASES if c["name"] == "V1003-K4-rules2")
    other = B.random_case("replay-other-values", 1003, 4, 2, 40, (0.8, 1, 3), n_sup=2, seed=77)
    other = dict(other, logits=first["logits"], suppress=first["suppress"], cap=first["cap"])      # the launch arguments stay; device values change
    assert len(B.seen_ids(other, 0)) != len(B.seen_ids(first, 0)) and other["rules"] != first["rules"] and other["eos"] != first["eos"]
    x, eos, sup, row0, held = B.device_args(first, DEV)
    o = B.buffers(first, DEV)
    ptrs = torch.tensor([o["seq"].data_ptr()], dtype=torch.int64, device=DEV)
    body = lambda: B.launch(ops, first, x, eos, sup, o, row0, held, ptrs)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream(DEV).wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with _capture_safe(), torch.cuda.graph(g):
        body()
    for case in (first, other):
        _, eos2, _, row02, held2 = B.device_args(case, DEV)
        eos.copy_(eos2); row0.copy_(row02); held.copy_(held2)
        for k, v in B.buffers(case, DEV).items():
            o[k].copy_(v)
        g.replay()
        torch.cuda.synchronize()
        want = B.run_step(ops, DEV, case)
        for k in o:
            got = o[k].cpu()
            assert R.same_bits(got, want[k]) if got.dtype == torch.float32 else torch.equal(got, want[k]), (case["name"], k)
        assert int(o["walk"][0]) >= case["K"]


# ---- the engine, mid model -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mid():
    from leopard_amd import compat
    from leopard_amd.config import mid_config
    from leopard_amd.ops import Ops
    from leopard_amd.weights import SynthSource
    from tools.gen_fulldepth_fixtures import sample_inputs
    cfg, ops = mid_config(), Ops()
    m = compat.LeopardForConditionalGeneration(cfg, lambda dev, dt: SynthSource(cfg, ops, dev, dt), torch.float16, ops, torch_dtype=torch.float16)
    m = m.to(DEV)
    u8, ids = sample_inputs(cfg, 1, 336, 336, seed=4)[:2]
    tiles, ids = torch.from_numpy(u8).to(DEV), R.engine_prompt(cfg, ids, PROMPT_SEED).to(DEV)
    host = B.HostLoop(m.engine, cfg, ids, tiles, torch.float16, DEV)
    return m, cfg, m.engine, tiles, ids, host, R.pick_eos(host, 4, T_NEW)


def test_generate_beams_with_rules_against_the_host_loop(mid):
    """tests/beam_rules_ref.engine_cases: the host loop's hypotheses and, within the two paths' rounding, its scores.  A case whose host
    loop has a near-tie step may end at that step; at most one in eight."""
    m, cfg, eng, tiles, ids, host, eos = mid
    cases, rules = B.engine_cases(), B.engine_rules()
    full, cuts, differ, held_back = 0, 0, 0, 0
    for K, decode, es, lp, name in cases:
        ok, cut, want, got = B.compare_with_host(eng, host, K, decode, es, lp, T_NEW, eos, rules[name])
        full += ok
        cuts += cut is not None
        held_back += host.held_back > 0
        plain = eng.generate_beams(ids, tiles, K, max_new_tokens=T_NEW, eos_token_id=eos, length_penalty=lp, early_stopping=es, decode=decode)
        differ += ok and not torch.equal(plain.sequences[0], got.sequences[0])
    print(f"[generate_beams rules mid] {full} / {len(cases)} cases identical at full length; host-loop near-tie steps in {cuts} cases; "
          f"{differ} cases differ from the call without rules; min_new_tokens held an eos back in {held_back}")
    assert len(cases) - full <= len(cases) // 8
    assert differ >= 1                                                 # the rules change the best sequence
    assert held_back >= 1                                              # a hypothesis that min_new_tokens kept from ending early


def test_one_beam_with_ngram_and_minimum_is_greedy_with_rules(mid):
    from leopard_amd.engine import LogitsRules
    from tests.test_gpu_shared_decode import assert_equal_or_near_tie
    m, cfg, eng, tiles, ids, host, eos = mid
    rules = LogitsRules(no_repeat_ngram_size=2, min_new_tokens=4)
    want = eng.generate(ids, tiles, max_new_tokens=T_NEW, eos_token_id=eos, rules=rules)
    for decode in ("shared", "copy"):
        got = eng.generate_beams(ids, tiles, 1, max_new_tokens=T_NEW, eos_token_id=eos, decode=decode, rules=rules)
        n = min(got.sequences[0].shape[1], want.shape[1])
        same = assert_equal_or_near_tie(eng, cfg, ids, tiles, want[:, :n], got.sequences[0][:, :n])
        assert got.sequences[0].shape == want.shape or not same        # another length: one stopped at an eos the other missed, on a near tie


def test_a_call_without_rules_replays_the_plain_graph(mid):
    """The step with rules is one more captured graph of the state; a call without rules afterwards replays the plain beam graph and gives
    its earlier result bit for bit."""
    from leopard_amd.engine import LogitsRules
    m, cfg, eng, tiles, ids, host, eos = mid
    for decode, key in (("shared", ("shared", 4)), ("copy", 4)):
        eng.release_batch_state()
        before = eng.generate_beams(ids, tiles, 4, max_new_tokens=T_NEW, eos_token_id=eos, num_return_sequences=4, decode=decode)
        st = eng._batch_states[key]
        assert len(st.graphs) == 1 and st.seq is None
        plain = next(iter(st.graphs.values()))
        eng.generate_beams(ids, tiles, 4, max_new_tokens=T_NEW, eos_token_id=eos, decode=decode,
                           rules=LogitsRules(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=3))
        assert eng._batch_states[key] is st and len(st.graphs) == 2 and st.seq is not None and st.rules is False and st.beams == 0
        eng.generate_beams(ids, tiles, 4, max_new_tokens=T_NEW, eos_token_id=eos[:1], decode=decode, rules=LogitsRules(repetition_penalty=0.8))
        assert len(st.graphs) == 2                                     # other rule values and eos ids: the same graph
        after = eng.generate_beams(ids, tiles, 4, max_new_tokens=T_NEW, eos_token_id=eos, num_return_sequences=4, decode=decode)
        assert len(st.graphs) == 2 and plain in st.graphs.values()
        assert all(torch.equal(a, b) for a, b in zip(before.sequences, after.sequences)) and before.scores == after.scores
    eng.release_batch_state()


def test_refusals(mid):
    from leopard_amd.engine import LogitsRules
    m, cfg, eng, tiles, ids, host, eos = mid
    launches = []
    was = eng.prefill
    eng.prefill = lambda *a, **k: launches.append(1) or was(*a, **k)
    rules = LogitsRules(repetition_penalty=1.3, min_new_tokens=2)
    try:
        with pytest.raises(TypeError, match="LogitsRules"):
            eng.generate_beams(ids, tiles, 2, rules=dict(repetition_penalty=1.3))
        with pytest.raises(NotImplementedError, match="eos ids"):
            eng.generate_beams(ids, tiles, 2, eos_token_id=tuple(range(5, 5 + eng.MAX_EOS + 1)), rules=rules)
        for attr, obj, val, match in (("tp_size", eng.W, 2, "tensor-parallel"), ("_fp8", eng, object(), "fp8"), ("split_operands", eng, True, "split")):
            had, old = hasattr(obj, attr), getattr(obj, attr, None)
            setattr(obj, attr, val)
            try:
                with pytest.raises(NotImplementedError, match=match):
                    eng.generate_beams(ids, tiles, 2, rules=rules)
            finally:
                setattr(obj, attr, old) if had else delattr(obj, attr)
        assert not launches
    finally:
        eng.prefill = was


# ---- the surfaces --------------------------------------------------------------------------------------------------------------------
def test_model_object_surface(mid, tmp_path):
    from leopard_amd import sampling
    from leopard_amd.engine import LogitsRules
    m, cfg, eng, tiles, ids, host, eos = mid
    rules = LogitsRules(repetition_penalty=1.3, no_repeat_ngram_size=2)
    want = eng.generate_beams(ids, tiles, 2, max_new_tokens=4, eos_token_id=eos, decode="shared", rules=rules)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = m.generate_beams(ids, tiles, num_beams=2, max_new_tokens=4, eos_token_id=list(eos), repetition_penalty=1.3, no_repeat_ngram_size=2)
    assert torch.equal(got, want.sequences[0])
    assert m.last_decoding == "beam(2, length_penalty=1.0) + repetition_penalty=1.3 + no_repeat_ngram_size=2"
    (tmp_path / "generation_config.json").write_text(json.dumps({"num_beams": 2, "repetition_penalty": 1.3, "no_repeat_ngram_size": 2}))
    had = m.generation_defaults, m.beam_defaults
    m.generation_defaults, m.beam_defaults = sampling.read_generation_defaults(str(tmp_path))
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            assert torch.equal(m.generate_beams(ids, tiles, max_new_tokens=4, eos_token_id=list(eos)), want.sequences[0])
        assert m.last_decoding == "beam(2, length_penalty=1.0) + repetition_penalty=1.3 + no_repeat_ngram_size=2"
    finally:
        m.generation_defaults, m.beam_defaults = had
    eng.release_batch_state()


def test_idefics2_surface_takes_the_rules(ops):
    """Idefics2 (sliding window, decode="copy", a suppress_tokens list): the named parameters run without a warning and give the engine's call."""
    import numpy as np
    from leopard_amd import idefics2_compat as IC
    from leopard_amd.config import idefics2_mid_config
    from leopard_amd.engine import LogitsRules
    from leopard_amd.idefics2 import Idefics2SynthSource
    cfg = idefics2_mid_config()
    m = IC.Idefics2ForConditionalGeneration(cfg, lambda dev, dt: Idefics2SynthSource(cfg, ops, dev, dt), torch.float16, ops, eos_token_id=(2,)).to(DEV)
    ids = torch.from_numpy(np.random.default_rng(2).integers(3, 7000, (1, 12))).to(DEV)
    rules = LogitsRules(repetition_penalty=1.2, no_repeat_ngram_size=3, min_new_tokens=2)
    want = m.engine.generate_beams(ids, None, 4, max_new_tokens=T_NEW, eos_token_id=(2,), decode="copy", rules=rules)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = m.generate_beams(ids, num_beams=4, max_new_tokens=T_NEW, repetition_penalty=1.2, no_repeat_ngram_size=3, min_new_tokens=2)
    assert torch.equal(got, want.sequences[0])
    assert m.last_decoding == "beam(4, length_penalty=1.0) + repetition_penalty=1.2 + no_repeat_ngram_size=3 + min_new_tokens=2"
    assert not set(got[0, 12:].tolist()) & set(m.bad_words_ids)
    m.engine.release_batch_state()
