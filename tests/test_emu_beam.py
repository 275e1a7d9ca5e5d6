"""Beam search on the CPU: lmi_beam_step and lmi_beam_reorder through the kernel-logic emulator on the cases of tests/beam_ref.py, their
argument checks, and ``generate_beams`` on the micro configuration of tests/test_emu_shared_decode.py against a host loop that keeps one
batch-1 cache per beam (tests/beam_ref.HostLoop)."""
import numpy as np
import pytest
import torch

from tests import beam_ref as R
from tests.emu_util import emu_ops

DEV = "cpu"
STEP_CASES = R.step_cases()
T_NEW = 5
PROMPT_SEED = 1                        # tests/beam_ref.engine_prompt: with this draw no host-loop step of the nine cases is a near tie


@pytest.fixture(scope="module")
def ops():
    return emu_ops()


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", STEP_CASES, ids=[c["name"] for c in STEP_CASES])
def test_beam_step(ops, case):
    R.check_beam_step(ops, DEV, case)


def test_beam_step_production_vocabulary(ops):
    R.check_beam_step(ops, DEV, R.big_case())


def test_beam_step_cases_cover_what_they_claim():
    """About the cases alone: eos entries inside and outside the first K ranks, walks longer than K, a first step, a beam that dies."""
    walks = {c["name"]: R.ref_walk(c) for c in STEP_CASES if not c["order_only"]}
    assert any(w.is_eos and w.rank < c["K"] for c in STEP_CASES if not c["order_only"] for w in walks[c["name"]])
    assert any(w.is_eos and w.rank >= c["K"] for c in STEP_CASES if not c["order_only"] for w in walks[c["name"]])
    assert any(len({w.parent for w in walks[c["name"]] if not w.is_eos}) < c["K"] for c in STEP_CASES if not c["order_only"] and c["logits"].shape[0] > 1)
    two = R.ref_walk(next(c for c in STEP_CASES if c["name"] == "best-two-are-eos"))
    assert [w.is_eos for w in two if w.parent == 1][:2] == [True, True]
    ties = R.ref_walk(next(c for c in STEP_CASES if c["name"] == "exact-ties"), np.float32)
    assert [(w.parent, w.id) for w in ties[:5]] == [(0, 5), (0, 100), (0, 700), (0, 701), (1, 5)]     # beam ascending, id ascending; 9 suppressed


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("width", [128, 1024])
def test_beam_reorder(ops, dtype, width):
    gen = np.random.default_rng(width)
    for K in (2, 4, 8):
        for name, parent in R.permutations_of(K).items():
            for held, row0 in R.REORDER_ROWS:
                R.check_beam_reorder(ops, DEV, dtype, width, K, held, row0, parent, gen)


def test_beam_entries_refuse_bad_arguments(ops):
    case = STEP_CASES[0]
    x, V, K = case["logits"], case["V"], 2
    eos = torch.full((4,), -1, dtype=torch.int64)
    mk = lambda: dict(score=torch.zeros(8), tok=torch.zeros(8, dtype=torch.int64), parent=torch.zeros(8, dtype=torch.int32),
                      walk=torch.zeros(R.WALK_WORDS, dtype=torch.int32), row_lse=torch.zeros(2), row_id=torch.zeros(2, 8, dtype=torch.int32),
                      row_lp=torch.zeros(2, 8), row_eos_lp=torch.zeros(2, 4))
    rows = torch.zeros(2, x.shape[1])
    ops.beam_step(rows, V, K, eos, **mk())
    with pytest.raises(ValueError, match="num_beams"):
        ops.beam_step(rows, V, 9, eos, **mk())
    with pytest.raises(ValueError, match="num_beams"):
        ops.beam_step(torch.zeros(3, x.shape[1]), V, 2, eos, **mk())
    with pytest.raises(TypeError, match="eos"):
        ops.beam_step(rows, V, K, eos[:2], **mk())
    with pytest.raises(TypeError, match="walk"):
        ops.beam_step(rows, V, K, eos, **dict(mk(), walk=torch.zeros(10, dtype=torch.int32)))
    with pytest.raises(TypeError, match="fp32"):
        ops.beam_step(rows.half(), V, K, eos, **mk())
    with pytest.raises(RuntimeError, match="lmi_beam_step"):
        ops.beam_step(rows, rows.shape[1] + 1, K, eos, **mk())         # ld_logits < vocab: the C entry's own check
    with pytest.raises(RuntimeError, match="lmi_beam_step"):
        ops._check(ops.lib.lmi_beam_step(None, *([0] * 19)))          # null pointers
    t = torch.zeros(2 * 4, 128, dtype=torch.float16)
    ptrs, par, one = torch.tensor([t.data_ptr()], dtype=torch.int64), torch.zeros(8, dtype=torch.int32), torch.ones(1, dtype=torch.int32)
    ops.beam_reorder(ptrs, par, 2, one, one, 256, 4, 256)
    with pytest.raises(ValueError, match="max_rows"):
        ops.beam_reorder(ptrs, par, 2, one, one, 256, 4, 100)
    with pytest.raises(ValueError, match="row_bytes"):
        ops.beam_reorder(ptrs, par, 2, one, one, 250, 4, 256)
    with pytest.raises(ValueError, match="num_beams"):
        ops.beam_reorder(ptrs, par, 9, one, one, 256, 4, 256)
    with pytest.raises(TypeError, match="parent"):
        ops.beam_reorder(ptrs, par.long(), 2, one, one, 256, 4, 256)
    with pytest.raises(RuntimeError, match="lmi_beam_reorder"):
        ops._check(ops.lib.lmi_beam_reorder(None, 1, None, 2, None, None, 256, 4, 256, None))
    assert not t.any()


# ---- the engine --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def micro(ops):
    from tests.test_emu_shared_decode import _engine_setup
    cfg, eng, u8, ids = _engine_setup(ops, torch.float16)
    ids = R.engine_prompt(cfg, ids, PROMPT_SEED)
    host = R.HostLoop(eng, cfg, ids, u8, torch.float16, DEV)
    return cfg, eng, u8, ids, host, R.pick_eos(host, 4, T_NEW)


def test_generate_beams_against_the_host_loop(micro):
    """Every (early_stopping, length_penalty) pair at K = 1, 2, 4, the decode modes alternating, num_return_sequences = K, two eos ids the
    unconstrained beams produce.  At most one case in eight may be cut short at a near tie of the host loop; about the host loop alone, the
    near-tie steps stay inside that cap."""
    cfg, eng, u8, ids, host, eos = micro
    cases = R.engine_cases()
    full, cuts, early = 0, 0, 0
    for K, decode, es, lp in cases:
        ok, cut, want = R.compare_with_host(eng, host, K, decode, es, lp, T_NEW, eos)
        full += ok
        cuts += cut is not None
        early += any(len(seq) < T_NEW for _, seq in want)
    print(f"[generate_beams emulator] {full} / {len(cases)} cases identical at full length; host-loop near-tie steps in {cuts} cases")
    assert cuts <= len(cases) // 8 and len(cases) - full <= len(cases) // 8
    assert early >= len(cases) // 2                                    # hypotheses do finish early
    eng.generate_beams(ids, u8, 4, max_new_tokens=2, eos_token_id=eos)
    st = eng._batch_states[("shared", 4)]
    assert st.kp is not None and all(t.shape[0] == 4 * st.capacity for t in st.k) and st.beams == 0


def test_one_beam_is_greedy(micro):
    cfg, eng, u8, ids, host, eos = micro
    for e in ((), eos):
        want = eng.generate(ids, u8, max_new_tokens=T_NEW, eos_token_id=e)
        for decode in ("shared", "copy"):
            got = eng.generate_beams(ids, u8, 1, max_new_tokens=T_NEW, eos_token_id=e, decode=decode)
            assert len(got.sequences) == 1 and torch.equal(got.sequences[0], want), (decode, got.sequences[0].tolist(), want.tolist())


def test_generate_beams_leaves_the_other_calls_alone(micro):
    """A pooled state that ran a beam search serves generate_batch afterwards (st.beams is reset), and the other way round."""
    cfg, eng, u8, ids, host, eos = micro
    a = eng.generate_batch([(ids, u8), (ids[:, :-3], u8)], max_new_tokens=4, eos_token_id=())
    got = eng.generate_beams(ids, u8, 2, max_new_tokens=4, eos_token_id=(), decode="copy")
    b = eng.generate_batch([(ids, u8), (ids[:, :-3], u8)], max_new_tokens=4, eos_token_id=())
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and len(got.sequences) == 1


def test_lo4_is_served_as_declared(micro, ops):
    """generate_beams declares precision "lo4" served: the pair (hl) step at B = K, against the host loop under the same precision."""
    from tests.test_emu_shared_decode import _engine_setup
    cfg, eng, u8, ids = _engine_setup(ops, torch.float16)
    assert eng.BEAMS_LO4 == "served"
    assert eng.lo4_supported()                                         # the micro configuration has the lo4 schedule
    eng.precision = "lo4"
    host = R.HostLoop(eng, cfg, ids, u8, torch.float16, DEV)
    R.compare_with_host(eng, host, 2, "shared", False, 1.0, 4, ())
    assert eng._batch_states[("shared", 2)].hl == eng.decode_hl(2)


def test_refusals(micro):
    cfg, eng, u8, ids, host, eos = micro
    launches = []
    was = eng.prefill
    eng.prefill = lambda *a, **k: launches.append(1) or was(*a, **k)
    try:
        for kw, exc, match in (
                (dict(num_beams=0), ValueError, "num_beams"), (dict(num_beams=9), ValueError, "num_beams"),
                (dict(num_beams=2, num_return_sequences=3), ValueError, "num_return_sequences"),
                (dict(num_beams=2, eos_token_id=(1, 2, 3, 4, 5)), ValueError, "eos ids"),
                (dict(num_beams=2, decode="paged"), ValueError, "decode"),
                (dict(num_beams=2, early_stopping="sometimes"), ValueError, "early_stopping")):
            with pytest.raises(exc, match=match):
                eng.generate_beams(ids, u8, **kw)
        V = cfg.text_config.vocab_size
        eng.suppress_tokens = torch.arange(V - 10, dtype=torch.int64)
        with pytest.raises(ValueError, match="vocabulary"):
            eng.generate_beams(ids, u8, 4, eos_token_id=(V - 1, V - 2))            # 10 ids left, (1 + 2) x 4 = 12 needed
        eng.suppress_tokens = None
        for attr, obj, val, match in (("tp_size", eng.W, 2, "tensor-parallel"), ("_fp8", eng, object(), "fp8"), ("split_operands", eng, True, "split")):
            had, old = hasattr(obj, attr), getattr(obj, attr, None)
            setattr(obj, attr, val)
            try:
                for decode in ("shared", "copy"):
                    with pytest.raises(NotImplementedError, match=match):
                        eng.generate_beams(ids, u8, 2, decode=decode)
            finally:
                setattr(obj, attr, old) if had else delattr(obj, attr)
        assert not launches
    finally:
        eng.suppress_tokens = None
        eng.prefill = was


def test_suppress_tokens_are_never_candidates(micro):
    cfg, eng, u8, ids, host, eos = micro
    free = eng.generate_beams(ids, u8, 2, max_new_tokens=4, eos_token_id=(), num_return_sequences=2)
    banned = sorted({int(t) for s in free.sequences for t in s[0, ids.numel():].tolist()})
    eng.suppress_tokens = torch.tensor(banned, dtype=torch.int64)
    try:
        R.compare_with_host(eng, host, 2, "shared", False, 1.0, 4, ())
        got = eng.generate_beams(ids, u8, 2, max_new_tokens=4, eos_token_id=(), num_return_sequences=2)
        assert not any(int(t) in banned for s in got.sequences for t in s[0, ids.numel():].tolist())
    finally:
        eng.suppress_tokens = None


# ---- the surfaces --------------------------------------------------------------------------------------------------------------------
def test_model_object_surface(micro, ops, tmp_path):
    """LeopardForConditionalGeneration.generate_beams: the engine's call with decode="shared", generation_config.json defaults, the return
    shapes, last_decoding; ``generate(num_beams=)`` still warns, names num_beams and points here."""
    import json
    import warnings
    from leopard_amd import compat, sampling
    from leopard_amd.weights import SynthSource
    cfg, eng, u8, ids, host, eos = micro
    m = compat.LeopardForConditionalGeneration(cfg, lambda dev, dt: SynthSource(cfg, ops, dev, dt), torch.float16, ops, torch_dtype=torch.float16)
    m = m.to("cpu").eval()
    want = eng.generate_beams(ids, u8, 2, max_new_tokens=4, eos_token_id=eos, length_penalty=2.0, num_return_sequences=2, decode="shared")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = m.generate_beams(ids, u8, num_beams=2, max_new_tokens=4, eos_token_id=list(eos), length_penalty=2.0, num_return_sequences=2)
    assert isinstance(got, list) and len(got) == 2 and all(torch.equal(a, b) for a, b in zip(got, want.sequences))
    assert m.last_decoding == "beam(2, length_penalty=2.0)" and list(m.engine._batch_states) == [("shared", 2)]
    one = m.generate_beams(ids, u8, num_beams=2, max_new_tokens=4, eos_token_id=list(eos), length_penalty=2.0)
    assert torch.is_tensor(one) and torch.equal(one, want.sequences[0])
    # generation_config.json: call arguments over the file over HF's defaults; the keys read before are unchanged
    (tmp_path / "generation_config.json").write_text(json.dumps({"num_beams": 2, "length_penalty": 2.0, "top_k": 40, "do_sample": False}))
    assert sampling.read_generation_config(str(tmp_path)) == {"do_sample": False, "top_k": 40}
    d = sampling.read_generation_config(str(tmp_path), beams=True)
    assert d == {"num_beams": 2, "length_penalty": 2.0}
    assert sampling.resolve_beams(d) == (2, 2.0, False) and sampling.resolve_beams(d, num_beams=4, early_stopping="never") == (4, 2.0, "never")
    assert sampling.resolve_beams(None) == (1, 1.0, False)
    m.beam_defaults = d
    assert torch.equal(m.generate_beams(ids, u8, max_new_tokens=4, eos_token_id=list(eos)), one) and m.last_decoding == "beam(2, length_penalty=2.0)"
    m.beam_defaults = {}
    greedy = m.generate(ids, u8, max_new_tokens=4, eos_token_id=list(eos))
    assert torch.equal(m.generate_beams(ids, u8, max_new_tokens=4, eos_token_id=list(eos)), greedy) and m.last_decoding == "beam(1, length_penalty=1.0)"
    with pytest.warns(UserWarning, match="diversity_penalty"):
        m.generate_beams(ids, u8, num_beams=2, max_new_tokens=2, eos_token_id=[], diversity_penalty=0.5)
    with pytest.warns(UserWarning, match="num_beams.*use generate_beams"):
        assert torch.equal(m.generate(ids, u8, max_new_tokens=4, eos_token_id=list(eos), num_beams=4), greedy)
    assert m.last_decoding == "greedy"
