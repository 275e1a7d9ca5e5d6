"""-m gpu: beam search on the MI355X — lmi_beam_step and lmi_beam_reorder on the cases of tests/beam_ref.py (the production vocabulary
included), and ``generate_beams`` on the 2 + 2-layer mid model against a host loop that keeps one batch-1 cache per beam: every
early_stopping / length_penalty pair, both decode modes, K = 1, 2, 4, K = 1 against greedy ``generate``, lo4 as declared, and two prompts
through ONE captured step."""
import numpy as np
import pytest
import torch

from tests import beam_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEP_CASES = R.step_cases()
T_NEW = 6
PROMPT_SEED = 0                         # tests/beam_ref.engine_prompt; if a run exceeds the near-tie cap, another seed — never another cap


@pytest.fixture(scope="module")
def ops():
    from leopard_amd.ops import Ops
    return Ops()


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", STEP_CASES, ids=[c["name"] for c in STEP_CASES])
def test_beam_step(ops, case):
    R.check_beam_step(ops, DEV, case)


def test_beam_step_production_vocabulary(ops):
    R.check_beam_step(ops, DEV, R.big_case())


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("width", [128, 1024])
def test_beam_reorder(ops, dtype, width):
    gen = np.random.default_rng(width)
    for K in (2, 4, 8):
        for name, parent in R.permutations_of(K).items():
            for held, row0 in R.REORDER_ROWS:
                R.check_beam_reorder(ops, DEV, dtype, width, K, held, row0, parent, gen)


def test_beam_step_and_reorder_replay_from_a_graph(ops):
    """Both entries captured in one HIP graph and replayed with other device values (scores, eos ids, rows held): what the eager launches give."""
    from leopard_amd.engine import _capture_safe
    case = STEP_CASES[2]                                               # V1003-K4-eos2
    K, V = case["K"], case["V"]
    x = case["logits"].to(DEV)
    eos = torch.tensor(sorted(case["eos"]) + [-1, -1], dtype=torch.int64, device=DEV)
    width, cap = 128, 300
    kv = [torch.from_numpy(np.random.default_rng(i).integers(-32768, 32768, (K * cap, width), dtype=np.int16)).view(torch.float16).to(DEV)
          for i in range(2)]
    ptrs = torch.tensor([t.data_ptr() for t in kv], dtype=torch.int64, device=DEV)
    row0 = torch.zeros(1, dtype=torch.int32, device=DEV)

    def buffers(scores, held):
        return dict(score=torch.tensor(scores + [0.0] * (8 - K), device=DEV), tok=torch.zeros(8, dtype=torch.int64, device=DEV),
                    parent=torch.zeros(8, dtype=torch.int32, device=DEV), walk=torch.zeros(R.WALK_WORDS, dtype=torch.int32, device=DEV),
                    row_lse=torch.zeros(K, device=DEV), row_id=torch.zeros(K, 8, dtype=torch.int32, device=DEV),
                    row_lp=torch.zeros(K, 8, device=DEV), row_eos_lp=torch.zeros(K, 4, device=DEV),
                    rows_held=torch.tensor([held], dtype=torch.int32, device=DEV))

    def body(o):
        ops.beam_step(x, V, K, eos, o["score"], o["tok"], o["parent"], o["walk"], o["row_lse"], o["row_id"], o["row_lp"], o["row_eos_lp"],
                      rows_held=o["rows_held"])
        ops.beam_reorder(ptrs, o["parent"], K, row0, o["rows_held"], width * 2, cap, 256)

    o = buffers(case["scores"], 4)
    start = [t.clone() for t in kv]
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        body(o)
    torch.cuda.current_stream(DEV).wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with _capture_safe(), torch.cuda.graph(g):
        body(o)
    for scores, held, eos_ids in ((case["scores"], 4, sorted(case["eos"])), ([-3.0, 0.0, -1.0, -0.5], 200, [case["eos"][0], 7])):
        eos.copy_(torch.tensor(eos_ids + [-1, -1], dtype=torch.int64))
        fresh = buffers(scores, held)
        for k, v in fresh.items():
            o[k].copy_(v)
        for t, s in zip(kv, start):
            t.copy_(s)
        g.replay()
        torch.cuda.synchronize()
        got_kv = [t.clone() for t in kv]
        for t, s in zip(kv, start):
            t.copy_(s)
        body(fresh)
        torch.cuda.synchronize()
        assert all(torch.equal(o[k], fresh[k]) for k in ("tok", "parent", "walk", "rows_held")) and R.same_bits(o["score"].cpu(), fresh["score"].cpu())
        assert all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(got_kv, kv))
        assert int(o["rows_held"][0]) == held + 1 and int(o["walk"][0]) >= K


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
    host = R.HostLoop(m.engine, cfg, ids, tiles, torch.float16, DEV)
    return m, cfg, m.engine, tiles, ids, host, R.pick_eos(host, 4, T_NEW)


def test_generate_beams_against_the_host_loop(mid):
    """tests/beam_ref.engine_cases with num_return_sequences = K and two eos ids the unconstrained beams produce: the host loop's hypotheses
    and, within the two paths' rounding, its scores.  A case whose host loop has a near-tie step may end at that step; at most one in eight."""
    m, cfg, eng, tiles, ids, host, eos = mid
    cases = R.engine_cases()
    full, cuts, early = 0, 0, 0
    for K, decode, es, lp in cases:
        ok, cut, want = R.compare_with_host(eng, host, K, decode, es, lp, T_NEW, eos)
        full += ok
        cuts += cut is not None
        early += any(len(seq) < T_NEW for _, seq in want)
    print(f"[generate_beams mid] {full} / {len(cases)} cases identical at full length; host-loop near-tie steps in {cuts} cases; "
          f"{early} cases with a hypothesis shorter than {T_NEW}")
    assert len(cases) - full <= len(cases) // 8
    assert early >= 1


def test_one_beam_is_greedy(mid):
    from tests.test_gpu_shared_decode import assert_equal_or_near_tie
    m, cfg, eng, tiles, ids, host, eos = mid
    for e in ((), eos):
        want = eng.generate(ids, tiles, max_new_tokens=T_NEW, eos_token_id=e)
        for decode in ("shared", "copy"):
            got = eng.generate_beams(ids, tiles, 1, max_new_tokens=T_NEW, eos_token_id=e, decode=decode)
            if got.sequences[0].shape == want.shape:
                assert_equal_or_near_tie(eng, cfg, ids, tiles, want, got.sequences[0])
            else:                                                      # one of the two stopped at an eos the other missed: only on a near tie
                n = min(got.sequences[0].shape[1], want.shape[1])
                assert not assert_equal_or_near_tie(eng, cfg, ids, tiles, want[:, :n], got.sequences[0][:, :n])


def test_two_prompts_replay_one_captured_step(mid):
    """Another prompt (another length, another eos list) replays the step the first call captured, and gives what it gives alone."""
    m, cfg, eng, tiles, ids, host, eos = mid
    other = R.engine_prompt(cfg, ids, PROMPT_SEED + 17)[:, :-2]
    for decode, key in (("shared", ("shared", 4)), ("copy", 4)):
        eng.release_batch_state()
        alone = eng.generate_beams(other, tiles, 4, max_new_tokens=T_NEW, eos_token_id=eos[:1], num_return_sequences=4, decode=decode)
        eng.release_batch_state()
        eng.generate_beams(ids, tiles, 4, max_new_tokens=T_NEW, eos_token_id=eos, num_return_sequences=4, decode=decode)
        st = eng._batch_states[key]
        n = len(st.graphs)
        assert n == 1 and st.beams == 0
        again = eng.generate_beams(other, tiles, 4, max_new_tokens=T_NEW, eos_token_id=eos[:1], num_return_sequences=4, decode=decode)
        assert eng._batch_states[key] is st and len(st.graphs) == n
        assert len(again.sequences) == len(alone.sequences) and all(torch.equal(a, b) for a, b in zip(again.sequences, alone.sequences))
        assert again.scores == alone.scores
    eng.release_batch_state()


def test_lo4_is_served_as_declared(mid):
    m, cfg, eng, tiles, ids, host, eos = mid
    assert eng.BEAMS_LO4 == "served"
    was = eng.precision
    eng.precision = "lo4"
    try:
        eng.release_batch_state()
        R.compare_with_host(eng, host, 2, "shared", False, 1.0, 4, eos)
        assert eng._batch_states[("shared", 2)].hl
    finally:
        eng.precision = was
        eng.release_batch_state()


def test_idefics2_surface_runs_copy_mode_inside_the_sliding_window(ops):
    """Idefics2 (sliding window, a suppress_tokens list): generate_beams decodes with decode="copy" — "shared" is refused for a windowed
    decoder — against the host loop; one beam is greedy ``generate``; a suppressed id is never generated."""
    from leopard_amd import idefics2_compat as IC
    from leopard_amd.config import idefics2_mid_config
    from leopard_amd.idefics2 import Idefics2SynthSource
    cfg = idefics2_mid_config()
    m = IC.Idefics2ForConditionalGeneration(cfg, lambda dev, dt: Idefics2SynthSource(cfg, ops, dev, dt), torch.float16, ops, eos_token_id=(2,)).to(DEV)
    eng = m.engine
    assert eng.suppress_tokens is not None and cfg.text_config.sliding_window
    ids = torch.from_numpy(np.random.default_rng(2).integers(3, 7000, (1, 12))).to(DEV)
    with pytest.raises(NotImplementedError, match="sliding_window"):
        eng.generate_beams(ids, None, 2, max_new_tokens=4, decode="shared")
    host = R.HostLoop(eng, cfg, ids, None, torch.float16, DEV)
    R.compare_with_host(eng, host, 4, "copy", False, 1.0, T_NEW, (2,))
    got = m.generate_beams(ids, num_beams=4, max_new_tokens=T_NEW, num_return_sequences=4)
    assert isinstance(got, list) and len(got) == 4 and m.last_decoding == "beam(4, length_penalty=1.0)"
    assert list(eng._batch_states) == [4] and eng._batch_states[4].kp is None
    assert not any(set(s[0, 12:].tolist()) & set(m.bad_words_ids) for s in got)
    # one beam: the host loop's batch-1 steps are greedy generate's, and generate_beams follows the host loop (or ends at its near tie)
    greedy = m.generate(ids, max_new_tokens=T_NEW)
    assert host.run(1, T_NEW, (2,))[0][1] == greedy[0, 12:].tolist()
    R.compare_with_host(eng, host, 1, "copy", False, 1.0, T_NEW, (2,))
    eng.release_batch_state()
