"""Wide batched decode (decode_batch_limit up to 64) on the device: the cases of tests/wide_decode_ref.py on the gfx950 kernels — the wide
projection entries bit for bit against the 16-row ones, the choice / rules / logprobs / pooled-attention entries at 64 rows — and the engine
on the mid model (full-width layers, 2 + 2, 8k vocabulary): a request decodes to the same tokens at widths 17, 33 and 64 as at 16."""
import pytest
import torch

from tests import wide_decode_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from leopard_amd.ops import Ops
    return Ops()


# ---- kernels ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("layout", R.LAYOUTS, ids=[l[0] for l in R.LAYOUTS])
def test_gemm_skinny_wide_rows_equal_their_16_row_groups(ops, dtype, layout):
    for M in R.WIDE_M:
        for K in R.WIDE_K:
            R.check_gemm_wide(ops, DEV, dtype, layout, M, K, seed=10 * M + K)


def test_gemm_skinny_wide_limits(ops):
    R.check_gemm_wide_rejects(ops, DEV)


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("M", [17, 64])
def test_gemm_skinny_wide_llama_decode_shapes(ops, dtype, M):
    R.check_gemm_wide_llama_shapes(ops, DEV, dtype, M)


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("layout", R.LAYOUTS, ids=[l[0] for l in R.LAYOUTS])
def test_rope_qkv_skinny_wide_rows_equal_their_16_row_groups(ops, dtype, layout):
    for M in (17, 33, 64):
        for folded in (False, True):
            R.check_rope_qkv_wide(ops, DEV, dtype, layout, M, folded, seed=M)


def test_choice_rules_logprobs_kernels_at_64_rows(ops):
    R.check_choice_kernels(ops, DEV)


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("case", sorted(R.ATTN_LENS))
def test_attention_decode_pool_at_64_sequences(ops, dtype, case):
    R.check_attention_pool_wide(ops, DEV, dtype, R.ATTN_LENS[case])


# ---- the engine, mid model --------------------------------------------------------------------------------------------------------------
T_NEW = 11                                                             # 10 decode steps: two HIST windows


@pytest.fixture(scope="module")
def mid(ops):
    from leopard_amd.config import mid_config
    from leopard_amd.engine import LeopardEngine
    from leopard_amd.weights import EngineWeights, SynthSource
    cfg = mid_config()
    W = EngineWeights.build(cfg, SynthSource(cfg, ops, torch.device(DEV), torch.float16), torch.float16)
    eng = LeopardEngine(cfg, W, ops=ops, device=torch.device(DEV))
    assert eng._batch_decode_supported() and eng.decode_batch_limit == eng.MAX_DECODE_BATCH == 16
    reqs = R.text_requests(128, 7900, 1, DEV, base_len=9)               # twice the widest batch
    free = eng.generate_stream(reqs, batch_size=16, max_new_tokens=T_NEW, eos_token_id=())
    eos = (R.early_eos(free, reqs, T_NEW),)
    ref16 = eng.generate_stream(reqs, batch_size=16, max_new_tokens=T_NEW, eos_token_id=eos)
    assert any(o.shape[1] < r[0].shape[1] + T_NEW for o, r in zip(ref16, reqs))
    yield eng, cfg, reqs, eos, ref16
    eng.release_batch_state()


def test_default_limit_clamps_to_16(mid):
    eng, cfg, reqs, eos, ref16 = mid
    eng.decode_batch_limit = 16
    stats = {}
    out = eng.generate_stream(reqs[:40], batch_size=20, max_new_tokens=T_NEW, eos_token_id=eos, stats=stats)
    assert stats["batch_size"] == 16
    R.assert_same_outputs(out, ref16[:40])
    for bad in (0, 65):
        with pytest.raises(ValueError):
            eng.decode_batch_limit = bad


@pytest.mark.parametrize("B", [17, 33, 64])
def test_generate_stream_wide_equals_width_16(mid, B):
    eng, cfg, reqs, eos, ref16 = mid
    eng.decode_batch_limit = 64
    n = 2 * B
    # (a request's tokens do not depend on which other requests run: the first n outputs of the 128-request run are the run over n requests)
    stats = {}
    out = eng.generate_stream(reqs[:n], batch_size=B, max_new_tokens=T_NEW, eos_token_id=eos, stats=stats)
    st = eng._batch_states[B]
    assert stats["batch_size"] == B and st.B == B and not st.hl
    assert st.graphs.get((False, False)) is not None                   # the wide step was captured and replayed
    R.assert_same_outputs(out, ref16[:n])


def test_one_step_bit_for_bit(mid):
    R.check_one_step_bitwise(mid[0], DEV, vocab_hi=7900)


def test_wide_sampled_logprobs_rules(mid):
    from leopard_amd.engine import LogitsRules
    from leopard_amd.sampling import SamplingParams
    eng, cfg, reqs, eos, _ = mid
    eng.decode_batch_limit = 64
    sub = reqs[:40]
    sp = SamplingParams(temperature=0.9, top_k=20, top_p=0.9, seed=5)
    R.assert_same_outputs(eng.generate_stream(sub, batch_size=33, max_new_tokens=T_NEW, eos_token_id=eos, sampling=sp),
                          eng.generate_stream(sub, batch_size=2, max_new_tokens=T_NEW, eos_token_id=eos, sampling=sp))
    a = eng.generate_stream(sub, batch_size=33, max_new_tokens=T_NEW, eos_token_id=eos, logprobs=2)
    b = eng.generate_stream(sub, batch_size=16, max_new_tokens=T_NEW, eos_token_id=eos, logprobs=2)
    R.assert_same_outputs(a.sequences, b.sequences)
    for ring in ("token_logprobs", "top_ids", "top_logprobs"):
        for x, y in zip(getattr(a, ring), getattr(b, ring)):
            assert torch.equal(x, y), ring
    rules = LogitsRules(1.3, 3, 4)
    R.assert_same_outputs(eng.generate_stream(sub, batch_size=33, max_new_tokens=T_NEW, eos_token_id=eos, rules=rules),
                          eng.generate_stream(sub, batch_size=16, max_new_tokens=T_NEW, eos_token_id=eos, rules=rules))


def test_generate_batch_20_samples_in_one_pool(mid):
    eng, cfg, reqs, eos, _ = mid
    sub = reqs[:20]
    eng.decode_batch_limit = 16
    eng.release_batch_state()
    chunked = eng.generate_batch(sub, max_new_tokens=T_NEW, eos_token_id=eos)
    assert sorted(eng._batch_states) == [4, 16]
    eng.decode_batch_limit = 32
    eng.release_batch_state()
    pooled = eng.generate_batch(sub, max_new_tokens=T_NEW, eos_token_id=eos)
    assert list(eng._batch_states) == [20] and eng._batch_states[20].B == 20
    R.assert_same_outputs(pooled, chunked)
    eng.decode_batch_limit = 16
    eng.release_batch_state()


def test_lo4_engine_decodes_17_on_the_fast_step(mid):
    eng, cfg, reqs, eos, _ = mid
    eng.release_batch_state()
    eng.precision = "lo4"
    try:
        assert eng.decode_hl(8) and not eng.decode_hl(17)
        eng.decode_batch_limit = 64
        sub, stats = reqs[:20], {}
        wide = eng.generate_stream(sub, batch_size=17, max_new_tokens=6, eos_token_id=(), stats=stats)
        assert stats["batch_size"] == 17 and eng._batch_states[17].hl is False
        R.assert_same_outputs(wide, eng.generate_stream(sub, batch_size=16, max_new_tokens=6, eos_token_id=()))
    finally:
        eng.precision = "fast"
        eng.decode_batch_limit = 16
        eng.release_batch_state()


def test_shape_without_batched_decode_falls_back(mid, monkeypatch):
    eng, cfg, reqs, eos, _ = mid
    eng.decode_batch_limit = 64
    eng.release_batch_state()
    monkeypatch.setattr(eng, "_batch_decode_supported", lambda: False)
    sub = reqs[:18]
    outs = eng.generate_stream(sub, batch_size=18, max_new_tokens=3, eos_token_id=())
    assert not eng._batch_states
    for (ids, _), o in zip(sub, outs):
        assert torch.equal(o, eng.generate(ids, None, max_new_tokens=3, eos_token_id=()))
    eng.decode_batch_limit = 16
