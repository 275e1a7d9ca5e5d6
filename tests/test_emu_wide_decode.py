"""Wide batched decode (decode_batch_limit up to 64) on the emulator: lmi_gemm_skinny_wide / lmi_rope_qkv_skinny_wide bit for bit against the
16-row entries on row groups, the choice / rules / logprobs / pooled-attention entries at 64 rows, and the engine on the micro configuration
(generate_stream and generate_batch at widths above 16 give every request the tokens it has at 16).  Cases: tests/wide_decode_ref.py."""
import pytest
import torch

from tests import wide_decode_ref as R
from tests.emu_util import emu_ops

DEV = "cpu"


@pytest.fixture(scope="module")
def ops():
    return emu_ops()


# ---- kernels ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("layout", R.LAYOUTS, ids=[l[0] for l in R.LAYOUTS])
@pytest.mark.parametrize("M", R.WIDE_M)
def test_gemm_skinny_wide_rows_equal_their_16_row_groups(ops, dtype, layout, M):
    for K in R.WIDE_K:
        R.check_gemm_wide(ops, DEV, dtype, layout, M, K, seed=10 * M + K)


def test_gemm_skinny_wide_limits(ops):
    R.check_gemm_wide_rejects(ops, DEV)


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("layout", R.LAYOUTS, ids=[l[0] for l in R.LAYOUTS])
@pytest.mark.parametrize("M", [17, 33, 64])
def test_rope_qkv_skinny_wide_rows_equal_their_16_row_groups(ops, dtype, layout, M):
    for folded in (False, True):
        R.check_rope_qkv_wide(ops, DEV, dtype, layout, M, folded, seed=M)


def test_choice_rules_logprobs_kernels_at_64_rows(ops):
    R.check_choice_kernels(ops, DEV)


@pytest.mark.parametrize("case", sorted(R.ATTN_LENS))
def test_attention_decode_pool_at_64_sequences(ops, case):
    R.check_attention_pool_wide(ops, DEV, torch.float16, R.ATTN_LENS[case])


# ---- the engine, micro configuration ----------------------------------------------------------------------------------------------------
T_NEW = 11                                                             # 10 decode steps: two HIST windows


@pytest.fixture(scope="module")
def micro(ops):
    from leopard_amd.engine import LeopardEngine
    from leopard_amd.weights import EngineWeights, SynthSource
    from tests.test_emu_engine import micro_config
    cfg = micro_config()
    W = EngineWeights.build(cfg, SynthSource(cfg, ops, DEV, torch.float16), torch.float16)
    eng = LeopardEngine(cfg, W, ops=ops, device=DEV)
    assert eng._batch_decode_supported() and eng.decode_batch_limit == eng.MAX_DECODE_BATCH == 16
    reqs = R.text_requests(66, 240, 1, DEV)                            # twice the widest emulated batch
    free = eng.generate_stream(reqs, batch_size=16, max_new_tokens=T_NEW, eos_token_id=())
    eos = (R.early_eos(free, reqs, T_NEW),)
    ref16 = eng.generate_stream(reqs, batch_size=16, max_new_tokens=T_NEW, eos_token_id=eos)
    assert any(o.shape[1] < r[0].shape[1] + T_NEW for o, r in zip(ref16, reqs)) and any(o.shape[1] == r[0].shape[1] + T_NEW for o, r in zip(ref16, reqs))
    return eng, cfg, reqs, eos, ref16


def test_decode_batch_limit_property(micro):
    eng = micro[0]
    eng.decode_batch_limit = 16
    for bad in (0, 65, -1, 2.5, "8", None, True):
        with pytest.raises(ValueError):
            eng.decode_batch_limit = bad
    assert eng.decode_batch_limit == 16
    for ok in (1, 32, 64):
        eng.decode_batch_limit = ok
        assert eng.decode_batch_limit == ok
    eng.decode_batch_limit = 16


def test_default_limit_clamps_to_16(micro):
    eng, cfg, reqs, eos, ref16 = micro
    eng.decode_batch_limit = 16
    stats = {}
    out = eng.generate_stream(reqs[:24], batch_size=20, max_new_tokens=T_NEW, eos_token_id=eos, stats=stats)
    assert stats["batch_size"] == 16
    R.assert_same_outputs(out, ref16[:24])


@pytest.mark.parametrize("B", [17, 33])
def test_generate_stream_wide_equals_width_16(micro, B):
    eng, cfg, reqs, eos, ref16 = micro
    eng.decode_batch_limit = 64
    n = 2 * B
    ref = ref16 if n == len(reqs) else eng.generate_stream(reqs[:n], batch_size=16, max_new_tokens=T_NEW, eos_token_id=eos)
    stats = {}
    out = eng.generate_stream(reqs[:n], batch_size=B, max_new_tokens=T_NEW, eos_token_id=eos, stats=stats)
    assert stats["batch_size"] == B and eng._batch_states[B].B == B and not eng._batch_states[B].hl
    R.assert_same_outputs(out, ref)


def test_one_step_bit_for_bit(micro):
    R.check_one_step_bitwise(micro[0], DEV)


def test_wide_sampled_logprobs_rules(micro):
    from leopard_amd.engine import LogitsRules
    from leopard_amd.sampling import SamplingParams
    eng, cfg, reqs, eos, _ = micro
    eng.decode_batch_limit = 64
    sub = reqs[:34]
    sp = SamplingParams(temperature=0.9, top_k=20, top_p=0.9, seed=5)
    # (5 new tokens: the two-slot run is 17 windows of HIST steps whatever the length, twice that with 11)
    R.assert_same_outputs(eng.generate_stream(sub, batch_size=33, max_new_tokens=5, eos_token_id=eos, sampling=sp),
                          eng.generate_stream(sub, batch_size=2, max_new_tokens=5, eos_token_id=eos, sampling=sp))
    a = eng.generate_stream(sub, batch_size=33, max_new_tokens=T_NEW, eos_token_id=eos, logprobs=2)
    b = eng.generate_stream(sub, batch_size=16, max_new_tokens=T_NEW, eos_token_id=eos, logprobs=2)
    R.assert_same_outputs(a.sequences, b.sequences)
    for ring in ("token_logprobs", "top_ids", "top_logprobs"):
        for x, y in zip(getattr(a, ring), getattr(b, ring)):
            assert torch.equal(x, y), ring
    rules = LogitsRules(1.3, 3, 4)
    R.assert_same_outputs(eng.generate_stream(sub, batch_size=33, max_new_tokens=T_NEW, eos_token_id=eos, rules=rules),
                          eng.generate_stream(sub, batch_size=16, max_new_tokens=T_NEW, eos_token_id=eos, rules=rules))


def test_generate_batch_20_samples_in_one_pool(micro):
    eng, cfg, reqs, eos, _ = micro
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


def test_lo4_engine_decodes_17_on_the_fast_step(ops):
    from leopard_amd.config import LeopardConfig, RopeScaling, TextConfig, VisionConfig
    from leopard_amd.engine import LeopardEngine
    from leopard_amd.weights import EngineWeights, SynthSource
    cfg = LeopardConfig(
        vision_config=VisionConfig(hidden_size=1152, intermediate_size=100, num_hidden_layers=1, num_attention_heads=16, image_size=28, patch_size=14),
        text_config=TextConfig(hidden_size=256, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1,
                               vocab_size=256, rope_scaling=RopeScaling()),
        image_token_index=250)
    W = EngineWeights.build(cfg, SynthSource(cfg, ops, DEV, torch.float16), torch.float16)
    eng = LeopardEngine(cfg, W, ops=ops, device=DEV)
    eng.precision = "lo4"
    assert eng.decode_hl(8) and not eng.decode_hl(17)
    eng.decode_batch_limit = 64
    reqs = R.text_requests(20, 240, 2, DEV)
    stats = {}
    wide = eng.generate_stream(reqs, batch_size=17, max_new_tokens=6, eos_token_id=(), stats=stats)
    assert stats["batch_size"] == 17 and eng._batch_states[17].hl is False
    R.assert_same_outputs(wide, eng.generate_stream(reqs, batch_size=16, max_new_tokens=6, eos_token_id=()))


def test_shape_without_batched_decode_falls_back(micro, monkeypatch):
    """An engine whose shape has no batched decode answers per request at any limit: no pooled state, the tokens of generate()."""
    eng, cfg, reqs, eos, _ = micro
    eng.decode_batch_limit = 64
    eng.release_batch_state()
    monkeypatch.setattr(eng, "_batch_decode_supported", lambda: False)
    sub = reqs[:18]
    outs = eng.generate_stream(sub, batch_size=18, max_new_tokens=3, eos_token_id=())
    assert not eng._batch_states
    for (ids, _), o in zip(sub, outs):
        assert torch.equal(o, eng.generate(ids, None, max_new_tokens=3, eos_token_id=()))
    assert len(eng.generate_batch(sub, max_new_tokens=2, eos_token_id=())) == 18 and not eng._batch_states
    eng.decode_batch_limit = 16


def test_model_objects_pass_the_limit_through():
    from leopard_amd import compat, idefics2_compat
    from leopard_amd.config import idefics2_tiny_config, tiny_config
    m = compat.LeopardForConditionalGeneration(tiny_config(), None)
    assert m.decode_batch_limit == 16
    m.decode_batch_limit = 48
    assert m.decode_batch_limit == 48 and m._decode_batch_limit == 48
    with pytest.raises(ValueError):
        m.decode_batch_limit = 65
    i = idefics2_compat.Idefics2ForConditionalGeneration(idefics2_tiny_config(), None)
    i.decode_batch_limit = 32
    assert i.decode_batch_limit == 32
    with pytest.raises(ValueError):
        i.decode_batch_limit = 0
