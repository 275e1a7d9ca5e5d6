"""Wide pair decode (decode_pair_limit up to 32) on the emulator: lmi_gemm_skinny_wide_hl / lmi_rope_qkv_skinny_wide_hl bit for bit against
the 8-pair entries on pair groups, lmi_attn_decode_pool_hl at 9 .. 32 sequences, and the lo4 engine on a small synthetic model
(generate_batch / generate_stream under decode_pair_limit = 32 give every request the tokens and log-probs of the 8-pair step).
Cases: tests/wide_pair_ref.py."""
import pytest
import torch

from tests import wide_decode_ref as R
from tests import wide_pair_ref as P
from tests.emu_util import emu_ops

DEV = "cpu"


@pytest.fixture(scope="module")
def ops():
    return emu_ops()


# ---- kernels ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", P.DTYPES)
@pytest.mark.parametrize("layout", P.LAYOUTS, ids=[l[0] for l in P.LAYOUTS])
@pytest.mark.parametrize("M", P.PAIR_M)
def test_gemm_skinny_wide_hl_pairs_equal_their_8_pair_groups(ops, dtype, layout, M):
    for K in P.PAIR_K:
        P.check_gemm_pair(ops, DEV, dtype, layout, M, K, seed=10 * M + K)


def test_wide_pair_entries_refuse_33_pairs_and_a_row_bias(ops):
    P.check_pair_refusals(ops, DEV)


@pytest.mark.parametrize("dtype", P.DTYPES)
@pytest.mark.parametrize("layout", P.LAYOUTS, ids=[l[0] for l in P.LAYOUTS])
@pytest.mark.parametrize("M", P.PAIR_M)
@pytest.mark.parametrize("K", P.PAIR_K)
def test_rope_qkv_skinny_wide_hl_pairs_equal_their_8_pair_groups(ops, dtype, layout, M, K):
    for folded in (False, True):
        P.check_rope_qkv_pair(ops, DEV, dtype, layout, M, K, folded, seed=M + K)


@pytest.mark.parametrize("window", [0, 128])
@pytest.mark.parametrize("B", P.ATT_SEQS)
def test_attention_decode_pool_hl_at_9_to_32_sequences(ops, B, window):
    P.check_attention_pool_pair(ops, DEV, torch.float16, B, window)


# ---- the engine: the small synthetic model of tests/test_emu_wide_decode.py, lo4 ----------------------------------------------------------
@pytest.fixture(scope="module")
def lo4(ops):
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
    assert eng.decode_pair_limit == eng.PAIR_DECODE_BATCH == 8 and eng.decode_hl(8) and not eng.decode_hl(9)
    reqs = R.text_requests(32, 240, 3, DEV)
    ref = P.batch_in_groups_of_8(eng, reqs, logprobs=2)                 # shared by the generate_batch cases: do not write to it
    yield eng, reqs, ref
    P.reset(eng)


@pytest.mark.parametrize("n", [9, 17, 32])
def test_generate_batch_on_the_wide_pair_step(lo4, n):
    eng, reqs, ref = lo4
    P.check_generate_batch_pair(eng, reqs, ref, n, captured=False)


def test_generate_stream_16_slots_on_the_wide_pair_step(lo4):
    eng, reqs, ref = lo4
    eos = (R.early_eos(ref.sequences, reqs, P.T_NEW),)
    P.check_stream_pair(eng, reqs[:24], eos)


def test_rules_on_the_wide_pair_step(lo4):
    P.check_rules_pair(lo4[0], lo4[1][:18])


def test_default_pair_limit_keeps_17_on_the_fast_step(lo4):
    P.check_default_limit_keeps_the_fast_step(lo4[0], lo4[1])


def test_decode_pair_limit_values(lo4):
    P.check_limit_values(lo4[0])


def test_state_of_another_limit_is_rebuilt(lo4):
    P.check_state_rebuilt_after_limit_change(lo4[0], lo4[1])


def test_generate_shared_keeps_the_8_pair_step(lo4):
    """decode_pair_limit = 32 does not reach generate_shared: a chunk of 9 suffixes decodes on the fast step in both decode modes (the q|k|v
    entry of the shared mode takes a row_bias, which has no wide form), to the tokens it has under the default limit."""
    eng, reqs, _ = lo4
    prefix = reqs[0][0]
    sfx = [r[0][0, :4] for r in reqs[1:10]]
    outs = {}
    for limit in (8, 32):
        P.set_limits(eng, limit)
        for mode in ("copy", "shared"):
            if mode == "shared" and eng._llm_heads()[0] != 4 * eng._llm_heads()[1]:
                continue
            outs[limit, mode] = eng.generate_shared(prefix, None, sfx, max_new_tokens=4, eos_token_id=(), decode=mode)
            st = eng._batch_states[9 if mode == "copy" else ("shared", 9)]
            assert st.hl is False
    for (limit, mode), o in outs.items():
        R.assert_same_outputs(o, outs[8, mode])


def test_model_objects_pass_the_pair_limit_through():
    from leopard_amd import compat, idefics2_compat
    from leopard_amd.config import idefics2_tiny_config, tiny_config
    m = compat.LeopardForConditionalGeneration(tiny_config(), None)
    assert m.decode_pair_limit == 8
    m.decode_pair_limit = 24
    assert m.decode_pair_limit == 24 and m._decode_pair_limit == 24
    for bad in (7, 33):
        with pytest.raises(ValueError):
            m.decode_pair_limit = bad
    i = idefics2_compat.Idefics2ForConditionalGeneration(idefics2_tiny_config(), None)
    i.decode_pair_limit = 32
    assert i.decode_pair_limit == 32
    with pytest.raises(ValueError):
        i.decode_pair_limit = 64
