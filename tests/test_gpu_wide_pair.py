"""Wide pair decode (decode_pair_limit up to 32) on the device: the cases of tests/wide_pair_ref.py on the gfx950 kernels — the wide pair
projection entries bit for bit against the 8-pair ones, lmi_attn_decode_pool_hl at 9 .. 32 sequences — and the lo4 engine on the mid model
(full-width layers, 2 + 2, 8k vocabulary): a request decodes to the same tokens and log-probs on a pair step of 9, 17 and 32 as on one of 8."""
import pytest
import torch

from tests import wide_decode_ref as R
from tests import wide_pair_ref as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from leopard_amd.ops import Ops
    return Ops()


# ---- kernels ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", P.DTYPES)
@pytest.mark.parametrize("layout", P.LAYOUTS, ids=[l[0] for l in P.LAYOUTS])
def test_gemm_skinny_wide_hl_pairs_equal_their_8_pair_groups(ops, dtype, layout):
    for M in P.PAIR_M:
        for K in P.PAIR_K:
            P.check_gemm_pair(ops, DEV, dtype, layout, M, K, seed=10 * M + K)


def test_wide_pair_entries_refuse_33_pairs_and_a_row_bias(ops):
    P.check_pair_refusals(ops, DEV)


@pytest.mark.parametrize("dtype", P.DTYPES)
@pytest.mark.parametrize("layout", P.LAYOUTS, ids=[l[0] for l in P.LAYOUTS])
def test_rope_qkv_skinny_wide_hl_pairs_equal_their_8_pair_groups(ops, dtype, layout):
    for M in P.PAIR_M:
        for K in P.PAIR_K:
            for folded in (False, True):
                P.check_rope_qkv_pair(ops, DEV, dtype, layout, M, K, folded, seed=M + K)


@pytest.mark.parametrize("dtype", P.DTYPES)
@pytest.mark.parametrize("window", [0, 128])
@pytest.mark.parametrize("B", P.ATT_SEQS)
def test_attention_decode_pool_hl_at_9_to_32_sequences(ops, dtype, B, window):
    P.check_attention_pool_pair(ops, DEV, dtype, B, window)


# ---- the engine, mid model, lo4 ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lo4(ops):
    from leopard_amd.config import mid_config
    from leopard_amd.engine import LeopardEngine
    from leopard_amd.weights import EngineWeights, SynthSource
    cfg = mid_config()
    W = EngineWeights.build(cfg, SynthSource(cfg, ops, torch.device(DEV), torch.float16), torch.float16)
    eng = LeopardEngine(cfg, W, ops=ops, device=torch.device(DEV))
    eng.precision = "lo4"
    assert eng.decode_pair_limit == eng.PAIR_DECODE_BATCH == 8 and eng.decode_hl(8) and not eng.decode_hl(9)
    reqs = R.text_requests(32, 7900, 3, DEV, base_len=9)
    ref = P.batch_in_groups_of_8(eng, reqs, logprobs=2)                 # shared by the generate_batch cases: do not write to it
    yield eng, reqs, ref
    P.reset(eng)


@pytest.mark.parametrize("n", [9, 17, 32])
def test_generate_batch_on_the_wide_pair_step(lo4, n):
    eng, reqs, ref = lo4
    P.check_generate_batch_pair(eng, reqs, ref, n, captured=True)


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
