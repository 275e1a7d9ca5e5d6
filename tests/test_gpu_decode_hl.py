"""-m gpu: the hi + lo pair ("hl") decode kernels on the device at batch sizes above 1 — lmi_gemm_skinny_hl, lmi_rope_qkv_skinny_hl,
lmi_split_rows_hl, lmi_attn_decode_fwd_hl / lmi_attn_decode_pool_hl and the captured batched step of precision = "lo4" that runs on them.
A wrong lane offset in this code gives logits a few 1e-4 off, which the end-to-end 1e-3 assertions absorb: here the projections run on
inputs whose fp32 sums are exact in any order (tests/decode_hl_ref.py), so the device must return the fp64 reference bit for bit."""
import numpy as np
import pytest
import torch

from tests import decode_hl_ref as R

pytestmark = pytest.mark.gpu
DTYPES = R.DTYPES
DEV = "cuda:0"
# K = 128: one k-step, seven idle waves; 1152: 9 steps, uneven across the 8 waves; 4096: 4 steps per wave (a tail for DEPTH 3, even for
# DEPTH 2); 14336: 14 steps per wave (a tail of 2)
KS = [128, 1152, 4096, 14336]


@pytest.fixture(scope="module")
def ops():
    from leopard_amd.ops import Ops
    assert torch.cuda.is_available()
    return Ops()


# ---- 1. gemm_skinny(hl=True), exact ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("M", [1, 3, 8])
def test_gemm_skinny_hl_exact_store_f32_residual_store(ops, dtype, K, M):
    R.check_gemm_hl_exact(ops, DEV, dtype, M, K)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("M", [1, 3, 8])
def test_gemm_skinny_hl_swiglu_on_exact_sums(ops, dtype, K, M):
    R.check_swiglu_hl(ops, DEV, dtype, M, K)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M", [1, 3, 8])
def test_gemm_skinny_hl_swiglu_column_mapping(ops, dtype, M):
    R.check_swiglu_hl_column_mapping(ops, DEV, dtype, M)


def test_split_rows_hl_on_the_device(ops):
    """lmi_split_rows_hl: [T(x); T(x - T(x))] bit for bit, source and destination rows strided, the guard row intact."""
    for dtype in DTYPES:
        for M, K in ((1, 128), (3, 1152), (8, 4096)):
            x32 = torch.randn(M, K, generator=torch.Generator().manual_seed(K + M)) * 2.0
            out = R.guarded(2 * M, K + 8, dtype, DEV)
            ops.split_rows_hl(R.strided_rows(x32, DEV), out[:2 * M, :K])
            out = out.cpu()
            assert torch.equal(out[:2 * M, :K], R.pair(x32, dtype)) and R.intact(out, 2 * M) and bool((out[:, K:] == R.GUARD).all())


# ---- 2. folded norm on pairs -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [128, 1152, 4096])
@pytest.mark.parametrize("M", [1, 3, 8])
def test_gemm_skinny_hl_folded_norm_producer(ops, dtype, K, M):
    R.check_producer_hl(ops, DEV, dtype, M, K)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", [64, 256])
@pytest.mark.parametrize("M", [1, 3, 8])
def test_gemm_skinny_hl_folded_norm_consumer(ops, dtype, P, M):
    R.check_consumer_hl(ops, DEV, dtype, M, P)


# ---- 3. rope_qkv_skinny(hl=True) ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("folded", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,KV", [(4, 1), (8, 2)])
@pytest.mark.parametrize("M", [1, 3, 8])
def test_rope_qkv_skinny_hl(ops, dtype, H, KV, M, folded):
    for K in (128, 1152):
        R.check_rope_qkv_hl(ops, DEV, dtype, M, K, H, KV, folded)


# ---- 4. Gaussian pairs: what the mode buys -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [4096, 14336])
@pytest.mark.parametrize("M", [1, 8])
def test_gemm_skinny_hl_gaussian_pairs_against_the_one_row_kernel(ops, dtype, K, M):
    """Against the fp64 product of the unrounded operand the pair launch is < 0.02 x the one-row launch's error; the printed line also gives
    its fp32 accumulation error beside a plain torch fp32 matmul's on the same hi + lo operand."""
    e = R.gaussian_pair_errors(ops, DEV, dtype, M, K)
    print(f"[hl gaussian] {str(dtype)[6:]} M={M} K={K}: pair / one-row error {e.pair:.3e} / {e.one:.3e} = {e.pair / e.one:.4f}; "
          f"accumulation error kernel / torch fp32 {e.acc:.3e} / {e.torch32:.3e} = {e.acc / max(e.torch32, 1e-30):.2f}")
    assert e.pair < 0.02 * e.one, (e.pair, e.one)


# ---- 5. decode attention writing pairs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,KV", [(32, 8), (4, 4)])                    # GQA-packed blocks; one block per head
def test_attention_decode_pool_hl_ragged_every_split_size(ops, dtype, H, KV):
    for st in (0, 1, 2, 4, 8):
        R.check_attention_pool_hl(ops, DEV, dtype, H, KV, st)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,KV", [(32, 8), (4, 4)])
def test_attention_decode_pool_hl_sliding_window(ops, dtype, H, KV):
    for st in (0, 1, 2, 4, 8):
        R.check_attention_pool_hl(ops, DEV, dtype, H, KV, st, window=128, lens=(700, 1023))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,KV", [(32, 8), (4, 4)])
def test_attention_decode_hl_one_sequence_every_split_size(ops, dtype, H, KV):
    for st in (0, 1, 2, 4, 8):
        R.check_attention_one_hl(ops, DEV, dtype, H, KV, st)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,KV", [(32, 8), (4, 4)])
def test_attention_decode_hl_one_sequence_sliding_window(ops, dtype, H, KV):
    for st in (0, 1, 2, 4, 8):
        R.check_attention_one_hl(ops, DEV, dtype, H, KV, st, window=128, lens=(700, 1023))


# ---- 6. the captured batched step on pairs -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lo4_engine(ops):
    from leopard_amd.config import mid_config
    from leopard_amd.engine import LeopardEngine
    from leopard_amd.weights import EngineWeights, SynthSource
    cfg = mid_config()
    W = EngineWeights.build(cfg, SynthSource(cfg, ops, torch.device(DEV), torch.float16), torch.float16)
    eng = LeopardEngine(cfg, W, ops=ops, device=torch.device(DEV))
    eng.precision = "lo4"
    yield cfg, eng, {}                                                  # {}: sample index -> this engine's generate() tokens
    eng.release_batch_state()


def small_samples(cfg, B):
    """One 336 x 336 image sample, then text-only prompts of different lengths."""
    from PIL import Image
    from leopard_amd.synth import synth_image_u8, synth_prompt_ids
    from leopard_amd.tiler import tile_sample, to_u8_tiles
    vit_inputs, plan = tile_sample([Image.fromarray(synth_image_u8(7, 336, 336))])
    ids = torch.from_numpy(synth_prompt_ids(plan.vit_inputs_per_image, cfg, seed=7)).reshape(1, -1)
    samples = [(ids, torch.from_numpy(to_u8_tiles(vit_inputs)).to(DEV))]
    for i in range(1, B):
        samples.append((torch.from_numpy(np.random.default_rng(300 + i).integers(3, 7000, (1, 5 + 3 * i))), None))
    return samples


@pytest.mark.parametrize("B", [3, 8, 9])
def test_generate_batch_lo4_runs_the_captured_step_on_pairs(lo4_engine, B):
    """precision = "lo4": the batched step of B <= 8 sequences runs on operand pairs (DecodeState.hl) as ONE captured graph; tokens equal the
    per-sample generate() (whose step is the batch-1 lo4 one), a difference only on a near tie of the batch-1 lo4 logits; a second call is
    bit-identical.  B = 9 (2 B > 16 rows): the step silently falls back to the fast one — hl is False."""
    from leopard_amd.engine import KVCache
    cfg, eng, singles_of = lo4_engine
    assert eng.precision == "lo4" and eng.decode_hl(B) == (B <= 8)
    samples = small_samples(cfg, B)
    T = 5
    for i, (ids, tiles) in enumerate(samples):                          # sample i is the same for every B: its batch-1 run is made once
        if i not in singles_of:
            singles_of[i] = eng.generate(ids, tiles, max_new_tokens=T, eos_token_id=())
    singles = [singles_of[i] for i in range(B)]
    steps = []
    body = eng._batch_decode_body
    eng._batch_decode_body = lambda st: (steps.append((st.B, st.hl)), body(st))[1]
    try:
        batch = eng.generate_batch(samples, max_new_tokens=T, eos_token_id=())
    finally:
        eng._batch_decode_body = body
    st = eng._batch_states[B]
    assert st.hl == (B <= 8)
    assert steps == [(B, B <= 8)] * 2 and st.graphs.get((False, False)) is not None          # warm-up + capture: afterwards the graph replays (no Python body)
    for (ids, tiles), one, got in zip(samples, singles, batch):
        S_in = ids.shape[1]
        assert got.shape == one.shape and int(got[0, S_in]) == int(one[0, S_in])
        if st.hl and not torch.equal(one, got):                         # (B = 9 decodes on the fast step: another schedule than generate()'s)
            j = int((one[0] != got[0]).nonzero()[0])
            cache = KVCache(cfg, one.shape[1] + 256 * 8, torch.float16, DEV)
            eng.prefill(ids, tiles, cache=cache)
            lg, nxt = None, int(one[0, S_in])
            for t in range(S_in + 1, j + 1):
                lg = eng.decode_step(nxt, cache).clone()
                nxt = int(one[0, t])
            assert cache._decode_state.hl
            top2 = lg.topk(2).values
            assert float(top2[0] - top2[1]) <= 2e-3 * float(lg.abs().max()), (j, top2)
    again = eng.generate_batch(samples, max_new_tokens=T, eos_token_id=())
    assert all(torch.equal(a, b) for a, b in zip(batch, again)) and eng._batch_states[B] is st
