"""Shared-prefix batched decode on the CPU emulator build: lmi_attn_decode_shared / _hl (one prefix K / V copy, walked once per step for the
whole batch) against plain fp32 attention over the materialised [prefix ; own] keys, the independence of a sequence from its batch mates
bit for bit, the KV append at a biased row, the argument checks, and LeopardEngine.generate_shared(decode="shared").  The emulator's LDS-DMA
asynchrony model (tests/test_hipemu_dma_model.py) is on for every launch here — an under-counted wait shows as NaNs."""
import os

import numpy as np
import pytest
import torch

from tests import shared_decode_ref as R
from tests.decode_hl_ref import pair_gain, pair_rows_checks
from tests.emu_util import emu_ops

DTYPES = [torch.float16, torch.bfloat16]
D = R.D
OWN = [1, 2, 64, 65, 129]                                      # own lengths, mixed over the batch
CAP_O = 136                                                    # slot rows: three 64-key tiles


@pytest.fixture(scope="module")
def ops():
    assert "HIPEMU_SYNC_DMA" not in os.environ, "the LDS-DMA asynchrony model must be on (unset HIPEMU_SYNC_DMA)"
    return emu_ops()


def own_lens(B, P):
    return [OWN[(s + P) % len(OWN)] for s in range(B)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [1, 3, 16])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 130])
def test_shared_decode_vs_fp32(ops, P, B, dtype):
    """Item 1: within 3 eps of fp32 over the materialised keys.  Prefix rows >= P and slot rows >= k_len are NaN: a row that is read without
    being masked — or a tile consumed before its pieces landed — is a NaN in the output.  B = 3 runs 8 query / 2 KV heads, the others 4 / 1."""
    H, KV = (8, 2) if B == 3 else (4, 1)
    c = R.make_case(P, P + 7, own_lens(B, P), CAP_O, H, KV, dtype, 1000 + 17 * P + B)
    out = R.run(ops, c)
    assert bool((out[B] == R.GUARD).all())
    got = out[:B].float()
    assert not torch.isnan(got).any()
    err = (got - R.reference(c)).abs().max().item()
    print(f"P={P} B={B} H={H} lens={c.lens} {dtype}: max abs err {err:.3e} (bound {3 * R.eps(dtype):.3e})")
    assert err <= 3 * R.eps(dtype)
    assert torch.equal(out, R.run(ops, c))                     # run to run


def growing_case(dtype, B=16, P=57 * 64 - 20):
    """The independence case.  57 prefix tiles are more than the prefix pass has splits (56), so a workgroup walks TWO tiles and the deferred
    rescale can fire at the second.  The K rows of odd tiles are doubled and every other q row is scaled by 8: a scaled row's maximum
    outgrows the threshold (2^8) at the second tile of a split, an unscaled row's does not — a wave-uniform update of the reference would
    rescale the unscaled rows with their batch mates and give them another rounding than they get alone."""
    c = R.make_case(P, P + 7, own_lens(B, P), CAP_O, 4, 1, dtype, 77, q_scale=[8.0 if s % 2 == 0 else 1.0 for s in range(B)])
    grow = (1 + (torch.arange(P) // 64) % 2).to(torch.float32)[:, None]
    c.kp[:P] = (c.kp[:P].float() * grow).to(dtype)
    return c


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_sequence_does_not_depend_on_its_batch_mates(ops, dtype):
    """Item 2: sequence j alone (B = 1) == sequence j among 16, bit for bit, for every j; two launches of the batch agree bit for bit."""
    c = growing_case(dtype)
    batch = R.run(ops, c)
    assert torch.equal(batch, R.run(ops, c))
    assert not torch.isnan(batch.float()).any()
    assert (batch[:c.B].float() - R.reference(c)).abs().max() <= 3 * R.eps(dtype)
    for j in range(c.B):
        alone = R.run(ops, c, rows=[j])
        assert torch.equal(alone[0], batch[j]), j


@pytest.mark.parametrize("dtype", DTYPES)
def test_shared_decode_hl_pairs(ops, dtype):
    """Item 3: out rows [0, B) == the plain launch, rows [B, 2 B) the 16-bit residuals of their rounding (the pair lmi_attn_decode_pool_hl
    writes: tests/decode_hl_ref.py's checks), and hi + lo is closer to the fp64 result than hi alone."""
    B, P = 8, 130
    c = R.make_case(P, P + 7, own_lens(B, P), CAP_O, 8, 2, dtype, 31)
    one, two = R.run(ops, c), R.run(ops, c, hl=True)
    assert torch.equal(two, R.run(ops, c, hl=True))
    pair_rows_checks(two, one[:B], B, dtype, "decode_shared_hl")
    assert two[B:2 * B].double().abs().max() > 0
    e_two, e_one = pair_gain(two, B, R.reference(c, ftype=torch.float64))
    print(f"{dtype}: hi + lo error {e_two:.3e}, hi alone {e_one:.3e}")
    assert e_two < 0.8 * e_one


def rope_tables(cap, hd):
    f = torch.arange(cap).float().reshape(-1, 1) * (1.0 / (10000.0 ** (torch.arange(0, hd, 2).float() / hd))).reshape(1, -1)
    return f.cos().contiguous(), f.sin().contiguous()


def rnd(shape, dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


@pytest.mark.parametrize("hl", [False, True])
@pytest.mark.parametrize("packed", [False, True])
def test_rope_qkv_skinny_appends_at_the_biased_row(ops, packed, hl):
    """Item 4: with row_bias = P the K / V rows go to m * stride + pos[m] - P, the rotation is that of pos[m] (q | k | v rows and the appended
    rows equal the unbiased call's bit for bit), no other row is written; row_bias = None is today's call."""
    from leopard_amd.weights import rope_permute_rows, skinny_pack
    dtype, H, KV, hd, B, K, P, own = torch.float16, 2, 1, 128, 3, 384, 9, 4
    cap = P + own
    w = rnd(((H + 2 * KV) * hd, K), dtype, 7, 0.1)
    x32 = rnd((B, K), torch.float32, 8)
    x = torch.cat([x32.to(dtype), (x32 - x32.to(dtype).float()).to(dtype)]) if hl else x32.to(dtype)
    cos, sin = rope_tables(cap, hd)
    pos = torch.tensor([P + 2, P, P + 3], dtype=torch.int32)
    w_rope = torch.cat([rope_permute_rows(w[:(H + KV) * hd]), w[(H + KV) * hd:]]).contiguous()
    w_arg = skinny_pack(w_rope) if packed else w_rope
    k0, v0 = torch.zeros(B * cap, KV * hd, dtype=dtype), torch.zeros(B * cap, KV * hd, dtype=dtype)
    want = torch.zeros(B, (H + 2 * KV) * hd, dtype=dtype)
    ops.rope_qkv_skinny(w_arg, x, want, H, KV, hd, cos, sin, k0, v0, cap, pos, packed=packed, hl=hl)
    k1, v1 = torch.zeros(B * own, KV * hd, dtype=dtype), torch.zeros(B * own, KV * hd, dtype=dtype)
    got = torch.zeros_like(want)
    ops.rope_qkv_skinny(w_arg, x, got, H, KV, hd, cos, sin, k1, v1, own, pos, packed=packed, hl=hl, row_bias=torch.tensor([P], dtype=torch.int32))
    assert torch.equal(got, want)
    touched = torch.zeros(B * own, dtype=torch.bool)
    for m in range(B):
        r = m * own + int(pos[m]) - P
        touched[r] = True
        assert torch.equal(k1[r], k0[m * cap + int(pos[m])]) and torch.equal(v1[r], v0[m * cap + int(pos[m])]) and k1[r].any()
    assert not k1[~touched].any() and not v1[~touched].any()
    k2, v2 = torch.zeros_like(k0), torch.zeros_like(v0)
    again = torch.zeros_like(want)
    ops.rope_qkv_skinny(w_arg, x, again, H, KV, hd, cos, sin, k2, v2, cap, pos, packed=packed, hl=hl, row_bias=None)
    assert torch.equal(again, want) and torch.equal(k2, k0) and torch.equal(v2, v0)


def test_rope_qk_rows_appends_at_the_biased_row(ops):
    """Item 4 for lmi_rope_qk_rows (head dims other than 128 ride here): the same statement."""
    dtype, H, KV, hd, B, P, own = torch.float16, 2, 1, 64, 3, 9, 4
    cap = P + own
    qkv = rnd((B, (H + 2 * KV) * hd), dtype, 1)
    cos, sin = rope_tables(cap, hd)
    pos = torch.tensor([P + 2, P, P + 3], dtype=torch.int32)
    k0, v0 = torch.zeros(B * cap, KV * hd, dtype=dtype), torch.zeros(B * cap, KV * hd, dtype=dtype)
    want = qkv.clone()
    ops.rope_qk_rows(want, H, KV, hd, cos, sin, k0, v0, cap, pos)
    k1, v1 = torch.zeros(B * own, KV * hd, dtype=dtype), torch.zeros(B * own, KV * hd, dtype=dtype)
    got = qkv.clone()
    ops.rope_qk_rows(got, H, KV, hd, cos, sin, k1, v1, own, pos, row_bias=torch.tensor([P], dtype=torch.int32))
    assert torch.equal(got, want)
    touched = torch.zeros(B * own, dtype=torch.bool)
    for m in range(B):
        r = m * own + int(pos[m]) - P
        touched[r] = True
        assert torch.equal(k1[r], k0[m * cap + int(pos[m])]) and torch.equal(v1[r], v0[m * cap + int(pos[m])]) and k1[r].any()
    assert not k1[~touched].any() and not v1[~touched].any()
    k2, v2 = torch.zeros_like(k0), torch.zeros_like(v0)
    again = qkv.clone()
    ops.rope_qk_rows(again, H, KV, hd, cos, sin, k2, v2, cap, pos, row_bias=None)
    assert torch.equal(again, want) and torch.equal(k2, k0) and torch.equal(v2, v0)


def test_shared_decode_rejects_bad_arguments_before_any_launch(ops):
    """Item 5: the limits are LMI_EINVAL (a RuntimeError from Ops), never a trap, and nothing is written."""
    dtype, H, KV, B, P = torch.float16, 4, 1, 2, 8
    c = R.make_case(P, P + 7, [3, 5], 16, H, KV, dtype, 600)
    plen = torch.tensor([P], dtype=torch.int32)
    k_begin, k_len = torch.tensor([0, 16], dtype=torch.int32), torch.tensor([3, 5], dtype=torch.int32)
    ws = torch.zeros(1 << 16)
    out = torch.full((B, H * D), R.GUARD, dtype=dtype)

    def call(q=c.q, kp=c.kp, heads=H, kv=KV, hd=D, cap_p=c.cap_p, n_seq=None, k_len_=k_len, k_begin_=k_begin):
        ops.attention_decode_shared(q, kp, c.vp, plen, cap_p, c.k, c.v, out, k_begin_, k_len_, 16, heads, kv, hd, hd ** -0.5, ws, n_seq=n_seq)

    call()                                                         # the arguments the cases below break one at a time are good
    assert not (out == R.GUARD).any()
    out.fill_(R.GUARD)
    with pytest.raises(RuntimeError, match="4 \\* n_kv_heads"):
        call(heads=2, kv=1)                                        # heads ratio 2
    with pytest.raises(RuntimeError, match="head_dim"):
        call(heads=8, kv=2, hd=64)
    with pytest.raises(RuntimeError, match="n_seq"):
        call(n_seq=33)
    with pytest.raises(RuntimeError, match="max_prefix_len"):
        call(cap_p=0)
    with pytest.raises(RuntimeError, match="strides"):
        wide = torch.zeros(c.cap_p, KV * D + 4, dtype=dtype)
        call(kp=wide[:, :KV * D])                                  # a row stride that is no multiple of 8
    with pytest.raises(RuntimeError, match="4 GiB"):
        call(cap_p=(1 << 31) // c.kp.stride(0) + 1)                # that many rows of this stride span >= 4 GiB
    with pytest.raises(RuntimeError):
        ops.decode_shared_workspace_elems(B, H, D, 0, 16)
    assert bool((out == R.GUARD).all())


# ---- engine: generate_shared(decode="shared") on a micro configuration with 4 query heads on 1 KV head -----------------------------------------
def _engine_setup(ops, dtype, hidden=512, heads=4):
    from leopard_amd.config import LeopardConfig, RopeScaling, TextConfig, VisionConfig
    from leopard_amd.engine import LeopardEngine
    from leopard_amd.synth import synth_prompt_ids
    from leopard_amd.weights import EngineWeights, SynthSource
    cfg = LeopardConfig(
        vision_config=VisionConfig(hidden_size=1152, intermediate_size=100, num_hidden_layers=1, num_attention_heads=16, image_size=28, patch_size=14),
        text_config=TextConfig(hidden_size=hidden, intermediate_size=128, num_hidden_layers=2, num_attention_heads=heads, num_key_value_heads=1,
                               vocab_size=256, rope_scaling=RopeScaling()),
        image_token_index=250)
    W = EngineWeights.build(cfg, SynthSource(cfg, ops, "cpu", dtype), dtype)
    eng = LeopardEngine(cfg, W, ops=ops, device="cpu")
    u8 = torch.from_numpy(np.random.default_rng(31).integers(0, 256, (2, 28, 28, 3), dtype=np.uint8))
    ids = torch.from_numpy(synth_prompt_ids([2], cfg, n_question=32)).reshape(1, -1)        # the last 48 ids: question + tail
    return cfg, eng, u8, ids


@pytest.fixture(scope="module")
def micro(ops):
    return _engine_setup(ops, torch.float16)


def test_generate_shared_decode_shared_equals_generate(micro):
    """Item 6: three suffixes, four new tokens — the tokens generate() gives for [prefix ; suffix] (strict equality, as the copy path's test in
    tests/test_emu_prefix.py); the caller's prefix cache is not written; the pool holds B x own_capacity rows and ONE prefix copy; a second
    call with a shorter prefix reuses the state."""
    from leopard_amd.engine import KVCache
    cfg, eng, u8, ids = micro
    assert eng._batch_decode_supported() and eng.cfg.text_config.head_dim == 128
    eng.release_batch_state()
    head = ids[:, :-48]
    sfx = [ids[:, -48:], ids[:, -48:-20], torch.tensor([[9, 8, 7, 6, 5]])]
    singles = [eng.generate(torch.cat([head, s], dim=1), u8, max_new_tokens=4, eos_token_id=()) for s in sfx]
    P = eng.merged_len(head)
    prefix = KVCache(cfg, P, torch.float16, "cpu")
    eng.prefill(head, u8, cache=prefix)
    k0, v0 = [t.clone() for t in prefix.k], [t.clone() for t in prefix.v]
    got = eng.generate_shared(head, u8, sfx, max_new_tokens=4, eos_token_id=(), prefix=prefix, decode="shared")
    for one, out in zip(singles, got):
        assert out.shape == one.shape and torch.equal(one, out), (one.tolist(), out.tolist())
    assert all(torch.equal(a, b) for a, b in zip(prefix.k, k0)) and all(torch.equal(a, b) for a, b in zip(prefix.v, v0)) and prefix.length == P
    assert list(eng._batch_states) == [("shared", 3)]
    st = eng._batch_states[("shared", 3)]
    assert st.capacity >= 48 + 4 and st.prefix_capacity >= P and int(st.prefix_len[0]) == P
    assert all(t.shape[0] == 3 * st.capacity for t in st.k + st.v) and all(t.shape[0] == st.prefix_capacity for t in st.kp + st.vp)
    # another, shorter prefix (three text ids cut off the head) through the same state: the prefix length is a device int
    assert not bool((head[0, :3] == cfg.image_token_index).any())
    head2 = head[:, 3:]
    P2 = eng.merged_len(head2)
    singles2 = [eng.generate(torch.cat([head2, s], dim=1), u8, max_new_tokens=4, eos_token_id=()) for s in sfx]
    got2 = eng.generate_shared(head2, u8, sfx, max_new_tokens=4, eos_token_id=(), decode="shared")
    assert eng._batch_states[("shared", 3)] is st and int(st.prefix_len[0]) == P2 and P2 == P - 3
    for one, out in zip(singles2, got2):
        assert torch.equal(one, out), (one.tolist(), out.tolist())
    alone = eng.generate_shared(head, u8, sfx[1:2], max_new_tokens=4, eos_token_id=(), decode="shared")      # one suffix: the batch-1 path
    assert torch.equal(alone[0], singles[1]) and list(eng._batch_states) == [("shared", 3)]
    eng.release_batch_state()
    assert not eng._batch_states


def test_generate_shared_decode_shared_sampled_request_does_not_depend_on_n(micro):
    from leopard_amd.engine import SamplingParams
    cfg, eng, u8, ids = micro
    head = ids[:, :-48]
    sfx = [ids[:, -48:], ids[:, -48:-20], torch.tensor([[9, 8, 7, 6, 5]])]
    sp = SamplingParams(temperature=0.9, top_k=20, top_p=0.95, seed=7)
    s3 = eng.generate_shared(head, u8, sfx, max_new_tokens=3, eos_token_id=(), sampling=sp, decode="shared")
    s2 = eng.generate_shared(head, u8, sfx[:2], max_new_tokens=3, eos_token_id=(), sampling=sp, decode="shared")
    s1 = eng.generate_shared(head, u8, sfx[:1], max_new_tokens=3, eos_token_id=(), sampling=sp, decode="shared")
    assert torch.equal(s3[0], s1[0]) and torch.equal(s3[0], s2[0]) and torch.equal(s3[1], s2[1])
    eng.release_batch_state()


def test_generate_shared_decode_argument_errors(ops, micro):
    """decode="bogus" is a ValueError; a shape the shared decode cannot serve (1 query head per KV head) a NotImplementedError that names the
    reason — both before any launch, and never another path taken silently."""
    cfg, eng, u8, ids = micro
    head, sfx = ids[:, :-48], [ids[:, -48:], torch.tensor([[9, 8, 7]])]
    launches = []
    check = ops._check
    ops._check = lambda rc: (launches.append(1), check(rc))[1]
    try:
        with pytest.raises(ValueError, match="decode"):
            eng.generate_shared(head, u8, sfx, max_new_tokens=2, decode="bogus")
        _, eng1, _, _ = _engine_setup(ops, torch.float16, hidden=128, heads=1)
        launches.clear()
        with pytest.raises(NotImplementedError, match="ratio must be 4"):
            eng1.generate_shared(head, u8, sfx, max_new_tokens=2, decode="shared")
        assert not launches
    finally:
        ops._check = check
