"""Continuing from a cached prefix, on the CPU emulator build: the two-range key walk of attn_fwd_dma_kernel (lmi_attn_prefix_fwd /
lmi_attn_prefix_fwd_lo4_rows) against plain fp32 attention over the materialised [prefix ; own] keys and, where the prefix is a whole number of
64-key tiles, bit for bit against the existing kernel on a contiguous copy; then LeopardEngine.extend / append / generate_shared on the micro
configuration of tests/test_emu_engine.py against the fp32 oracle.  The emulator's LDS-DMA asynchrony model (tests/test_hipemu_dma_model.py:
a piece poisons its destination when issued and lands at the counted wait) is on for every launch here — an under-counted wait shows as NaNs."""
import os

import numpy as np
import pytest
import torch

from leopard_amd.ops import Lo4Act, lo4_head_k4
from tests.emu_util import emu_ops

DTYPES = [torch.float16, torch.bfloat16]
D = 128
OWN_SETS = [[1, 31, 130], [77]]                                # one launch of three sequences, one of a single sequence


@pytest.fixture(scope="module")
def ops():
    assert "HIPEMU_SYNC_DMA" not in os.environ, "the LDS-DMA asynchrony model must be on (unset HIPEMU_SYNC_DMA)"
    return emu_ops()


def rnd(shape, dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def eps(dtype):
    return 2.0 ** -10 if dtype == torch.float16 else 2.0 ** -7          # one rounding of the 16-bit type (tests/test_gpu_kernels.py)


def prefix_ref(q, k, v, kp, vp, cu, H, KV):
    """fp32 attention of every packed sequence over [prefix ; own] keys with the bottom-right causal mask."""
    P = kp.shape[0]
    out = torch.zeros(q.shape[0], H * D)
    for s in range(len(cu) - 1):
        a, b = cu[s], cu[s + 1]
        qs = q[a:b].float().view(-1, H, D).transpose(0, 1)
        ks = torch.cat([kp, k[a:b]]).float().view(-1, KV, D).transpose(0, 1).repeat_interleave(H // KV, 0)
        vs = torch.cat([vp, v[a:b]]).float().view(-1, KV, D).transpose(0, 1).repeat_interleave(H // KV, 0)
        sc = qs @ ks.transpose(-1, -2) * D ** -0.5
        m = torch.arange(P + b - a)[None, :] <= torch.arange(b - a)[:, None] + P
        o = torch.softmax(sc.masked_fill(~m, float("-inf")), -1) @ vs
        out[a:b] = o.transpose(0, 1).reshape(-1, H * D)
    return out


def make_case(P, lens, H, KV, dtype, seed):
    """A packed qkv buffer (the own rows) and a prefix K / V with ANOTHER row stride (a cache layer: [cap, KV * D] views of wider rows)."""
    T = sum(lens)
    cu = [0] + list(np.cumsum(lens))
    qkv = rnd((T, (H + 2 * KV) * D), dtype, seed)
    q, k, v = qkv[:, :H * D], qkv[:, H * D:(H + KV) * D], qkv[:, (H + KV) * D:]
    cache = rnd((P + 3, 2 * KV * D + 8), dtype, seed + 1)       # 3 spare rows past P: must never be seen
    kp, vp = cache[:P, :KV * D], cache[:P, KV * D:2 * KV * D]
    return q, k, v, kp, vp, [int(c) for c in cu]


def run_prefix(ops, lo4, q, k, v, kp, vp, cu, H, KV, dtype, row_sel=None):
    T = q.shape[0]
    cu_t = torch.tensor(cu, dtype=torch.int32)
    mx = max(b - a for a, b in zip(cu, cu[1:]))
    if not lo4:
        out = torch.full((T, H * D), float("nan"), dtype=dtype)
        ops.attention_prefix(q, k, v, kp, vp, kp.shape[0], out, cu_t, mx, H, KV, D, D ** -0.5)
        return out, None
    act = Lo4Act.empty(T, H * D, dtype, "cpu", k4=lo4_head_k4(H, D))
    act.hi.fill_(float("nan"))
    if row_sel is not None:
        act.row_sel = row_sel
    ops.attention_prefix_lo4(q, k, v, kp, vp, kp.shape[0], act, cu_t, mx, H, KV, D, D ** -0.5)
    return act.hi, act


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lo4", [False, True])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 200])
def test_prefix_attention_vs_fp32(ops, P, lo4, dtype):
    """Items 1 and 3: both entry points, f16 and bf16, within 3 eps of fp32 over the materialised keys — with the DMA model on, so a tile consumed
    before its pieces landed (or a prefix row >= P that was not masked) would be a NaN / a miss."""
    for i, lens in enumerate(OWN_SETS):
        H, KV = (4, 1) if i == 0 else (8, 2)
        q, k, v, kp, vp, cu = make_case(P, lens, H, KV, dtype, 100 + P)
        out, _ = run_prefix(ops, lo4, q, k, v, kp, vp, cu, H, KV, dtype)
        ref = prefix_ref(q, k, v, kp, vp, cu, H, KV)
        assert not torch.isnan(out.float()).any()
        err = (out.float() - ref).abs().max().item()
        print(f"P={P} lens={lens} lo4={lo4} {dtype}: max abs err {err:.3e} (bound {3 * eps(dtype):.3e})")
        assert err <= 3 * eps(dtype), (P, lens, err)


@pytest.mark.parametrize("lo4", [False, True])
@pytest.mark.parametrize("P", [64, 128])
def test_prefix_attention_bits_at_aligned_prefix(ops, P, lo4):
    """Item 2: a prefix of whole 64-key tiles gives the key-order tile partition of a contiguous [prefix ; own] launch — the same arithmetic,
    the same bits: 16-bit rows and, for lo4, the residual image and its scales."""
    dtype, H, KV = torch.float16, 4, 1
    for lens in OWN_SETS:
        q, k, v, kp, vp, cu = make_case(P, lens, H, KV, dtype, 300 + P)
        out, act = run_prefix(ops, lo4, q, k, v, kp, vp, cu, H, KV, dtype)
        for a, b in zip(cu, cu[1:]):
            s = b - a
            kc, vc = torch.cat([kp, k[a:b]]).contiguous(), torch.cat([vp, v[a:b]]).contiguous()
            cq, ck = torch.tensor([0, s], dtype=torch.int32), torch.tensor([0, P + s], dtype=torch.int32)
            qs = q[a:b].contiguous()
            if not lo4:
                one = torch.empty(s, H * D, dtype=dtype)
                ops.attention(qs, kc, vc, one, cq, ck, s, H, KV, D, D ** -0.5, True)
                assert torch.equal(out[a:b], one), (P, lens, a)
            else:
                ref = Lo4Act.empty(s, H * D, dtype, "cpu", k4=lo4_head_k4(H, D))
                ops.attention_lo4(qs, kc, vc, ref, cq, ck, s, H, KV, D, D ** -0.5, True)
                assert torch.equal(act.hi[a:b], ref.hi) and torch.equal(act.img[a:b], ref.img) and torch.equal(act.sc[a:b], ref.sc), (P, lens, a)


def test_prefix_attention_row_selection_and_untouched_prefix(ops):
    """row_sel as lmi_attn_varlen_fwd_lo4_rows: unselected rows get their 16-bit row only; the prefix buffers are read, never written."""
    dtype, H, KV, P, lens = torch.float16, 4, 1, 65, [40, 9]
    q, k, v, kp, vp, cu = make_case(P, lens, H, KV, dtype, 500)
    kp0, vp0 = kp.clone(), vp.clone()
    full, act_full = run_prefix(ops, True, q, k, v, kp, vp, cu, H, KV, dtype)
    sel = torch.zeros(sum(lens), dtype=torch.uint8)
    sel[30:40] = 1
    sel[-2:] = 1
    act = Lo4Act.empty(sum(lens), H * D, dtype, "cpu", k4=lo4_head_k4(H, D))
    act.img.fill_(0x5A)
    act.sc.fill_(0x5A)
    act.row_sel = sel
    ops.attention_prefix_lo4(q, k, v, kp, vp, P, act, torch.tensor(cu, dtype=torch.int32), max(lens), H, KV, D, D ** -0.5)
    assert torch.equal(act.hi, full)
    on = sel.bool()
    assert torch.equal(act.img[on], act_full.img[on]) and torch.equal(act.sc[on], act_full.sc[on])
    assert bool((act.img[~on] == 0x5A).all()) and bool((act.sc[~on] == 0x5A).all())
    assert torch.equal(kp, kp0) and torch.equal(vp, vp0)


def test_prefix_attention_rejects_bad_arguments(ops):
    """The limits are LMI_EINVAL (a RuntimeError from Ops), never a trap: head_dim, empty prefix, the 4 GiB extent rule."""
    dtype, H, KV = torch.float16, 4, 1
    q, k, v, kp, vp, cu = make_case(8, [5], H, KV, dtype, 600)
    cu_t = torch.tensor(cu, dtype=torch.int32)
    out = torch.empty(5, H * D, dtype=dtype)
    with pytest.raises(RuntimeError):
        ops.attention_prefix(q, k, v, kp, vp, 0, out, cu_t, 5, H, KV, D, D ** -0.5)
    with pytest.raises(RuntimeError):
        ops.attention_prefix(q, k, v, kp, vp, 8, out, cu_t, 5, H, KV, 72, 72 ** -0.5)
    with pytest.raises(RuntimeError):                          # (P + longest own range) rows of this stride span >= 4 GiB
        ops.attention_prefix(q, k, v, kp, vp, (1 << 31) // kp.stride(0), out, cu_t, 5, H, KV, D, D ** -0.5)
    with pytest.raises(RuntimeError):
        ops.attention_prefix(q, k, v, kp, vp, 8, out, cu_t, 5, H, 3, D, D ** -0.5)


# ---- engine: extend / append / generate_shared on the micro configuration of tests/test_emu_engine.py ------------------------------------------
def _engine_setup(ops, dtype, hidden=128, heads=1):
    from leopard_amd.config import LeopardConfig, RopeScaling, TextConfig, VisionConfig
    from leopard_amd.engine import LeopardEngine
    from leopard_amd.synth import synth_prompt_ids, synth_state_dict_numpy
    from leopard_amd.tiler import siglip_normalize
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
    pix = torch.from_numpy(siglip_normalize(u8.numpy()))
    return cfg, eng, u8, pix, ids, synth_state_dict_numpy(cfg)


def _prefilled(eng, cfg, ids, u8, dtype, spare=0):
    from leopard_amd.engine import KVCache
    cache = KVCache(cfg, eng.merged_len(ids) + spare, dtype, "cpu")
    eng.prefill(ids, u8, cache=cache)
    return cache


@pytest.mark.parametrize("dtype,tol", [(torch.float16, 2e-3), (torch.bfloat16, 1.6e-2)])
def test_extend_last_row_logits_match_the_oracle_of_the_whole_prompt(ops, dtype, tol):
    """Item 4: prefix = everything before the question, suffix = the last 48 ids; the last-row logits against the fp32 oracle's last position
    of the WHOLE prompt, at test_engine_prefill_matches_oracle's tolerance; the prefix cache is not touched."""
    from oracle import leopard_oracle as O
    cfg, eng, u8, pix, ids, Wn = _engine_setup(ops, dtype)
    head, tail = ids[:, :-48], ids[:, -48:]
    ref = O.prefill_logits(ids, pix, O.weights_from_numpy(Wn), cfg)[0, -1]
    prefix = _prefilled(eng, cfg, head, u8, dtype)
    k0, v0 = [t.clone() for t in prefix.k], [t.clone() for t in prefix.v]
    res = eng.extend(prefix, [tail])
    scratch = eng.prefill(ids, u8).logits_last
    print(f"{dtype}: extend vs oracle {(res.logits[0] - ref).abs().max():.3e}, from-scratch prefill vs oracle {(scratch - ref).abs().max():.3e} "
          f"(bound {2 * tol:.1e})")
    assert res.logits.shape == (1, cfg.text_config.vocab_size) and res.seq_lens == [48] and res.prefix_len == prefix.length
    assert (res.logits[0] - ref).abs().max() <= tol * 2
    assert int(res.logits[0].argmax()) == int(ref.argmax())
    assert all(torch.equal(a, b) for a, b in zip(prefix.k, k0)) and all(torch.equal(a, b) for a, b in zip(prefix.v, v0))
    assert prefix.length == eng.merged_len(head)


@pytest.mark.parametrize("precision", ["fast", "lo4"])
def test_extend_on_the_fused_schedule_fan_out_kv_out_and_reuse(ops, precision):
    """Hidden 256 (the fused layer; lo4 needs it): oracle distance of the last row; three suffixes through one extend == each alone, bit for
    bit; kv_out holds the suffix K / V at packed offsets (== what a from-scratch prefill appends, up to the 16-bit noise); prefix unchanged
    and extendable again."""
    from leopard_amd.engine import KVCache
    from oracle import leopard_oracle as O
    dtype = torch.float16
    cfg, eng, u8, pix, ids, Wn = _engine_setup(ops, dtype, hidden=256, heads=2)
    eng.precision = precision
    head, tail = ids[:, :-48], ids[:, -48:]
    ref = O.prefill_logits(ids, pix, O.weights_from_numpy(Wn), cfg)[0, -1]
    prefix = _prefilled(eng, cfg, head, u8, dtype)
    P = prefix.length
    k0, v0 = [t.clone() for t in prefix.k], [t.clone() for t in prefix.v]
    sfx = [tail, tail[:, :5], torch.tensor([[9, 8, 7, 6, 5, 4, 3, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20]])]
    kv = KVCache(cfg, 48 + 5 + 17, dtype, "cpu")
    res = eng.extend(prefix, sfx, kv_out=kv)
    err = (res.logits[0] - ref).abs().max().item()
    print(f"{precision}: extend vs oracle {err:.3e} (bound 4e-3)")
    assert err <= 2e-3 * 2 and int(res.logits[0].argmax()) == int(ref.argmax())
    assert res.kv_out is kv and kv.length == 70 and res.seq_lens == [48, 5, 17]
    for j, s in enumerate(sfx):
        one = eng.extend(prefix, [s])
        assert torch.equal(one.logits[0], res.logits[j]), j
    whole = KVCache(cfg, P + 48, dtype, "cpu")
    eng.prefill(ids, u8, cache=whole)
    for i in range(len(kv.k)):                                     # 8 eps of the layer's K / V scale: one layer of 16-bit hand-over roundings apart
        for got, want in ((kv.k[i][:48].float(), whole.k[i][P:P + 48].float()), (kv.v[i][:48].float(), whole.v[i][P:P + 48].float())):
            assert (got - want).abs().max() <= 8 * eps(dtype) * want.abs().max(), i
    assert all(torch.equal(a, b) for a, b in zip(prefix.k, k0)) and all(torch.equal(a, b) for a, b in zip(prefix.v, v0))
    assert torch.equal(eng.extend(prefix, sfx).logits, res.logits)


@pytest.mark.parametrize("hidden,heads", [(128, 1), (256, 2)])
def test_append_then_decode_step_follow_the_oracle(ops, hidden, heads):
    """append: the n new rows' K / V land in the cache at rows P .., cache.length advances, the logits of the n rows come back; the next
    decode_step over the grown cache gives the oracle's next greedy token."""
    from oracle import leopard_oracle as O
    dtype = torch.float16
    cfg, eng, u8, pix, ids, Wn = _engine_setup(ops, dtype, hidden=hidden, heads=heads)
    head, tail = ids[:, :-48], ids[:, -48:]
    Wt = O.weights_from_numpy(Wn)
    ref_all = O.prefill_logits(ids, pix, Wt, cfg)[0]
    gen = O.greedy_generate(ids, pix, Wt, cfg, 2)[0, -2:].tolist()
    cache = _prefilled(eng, cfg, head, u8, dtype, spare=64)
    P = cache.length
    logits = eng.append(cache, tail)
    assert logits.shape == (48, cfg.text_config.vocab_size) and cache.length == P + 48
    assert (logits - ref_all[-48:]).abs().max() <= 2e-3 * 2
    assert int(logits[-1].argmax()) == gen[0]
    nxt = eng.decode_step(gen[0], cache)
    assert int(nxt.argmax()) == gen[1] and cache.length == P + 49
    with pytest.raises(ValueError, match="capacity"):
        eng.append(cache, torch.zeros(1, 64, dtype=torch.int64) + 3)


def test_generate_shared_equals_generate_on_the_concatenated_prompts(ops):
    """generate_shared: one prefix prefill, one extend, the pooled decode — the tokens generate() gives for [prefix ; suffix] (strict equality,
    as the generate_batch test of tests/test_emu_engine.py); the vision tower runs ONCE; a single suffix takes the batch-1 path; sampled:
    request i does not depend on N."""
    from leopard_amd.engine import SamplingParams
    dtype = torch.float16
    cfg, eng, u8, pix, ids, Wn = _engine_setup(ops, dtype)
    assert eng._batch_decode_supported()
    head = ids[:, :-48]
    sfx = [ids[:, -48:], ids[:, -48:-20], torch.tensor([[9, 8, 7, 6, 5]])]
    singles = [eng.generate(torch.cat([head, s], dim=1), u8, max_new_tokens=4, eos_token_id=()) for s in sfx]
    towers = []
    enc = eng.encode_images
    eng.encode_images = lambda *a, **k: (towers.append(1), enc(*a, **k))[1]
    got = eng.generate_shared(head, u8, sfx, max_new_tokens=4, eos_token_id=())
    assert len(towers) == 1
    for one, out in zip(singles, got):
        assert out.shape == one.shape and torch.equal(one, out), (one.tolist(), out.tolist())
    alone = eng.generate_shared(head, u8, sfx[1:2], max_new_tokens=4, eos_token_id=())
    assert torch.equal(alone[0], singles[1])
    eos = (int(singles[0][0, ids.shape[1] + 1]),)                  # request 0's second new token: it stops there
    cut = eng.generate_shared(head, u8, sfx, max_new_tokens=4, eos_token_id=eos)
    assert cut[0].shape[1] == ids.shape[1] + 2 and torch.equal(cut[0], singles[0][:, :ids.shape[1] + 2])
    sp = SamplingParams(temperature=0.9, top_k=20, top_p=0.95, seed=7)
    s3 = eng.generate_shared(head, u8, sfx, max_new_tokens=3, eos_token_id=(), sampling=sp)
    s1 = eng.generate_shared(head, u8, sfx[:1], max_new_tokens=3, eos_token_id=(), sampling=sp)
    assert torch.equal(s3[0], s1[0])


def test_continuation_error_paths_raise_before_any_launch(ops):
    from leopard_amd.engine import KVCache
    dtype = torch.float16
    cfg, eng, u8, pix, ids, Wn = _engine_setup(ops, dtype)
    head, tail = ids[:, :-48], ids[:, -48:]
    prefix = _prefilled(eng, cfg, head, u8, dtype)
    launches = []
    check = ops._check
    ops._check = lambda rc: (launches.append(1), check(rc))[1]
    try:
        with pytest.raises(ValueError, match="image token"):
            eng.extend(prefix, [torch.tensor([[5, cfg.image_token_index, 6]])])
        with pytest.raises(ValueError, match="empty"):
            eng.extend(prefix, [tail, torch.zeros(1, 0, dtype=torch.int64)])
        with pytest.raises(ValueError, match="empty"):
            eng.extend(KVCache(cfg, 16, dtype, "cpu"), [tail])
        with pytest.raises(ValueError, match="empty"):
            eng.append(KVCache(cfg, 16, dtype, "cpu"), tail)
        with pytest.raises(ValueError, match="image token"):
            eng.generate_shared(head, u8, [torch.tensor([[cfg.image_token_index]])])
        with pytest.raises(ValueError, match="kv_out"):
            eng.extend(prefix, [tail], kv_out=KVCache(cfg, 8, dtype, "cpu"))
        eng.split_operands = True
        with pytest.raises(NotImplementedError, match="split"):
            eng.extend(prefix, [tail])
        eng.split_operands = False
        cfg.text_config.sliding_window = 16
        with pytest.raises(NotImplementedError, match="sliding_window"):
            eng.extend(prefix, [tail])
        with pytest.raises(NotImplementedError, match="sliding_window"):
            eng.generate_shared(head, u8, [tail])
        cfg.text_config.sliding_window = 0
        eng._fp8 = object()
        with pytest.raises(NotImplementedError, match="fp8"):
            eng.append(prefix, tail)
        eng._fp8 = None
        eng.W.tp_size = 2
        with pytest.raises(NotImplementedError, match="tensor-parallel"):
            eng.extend(prefix, [tail])
        eng.W.tp_size = 1
        assert not launches
    finally:
        ops._check = check
