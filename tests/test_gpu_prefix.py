"""Continuing from a cached prefix on the MI355X: the two-range attention launch at the production shape, LeopardEngine.extend / append /
generate_shared on the mid model (full-width layers, 2 + 2, 8k vocabulary) against the fp32 oracle, extend at FULL depth against the committed
fixtures (tests/golden/c*_full_depth.npz), the multi-turn forward() of the model object, and the condition that sharing the prefix really saves
the work."""
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = 128
SUFFIX = 48                                       # synth_prompt_ids: the last 48 ids are the question and the assistant tail


def eps(dtype):
    return 2.0 ** -10 if dtype == torch.float16 else 2.0 ** -7          # one rounding of the 16-bit type (tests/test_gpu_kernels.py)


@pytest.fixture(scope="module")
def ops():
    from leopard_amd.ops import Ops
    return Ops()


# ---- 5. the kernel at the production shape ----------------------------------------------------------------------------------------------
def prefix_ref(q, k, v, kp, vp, cu, H, KV):
    """fp32 attention over the materialised [prefix ; own] keys, bottom-right causal (on the device: 7k keys x 32 heads)."""
    P = kp.shape[0]
    out = torch.zeros(q.shape[0], H * D, device=q.device)
    for a, b in zip(cu, cu[1:]):
        qs = q[a:b].float().view(-1, H, D).transpose(0, 1)
        ks = torch.cat([kp, k[a:b]]).float().view(-1, KV, D).transpose(0, 1).repeat_interleave(H // KV, 0)
        vs = torch.cat([vp, v[a:b]]).float().view(-1, KV, D).transpose(0, 1).repeat_interleave(H // KV, 0)
        sc = qs @ ks.transpose(-1, -2) * D ** -0.5
        m = torch.arange(P + b - a, device=q.device)[None, :] <= torch.arange(b - a, device=q.device)[:, None] + P
        o = torch.softmax(sc.masked_fill(~m, float("-inf")), -1) @ vs
        out[a:b] = o.transpose(0, 1).reshape(-1, H * D)
    return out


@pytest.mark.parametrize("P", [7139, 7104])
def test_prefix_attention_production_shape(ops, P):
    """H 32 / KV 8 / D 128, f16, the C3 prefix (7139 rows, not a multiple of 64) and an aligned one, eight own ranges of 33 .. 300 rows: within
    3 eps of fp32; run to run bit-identical; aligned: bit-identical to the existing kernel on the materialised copy."""
    H, KV, dtype = 32, 8, torch.float16
    lens = [33, 64, 65, 100, 129, 200, 257, 300]
    cu = [0] + [int(c) for c in np.cumsum(lens)]
    T = cu[-1]
    g = torch.Generator(device="cpu").manual_seed(P)
    qkv = torch.randn(T, (H + 2 * KV) * D, generator=g).to(dtype).to(DEV)
    q, k, v = qkv[:, :H * D], qkv[:, H * D:(H + KV) * D], qkv[:, (H + KV) * D:]
    cache = torch.randn(2, P + 64, KV * D, generator=g).to(dtype).to(DEV)             # rows >= P: must never be seen
    kp, vp = cache[0, :P], cache[1, :P]
    cu_t = torch.tensor(cu, dtype=torch.int32, device=DEV)
    outs = []
    for _ in range(2):
        out = torch.full((T, H * D), float("nan"), dtype=dtype, device=DEV)
        ops.attention_prefix(q, k, v, kp, vp, P, out, cu_t, max(lens), H, KV, D, D ** -0.5)
        outs.append(out)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    ref = prefix_ref(q, k, v, kp, vp, cu, H, KV)
    err = (outs[0].float() - ref).abs().max().item()
    print(f"[prefix attention P={P}] max abs err vs fp32 {err:.3e} (bound {3 * eps(dtype):.3e})")
    assert err <= 3 * eps(dtype)
    # the lo4 form: the same 16-bit rows
    from leopard_amd.ops import Lo4Act, lo4_head_k4
    act = Lo4Act.empty(T, H * D, dtype, DEV, k4=lo4_head_k4(H, D))
    ops.attention_prefix_lo4(q, k, v, kp, vp, P, act, cu_t, max(lens), H, KV, D, D ** -0.5)
    assert torch.equal(act.hi, outs[0])
    if P % 64 == 0:
        for a, b in zip(cu, cu[1:]):
            s = b - a
            kc, vc = torch.cat([kp, k[a:b]]).contiguous(), torch.cat([vp, v[a:b]]).contiguous()
            one = torch.empty(s, H * D, dtype=dtype, device=DEV)
            ops.attention(q[a:b].contiguous(), kc, vc, one, torch.tensor([0, s], dtype=torch.int32, device=DEV),
                          torch.tensor([0, P + s], dtype=torch.int32, device=DEV), s, H, KV, D, D ** -0.5, True)
            assert torch.equal(outs[0][a:b], one), (a, b)


# ---- the mid model (tests/test_gpu_scoring.py builds it the same way) ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def mid():
    from leopard_amd import compat
    from leopard_amd.config import mid_config
    from leopard_amd.ops import Ops
    from leopard_amd.weights import SynthSource
    cfg, ops = mid_config(), Ops()
    m = compat.LeopardForConditionalGeneration(cfg, lambda dev, dt: SynthSource(cfg, ops, dev, dt), torch.float16, ops, torch_dtype=torch.float16)
    return m.to(DEV)


def mid_sample(cfg, n_images=1, seed=0, w=800, h=500):
    from tools.gen_fulldepth_fixtures import sample_inputs
    u8, ids = sample_inputs(cfg, n_images, w, h, seed=seed)[:2]
    return torch.from_numpy(u8).to(DEV), ids


def prefilled(eng, cfg, ids, tiles, spare=0):
    from leopard_amd.engine import KVCache
    cache = KVCache(cfg, eng.merged_len(ids) + spare, eng.dtype, DEV)
    eng.prefill(ids.to(DEV), tiles, cache=cache)
    return cache


def suffixes_of(cfg, n, lo=33, seed=0):
    """n text suffixes of different lengths lo, lo + 1, ..."""
    g = np.random.default_rng(seed)
    hi = min(cfg.text_config.vocab_size, 128000)
    out = []
    for j in range(n):
        x = g.integers(3, hi, lo + j)
        x[x == cfg.image_token_index] = 3
        out.append(torch.from_numpy(x).reshape(1, -1).to(DEV))
    return out


@pytest.mark.parametrize("precision,tol", [("fast", 1.25e-3), ("lo4", 1.0e-3)])
def test_extend_mid_model_vs_oracle(mid, precision, tol):
    """6. extend's last-row logits against the fp32 oracle's last position of the whole prompt, normalised by the logit scale: LOGIT_TOL[f16]
    on the fast schedule, 1e-3 under lo4, argmax equal; the from-scratch prefill's own distance printed beside it."""
    from leopard_amd.synth import synth_state_dict_numpy
    from leopard_amd.tiler import siglip_normalize
    from oracle import leopard_oracle as O
    cfg, eng = mid.config, mid.engine
    tiles, ids = mid_sample(cfg)
    W = O.weights_from_numpy(synth_state_dict_numpy(cfg))
    ref = O.prefill_logits(ids, torch.from_numpy(siglip_normalize(tiles.cpu().numpy())), W, cfg, last_only=True)[0, 0]
    was = eng.precision
    eng.precision = precision
    try:
        prefix = prefilled(eng, cfg, ids[:, :-SUFFIX], tiles)
        got = eng.extend(prefix, [ids[:, -SUFFIX:].to(DEV)]).logits[0].float().cpu()
        scratch = eng.prefill(ids.to(DEV), tiles).logits_last.float().cpu()
    finally:
        eng.precision = was
    scale = ref.abs().max().item()
    n, n0 = (got - ref).abs().max().item() / scale, (scratch - ref).abs().max().item() / scale
    print(f"[extend, mid, {precision}] normalised max|logit diff| vs fp32 oracle: extend {n:.3e}, from-scratch prefill {n0:.3e} (bound {tol:.2e})")
    assert n <= tol and int(got.argmax()) == int(ref.argmax())


# ---- 7. full depth, the committed fixtures ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full_engine(ops):
    from leopard_amd.config import full_config
    from leopard_amd.engine import LeopardEngine
    from leopard_amd.weights import EngineWeights, SynthSource
    cfg = full_config()
    W = EngineWeights.build(cfg, SynthSource(cfg, ops, torch.device(DEV), torch.float16), torch.float16)
    eng = LeopardEngine(cfg, W, ops=ops, device=torch.device(DEV))
    yield eng
    del eng, W
    torch.cuda.empty_cache()


@pytest.mark.parametrize("precision", ["lo4", "fast"])
@pytest.mark.parametrize("case", ["c1", "c2", "c3"])
def test_extend_full_depth_vs_committed_fixtures(full_engine, case, precision):
    """27 SigLIP + 32 Llama-3.1-8B layers: the fixture's inputs regenerated (ids and tile hash checked), split at len(ids) - 48, the prefix
    prefilled and the suffix extended; last-position logits against the fixture's fp32 oracle, normalised by the logit scale, with its argmax:
    within 1e-3 under lo4 (the bound test_full_depth_lo4_meets_1e_3 holds the from-scratch prefill to; measured there 6.4e-4 / 4.0e-4 /
    2.75e-4), and on the fast schedule within FULL_TOL of tests/test_gpu_parity.py for the same case."""
    from tests.test_gpu_parity import FULL_TOL, FullDepthFixture
    fx = FullDepthFixture(case)
    eng, cfg = full_engine, full_engine.cfg
    eng.precision = precision
    tiles = torch.from_numpy(fx.u8).to(DEV)
    prefix = prefilled(eng, cfg, fx.ids[:, :-SUFFIX], tiles)
    assert prefix.length == fx.S - SUFFIX
    got = eng.extend(prefix, [fx.ids[:, -SUFFIX:].to(DEV)]).logits[0].float().cpu()
    scratch = eng.prefill(fx.ids.to(DEV), tiles).logits_last.float().cpu()
    scale = fx.ref.abs().max().item()
    n, n0 = (got - fx.ref).abs().max().item() / scale, (scratch - fx.ref).abs().max().item() / scale
    tol = 1.0e-3 if precision == "lo4" else FULL_TOL[(case, torch.float16)]
    print(f"[extend, {case} full depth fp16, {precision}] normalised max|logit diff| vs fp32 oracle: extend {n:.3e}, from-scratch prefill {n0:.3e} "
          f"(bound {tol:.2e}); argmax equal = {int(got.argmax()) == int(fx.ref.argmax())}")
    del prefix
    torch.cuda.empty_cache()
    assert n <= tol and int(got.argmax()) == int(fx.ref.argmax())


# ---- 8. fan-out and reuse ---------------------------------------------------------------------------------------------------------------
def test_extend_fan_out_reuse_and_order(mid):
    """Eight suffixes of different lengths (all > 32 rows) through one extend == each alone, bit for bit; a second extend on the same prefix,
    after a generation that started from it, gives the first one's bits (the prefix is never written); 17 suffixes (> MAX_DECODE_BATCH) come
    back in order."""
    cfg, eng = mid.config, mid.engine
    tiles, ids = mid_sample(cfg, seed=2)
    head = ids[:, :-SUFFIX].to(DEV)
    prefix = prefilled(eng, cfg, head, tiles)
    k0, v0 = [t.clone() for t in prefix.k], [t.clone() for t in prefix.v]
    sfx = suffixes_of(cfg, 8)
    both = eng.extend(prefix, sfx).logits.clone()
    for j, s in enumerate(sfx):
        assert torch.equal(eng.extend(prefix, [s]).logits[0], both[j]), j
    outs = eng.generate_shared(head, tiles, sfx[:3], max_new_tokens=4, eos_token_id=(), prefix=prefix)
    assert all(o.shape[1] == head.shape[1] + s.shape[1] + 4 for o, s in zip(outs, sfx))
    assert torch.equal(eng.extend(prefix, sfx).logits, both)
    assert all(torch.equal(a, b) for a, b in zip(prefix.k, k0)) and all(torch.equal(a, b) for a, b in zip(prefix.v, v0))
    many = suffixes_of(cfg, 17, seed=5)
    assert len(many) > eng.MAX_DECODE_BATCH
    got = eng.generate_shared(head, tiles, many, max_new_tokens=2, eos_token_id=(), prefix=prefix)
    assert len(got) == 17
    for j, (s, o) in enumerate(zip(many, got)):
        n_in = head.shape[1] + s.shape[1]
        assert o.shape == (1, n_in + 2) and torch.equal(o[0, :head.shape[1]], head[0]) and torch.equal(o[0, head.shape[1]:n_in], s[0]), j
        assert int(o[0, n_in]) == int(eng.extend(prefix, [s]).logits[0].argmax()), j
    eng.release_batch_state()


# ---- 9. generation ----------------------------------------------------------------------------------------------------------------------
def assert_equal_or_near_tie(eng, cfg, ids, tiles, one, got):
    """tests/test_gpu_parity.py, generate_batch: equal, or differing first where the reference run's top two logits are within the 16-bit noise."""
    from leopard_amd.engine import KVCache
    assert got.shape == one.shape
    if torch.equal(one, got):
        return True
    S_in = ids.shape[1]
    j = int((one[0] != got[0]).nonzero()[0])
    assert j >= S_in
    cache = KVCache(cfg, one.shape[1] + 256 * 8 + eng.merged_len(ids), torch.float16, DEV)
    lg = eng.prefill(ids, tiles, cache=cache).logits_last.clone()
    nxt = int(one[0, S_in])
    for t in range(S_in + 1, j + 1):
        lg = eng.decode_step(nxt, cache).clone()
        nxt = int(one[0, t])
    top2 = lg.topk(2).values
    assert float(top2[0] - top2[1]) <= 2e-3 * float(lg.abs().max()), (j, top2)
    return False


@pytest.mark.parametrize("w,h", [(336, 336), (1344, 896)])
def test_generate_shared_vs_generate(mid, w, h):
    """generate_shared (greedy) against generate on each concatenated prompt, C1- and C2-size images, 16 new tokens: equal, or a near tie of
    the reference run at the first difference."""
    cfg, eng = mid.config, mid.engine
    tiles, ids = mid_sample(cfg, seed=4, w=w, h=h)
    head = ids[:, :-SUFFIX].to(DEV)
    sfx = [ids[:, -SUFFIX:].to(DEV)] + suffixes_of(cfg, 3, lo=40, seed=9)
    T = 16
    singles = [eng.generate(torch.cat([head, s], dim=1), tiles, max_new_tokens=T, eos_token_id=()) for s in sfx]
    got = eng.generate_shared(head, tiles, sfx, max_new_tokens=T, eos_token_id=())
    same = [assert_equal_or_near_tie(eng, cfg, torch.cat([head, s], dim=1), tiles, one, out) for s, one, out in zip(sfx, singles, got)]
    print(f"[generate_shared {w}x{h}] {sum(same)} / {len(sfx)} outputs identical to generate() on the concatenated prompt")
    eng.release_batch_state()


def test_generate_shared_sampled_request_does_not_depend_on_n(mid):
    """Request i draws with sampling.for_request(i): the same tokens whether 1, 2 or 4 suffixes run (same seed), as
    tests/test_gpu_sampling.py asserts for generate_stream across batch sizes."""
    cfg, eng = mid.config, mid.engine
    tiles, ids = mid_sample(cfg, seed=6)
    head = ids[:, :-SUFFIX].to(DEV)
    sfx = suffixes_of(cfg, 4, lo=40, seed=3)
    n_in = head.shape[1] + sfx[0].shape[1]
    kw = dict(max_new_tokens=8, eos_token_id=[], do_sample=True, temperature=0.8, top_k=40, top_p=0.95, seed=11)
    one = mid.generate_shared(head, tiles, sfx[:1], **kw)
    two = mid.generate_shared(head, tiles, sfx[:2], **kw)
    four = mid.generate_shared(head, tiles, sfx, **kw)
    print(f"[generate_shared sampled] request 0: N=1 {one[0][0, n_in:].tolist()} N=4 {four[0][0, n_in:].tolist()}")
    assert one[0].shape == four[0].shape == (1, n_in + 8)
    assert torch.equal(two[0], four[0]) and torch.equal(two[1], four[1])
    assert torch.equal(one[0], four[0])
    assert not torch.equal(four[0][0, n_in:], four[1][0, four[1].shape[1] - 8:])          # per-request seeds: different draws
    eng.release_batch_state()


# ---- 10. multi-turn -----------------------------------------------------------------------------------------------------------------------
def test_forward_multi_turn_appends_to_the_cache(mid):
    """forward(images, use_cache=True), then forward(past_key_values=cache, 20 more ids): the second call's logits against the oracle's logits
    of the concatenation at those 20 rows (LOGIT_TOL[f16], normalised), cache.length advanced by 20, and an n == 1 decode call still works."""
    from leopard_amd.synth import synth_state_dict_numpy
    from leopard_amd.tiler import siglip_normalize
    from oracle import leopard_oracle as O
    cfg, eng = mid.config, mid.engine
    tiles, ids = mid_sample(cfg, seed=1)
    more = suffixes_of(cfg, 1, lo=20, seed=8)[0]
    first = mid.forward(ids.to(DEV), tiles, use_cache=True)
    cache = first.past_key_values
    L0 = cache.length
    second = mid.forward(more, past_key_values=cache)
    assert second.logits.shape == (1, 20, cfg.text_config.vocab_size) and cache.length == L0 + 20 and second.past_key_values is cache
    W = O.weights_from_numpy(synth_state_dict_numpy(cfg))
    whole = torch.cat([ids, more.cpu()], dim=1)
    ref = O.prefill_logits(whole, torch.from_numpy(siglip_normalize(tiles.cpu().numpy())), W, cfg)[0]
    n = (second.logits[0].float().cpu() - ref[-20:]).abs().max().item() / ref.abs().max().item()
    print(f"[multi-turn forward] 20 appended rows vs fp32 oracle of the concatenation: normalised max|logit diff| {n:.3e} (bound 1.25e-3)")
    assert n <= 1.25e-3
    nxt = int(second.logits[0, -1].argmax())
    third = mid.forward(torch.tensor([[nxt]], device=DEV), past_key_values=cache)
    assert third.logits.shape == (1, 1, cfg.text_config.vocab_size) and cache.length == L0 + 21
    ref3 = O.prefill_logits(torch.cat([whole, torch.tensor([[nxt]])], dim=1), torch.from_numpy(siglip_normalize(tiles.cpu().numpy())), W, cfg,
                            last_only=True)[0, 0]
    assert (third.logits[0, 0].float().cpu() - ref3).abs().max().item() / ref3.abs().max().item() <= 1.25e-3
    with pytest.raises(NotImplementedError):
        mid.forward(more, past_key_values=cache, labels=more)


# ---- 11. it must actually save the work ---------------------------------------------------------------------------------------------------
def test_generate_shared_saves_the_prefill_work(mid):
    """The mid model, the C3-size sample (6 x 1344x896: 7187 merged rows, 7139 of them shared), eight 48-id suffixes, max_new_tokens = 1:
    median of 5 timed runs after 2 warm-ups of generate_shared against generate_batch of the eight concatenated prompts, same process.
    Required: generate_shared <= 0.5 x generate_batch.  The rows through the towers fall from 8 x 7187 to 7139 + 8 x 48 (0.13 of the work);
    the bound leaves a factor 3.8 for the small-M GEMMs of the extend step and the slot copies."""
    cfg, eng = mid.config, mid.engine
    tiles, ids = mid_sample(cfg, n_images=6, w=1344, h=896)
    head = ids[:, :-SUFFIX].to(DEV)
    assert eng.merged_len(ids) == 7187 and eng.merged_len(head) == 7139
    g = np.random.default_rng(12)
    sfx = [ids[:, -SUFFIX:].to(DEV)]
    for _ in range(7):
        x = g.integers(3, min(cfg.text_config.vocab_size, 128000), SUFFIX)
        x[x == cfg.image_token_index] = 3
        sfx.append(torch.from_numpy(x).reshape(1, -1).to(DEV))
    full = [(torch.cat([head, s], dim=1), tiles) for s in sfx]

    def timed(fn):
        for _ in range(2):
            out = fn()
        ts = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)), out

    t_shared, a = timed(lambda: eng.generate_shared(head, tiles, sfx, max_new_tokens=1, eos_token_id=()))
    t_batch, b = timed(lambda: eng.generate_batch(full, max_new_tokens=1, eos_token_id=()))
    agree = sum(torch.equal(x, y) for x, y in zip(a, b))
    print(f"[prefix reuse, mid model, C3 sample, 8 x 48-id suffixes] generate_shared {t_shared * 1e3:.1f} ms, generate_batch {t_batch * 1e3:.1f} ms: "
          f"ratio {t_shared / t_batch:.3f} (required <= 0.5); {agree} / 8 first tokens equal")
    eng.release_batch_state()
    assert all(x.shape == y.shape for x, y in zip(a, b))
    assert t_shared <= 0.5 * t_batch
