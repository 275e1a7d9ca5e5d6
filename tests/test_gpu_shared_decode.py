"""-m gpu: shared-prefix batched decode on the MI355X — lmi_attn_decode_shared / _hl at small shapes and once at the production shape (also
inside a captured graph whose key counts advance on the device), LeopardEngine.generate_shared(decode="shared") on the mid model against
generate() on the concatenated prompts, and the memory the decode state holds.  No timing assertions: time is reported by
tools/prefix_reuse_bench.py --decode shared."""
import numpy as np
import pytest
import torch

from tests import shared_decode_ref as R
from tests.decode_hl_ref import pair_gain, pair_rows_checks

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = R.D
SUFFIX = 48                                       # synth_prompt_ids: the last 48 ids are the question and the assistant tail
H, KV = 32, 8


@pytest.fixture(scope="module")
def ops():
    from leopard_amd.ops import Ops
    return Ops()


def mixed_lens(B, seed):
    """Own lengths 1 .. 600, the ends included: slots of 640 rows are ten tiles in several splits — empty for some sequences, all used by others."""
    g = np.random.default_rng(seed)
    return ([1, 600, 64, 65, 129] + [int(x) for x in g.integers(1, 601, 16)])[:B]


# ---- 1. the kernel, small ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("B", [1, 5, 16])
@pytest.mark.parametrize("P", [64, 513, 1100])
def test_shared_decode_small_vs_fp32(ops, P, B, dtype):
    """H 32 / KV 8: within 3 eps of fp32 over the materialised [prefix ; own] keys (prefix rows >= P and slot rows >= k_len are NaN and must
    never be seen), run to run bit-identical."""
    c = R.make_case(P, P + 64, mixed_lens(B, P + B), 640, H, KV, dtype, 2000 + P + B)
    args = tuple(t.to(DEV) for t in (c.kp, c.vp, c.k, c.v))
    out = R.run(ops, c, DEV, device_args=args)
    assert bool((out[B] == R.GUARD).all()) and not torch.isnan(out.float()).any()
    err = (out[:B].float() - R.reference(c, DEV).cpu()).abs().max().item()
    print(f"[decode_shared P={P} B={B} {dtype}] max abs err vs fp32 {err:.3e} (bound {3 * R.eps(dtype):.3e})")
    assert err <= 3 * R.eps(dtype)
    assert torch.equal(out, R.run(ops, c, DEV, device_args=args))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_a_sequence_does_not_depend_on_its_batch_mates(ops, dtype):
    """Sequence j alone == sequence j among 16, bit for bit, for every j.  P = 4200 is 67 tiles in 23 prefix splits of three, so the deferred
    rescale can fire inside a split; the K rows of odd tiles are doubled and every other q row is scaled by 8, so scaled rows cross the
    threshold where unscaled ones do not (tests/test_emu_shared_decode.py: a wave-uniform update fails this for every unscaled row)."""
    B, P = 16, 4200
    c = R.make_case(P, P + 64, mixed_lens(B, 5), 640, H, KV, dtype, 77, q_scale=[8.0 if s % 2 == 0 else 1.0 for s in range(B)])
    c.kp[:P] = (c.kp[:P].float() * (1 + (torch.arange(P) // 64) % 2).to(torch.float32)[:, None]).to(dtype)
    args = tuple(t.to(DEV) for t in (c.kp, c.vp, c.k, c.v))
    batch = R.run(ops, c, DEV, device_args=args)
    assert not torch.isnan(batch.float()).any()
    assert (batch[:B].float() - R.reference(c, DEV).cpu()).abs().max() <= 3 * R.eps(dtype)
    for j in range(B):
        assert torch.equal(R.run(ops, c, DEV, rows=[j], device_args=args)[0], batch[j]), j


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_shared_decode_hl_pairs_b8(ops, dtype):
    """_hl at B = 8: hi rows == the plain launch, lo rows the residuals of their rounding, hi + lo closer to fp64 than hi alone."""
    B, P = 8, 513
    c = R.make_case(P, P + 64, mixed_lens(B, 9), 640, H, KV, dtype, 31)
    args = tuple(t.to(DEV) for t in (c.kp, c.vp, c.k, c.v))
    one, two = R.run(ops, c, DEV, device_args=args), R.run(ops, c, DEV, hl=True, device_args=args)
    assert torch.equal(two, R.run(ops, c, DEV, hl=True, device_args=args))
    pair_rows_checks(two, one[:B], B, dtype, "decode_shared_hl")
    assert two[B:2 * B].double().abs().max() > 0
    e_two, e_one = pair_gain(two, B, R.reference(c, DEV, torch.float64).cpu())
    print(f"[decode_shared_hl {dtype}] hi + lo error {e_two:.3e}, hi alone {e_one:.3e}")
    assert e_two < 0.8 * e_one


# ---- 2. the kernel at the production shape, once ------------------------------------------------------------------------------------------
def test_shared_decode_production_shape_and_graph_replay(ops):
    """P = 7139 in a prefix buffer of 7168 rows, B = 16, own lengths 49 .. 176 in slots of 256 rows: within 3 eps of fp32 (reference on the
    device); then the launch inside a captured graph, replayed twice with k_len advanced on the device in between — each replay equals an
    eager launch at those lengths."""
    from leopard_amd.engine import _capture_safe
    dtype, P, cap_p, cap_o, B = torch.float16, 7139, 7168, 256, 16
    lens = [49 + (127 * s) // 15 for s in range(B)]
    assert lens[0] == 49 and lens[-1] == 176
    c = R.make_case(P, cap_p, lens, cap_o, H, KV, dtype, 4242)
    kp, vp, k, v = (t.to(DEV) for t in (c.kp, c.vp, c.k, c.v))
    out = R.run(ops, c, DEV, device_args=(kp, vp, k, v))
    assert not torch.isnan(out.float()).any()
    err = (out[:B].float() - R.reference(c, DEV).cpu()).abs().max().item()
    print(f"[decode_shared production shape] max abs err vs fp32 {err:.3e} (bound {3 * R.eps(dtype):.3e})")
    assert err <= 3 * R.eps(dtype)
    # captured: rows behind k_len become real keys as k_len advances (finite values now, as after an append)
    pool = torch.cat([k, v], dim=1)
    pool[torch.isnan(pool)] = 0.25
    k, v = pool[:, :KV * D], pool[:, KV * D:]
    q = c.q.to(DEV)
    plen = torch.tensor([P], dtype=torch.int32, device=DEV)
    k_begin = (torch.arange(B, dtype=torch.int32) * cap_o).to(DEV)
    k_len = torch.tensor(lens, dtype=torch.int32, device=DEV)
    ws = torch.empty(ops.decode_shared_workspace_elems(B, H, D, cap_p, cap_o), dtype=torch.float32, device=DEV)
    got = torch.zeros(B, H * D, dtype=dtype, device=DEV)

    def launch(o, kl):
        ops.attention_decode_shared(q, kp, vp, plen, cap_p, k, v, o, k_begin, kl, cap_o, H, KV, D, D ** -0.5, ws)

    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        launch(got, k_len)
    torch.cuda.current_stream(DEV).wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with _capture_safe(), torch.cuda.graph(g):
        launch(got, k_len)
    for step in (1, 2):
        k_len += 1
        g.replay()
        want = torch.zeros_like(got)
        launch(want, k_len.clone())
        torch.cuda.synchronize()
        assert torch.equal(got, want), step
    assert not torch.equal(got, out[:B].to(DEV))                   # the two more keys were seen


# ---- 3. the engine, mid model -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mid():
    from leopard_amd import compat
    from leopard_amd.config import mid_config
    from leopard_amd.ops import Ops
    from leopard_amd.weights import SynthSource
    cfg, ops = mid_config(), Ops()
    m = compat.LeopardForConditionalGeneration(cfg, lambda dev, dt: SynthSource(cfg, ops, dev, dt), torch.float16, ops, torch_dtype=torch.float16)
    return m.to(DEV)


def mid_sample(cfg, n_images=1, seed=0, w=336, h=336):
    from tools.gen_fulldepth_fixtures import sample_inputs
    u8, ids = sample_inputs(cfg, n_images, w, h, seed=seed)[:2]
    return torch.from_numpy(u8).to(DEV), ids


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


def assert_equal_or_near_tie(eng, cfg, ids, tiles, one, got):
    """tests/test_gpu_prefix.py: equal, or differing first where the reference run's top two logits are within the 16-bit noise."""
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


@pytest.mark.parametrize("precision", ["fast", "lo4"])
def test_generate_shared_decode_shared_vs_generate(mid, precision):
    """A 336 x 336 image, 4 suffixes, 12 new tokens, greedy: decode="shared" against generate() on each concatenated prompt — equal, or a near
    tie of the reference run at the first difference.  Under lo4 the step is the pair (hl) one at B = 4.  The caller's prefix is untouched."""
    from leopard_amd.engine import KVCache
    cfg, eng = mid.config, mid.engine
    tiles, ids = mid_sample(cfg, seed=4)
    head = ids[:, :-SUFFIX].to(DEV)
    sfx = [ids[:, -SUFFIX:].to(DEV)] + suffixes_of(cfg, 3, lo=40, seed=9)
    T = 12
    was = eng.precision
    eng.precision = precision
    try:
        singles = [eng.generate(torch.cat([head, s], dim=1), tiles, max_new_tokens=T, eos_token_id=()) for s in sfx]
        prefix = KVCache(cfg, eng.merged_len(head), eng.dtype, DEV)
        eng.prefill(head, tiles, cache=prefix)
        k0 = [t.clone() for t in prefix.k]
        got = eng.generate_shared(head, tiles, sfx, max_new_tokens=T, eos_token_id=(), prefix=prefix, decode="shared")
        st = eng._batch_states[("shared", 4)]
        assert st.hl == (precision == "lo4") and st.kp is not None and int(st.prefix_len[0]) == prefix.length
        assert all(torch.equal(a, b) for a, b in zip(prefix.k, k0))
        same = [assert_equal_or_near_tie(eng, cfg, torch.cat([head, s], dim=1), tiles, one, out) for s, one, out in zip(sfx, singles, got)]
        print(f"[generate_shared decode=shared {precision}] {sum(same)} / {len(sfx)} outputs identical to generate() on the concatenated prompt")
    finally:
        eng.precision = was
        eng.release_batch_state()


def test_generate_shared_decode_shared_sampled_request_does_not_depend_on_n(mid):
    """Sampled: request i draws the same tokens for N = 2 and N = 4 (same seed)."""
    cfg = mid.config
    tiles, ids = mid_sample(cfg, seed=6)
    head = ids[:, :-SUFFIX].to(DEV)
    sfx = suffixes_of(cfg, 4, lo=40, seed=3)
    kw = dict(max_new_tokens=8, eos_token_id=[], do_sample=True, temperature=0.8, top_k=40, top_p=0.95, seed=11, decode="shared")
    two = mid.generate_shared(head, tiles, sfx[:2], **kw)
    four = mid.generate_shared(head, tiles, sfx, **kw)
    assert torch.equal(two[0], four[0]) and torch.equal(two[1], four[1])
    assert not torch.equal(four[0][0, -8:], four[1][0, -8:])       # per-request seeds: different draws
    mid.engine.release_batch_state()


# ---- 4. memory, deterministic -----------------------------------------------------------------------------------------------------------
def test_shared_decode_state_memory(mid):
    """P about 1200 (a 1344 x 896 image: 7 tiles of 169 tokens), 8 suffixes: the decode state's K / V bytes under "shared" are exactly (prefix_capacity + B x
    own_capacity) x row bytes x layers, and below half of the "copy" state's for the same call."""
    cfg, eng = mid.config, mid.engine
    tiles, ids = mid_sample(cfg, seed=2, w=1344, h=896)
    head = ids[:, :-SUFFIX].to(DEV)
    P = eng.merged_len(head)
    assert 1000 <= P <= 1400, P
    sfx = suffixes_of(cfg, 8)
    eng.release_batch_state()
    kv_bytes = lambda ts: sum(t.numel() * t.element_size() for t in ts)
    eng.generate_shared(head, tiles, sfx, max_new_tokens=3, eos_token_id=(), decode="shared")
    st = eng._batch_states[("shared", 8)]
    tc = cfg.text_config
    row = 2 * tc.num_key_value_heads * tc.head_dim * 2
    shared = kv_bytes(st.k + st.v + st.kp + st.vp)
    assert shared == (st.prefix_capacity + 8 * st.capacity) * row * tc.num_hidden_layers
    assert st.prefix_capacity >= P and st.capacity >= max(s.shape[1] for s in sfx) + 3
    eng.generate_shared(head, tiles, sfx, max_new_tokens=3, eos_token_id=())
    sc = eng._batch_states[8]
    copy = kv_bytes(sc.k + sc.v)
    print(f"[decode state K / V bytes, P={P}, 8 suffixes] shared {shared} ({st.prefix_capacity} + 8 x {st.capacity} rows), copy {copy} (8 x {sc.capacity} rows)")
    assert shared < 0.5 * copy
    eng.release_batch_state()
