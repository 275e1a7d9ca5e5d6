"""-m gpu: row-packed two-range attention on the MI355X — lmi_attn_prefix_rows at H 32 / KV 8 against fp32 attention over the materialised
keys: row tiles of 32 with rows of many continuations, per-row own ranges, the fp32-output merge and lmi_split_lo4 behind it, and once at the
production shape beside lmi_attn_prefix_fwd.  No timing assertions: time is reported by tools/score_shared_bench.py."""
import numpy as np
import pytest
import torch

from tests import prefix_rows_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = R.D
H, KV = 32, 8
FORTY = [1 + (7 * j) % 3 for j in range(40)]                   # 40 suffixes of 1 - 3 rows: R = 79 > 32, tiles that mix many suffixes
SUFFIXES = {"four_single": [1, 1, 1, 1], "ragged": [1, 2, 33, 64, 65], "forty_short": FORTY}


@pytest.fixture(scope="module")
def ops():
    from leopard_amd.ops import Ops
    return Ops()


def on_device(c):
    return tuple(t.to(DEV) for t in (c.kp, c.vp, c.k, c.v))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("name", list(SUFFIXES))
@pytest.mark.parametrize("P", [64, 513, 1100])
def test_prefix_rows_small_vs_fp32(ops, P, name, dtype):
    """Within 3 eps of fp32 over the materialised [prefix ; own] keys (the bound tests/test_gpu_shared_decode.py holds the same arithmetic to;
    prefix rows >= P and pool rows outside every range are NaN and must never be seen); the guard row after R is untouched; a relaunch is
    bit-identical."""
    lens = SUFFIXES[name]
    c = R.make_case(P, lens, H, KV, dtype, 3000 + P + len(lens))
    args = on_device(c)
    out = R.run(ops, c, DEV, device_args=args)
    assert bool((out[c.R] == R.GUARD).all()) and not torch.isnan(out.float()).any()
    err = (out[:c.R].float() - R.reference(c, DEV).cpu()).abs().max().item()
    print(f"[prefix_rows P={P} {name} R={c.R} {dtype}] max abs err vs fp32 {err:.3e} (bound {3 * R.eps(dtype):.3e})")
    assert err <= 3 * R.eps(dtype)
    assert torch.equal(out, R.run(ops, c, DEV, device_args=args))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_a_row_does_not_depend_on_the_other_rows(ops, dtype):
    """Row r alone == row r among all others, bit for bit, for every r.  P = 4200 is 67 tiles in 23 prefix splits of three, so the deferred
    rescale can fire inside a split; the K rows of odd tiles are doubled and every other q row is scaled by 8, so scaled rows cross the
    threshold where their unscaled tile mates do not (test_a_sequence_does_not_depend_on_its_batch_mates' construction)."""
    P, lens = 4200, [1, 2, 33]
    Rn = sum(lens)
    c = R.make_case(P, lens, H, KV, dtype, 77, q_scale=[8.0 if r % 2 == 0 else 1.0 for r in range(Rn)])
    c.kp[:P] = (c.kp[:P].float() * (1 + (torch.arange(P) // 64) % 2).to(torch.float32)[:, None]).to(dtype)
    args = on_device(c)
    batch = R.run(ops, c, DEV, device_args=args)
    assert not torch.isnan(batch.float()).any()
    assert (batch[:Rn].float() - R.reference(c, DEV).cpu()).abs().max() <= 3 * R.eps(dtype)
    for r in range(Rn):
        assert torch.equal(R.run(ops, c, DEV, rows=[r], device_args=args)[0], batch[r]), r


def test_causality_is_the_key_count(ops):
    """Overwriting the own rows > i of a suffix leaves its rows <= i bit-identical (rows > i change: they saw those keys)."""
    dtype, P, lens, i = torch.float16, 513, [5, 33, 2], 10
    c = R.make_case(P, lens, H, KV, dtype, 91)
    before = R.run(ops, c, DEV)
    b = c.begin[1]
    c.k[b + i + 1:b + 33] = c.k[b + i + 1:b + 33] * -3.0 + 1.0
    c.v[b + i + 1:b + 33] = 5.0
    after = R.run(ops, c, DEV)
    first = 5                                                      # the 33-row suffix starts at query row 5
    assert torch.equal(after[:first + i + 1], before[:first + i + 1])
    assert torch.equal(after[first + 33:], before[first + 33:])
    assert not torch.equal(after[first + i + 1:first + 33], before[first + i + 1:first + 33])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_fp32_rows_and_the_lo4_pair_made_of_them(ops, dtype):
    """The fp32-output launch writes the T rows of the plain launch; lmi_split_lo4 of its fp32 rows gives those T rows again and a residual
    image that, dequantised and added to T, is closer to the fp64 reference than T alone."""
    from leopard_amd.ops import Lo4Act, lo4_head_k4
    from tests.test_emu_lowbit import decode_img
    P, lens = 513, [1, 2, 33, 4]
    c = R.make_case(P, lens, H, KV, dtype, 57)
    args = on_device(c)
    plain = R.run(ops, c, DEV, device_args=args)
    out, o32 = R.run(ops, c, DEV, f32=True, device_args=args)
    assert torch.equal(out, plain)
    assert bool((o32[c.R] == R.GUARD).all()) and not torch.isnan(o32).any()
    act = Lo4Act.empty(c.R, H * D, dtype, DEV, k4=lo4_head_k4(H, D))
    ops.split_lo4(o32[:c.R].to(DEV), act)
    torch.cuda.synchronize()
    assert torch.equal(act.hi.cpu(), out[:c.R])
    ref = R.reference(c, DEV, torch.float64).cpu()
    hi = act.hi.cpu().double()
    both = hi + decode_img(act.img.cpu(), act.sc.cpu(), H * D).double()
    e_hi, e_both = (hi - ref).abs().max().item(), (both - ref).abs().max().item()
    print(f"[prefix_rows + split_lo4 {dtype}] T + image error {e_both:.3e}, T alone {e_hi:.3e}: ratio {e_both / e_hi:.3f}")
    assert e_both < e_hi


def test_production_shape_beside_the_two_range_launch(ops):
    """P = 7139, 16 suffixes of 1 - 8 rows: lmi_attn_prefix_rows and lmi_attn_prefix_fwd on the same inputs, both within 3 eps of fp32."""
    dtype, P = torch.float16, 7139
    lens = [1 + (5 * j) % 8 for j in range(16)]
    assert min(lens) == 1 and max(lens) == 8
    c = R.make_case(P, lens, H, KV, dtype, 4242)
    kp, vp, k, v = on_device(c)
    ref = R.reference(c, DEV).cpu()
    rows = R.run(ops, c, DEV, device_args=(kp, vp, k, v))[:c.R]
    own = torch.from_numpy(c.k_begin + c.k_len - 1).to(DEV, torch.int64)         # query row r's own K / V row in the pool
    kc, vc = k[own].contiguous(), v[own].contiguous()
    cu = torch.tensor([0] + [int(x) for x in np.cumsum(lens)], dtype=torch.int32, device=DEV)
    two = torch.full((c.R, H * D), float("nan"), dtype=dtype, device=DEV)
    ops.attention_prefix(c.q.to(DEV), kc, vc, kp[:P], vp[:P], P, two, cu, max(lens), H, KV, D, D ** -0.5)
    torch.cuda.synchronize()
    e_rows, e_two = (rows.float() - ref).abs().max().item(), (two.cpu().float() - ref).abs().max().item()
    print(f"[production shape P={P} R={c.R}] max abs err vs fp32: rows {e_rows:.3e}, two-range {e_two:.3e} (bound {3 * R.eps(dtype):.3e})")
    assert e_rows <= 3 * R.eps(dtype) and e_two <= 3 * R.eps(dtype)


def test_prefix_rows_rejects_bad_arguments(ops):
    """LMI_EINVAL (a RuntimeError from Ops), never a trap, and nothing written: head_dim 64, 32 / 32 heads, a short workspace."""
    dtype = torch.float16
    c = R.make_case(64, [3, 5], H, KV, dtype, 600)
    kp, vp, k, v = on_device(c)
    q = c.q.to(DEV)
    k_begin, k_len = torch.from_numpy(c.k_begin).to(DEV), torch.from_numpy(c.k_len).to(DEV)
    need = ops.prefix_rows_workspace_elems(c.R, H, D, c.P, c.max_k)
    ws = torch.zeros(need, device=DEV)
    out = torch.full((c.R, H * D), R.GUARD, dtype=dtype, device=DEV)

    def call(heads=H, kv=KV, hd=D, ws_=ws):
        ops.attention_prefix_rows(q, kp, vp, c.P, k, v, out, k_begin, k_len, c.max_k, heads, kv, hd, hd ** -0.5, ws_)

    with pytest.raises(RuntimeError, match="head_dim"):
        call(heads=64, kv=16, hd=64)
    with pytest.raises(RuntimeError, match="4 \\* n_kv_heads"):
        call(heads=32, kv=32)
    with pytest.raises(RuntimeError, match="workspace"):
        call(ws_=ws[:need - 4])
    torch.cuda.synchronize()
    assert bool((out == R.GUARD).all())
    call()
    torch.cuda.synchronize()
    assert not bool((out == R.GUARD).any())
