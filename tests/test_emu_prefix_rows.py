"""Row-packed two-range attention on the CPU emulator build: lmi_attn_prefix_rows (R packed query rows behind one cached prefix; the prefix
pass of lmi_attn_decode_shared with more than one 32-row block, the pooled own pass with a key range per ROW, one merge that can also hand over
fp32 rows) against plain fp32 attention over the materialised keys.  The emulator's LDS-DMA asynchrony model (tests/test_hipemu_dma_model.py)
is on for every launch here — an under-counted wait shows as NaNs.  The file also passes under HIPEMU_ORDER=reverse."""
import os

import pytest
import torch

from tests import prefix_rows_ref as R
from tests.emu_util import emu_ops

D = R.D
H, KV = 4, 1
SUFFIXES = [[1, 2, 33], [64, 5]]                               # R = 36 and 69: the row-tile edges 32 / 33 and 64 / 65


@pytest.fixture(scope="module")
def ops():
    assert "HIPEMU_SYNC_DMA" not in os.environ, "the LDS-DMA asynchrony model must be on (unset HIPEMU_SYNC_DMA)"
    return emu_ops()


@pytest.mark.parametrize("lens", SUFFIXES)
@pytest.mark.parametrize("P", [1, 63, 64, 65, 200])
def test_prefix_rows_vs_fp32(ops, P, lens):
    """Within 3 eps of fp32 over the materialised keys (the bound of tests/test_emu_shared_decode.py: the same arithmetic).  Prefix rows >= P
    and pool rows outside every range are NaN: a row read without being masked — or a tile consumed before its pieces landed — is a NaN in
    the output.  The guard row behind the R rows is untouched and two runs agree bit for bit."""
    dtype = torch.float16
    c = R.make_case(P, lens, H, KV, dtype, 2000 + 13 * P + len(lens))
    out = R.run(ops, c)
    assert bool((out[c.R] == R.GUARD).all())
    got = out[:c.R].float()
    assert not torch.isnan(got).any()
    err = (got - R.reference(c)).abs().max().item()
    print(f"P={P} lens={lens} R={c.R}: max abs err {err:.3e} (bound {3 * R.eps(dtype):.3e})")
    assert err <= 3 * R.eps(dtype)
    assert torch.equal(out, R.run(ops, c))


def test_prefix_rows_bf16_and_fp32_rows(ops):
    """bf16 once; the fp32-output launch writes the same T rows and fp32 rows that round to them, guard rows untouched."""
    dtype = torch.bfloat16
    c = R.make_case(65, [64, 5], H, KV, dtype, 41)
    plain = R.run(ops, c)
    out, o32 = R.run(ops, c, f32=True)
    assert torch.equal(out, plain)
    assert bool((o32[c.R] == R.GUARD).all()) and not torch.isnan(o32).any()
    assert torch.equal(o32[:c.R].to(dtype), out[:c.R])
    assert (out[:c.R].float() - R.reference(c)).abs().max() <= 3 * R.eps(dtype)


def test_a_row_does_not_depend_on_its_tile_mates(ops):
    """Row r alone == row r among all others, bit for bit.  57 prefix tiles are more than the prefix pass has splits (56): a workgroup walks
    two tiles and the deferred rescale can fire at the second; odd tiles' K rows are doubled and every other q row is scaled by 8, so a scaled
    row moves its reference where its unscaled tile mates must not (tests/test_emu_shared_decode.py's construction)."""
    dtype, P, lens = torch.float16, 57 * 64 - 20, [1, 2, 33]
    Rn = sum(lens)
    c = R.make_case(P, lens, H, KV, dtype, 77, q_scale=[8.0 if r % 2 == 0 else 1.0 for r in range(Rn)])
    grow = (1 + (torch.arange(P) // 64) % 2).to(torch.float32)[:, None]
    c.kp[:P] = (c.kp[:P].float() * grow).to(dtype)
    batch = R.run(ops, c)
    assert not torch.isnan(batch.float()).any()
    assert (batch[:Rn].float() - R.reference(c)).abs().max() <= 3 * R.eps(dtype)
    for r in (0, 1, 2, 3, 34, 35):                             # both kinds of row, the first and the second row tile
        alone = R.run(ops, c, rows=[r])
        assert torch.equal(alone[0], batch[r]), r


def test_prefix_rows_rejects_bad_arguments_before_any_launch(ops):
    """The limits are LMI_EINVAL (a RuntimeError from Ops), never a trap, and nothing is written."""
    dtype = torch.float16
    c = R.make_case(8, [3, 5], H, KV, dtype, 600)
    k_begin, k_len = torch.from_numpy(c.k_begin), torch.from_numpy(c.k_len)
    ws = torch.zeros(1 << 16)
    out = torch.full((c.R, H * D), R.GUARD, dtype=dtype)

    def call(q=c.q, kp=c.kp, heads=H, kv=KV, hd=D, P=c.P, ws_=ws):
        ops.attention_prefix_rows(q, kp, c.vp, P, c.k, c.v, out, k_begin, k_len, c.max_k, heads, kv, hd, hd ** -0.5, ws_)

    call()                                                         # the arguments the cases below break one at a time are good
    assert not (out == R.GUARD).any()
    out.fill_(R.GUARD)
    with pytest.raises(RuntimeError, match="4 \\* n_kv_heads"):
        call(heads=2, kv=1)
    with pytest.raises(RuntimeError, match="4 \\* n_kv_heads"):
        call(heads=4, kv=4)
    with pytest.raises(RuntimeError, match="head_dim"):
        call(heads=8, kv=2, hd=64)
    with pytest.raises(RuntimeError, match="prefix_len"):
        call(P=0)
    with pytest.raises(RuntimeError, match="strides"):
        wide = torch.zeros(c.P + R.SPARE, KV * D + 4, dtype=dtype)
        call(kp=wide[:, :KV * D])                                  # a row stride that is no multiple of 8
    with pytest.raises(RuntimeError, match="4 GiB"):
        call(P=(1 << 31) // c.kp.stride(0) + 1)
    with pytest.raises(RuntimeError, match="workspace"):
        call(ws_=torch.zeros(ops.prefix_rows_workspace_elems(c.R, H, D, c.P, c.max_k) - 4))
    with pytest.raises(RuntimeError):
        ops.prefix_rows_workspace_elems(c.R, H, D, 0, 5)
    assert bool((out == R.GUARD).all())
