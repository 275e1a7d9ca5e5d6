"""LeopardEngine.last_layer_rows (CPU emulator): the last Llama layer of a one-sequence prefill runs q, the attention, o_proj, gate/up and
down_proj only on a trailing 128-aligned row window ("read") — the logits of the last row and every layer's K / V are bit for bit those of
the full layer ("all"), for the fast and the lo4 schedule, at sequence lengths on both sides of the window and query-block edges; runs that
read more than the last row keep the full layer; and the head-subset launches of lmi_rmsnorm_rope(_lo4) (k | v alone, q alone, q alone over
a row window) write exactly the columns and cache rows of the full launch.  Micro model of tests/test_emu_engine.py at hidden 256 (the
fused schedule needs hidden % 256 == 0), text-only prompts (long sequences without the emulated ViT)."""
import numpy as np
import pytest
import torch

from leopard_amd.config import LeopardConfig, RopeScaling, TextConfig, VisionConfig
from leopard_amd.engine import KVCache, LeopardEngine
from leopard_amd.ops import Lo4Act, Lo4Weight
from leopard_amd.weights import EngineWeights, SynthSource, as_packed, rope_permute_rows
from tests.emu_util import emu_ops


def micro_config():
    return LeopardConfig(
        vision_config=VisionConfig(hidden_size=1152, intermediate_size=100, num_hidden_layers=1, num_attention_heads=16, image_size=28, patch_size=14),
        text_config=TextConfig(hidden_size=256, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1,
                               vocab_size=256, rope_scaling=RopeScaling()),
        image_token_index=250)


@pytest.fixture(scope="module")
def setup():
    ops = emu_ops()
    cfg = micro_config()
    W = EngineWeights.build(cfg, SynthSource(cfg, ops, "cpu", torch.float16), torch.float16)
    eng = LeopardEngine(cfg, W, ops=ops, device="cpu")
    assert eng.last_layer_rows == "read"
    yield ops, cfg, eng
    ops.set_option("gemm.config", -1)


def text_ids(S: int, seed: int = 0) -> torch.Tensor:
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 240, (1, S)))          # no image token (250)


class QueryRows:
    """Counts the query rows of every attention launch (both schedules)."""
    def __init__(self, ops):
        self.ops, self.rows = ops, []
        self.inner = {n: getattr(ops, n) for n in ("attention", "attention_lo4")}

    def __enter__(self):
        for n, fn in self.inner.items():
            setattr(self.ops, n, (lambda fn: lambda q, *a, **k: (self.rows.append(q.shape[0]), fn(q, *a, **k))[1])(fn))
        return self

    def __exit__(self, *exc):
        for n in self.inner:
            delattr(self.ops, n)                                 # instance attributes shadowing the methods


def run(eng, ops, cfg, ids, rows_mode):
    S = ids.shape[1]
    eng.last_layer_rows = rows_mode
    cache = KVCache(cfg, S, eng.dtype, "cpu")
    with QueryRows(ops) as qr:
        res = eng.prefill(ids, None, cache=cache)
    assert cache.length == S
    return res.logits_last.clone(), cache, qr.rows


LENGTHS = [100, 128, 129, 255, 256, 257, 383]                    # <= 128; 128 k, 128 k + 1, 128 k + 127 for k = 1, 2


@pytest.mark.parametrize("S", LENGTHS)
@pytest.mark.parametrize("precision", ["fast", "lo4"])
def test_read_rows_equal_all_rows_bit_for_bit(setup, precision, S):
    ops, cfg, eng = setup
    eng.precision = precision
    eng.lo4_rows = 16                                             # the tail of a long production sequence (LO4_TAIL_ROWS), at emulator lengths
    try:
        ids = text_ids(S, seed=S)
        first_needed = S - 1 if precision == "fast" else S - 16
        w0 = first_needed // 128 * 128                            # the window rule, restated
        la, ca, rows_a = run(eng, ops, cfg, ids, "all")
        lr, cr, rows_r = run(eng, ops, cfg, ids, "read")
        assert rows_a == [S, S] and rows_r == [S, S - w0]          # the last layer really ran on the window (whole sequence when w0 == 0)
        assert torch.equal(lr, la)
        for i in range(len(ca.k)):
            assert torch.equal(cr.k[i], ca.k[i]) and torch.equal(cr.v[i], ca.v[i])
            assert bool(ca.k[i][S - 1].abs().sum() > 0)
    finally:
        eng.last_layer_rows, eng.lo4_rows, eng.precision = "read", "auto", "fast"


@pytest.mark.parametrize("precision", ["fast", "lo4"])
def test_sliding_window_attention_through_the_row_window(setup, precision):
    """Mistral's sliding window (Leopard-Idefics2): the window mask follows q + shift, so the trimmed last layer keeps its bits too — with
    a window shorter than the sequence, so that the mask is live for the read rows."""
    ops = setup[0]
    cfg = micro_config()
    cfg.text_config.sliding_window = 100
    W = EngineWeights.build(cfg, SynthSource(cfg, ops, "cpu", torch.float16), torch.float16)
    eng = LeopardEngine(cfg, W, ops=ops, device="cpu")
    eng.precision, eng.lo4_rows = precision, 16
    ids = text_ids(300, seed=9)
    la, ca, rows_a = run(eng, ops, cfg, ids, "all")
    lr, cr, rows_r = run(eng, ops, cfg, ids, "read")
    assert rows_a == [300, 300] and rows_r == [300, 300 - 256] and torch.equal(lr, la)
    assert all(torch.equal(a, b) for a, b in zip(ca.k + ca.v, cr.k + cr.v))
    cfg.text_config.sliding_window = None                          # (read at every launch)
    assert not torch.equal(run(eng, ops, cfg, ids, "read")[0], lr)  # the sliding window really masked keys


def test_lo4_with_every_row_selected_keeps_the_full_layer(setup):
    """lo4_rows 'auto' on a short sequence selects every row: the window would have to hold them all."""
    ops, cfg, eng = setup
    eng.precision = "lo4"
    try:
        ids = text_ids(200, seed=1)
        assert eng.lo4_tail_rows(200) == 200
        la, ca, rows_a = run(eng, ops, cfg, ids, "all")
        lr, cr, rows_r = run(eng, ops, cfg, ids, "read")
        assert rows_a == rows_r == [200, 200] and torch.equal(lr, la)
        assert all(torch.equal(a, b) for a, b in zip(ca.k + ca.v, cr.k + cr.v))
    finally:
        eng.last_layer_rows, eng.precision = "read", "fast"


@pytest.mark.parametrize("precision", ["fast", "lo4"])
def test_runs_that_read_more_than_the_last_row_keep_the_full_layer(setup, precision):
    """all_logits, score and trace runs: every attention launch sees every row under "read", and the results are those of "all"."""
    ops, cfg, eng = setup
    eng.precision = precision
    eng.lo4_rows = 16
    S = 200
    ids = text_ids(S, seed=2)
    labels = ids.clone()
    labels[0, :150] = -100
    out = {}
    try:
        for mode in ("all", "read"):
            eng.last_layer_rows = mode
            with QueryRows(ops) as qr:
                logits_all = eng.prefill(ids, None, all_logits=True).logits_all.clone()
                sc = eng.score(ids, None, labels)
                seen = []
                eng.trace = lambda name, x: seen.append((name, x.clone()))
                traced = eng.prefill(ids, None).logits_last.clone()
                eng.trace = None
            assert qr.rows == [S] * 6
            out[mode] = (logits_all, sc.token_logprobs.clone(), sc.argmax.clone(), traced, seen)
        a, r = out["all"], out["read"]
        assert all(torch.equal(x, y) for x, y in zip(a[:4], r[:4]))
        assert [n for n, _ in a[4]] == [n for n, _ in r[4]] == ["llm.embed", "llm.0", "llm.1"]
        assert all(torch.equal(x, y) for (_, x), (_, y) in zip(a[4], r[4]))
        eng.last_layer_rows = "read"
        with QueryRows(ops) as qr:                                # ... and a packed batch of several sequences does too
            eng.llm_prefill(torch.randn(S + 150, 256, generator=torch.Generator().manual_seed(4)), [S, 150])
        assert qr.rows == [S + 150] * 2
    finally:
        eng.trace = None
        eng.last_layer_rows, eng.lo4_rows, eng.precision = "read", "auto", "fast"


def test_switch_values(setup, monkeypatch):
    ops, cfg, eng = setup
    monkeypatch.setenv("LMI_LAST_LAYER_ROWS", "all")
    assert LeopardEngine(cfg, eng.W, ops=ops, device="cpu", pack_llm_weights=False).last_layer_rows == "all"
    monkeypatch.setenv("LMI_LAST_LAYER_ROWS", "some")
    with pytest.raises(ValueError, match="LMI_LAST_LAYER_ROWS"):
        LeopardEngine(cfg, eng.W, ops=ops, device="cpu", pack_llm_weights=False)


# ---- the head-subset launches -------------------------------------------------------------------------------------------------------------
def rnd(shape, dtype, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype)


def rope_operands(S, nq, nkv, K, dtype):
    D = 128
    wq, wk, wv = rnd((nq * D, K), dtype, 31, 0.1), rnd((nkv * D, K), dtype, 32, 0.1), rnd((nkv * D, K), dtype, 33, 0.1)
    w_rope = torch.cat([rope_permute_rows(torch.cat([wq, wk], 0)), wv], 0).contiguous()
    pos = torch.arange(3000, 3000 + S).float()
    inv = 1.0 / (5e5 ** (torch.arange(0, D, 2).float() / D))
    cos, sin = (pos[:, None] * inv[None]).cos().contiguous(), (pos[:, None] * inv[None]).sin().contiguous()
    sq = rnd((S, K), torch.float32, 34, 2.0).pow(2).view(S, K // 64, 64).sum(-1).contiguous()
    return w_rope, cos, sin, sq


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("gemm_cfg", [-1, 5, 8])
def test_rmsnorm_rope_head_subsets(setup, gemm_cfg, packed):
    """k | v alone and q alone == the columns / cache rows of the full launch at the same M; q alone over a trailing row window (another M,
    another tile geometry under the default dispatch) == those rows."""
    ops = setup[0]
    dtype, S, nq, nkv, D, K, w0 = torch.float16, 300, 2, 1, 128, 256, 128
    qw, kw = nq * D, nkv * D
    w_rope, cos, sin, sq = rope_operands(S, nq, nkv, K, dtype)
    a = rnd((S, K), dtype, 30, 2.0)
    w = as_packed(w_rope) if packed else w_rope
    wq, wkv = LeopardEngine._qkv_weight_parts(w, qw)
    ops.set_option("gemm.config", gemm_cfg)
    try:
        full = torch.full((S, qw + 2 * kw), float("nan"), dtype=dtype)
        kc, vc = torch.zeros(S + 7, kw, dtype=dtype), torch.zeros(S + 7, kw, dtype=dtype)
        ops.rmsnorm_rope(a, w, full, sq, 1e-5, cos, sin, kc, vc, 3, nq, nkv, D)
        part = torch.full_like(full, float("nan"))
        kc2, vc2 = torch.zeros_like(kc), torch.zeros_like(vc)
        ops.rmsnorm_rope(a, wkv, part[:, qw:], sq, 1e-5, cos, sin, kc2, vc2, 3, 0, nkv, D)
        assert torch.equal(part[:, qw:], full[:, qw:]) and torch.equal(kc2, kc) and torch.equal(vc2, vc) and bool(part[:, :qw].isnan().all())
        ops.rmsnorm_rope(a, wq, part[:, :qw], sq, 1e-5, cos, sin, None, None, 0, nq, 0, D)
        assert torch.equal(part, full)
        win = torch.full((S - w0, qw), float("nan"), dtype=dtype)
        ops.rmsnorm_rope(a[w0:], wq, win, sq[w0:], 1e-5, cos[w0:], sin[w0:], None, None, 0, nq, 0, D)
        assert torch.equal(win, full[w0:, :qw])
        with pytest.raises(RuntimeError, match="bad argument"):   # a q-only launch has nothing to append
            ops.rmsnorm_rope(a, wq, part[:, :qw], sq, 1e-5, cos, sin, kc2, vc2, 3, nq, 0, D)
        with pytest.raises(RuntimeError, match="bad argument"):   # ... and no heads at all is no launch
            ops.rmsnorm_rope(a, wq[:0], part[:, :0], sq, 1e-5, cos, sin, None, None, 0, 0, 0, D)
    finally:
        ops.set_option("gemm.config", -1)


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("gemm_cfg", [-1, 5, 8])
def test_rmsnorm_rope_lo4_head_subsets_with_a_row_selection(setup, gemm_cfg, packed):
    """The same with the correction phase and a row selection: rows 280.. carry images.  The window [128, 300) holds an unselected 64-row
    block (128..191: its tile skips the fp4 k-tiles in the 64-row geometry) and the selected ones; the sliced weight image / scales, row_sel,
    unit_sel and the shifted sel_ranges give the bits of the full launch."""
    ops = setup[0]
    dtype, S, nq, nkv, D, K, w0 = torch.float16, 300, 2, 1, 128, 256, 128
    qw, kw = nq * D, nkv * D
    w_rope, cos, sin, sq = rope_operands(S, nq, nkv, K, dtype)
    w4 = ops.quantize_w4(w_rope)
    w = as_packed(w_rope) if packed else w_rope
    wq, wkv = LeopardEngine._qkv_weight_parts(w, qw)
    q4, kv4 = Lo4Weight(w4.img[:qw], w4.sc[:qw]), Lo4Weight(w4.img[qw:], w4.sc[qw:])
    row = np.zeros(S, dtype=np.uint8)
    row[280:] = 1
    unit = np.zeros((S + 63) // 64 * 64, dtype=np.uint8)
    unit[:S] = row
    sel = (torch.from_numpy(row), torch.from_numpy(unit.reshape(-1, 64).max(axis=1)), np.array([[280, S]], dtype=np.int32))
    assert sel[1].tolist() == [0, 0, 0, 0, 1]
    act = Lo4Act.empty(S, K, dtype, "cpu", sel=sel)
    ops.split_lo4(rnd((S, K), torch.float32, 30, 2.0), act)
    act.img[:280] = 0                                             # the contract of a selected pass: unselected rows carry zero images
    act.sc[:280] = 0
    ops.set_option("gemm.config", gemm_cfg)
    try:
        full = torch.full((S, qw + 2 * kw), float("nan"), dtype=dtype)
        kc, vc = torch.zeros(S + 7, kw, dtype=dtype), torch.zeros(S + 7, kw, dtype=dtype)
        ops.rmsnorm_rope_lo4(act, w, w4, full, sq, 1e-5, cos, sin, kc, vc, 3, nq, nkv, D)
        fast = torch.empty_like(full)
        ops.rmsnorm_rope(act.hi, w, fast, sq, 1e-5, cos, sin, None, None, 0, nq, nkv, D)
        assert torch.equal(full[:280], fast[:280]) and not torch.equal(full[280:], fast[280:])      # the selection is live
        part = torch.full_like(full, float("nan"))
        kc2, vc2 = torch.zeros_like(kc), torch.zeros_like(vc)
        ops.rmsnorm_rope_lo4(act, wkv, kv4, part[:, qw:], sq, 1e-5, cos, sin, kc2, vc2, 3, 0, nkv, D)
        assert torch.equal(part[:, qw:], full[:, qw:]) and torch.equal(kc2, kc) and torch.equal(vc2, vc)
        ops.rmsnorm_rope_lo4(act, wq, q4, part[:, :qw], sq, 1e-5, cos, sin, None, None, 0, nq, 0, D)
        assert torch.equal(part, full)
        wsel = (sel[0][w0:], sel[1][w0 // 64:], np.ascontiguousarray(sel[2] - w0))
        win = torch.full((S - w0, qw), float("nan"), dtype=dtype)
        ops.rmsnorm_rope_lo4(act.rows_from(w0, wsel), wq, q4, win, sq[w0:], 1e-5, cos[w0:], sin[w0:], None, None, 0, nq, 0, D)
        assert torch.equal(win, full[w0:, :qw])
    finally:
        ops.set_option("gemm.config", -1)
