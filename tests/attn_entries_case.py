"""Test helper: the fixed calls behind tests/golden/attn_entries_emu_bits.json — every attention entry of the library through ``Ops`` at the smallest
shapes at which a host decision flips (split geometry, GQA packing, own-pass instantiation, kernel choice, output kind), in f16 and bf16.  Inputs are made
by integer arithmetic only, so every machine builds the same bits; ``run_all`` returns a SHA-256 per output tensor.

Every case function takes its input tensors (``inp``, default: the ``*_inputs`` function of the same name) and its allocation (``mem``: ``Plain``,
the digest path, or ``Guarded``) from the caller; ``launch`` returns the inputs together with the outputs.  tests/attn_entries_ref.py builds the
value tests on that, over CASES and the value-only EXTRA cases."""
import contextlib
import hashlib

import numpy as np
import torch

from leopard_amd.ops import Lo4Act, lo4_head_k4

DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}


def _vals(n, salt):
    """n fp32 values in [-1, 1), multiples of 2^-9, from an integer hash of the index."""
    i = np.arange(n, dtype=np.uint64) + np.uint64(salt) * np.uint64(1000003)
    h = (i * np.uint64(2654435761) + (i >> np.uint64(7)) * np.uint64(40503) + np.uint64(12345)) & np.uint64(0x3FF)
    return (h.astype(np.float32) - np.float32(512.0)) * np.float32(2.0 ** -9)


def _rows(rows, cols, dt, dev, salt):
    return torch.from_numpy(_vals(rows * cols, salt).reshape(rows, cols)).to(dt).to(dev)


def _i32(xs, dev):
    return torch.tensor(list(xs), dtype=torch.int32, device=dev)


def _cu(lens, dev):
    return _i32(np.concatenate([[0], np.cumsum(lens)]), dev)


@contextlib.contextmanager
def _option(ops, key, value):
    old = ops.get_option(key)
    ops.set_option(key, value)
    try:
        yield
    finally:
        ops.set_option(key, old)


GUARD = 7.0


class Plain:
    """Allocation of the digest path: zeroed outputs and workspaces of exactly the launch's size."""

    def __init__(self, dev):
        self.dev = dev

    def out(self, rows, cols, dtype=torch.float32):
        return torch.zeros(rows, cols, dtype=dtype, device=self.dev)

    def ws(self, n):
        return torch.zeros(n, device=self.dev)


class Guarded(Plain):
    """Allocation of the value-test path: a guard row behind every output tensor (the rows themselves start out zero, as Plain's do: a
    row-selected image keeps its initial bytes) and workspaces filled with NaN."""

    def __init__(self, dev):
        super().__init__(dev)
        self.full = []

    def out(self, rows, cols, dtype=torch.float32):
        t = torch.zeros(rows + 1, cols, dtype=dtype)
        t[rows:] = GUARD
        self.full.append(t.to(self.dev))
        return self.full[-1][:rows]

    def ws(self, n):
        return torch.full((n,), float("nan"), device=self.dev)

    def intact(self):
        return all(bool((t[-1] == GUARD).all()) for t in self.full)


def decode_inputs(dt, dev, q_lens, k_lens, H=4, KV=1, pooled=False, D=128, **_):
    """q rows packed; k / v packed (cu_k) or, pooled, slot s owning rows [s * stride, s * stride + k_len[s]) with stride = max_k + 3."""
    rows = len(q_lens) * (max(k_lens) + 3) if pooled else sum(k_lens)
    return {"q": _rows(sum(q_lens), H * D, dt, dev, 1), "k": _rows(rows, KV * D, dt, dev, 2), "v": _rows(rows, KV * D, dt, dev, 3)}


def decode(ops, dt, dev, q_lens, k_lens, H=4, KV=1, window=0, pooled=False, hl=False, D=128, inp=None, mem=None):
    """attention_decode (packed sequences) or attention_decode_pool (slots of one pooled cache, one query row each)."""
    inp, mem = inp or decode_inputs(dt, dev, q_lens, k_lens, H, KV, pooled, D), mem or Plain(dev)
    n, tq, max_k = len(q_lens), sum(q_lens), max(k_lens)
    q, k, v = inp["q"], inp["k"], inp["v"]
    out = mem.out(2 * tq if hl else tq, H * D, dt)
    ws = mem.ws(ops.decode_workspace_elems(tq, H, D, max_k))
    if pooled:
        stride = max_k + 3                                           # slot s owns rows [s * stride, s * stride + k_len[s])
        ops.attention_decode_pool(q, k, v, out, _cu(q_lens, dev), _i32([s * stride for s in range(n)], dev), _i32(k_lens, dev), max_k, H, KV, D,
                                  D ** -0.5, ws, window=window, hl=hl)
    else:
        ops.attention_decode(q, k, v, out, _cu(q_lens, dev), _cu(k_lens, dev), max(q_lens), max_k, H, KV, D, D ** -0.5, ws, window=window, hl=hl)
    return {"out": out}


def shared_inputs(dt, dev, k_lens, max_prefix, max_k=None, H=4, KV=1, D=128, **_):
    n, max_k = len(k_lens), max(k_lens) if max_k is None else max_k
    return {"q": _rows(n, H * D, dt, dev, 1), "kp": _rows(max_prefix, KV * D, dt, dev, 4), "vp": _rows(max_prefix, KV * D, dt, dev, 5),
            "k": _rows(n * (max_k + 3), KV * D, dt, dev, 2), "v": _rows(n * (max_k + 3), KV * D, dt, dev, 3)}


def shared(ops, dt, dev, k_lens, max_prefix, prefix=None, max_k=None, H=4, KV=1, hl=False, D=128, inp=None, mem=None):
    """attention_decode_shared: sequence s = row s of q, behind ``prefix`` (device) <= max_prefix shared rows."""
    inp, mem = inp or shared_inputs(dt, dev, k_lens, max_prefix, max_k, H, KV, D), mem or Plain(dev)
    n, max_k = len(k_lens), max(k_lens) if max_k is None else max_k
    stride = max_k + 3
    out = mem.out(2 * n if hl else n, H * D, dt)
    ws = mem.ws(ops.decode_shared_workspace_elems(n, H, D, max_prefix, max_k))
    ops.attention_decode_shared(inp["q"], inp["kp"], inp["vp"], _i32([max_prefix if prefix is None else prefix], dev), max_prefix, inp["k"], inp["v"],
                                out, _i32([s * stride for s in range(n)], dev), _i32(k_lens, dev), max_k, H, KV, D, D ** -0.5, ws, hl=hl)
    return {"out": out}


def prefix_rows_inputs(dt, dev, k_lens, prefix, H=4, KV=1, D=128, **_):
    n, max_k = len(k_lens), max(max(k_lens), 1)
    return {"q": _rows(n, H * D, dt, dev, 1), "kp": _rows(prefix, KV * D, dt, dev, 4), "vp": _rows(prefix, KV * D, dt, dev, 5),
            "k": _rows(2 * n + max_k, KV * D, dt, dev, 2), "v": _rows(2 * n + max_k, KV * D, dt, dev, 3)}


def prefix_rows(ops, dt, dev, k_lens, prefix, f32=False, H=4, KV=1, D=128, inp=None, mem=None):
    """attention_prefix_rows: row r sees the prefix and k_len[r] pooled rows from k_begin[r] = 2 r (overlapping ranges, as a continuation's rows have)."""
    inp, mem = inp or prefix_rows_inputs(dt, dev, k_lens, prefix, H, KV, D), mem or Plain(dev)
    n, max_k = len(k_lens), max(max(k_lens), 1)
    out = mem.out(n, H * D, dt)
    out32 = mem.out(n, H * D) if f32 else None
    ws = mem.ws(ops.prefix_rows_workspace_elems(n, H, D, prefix, max_k))
    ops.attention_prefix_rows(inp["q"], inp["kp"], inp["vp"], prefix, inp["k"], inp["v"], out, _i32([2 * r for r in range(n)], dev), _i32(k_lens, dev),
                              max_k, H, KV, D, D ** -0.5, ws, out_f32=out32)
    return {"out": out, "out_f32": out32} if f32 else {"out": out}


def _lo4_act(rows, H, D, dt, dev, sel, mem):
    k4 = lo4_head_k4(H, D)
    act = Lo4Act(mem.out(rows, H * D, dt), mem.out(rows, k4 // 2, torch.uint8), mem.out(rows, k4 // 32, torch.uint8))
    if sel is not None:
        row_sel = torch.tensor([1 if sel(r) else 0 for r in range(rows)], dtype=torch.uint8)
        unit_sel = torch.tensor([int(row_sel[u * 64:(u + 1) * 64].any()) for u in range((rows + 63) // 64)], dtype=torch.uint8)
        act.row_sel, act.unit_sel = row_sel.to(dev), unit_sel.to(dev)
    return act


def varlen_inputs(dt, dev, q_lens, k_lens=None, D=128, H=4, KV=1, **_):
    tq, tk = sum(q_lens), sum(q_lens if k_lens is None else k_lens)
    return {"q": _rows(tq, H * D, dt, dev, 1), "k": _rows(tk, KV * D, dt, dev, 2), "v": _rows(tk, KV * D, dt, dev, 3)}


def varlen(ops, dt, dev, q_lens, k_lens=None, D=128, H=4, KV=1, causal=True, window=0, kind="out", sel=None, inp=None, mem=None):
    """The varlen forward: self-attention (cu_k is cu_q) or, with k_lens, keys of their own; kind = out | f32 | fp8 | lo4."""
    inp, mem = inp or varlen_inputs(dt, dev, q_lens, k_lens, D, H, KV), mem or Plain(dev)
    tq = sum(q_lens)
    q, k, v = inp["q"], inp["k"], inp["v"]
    cu_q = _cu(q_lens, dev)
    cu_k = cu_q if k_lens is None else _cu(k_lens, dev)
    args = (cu_q, cu_k, max(q_lens), H, KV, D, D ** -0.5, causal)
    if kind == "f32":
        return {"out_f32": ops.attention_f32out(q, k, v, mem.out(tq, H * D), *args, window=window)}
    if kind == "fp8":
        return {"out_fp8": ops.attention_fp8out(q, k, v, mem.out(tq, H * D, torch.uint8), 16.0, *args, window=window)}
    if kind == "lo4":
        act = ops.attention_lo4(q, k, v, _lo4_act(tq, H, D, dt, dev, sel, mem), *args, window=window)
        return {"out": act.hi, "img": act.img, "scales": act.sc}
    return {"out": ops.attention(q, k, v, mem.out(tq, H * D, dt), *args, window=window)}


def prefix_fwd_inputs(dt, dev, q_lens, prefix, H=4, KV=1, D=128, **_):
    tq = sum(q_lens)
    return {"q": _rows(tq, H * D, dt, dev, 1), "k": _rows(tq, KV * D, dt, dev, 2), "v": _rows(tq, KV * D, dt, dev, 3),
            "kp": _rows(prefix, KV * D, dt, dev, 4), "vp": _rows(prefix, KV * D, dt, dev, 5)}


def prefix_fwd(ops, dt, dev, q_lens, prefix, sel=None, lo4=False, H=4, KV=1, D=128, inp=None, mem=None):
    inp, mem = inp or prefix_fwd_inputs(dt, dev, q_lens, prefix, H, KV, D), mem or Plain(dev)
    tq = sum(q_lens)
    q, k, v, kp, vp = inp["q"], inp["k"], inp["v"], inp["kp"], inp["vp"]
    if lo4:
        act = ops.attention_prefix_lo4(q, k, v, kp, vp, prefix, _lo4_act(tq, H, D, dt, dev, sel, mem), _cu(q_lens, dev), max(q_lens), H, KV, D, D ** -0.5)
        return {"out": act.hi, "img": act.img, "scales": act.sc}
    return {"out": ops.attention_prefix(q, k, v, kp, vp, prefix, mem.out(tq, H * D, dt), _cu(q_lens, dev), max(q_lens), H, KV, D, D ** -0.5)}


INPUTS = {decode: decode_inputs, shared: shared_inputs, prefix_rows: prefix_rows_inputs, varlen: varlen_inputs, prefix_fwd: prefix_fwd_inputs}


LONG_PREFIX = 57 * 64 - 20          # 57 tiles: more than the 56 splits the prefix pass may take with one kv head, so pre_tiles becomes 2
MIXED32 = [(7 * r) % 40 + 1 for r in range(32)]
ROWS33 = [(5 * r) % 41 for r in range(33)]           # row 0 has no own key

# name -> (function, keyword arguments, {option: value} held during the call)
CASES = {
    # decode: key tiles 1, 1, 2 and 65 (65 tiles: more than 64 splits, split_tiles doubles)
    "decode_k1": (decode, dict(q_lens=[1], k_lens=[1]), {}),
    "decode_k64": (decode, dict(q_lens=[1], k_lens=[64]), {}),
    "decode_k65": (decode, dict(q_lens=[1], k_lens=[65]), {}),
    "decode_k4097": (decode, dict(q_lens=[1], k_lens=[4097]), {}),
    "decode_k65_hl": (decode, dict(q_lens=[1, 1], k_lens=[65, 30], hl=True), {}),
    "decode_split_tiles4": (decode, dict(q_lens=[1, 1], k_lens=[600, 130]), {"attn.decode_split_tiles": 4}),
    "decode_q32_packed": (decode, dict(q_lens=[32, 5], k_lens=[100, 70]), {}),
    "decode_q32_packed_no_stream": (decode, dict(q_lens=[32, 5], k_lens=[100, 70]), {"attn.stream_kv": 0}),
    "decode_q33_unpacked": (decode, dict(q_lens=[33, 5], k_lens=[100, 70]), {}),
    "decode_heads_2_1": (decode, dict(q_lens=[1, 3], k_lens=[65, 130], H=2, KV=1), {}),
    "decode_window": (decode, dict(q_lens=[1, 2], k_lens=[200, 90], window=40), {}),
    "pool_k65": (decode, dict(q_lens=[1, 1, 1], k_lens=[65, 1, 40], pooled=True), {}),
    "pool_k65_hl": (decode, dict(q_lens=[1, 1, 1], k_lens=[65, 1, 40], pooled=True, hl=True), {}),
    "pool_no_stream": (decode, dict(q_lens=[1, 1, 1], k_lens=[65, 1, 40], pooled=True), {"attn.stream_kv": 0}),
    "pool_window": (decode, dict(q_lens=[1, 1], k_lens=[200, 90], pooled=True, window=40), {}),
    # shared-prefix decode: n_seq 1 / 3 / 32, prefix 1 / 64 / 65 / LONG_PREFIX, own range 1 tile and 9 tiles (own_tiles 2)
    "shared_n1_long": (shared, dict(k_lens=[1], max_prefix=LONG_PREFIX), {}),
    "shared_n3_p65_own513": (shared, dict(k_lens=[513, 1, 200], max_prefix=65), {}),
    "shared_n3_p65_own513_hl": (shared, dict(k_lens=[513, 1, 200], max_prefix=65, hl=True), {}),
    "shared_n32_p64": (shared, dict(k_lens=MIXED32, max_prefix=64), {}),
    "shared_n3_p1_hl": (shared, dict(k_lens=[1, 1, 1], max_prefix=1, hl=True), {}),
    "shared_short_device_prefix": (shared, dict(k_lens=[30, 2, 64], max_prefix=200, prefix=130), {}),
    "shared_no_stream": (shared, dict(k_lens=[30, 2, 64], max_prefix=65), {"attn.stream_kv": 0}),
    "shared_heads_8_2": (shared, dict(k_lens=[30, 2, 64], max_prefix=65, H=8, KV=2), {}),
    # row-packed prefix attention: 1, 32 and 33 rows (one and two packed row blocks)
    "rows_n1_long": (prefix_rows, dict(k_lens=[1], prefix=LONG_PREFIX), {}),
    "rows_n32_p65_f32": (prefix_rows, dict(k_lens=[0] + MIXED32[1:], prefix=65, f32=True), {}),
    "rows_n33_p64": (prefix_rows, dict(k_lens=ROWS33, prefix=64), {}),
    "rows_n3_p1_f32": (prefix_rows, dict(k_lens=[0, 1, 64], prefix=1, f32=True), {}),
    "rows_own513": (prefix_rows, dict(k_lens=[513, 0, 77], prefix=65), {}),
    "rows_no_stream": (prefix_rows, dict(k_lens=[513, 0, 77], prefix=65, f32=True), {"attn.stream_kv": 0}),
    # varlen forward
    "varlen_d128_causal_ragged": (varlen, dict(q_lens=[70, 0, 130]), {}),
    "varlen_d128_full_ragged": (varlen, dict(q_lens=[33, 0, 70], causal=False), {}),
    "varlen_d96_full": (varlen, dict(q_lens=[50, 77], D=96, H=2, KV=2, causal=False), {}),
    "varlen_d72_full": (varlen, dict(q_lens=[50, 77], D=72, H=2, KV=2, causal=False), {}),
    "varlen_d72_causal": (varlen, dict(q_lens=[50, 77], D=72, H=2, KV=2), {}),
    "varlen_cross_causal": (varlen, dict(q_lens=[5, 0, 40], k_lens=[40, 0, 100]), {}),
    "varlen_cross_full": (varlen, dict(q_lens=[5, 0, 40], k_lens=[40, 0, 100], causal=False), {}),
    "varlen_window": (varlen, dict(q_lens=[20, 100], window=33), {}),
    "varlen_f32": (varlen, dict(q_lens=[33, 0, 70], kind="f32"), {}),
    "varlen_fp8": (varlen, dict(q_lens=[33, 0, 70], kind="fp8"), {}),
    "varlen_lo4": (varlen, dict(q_lens=[33, 0, 70], kind="lo4"), {}),
    "varlen_lo4_d72": (varlen, dict(q_lens=[50, 77], D=72, H=2, KV=2, causal=False, kind="lo4"), {}),
    "varlen_lo4_row_sel": (varlen, dict(q_lens=[33, 0, 70], kind="lo4", sel=lambda r: r % 3 == 0 and r < 80), {}),
    "varlen_register_staged": (varlen, dict(q_lens=[33, 0, 70]), {"attn.dma": 0}),
    # two-range prefill
    "prefix_fwd_p1": (prefix_fwd, dict(q_lens=[5, 70], prefix=1), {}),
    "prefix_fwd_p65": (prefix_fwd, dict(q_lens=[5, 70], prefix=65), {}),
    "prefix_fwd_p65_two_q_blocks": (prefix_fwd, dict(q_lens=[129, 3], prefix=65), {}),
    "prefix_fwd_lo4_row_sel": (prefix_fwd, dict(q_lens=[5, 70], prefix=65, lo4=True, sel=lambda r: r in (4, 74)), {}),
    "prefix_fwd_lo4_p1": (prefix_fwd, dict(q_lens=[5, 70], prefix=1, lo4=True, sel=lambda r: r >= 64), {}),
}


_R64 = {"attn.rows64_min": 0}
EDGE_LENS = [63, 64, 65, 127, 128, 129, 1]          # one below, at and one above the 64-key tile and the 128-row query block
# Value-only cases (tests/attn_entries_ref.py): never digested, so the golden fixture keeps listing exactly CASES.
EXTRA = {
    "x_varlen_edges_h4_kv1": (varlen, dict(q_lens=EDGE_LENS), {}),
    "x_varlen_edges_h8_kv2": (varlen, dict(q_lens=EDGE_LENS, H=8, KV=2), {}),
    "x_varlen_window1": (varlen, dict(q_lens=[20, 130], window=1), {}),
    "x_varlen_window64": (varlen, dict(q_lens=[20, 130], window=64), {}),
    "x_varlen_window65": (varlen, dict(q_lens=[20, 130], window=65), {}),
    "x_varlen_window_above_all": (varlen, dict(q_lens=[20, 130], window=131), {}),
    "x_varlen_cross_causal_plus1": (varlen, dict(q_lens=[5, 0, 40], k_lens=[6, 0, 41]), {}),
    "x_varlen_cross_causal_plus64": (varlen, dict(q_lens=[5, 0, 40], k_lens=[69, 0, 104]), {}),
    **{f"x_decode_window{w}": (decode, dict(q_lens=[1, 2], k_lens=[200, 90], window=w), {}) for w in (1, 90, 91, 200, 201)},
    **{f"x_pool_window{w}": (decode, dict(q_lens=[1, 1], k_lens=[200, 90], pooled=True, window=w), {}) for w in (1, 90, 91, 200, 201)},
    # the software-pipelined kernels (256-row blocks): one block and a part, a sequence below one block, with and without a window
    **{f"x_rows64_{r}_window{w}": (varlen, dict(q_lens=[300, 40, 70], window=w), dict(_R64, **{"attn.rows64": r})) for r in (1, 2) for w in (0, 33)},
    **{f"x_prefix_fwd_p{p}": (prefix_fwd, dict(q_lens=[1, 128, 129], prefix=p), {}) for p in (63, 64, 65)},
}


def make_inputs(fn, kw, dtype, device="cpu"):
    """The case's own (integer-hash) input tensors: {"q", "k", "v"[, "kp", "vp"]}."""
    return INPUTS[fn](DTYPES[dtype], device, **kw)


def launch(ops, fn, kw, options, dtype, device="cpu", inp=None, mem=None, **more):
    """One launch of a case (``more``: keyword arguments that replace the case's) on the caller's inputs (default: the case's own) with the
    caller's allocation (default: Plain).  Returns (inputs, outputs), the device synchronised."""
    kw = dict(kw, **more)
    inp = make_inputs(fn, kw, dtype, device) if inp is None else inp
    with contextlib.ExitStack() as stack:
        for key, value in options.items():
            stack.enter_context(_option(ops, key, value))
        outs = fn(ops, DTYPES[dtype], device, inp=inp, mem=mem, **kw)
        if device != "cpu":
            torch.cuda.synchronize()
    return inp, outs


def run_case(ops, name, dtype, device="cpu"):
    """{output name: sha256 hex of the tensor's bytes} of one case in one dtype."""
    outs = launch(ops, *CASES[name], dtype, device)[1]
    return {key: hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest() for key, t in outs.items()}


def run_all(ops, device="cpu"):
    return {f"{name}/{dtype}": run_case(ops, name, dtype, device) for name in CASES for dtype in DTYPES}


if __name__ == "__main__":          # python -m tests.attn_entries_case [cuda]: the digests of the library LEOPARD_AMD_LIB names (cpu: an emulator build)
    import json
    import sys

    from leopard_amd import _lib
    from leopard_amd.ops import Ops
    dev = sys.argv[1] if len(sys.argv) > 1 else "cpu"
    json.dump(run_all(Ops(lib=_lib.bind(_lib.LIB_PATH), emulated=dev == "cpu"), dev), sys.stdout, indent=0, sort_keys=True)
