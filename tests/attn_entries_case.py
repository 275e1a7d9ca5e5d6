"""Test helper: the fixed calls behind tests/golden/attn_entries_emu_bits.json — every attention entry of the library through ``Ops`` at the smallest
shapes at which a host decision flips (split geometry, GQA packing, own-pass instantiation, kernel choice, output kind), in f16 and bf16.  Inputs are made
by integer arithmetic only, so every machine builds the same bits; ``run_all`` returns a SHA-256 per output tensor."""
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


def decode(ops, dt, dev, q_lens, k_lens, H=4, KV=1, window=0, pooled=False, hl=False, D=128):
    """attention_decode (packed sequences) or attention_decode_pool (slots of one pooled cache, one query row each)."""
    n, tq, max_k = len(q_lens), sum(q_lens), max(k_lens)
    q = _rows(tq, H * D, dt, dev, 1)
    out = torch.zeros(2 * tq if hl else tq, H * D, dtype=dt, device=dev)
    if pooled:
        stride = max_k + 3                                           # slot s owns rows [s * stride, s * stride + k_len[s])
        k, v = _rows(n * stride, KV * D, dt, dev, 2), _rows(n * stride, KV * D, dt, dev, 3)
        ws = torch.zeros(ops.decode_workspace_elems(tq, H, D, max_k), device=dev)
        ops.attention_decode_pool(q, k, v, out, _cu(q_lens, dev), _i32([s * stride for s in range(n)], dev), _i32(k_lens, dev), max_k, H, KV, D,
                                  D ** -0.5, ws, window=window, hl=hl)
    else:
        k, v = _rows(sum(k_lens), KV * D, dt, dev, 2), _rows(sum(k_lens), KV * D, dt, dev, 3)
        ws = torch.zeros(ops.decode_workspace_elems(tq, H, D, max_k), device=dev)
        ops.attention_decode(q, k, v, out, _cu(q_lens, dev), _cu(k_lens, dev), max(q_lens), max_k, H, KV, D, D ** -0.5, ws, window=window, hl=hl)
    return {"out": out}


def shared(ops, dt, dev, k_lens, max_prefix, prefix=None, max_k=None, H=4, KV=1, hl=False, D=128):
    """attention_decode_shared: sequence s = row s of q, behind ``prefix`` (device) <= max_prefix shared rows."""
    n, max_k = len(k_lens), max(k_lens) if max_k is None else max_k
    stride = max_k + 3
    q = _rows(n, H * D, dt, dev, 1)
    kp, vp = _rows(max_prefix, KV * D, dt, dev, 4), _rows(max_prefix, KV * D, dt, dev, 5)
    k, v = _rows(n * stride, KV * D, dt, dev, 2), _rows(n * stride, KV * D, dt, dev, 3)
    out = torch.zeros(2 * n if hl else n, H * D, dtype=dt, device=dev)
    ws = torch.zeros(ops.decode_shared_workspace_elems(n, H, D, max_prefix, max_k), device=dev)
    ops.attention_decode_shared(q, kp, vp, _i32([max_prefix if prefix is None else prefix], dev), max_prefix, k, v, out,
                                _i32([s * stride for s in range(n)], dev), _i32(k_lens, dev), max_k, H, KV, D, D ** -0.5, ws, hl=hl)
    return {"out": out}


def prefix_rows(ops, dt, dev, k_lens, prefix, f32=False, H=4, KV=1, D=128):
    """attention_prefix_rows: row r sees the prefix and k_len[r] pooled rows from k_begin[r] (overlapping ranges, as a continuation's rows have)."""
    n, max_k = len(k_lens), max(max(k_lens), 1)
    q = _rows(n, H * D, dt, dev, 1)
    kp, vp = _rows(prefix, KV * D, dt, dev, 4), _rows(prefix, KV * D, dt, dev, 5)
    k, v = _rows(2 * n + max_k, KV * D, dt, dev, 2), _rows(2 * n + max_k, KV * D, dt, dev, 3)
    out = torch.zeros(n, H * D, dtype=dt, device=dev)
    out32 = torch.zeros(n, H * D, device=dev) if f32 else None
    ws = torch.zeros(ops.prefix_rows_workspace_elems(n, H, D, prefix, max_k), device=dev)
    ops.attention_prefix_rows(q, kp, vp, prefix, k, v, out, _i32([2 * r for r in range(n)], dev), _i32(k_lens, dev), max_k, H, KV, D, D ** -0.5, ws,
                              out_f32=out32)
    return {"out": out, "out_f32": out32} if f32 else {"out": out}


def _lo4_act(rows, H, D, dt, dev, sel):
    if sel is not None:
        row_sel = torch.tensor([1 if sel(r) else 0 for r in range(rows)], dtype=torch.uint8)
        unit_sel = torch.tensor([int(row_sel[u * 64:(u + 1) * 64].any()) for u in range((rows + 63) // 64)], dtype=torch.uint8)
        sel = (row_sel.to(dev), unit_sel.to(dev))
    act = Lo4Act.empty(rows, H * D, dt, dev, k4=lo4_head_k4(H, D), sel=sel)
    act.hi.zero_(), act.img.zero_(), act.sc.zero_()
    return act


def varlen(ops, dt, dev, q_lens, k_lens=None, D=128, H=4, KV=1, causal=True, window=0, kind="out", sel=None):
    """The varlen forward: self-attention (cu_k is cu_q) or, with k_lens, keys of their own; kind = out | f32 | fp8 | lo4."""
    tq, tk = sum(q_lens), sum(q_lens if k_lens is None else k_lens)
    q, k, v = _rows(tq, H * D, dt, dev, 1), _rows(tk, KV * D, dt, dev, 2), _rows(tk, KV * D, dt, dev, 3)
    cu_q = _cu(q_lens, dev)
    cu_k = cu_q if k_lens is None else _cu(k_lens, dev)
    args = (cu_q, cu_k, max(q_lens), H, KV, D, D ** -0.5, causal)
    if kind == "f32":
        return {"out_f32": ops.attention_f32out(q, k, v, torch.zeros(tq, H * D, device=dev), *args, window=window)}
    if kind == "fp8":
        return {"out_fp8": ops.attention_fp8out(q, k, v, torch.zeros(tq, H * D, dtype=torch.uint8, device=dev), 16.0, *args, window=window)}
    if kind == "lo4":
        act = ops.attention_lo4(q, k, v, _lo4_act(tq, H, D, dt, dev, sel), *args, window=window)
        return {"out": act.hi, "img": act.img, "scales": act.sc}
    return {"out": ops.attention(q, k, v, torch.zeros(tq, H * D, dtype=dt, device=dev), *args, window=window)}


def prefix_fwd(ops, dt, dev, q_lens, prefix, sel=None, lo4=False, H=4, KV=1, D=128):
    tq = sum(q_lens)
    q, k, v = _rows(tq, H * D, dt, dev, 1), _rows(tq, KV * D, dt, dev, 2), _rows(tq, KV * D, dt, dev, 3)
    kp, vp = _rows(prefix, KV * D, dt, dev, 4), _rows(prefix, KV * D, dt, dev, 5)
    if lo4:
        act = ops.attention_prefix_lo4(q, k, v, kp, vp, prefix, _lo4_act(tq, H, D, dt, dev, sel), _cu(q_lens, dev), max(q_lens), H, KV, D, D ** -0.5)
        return {"out": act.hi, "img": act.img, "scales": act.sc}
    return {"out": ops.attention_prefix(q, k, v, kp, vp, prefix, torch.zeros(tq, H * D, dtype=dt, device=dev), _cu(q_lens, dev), max(q_lens), H, KV, D,
                                        D ** -0.5)}


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


def run_case(ops, name, dtype, device="cpu"):
    """{output name: sha256 hex of the tensor's bytes} of one case in one dtype."""
    fn, kw, options = CASES[name]
    with contextlib.ExitStack() as stack:
        for key, value in options.items():
            stack.enter_context(_option(ops, key, value))
        outs = fn(ops, DTYPES[dtype], device, **kw)
        if device != "cpu":
            torch.cuda.synchronize()
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
