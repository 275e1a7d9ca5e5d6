"""Inputs, references and launch helpers for lmi_attn_prefix_rows (row-packed two-range attention: R packed query rows behind one cached
prefix, row r seeing the pooled own rows k_begin[r] .. k_begin[r] + k_len[r])), shared by tests/test_emu_prefix_rows.py (the CPU emulator) and
tests/test_gpu_prefix_rows.py (the device): every helper takes the Ops object and the device its tensors live on.  No fixtures, no pytest hooks."""
from types import SimpleNamespace

import numpy as np
import torch

D = 128
GUARD = 7.0
SPARE = 3                                                      # NaN rows behind the prefix and behind every suffix's own rows


def eps(dtype):
    return 2.0 ** -10 if dtype == torch.float16 else 2.0 ** -7          # one rounding of the 16-bit type (tests/test_gpu_kernels.py)


def sync(dev):
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()


def make_case(P, lens, H, KV, dtype, seed, q_scale=None):
    """R = sum(lens) query rows q [R, H D]: row i of suffix j sees the prefix and the own rows begin[j] .. begin[j] + i (causality as a key
    count).  The prefix K / V have a row stride of their own and SPARE NaN rows behind row P; the pool holds every suffix's rows followed by
    SPARE NaN rows — rows outside every range, which must never be seen.  ``q_scale``: a per-row factor on q."""
    R = sum(lens)
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(R, H * D, generator=g)
    if q_scale is not None:
        q = q * torch.tensor(q_scale, dtype=torch.float32)[:, None]
    q = q.to(dtype)
    pre = torch.randn(P + SPARE, 2 * KV * D + 8, generator=g).to(dtype)
    pre[P:] = float("nan")
    kp, vp = pre[:, :KV * D], pre[:, KV * D:2 * KV * D]
    begin = [int(b) for b in np.cumsum([0] + [l + SPARE for l in lens[:-1]])]
    pool = torch.randn(sum(lens) + SPARE * len(lens), 2 * KV * D, generator=g).to(dtype)
    for b, l in zip(begin, lens):
        pool[b + l:b + l + SPARE] = float("nan")
    k, v = pool[:, :KV * D], pool[:, KV * D:]
    k_begin = np.concatenate([np.full(l, b, dtype=np.int32) for l, b in zip(lens, begin)])
    k_len = np.concatenate([np.arange(1, l + 1, dtype=np.int32) for l in lens])
    return SimpleNamespace(q=q, kp=kp, vp=vp, k=k, v=v, P=P, lens=list(lens), begin=begin, k_begin=k_begin, k_len=k_len, R=R, H=H, KV=KV,
                           dtype=dtype, max_k=max(lens))


def reference(c, dev="cpu", ftype=torch.float32, rows=None):
    """Plain attention of every query row over its materialised [prefix ; own] keys, every key visible."""
    rows = list(range(c.R)) if rows is None else list(rows)
    out = torch.zeros(len(rows), c.H * D, dtype=ftype, device=dev)
    q, kp, vp, k, v = (t.to(dev) for t in (c.q, c.kp, c.vp, c.k, c.v))
    kpf = kp[:c.P].to(ftype).view(-1, c.KV, D).transpose(0, 1).repeat_interleave(c.H // c.KV, 0)
    vpf = vp[:c.P].to(ftype).view(-1, c.KV, D).transpose(0, 1).repeat_interleave(c.H // c.KV, 0)
    for n, r in enumerate(rows):
        a, L = int(c.k_begin[r]), int(c.k_len[r])
        ks = torch.cat([kpf, k[a:a + L].to(ftype).view(-1, c.KV, D).transpose(0, 1).repeat_interleave(c.H // c.KV, 0)], dim=1)
        vs = torch.cat([vpf, v[a:a + L].to(ftype).view(-1, c.KV, D).transpose(0, 1).repeat_interleave(c.H // c.KV, 0)], dim=1)
        qs = q[r].to(ftype).view(c.H, 1, D)
        out[n] = (torch.softmax(qs @ ks.transpose(-1, -2) * D ** -0.5, -1) @ vs).reshape(-1)
    return out


def run(ops, c, dev="cpu", rows=None, f32=False, device_args=None):
    """One launch over the query rows ``rows`` (default: all) of case ``c``.  Returns the T output with a guard row behind it (CPU tensor) and,
    ``f32``: also the fp32 rows with their guard row."""
    rows = list(range(c.R)) if rows is None else list(rows)
    n = len(rows)
    q = c.q[rows].contiguous().to(dev)
    kp, vp, k, v = (t.to(dev) for t in (c.kp, c.vp, c.k, c.v)) if device_args is None else device_args
    k_begin = torch.from_numpy(c.k_begin[rows]).to(dev)
    k_len = torch.from_numpy(c.k_len[rows]).to(dev)
    ws = torch.full((ops.prefix_rows_workspace_elems(n, c.H, D, c.P, c.max_k),), float("nan"), dtype=torch.float32).to(dev)
    out = torch.full((n + 1, c.H * D), GUARD, dtype=c.dtype).to(dev)
    o32 = torch.full((n + 1, c.H * D), GUARD, dtype=torch.float32).to(dev) if f32 else None
    ops.attention_prefix_rows(q, kp, vp, c.P, k, v, out[:-1], k_begin, k_len, c.max_k, c.H, c.KV, D, D ** -0.5, ws, out_f32=None if o32 is None else o32[:-1])
    sync(dev)
    return (out.cpu(), o32.cpu()) if f32 else out.cpu()
