"""Inputs, references and launch helpers for lmi_attn_decode_shared (decode attention of a batch behind one shared prefix), shared by
tests/test_emu_shared_decode.py (the CPU emulator) and tests/test_gpu_shared_decode.py (the device): every helper takes the Ops object and the
device its tensors live on.  No fixtures, no pytest hooks."""
from types import SimpleNamespace

import torch

D = 128
GUARD = 7.0


def eps(dtype):
    return 2.0 ** -10 if dtype == torch.float16 else 2.0 ** -7          # one rounding of the 16-bit type (tests/test_gpu_kernels.py)


def sync(dev):
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()


def make_case(P, cap_p, lens, cap_o, H, KV, dtype, seed, q_scale=None):
    """q [B, H D]; a prefix K / V of ``cap_p`` rows of which the first P are real — the rest are NaN and must never be seen — with a row stride
    of its own (a [cap, KV D] view of wider rows); a pool of B slots of ``cap_o`` rows, slot s holding lens[s] real rows and NaN behind them.
    ``q_scale``: a per-row factor on q (batch mates whose running maxima move at other tiles)."""
    B = len(lens)
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H * D, generator=g)
    if q_scale is not None:
        q = q * torch.tensor(q_scale, dtype=torch.float32)[:, None]
    q = q.to(dtype)
    pre = torch.randn(cap_p, 2 * KV * D + 8, generator=g).to(dtype)
    pre[P:] = float("nan")
    kp, vp = pre[:, :KV * D], pre[:, KV * D:2 * KV * D]
    pool = torch.randn(B * cap_o, 2 * KV * D, generator=g).to(dtype)
    for s, L in enumerate(lens):
        pool[s * cap_o + L:(s + 1) * cap_o] = float("nan")
    k, v = pool[:, :KV * D], pool[:, KV * D:]
    return SimpleNamespace(q=q, kp=kp, vp=vp, k=k, v=v, P=P, cap_p=cap_p, lens=list(lens), cap_o=cap_o, H=H, KV=KV, B=B, dtype=dtype)


def reference(c, dev="cpu", ftype=torch.float32):
    """Plain attention of every sequence's one query row over the materialised [prefix ; own] keys, every key visible."""
    out = torch.zeros(c.B, c.H * D, dtype=ftype, device=dev)
    q, kp, vp, k, v = (t.to(dev) for t in (c.q, c.kp, c.vp, c.k, c.v))
    for s, L in enumerate(c.lens):
        a = s * c.cap_o
        ks = torch.cat([kp[:c.P], k[a:a + L]]).to(ftype).view(-1, c.KV, D).transpose(0, 1).repeat_interleave(c.H // c.KV, 0)
        vs = torch.cat([vp[:c.P], v[a:a + L]]).to(ftype).view(-1, c.KV, D).transpose(0, 1).repeat_interleave(c.H // c.KV, 0)
        qs = q[s].to(ftype).view(c.H, 1, D)
        out[s] = (torch.softmax(qs @ ks.transpose(-1, -2) * D ** -0.5, -1) @ vs).reshape(-1)
    return out


def run(ops, c, dev="cpu", hl=False, rows=None, device_args=None):
    """One launch over the sequences ``rows`` (default: all) of case ``c``.  Returns the output with a guard row behind it (CPU tensor)."""
    rows = list(range(c.B)) if rows is None else list(rows)
    n = len(rows)
    q = c.q[rows].contiguous().to(dev)
    kp, vp, k, v = (t.to(dev) for t in (c.kp, c.vp, c.k, c.v)) if device_args is None else device_args
    plen = torch.tensor([c.P], dtype=torch.int32).to(dev)
    k_begin = torch.tensor([r * c.cap_o for r in rows], dtype=torch.int32).to(dev)
    k_len = torch.tensor([c.lens[r] for r in rows], dtype=torch.int32).to(dev)
    ws = torch.full((ops.decode_shared_workspace_elems(n, c.H, D, c.cap_p, c.cap_o),), float("nan"), dtype=torch.float32).to(dev)
    out = torch.full(((2 * n if hl else n) + 1, c.H * D), GUARD, dtype=c.dtype).to(dev)
    ops.attention_decode_shared(q, kp, vp, plen, c.cap_p, k, v, out[:-1], k_begin, k_len, c.cap_o, c.H, c.KV, D, D ** -0.5, ws, hl=hl)
    sync(dev)
    return out.cpu()
