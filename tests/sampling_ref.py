"""Test helper: the float64 restatement of lmi_decode_sample's kept set (leopard_amd/csrc/sample.h) and a kernel driver that
collects many draws.  Shared by tests/test_emu_sampling.py (emulator) and tests/test_gpu_sampling.py (MI355X)."""
import math

import numpy as np
import torch


def kept_set(row: torch.Tensor, vocab: int, T: float, top_k: int, top_p: float, suppress=()) -> list:
    """Indices that can be drawn, in the kernel's order (scaled logit descending, lower index first on ties)."""
    s32 = (row[:vocab].float().cpu() / torch.tensor(T, dtype=torch.float32))           # the kernel's fp32 division
    s = s32.double().numpy()
    allowed = np.isfinite(s) | (s == np.inf)
    allowed &= ~np.isneginf(s)
    for j in suppress:
        allowed[int(j)] = False
    idx = np.nonzero(allowed)[0]
    order = idx[np.lexsort((idx, -s[idx]))]
    if top_k > 0:
        order = order[:top_k]
    top_p = float(np.float32(top_p))                                    # the kernel's parameter is fp32
    if top_p < 1.0 and len(order):
        w = np.exp(s[order] - s[order[0]])
        cum = np.cumsum(w)
        L = int(np.searchsorted(cum, top_p * cum[-1] * (1 - 1e-12), side="left")) + 1
        order = order[:max(1, min(L, len(order)))]
    return [int(i) for i in order]


def kept_probs(row: torch.Tensor, kept: list, T: float) -> np.ndarray:
    s = (row[kept].float().cpu() / torch.tensor(T, dtype=torch.float32)).double().numpy()
    w = np.exp(s - s.max())
    return w / w.sum()


def draw_many(ops, row: torch.Tensor, vocab: int, T: float, top_k: int, top_p: float, n_rows: int, n_steps: int, seed0: int = 1,
              suppress=None) -> np.ndarray:
    """n_rows x n_steps draws from one logits row: n_rows copies in one launch (seeds seed0..), the kernel advancing step itself."""
    dev = row.device
    logits = row.reshape(1, -1).expand(n_rows, -1).contiguous()
    temp = torch.full((n_rows,), float(T), dtype=torch.float32, device=dev)
    k = torch.full((n_rows,), int(top_k), dtype=torch.int32, device=dev)
    p = torch.full((n_rows,), float(top_p), dtype=torch.float32, device=dev)
    seed = torch.arange(seed0, seed0 + n_rows, dtype=torch.int64, device=dev)
    step = torch.zeros(n_rows, dtype=torch.int32, device=dev)
    tok = torch.zeros(n_rows, dtype=torch.int64, device=dev)
    pos = torch.zeros(n_rows, dtype=torch.int32, device=dev)
    out = []
    for _ in range(n_steps):
        ops.decode_sample(logits, vocab, temp, k, p, seed, step, tok, pos, suppress=suppress)
        out.append(tok.cpu().numpy().copy())
    return np.concatenate(out)


def chi2_ok(draws: np.ndarray, kept: list, probs: np.ndarray, z: float = 3.09) -> tuple:
    """Pearson chi-square of the draws against probs (kept tokens; expected counts < 5 pooled into one cell), compared with the upper
    0.1 % point of chi2(df) (Wilson-Hilferty; z = 3.09).  Returns (ok, statistic, critical value)."""
    n = len(draws)
    counts = np.array([(draws == t).sum() for t in kept], dtype=np.float64)
    exp_ = probs * n
    big = exp_ >= 5
    obs_c, exp_c = list(counts[big]), list(exp_[big])
    if (~big).any():
        obs_c.append(counts[~big].sum()); exp_c.append(exp_[~big].sum())
    obs_c, exp_c = np.array(obs_c), np.array(exp_c)
    stat = float(((obs_c - exp_c) ** 2 / exp_c).sum())
    df = max(len(obs_c) - 1, 1)
    crit = df * (1 - 2 / (9 * df) + z * math.sqrt(2 / (9 * df))) ** 3
    return stat <= crit, stat, crit
