"""Test helper: the fixed inputs of tests/golden/token_logprobs_bits.npz — rows of fp32 logits made by integer arithmetic only, so that every
machine builds the same bits — and the call that turns them into (logprob, lse, argmax)."""
import numpy as np
import torch

CASES = {"v128256": (6, 128256, 128256 + 128, None), "v1001": (5, 1001, 1008, [3, 0, 4, 3, 1])}


def case_inputs(name):
    """(logits [R, ld] fp32 with 1e30 in the padding, vocab, targets int64 [n], rows int64 [n] or None)."""
    R, V, ld, rows = CASES[name]
    i = np.arange(R * V, dtype=np.uint64)
    h = (i * np.uint64(2654435761) + (i >> np.uint64(7)) * np.uint64(40503) + np.uint64(12345)) & np.uint64(0xFFFFFF)
    x = np.full((R, ld), 1e30, dtype=np.float32)
    x[:, :V] = (h.astype(np.float32) * np.float32(2.0 ** -20) - np.float32(8.0)).reshape(R, V)      # exact: 24-bit integers scaled by a power of two
    x[1, [5, V - 3, 77]] = np.float32(9.5)                                                           # tied maxima
    n = R if rows is None else len(rows)
    targets = (np.arange(n, dtype=np.int64) * 7919 + 3) % V
    return (torch.from_numpy(x), V, torch.from_numpy(targets), None if rows is None else torch.tensor(rows, dtype=torch.int64))


def run_case(ops, name, device="cpu"):
    """{key: numpy array} of the case's outputs, floats as their int32 bit patterns."""
    x, V, t, rows = case_inputs(name)
    n = t.numel()
    x, t = x.to(device), t.to(device)
    rows = None if rows is None else rows.to(device)
    lp, lse = torch.empty(n, device=device), torch.empty(n, device=device)
    am = torch.empty(n, dtype=torch.int64, device=device)
    ops.token_logprobs(x, V, t, lp, lse, am, rows=rows)
    if device != "cpu":
        torch.cuda.synchronize()
    return {f"{name}_logprob": lp.cpu().view(torch.int32).numpy(), f"{name}_lse": lse.cpu().view(torch.int32).numpy(),
            f"{name}_argmax": am.cpu().numpy()}
