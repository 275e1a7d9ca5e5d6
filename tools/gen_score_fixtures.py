#!/usr/bin/env python3
"""Full-depth oracle fixture of SCORING (test infrastructure; HOST cores, no GPU).

    python tools/gen_score_fixtures.py [--out tests/golden/score_c2_full_depth.npz]

One C2 sample (1 x 1344x896 -> 7 ViT inputs, S = 1242: longer than LeopardEngine.LO4_FULL_BELOW, so the row-selective lo4 policy applies)
followed by a 24-token continuation.  Labels (ignore index -100 elsewhere): the continuation, and the last INTERIOR text tokens of the prompt,
whose predicting rows sit more than 16 rows before the end (outside the lo4 tail selection).  The fp32 CPU oracle runs the whole sequence at
FULL depth (27 + 32 layers, ``llama_forward(..., last_only=False)``); the 4.38 merge with labels and the reference shift (EVAL:333-348) give
the scored rows, and float64 arithmetic on the oracle's fp32 logits gives, per scored row: target, logprob, lse, argmax and the top-2 logits
(their margin), plus max|logit| of the row.  Inputs are regenerated from their seeds by tests/test_gpu_scoring.py and checked against the
SHA-256s stored here."""
from __future__ import annotations

import argparse
import hashlib
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from leopard_amd.config import full_config  # noqa: E402
from tools.gen_fulldepth_fixtures import host_weights, sample_inputs  # noqa: E402

N_CONT = 24            # appended continuation tokens
N_INTERIOR = 20        # labelled prompt text tokens (> 16 rows before the end)


def score_request(cfg, seed: int = 0):
    """(u8 tiles, ids [1, S_in], labels [1, S_in]) of the fixture: C2 sample + continuation; the labels as described above."""
    u8, ids, _ = sample_inputs(cfg, 1, 1344, 896, seed=seed)
    rng = np.random.default_rng(1000 + seed)
    cont = torch.from_numpy(rng.integers(1000, 100000, N_CONT)).reshape(1, -1)
    full = torch.cat([ids, cont], dim=1)
    labels = torch.full_like(full, -100)
    labels[0, ids.shape[1]:] = cont[0]
    text = np.nonzero(ids[0].numpy() != cfg.image_token_index)[0]
    interior = text[text > 0][-N_INTERIOR:]
    labels[0, interior] = full[0, interior]
    return u8, full, labels


def merged_targets(ids: np.ndarray, labels: np.ndarray, image_token_index: int, tokens_per_tile: int):
    """transformers-4.38 merge with labels (visual rows -100, text labels scattered to their merged rows) + the shift of EVAL:337-343:
    merged row s predicts merged label s + 1.  Returns (rows, targets) of the non-ignored targets."""
    is_img = ids == image_token_index
    width = np.where(is_img, tokens_per_tile, 1)
    start = np.cumsum(width) - width
    merged = np.full(int(width.sum()), -100, dtype=np.int64)
    merged[start[~is_img]] = labels[~is_img]
    tgt = merged[1:]
    rows = np.nonzero(tgt != -100)[0]
    return rows.astype(np.int64), tgt[rows].astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "score_c2_full_depth.npz"))
    ap.add_argument("--threads", type=int, default=os.cpu_count() or 8)
    args = ap.parse_args()
    torch.set_num_threads(args.threads)
    from leopard_amd.tiler import siglip_normalize
    from oracle import leopard_oracle as O
    cfg = full_config()
    W = host_weights(cfg, args.threads)
    u8, ids, labels = score_request(cfg)
    rows, targets = merged_targets(ids[0].numpy(), labels[0].numpy(), cfg.image_token_index, cfg.tokens_per_tile)
    t0 = time.perf_counter()
    with torch.no_grad():
        feats = O.projector(O.siglip_vision_tower(torch.from_numpy(siglip_normalize(u8)), W, cfg), W)
        emb, _, pos = O.embed_and_merge(ids, feats, W, cfg)
        logits = O.llama_forward(emb, pos, W, cfg, last_only=False)[0]
    secs = time.perf_counter() - t0
    S = logits.shape[0]
    sel = logits[torch.from_numpy(rows)].double()
    lse = torch.logsumexp(sel, dim=-1)
    lp = sel.gather(1, torch.from_numpy(targets).reshape(-1, 1))[:, 0] - lse
    top2 = sel.topk(2, dim=-1).values
    am = sel.argmax(dim=-1)
    print(f"fp32 oracle: S = {S}, {secs:.0f} s on {args.threads} threads; {len(rows)} scored rows ({int((rows < S - 16).sum())} outside the "
          f"last 16); mean -logprob {float(-lp.mean()):.4f}; max|logit| {float(sel.abs().max()):.3f}", flush=True)
    out = {
        "ids": ids.numpy(), "labels": labels.numpy(), "seq_len": np.asarray([S]),
        "tiles_sha256": np.frombuffer(hashlib.sha256(np.ascontiguousarray(u8).tobytes()).digest(), dtype=np.uint8),
        "ids_sha256": np.frombuffer(hashlib.sha256(np.ascontiguousarray(ids.numpy()).tobytes()).digest(), dtype=np.uint8),
        "rows": rows, "targets": targets,
        "logprob": lp.numpy(), "lse": lse.numpy(), "argmax": am.numpy().astype(np.int64), "top2": top2.numpy(),
        "row_max_abs_logit": sel.abs().amax(dim=-1).numpy(), "max_abs_logit": np.asarray([float(sel.abs().max())]),
        "oracle_seconds": np.asarray([secs]), "oracle_threads": np.asarray([args.threads]),
    }
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out} ({os.path.getsize(args.out) / 1e3:.1f} kB)", flush=True)


if __name__ == "__main__":
    main()
