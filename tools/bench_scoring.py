#!/usr/bin/env python3
"""Cost of scoring (LeopardEngine.score / score_batch, lmi_token_logprobs) on the Llama-3.1-8B geometry with synthetic weights.

    python tools/bench_scoring.py --part kernel|mc|c3 [--out profiles/scoring_<part>.json]

  kernel  lmi_token_logprobs alone on R = 1024 rows of V = 128 256 fp32 logits (525 MB read).
  mc      four-option multiple choice on C2-size requests (1 x 1344x896 + question, each option a 4-token continuation), full depth:
          score_batch of the four requests against prefill_batch of the same four, fast and lo4 schedules, interleaved round by round.
  c3      every row of a C3-length sequence (S = 7187 text tokens: a visual row is never a target under the 4.38 merge) at reduced depth
          (2 + 2 layers): score against prefill(all_logits=True) — time and torch.cuda.max_memory_allocated above the state before the call.
Times are device time between events, the median of --rounds rounds.  Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from leopard_amd.config import full_config  # noqa: E402
from leopard_amd.engine import LeopardEngine  # noqa: E402
from leopard_amd.ops import Ops  # noqa: E402
from leopard_amd.weights import EngineWeights, SynthSource  # noqa: E402
from tools.gen_fulldepth_fixtures import sample_inputs  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--part", choices=["kernel", "mc", "c3"], required=True)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--kernel-iters", type=int, default=100)
ap.add_argument("--out", default="")
args = ap.parse_args()
dev = torch.device("cuda:0")


def timed(fn, n=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def engine(layers=None):
    cfg = full_config()
    if layers:
        cfg.vision_config.num_hidden_layers, cfg.text_config.num_hidden_layers = layers
    ops = Ops()
    return cfg, LeopardEngine(cfg, EngineWeights.build(cfg, SynthSource(cfg, ops, dev, torch.float16), torch.float16), ops=ops, device=dev)


result = {"part": args.part, "geometry": "Llama-3.1-8B + SigLIP (synthetic weights, fp16), vocab 128256"}
if args.part == "kernel":
    ops = Ops()
    R, V = 1024, 128256
    x = torch.randn(R, V, device=dev, generator=torch.Generator(device=dev).manual_seed(0)) * 3
    t = torch.randint(0, V, (R,), device=dev)
    lp, lse = torch.empty(R, device=dev), torch.empty(R, device=dev)
    am = torch.empty(R, dtype=torch.int64, device=dev)
    run = lambda: ops.token_logprobs(x, V, t, lp, lse, am)  # noqa: E731
    run()
    ts = [timed(run, args.kernel_iters) for _ in range(args.rounds)]
    ms = statistics.median(ts)
    result.update(rows=R, vocab=V, bytes_read=R * V * 4, median_us=round(1e3 * ms, 2), min_us=round(1e3 * min(ts), 2),
                  effective_TBps=round(R * V * 4 / (ms * 1e-3) / 1e12, 3))
    print(f"lmi_token_logprobs R={R} V={V}: {1e3 * ms:.1f} us median ({result['effective_TBps']} TB/s)", flush=True)
elif args.part == "mc":
    cfg, eng = engine()
    u8, ids, _ = sample_inputs(cfg, 1, 1344, 896)
    rng = np.random.default_rng(0)
    tiles = torch.from_numpy(u8).to(dev)
    score_reqs, prefill_reqs = [], []
    for k in range(4):
        opt = torch.from_numpy(rng.integers(1000, 100000, (1, 4)))
        full = torch.cat([ids, opt], dim=1)
        lab = torch.cat([torch.full_like(ids, -100), opt], dim=1)
        score_reqs.append((full.to(dev), tiles, lab))
        prefill_reqs.append((full.to(dev), tiles))
    result["requests"] = {"n": 4, "seq_len": int(ids.shape[1] + u8.shape[0] * (cfg.tokens_per_tile - 1) + 4), "scored_rows_per_request": 4}
    for mode in ("fast", "lo4"):
        eng.precision = mode
        res = {"score_batch": [], "prefill_batch": []}
        for r in range(args.rounds + 1):
            a = timed(lambda: eng.score_batch(score_reqs))
            b = timed(lambda: eng.prefill_batch(prefill_reqs))
            if r > 0:
                res["score_batch"].append(a)
                res["prefill_batch"].append(b)
        s, p = statistics.median(res["score_batch"]), statistics.median(res["prefill_batch"])
        result[mode] = {"score_batch_ms": round(s, 3), "prefill_batch_ms": round(p, 3), "overhead_pct": round(100 * (s / p - 1), 2)}
        print(f"[{mode}] 4-option scoring: score_batch {s:.3f} ms vs prefill_batch {p:.3f} ms ({100 * (s / p - 1):+.2f} %)", flush=True)
else:
    cfg, eng = engine((2, 2))
    ids, tiles = torch.from_numpy(np.random.default_rng(6).integers(1000, 100000, (1, 7187))).to(dev), None

    def measure(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        ms = timed(fn)
        return ms, torch.cuda.max_memory_allocated() - base

    eng.prefill(ids, tiles)                                           # warm: workspaces exist before anything is measured
    plain_ms, plain_mem = measure(lambda: eng.prefill(ids, tiles))
    res = {"score": [], "all_logits": []}
    mem = {}
    for r in range(args.rounds + 1):
        for name, fn in (("score", lambda: eng.score(ids, tiles, ids)), ("all_logits", lambda: eng.prefill(ids, tiles, all_logits=True))):
            ms, m = measure(fn)
            mem[name] = max(mem.get(name, 0), m)
            if r > 0:
                res[name].append(ms)
    plain_ms = statistics.median([measure(lambda: eng.prefill(ids, tiles))[0] for _ in range(args.rounds)])
    s, a = statistics.median(res["score"]), statistics.median(res["all_logits"])
    result.update(depth="2 + 2 layers", seq_len=int(ids.shape[1]), scored_rows=int(ids.shape[1]) - 1,
                  score_ms=round(s, 3), all_logits_ms=round(a, 3), plain_prefill_ms=round(plain_ms, 3),
                  score_extra_MiB=round((mem["score"] - plain_mem) / 2**20, 1), all_logits_extra_MiB=round((mem["all_logits"] - plain_mem) / 2**20, 1),
                  plain_prefill_peak_MiB=round(plain_mem / 2**20, 1), score_chunk_rows=eng.score_chunk_rows)
    print(f"C3 length, all rows: score {s:.3f} ms vs all_logits {a:.3f} ms (plain prefill {plain_ms:.3f} ms); extra memory over the plain "
          f"prefill: score {result['score_extra_MiB']} MiB, all_logits {result['all_logits_extra_MiB']} MiB", flush=True)
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
