#!/usr/bin/env python3
"""Sampled vs greedy decode on the Llama-3.1-8B geometry (synthetic weights): the captured decode step at B = 1 and B = 16 with its tail
lmi_decode_advance (greedy) or lmi_decode_sample (temperature / top-k / top-p), and the two tail kernels alone on [B, 128256] fp32 rows.
Step times are back-to-back graph replays timed with events (device time per token), greedy and sampled interleaved round by round;
the median round is reported.  Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from leopard_amd.config import full_config  # noqa: E402
from leopard_amd.engine import LeopardEngine, SamplingParams  # noqa: E402
from leopard_amd.ops import Ops  # noqa: E402
from leopard_amd.weights import EngineWeights, SynthSource  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=48, help="replays per timed round")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--kernel-iters", type=int, default=200)
ap.add_argument("--batch", type=int, nargs="*", default=[1, 16])
ap.add_argument("--out", default="")
args = ap.parse_args()
dev = torch.device("cuda:0")
cfg = full_config()
V = cfg.text_config.vocab_size
ops = Ops()
eng = LeopardEngine(cfg, EngineWeights.build(cfg, SynthSource(cfg, ops, dev, torch.float16), torch.float16), ops=ops, device=dev)
HF = SamplingParams(temperature=0.7, top_k=50, top_p=0.9, seed=1)        # a common sampled setting: both filters active


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def step_times(B):
    """(greedy ms, sampled ms) per replay of the B-row step: rounds interleaved, median of each."""
    n_total = args.steps * (args.rounds + 1) * 2 + 16
    if B == 1:
        cache = eng._generation_cache(64 + n_total)
        ids = torch.arange(1, 33, dtype=torch.long).reshape(1, -1).to(dev)
        eng.prefill(ids, None, cache=cache)
        st = eng._decode_state(cache)
        eng._decode_seed(st, cache, 5)
        eng._set_sampling(st, 0, HF)
        run = lambda: eng._decode_run(st, cache)  # noqa: E731
    else:
        st = eng._batch_state(B, 64 + n_total)
        st.tok.fill_(5); st.pos.fill_(32); st.k_len.fill_(33); st.live.fill_(1); st.budget.fill_(1 << 30); st.eos.fill_(-1)
        for j in range(B):
            eng._set_sampling(st, j, HF.for_request(j))
        run = lambda: eng._batch_decode_run(st)  # noqa: E731
    res = {False: [], True: []}
    for r in range(args.rounds + 1):
        for mode in (False, True):
            st.sampling = mode
            if B > 1:
                st.hist_pos.zero_()
            run()                                                             # (captures on first use)
            t = timed(run, args.steps)
            if r > 0:                                                         # round 0: capture + warm-up
                res[mode].append(t)
    st.sampling = False
    return statistics.median(res[False]), statistics.median(res[True])


def kernel_times(B):
    g = torch.Generator(device=dev).manual_seed(0)
    logits = torch.randn(B, V, device=dev, generator=g) * 3
    tok = torch.zeros(B, dtype=torch.int64, device=dev)
    pos = torch.zeros(B, dtype=torch.int32, device=dev)
    k_len = torch.ones(B, dtype=torch.int32, device=dev)
    seed = torch.arange(B, dtype=torch.int64, device=dev)
    step = torch.zeros(B, dtype=torch.int32, device=dev)
    out = {"decode_advance_us": 1e3 * timed(lambda: ops.decode_advance(logits, V, tok, pos, k_len=k_len), args.kernel_iters)}
    for name, (T, k, p) in {"t0.7_k50_p0.9": (0.7, 50, 0.9), "t1_k50": (1.0, 50, 1.0), "t1_p0.9": (1.0, 0, 0.9), "t1_plain": (1.0, 0, 1.0)}.items():
        temp = torch.full((B,), T, device=dev)
        kk = torch.full((B,), k, dtype=torch.int32, device=dev)
        pp = torch.full((B,), p, device=dev)
        out[f"decode_sample_{name}_us"] = 1e3 * timed(lambda: ops.decode_sample(logits, V, temp, kk, pp, seed, step, tok, pos, k_len=k_len),
                                                      args.kernel_iters)
    return out


result = {"geometry": "Llama-3.1-8B (synthetic weights, fp16, fast schedule), vocab %d" % V, "sampling": HF.describe(), "steps": {}, "kernel": {}}
for B in args.batch:
    g, s = step_times(B)
    result["steps"][f"B{B}"] = {"greedy_ms": round(g, 4), "sampled_ms": round(s, 4), "overhead_pct": round(100 * (s / g - 1), 2)}
    print(f"B={B}: greedy step {g:.4f} ms, sampled step {s:.4f} ms ({100 * (s / g - 1):+.2f} %)", flush=True)
for B in args.batch:
    result["kernel"][f"B{B}"] = {k: round(v, 2) for k, v in kernel_times(B).items()}
    print(f"B={B}: kernels (us) {result['kernel'][f'B{B}']}", flush=True)
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
