#!/usr/bin/env python3
"""What scoring from a cached prefix saves (LeopardEngine.score_shared / extend_score, lmi_attn_prefix_fwd against lmi_attn_prefix_rows) on the
Llama-3.1-8B + SigLIP geometry with synthetic weights, full depth, fp16, precision lo4: N candidate continuations of the C3 sample
(6 x 1344x896: 7187 merged rows), of 1 and of 8 ids each.

    python tools/score_shared_bench.py --n 1,4,8,16,64 --out profiles/score_shared.json

A run with another --n into the same --out adds its rows to the file (N = 64 spends most of the time in arm 1: it can run as a step of its
own).  On a shared machine run every step under its own time limit and chain them:
    timeout -k 10 900 python tools/score_shared_bench.py --n 1,4,8,16 --out X && timeout -k 10 900 python tools/score_shared_bench.py --n 64 --out X

For every N and continuation length, in ms, the median (and min / max) of --rounds rounds after one warm-up round, the three arms in the same
process, interleaved round by round:
  arm 1  loglikelihood of the N full prompts (N tower passes, N x 7187 LLM rows: the path without this feature, the baseline)
  arm 2  loglikelihood_shared, attention="ranges" (lmi_attn_prefix_fwd: one workgroup per (continuation, query head) walks the prefix)
  arm 3  loglikelihood_shared, attention="rows"   (lmi_attn_prefix_rows: the prefix read once per 32 packed rows)
with, per arm, the split of the time into the prefix prefill (arm 1: the towers and the packed LLM pass), the suffix pass and the head —
host clock around device synchronises placed at those boundaries, inside the same timed calls.  Then the two attention launches alone at the
same shapes (H 32 / KV 8 / D 128, P = 7186, N continuations of 1 and of 8 rows).  ``rows_is_default`` applies the rule of README "Scoring
from a cached prefix": arm 3 ahead of arm 2 by more than arm 2's round-to-round spread (max - min) at N = 4 and at N = 16, for both lengths.
Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from leopard_amd import compat  # noqa: E402
from leopard_amd.config import full_config  # noqa: E402
from leopard_amd.ops import Ops  # noqa: E402
from leopard_amd.weights import SynthSource  # noqa: E402
from tools.gen_fulldepth_fixtures import sample_inputs  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", default="1,4,8,16,64")
ap.add_argument("--lengths", default="1,8", help="continuation lengths (ids)")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--precision", choices=["fast", "lo4"], default="lo4")
ap.add_argument("--layers", default="", help="V,L: reduced depth (a rehearsal; the committed numbers are full depth)")
ap.add_argument("--out", default="")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("score_shared_bench.py measures on the GPU; no device found")
dev = torch.device("cuda:0")

cfg = full_config()
if args.layers:
    cfg.vision_config.num_hidden_layers, cfg.text_config.num_hidden_layers = (int(x) for x in args.layers.split(","))
ops = Ops()
model = compat.LeopardForConditionalGeneration(cfg, lambda d, dt: SynthSource(cfg, ops, d, dt), torch.float16, ops, torch_dtype=torch.float16,
                                               precision=args.precision).to(dev)
eng = model.engine
u8, ids, _ = sample_inputs(cfg, 6, 1344, 896)
tiles = torch.from_numpy(u8).to(dev)
empty = torch.zeros(1, 0, dtype=torch.int64)

# ---- where the time goes: synchronising timers at the boundaries prefix prefill | suffix pass | head --------------------------------------
parts = {}
depth = {"prefill": 0}


def timed_part(name, fn, nested_in_prefill=False):
    def wrapper(*a, **k):
        if nested_in_prefill and depth["prefill"]:
            return fn(*a, **k)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if name == "prefix_prefill":
            depth["prefill"] += 1
        try:
            return fn(*a, **k)
        finally:
            if name == "prefix_prefill":
                depth["prefill"] -= 1
            torch.cuda.synchronize()
            parts[name] = parts.get(name, 0.0) + 1e3 * (time.perf_counter() - t0)
    return wrapper


eng.prefill = timed_part("prefix_prefill", eng.prefill)
eng._llm_layers = timed_part("llm_pass", eng._llm_layers, nested_in_prefill=True)
eng._score_head = timed_part("head", eng._score_head)


def run(fn):
    parts.clear()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return {"total": 1e3 * (time.perf_counter() - t0), **parts}


def measure(fns, rounds):
    """{arm: {part: {median, min, max}}} of the callables, interleaved round by round after one warm-up round."""
    ts = {k: [] for k in fns}
    for r in range(rounds + 1):
        for k, fn in fns.items():
            one = run(fn)
            if r > 0:
                ts[k].append(one)
    out = {}
    for k, rs in ts.items():
        out[k] = {p: {"median": round(statistics.median(x[p] for x in rs), 3), "min": round(min(x[p] for x in rs), 3),
                      "max": round(max(x[p] for x in rs), 3)} for p in rs[0]}
    return out


result = {"geometry": "Llama-3.1-8B + SigLIP (synthetic weights, fp16)",
          "depth": f"{cfg.vision_config.num_hidden_layers} + {cfg.text_config.num_hidden_layers} layers", "precision": args.precision,
          "sample": "C3: 6 x 1344x896", "merged_rows": eng.merged_len(ids), "rounds": args.rounds,
          "parts": "arm 1: llm_pass = the packed LLM pass of the full prompts, total - llm_pass - head = towers, embedding, host; arms 2 / 3: "
                   "prefix_prefill (towers + 7186 rows), llm_pass = the suffix pass, head", "per_n": {}, "kernel": {}}
if args.out and os.path.exists(args.out):
    with open(args.out) as f:
        old = json.load(f)
    if all(old.get(k) == result[k] for k in ("depth", "precision", "merged_rows", "rounds")):
        result["per_n"], result["kernel"] = old.get("per_n", {}), old.get("kernel", {})
rng = np.random.default_rng(0)
H, KV, D = 32, 8, 128
P = eng.merged_len(ids[:, :-1])
for N in [int(x) for x in args.n.split(",")]:
    for m in [int(x) for x in args.lengths.split(",")]:
        conts = [torch.from_numpy(rng.integers(1000, 100000, m)).reshape(1, -1) for _ in range(N)]
        full = [(ids, c, tiles) for c in conts]
        shared = [(empty, c) for c in conts]
        r = measure({"arm1_loglikelihood": lambda: model.loglikelihood(full),
                     "arm2_shared_ranges": lambda: model.loglikelihood_shared(ids, tiles, shared, attention="ranges"),
                     "arm3_shared_rows": lambda: model.loglikelihood_shared(ids, tiles, shared, attention="rows")}, args.rounds)
        a1, a2, a3 = (r[k]["total"] for k in ("arm1_loglikelihood", "arm2_shared_ranges", "arm3_shared_rows"))
        r["arm1_over_arm2"] = round(a1["median"] / a2["median"], 2)
        r["arm1_over_arm3"] = round(a1["median"] / a3["median"], 2)
        r["arm2_minus_arm3_ms"] = round(a2["median"] - a3["median"], 3)
        r["arm2_spread_ms"] = round(a2["max"] - a2["min"], 3)
        result["per_n"][f"{N}x{m}"] = r
        print(f"N={N} m={m}: arm 1 {a1['median']:.1f} ms | arm 2 ranges {a2['median']:.1f} ms (suffix pass "
              f"{r['arm2_shared_ranges']['llm_pass']['median']:.2f}) | arm 3 rows {a3['median']:.1f} ms (suffix pass "
              f"{r['arm3_shared_rows']['llm_pass']['median']:.2f}) | arm 2 - arm 3 = {r['arm2_minus_arm3_ms']} ms, arm 2 spread {r['arm2_spread_ms']} ms",
              flush=True)

        # ---- the two attention launches alone at this shape: N continuations of m rows behind P cached rows -----------------------------------
        lens = [m] * N
        cu = [0] + [int(c) for c in np.cumsum(lens)]
        g = torch.Generator(device="cpu").manual_seed(N * 16 + m)
        qkv = torch.randn(cu[-1], (H + 2 * KV) * D, generator=g).to(torch.float16).to(dev)
        q, k, v = qkv[:, :H * D], qkv[:, H * D:(H + KV) * D], qkv[:, (H + KV) * D:]
        cache = torch.randn(2, P, KV * D, generator=g).to(torch.float16).to(dev)
        out = torch.empty(cu[-1], H * D, dtype=torch.float16, device=dev)
        cu_t = torch.tensor(cu, dtype=torch.int32, device=dev)
        k_begin = torch.tensor(np.repeat(cu[:-1], m), dtype=torch.int32, device=dev)
        k_len = torch.tensor(np.tile(np.arange(1, m + 1), N), dtype=torch.int32, device=dev)
        ws = torch.empty(ops.prefix_rows_workspace_elems(cu[-1], H, D, P, m), dtype=torch.float32, device=dev)
        o32 = torch.empty(cu[-1], H * D, dtype=torch.float32, device=dev)
        reps = 20
        kern = {"lmi_attn_prefix_fwd": lambda: [ops.attention_prefix(q, k, v, cache[0], cache[1], P, out, cu_t, m, H, KV, D, D ** -0.5) for _ in range(reps)],
                "lmi_attn_prefix_rows": lambda: [ops.attention_prefix_rows(q, cache[0], cache[1], P, k, v, out, k_begin, k_len, m, H, KV, D, D ** -0.5, ws)
                                                 for _ in range(reps)],
                "lmi_attn_prefix_rows_f32": lambda: [ops.attention_prefix_rows(q, cache[0], cache[1], P, k, v, out, k_begin, k_len, m, H, KV, D, D ** -0.5,
                                                                                ws, out_f32=o32) for _ in range(reps)]}
        km = {}
        for name, fn in kern.items():
            ts = []
            for rr in range(max(args.rounds, 5) + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if rr > 0:
                    ts.append(1e6 * (time.perf_counter() - t0) / reps)
            km[name + "_us"] = round(statistics.median(ts), 1)
        result["kernel"][f"{N}x{m}"] = km
        print(f"N={N} m={m}: the launches alone (P = {P}, {cu[-1]} rows): {json.dumps(km)}", flush=True)
        del qkv, cache, out, ws, o32, full
        torch.cuda.empty_cache()

rule = []
for key in [f"{n}x{m}" for n in (4, 16) for m in (1, 8)]:
    r = result["per_n"].get(key)
    rule.append(None if r is None else bool(r["arm2_minus_arm3_ms"] > r["arm2_spread_ms"]))
result["rows_is_default"] = None if None in rule else all(rule)
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
