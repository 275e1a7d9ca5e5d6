#!/usr/bin/env python3
"""What a decode step wider than 16 sequences costs, on the Llama-3.1-8B geometry (synthetic weights, fp16, fast schedule, full depth): the
captured greedy step at B = 16 (lmi_gemm_skinny), 32 and 64 (lmi_gemm_skinny_wide), each with 256 and with 7187 key rows in every slot, and
the projection entries alone at the five shapes of the step (q|k|v + RoPE, o, gate/up, down, head) at 16, 32 and 64 rows.  Protocol of
tools/gen_rules_bench.py: one process, back-to-back graph replays timed with events, the arms interleaved round by round, medians of the
rounds after a warm-up round (which also captures the graphs), with the round-to-round spread (max - min).  The alternative to one step of
2 B rows is two steps of B rows, so a width is worth offering only if step(32) < 2 step(16) and step(64) < 2 step(32), at both contexts, by
more than the spreads.  Prints one JSON object (and writes it to --out, default profiles/wide_decode_step.json)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from leopard_amd.config import full_config  # noqa: E402
from leopard_amd.engine import LeopardEngine  # noqa: E402
from leopard_amd.ops import Ops  # noqa: E402
from leopard_amd.weights import EngineWeights, SynthSource  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=48, help="replays per timed round")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--kernel-iters", type=int, default=128)
ap.add_argument("--batch", type=int, nargs="*", default=[16, 32, 64])
ap.add_argument("--context", type=int, nargs="*", default=[256, 7187], help="key rows per slot when a timed round starts")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_decode_step.json"))
args = ap.parse_args()
dev = torch.device("cuda:0")
cfg = full_config()
tc = cfg.text_config
ops = Ops()
eng = LeopardEngine(cfg, EngineWeights.build(cfg, SynthSource(cfg, ops, dev, torch.float16), torch.float16), ops=ops, device=dev)
eng.decode_batch_limit = max(args.batch + [16])


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def step_times():
    """{(B, context): [ms per replay of every timed round]}.  One pooled state per arm (a context's capacity is what generate_stream would
    allocate for it: rounded up to 1024 rows), all kept alive for the whole run; short contexts first, so that no state is reused for a
    longer one."""
    states = {}
    for ctx in sorted(args.context):
        for B in args.batch:
            st = eng._batch_state(B, ctx + args.steps + 2)
            st.tok.fill_(5); st.live.fill_(1); st.budget.fill_(1 << 30); st.eos.fill_(-1)
            st.sampling, st.beams = False, 0
            eng._set_logprobs(st, None)
            eng._set_rules(st, None, ())
            states[(B, ctx)] = st
    res = {k: [] for k in states}
    for r in range(args.rounds + 1):
        for (B, ctx), st in states.items():
            def start():
                st.pos.fill_(ctx - 1); st.k_len.fill_(ctx); st.hist_pos.zero_()
            start()
            eng._batch_decode_run(st)                                         # (captures on first use)
            start()
            t = timed(lambda: eng._batch_decode_run(st), args.steps)
            if r > 0:                                                         # round 0: capture + warm-up
                res[(B, ctx)].append(t)
    return res, {k: st.capacity for k, st in states.items()}


def kernel_times():
    """us per launch of the five projections of a step at M rows, walking the 32 layers' weights as the step does (one layer's weights would
    sit in the last-level cache); the head has one copy (1 GB)."""
    W, D = eng.W, tc.hidden_size
    (H, KV), hd = eng._llm_heads(), tc.head_dim
    out = {}
    for M in args.batch:
        wide = M > 16
        gemm = ops.gemm_skinny_wide if wide else ops.gemm_skinny
        rope = ops.rope_qkv_skinny_wide if wide else ops.rope_qkv_skinny
        x = torch.randn(M, D, device=dev).to(torch.float16)
        xf = torch.randn(M, W.llm_ff, device=dev).to(torch.float16)
        qkv = torch.empty(M, (H + 2 * KV) * hd, dtype=torch.float16, device=dev)
        res = torch.zeros(M, D, dtype=torch.float32, device=dev)
        gu = torch.empty(M, W.llm_ff, dtype=torch.float16, device=dev)
        logits = torch.empty(M, W.lm_head.shape[0], dtype=torch.float32, device=dev)
        cap = 64
        kc, vc = torch.zeros(M * cap, KV * hd, dtype=torch.float16, device=dev), torch.zeros(M * cap, KV * hd, dtype=torch.float16, device=dev)
        cos, sin = eng.rope_tables(torch.arange(cap))
        pos = torch.full((M,), 7, dtype=torch.int32, device=dev)
        layer = [0]

        def walk(fn):
            def run():
                fn(W.llm_layers[layer[0] % len(W.llm_layers)])
                layer[0] += 1
            return run
        calls = {"qkv_rope": (walk(lambda L: rope(L.qkv_w_rope, x, qkv, H, KV, hd, cos, sin, kc, vc, cap, pos)), (H + 2 * KV) * hd * D),
                 "o": (walk(lambda L: gemm(L.o_w, x, res, 1)), D * D),
                 "gate_up": (walk(lambda L: gemm(L.gu_w, x, gu, 2)), 2 * W.llm_ff * D),
                 "down": (walk(lambda L: gemm(L.down_w, xf, res, 1)), D * W.llm_ff),
                 "head": (lambda: gemm(eng._skinny_head(), x, logits, 3), W.lm_head.shape[0] * D)}
        row = {}
        for name, (fn, w_elems) in calls.items():
            timed(fn, 8)
            rounds = [timed(fn, args.kernel_iters) for _ in range(args.rounds)]
            us = 1e3 * statistics.median(rounds)
            row[name] = {"us": round(us, 2), "spread_us": round(1e3 * (max(rounds) - min(rounds)), 2), "weight_GBps": round(2 * w_elems / us / 1e3, 1)}
        out[f"M{M}"] = row
    return out


result = {"geometry": "Llama-3.1-8B (synthetic weights, fp16, fast schedule, full depth), greedy captured step", "rounds": args.rounds,
          "steps_per_round": args.steps, "steps": {}, "conditions": {}, "kernel": {}}
times, caps = step_times()
med = {k: statistics.median(v) for k, v in times.items()}
spread = {k: max(v) - min(v) for k, v in times.items()}
for (B, ctx), v in times.items():
    result["steps"][f"B{B}_ctx{ctx}"] = {"ms": round(med[(B, ctx)], 4), "spread_ms": round(spread[(B, ctx)], 4), "rounds_ms": [round(t, 4) for t in v],
                                         "tokens_per_s": round(1e3 * B / med[(B, ctx)], 1), "slot_capacity": caps[(B, ctx)]}
    print(f"B={B} ctx={ctx}: {med[(B, ctx)]:.4f} ms (spread {spread[(B, ctx)]:.4f}), {1e3 * B / med[(B, ctx)]:.0f} tokens/s", flush=True)
for ctx in args.context:
    for small, big in zip(args.batch[:-1], args.batch[1:]):
        if big != 2 * small:
            continue
        a, b = (small, ctx), (big, ctx)
        margin = 2 * med[a] - med[b]
        result["conditions"][f"step{big}_lt_2x_step{small}_ctx{ctx}"] = {
            "two_small_steps_ms": round(2 * med[a], 4), "one_big_step_ms": round(med[b], 4), "margin_ms": round(margin, 4),
            "spreads_ms": round(2 * spread[a] + spread[b], 4), "met": bool(margin > 2 * spread[a] + spread[b])}
    if (16, ctx) in med and (32, ctx) in med:
        result["conditions"][f"step32_minus_step16_over_step16_ctx{ctx}"] = round((med[(32, ctx)] - med[(16, ctx)]) / med[(16, ctx)], 4)
print(json.dumps(result["conditions"]), flush=True)
result["kernel"] = kernel_times()
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
