#!/usr/bin/env python3
"""What the pair (hl) decode step costs above 8 sequences, on the Llama-3.1-8B geometry (synthetic weights, fp16, precision "lo4", full
depth): the captured greedy step as the pair step at B = 8 (lmi_gemm_skinny_hl), 16 and 32 (lmi_gemm_skinny_wide_hl, decode_pair_limit = 32)
and as the fast step at B = 16 (lmi_gemm_skinny) and 32 (lmi_gemm_skinny_wide), each with 256 and with 7187 key rows in every slot.
Protocol of tools/wide_decode_bench.py: one process, back-to-back graph replays timed with events, the arms interleaved round by round,
medians of the rounds after a warm-up round (which also captures the graphs), with the round-to-round spread (max - min).  The alternative
to one pair step of 2 B sequences is two pair steps of B, so a width is worth offering only if pair(16) < 2 pair(8) and pair(32) < 2 pair(16),
at both contexts, by more than the spreads.  Prints one JSON object (and writes it to --out, default profiles/wide_pair_step.json).  Run it
under a time limit of its own (timeout -k 10 900 python tools/wide_pair_bench.py): it starts nothing after a failed step."""
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
ap.add_argument("--context", type=int, nargs="*", default=[256, 7187], help="key rows per slot when a timed round starts")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_pair_step.json"))
args = ap.parse_args()
ARMS = (("pair", 8), ("fast", 16), ("pair", 16), ("fast", 32), ("pair", 32))
dev = torch.device("cuda:0")
cfg = full_config()
ops = Ops()
eng = LeopardEngine(cfg, EngineWeights.build(cfg, SynthSource(cfg, ops, dev, torch.float16), torch.float16), ops=ops, device=dev)
eng.precision = "lo4"
eng.decode_batch_limit = 32


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def step_times():
    """{(arm, B, context): [ms per replay of every timed round]}.  One pooled state per arm (a context's capacity is what generate_stream would
    allocate for it: rounded up to 1024 rows), all kept alive for the whole run.  A state is the pair or the fast step by the pair limit it
    was built under (8: B = 16 and 32 decode on the fast step; 32: on pairs)."""
    states = {}
    for ctx in sorted(args.context):
        for arm, B in ARMS:
            eng.decode_pair_limit = 32 if arm == "pair" else 8
            st = eng._batch_state(B, ctx + args.steps + 2)
            assert st.hl == (arm == "pair") and st.B == B
            st.tok.fill_(5); st.live.fill_(1); st.budget.fill_(1 << 30); st.eos.fill_(-1)
            st.sampling, st.beams = False, 0
            eng._set_logprobs(st, None)
            eng._set_rules(st, None, ())
            states[(arm, B, ctx)] = st
    res = {k: [] for k in states}
    for r in range(args.rounds + 1):
        for (arm, B, ctx), st in states.items():
            def start():
                st.pos.fill_(ctx - 1); st.k_len.fill_(ctx); st.hist_pos.zero_()
            start()
            eng._batch_decode_run(st)                                         # (captures on first use)
            start()
            t = timed(lambda: eng._batch_decode_run(st), args.steps)
            if r > 0:                                                         # round 0: capture + warm-up
                res[(arm, B, ctx)].append(t)
    return res, {k: st.capacity for k, st in states.items()}


result = {"geometry": "Llama-3.1-8B (synthetic weights, fp16, precision lo4, full depth), greedy captured step", "rounds": args.rounds,
          "steps_per_round": args.steps, "steps": {}, "conditions": {}, "pair_over_fast": {},
          "not_measured": ["bf16", "contexts other than those listed", "generate_stream end to end"]}
times, caps = step_times()
med = {k: statistics.median(v) for k, v in times.items()}
spread = {k: max(v) - min(v) for k, v in times.items()}
for (arm, B, ctx), v in times.items():
    k = (arm, B, ctx)
    result["steps"][f"{arm}_B{B}_ctx{ctx}"] = {"ms": round(med[k], 4), "spread_ms": round(spread[k], 4), "rounds_ms": [round(t, 4) for t in v],
                                               "tokens_per_s": round(1e3 * B / med[k], 1), "slot_capacity": caps[k]}
    print(f"{arm} B={B} ctx={ctx}: {med[k]:.4f} ms (spread {spread[k]:.4f}), {1e3 * B / med[k]:.0f} tokens/s", flush=True)
for ctx in args.context:
    for small, big in ((8, 16), (16, 32)):
        a, b = ("pair", small, ctx), ("pair", big, ctx)
        margin = 2 * med[a] - med[b]
        result["conditions"][f"pair{big}_lt_2x_pair{small}_ctx{ctx}"] = {
            "two_small_steps_ms": round(2 * med[a], 4), "one_big_step_ms": round(med[b], 4), "margin_ms": round(margin, 4),
            "spreads_ms": round(2 * spread[a] + spread[b], 4), "met": bool(margin > 2 * spread[a] + spread[b])}
    for B in (16, 32):
        result["pair_over_fast"][f"B{B}_ctx{ctx}"] = round(med[("pair", B, ctx)] / med[("fast", B, ctx)], 4)
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
