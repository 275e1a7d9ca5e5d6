#!/usr/bin/env python3
"""What min_p / typical_p / epsilon_cutoff / eta_cutoff add to a sampled decode step, on the Llama-3.1-8B geometry (synthetic weights,
fp16, full depth): the captured step at B = 1 and B = 16 — greedy, sampled (lmi_decode_sample, the untouched kernel), and
lmi_decode_sample_ex with min_p, with epsilon_cutoff, with eta_cutoff, with typical_p and with all four.  The protocol of
tools/gen_rules_bench.py: one process; step times are back-to-back graph replays timed with events (device time per token), the arms
interleaved round by round, medians of the rounds after a warm-up round (which also captures the graphs); the spread of the rounds
((max - min) / median) is recorded per arm.  The yardstick is the plain sampled arm of the same run.  Prints one JSON object and a
markdown table, and writes the JSON to --out (default profiles/sampling_ext_step.json)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from leopard_amd.config import full_config  # noqa: E402
from leopard_amd.engine import LeopardEngine, SamplingParams  # noqa: E402
from leopard_amd.ops import Ops  # noqa: E402
from leopard_amd.weights import EngineWeights, SynthSource  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=48, help="replays per timed round")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--batch", type=int, nargs="*", default=[1, 16])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampling_ext_step.json"))
args = ap.parse_args()
dev = torch.device("cuda:0")
cfg = full_config()
V = cfg.text_config.vocab_size
ops = Ops()
eng = LeopardEngine(cfg, EngineWeights.build(cfg, SynthSource(cfg, ops, dev, torch.float16), torch.float16), ops=ops, device=dev)
BASE = dict(temperature=0.7, top_k=50, top_p=0.9, seed=1)                # tools/bench_sampling.py's sampled setting: both filters active
ARMS = {"greedy": None, "sampled": SamplingParams(**BASE),
        "min_p": SamplingParams(min_p=0.05, **BASE), "epsilon": SamplingParams(epsilon_cutoff=3e-4, **BASE),
        "eta": SamplingParams(eta_cutoff=2e-3, **BASE), "typical": SamplingParams(typical_p=0.9, **BASE),
        "all_four": SamplingParams(min_p=0.05, typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=2e-3, **BASE)}


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def step_times(B):
    """{arm: (median ms per replay, spread of the rounds)} of the B-row step."""
    need = 64 + (args.steps + 1) * (args.rounds + 1) * len(ARMS) + 16
    if B == 1:
        cache = eng._generation_cache(need)
        ids = torch.arange(1, 33, dtype=torch.long).reshape(1, -1).to(dev)
        eng.prefill(ids, None, cache=cache)
        st = eng._decode_state(cache)
        eng._decode_seed(st, cache, 5)
        run = lambda: eng._decode_run(st, cache)  # noqa: E731
    else:
        st = eng._batch_state(B, need)
        st.tok.fill_(5); st.pos.fill_(32); st.k_len.fill_(33); st.live.fill_(1); st.budget.fill_(1 << 30); st.eos.fill_(-1)
        run = lambda: eng._batch_decode_run(st)  # noqa: E731
    eng._set_logprobs(st, None)
    eng._set_rules(st, None)
    res = {a: [] for a in ARMS}
    for r in range(args.rounds + 1):
        for arm, sp in ARMS.items():
            st.sampling, st.sample_ex = sp is not None, sp is not None and sp.extended
            if sp is not None:
                for j in range(B):
                    eng._set_sampling(st, j, sp.for_request(j))
            if B > 1:
                st.hist_pos.zero_()
            run()                                                             # (captures on first use)
            t = timed(run, args.steps)
            if r > 0:                                                         # round 0: capture + warm-up
                res[arm].append(t)
    st.sampling, st.sample_ex = False, False
    return {a: (statistics.median(v), (max(v) - min(v)) / statistics.median(v)) for a, v in res.items()}


result = {"geometry": "Llama-3.1-8B (synthetic weights, fp16, fast schedule, full depth), vocab %d" % V,
          "arms": {a: "greedy" if sp is None else sp.describe() for a, sp in ARMS.items()}, "rounds": args.rounds, "steps_per_round": args.steps,
          "steps": {}}
for B in args.batch:
    t = step_times(B)
    g, s = t["greedy"][0], t["sampled"][0]
    result["steps"][f"B{B}"] = {
        "ms": {a: round(v[0], 4) for a, v in t.items()}, "round_spread_pct": {a: round(100 * v[1], 2) for a, v in t.items()},
        "over_greedy_pct": {a: round(100 * (v[0] / g - 1), 2) for a, v in t.items() if a != "greedy"},
        # the arm's surcharge over the plain sampled step, in units of the plain sampled step's surcharge over greedy
        "over_sampled_in_sampled_surcharges": {a: round((v[0] - s) / (s - g), 3) for a, v in t.items() if a not in ("greedy", "sampled")}}
    print(f"B={B}: " + ", ".join(f"{a} {v[0]:.4f} ms" for a, v in t.items()), flush=True)
print(json.dumps(result))
print("\n| arm | " + " | ".join(f"B = {B}: ms / step | over greedy | round spread" for B in args.batch) + " |")
print("|---|" + "---|---|---|" * len(args.batch))
for a in ARMS:
    cells = []
    for B in args.batch:
        e = result["steps"][f"B{B}"]
        cells.append(f"{e['ms'][a]:.3f} | " + ("—" if a == "greedy" else f"+{e['over_greedy_pct'][a]:.1f} %") + f" | {e['round_spread_pct'][a]:.1f} %")
    print(f"| {a} | " + " | ".join(cells) + " |")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
