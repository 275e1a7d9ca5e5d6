#!/usr/bin/env python3
"""What generate(logprobs=k) adds to a decode step, on the Llama-3.1-8B geometry (synthetic weights, fp16, full depth): the captured step
at B = 1 and B = 16 in four arms — greedy, greedy + logprobs=0, greedy + logprobs=8, sampled — and lmi_decode_logprobs alone on
[B, 128256] fp32 rows.  One process; step times are back-to-back graph replays timed with events (device time per token), the arms
interleaved round by round, medians of the rounds after a warm-up round (which also captures the graphs).  The yardstick is the sampled
step of the same run: the logprobs surcharge over greedy should not exceed the sampled step's.  Prints one JSON object (and writes it to
--out, default profiles/gen_logprobs_step.json)."""
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
ap.add_argument("--kernel-iters", type=int, default=200)
ap.add_argument("--batch", type=int, nargs="*", default=[1, 16])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gen_logprobs_step.json"))
args = ap.parse_args()
dev = torch.device("cuda:0")
cfg = full_config()
V = cfg.text_config.vocab_size
ops = Ops()
eng = LeopardEngine(cfg, EngineWeights.build(cfg, SynthSource(cfg, ops, dev, torch.float16), torch.float16), ops=ops, device=dev)
HF = SamplingParams(temperature=0.7, top_k=50, top_p=0.9, seed=1)        # tools/bench_sampling.py's sampled setting: both filters active
ARMS = {"greedy": (False, None), "greedy_logprobs0": (False, 0), "greedy_logprobs8": (False, 8), "sampled": (True, None)}


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def step_times(B):
    """{arm: median ms per replay} of the B-row step."""
    n_total = (args.steps + 1) * (args.rounds + 1) * len(ARMS) + 16
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
    res = {a: [] for a in ARMS}
    graphs = {}                                                               # logprobs=0 and logprobs=8 are two captures of the same two graph slots
    slot = lambda: (st.sampling, True)  # noqa: E731  (DecodeState.graphs)
    for r in range(args.rounds + 1):
        for arm, (sampled, k) in ARMS.items():
            st.sampling = sampled
            eng._set_logprobs(st, k)                                          # (allocates the rings on first use; a new k drops the captured pair)
            if arm in graphs:
                st.graphs[slot()] = graphs[arm]
            if B > 1:
                st.hist_pos.zero_()
            run()                                                             # (captures on first use)
            if k is not None:
                graphs[arm] = st.graphs[slot()]
            t = timed(run, args.steps)
            if r > 0:                                                         # round 0: capture + warm-up
                res[arm].append(t)
    st.sampling, st.logprobs = False, None
    return {a: statistics.median(v) for a, v in res.items()}


def kernel_times(B):
    g = torch.Generator(device=dev).manual_seed(0)
    logits = torch.randn(B, V, device=dev, generator=g) * 3
    tok = torch.zeros(B, dtype=torch.int64, device=dev)
    K = ops.MAX_TOP_LOGPROBS
    lp = torch.zeros(1, B, device=dev)
    ti, tl = torch.zeros(1, B, K, dtype=torch.int32, device=dev), torch.zeros(1, B, K, device=dev)
    out = {}
    for k in (0, 1, 8):
        out[f"decode_logprobs_k{k}_us"] = 1e3 * timed(lambda: ops.decode_logprobs(logits, V, tok, k, lp, ti, tl), args.kernel_iters)
    lse, am = torch.zeros(B, device=dev), torch.zeros(B, dtype=torch.int64, device=dev)
    out["token_logprobs_us"] = 1e3 * timed(lambda: ops.token_logprobs(logits, V, tok, lp[0], lse, am), args.kernel_iters)
    pos, k_len = torch.zeros(B, dtype=torch.int32, device=dev), torch.ones(B, dtype=torch.int32, device=dev)
    out["decode_advance_us"] = 1e3 * timed(lambda: ops.decode_advance(logits, V, tok, pos, k_len=k_len), args.kernel_iters)
    return out


result = {"geometry": "Llama-3.1-8B (synthetic weights, fp16, fast schedule, full depth), vocab %d" % V, "sampling": HF.describe(),
          "rounds": args.rounds, "steps_per_round": args.steps, "steps": {}, "kernel": {}}
for B in args.batch:
    t = step_times(B)
    g = t["greedy"]
    pct = {a: round(100 * (t[a] / g - 1), 2) for a in t if a != "greedy"}
    result["steps"][f"B{B}"] = {"ms": {a: round(v, 4) for a, v in t.items()}, "surcharge_over_greedy_pct": pct,
                                "logprobs8_within_sampled_surcharge": bool(t["greedy_logprobs8"] <= t["sampled"]),
                                "logprobs0_within_sampled_surcharge": bool(t["greedy_logprobs0"] <= t["sampled"])}
    print(f"B={B}: " + ", ".join(f"{a} {v:.4f} ms" for a, v in t.items()) + f"; over greedy: {pct}", flush=True)
for B in args.batch:
    result["kernel"][f"B{B}"] = {k: round(v, 2) for k, v in kernel_times(B).items()}
    print(f"B={B}: kernels (us) {result['kernel'][f'B{B}']}", flush=True)
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
