#!/usr/bin/env python3
"""What generate(rules=...) adds to a decode step, on the Llama-3.1-8B geometry (synthetic weights, fp16, full depth): the captured step at
B = 1 and B = 16 — greedy, greedy + repetition penalty, greedy + all three rules, with 512 and with 8192 ids in every slot's ``seq`` — and
lmi_decode_rules alone on [B, 128256] fp32 rows.  One process; step times are back-to-back graph replays timed with events (device time
per token), the arms interleaved round by round, medians of the rounds after a warm-up round (which also captures the graphs).  Every
timed round starts from the arm's sequence length (the step appends one id per replay: a round ends ``--steps`` ids later).  The yardstick
is the sampled step of the same run: the rules surcharge over greedy should stay below the sampled step's.  Prints one JSON object (and
writes it to --out, default profiles/gen_rules_step.json)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from leopard_amd.config import full_config  # noqa: E402
from leopard_amd.engine import LeopardEngine, LogitsRules, SamplingParams  # noqa: E402
from leopard_amd.ops import Ops  # noqa: E402
from leopard_amd.weights import EngineWeights, SynthSource  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=48, help="replays per timed round")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--kernel-iters", type=int, default=200)
ap.add_argument("--batch", type=int, nargs="*", default=[1, 16])
ap.add_argument("--seq", type=int, nargs="*", default=[512, 8192], help="ids in seq when a timed round starts")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gen_rules_step.json"))
args = ap.parse_args()
dev = torch.device("cuda:0")
cfg = full_config()
V = cfg.text_config.vocab_size
ops = Ops()
eng = LeopardEngine(cfg, EngineWeights.build(cfg, SynthSource(cfg, ops, dev, torch.float16), torch.float16), ops=ops, device=dev)
HF = SamplingParams(temperature=0.7, top_k=50, top_p=0.9, seed=1)        # tools/bench_sampling.py's sampled setting: both filters active
PENALTY = LogitsRules(repetition_penalty=1.2)
ALL = LogitsRules(repetition_penalty=1.2, no_repeat_ngram_size=3, min_new_tokens=1 << 20)    # (the countdown never runs out inside the run)
EOS = (128001, 128009)
ARMS = {"greedy": (False, None, 0), "sampled": (True, None, 0)}
for L in args.seq:
    ARMS[f"penalty_seq{L}"] = (False, PENALTY, L)
    ARMS[f"all_rules_seq{L}"] = (False, ALL, L)


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def prompt_ids(L, j):
    """L ids of a text-like sequence: draws from 2000 distinct ids, so ids and n-grams repeat."""
    g = torch.Generator().manual_seed(100 + j)
    return (torch.randint(0, 2000, (L,), generator=g) * 61 % V).tolist()


def step_times(B):
    """{arm: median ms per replay} of the B-row step."""
    n_total = (args.steps + 1) * (args.rounds + 1) * len(ARMS) + 16
    need = max(args.seq) + 64 + n_total
    if B == 1:
        cache = eng._generation_cache(need)
        ids = torch.arange(1, 33, dtype=torch.long).reshape(1, -1).to(dev)
        eng.prefill(ids, None, cache=cache)
        st = eng._decode_state(cache)
        eng._decode_seed(st, cache, 5)
        eng._set_sampling(st, 0, HF)
        run = lambda: eng._decode_run(st, cache)  # noqa: E731
    else:
        st = eng._batch_state(B, need)
        st.tok.fill_(5); st.pos.fill_(32); st.k_len.fill_(33); st.live.fill_(1); st.budget.fill_(1 << 30); st.eos.fill_(-1)
        for j in range(B):
            eng._set_sampling(st, j, HF.for_request(j))
        run = lambda: eng._batch_decode_run(st)  # noqa: E731
    prompts = {L: [prompt_ids(L, j) for j in range(B)] for L in args.seq}
    res = {a: [] for a in ARMS}
    for r in range(args.rounds + 1):
        for arm, (sampled, rules, L) in ARMS.items():
            st.sampling = sampled
            eng._set_rules(st, rules, EOS)                                    # (allocates the buffers on first use)

            def start():
                if rules is not None:
                    for j in range(B):
                        eng._fill_rules(st, j, prompts[L][j], rules)
                    st.rule_min_left.fill_(int(rules.min_new_tokens))
                if B > 1:
                    st.hist_pos.zero_()
            start()
            run()                                                             # (captures on first use)
            start()
            t = timed(run, args.steps)
            if r > 0:                                                         # round 0: capture + warm-up
                res[arm].append(t)
    st.sampling, st.rules = False, False
    return {a: statistics.median(v) for a, v in res.items()}


def kernel_times(B):
    out = {}
    for L in args.seq:
        for name, rules in (("penalty", PENALTY), ("all_rules", ALL)):
            g = torch.Generator(device=dev).manual_seed(0)
            logits = torch.randn(B, V, device=dev, generator=g) * 3
            seq = torch.tensor([prompt_ids(L, j) for j in range(B)], dtype=torch.int32).to(dev)
            full = lambda v, dt: torch.full((B,), v, dtype=dt, device=dev)    # noqa: E731
            seq_len, pen = full(L, torch.int32), full(float(rules.repetition_penalty), torch.float32)
            ngram, min_left = full(int(rules.no_repeat_ngram_size), torch.int32), full(int(rules.min_new_tokens), torch.int32)
            eos = torch.tensor(EOS, dtype=torch.int64, device=dev)
            # tok = None: nothing is appended, every launch sees L ids
            out[f"decode_rules_{name}_seq{L}_us"] = 1e3 * timed(lambda: ops.decode_rules(logits, V, seq, seq_len, pen, ngram, min_left, eos=eos),
                                                                args.kernel_iters)
    logits = torch.randn(B, V, device=dev) * 3
    tok, pos = torch.zeros(B, dtype=torch.int64, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    k_len = torch.ones(B, dtype=torch.int32, device=dev)
    out["decode_advance_us"] = 1e3 * timed(lambda: ops.decode_advance(logits, V, tok, pos, k_len=k_len), args.kernel_iters)
    return out


result = {"geometry": "Llama-3.1-8B (synthetic weights, fp16, fast schedule, full depth), vocab %d" % V, "sampling": HF.describe(),
          "penalty": PENALTY.describe(), "all_rules": ALL.describe(), "rounds": args.rounds, "steps_per_round": args.steps, "steps": {},
          "kernel": {}}
for B in args.batch:
    t = step_times(B)
    g = t["greedy"]
    pct = {a: round(100 * (t[a] / g - 1), 2) for a in t if a != "greedy"}
    result["steps"][f"B{B}"] = {"ms": {a: round(v, 4) for a, v in t.items()}, "surcharge_over_greedy_pct": pct,
                                "rules_within_sampled_surcharge": bool(max(v for a, v in t.items() if a not in ("greedy", "sampled")) <= t["sampled"])}
    print(f"B={B}: " + ", ".join(f"{a} {v:.4f} ms" for a, v in t.items()) + f"; over greedy: {pct}", flush=True)
for B in args.batch:
    result["kernel"][f"B{B}"] = {k: round(v, 2) for k, v in kernel_times(B).items()}
    print(f"B={B}: kernels (us) {result['kernel'][f'B{B}']}", flush=True)
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
