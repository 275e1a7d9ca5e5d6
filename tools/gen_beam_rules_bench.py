#!/usr/bin/env python3
"""What the logits processors add to a beam step, on the Llama-3.1-8B geometry (synthetic weights, fp16, full depth) with a C3-length
prefix (7187 rows): per K = 4, 8 the captured step at B = K in "shared" mode — the plain beam step, "beam + penalty" and "beam + all three"
(penalty, n-gram ban of 3, eos banned by min_new_tokens) at 512 and at 8192 prompt ids per beam — and lmi_beam_step / lmi_beam_step_rules
alone.  The protocol of tools/gen_beam_bench.py: one process; a full K-cycle is forced as the permutation (a device copy of one static
parent tensor in front of the K / V reorder launch; the id reorder reads the same parent); step times are back-to-back graph replays timed
with events, the arms interleaved round by round, medians of the rounds after a warm-up round (which also captures the graphs).  Every
timed round starts from the arm's id count and 32 own rows.  The number to compare a rules arm with is the plain arm of the same run; its
round-to-round spread is recorded next to it.  Prints one JSON object (and writes it to --out, default profiles/gen_beam_rules_step.json)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from leopard_amd.config import full_config  # noqa: E402
from leopard_amd.engine import LeopardEngine, LogitsRules  # noqa: E402
from leopard_amd.ops import Ops  # noqa: E402
from leopard_amd.weights import EngineWeights, SynthSource  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=48, help="replays per timed round")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--kernel-iters", type=int, default=200)
ap.add_argument("--beams", type=int, nargs="*", default=[4, 8])
ap.add_argument("--ids", type=int, nargs="*", default=[512, 8192], help="prompt ids per beam when a timed round starts")
ap.add_argument("--prefix", type=int, default=7187, help="prompt rows (a C3 sample)")
ap.add_argument("--own", type=int, default=32, help="own rows when a timed round starts")
ap.add_argument("--layers", type=int, default=0, help="LLM layers (0 = full depth)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gen_beam_rules_step.json"))
args = ap.parse_args()
dev = torch.device("cuda:0")
cfg = full_config()
if args.layers:
    cfg.text_config.num_hidden_layers = args.layers
V = cfg.text_config.vocab_size
ops = Ops()
eng = LeopardEngine(cfg, EngineWeights.build(cfg, SynthSource(cfg, ops, dev, torch.float16), torch.float16), ops=ops, device=dev)
P, EOS = args.prefix, (128001, 128009)
NEED_OWN = args.own + args.steps + 8
RULES = {"penalty": LogitsRules(repetition_penalty=1.2),
         "all": LogitsRules(repetition_penalty=1.2, no_repeat_ngram_size=3, min_new_tokens=1 << 20)}

forced = torch.arange(ops.MAX_BEAMS, dtype=torch.int32, device=dev)
reorder = ops.beam_reorder


def forced_reorder(ptrs, parent, K, row0, held, row_bytes, *a):
    if row_bytes != 16:                                                       # the K / V launch comes first; the id launch reads the same parent
        parent.copy_(forced)
    reorder(ptrs, parent, K, row0, held, row_bytes, *a)


ops.beam_reorder = forced_reorder


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def prompt_ids(n, seed):
    """n ids as a chat prompt holds them: text ids with repeats, and runs of the image placeholder (an id >= vocab is compared, never written)."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, 32000, (n,), generator=g)
    ids[n // 8: n // 8 + n // 2] = cfg.image_token_index
    return ids.tolist()


def step_times(K):
    st = eng._shared_state(K, NEED_OWN, P)
    for t in st.kp + st.vp + st.k + st.v:
        t.normal_(0, 0.5)
    st.prefix_len.fill_(P)
    cycle = torch.arange(ops.MAX_BEAMS, dtype=torch.int32, device=dev)
    cycle[:K] = (torch.arange(K, dtype=torch.int32) + 1) % K
    forced.copy_(cycle)
    arms = {"beam": (None, ())}
    for n in args.ids:
        for name, rules in RULES.items():
            arms[f"beam_{name}_ids{n}"] = (rules, prompt_ids(n, n))
    res = {a: [] for a in arms}
    run = lambda: eng._batch_decode_run(st)  # noqa: E731
    for r in range(args.rounds + 1):
        for arm, (rules, prompt) in arms.items():
            def start():
                eng._set_beams(st, K, set(EOS), 0, NEED_OWN, rules, prompt)
                st.beam_held.fill_(args.own)
                st.tok.copy_(torch.arange(5, 5 + K))
                st.pos.fill_(P + args.own); st.k_len.fill_(args.own + 1)
            start()
            run()                                                             # (captures on first use)
            start()
            t = timed(run, args.steps)
            if r > 0:                                                         # round 0: capture + warm-up
                res[arm].append(t)
            if rules is not None and r == args.rounds:                        # the timed graph did append and permute the id lists
                n = len(prompt)
                torch.cuda.synchronize()
                assert st.seq_len[:K].tolist() == [n + args.steps] * K, st.seq_len.tolist()
                assert st.seq[:K, :n].cpu().tolist() == [prompt] * K
    st.beams, st.rules = 0, False
    forced.copy_(torch.arange(ops.MAX_BEAMS, dtype=torch.int32))
    return res


def kernel_times(K):
    """The two entries alone, back-to-back eager launches on K random rows."""
    out = {}
    logits = torch.randn(K, V, device=dev) * 3
    eos = torch.tensor(list(EOS) + [-1, -1], dtype=torch.int64, device=dev)
    score, tok = torch.zeros(8, device=dev), torch.zeros(8, dtype=torch.int64, device=dev)
    parent, walk = torch.zeros(8, dtype=torch.int32, device=dev), torch.zeros(ops.BEAM_WALK_WORDS, dtype=torch.int32, device=dev)
    rows = (torch.zeros(K, device=dev), torch.zeros(K, 8, dtype=torch.int32, device=dev), torch.zeros(K, 8, device=dev), torch.zeros(K, 4, device=dev))

    def plain():
        score.zero_()
        ops.beam_step(logits, V, K, eos, score, tok, parent, walk, *rows)
    out["beam_step_us"] = 1e3 * timed(plain, args.kernel_iters)
    for n in args.ids:
        seq = torch.tensor([prompt_ids(n, n)] * K, dtype=torch.int32, device=dev)
        seq_len = torch.full((K,), n, dtype=torch.int32, device=dev)
        for name, rules in RULES.items():
            pen = torch.full((K,), float(rules.repetition_penalty), device=dev)
            ng = torch.full((K,), int(rules.no_repeat_ngram_size), dtype=torch.int32, device=dev)
            ml = torch.full((K,), int(rules.min_new_tokens), dtype=torch.int32, device=dev)

            def ruled():
                score.zero_()
                ops.beam_step_rules(logits, V, K, eos, score, tok, parent, walk, *rows, seq, seq_len, pen, ng, ml)
            out[f"beam_step_rules_{name}_ids{n}_us"] = 1e3 * timed(ruled, args.kernel_iters)
    return out


result = {"geometry": "Llama-3.1-8B (synthetic weights, fp16, fast schedule, %s), vocab %d, prefix %d rows, shared decode, forced K-cycle"
          % ("full depth" if not args.layers else f"{args.layers} layers", V, P),
          "rounds": args.rounds, "steps_per_round": args.steps, "steps": {}, "kernel": {}}
for K in args.beams:
    res = step_times(K)
    med = {a: statistics.median(v) for a, v in res.items()}
    base = med["beam"]
    result["steps"][f"K{K}"] = {"ms": {a: round(v, 4) for a, v in med.items()},
                                "plain_rounds_ms": [round(v, 4) for v in res["beam"]],
                                "plain_spread_us": round(1e3 * (max(res["beam"]) - min(res["beam"])), 2),
                                "surcharge_over_plain_beam_us": {a: round(1e3 * (v - base), 2) for a, v in med.items() if a != "beam"}}
    print(f"K={K}: {result['steps'][f'K{K}']}", flush=True)
    eng.release_batch_state()
for K in args.beams:
    result["kernel"][f"K{K}"] = {k: round(v, 2) for k, v in kernel_times(K).items()}
    print(f"K={K}: kernels {result['kernel'][f'K{K}']}", flush=True)
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
