#!/usr/bin/env python3
"""What beam search adds to a batched decode step, on the Llama-3.1-8B geometry (synthetic weights, fp16, full depth) with a C3-length
prefix (7187 rows): per K = 2, 4, 8 the captured step at B = K in "shared" mode (K = 4 in "copy" mode too) — greedy (the path as it is
without beam search), the beam step with an identity permutation, the beam step with a full K-cycle at 32 and at 256 own rows — and
lmi_beam_step / lmi_beam_reorder alone.  The permutation is forced: a device copy of ONE static parent tensor in front of the reorder launch
(one more tiny node in the beam arms), which each arm fills before its rounds; after an arm's last timed round one more replay over marked
rows checks that the captured step moved the rows the arm says (recorded as slot_held_after_one_replay).  One process; step times are
back-to-back graph replays timed with events, the arms interleaved round by round, medians of the rounds after a warm-up round (which
also captures the graphs): the protocol of tools/gen_rules_bench.py.
Every timed round starts from the arm's row count (a replay appends one row).  Prints one JSON object (and writes it to --out, default
profiles/gen_beam_step.json)."""
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
ap.add_argument("--kernel-iters", type=int, default=200)
ap.add_argument("--beams", type=int, nargs="*", default=[2, 4, 8])
ap.add_argument("--copy-beams", type=int, nargs="*", default=[4], help="K values also measured in copy mode")
ap.add_argument("--prefix", type=int, default=7187, help="prompt rows (a C3 sample)")
ap.add_argument("--rows", type=int, nargs="*", default=[32, 256], help="own rows when a timed K-cycle round starts")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gen_beam_step.json"))
args = ap.parse_args()
dev = torch.device("cuda:0")
cfg = full_config()
V = cfg.text_config.vocab_size
ops = Ops()
eng = LeopardEngine(cfg, EngineWeights.build(cfg, SynthSource(cfg, ops, dev, torch.float16), torch.float16), ops=ops, device=dev)
P, EOS = args.prefix, (128001, 128009)
NEED_OWN = max(args.rows) + args.steps + 8

# The forced permutation: ONE static device tensor, read by a copy node that every captured beam step holds in front of its reorder
# launch; an arm writes its parent array INTO it before its rounds (another tensor per arm would leave the graph copying the first one's)
forced = torch.arange(ops.MAX_BEAMS, dtype=torch.int32, device=dev)
reorder = ops.beam_reorder


def forced_reorder(ptrs, parent, *a):
    parent.copy_(forced)
    reorder(ptrs, parent, *a)


ops.beam_reorder = forced_reorder


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def step_times(K, mode, slots):
    """{arm: median ms per replay} of the K-slot step; ``slots[arm]``: after one more replay, the slot whose marked row each slot holds."""
    if mode == "shared":
        st = eng._shared_state(K, NEED_OWN, P)
        for t in st.kp + st.vp:
            t.normal_(0, 0.5)
        st.prefix_len.fill_(P)
        row0 = 0
    else:
        st = eng._batch_state(K, P + NEED_OWN)
        row0 = P
    for t in st.k + st.v:
        t.normal_(0, 0.5)
    ident = torch.arange(ops.MAX_BEAMS, dtype=torch.int32, device=dev)
    cycle = ident.clone()
    cycle[:K] = (torch.arange(K, dtype=torch.int32) + 1) % K
    arms = {"greedy": (False, ident, args.rows[0]), "beam_identity": (True, ident, args.rows[0])}
    for r in args.rows:
        arms[f"beam_cycle_rows{r}"] = (True, cycle, r)
    res = {a: [] for a in arms}
    run = lambda: eng._batch_decode_run(st)  # noqa: E731
    marks = torch.arange(1, K + 1, dtype=torch.float16, device=dev)

    def moved(parent, own):
        """One more replay over marked rows: row ``row0`` of slot b of the first K tensor holds b + 1 before it (the step appends at row
        row0 + own, so the mark is only ever touched by the permutation); which slot's mark each slot holds afterwards."""
        k0 = st.k[0].view(K, st.capacity, -1)
        k0[:, row0, :] = marks[:, None]
        run()
        torch.cuda.synchronize()
        got = (k0[:, row0, 0].float().cpu() - 1).to(torch.int32).tolist()
        assert got == parent[:K].tolist(), (got, parent[:K].tolist())
        return got
    for r in range(args.rounds + 1):
        for arm, (beam, parent, own) in arms.items():
            def start():
                if beam:
                    eng._set_beams(st, K, set(EOS), row0, NEED_OWN)
                    st.beam_held.fill_(row0 + own)
                else:
                    st.beams = 0
                    st.live.fill_(1); st.budget.fill_(1 << 30); st.eos.fill_(-1); st.hist_pos.zero_()
                forced.copy_(parent)
                st.tok.fill_(5); st.pos.fill_(P + own); st.k_len.fill_(row0 + own + 1)
            start()
            run()                                                             # (captures on first use)
            start()
            t = timed(run, args.steps)
            if r > 0:                                                         # round 0: capture + warm-up
                res[arm].append(t)
            if beam and r == args.rounds:                                     # the timed graph did move (or keep) the rows the arm says
                start()
                slots[arm] = moved(parent, own)
    st.beams = 0
    forced.copy_(ident)
    return {a: statistics.median(v) for a, v in res.items()}


def kernel_times(K):
    """The entries alone, back-to-back eager launches (``reorder`` is the unwrapped entry: its parent array is the one passed)."""
    tc = cfg.text_config
    L, row_bytes = tc.num_hidden_layers, tc.num_key_value_heads * tc.head_dim * 2
    out = {}
    logits = torch.randn(K, V, device=dev) * 3
    eos = torch.tensor(list(EOS) + [-1, -1], dtype=torch.int64, device=dev)
    score, tok = torch.zeros(8, device=dev), torch.zeros(8, dtype=torch.int64, device=dev)
    parent, walk = torch.zeros(8, dtype=torch.int32, device=dev), torch.zeros(ops.BEAM_WALK_WORDS, dtype=torch.int32, device=dev)
    rows = (torch.zeros(K, device=dev), torch.zeros(K, 8, dtype=torch.int32, device=dev), torch.zeros(K, 8, device=dev), torch.zeros(K, 4, device=dev))

    def step():
        score.zero_()
        ops.beam_step(logits, V, K, eos, score, tok, parent, walk, *rows)
    out["beam_step_us"] = 1e3 * timed(step, args.kernel_iters)
    out["score_zero_us"] = 1e3 * timed(score.zero_, args.kernel_iters)
    tk, lp, ti, tl = torch.zeros(K, dtype=torch.int64, device=dev), torch.zeros(1, K, device=dev), torch.zeros(1, K, 8, dtype=torch.int32, device=dev), torch.zeros(1, K, 8, device=dev)
    out["decode_logprobs_k8_us"] = 1e3 * timed(lambda: ops.decode_logprobs(logits, V, tk, 8, lp, ti, tl), args.kernel_iters)
    pos = torch.zeros(K, dtype=torch.int32, device=dev)
    out["decode_advance_us"] = 1e3 * timed(lambda: ops.decode_advance(logits, V, tk, pos), args.kernel_iters)
    cap = 512
    kv = [torch.zeros(K * cap, row_bytes // 2, dtype=torch.float16, device=dev) for _ in range(2 * L)]
    ptrs = torch.tensor([t.data_ptr() for t in kv], dtype=torch.int64, device=dev)
    cyc = torch.zeros(8, dtype=torch.int32, device=dev)
    cyc[:K] = (torch.arange(K, dtype=torch.int32) + 1) % K
    zero = torch.zeros(1, dtype=torch.int32, device=dev)
    for r in args.rows:
        held = torch.tensor([r], dtype=torch.int32, device=dev)
        bound = (r + 255) // 256 * 256
        us = 1e3 * timed(lambda: reorder(ptrs, cyc, K, zero, held, row_bytes, cap, bound), args.kernel_iters)
        moved = K * r * row_bytes * 2 * L
        out[f"beam_reorder_cycle_rows{r}_us"] = us
        out[f"beam_reorder_cycle_rows{r}_bytes_each_way"] = moved
        out[f"beam_reorder_cycle_rows{r}_TBps"] = round(2 * moved / (us * 1e-6) / 1e12, 3)
    ident = torch.arange(8, dtype=torch.int32, device=dev)
    held = torch.tensor([max(args.rows)], dtype=torch.int32, device=dev)
    k0 = kv[0].view(K, cap, -1)                                           # the cycle launches above did move rows: one more, over marks
    k0[:, 0, :] = torch.arange(1, K + 1, dtype=torch.float16, device=dev)[:, None]
    reorder(ptrs, cyc, K, zero, held, row_bytes, cap, 256)
    torch.cuda.synchronize()
    assert (k0[:, 0, 0].float().cpu() - 1).to(torch.int32).tolist() == cyc[:K].tolist()
    out["beam_reorder_identity_us"] = 1e3 * timed(lambda: reorder(ptrs, ident, K, zero, held, row_bytes, cap, 256), args.kernel_iters)
    return out


result = {"geometry": "Llama-3.1-8B (synthetic weights, fp16, fast schedule, full depth), vocab %d, prefix %d rows" % (V, P),
          "rounds": args.rounds, "steps_per_round": args.steps, "steps": {}, "kernel": {}}
for K in args.beams:
    for mode in ["shared"] + (["copy"] if K in args.copy_beams else []):
        slots = {}
        t = step_times(K, mode, slots)
        g = t["greedy"]
        pct = {a: round(100 * (t[a] / g - 1), 2) for a in t if a != "greedy"}
        result["steps"][f"K{K}_{mode}"] = {"ms": {a: round(v, 4) for a, v in t.items()}, "surcharge_over_greedy_pct": pct,
                                           "slot_held_after_one_replay": slots}
        print(f"K={K} {mode}: " + ", ".join(f"{a} {v:.4f} ms" for a, v in t.items()) + f"; over greedy: {pct}", flush=True)
        eng.release_batch_state()
for K in args.beams:
    result["kernel"][f"K{K}"] = {k: (round(v, 2) if isinstance(v, float) else v) for k, v in kernel_times(K).items()}
    print(f"K={K}: kernels {result['kernel'][f'K{K}']}", flush=True)
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
