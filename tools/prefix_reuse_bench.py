#!/usr/bin/env python3
"""What continuing from a cached prefix saves (LeopardEngine.generate_shared / extend, lmi_attn_prefix_fwd) on the Llama-3.1-8B + SigLIP geometry
with synthetic weights, full depth, the C3 sample (6 x 1344x896: 7187 merged rows, 7139 of them before the question).

    python tools/prefix_reuse_bench.py [--precision lo4|fast] [--n 1,4,8,16] [--out profiles/prefix_reuse.json]
    python tools/prefix_reuse_bench.py --decode shared --n 2,16 --out profiles/prefix_reuse_shared_decode.json

For every N (questions of 48 ids about the same six pages), in ms, the median of --rounds rounds after one warm-up round, both arms in the same
process, interleaved round by round:
  a  generate_batch of the N full prompts, max_new_tokens = 1 (N tower passes, N x 7187 LLM rows)
  b  the prefix prefill into a cache of exactly P rows (one tower pass, 7139 rows)
  c  extend of the N suffixes with kv_out (N x 48 rows against the cached prefix)
  d  the copies into the decode slots (prefix rows + own rows per request)
  e  the per-token decode step after either path: (generation with 1 + --decode-tokens tokens - generation with 1 token) / --decode-tokens; the
     same captured step runs on both paths
and the kernel alone at H 32 / KV 8 / D 128, P = 7139, eight own ranges of 33 .. 300 rows: lmi_attn_prefix_fwd against lmi_attn_varlen_fwd per
sequence on a materialised [prefix ; own] copy (the copies timed separately).
--decode shared adds the shared-prefix decode arm (generate_shared(decode="shared"): ONE prefix copy in the decode state, read once per step
by lmi_attn_decode_shared) next to the copy arm, in the same rounds: its slot fill (d: one prefix copy + N own ranges), its per-token step by
the same formula as e, the K / V bytes both decode states hold, and the step saving against the byte-count prediction
(N - 1) x P x 131 072 B / 5.8 TB/s.  Times are host clock around work that ends in a device synchronise
(the calls read tokens back).  Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from leopard_amd.config import full_config  # noqa: E402
from leopard_amd.engine import KVCache, LeopardEngine  # noqa: E402
from leopard_amd.ops import Ops  # noqa: E402
from leopard_amd.weights import EngineWeights, SynthSource  # noqa: E402
from tools.gen_fulldepth_fixtures import sample_inputs  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--precision", choices=["fast", "lo4"], default="lo4")
ap.add_argument("--n", default="1,4,8,16")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--decode-tokens", type=int, default=16)
ap.add_argument("--layers", default="", help="V,L: reduced depth (a rehearsal; the committed numbers are full depth)")
ap.add_argument("--decode", choices=["copy", "shared"], default="copy", help="shared: also measure generate_shared(decode='shared') next to the copy arm")
ap.add_argument("--out", default="")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("prefix_reuse_bench.py measures on the GPU; no device found")
dev = torch.device("cuda:0")
SUFFIX = 48


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def median_of(fns, rounds):
    """{name: median ms} of the callables, interleaved round by round after one warm-up round."""
    ts = {k: [] for k in fns}
    for r in range(rounds + 1):
        for k, fn in fns.items():
            ms, _ = wall(fn)
            if r > 0:
                ts[k].append(ms)
    return {k: statistics.median(v) for k, v in ts.items()}


cfg = full_config()
if args.layers:
    cfg.vision_config.num_hidden_layers, cfg.text_config.num_hidden_layers = (int(x) for x in args.layers.split(","))
ops = Ops()
eng = LeopardEngine(cfg, EngineWeights.build(cfg, SynthSource(cfg, ops, dev, torch.float16), torch.float16), ops=ops, device=dev)
eng.precision = args.precision
u8, ids, _ = sample_inputs(cfg, 6, 1344, 896)
tiles = torch.from_numpy(u8).to(dev)
head = ids[:, :-SUFFIX].to(dev)
P = eng.merged_len(head)
rng = np.random.default_rng(0)
result = {"geometry": "Llama-3.1-8B + SigLIP (synthetic weights, fp16)", "depth": f"{cfg.vision_config.num_hidden_layers} + {cfg.text_config.num_hidden_layers} layers",
          "precision": args.precision, "sample": "C3: 6 x 1344x896", "merged_rows": eng.merged_len(ids), "prefix_rows": P, "suffix_ids": SUFFIX,
          "rounds": args.rounds, "decode_tokens": args.decode_tokens, "decode_arms": ["copy"] + (["shared"] if args.decode == "shared" else []), "per_n": {}}
T = args.decode_tokens
for N in [int(x) for x in args.n.split(",")]:
    sfx = [ids[:, -SUFFIX:].to(dev)]
    for _ in range(N - 1):
        x = rng.integers(1000, 100000, SUFFIX)
        sfx.append(torch.from_numpy(x).reshape(1, -1).to(dev))
    full = [(torch.cat([head, s], dim=1), tiles) for s in sfx]
    prefix = KVCache(cfg, P, eng.dtype, dev)
    kv = KVCache(cfg, N * SUFFIX, eng.dtype, dev)

    def prefill_prefix():
        prefix.length = 0
        eng.prefill(head, tiles, cache=prefix)

    def copies():
        if N == 1 or not eng._batch_decode_supported():
            c = eng._generation_cache(P + SUFFIX + T + 1)
            eng._move_kv(prefix, 0, P, c.k, c.v, 0)
            eng._move_kv(kv, 0, SUFFIX, c.k, c.v, P)
            return
        st = eng._batch_state(N, P + SUFFIX + T + 1)
        for j in range(N):
            eng._move_kv(prefix, 0, P, st.k, st.v, j * st.capacity)
            eng._move_kv(kv, j * SUFFIX, SUFFIX, st.k, st.v, j * st.capacity + P)

    def fill_shared():
        st = eng._shared_state(N, SUFFIX + T + 1, P)
        eng._move_kv(prefix, 0, P, st.kp, st.vp, 0)
        for j in range(N):
            eng._move_kv(kv, j * SUFFIX, SUFFIX, st.k, st.v, j * st.capacity)

    shared_arm = args.decode == "shared" and N > 1 and eng._batch_decode_supported()
    prefill_prefix()
    eng.extend(prefix, sfx, kv_out=kv)
    extra_m = {"d_slot_fill_shared_decode": fill_shared} if shared_arm else {}
    extra_d = ({"shared_decode_T": lambda: eng.generate_shared(head, tiles, sfx, max_new_tokens=1 + T, eos_token_id=(), prefix=prefix, decode="shared")}
               if shared_arm else {})
    m = median_of({**extra_m, "a_generate_batch": lambda: eng.generate_batch(full, max_new_tokens=1, eos_token_id=()),
                   "shared_total": lambda: eng.generate_shared(head, tiles, sfx, max_new_tokens=1, eos_token_id=()),
                   "b_prefix_prefill": prefill_prefix,
                   "c_extend": lambda: eng.extend(prefix, sfx, kv_out=kv),
                   "d_slot_copies": copies}, args.rounds)
    # the per-token step: the same captured graph after either path
    d = median_of({**extra_d, "batch_T": lambda: eng.generate_batch(full, max_new_tokens=1 + T, eos_token_id=()),
                   "shared_T": lambda: eng.generate_shared(head, tiles, sfx, max_new_tokens=1 + T, eos_token_id=(), prefix=prefix),
                   "shared_1": lambda: eng.generate_shared(head, tiles, sfx, max_new_tokens=1, eos_token_id=(), prefix=prefix)}, args.rounds)
    bcd = m["b_prefix_prefill"] + m["c_extend"] + m["d_slot_copies"]
    row = {k: round(v, 3) for k, v in m.items()}
    row.update(b_plus_c_plus_d=round(bcd, 3), a_over_bcd=round(m["a_generate_batch"] / bcd, 2),
               e_step_after_generate_batch=round((d["batch_T"] - m["a_generate_batch"]) / T, 3),
               e_step_after_generate_shared=round((d["shared_T"] - d["shared_1"] - m["d_slot_copies"]) / T, 3))
    if shared_arm:
        kv_bytes = lambda ts: sum(t.numel() * t.element_size() for t in ts)
        sc, ss = eng._batch_states[N], eng._batch_states[("shared", N)]
        step_copy = (d["shared_T"] - d["shared_1"] - m["d_slot_copies"]) / T
        step_shared = (d["shared_decode_T"] - d["shared_1"] - m["d_slot_fill_shared_decode"]) / T
        predicted = 1e3 * (N - 1) * P * 131072 / 5.8e12
        row.update(e_step_shared_decode=round(step_shared, 3), step_saving_ms=round(step_copy - step_shared, 3),
                   predicted_saving_ms=round(predicted, 3), saving_over_half_predicted=bool(step_copy - step_shared >= 0.5 * predicted),
                   shared_not_slower_than_copy_by_6_percent=bool(step_shared <= 1.06 * step_copy),
                   decode_state_kv_bytes_copy=kv_bytes(sc.k + sc.v), decode_state_kv_bytes_shared=kv_bytes(ss.k + ss.v + ss.kp + ss.vp),
                   decode_state_rows_copy=f"{N} x {sc.capacity}", decode_state_rows_shared=f"{ss.prefix_capacity} + {N} x {ss.capacity}",
                   hl_step=bool(ss.hl))
        print(f"N={N}: shared-prefix decode: step {step_shared:.3f} ms against copy {step_copy:.3f} ms (saving {step_copy - step_shared:.3f} ms, predicted "
              f"{predicted:.3f}); slot fill {m['d_slot_fill_shared_decode']:.2f} ms against {m['d_slot_copies']:.2f} ms; K / V bytes "
              f"{row['decode_state_kv_bytes_shared']} against {row['decode_state_kv_bytes_copy']}", flush=True)
    result["per_n"][str(N)] = row
    print(f"N={N}: a generate_batch {m['a_generate_batch']:.1f} ms | b prefix prefill {m['b_prefix_prefill']:.1f} + c extend {m['c_extend']:.1f} + d copies "
          f"{m['d_slot_copies']:.1f} = {bcd:.1f} ms (a / (b + c + d) = {row['a_over_bcd']}) | generate_shared end to end {m['shared_total']:.1f} ms | "
          f"e step: {row['e_step_after_generate_batch']} / {row['e_step_after_generate_shared']} ms", flush=True)
    del prefix, kv, full
    eng.release_batch_state()

# ---- the kernel alone ---------------------------------------------------------------------------------------------------------------------
H, KV, D, PK = 32, 8, 128, 7139
lens = [33, 64, 65, 100, 129, 200, 257, 300]
cu = [0] + [int(c) for c in np.cumsum(lens)]
g = torch.Generator(device="cpu").manual_seed(0)
qkv = torch.randn(cu[-1], (H + 2 * KV) * D, generator=g).to(torch.float16).to(dev)
q, k, v = qkv[:, :H * D], qkv[:, H * D:(H + KV) * D], qkv[:, (H + KV) * D:]
cache = torch.randn(2, PK, KV * D, generator=g).to(torch.float16).to(dev)
out = torch.empty(cu[-1], H * D, dtype=torch.float16, device=dev)
cu_t = torch.tensor(cu, dtype=torch.int32, device=dev)
cq = [torch.tensor([0, s], dtype=torch.int32, device=dev) for s in lens]
ck = [torch.tensor([0, PK + s], dtype=torch.int32, device=dev) for s in lens]
copies_kv = [None] * len(lens)


def materialise():
    for j, (a, b) in enumerate(zip(cu, cu[1:])):
        copies_kv[j] = (torch.cat([cache[0], k[a:b]]), torch.cat([cache[1], v[a:b]]))


def contiguous():
    for j, (a, b) in enumerate(zip(cu, cu[1:])):
        ops.attention(q[a:b], copies_kv[j][0], copies_kv[j][1], out[a:b], cq[j], ck[j], lens[j], H, KV, D, D ** -0.5, True)


def repeat(fn, n=20):
    return lambda: [fn() for _ in range(n)]


materialise()
km = median_of({"prefix_kernel": repeat(lambda: ops.attention_prefix(q, k, v, cache[0], cache[1], PK, out, cu_t, max(lens), H, KV, D, D ** -0.5)),
                "contiguous_kernels": repeat(contiguous), "materialise_copies": repeat(materialise)}, max(args.rounds, 5))
result["kernel"] = {"shape": f"H {H} / KV {KV} / D {D}, P = {PK}, own rows {lens}", "lmi_attn_prefix_fwd_us": round(1e3 * km["prefix_kernel"] / 20, 1),
                    "lmi_attn_varlen_fwd_on_copies_us": round(1e3 * km["contiguous_kernels"] / 20, 1),
                    "materialising_the_copies_us": round(1e3 * km["materialise_copies"] / 20, 1)}
print("kernel alone:", json.dumps(result["kernel"]), flush=True)
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
