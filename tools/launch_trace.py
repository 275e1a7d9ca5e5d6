"""Launch-trace recorder: which library entries the engine calls, in which order, with which scalar arguments — without a GPU.

Every kernel goes through ``Ops.lib.<lmi_...>``.  This script wraps the emulator build of the library (``make emu``) in a recording proxy
(entry name + every non-pointer scalar argument; a pointer is recorded as null / non-null only), drives LeopardEngine through its host
paths on the micro configuration of tests/test_emu_engine.py (LLM width 256, which the lo4 schedule needs) — and Idefics2Engine and the
tensor-parallel loop (rank 0 of 2 over a loop-back communicator) on theirs — and prints one SHA-256 per scenario.  Two commits whose engine issues the
same launches print the same hashes: the check for a refactor of the host plumbing (``--dump DIR`` writes the traces themselves).

    make emu && python tools/launch_trace.py
"""
import argparse
import ctypes
import hashlib
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np   # noqa: E402
import torch         # noqa: E402

from leopard_amd import _lib                                                            # noqa: E402
from leopard_amd.config import LeopardConfig, RopeScaling, TextConfig, VisionConfig     # noqa: E402
from leopard_amd.dist import Comm                                                       # noqa: E402
from leopard_amd.engine import KVCache, LeopardEngine, SamplingParams                   # noqa: E402
from leopard_amd.ops import Ops                                                         # noqa: E402
from leopard_amd.weights import EngineWeights, SynthSource                              # noqa: E402

EMU = os.path.join(REPO, "tools", "hipemu", "libleopard_amd_emu.so")
QUIET = ("lmi_last_error", "lmi_abi_version")        # not launches


class Recorder:
    """Stands in for the bound library: forwards every call, keeps (name, scalars) of each."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    @staticmethod
    def _scalar(a):
        if isinstance(a, ctypes.c_void_p):
            return "p" if a.value else "null"
        if isinstance(a, (bool, int, float, bytes, str)):
            return a
        if isinstance(a, ctypes._SimpleCData):
            return a.value
        return None                                   # arrays the entry fills in (workspace offsets): not an argument value

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name in QUIET:
            return fn

        def call(*args):
            self.calls.append((name,) + tuple(s for s in map(self._scalar, args) if s is not None))
            return fn(*args)
        return call


def micro_config(vit_layers=1):
    return LeopardConfig(
        vision_config=VisionConfig(hidden_size=1152, intermediate_size=100, num_hidden_layers=vit_layers, num_attention_heads=16,
                                   image_size=28, patch_size=14),
        text_config=TextConfig(hidden_size=256, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2,
                               num_key_value_heads=1, vocab_size=256, rope_scaling=RopeScaling()),
        image_token_index=250)


class LoopbackComm(Comm):
    """Rank 0 of a two-rank group without a second process: every collective hands the rank its own block back, so the tensor-parallel
    loop issues the launches of a real rank 0 (the values are not those of a two-rank run)."""
    rank, world, backend = 0, 2, "loopback"

    def all_gather(self, out, inp, stream=None):
        out.view(self.world, *inp.shape).copy_(inp.unsqueeze(0).expand(self.world, *inp.shape))

    def reduce_scatter(self, out, inp, stream=None):
        out.copy_(inp[:out.shape[0]])

    def all_reduce(self, t, stream=None):
        pass

    def broadcast(self, t, root, stream=None):
        if root != self.rank:
            t.zero_()


def tiles(seed, n):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (n, 28, 28, 3), dtype=np.uint8))


def engine(ops, vit_layers=1):
    cfg = micro_config(vit_layers)
    W = EngineWeights.build(cfg, SynthSource(cfg, ops, "cpu", torch.float16), torch.float16)
    return LeopardEngine(cfg, W, ops=ops, device="cpu")


def scenarios(ops):
    """name -> zero-argument callable: the recorded part of the scenario (engines, weights and fp8 plans are built here, outside it)."""
    ids3 = torch.tensor([[5, 250, 9, 250, 250, 17, 33]])
    samples = [(torch.tensor([[5, 250, 9, 250, 17]]), tiles(5, 2)), (torch.tensor([[7, 8, 9]]), None), (torch.tensor([[250, 3]]), tiles(6, 1))]
    text_only = [(torch.tensor([[7, 8, 9]]), None), (torch.tensor([[1, 2, 3, 4]]), None)]
    long_ids = torch.tensor([[250] + [int(v) for v in np.random.default_rng(1).integers(0, 240, 39)]])
    sp = SamplingParams(temperature=0.8, top_k=20, top_p=0.9, seed=11)
    out = {}

    def prefill(mode):
        eng = engine(ops)
        eng.precision = mode
        return lambda: eng.prefill(ids3, tiles(3, 3))
    for mode in ("fast", "lo4", "split"):
        out[f"prefill_{mode}"] = prefill(mode)

    def prefill_unfused():
        eng = engine(ops)
        eng.fuse_norm_rope = False
        return lambda: eng.prefill(ids3, tiles(3, 3), cache=None, all_logits=True)
    out["prefill_fast_unfused_all_logits"] = prefill_unfused()

    def prefill_batch(mode, smp, full_below=None):
        eng = engine(ops)
        eng.precision = mode
        if full_below is not None:                    # "auto" lo4_vit: samples above this many rows keep the fast tower -> mixed ViT flags
            eng.LO4_FULL_BELOW = full_below
        return lambda: eng.prefill_batch(smp)
    out["prefill_batch_fast"] = prefill_batch("fast", samples)
    out["prefill_batch_fast_text_only"] = prefill_batch("fast", text_only)
    out["prefill_batch_lo4"] = prefill_batch("lo4", samples)
    out["prefill_batch_lo4_mixed_tower"] = prefill_batch("lo4", samples, full_below=4)

    def score_batch(rows, n_text):
        eng = engine(ops)
        eng.precision = "lo4"
        eng.lo4_rows = rows
        ids = torch.tensor([[250] + [int(v) for v in np.random.default_rng(2).integers(0, 240, n_text)]])
        lab = torch.full_like(ids, -100)
        lab[0, 3:6] = ids[0, 3:6]
        lab[0, -2:] = ids[0, -2:]
        short = torch.tensor([[7, 8, 9, 10]])
        reqs = [(ids, tiles(7, 1), lab), (short, None, torch.tensor([[-100, -100, 9, 10]]))]
        return lambda: (eng.score_batch(reqs), eng.score(ids, tiles(7, 1), lab))
    out["score_batch_lo4_tail8"] = score_batch(8, 39)
    out["score_batch_lo4_auto_long"] = score_batch("auto", 1100)

    def gen(kind, sampling):
        eng = engine(ops)
        if kind == "generate":
            return lambda: eng.generate(long_ids[:, :6], tiles(4, 1), max_new_tokens=4, eos_token_id=(), sampling=sampling)
        if kind == "generate_batch":
            return lambda: eng.generate_batch(samples, max_new_tokens=4, eos_token_id=(), sampling=sampling)
        return lambda: eng.generate_stream(samples + text_only, batch_size=2, max_new_tokens=11, eos_token_id=(), sampling=sampling)
    for kind in ("generate", "generate_batch", "generate_stream"):
        out[f"{kind}_greedy"] = gen(kind, None)
        out[f"{kind}_sampled"] = gen(kind, sp)

    def gen_lo4():
        eng = engine(ops)
        eng.precision = "lo4"
        return lambda: (eng.generate(long_ids[:, :6], tiles(4, 1), max_new_tokens=3, eos_token_id=()),
                        eng.generate_batch(samples, max_new_tokens=3, eos_token_id=()))
    out["generate_and_batch_lo4"] = gen_lo4()

    def fp8():
        eng = engine(ops, vit_layers=2)
        eng.enable_fp8([(torch.tensor([[3, 250, 250, 8]]), tiles(9, 2))])
        return lambda: eng.prefill(ids3, tiles(3, 3), all_logits=True)
    out["prefill_fp8"] = fp8()

    # the paths a fold of the fast and lo4 layer loops rewrites: the last layer's row window, the continuation arguments, the NaViT tower of
    # Idefics2Engine and the tensor-parallel loop
    def last_layer_window(mode):
        eng = engine(ops)
        eng.precision, eng.lo4_rows = mode, 16
        ids = torch.tensor([[int(v) for v in np.random.default_rng(3).integers(0, 240, 300)]])
        return lambda: eng.prefill(ids, None, cache=KVCache(eng.cfg, 300, torch.float16, "cpu"))

    def continuation(mode):
        eng = engine(ops)
        eng.precision = mode
        sfx = [torch.tensor([[7, 8, 9]]), torch.tensor([[11, 12, 13, 14, 15]])]

        def run():
            cache = KVCache(eng.cfg, 32, torch.float16, "cpu")
            eng.prefill(ids3[:, :4], tiles(3, 2), cache=cache)
            eng.extend(cache, sfx, kv_out=KVCache(eng.cfg, 8, torch.float16, "cpu"))
            eng.append(cache, torch.tensor([[21, 22, 23]]))
            eng.generate_shared(ids3[:, :4], tiles(3, 2), sfx, max_new_tokens=3, eos_token_id=())
        return run

    def idefics2_micro():
        from leopard_amd.config import Idefics2Config, PerceiverConfig
        cfg = Idefics2Config(
            vision_config=VisionConfig(hidden_size=1152, intermediate_size=100, num_hidden_layers=1, num_attention_heads=16,
                                       image_size=56, patch_size=14),
            text_config=TextConfig(hidden_size=256, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2,
                                   num_key_value_heads=1, vocab_size=256, rope_theta=10000.0, rope_scaling=None, sliding_window=6),
            perceiver_config=PerceiverConfig(n_latents=3, depth=2, n_heads=1, head_dim=96, num_key_value_heads=1),
            image_token_id=250, longest_edge=56)
        rng = np.random.default_rng(8)
        images = [torch.from_numpy(rng.standard_normal(s).astype(np.float32)) for s in ((3, 42, 56), (3, 58, 30))]
        ids = torch.tensor([[5, 7] + [250] * 3 + [9, 11, 13] + [250] * 3 + [17, 19]])
        return cfg, images, ids

    def idefics2(mode):
        from leopard_amd.idefics2 import Idefics2Engine, Idefics2SynthSource, Idefics2Weights
        cfg, images, ids = idefics2_micro()
        eng = Idefics2Engine(cfg, Idefics2Weights.build(cfg, Idefics2SynthSource(cfg, ops, "cpu", torch.float16), torch.float16), ops=ops,
                             device="cpu")
        eng.precision = mode
        return lambda: eng.prefill(ids, images)

    def tensor_parallel(mode):
        cfg = micro_config()
        cfg.text_config = TextConfig(hidden_size=512, intermediate_size=256, num_hidden_layers=2, num_attention_heads=4,
                                     num_key_value_heads=2, vocab_size=256, rope_scaling=RopeScaling())
        W = EngineWeights.build(cfg, SynthSource(cfg, ops, "cpu", torch.float16), torch.float16, tp_rank=0, tp_size=2)
        eng = LeopardEngine(cfg, W, ops=ops, device="cpu", comm=LoopbackComm())
        eng.precision = mode
        return lambda: eng.prefill(ids3, tiles(3, 3))
    for mode in ("fast", "lo4"):
        out[f"last_layer_window_{mode}"] = last_layer_window(mode)
        out[f"extend_append_shared_{mode}"] = continuation(mode)
        out[f"idefics2_prefill_{mode}"] = idefics2(mode)
        out[f"tp_prefill_{mode}"] = tensor_parallel(mode)

    # the generation paths a fold of the first-token rule, the step runner, the slot filler and the output assembly rewrites: logprobs on
    # every entry point, a ring drain inside generate_batch, its chunking, the sequential fallback of shapes without a batched decode, every
    # arm of generate_shared and generate through the Idefics2 surface class
    def gen_logprobs(kind, sampling, k):
        eng = engine(ops)
        if kind == "generate":
            return lambda: eng.generate(long_ids[:, :6], tiles(4, 1), max_new_tokens=4, eos_token_id=(), sampling=sampling, logprobs=k)
        if kind == "generate_batch":                  # 10 steps: the rings drain after step 8 (HIST) and again at the end
            return lambda: eng.generate_batch(samples, max_new_tokens=11, eos_token_id=(), sampling=sampling, logprobs=k)
        return lambda: eng.generate_stream(samples + text_only, batch_size=2, max_new_tokens=11, eos_token_id=(), sampling=sampling, logprobs=k)
    out["generate_greedy_logprobs0"] = gen_logprobs("generate", None, 0)
    out["generate_sampled_logprobs3"] = gen_logprobs("generate", sp, 3)
    out["generate_batch_sampled_logprobs3_two_drains"] = gen_logprobs("generate_batch", sp, 3)
    out["generate_stream_greedy_logprobs2"] = gen_logprobs("generate_stream", None, 2)
    out["generate_stream_sampled_logprobs2"] = gen_logprobs("generate_stream", sp, 2)

    def gen_batch_chunks():                           # a chunk of MAX_DECODE_BATCH requests + the single-request arm
        eng = engine(ops)
        g = np.random.default_rng(4)
        reqs = [(torch.tensor([[int(v) for v in g.integers(0, 240, 3 + j % 4)]]), None) for j in range(17)]
        return lambda: eng.generate_batch(reqs, max_new_tokens=2, eos_token_id=(), logprobs=1)
    out["generate_batch_17_requests_logprobs1"] = gen_batch_chunks()

    sfx2 = [torch.tensor([[7, 8, 9]]), torch.tensor([[11, 12, 13, 14, 15]])]

    def sequential_fallback():
        eng = engine(ops)
        eng._batch_decode_supported = lambda: False
        return lambda: (eng.generate_batch(samples, max_new_tokens=11, eos_token_id=(), sampling=sp, logprobs=3),
                        eng.generate_shared(ids3[:, :4], tiles(3, 2), sfx2, max_new_tokens=3, eos_token_id=(), logprobs=0))
    out["sequential_fallback_batch_and_shared"] = sequential_fallback()

    def shared_copy():
        eng = engine(ops)
        return lambda: eng.generate_shared(ids3[:, :4], tiles(3, 2), sfx2, max_new_tokens=11, eos_token_id=(), sampling=sp, decode="copy",
                                           logprobs=2)
    out["generate_shared_copy_sampled_logprobs2"] = shared_copy()

    def shared_small():                               # one suffix: the batch-1 arm; max_new_tokens=1: no stepping
        eng = engine(ops)
        return lambda: (eng.generate_shared(ids3[:, :4], tiles(3, 2), sfx2[:1], max_new_tokens=3, eos_token_id=(), logprobs=1),
                        eng.generate_shared(ids3[:, :4], tiles(3, 2), sfx2, max_new_tokens=1, eos_token_id=(), sampling=sp, logprobs=1),
                        eng.generate_shared(ids3[:, :4], tiles(3, 2), sfx2, max_new_tokens=1, eos_token_id=()))
    out["generate_shared_one_suffix_and_one_token"] = shared_small()

    def shared_decode(sampling, k):                   # decode="shared" needs 4 query heads per KV head (the 2 : 1 micro configuration is refused)
        cfg = micro_config()
        cfg.text_config = TextConfig(hidden_size=512, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4,
                                     num_key_value_heads=1, vocab_size=256, rope_scaling=RopeScaling())
        eng = LeopardEngine(cfg, EngineWeights.build(cfg, SynthSource(cfg, ops, "cpu", torch.float16), torch.float16), ops=ops, device="cpu")
        return lambda: eng.generate_shared(ids3[:, :4], tiles(3, 2), sfx2 + [torch.tensor([[21]])], max_new_tokens=11, eos_token_id=(),
                                           sampling=sampling, decode="shared", logprobs=k)
    out["generate_shared_decode_shared_greedy"] = shared_decode(None, None)
    out["generate_shared_decode_shared_sampled_logprobs2"] = shared_decode(sp, 2)

    def idefics2_surface(kw):
        from leopard_amd.idefics2 import Idefics2SynthSource
        from leopard_amd.idefics2_compat import Idefics2ForConditionalGeneration
        cfg, images, ids = idefics2_micro()
        m = Idefics2ForConditionalGeneration(cfg, lambda dev, dt: Idefics2SynthSource(cfg, ops, dev, dt), torch.float16, ops).to("cpu")
        H, W = max(im.shape[1] for im in images), max(im.shape[2] for im in images)
        pix, mask = torch.zeros(1, len(images), 3, H, W), torch.zeros(1, len(images), H, W, dtype=torch.int64)
        for i, im in enumerate(images):
            pix[0, i, :, :im.shape[1], :im.shape[2]] = im
            mask[0, i, :im.shape[1], :im.shape[2]] = 1
        return lambda: m.generate(ids, pixel_values=pix, pixel_attention_mask=mask, max_new_tokens=4, eos_token_id=[], **kw)
    out["idefics2_surface_generate_greedy"] = idefics2_surface({})
    out["idefics2_surface_generate_sampled_logprobs2"] = idefics2_surface(dict(do_sample=True, temperature=0.8, top_k=20, top_p=0.9, seed=11,
                                                                               logprobs=2))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--only", nargs="*", help="scenario names (default: all)")
    ap.add_argument("--dump", help="directory for one text file per scenario: a call per line")
    args = ap.parse_args()
    if not os.path.exists(EMU):
        sys.exit("build the emulator library first: make emu")
    rec = Recorder(_lib.bind(EMU))
    ops = Ops(lib=rec, emulated=True)
    for name, run in scenarios(ops).items():
        if args.only and name not in args.only:
            continue
        rec.calls = []
        run()
        text = "\n".join(repr(c) for c in rec.calls)
        if args.dump:
            os.makedirs(args.dump, exist_ok=True)
            with open(os.path.join(args.dump, name + ".txt"), "w") as f:
                f.write(text + "\n")
        print(f"{name:48s} {len(rec.calls):6d} calls  sha256 {hashlib.sha256(text.encode()).hexdigest()[:16]}")


if __name__ == "__main__":
    main()
