"""-m gpu: scoring N continuations after one prefill on the MI355X — LeopardEngine.score_shared / extend_score and the loglikelihood_shared
surface on the mid model (tests/test_gpu_scoring.py builds it the same way) against the fp32 oracle's log-softmax, with both attention
launches and both schedules; the work it saves against loglikelihood of the full prompts; one full-depth case on the C2 sample."""
import os
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SUFFIX = 48                                       # synth_prompt_ids: the last 48 ids are the question and the assistant tail
LOGIT_TOL_F16 = 1.25e-3                           # tests/test_gpu_parity.py LOGIT_TOL[f16] (tests/test_gpu_scoring.py)
TOL = {"fast": LOGIT_TOL_F16, "lo4": 1.0e-3}      # tests/test_gpu_prefix.py: extend's bounds on the mid model


@pytest.fixture(scope="module")
def mid():
    from leopard_amd import compat
    from leopard_amd.config import mid_config
    from leopard_amd.ops import Ops
    from leopard_amd.weights import SynthSource
    cfg, ops = mid_config(), Ops()
    m = compat.LeopardForConditionalGeneration(cfg, lambda dev, dt: SynthSource(cfg, ops, dev, dt), torch.float16, ops, torch_dtype=torch.float16)
    return m.to(DEV)


def mid_sample(cfg, n_images=1, seed=0, w=336, h=336):
    from tools.gen_fulldepth_fixtures import sample_inputs
    u8, ids = sample_inputs(cfg, n_images, w, h, seed=seed)[:2]
    return torch.from_numpy(u8), ids


def continuations(cfg, n, seed):
    """n (tail, continuation) pairs: tails of 1 - 3 ids, continuations of 1 - 6 ids."""
    g = np.random.default_rng(seed)
    hi = min(cfg.text_config.vocab_size, 128000)

    def ids(m):
        x = g.integers(3, hi, m)
        x[x == cfg.image_token_index] = 3
        return torch.from_numpy(x).reshape(1, -1)
    return [(ids(1 + j % 3), ids(1 + (5 * j) % 6)) for j in range(n)]


@pytest.fixture(scope="module")
def oracle_case(mid):
    """One one-image prompt, 8 continuations of 1 - 6 ids, and the fp32 oracle's logits at every continuation position of every concatenated
    prompt (the towers once, the language model once per prompt) — computed once, shared by the cases below and left unchanged."""
    from leopard_amd.synth import synth_state_dict_numpy
    from leopard_amd.tiler import siglip_normalize
    from oracle import leopard_oracle as O
    cfg = mid.config
    u8, ids = mid_sample(cfg, seed=5)
    reqs = continuations(cfg, 8, seed=21)
    assert sorted({c.numel() for _, c in reqs}) == [1, 2, 3, 4, 5, 6]
    W = O.weights_from_numpy(synth_state_dict_numpy(cfg))
    with torch.no_grad():
        vis = O.projector(O.siglip_vision_tower(torch.from_numpy(siglip_normalize(u8.numpy())), W, cfg), W)
        rows = []
        for t, c in reqs:
            emb, _, pos = O.embed_and_merge(torch.cat([ids, t, c], dim=1), vis, W, cfg)
            logits = O.llama_forward(emb, pos, W, cfg)[0]
            m = c.numel()
            rows.append(logits[-m - 1:-1].clone())                   # the rows that predict c_0 .. c_{m-1}
    return u8, ids, reqs, rows


@pytest.mark.parametrize("attention", ["ranges", "rows"])
@pytest.mark.parametrize("precision", ["fast", "lo4"])
def test_score_shared_vs_the_oracle(mid, oracle_case, precision, attention):
    """Every token log-prob within 2 x tol x max|logit| of the fp32 oracle's log-softmax at that position (tol: LOGIT_TOL_F16 on the fast
    schedule, 1e-3 under lo4 — the bounds of tests/test_gpu_scoring.py and tests/test_gpu_prefix.py); the reported argmax has an oracle logit
    within that bound of the oracle's maximum; no row is left out.  The vision tower launches once."""
    u8, ids, reqs, ref_rows = oracle_case
    eng = mid.engine
    was = eng.precision
    eng.precision = precision
    towers = []
    enc = eng.encode_images
    eng.encode_images = lambda *a, **k: (towers.append(1), enc(*a, **k))[1]
    try:
        got = eng.score_shared(ids.to(DEV), u8.to(DEV), [(t.to(DEV), c.to(DEV)) for t, c in reqs], attention=attention)
        torch.cuda.synchronize()
    finally:
        eng.encode_images = enc
        eng.precision = was
    assert len(towers) == 1 and len(got) == 8
    worst_lp = worst_am = 0.0
    for (t, c), g, ref in zip(reqs, got, ref_rows):
        m = c.numel()
        assert g.rows.tolist() == list(range(t.numel() - 1, t.numel() - 1 + m)) and g.target_ids.cpu().tolist() == c.reshape(-1).tolist()
        bound = 2 * TOL[precision] * ref.abs().max().item()
        lp_ref = torch.log_softmax(ref.double(), dim=-1).gather(1, c.reshape(-1, 1))[:, 0]
        d_lp = (g.token_logprobs.cpu().double() - lp_ref).abs().max().item()
        d_am = (ref.max(dim=-1).values - ref.gather(1, g.argmax.cpu().reshape(-1, 1))[:, 0]).max().item()
        worst_lp, worst_am = max(worst_lp, d_lp / bound), max(worst_am, d_am / bound)
        print(f"[score_shared {precision} {attention}] m={m}: max|d logprob| {d_lp:.3e}, oracle max - oracle[argmax] {d_am:.3e} (bound {bound:.3e})")
        assert d_lp <= bound and d_am <= bound
    print(f"[score_shared {precision} {attention}] worst / bound: logprob {worst_lp:.3f}, argmax {worst_am:.3f}")


def test_loglikelihood_shared_saves_the_prefill_work(mid):
    """loglikelihood_shared of 8 continuations against loglikelihood of the same 8 full prompts, same process, one 1344 x 896 image (the C2
    size, 1242 merged rows: enough rows for the time to be work, not launches): median of 3 timed runs after a warm-up.  Required: shared
    <= 0.5 x full (the ratio tests/test_gpu_prefix.py requires of generate_shared); the rows through the towers fall from 8 x S to about
    S + 8 x 5 — about 0.15 of the work."""
    cfg = mid.config
    u8, ids = mid_sample(cfg, seed=2, w=1344, h=896)
    reqs = continuations(cfg, 8, seed=4)
    full = [(torch.cat([ids, t], dim=1), c, u8) for t, c in reqs]

    def timed(fn):
        out = fn()
        ts = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)), out

    t_shared, a = timed(lambda: mid.loglikelihood_shared(ids, u8, reqs))
    t_full, b = timed(lambda: mid.loglikelihood(full))
    S = mid.engine.merged_len(ids)
    print(f"[score reuse, mid model, S = {S}, 8 continuations] loglikelihood_shared {t_shared * 1e3:.1f} ms, loglikelihood {t_full * 1e3:.1f} ms: "
          f"ratio {t_shared / t_full:.3f} (required <= 0.5)")
    assert len(a) == len(b) == 8
    assert t_shared <= 0.5 * t_full
    # share_prefix=True finds the same split (every context is ids + a tail of its own): the same call, the same numbers, in request order
    assert mid.loglikelihood(full, share_prefix=True) == a


def test_full_depth_c2_rows_lo4_vs_score_batch():
    """27 SigLIP + 32 Llama-3.1-8B layers, the C2 sample, precision lo4, attention "rows": 4 continuations through score_shared against
    score_batch of the concatenated prompts — token log-probs within 2 x 1e-3 x the logit scale, argmax equal."""
    from leopard_amd.config import full_config
    from leopard_amd.engine import LeopardEngine
    from leopard_amd.ops import Ops
    from leopard_amd.weights import EngineWeights, SynthSource
    from tests.test_gpu_parity import GOLDEN, FullDepthFixture
    if not os.path.exists(os.path.join(GOLDEN, "c2_full_depth.npz")):
        pytest.skip("the C2 full-depth fixture is not available")
    fx = FullDepthFixture("c2")
    cfg, ops = full_config(), Ops()
    W = EngineWeights.build(cfg, SynthSource(cfg, ops, torch.device(DEV), torch.float16), torch.float16)
    eng = LeopardEngine(cfg, W, ops=ops, device=torch.device(DEV))
    eng.precision = "lo4"
    tiles = torch.from_numpy(fx.u8).to(DEV)
    head = fx.ids[:, :-SUFFIX]
    q = fx.ids[0, -SUFFIX:]
    reqs = [(q[:40].reshape(1, -1), q[40:].reshape(1, -1)), (q[:20].reshape(1, -1), q[20:26].reshape(1, -1))] + continuations(cfg, 2, seed=9)
    full = []
    for t, c in reqs:
        ctx = torch.cat([head, t], dim=1)
        full.append((torch.cat([ctx, c], dim=1).to(DEV), tiles, torch.cat([torch.full_like(ctx, -100), c], dim=1)))
    want = eng.score_batch(full)
    got = eng.score_shared(head.to(DEV), tiles, [(t.to(DEV), c.to(DEV)) for t, c in reqs], attention="rows")
    torch.cuda.synchronize()
    bound = 2 * 1.0e-3 * fx.ref.abs().max().item()
    P = eng.merged_len(head)
    for j, (g, w) in enumerate(zip(got, want)):
        d = (g.token_logprobs - w.token_logprobs).abs().max().item()
        print(f"[C2 full depth, lo4, rows] request {j}: {g.rows.numel()} rows, max|d logprob| vs score_batch {d:.3e} (bound {bound:.3e}); "
              f"argmax equal = {torch.equal(g.argmax, w.argmax)}")
        assert torch.equal(g.rows, w.rows - P) and torch.equal(g.target_ids, w.target_ids)
        assert d <= bound and torch.equal(g.argmax, w.argmax)
    del eng, W
    torch.cuda.empty_cache()
