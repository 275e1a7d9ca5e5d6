"""Scoring on the MI355X: lmi_token_logprobs at production sizes, LeopardEngine.score / score_batch, forward(labels=) and loglikelihood
against the fp32 oracle and against the all-position logits path, the lo4 selection of scored rows at full depth (tests/golden/
score_c2_full_depth.npz, tools/gen_score_fixtures.py), the memory bound of the chunked head, and Idefics2."""
import hashlib
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOGIT_TOL_F16 = 1.25e-3              # tests/test_gpu_parity.py LOGIT_TOL[f16]: mid configuration, all-position logits vs the fp32 oracle


def f64_logprobs(logits: torch.Tensor, rows: torch.Tensor, targets: torch.Tensor):
    d = logits[rows].double()
    lse = torch.logsumexp(d, dim=-1)
    return d.gather(1, targets.reshape(-1, 1))[:, 0] - lse, lse, d.argmax(dim=-1)


# ---- 1. the kernel at production sizes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [128256, 32000])
@pytest.mark.parametrize("R", [1, 7, 1024])
def test_token_logprobs_production_sizes(V, R):
    from leopard_amd.ops import Ops
    ops = Ops()
    ld = (V + 127) // 128 * 128 + 128
    g = torch.Generator(device=DEV).manual_seed(R)
    x = torch.full((R, ld), 1e30, device=DEV)
    scale = 3e4 if R == 7 else 6.0
    x[:, :V] = (torch.rand(R, V, generator=g, device=DEV) * 2 - 1) * scale
    t = torch.randint(0, V, (R,), generator=g, device=DEV)
    t[0], t[-1] = 0, V - 1
    if R > 2:
        x[1, 3] = x[1, V - 1] = x[1, 9] = 2 * scale                    # tied maxima: the lowest index
    out = []
    for _ in range(2):
        lp, lse = torch.empty(R, device=DEV), torch.empty(R, device=DEV)
        am = torch.empty(R, dtype=torch.int64, device=DEV)
        ops.token_logprobs(x, V, t, lp, lse, am)
        out.append((lp, lse, am))
    torch.cuda.synchronize()
    (lp, lse, am), (lp2, lse2, am2) = out
    assert torch.equal(lp, lp2) and torch.equal(lse, lse2) and torch.equal(am, am2)          # run-to-run bit-identical
    rp, rl, ra = f64_logprobs(x[:, :V], torch.arange(R, device=DEV), t)
    tol = 1e-5 * rl.abs().clamp_min(1.0)
    assert ((lse.double() - rl).abs() <= tol).all() and ((lp.double() - rp).abs() <= tol).all()
    assert torch.equal(am, ra)
    if R > 2:
        assert int(am[1]) == 3


# ---- a mid-size model: full-width layers, 2 + 2 layers, 8k vocabulary ----------------------------------------------------------------
@pytest.fixture(scope="module")
def mid():
    from leopard_amd import compat
    from leopard_amd.config import mid_config
    from leopard_amd.ops import Ops
    from leopard_amd.weights import SynthSource
    cfg, ops = mid_config(), Ops()
    m = compat.LeopardForConditionalGeneration(cfg, lambda dev, dt: SynthSource(cfg, ops, dev, dt), torch.float16, ops, torch_dtype=torch.float16)
    return m.to(DEV)


def mid_sample(cfg, n_images=1, seed=0, w=800, h=500):
    from tools.gen_fulldepth_fixtures import sample_inputs
    return sample_inputs(cfg, n_images, w, h, seed=seed)[:2]


def test_forward_labels_vs_oracle(mid):
    """2. forward(labels=)'s loss against the fp32 oracle's cross-entropy (its all-position logits, the 4.38 merge, the shift) in fp64."""
    from leopard_amd.tiler import siglip_normalize
    from leopard_amd.synth import synth_state_dict_numpy
    from oracle import leopard_oracle as O
    from tests.test_emu_logprob import reference_loss
    cfg = mid.config
    u8, ids = mid_sample(cfg)
    labels = ids.clone()
    labels[0, :ids.shape[1] // 3] = -100
    W = O.weights_from_numpy(synth_state_dict_numpy(cfg))
    ref_logits = O.prefill_logits(ids, torch.from_numpy(siglip_normalize(u8)), W, cfg)[0]
    ref_loss, rows, tgt, ref_lp = reference_loss(ref_logits, ids[0].tolist(), labels[0].tolist(), cfg.image_token_index, cfg.tokens_per_tile)
    out = mid.forward(ids.to(DEV), torch.from_numpy(u8).to(DEV), labels=labels.to(DEV))
    scale = float(ref_logits.abs().max())
    d = abs(float(out[0]) - float(ref_loss))
    print(f"[forward(labels=) vs fp32 oracle] loss {float(out[0]):.6f} vs {float(ref_loss):.6f}: |d| {d:.3e} "
          f"(bound {2 * LOGIT_TOL_F16 * scale:.3e}); {len(rows)} targets")
    assert out.loss is out[0] and out.loss.dtype == torch.float32
    assert d <= 2 * LOGIT_TOL_F16 * scale
    plain = mid.forward(ids.to(DEV), torch.from_numpy(u8).to(DEV))
    assert plain.loss is None and torch.equal(plain.logits, out.logits)                 # the logits are those of forward without labels


def test_score_matches_all_logits_fast(mid):
    """3. score() against a float64 log-softmax of prefill(all_logits=True) at the same rows (the fast schedule)."""
    eng = mid.engine
    u8, ids = mid_sample(mid.config, seed=3)
    labels = ids.clone()
    labels[0, :5] = -100
    res = eng.score(ids.to(DEV), torch.from_numpy(u8).to(DEV), labels.to(DEV))
    la = eng.prefill(ids.to(DEV), torch.from_numpy(u8).to(DEV), all_logits=True).logits_all
    rp, _, ra = f64_logprobs(la, res.rows, res.target_ids)
    d = (res.token_logprobs.double() - rp).abs().max().item()
    own_lp, own_am = eng.logits_logprobs(la, res.rows.cpu().numpy(), res.target_ids.cpu().numpy())
    bit = torch.equal(own_lp, res.token_logprobs)
    print(f"[score vs all_logits, fast] {res.rows.numel()} rows: max|d logprob| vs fp64 log-softmax {d:.3e}; "
          f"bit-equal to lmi_token_logprobs on the all-position logits: {bit}")
    assert d <= 2e-5 and torch.equal(res.argmax, ra)
    assert abs(float(res.loss) + float(rp.mean())) <= 2e-5


def test_score_batch_and_loglikelihood(mid):
    """4. score_batch == per-request score, bit for bit (different lengths, one request without images); loglikelihood == the sums and
    argmax flags of the corresponding score calls."""
    eng, cfg = mid.engine, mid.config
    rng = np.random.default_rng(7)
    (u8a, ida), (u8b, idb) = mid_sample(cfg, seed=1), mid_sample(cfg, seed=2, w=400, h=400)
    text = torch.from_numpy(rng.integers(1, 7000, (1, 60)))
    reqs = []
    for ids, u8 in ((ida, u8a), (text, None), (idb, u8b)):
        lab = ids.clone()
        lab[0, :ids.shape[1] - 12] = -100
        reqs.append((ids.to(DEV), None if u8 is None else torch.from_numpy(u8).to(DEV), lab))
    batch = eng.score_batch(reqs)
    singles = [eng.score(*r) for r in reqs]
    for s, b in zip(singles, batch):
        assert torch.equal(s.rows, b.rows) and torch.equal(s.target_ids, b.target_ids) and s.seq_len == b.seq_len
        assert torch.equal(s.token_logprobs, b.token_logprobs) and torch.equal(s.argmax, b.argmax) and torch.equal(s.loss, b.loss)
    ll_reqs = [(r[0][:, :-12].cpu(), r[0][:, -12:].cpu(), None if u8 is None else torch.from_numpy(u8))
               for r, u8 in zip(reqs, (u8a, None, u8b))]
    ll = mid.loglikelihood(ll_reqs, batch_size=2)
    for (lsum, greedy), s in zip(ll, singles):
        assert lsum == float(s.token_logprobs.double().sum())
        assert greedy == bool((s.argmax == s.target_ids).all())
    # a continuation made of the model's own argmax tokens is greedy
    ctx = text[:, :40]
    first = eng.score(text.to(DEV), None, torch.cat([torch.full((1, 40), -100), text[:, 40:]], dim=1))
    assert mid.loglikelihood([(ctx, first.argmax[:1].reshape(1, 1).cpu(), None)])[0][1]


def test_lo4_mid_scores_every_row(mid):
    """lo4 on a sequence of <= 1024 rows corrects every row, as before; the scores stay close to the fast schedule's."""
    eng = mid.engine
    u8, ids = mid_sample(mid.config, seed=3)
    lab = ids.clone()
    fast = eng.score(ids.to(DEV), torch.from_numpy(u8).to(DEV), lab)
    eng.precision = "lo4"
    try:
        res = eng.score(ids.to(DEV), torch.from_numpy(u8).to(DEV), lab)
        assert eng.last_lo4_ranges.tolist() == [[0, res.seq_len]]
    finally:
        eng.precision = "fast"
    assert (res.token_logprobs - fast.token_logprobs).abs().max().item() <= 0.05


# ---- 5. full depth, C2, lo4, against the oracle fixture ---------------------------------------------------------------------------------
def test_full_depth_c2_lo4_vs_fixture():
    from leopard_amd.config import full_config
    from leopard_amd.engine import LeopardEngine
    from leopard_amd.ops import Ops
    from leopard_amd.weights import EngineWeights, SynthSource
    from tools.gen_score_fixtures import score_request
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "score_c2_full_depth.npz"))
    cfg, ops = full_config(), Ops()
    u8, ids, labels = score_request(cfg)
    assert hashlib.sha256(np.ascontiguousarray(u8).tobytes()).digest() == z["tiles_sha256"].tobytes(), "tiler output drifted from the fixture"
    assert hashlib.sha256(np.ascontiguousarray(ids.numpy()).tobytes()).digest() == z["ids_sha256"].tobytes()
    W = EngineWeights.build(cfg, SynthSource(cfg, ops, torch.device(DEV), torch.float16), torch.float16)
    eng = LeopardEngine(cfg, W, ops=ops, device=torch.device(DEV))
    errs = {}
    for mode in ("fast", "lo4"):
        eng.precision = mode
        res = eng.score(ids.to(DEV), torch.from_numpy(u8).to(DEV), labels)
        assert res.seq_len == int(z["seq_len"][0]) and np.array_equal(res.rows.cpu().numpy(), z["rows"])
        assert np.array_equal(res.target_ids.cpu().numpy(), z["targets"])
        errs[mode] = (np.abs(res.token_logprobs.cpu().double().numpy() - z["logprob"]) / float(z["max_abs_logit"][0]), res.argmax.cpu().numpy())
        if mode == "lo4":
            sel = np.zeros(res.seq_len, dtype=bool)
            for b, e in eng.last_lo4_ranges:
                sel[b:e] = True
            interior = z["rows"][z["rows"] < res.seq_len - eng.LO4_TAIL_ROWS]
            assert len(interior) >= 16 and sel[interior].all() and not sel.all()     # the interior scored rows were corrected, not every row
    bound = 2e-3
    for mode, (e, am) in errs.items():
        print(f"[C2 full depth, {mode}] {len(e)} scored rows: max |d logprob| / max|logit| = {e.max():.3e} (interior rows {e[:20].max():.3e}); "
              f"argmax equal on {int((am == z['argmax']).sum())} / {len(am)}")
    e, am = errs["lo4"]
    assert e.max() <= bound
    margin = z["top2"][:, 0] - z["top2"][:, 1]
    decided = margin > 10 * bound * float(z["max_abs_logit"][0])
    assert np.array_equal(am[decided], z["argmax"][decided])


# ---- 6. memory of scoring every row of a C3-length sequence ------------------------------------------------------------------------------
def test_c3_length_all_rows_memory_and_chunking():
    """Every row of a C3-length sequence (S = 7187 text tokens: under the 4.38 merge a visual row is never a target, so only a text sequence
    of that length has every row scored), 2 + 2 layers."""
    from leopard_amd.config import full_config
    from leopard_amd.engine import LeopardEngine
    from leopard_amd.ops import Ops
    from leopard_amd.weights import EngineWeights, SynthSource
    cfg, ops = full_config(), Ops()
    cfg.vision_config.num_hidden_layers = 2
    cfg.text_config.num_hidden_layers = 2
    W = EngineWeights.build(cfg, SynthSource(cfg, ops, torch.device(DEV), torch.float16), torch.float16)
    eng = LeopardEngine(cfg, W, ops=ops, device=torch.device(DEV))
    ids = torch.from_numpy(np.random.default_rng(6).integers(1000, 100000, (1, 7187))).to(DEV)
    u8 = None
    eng.prefill(ids, u8)                                              # warm: workspaces and caches exist before the measurements
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base0 = torch.cuda.memory_allocated()
    eng.prefill(ids, u8)
    torch.cuda.synchronize()
    plain = torch.cuda.max_memory_allocated() - base0
    torch.cuda.reset_peak_memory_stats()
    base1 = torch.cuda.memory_allocated()
    res = eng.score(ids, u8, ids)
    torch.cuda.synchronize()
    scored = torch.cuda.max_memory_allocated() - base1
    S, Vp = res.seq_len, W.lm_head.shape[0]
    chunk = eng.score_chunk_rows * Vp * 4
    print(f"[C3 length, 2 + 2 layers] {res.rows.numel()} scored rows of {S}: peak over the start {scored / 2**20:.0f} MiB vs plain prefill "
          f"{plain / 2**20:.0f} MiB (+{(scored - plain) / 2**20:.0f} MiB; bound one chunk {chunk / 2**20:.0f} MiB + 256 MiB)")
    assert res.rows.numel() == S - 1
    assert scored - plain <= chunk + 256 * 2**20
    eng.score_chunk_rows = S
    whole = eng.score(ids, u8, ids)
    assert torch.equal(whole.token_logprobs, res.token_logprobs) and torch.equal(whole.argmax, res.argmax)


# ---- 7. Idefics2 -------------------------------------------------------------------------------------------------------------------------
def test_idefics2_score_matches_all_logits():
    from leopard_amd.config import idefics2_mid_config
    from leopard_amd.idefics2 import Idefics2Engine, Idefics2SynthSource, Idefics2Weights
    from leopard_amd.ops import Ops
    cfg, ops = idefics2_mid_config(), Ops()
    cfg.text_config.vocab_size = 32000
    W = Idefics2Weights.build(cfg, Idefics2SynthSource(cfg, ops, torch.device(DEV), torch.float16), torch.float16)
    eng = Idefics2Engine(cfg, W, ops=ops, device=torch.device(DEV))
    rng = np.random.default_rng(4)
    img = torch.from_numpy(rng.integers(0, 256, (378, 490, 3), dtype=np.uint8)).to(DEV)
    n_lat = cfg.perceiver_config.n_latents
    ids = torch.from_numpy(np.concatenate([rng.integers(3, 7000, 5), np.full(n_lat, cfg.image_token_id), rng.integers(3, 7000, 30)])).reshape(1, -1)
    labels = ids.clone()
    labels[0, :10] = -100
    res = eng.score(ids.to(DEV), [img], labels)
    la = eng.prefill(ids.to(DEV), [img], all_logits=True).logits_all
    rp, _, ra = f64_logprobs(la, res.rows, res.target_ids)
    d = (res.token_logprobs.double() - rp).abs().max().item()
    print(f"[Idefics2 score vs all_logits] {res.rows.numel()} rows, V = {cfg.text_config.vocab_size}: max|d| {d:.3e}")
    assert res.rows.tolist() == list(range(9, ids.shape[1] - 1))          # labels map 1:1 to the rows
    assert d <= 2e-5 and torch.equal(res.argmax, ra)


# ---- 8. nothing else moved -------------------------------------------------------------------------------------------------------------
def test_scoring_leaves_prefill_and_generate_unchanged(mid):
    eng = mid.engine
    u8, ids = mid_sample(mid.config, seed=5)
    ids, u8 = ids.to(DEV), torch.from_numpy(u8).to(DEV)
    before = eng.prefill(ids, u8, all_logits=True)
    gen0 = eng.generate(ids, u8, max_new_tokens=4, eos_token_id=())
    eng.score(ids, u8, ids)
    after = eng.prefill(ids, u8, all_logits=True)
    assert torch.equal(before.logits_all, after.logits_all) and torch.equal(before.logits_last, after.logits_last)
    assert torch.equal(eng.generate(ids, u8, max_new_tokens=4, eos_token_id=()), gen0)
