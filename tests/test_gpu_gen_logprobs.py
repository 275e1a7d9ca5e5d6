"""-m gpu: generate(logprobs=k) on the MI355X — lmi_decode_logprobs at the production vocabulary (bit-equal to lmi_token_logprobs, top-k
against a stable sort in torch, run-to-run and batch independence, inside a captured graph whose ring counter advances on the device), the
four generation calls of the mid model with and without ``logprobs`` under "fast" and "lo4", the agreement of a generated token's
log-probability with what scoring the same text reports, and the Idefics2 surface."""
import numpy as np
import pytest
import torch

from tests.test_emu_gen_logprobs import INF, K, crafted_rows, random_rows, same_bits, stable_order

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SUFFIX = 48                                       # synth_prompt_ids: the last 48 ids are the question and the assistant tail


@pytest.fixture(scope="module")
def ops():
    from leopard_amd.ops import Ops
    return Ops()


# ---- the kernel ----------------------------------------------------------------------------------------------------------------------
def launch(ops, x, V, tok, k, ring=1, hist_pos=None):
    B = x.shape[0]
    lp = torch.full((ring, B), 7.0, device=DEV)
    ti = torch.full((ring, B, K), -7, dtype=torch.int32, device=DEV)
    tl = torch.full((ring, B, K), 7.0, device=DEV)
    ops.decode_logprobs(x, V, tok, k, lp, ti, tl, hist_pos=hist_pos)
    torch.cuda.synchronize()
    return lp, ti, tl


def check_rows(ops, x, V, tok, k, lp, ti, tl):
    n = tok.numel()
    rlp, rlse, am = torch.empty(n, device=DEV), torch.empty(n, device=DEV), torch.empty(n, dtype=torch.int64, device=DEV)
    ops.token_logprobs(x, V, tok, rlp, rlse, am)
    torch.cuda.synchronize()
    assert same_bits(lp, rlp), (lp, rlp)                               # lp: the bits of lmi_token_logprobs
    for b in range(x.shape[0]):
        order = stable_order(x[b, :V].cpu())[:k].to(DEV)
        m = order.numel()
        assert torch.equal(ti[b, :m].long(), order), (b, ti[b], order)
        assert same_bits(tl[b, :m], x[b, order] - rlse[b])              # logit - lse with lmi_token_logprobs' lse: the lse bits too
        assert (ti[b, m:k] == -1).all() and (tl[b, m:k] == -INF).all()
        assert (ti[b, k:] == -7).all() and (tl[b, k:] == 7.0).all()     # entries >= top_k: not written


@pytest.mark.parametrize("V,B,ld", [(128256, 1, 128256), (128256, 16, 128256), (1027, 3, 1040)])
def test_kernel_at_production_vocabulary(ops, V, B, ld):
    x, tok = random_rows(B, V, ld, seed=V + B)
    if B > 1:
        x[1, [5, 4 * 70, 70000 % V, V - 1]] = 60.0                      # ties across lanes, waves and (V = 1027) the V % 4 tail
    x, tok = x.to(DEV), tok.to(DEV)
    for k in (0, 8):
        a = launch(ops, x, V, tok, k)
        check_rows(ops, x, V, tok, k, a[0][0], a[1][0], a[2][0])
        for _ in range(2):                                              # three launches: bit-identical
            b = launch(ops, x, V, tok, k)
            assert all(same_bits(p.float(), q.float()) for p, q in zip(a, b))
    if B == 16:                                                         # a row alone == the same row as row 7 of 16
        alone = launch(ops, x[7:8].clone(), V, tok[7:8].clone(), 8)
        assert same_bits(alone[0][0, 0], a[0][0, 7]) and torch.equal(alone[1][0, 0], a[1][0, 7]) and same_bits(alone[2][0, 0], a[2][0, 7])


def test_kernel_crafted_rows(ops):
    x, V, tok = crafted_rows()
    x, tok = x.to(DEV), tok.to(DEV)
    lp, ti, tl = launch(ops, x, V, tok, 8)
    check_rows(ops, x, V, tok, 8, lp[0], ti[0], tl[0])
    assert ti[0, 0, :7].tolist() == [5, 13, 280, 1026, 6, 802, 1025]    # the lower id wins every tie
    assert ti[0, 1, 5:].tolist() == [3, 6, 7] and (tl[0, 1, 5:] == -INF).all()
    assert 77 not in ti[0, 2].tolist() and torch.isnan(lp[0, 2]) and torch.isnan(tl[0, 2]).all()
    assert (ti[0, 3] == -1).all() and (tl[0, 3] == -INF).all() and torch.isnan(lp[0, 3])
    assert ti[0, 4].tolist() == list(range(8))


def test_kernel_in_a_captured_graph_follows_the_ring(ops):
    """Captured once, replayed twice with hist_pos advanced on the device in between: slots (hist_pos - 1) mod 4 = 3, then 0."""
    from leopard_amd.engine import _capture_safe
    V, B, ring = 128256, 3, 4
    x, tok = random_rows(B, V, V, seed=9)
    x, tok = x.to(DEV), tok.to(DEV)
    hp = torch.full((B,), 4, dtype=torch.int32, device=DEV)
    lp, ti, tl = torch.full((ring, B), 7.0, device=DEV), torch.full((ring, B, K), -7, dtype=torch.int32, device=DEV), torch.full((ring, B, K), 7.0, device=DEV)
    body = lambda: ops.decode_logprobs(x, V, tok, 8, lp, ti, tl, hist_pos=hp)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream(DEV).wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with _capture_safe(), torch.cuda.graph(g):
        body()
    lp.fill_(7.0); ti.fill_(-7); tl.fill_(7.0)
    g.replay()
    torch.cuda.synchronize()
    assert not (lp[3] == 7.0).any() and (lp[:3] == 7.0).all()
    tok2 = (tok + 11) % V
    tok.copy_(tok2)                                                     # the next step's tokens, and its counter: device memory only
    hp += 1
    g.replay()
    torch.cuda.synchronize()
    one = launch(ops, x, V, tok, 8)
    assert same_bits(lp[0], one[0][0]) and torch.equal(ti[0], one[1][0]) and same_bits(tl[0], one[2][0])
    assert (lp[1:3] == 7.0).all() and (ti[1:3] == -7).all() and not (lp[3] == 7.0).any() and not same_bits(lp[3], lp[0])


# ---- the engine, mid model -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mid():
    from leopard_amd import compat
    from leopard_amd.config import mid_config
    from leopard_amd.ops import Ops
    from leopard_amd.weights import SynthSource
    cfg, ops = mid_config(), Ops()
    m = compat.LeopardForConditionalGeneration(cfg, lambda dev, dt: SynthSource(cfg, ops, dev, dt), torch.float16, ops, torch_dtype=torch.float16)
    return m.to(DEV)


def mid_sample(cfg, seed=0):
    from tools.gen_fulldepth_fixtures import sample_inputs
    u8, ids = sample_inputs(cfg, 1, 336, 336, seed=seed)[:2]
    return torch.from_numpy(u8).to(DEV), ids.to(DEV)


def text_requests(cfg, n, seed):
    g = np.random.default_rng(seed)
    out = []
    for j in range(n):
        x = g.integers(3, 7900, 33 + 5 * j)
        out.append((torch.from_numpy(x).reshape(1, -1).to(DEV), None))
    return out


def check_output(out, plain, n_prompt, k, greedy=True):
    seqs = out.sequences if isinstance(out.sequences, list) else [out.sequences]
    plain = plain if isinstance(plain, list) else [plain]
    assert len(seqs) == len(plain) == len(out.token_logprobs)
    for s, p, n, lp, ti, tl in zip(seqs, plain, n_prompt, out.token_logprobs, out.top_ids, out.top_logprobs):
        assert torch.equal(s, p), (s.tolist()[0][n:], p.tolist()[0][n:])                 # the tokens of the call without logprobs
        T = s.shape[1] - n
        assert lp.shape == (T,) and ti.shape == (T, k) and tl.shape == (T, k)            # one row per generated token
        assert torch.isfinite(lp).all() and (lp <= 0).all() and (tl[:, :-1] >= tl[:, 1:]).all()
        if greedy:                                                                       # no suppress list: the greedy token is the top entry
            assert torch.equal(ti[:, 0], s[0, n:].cpu()) and torch.equal(tl[:, 0], lp)


@pytest.mark.parametrize("precision", ["fast", "lo4"])
def test_engine_calls_with_logprobs(mid, precision):
    cfg, eng = mid.config, mid.engine
    tiles, ids = mid_sample(cfg, seed=4)
    was = eng.precision
    eng.precision = precision
    try:
        T = 12
        plain = eng.generate(ids, tiles, max_new_tokens=T, eos_token_id=())
        out = eng.generate(ids, tiles, max_new_tokens=T, eos_token_id=(), logprobs=4)
        check_output(out, plain, [ids.shape[1]], 4)
        reqs = text_requests(cfg, 3, seed=1)
        n = [r[0].shape[1] for r in reqs]
        check_output(eng.generate_batch(reqs, max_new_tokens=T, eos_token_id=(), logprobs=4),
                     eng.generate_batch(reqs, max_new_tokens=T, eos_token_id=()), n, 4)
        reqs = text_requests(cfg, 5, seed=2)
        n = [r[0].shape[1] for r in reqs]
        check_output(eng.generate_stream(reqs, batch_size=2, max_new_tokens=T, eos_token_id=(), logprobs=4),
                     eng.generate_stream(reqs, batch_size=2, max_new_tokens=T, eos_token_id=()), n, 4)
        head = ids[:, :-SUFFIX]
        sfx = [ids[:, -SUFFIX:]] + [r[0] for r in text_requests(cfg, 2, seed=3)]
        n = [head.shape[1] + s.shape[1] for s in sfx]
        for decode in ("copy", "shared"):
            check_output(eng.generate_shared(head, tiles, sfx, max_new_tokens=T, eos_token_id=(), decode=decode, logprobs=4),
                         eng.generate_shared(head, tiles, sfx, max_new_tokens=T, eos_token_id=(), decode=decode), n, 4)
    finally:
        eng.precision = was
        eng.release_batch_state()


def test_sampled_stream_with_logprobs(mid):
    """Sampled, an eos id that stops requests early, logprobs=8: the tokens of the call without logprobs, one row per token."""
    cfg = mid.config
    reqs = text_requests(cfg, 5, seed=5)
    n = [r[0].shape[1] for r in reqs]
    kw = dict(batch_size=2, max_new_tokens=12, do_sample=True, temperature=4.0, top_k=0, top_p=0.98, seed=11)
    free = mid.generate_stream(reqs, eos_token_id=[], **kw)
    eos = [int(free[1][0, n[1] + 5])]
    plain = mid.generate_stream(reqs, eos_token_id=eos, **kw)
    got = mid.generate_stream(reqs, eos_token_id=eos, logprobs=8, **kw)
    assert plain[1].shape[1] <= n[1] + 6
    for g, p, m in zip(got, plain, n):
        assert torch.equal(g.sequences, p) and g.token_logprobs.shape == (p.shape[1] - m,) and g.top_token_ids.shape == (p.shape[1] - m, 8)
        assert g.sequence_logprob == float(g.token_logprobs.to(torch.float64).sum())
    mid.engine.release_batch_state()


def test_generated_logprobs_agree_with_score(mid, ops):
    """A generated token's log-probability against what scoring [prompt ; generated] reports for it.  The two come from different logits
    rows — the decode step's and the prefill's — and log-softmax moves by at most twice the largest logit change, so the bound is
    2 * max_i |logit_i(prefill) - logit_i(step)| + 1e-5 per token; against the step's own row the value is bit-equal to lmi_token_logprobs."""
    from leopard_amd.engine import KVCache
    cfg, eng = mid.config, mid.engine
    tiles, ids = mid_sample(cfg, seed=6)
    T, n, V = 10, ids.shape[1], cfg.text_config.vocab_size
    out = eng.generate(ids, tiles, max_new_tokens=T, eos_token_id=(), logprobs=0)
    toks = out.sequences[0, n:]
    S = eng.merged_len(ids)
    whole = eng.prefill(out.sequences, tiles, all_logits=True).logits_all          # [S + T, V]: row S - 1 + t predicts generated token t
    cache = KVCache(cfg, S + T, eng.dtype, DEV)
    steps = [eng.prefill(ids, tiles, cache=cache).logits_last.clone()]
    for t in toks[:-1].tolist():
        steps.append(eng.decode_step(int(t), cache).clone())
    steps = torch.stack(steps)
    lp_step, _ = eng.logits_logprobs(steps, np.arange(T), toks.cpu().numpy())
    lp_score, _ = eng.logits_logprobs(whole, np.arange(S - 1, S - 1 + T), toks.cpu().numpy())
    gen = out.token_logprobs[0]
    assert torch.equal(gen, lp_step.cpu())
    gap = (gen.double() - lp_score.cpu().double()).abs()
    bound = 2 * (whole[S - 1:S - 1 + T, :V] - steps[:, :V]).abs().max(dim=1).values.cpu().double() + 1e-5
    print(f"[generate(logprobs) vs score] largest |token logprob gap| {gap.max():.3e} (its bound {bound[gap.argmax()]:.3e}; "
          f"largest logit change between the prefill's and the step's rows {(bound.max() - 1e-5) / 2:.3e})")
    assert (gap <= bound).all(), (gap, bound)


def test_a_different_k_captures_the_logprobs_step_again(mid, monkeypatch):
    """The captured steps of one decode state across calls: the same k replays the logprobs step it captured (the Python body ran twice in
    all, warm-up and capture); a different k — top_k is a launch argument — captures a new one and leaves the greedy step's graph alone; a
    greedy call in between replays that old graph."""
    cfg, eng = mid.config, mid.engine
    ids = text_requests(cfg, 1, seed=7)[0][0]
    gen = lambda k: eng.generate(ids, None, max_new_tokens=4, eos_token_id=(), logprobs=k)
    plain = gen(None)
    gen(1)                                                              # whatever k the earlier tests left behind: now it is 1
    st = eng._gen_cache._decode_state
    greedy = st.graphs[(False, False)]
    assert greedy is not None and st.lp_k == 1
    bodies = []
    real = eng._decode_body
    monkeypatch.setattr(eng, "_decode_body", lambda s, cache: (bodies.append(s.logprobs), real(s, cache))[1])
    two = gen(2)
    g2 = st.graphs[(False, True)]
    assert g2 is not None and bodies == [2, 2]                          # warm-up + capture; the other steps are replays
    again = gen(2)
    assert st.graphs[(False, True)] is g2 and bodies == [2, 2]          # same k: the same object, no Python body
    assert torch.equal(gen(None), plain) and st.graphs[(False, False)] is greedy and st.graphs[(False, True)] is g2 and bodies == [2, 2]
    three = gen(3)
    g3 = st.graphs[(False, True)]
    assert g3 is not None and g3 is not g2 and bodies == [2, 2, 3, 3] and st.lp_k == 3
    assert st.graphs[(False, False)] is greedy                          # the greedy step was not captured again ...
    assert torch.equal(gen(None), plain) and bodies == [2, 2, 3, 3]     # ... and still replays
    assert eng._gen_cache._decode_state is st
    for out, k in ((two, 2), (again, 2), (three, 3)):
        assert torch.equal(out.sequences, plain) and out.top_ids[0].shape == (4, k)
    assert torch.equal(two.token_logprobs[0], again.token_logprobs[0]) and torch.equal(two.token_logprobs[0], three.token_logprobs[0])
    assert torch.equal(three.top_ids[0][:, :2], two.top_ids[0])


def test_idefics2_surface(ops):
    """Idefics2 (sliding window, a suppress_tokens list): tokens as without logprobs; a suppressed id is never generated."""
    from leopard_amd import idefics2_compat as IC, sampling
    from leopard_amd.config import idefics2_mid_config
    from leopard_amd.idefics2 import Idefics2SynthSource
    cfg = idefics2_mid_config()
    m = IC.Idefics2ForConditionalGeneration(cfg, lambda dev, dt: Idefics2SynthSource(cfg, ops, dev, dt), torch.float16, ops, eos_token_id=(2,)).to(DEV)
    assert m.engine.suppress_tokens is not None and cfg.text_config.sliding_window
    ids = torch.from_numpy(np.random.default_rng(2).integers(3, 7000, (1, 12))).to(DEV)
    plain = m.generate(ids, max_new_tokens=8)
    out = m.generate(ids, max_new_tokens=8, logprobs=2)
    assert isinstance(out, sampling.GenerationLogprobs) and torch.equal(out.sequences, plain)
    T = plain.shape[1] - 12
    assert out.token_logprobs.shape == (T,) and out.top_token_ids.shape == (T, 2) and torch.isfinite(out.token_logprobs).all()
    assert not (set(plain[0, 12:].tolist()) & set(m.bad_words_ids))
    assert (out.token_logprobs <= out.top_logprobs[:, 0]).all()
    hit = out.top_token_ids[:, 0] == plain[0, 12:].cpu()                # where the top entry is not suppressed it IS the greedy token
    banned = torch.isin(out.top_token_ids[:, 0], torch.tensor(m.bad_words_ids))
    assert (hit | banned).all()
    assert out.sequence_logprob == float(out.token_logprobs.to(torch.float64).sum())
