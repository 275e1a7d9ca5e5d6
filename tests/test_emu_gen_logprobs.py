"""generate(logprobs=k) on the CPU: lmi_decode_logprobs through the kernel-logic emulator (bit-equal to lmi_token_logprobs on the same rows,
top-k against a stable sort, ties, -inf, NaN, the ring slot, the argument checks), the engine's four generation calls with and without
``logprobs`` on a micro configuration (4 query heads on 1 KV head, hidden 512: every decode path including the shared-prefix step), and the
generate() surfaces."""
import numpy as np
import pytest
import torch

from leopard_amd.engine import GenerateOutput, KVCache, SamplingParams
from tests.emu_util import emu_ops

K = 8                                                                 # LMI_MAX_TOP_LOGPROBS
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def ops():
    return emu_ops()


# ---- the kernel ----------------------------------------------------------------------------------------------------------------------
def launch(ops, x, V, tok, k, ring=1, hist_pos=None):
    """The three outputs, pre-filled with sentinels (7.0 / -7)."""
    B = x.shape[0]
    lp, ti, tl = torch.full((ring, B), 7.0), torch.full((ring, B, K), -7, dtype=torch.int32), torch.full((ring, B, K), 7.0)
    ops.decode_logprobs(x, V, tok, k, lp, ti, tl, hist_pos=hist_pos)
    return lp, ti, tl


def scored(ops, x, V, tok):
    n = tok.numel()
    lp, lse, am = torch.empty(n), torch.empty(n), torch.empty(n, dtype=torch.int64)
    ops.token_logprobs(x, V, tok, lp, lse, am)
    return lp, lse


def same_bits(a, b):
    """fp32 equality that takes NaN == NaN."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(a[~na], b[~nb])


def stable_order(row):
    """ids of a row by value descending, id ascending, NaN left out."""
    nan = torch.isnan(row)
    order = torch.sort(torch.where(nan, torch.tensor(-INF), row), descending=True, stable=True).indices
    return order[~nan[order]]


def check_rows(ops, x, V, tok, k, lp, ti, tl):
    """lp [B], ti / tl [B, 8] of one launch against lmi_token_logprobs and the stable sort."""
    rlp, rlse = scored(ops, x, V, tok)
    assert same_bits(lp, rlp), (lp, rlp)
    for b in range(x.shape[0]):
        order = stable_order(x[b, :V])[:k]
        n = order.numel()
        assert ti[b, :n].tolist() == order.tolist(), (b, ti[b], order)
        assert same_bits(tl[b, :n], x[b, order] - rlse[b])              # logit - lse with lmi_token_logprobs' lse: bit-equal lse
        assert (ti[b, n:k] == -1).all() and (tl[b, n:k] == -INF).all()  # fewer than k entries: fillers
        assert (ti[b, k:] == -7).all() and (tl[b, k:] == 7.0).all()     # entries >= top_k: not written


def random_rows(B, V, ld, seed, scale=4.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.full((B, ld), NAN)                                        # the padding columns hold NaN: they are never read
    x[:, :V] = torch.randn(B, V, generator=g) * scale
    tok = torch.randint(0, V, (B,), generator=g)
    return x, tok


@pytest.mark.parametrize("V", [5, 255, 256, 1027])
@pytest.mark.parametrize("B", [1, 3])
def test_kernel_vs_token_logprobs_and_stable_sort(ops, V, B):
    x, tok = random_rows(B, V, (V + 3) // 4 * 4 + 8, seed=V * 7 + B)
    assert float(x[:, :V].double().logsumexp(-1).abs().max()) < 40      # (sanity of the float64 side)
    for k in (0, 1, 3, 8):
        lp, ti, tl = launch(ops, x, V, tok, k)
        check_rows(ops, x, V, tok, k, lp[0], ti[0], tl[0])
    # against float64 as well: the shared scan is the scored one
    lp, ti, tl = launch(ops, x, V, tok, 8)
    d = x[:, :V].double()
    want = d.gather(1, tok.reshape(-1, 1))[:, 0] - d.logsumexp(-1)
    assert (lp[0].double() - want).abs().max() <= 1e-5


def crafted_rows():
    """V = 1027, 512 threads: element e sits in the 16-byte vector e // 4 of thread (e // 4) % 512 (lane = thread % 64, wave = thread // 64);
    elements 1024 .. 1026 are the V % 4 tail of threads 0 .. 2."""
    V, ld = 1027, 1032
    x, tok = random_rows(6, V, ld, seed=3)
    x[0, [5, 13, 280, 1026]] = 50.0                                     # ties across lanes (threads 1 / 3), waves (thread 70) and the tail
    x[0, [1025, 6, 4 * 200 + 2]] = 49.0                                 # a second group: tail first in memory, lowest id still wins
    x[1, 6:] = -INF                                                     # five finite entries (0, 1, 2, 4, 5), then real -inf entries by id
    x[1, 3] = -INF
    x[2, 77] = NAN                                                      # one NaN: lse is NaN, id 77 never enters
    x[3, :V] = NAN                                                      # nothing but NaN
    x[4, :V] = 1.5                                                      # every entry tied: ids 0 .. 7
    tok = torch.tensor([13, 2, 5, 0, 1026, 9])
    return x, V, tok


def test_kernel_crafted_rows(ops):
    x, V, tok = crafted_rows()
    lp, ti, tl = launch(ops, x, V, tok, 8)
    check_rows(ops, x, V, tok, 8, lp[0], ti[0], tl[0])
    assert ti[0, 0, :7].tolist() == [5, 13, 280, 1026, 6, 802, 1025]    # the lower id wins every tie
    assert sorted(ti[0, 1, :5].tolist()) == [0, 1, 2, 4, 5] and ti[0, 1, 5:].tolist() == [3, 6, 7]    # -inf entries follow the finite ones, lowest id first
    assert torch.isfinite(tl[0, 1, :5]).all() and (tl[0, 1, 5:] == -INF).all() and torch.isfinite(lp[0, 1])
    assert 77 not in ti[0, 2].tolist() and torch.isnan(lp[0, 2]) and torch.isnan(tl[0, 2]).all()
    assert (ti[0, 3] == -1).all() and (tl[0, 3] == -INF).all() and torch.isnan(lp[0, 3])
    assert ti[0, 4].tolist() == list(range(8))
    # V = 5, k = 8: three fillers
    x5, tok5 = random_rows(1, 5, 8, seed=11)
    lp5, ti5, tl5 = launch(ops, x5, 5, tok5, 8)
    assert ti5[0, 0, 5:].tolist() == [-1, -1, -1] and (tl5[0, 0, 5:] == -INF).all() and (ti5[0, 0, :5] >= 0).all()
    # tok out of range: NaN, as lmi_token_logprobs
    for bad in (-1, V, 1 << 40):
        lpb, _, _ = launch(ops, x[:1], V, torch.tensor([bad]), 2)
        assert torch.isnan(lpb[0, 0])


def test_kernel_ring_slot_and_untouched_entries(ops):
    x, V, tok = crafted_rows()
    x, tok = x[:3], tok[:3]
    ring = 4
    for hp, slots in (([1, 2, 3], [0, 1, 2]), ([4, 5, 9], [3, 0, 0]), ([0, 8, 6], [3, 3, 1])):     # (hist_pos - 1) mod ring, wrap-around included
        lp, ti, tl = launch(ops, x, V, tok, 3, ring=ring, hist_pos=torch.tensor(hp, dtype=torch.int32))
        one = launch(ops, x, V, tok, 3)
        for b, s in enumerate(slots):
            assert same_bits(lp[s, b], one[0][0, b]) and torch.equal(ti[s, b], one[1][0, b]) and same_bits(tl[s, b], one[2][0, b])
            other = [r for r in range(ring) if r != s]
            assert (lp[other, b] == 7.0).all() and (ti[other, b] == -7).all() and (tl[other, b] == 7.0).all()    # other steps' slots: untouched
    lp, ti, tl = launch(ops, x, V, tok, 3, ring=ring)                   # null hist_pos: slot 0
    assert (lp[1:] == 7.0).all() and not (lp[0] == 7.0).any()


def test_kernel_row_does_not_depend_on_batch_or_run(ops):
    V = 1027
    x, tok = random_rows(3, V, 1032, seed=21)
    x[2, [9, 600, 1024]] = 30.0
    a = launch(ops, x, V, tok, 8)
    for _ in range(2):                                                  # three launches: bit-identical
        b = launch(ops, x, V, tok, 8)
        assert all(same_bits(p.float(), q.float()) for p, q in zip(a, b))
    alone = launch(ops, x[2:3].clone(), V, tok[2:3], 8)                 # B = 1 against row 2 of B = 3
    assert same_bits(alone[0][0, 0], a[0][0, 2]) and torch.equal(alone[1][0, 0], a[1][0, 2]) and same_bits(alone[2][0, 0], a[2][0, 2])


def test_kernel_argument_checks_launch_nothing(ops):
    import ctypes as C
    V = 64
    x, tok = random_rows(2, V, 64, seed=1)
    good = []
    check = ops._check
    ops._check = lambda rc: (good.append(1) if rc == 0 else None, check(rc))[1]
    lp, ti, tl = torch.full((1, 2), 7.0), torch.full((1, 2, K), -7, dtype=torch.int32), torch.full((1, 2, K), 7.0)
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    raw = lambda lg=x, tk=tok, ring=1, k=2, o1=lp, o2=ti, o3=tl, vocab=V, ld=64: ops._check(ops.lib.lmi_decode_logprobs(
        p(lg), 2, vocab, ld, p(tk), p(None), ring, k, p(o1), p(o2), p(o3), C.c_void_p(0)))
    try:
        for kw in (dict(lg=None), dict(tk=None), dict(o1=None), dict(o2=None), dict(o3=None),                    # null pointers
                   dict(k=-1), dict(k=9), dict(ring=0), dict(ring=-3), dict(vocab=65), dict(vocab=61, ld=60), dict(vocab=0)):
            with pytest.raises(RuntimeError, match="lmi_decode_logprobs"):
                raw(**kw)
        with pytest.raises(RuntimeError, match="lmi_decode_logprobs"):
            ops.decode_logprobs(x, 65, tok, 2, lp, ti, tl)              # through the wrapper: ld_logits < vocab
        with pytest.raises(RuntimeError, match="top_k"):
            ops.decode_logprobs(x, V, tok, 9, lp, ti, tl)
        assert not good                                                 # no call got as far as a launch
        assert (lp == 7.0).all() and (ti == -7).all() and (tl == 7.0).all()
        raw()                                                           # the same call with good arguments does launch
        assert len(good) == 1 and not (lp == 7.0).any()
    finally:
        ops._check = check


# ---- the engine ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def micro(ops):
    from tests.test_emu_shared_decode import _engine_setup
    cfg, eng, u8, ids = _engine_setup(ops, torch.float16)               # hidden 512, 4 query heads on 1 KV head: every decode path exists
    assert eng._batch_decode_supported()
    return cfg, eng, u8, ids


SP = SamplingParams(temperature=0.9, top_k=20, top_p=0.95, seed=7)


def check_output(out, plain, n_prompt, k):
    """A GenerateOutput against the same call without logprobs: equal tokens, one row per generated token."""
    assert isinstance(out, GenerateOutput)
    seqs = out.sequences if isinstance(out.sequences, list) else [out.sequences]
    plain = plain if isinstance(plain, list) else [plain]
    assert len(seqs) == len(plain) == len(out.token_logprobs) == len(out.top_ids) == len(out.top_logprobs)
    for s, p, n, lp, ti, tl in zip(seqs, plain, n_prompt, out.token_logprobs, out.top_ids, out.top_logprobs):
        assert torch.equal(s, p), (s.tolist(), p.tolist())
        T = s.shape[1] - n
        assert lp.shape == (T,) and lp.dtype == torch.float32 and ti.shape == (T, k) and tl.shape == (T, k) and tl.dtype == torch.float32
        assert not ti.dtype.is_floating_point
        assert torch.isfinite(lp).all() and (lp <= 0).all()
        if k:
            assert (tl[:, :-1] >= tl[:, 1:]).all() and (ti >= 0).all()
            assert (lp <= tl[:, 0]).all()                               # nothing is more likely than the top entry


@pytest.mark.parametrize("sampling", [None, SP], ids=["greedy", "sampled"])
def test_generate_and_per_step_bits(micro, ops, sampling):
    """generate(logprobs=k): the tokens of generate(); token_logprobs[t] is bit for bit lmi_token_logprobs of the logits row the token was
    chosen from — the prefill row, then the rows decode_step returns when the generated tokens are replayed."""
    cfg, eng, u8, ids = micro
    T, n = 5, ids.shape[1]
    plain = eng.generate(ids, u8, max_new_tokens=T, eos_token_id=(), sampling=sampling)
    out = eng.generate(ids, u8, max_new_tokens=T, eos_token_id=(), sampling=sampling, logprobs=3)
    check_output(out, plain, [n], 3)
    toks = out.sequences[0, n:]
    if sampling is None:
        assert torch.equal(out.top_ids[0][:, 0], toks)                   # greedy, no suppress list: the token is the top entry
    V = cfg.text_config.vocab_size
    cache = KVCache(cfg, eng.merged_len(ids) + T, eng.dtype, "cpu")
    rows = [eng.prefill(ids, u8, cache=cache).logits_last.clone()]
    for t in toks[:-1].tolist():
        rows.append(eng.decode_step(int(t), cache).clone())
    x = torch.stack(rows)
    want, lse = scored(ops, x, V, toks.clone())
    assert torch.equal(out.token_logprobs[0], want)
    for t in range(T):
        order = stable_order(x[t])[:3]
        assert out.top_ids[0][t].tolist() == order.tolist() and torch.equal(out.top_logprobs[0][t], x[t, order] - lse[t])
    # an early stop on eos: as many rows as tokens
    eos = (int(toks[2]),)
    cut = eng.generate(ids, u8, max_new_tokens=T, eos_token_id=eos, sampling=sampling, logprobs=0)
    stop = toks.tolist().index(eos[0]) + 1
    assert cut.sequences.shape[1] == n + stop and cut.token_logprobs[0].shape == (stop,) and cut.top_ids[0].shape == (stop, 0)
    assert torch.equal(cut.token_logprobs[0], out.token_logprobs[0][:stop])


def requests_of(ids, u8):
    """One request with images, four short text-only ones (the emulated vision tower is the slow part of a request)."""
    g = torch.Generator().manual_seed(17)
    return [(ids, u8)] + [(torch.randint(3, 240, (1, 9 + 3 * j), generator=g), None) for j in range(4)]


@pytest.mark.parametrize("sampling", [None, SP], ids=["greedy", "sampled"])
def test_generate_batch(micro, sampling):
    """10 new tokens: nine steps, so the rings are drained once full (HIST = 8) and once at the end."""
    cfg, eng, u8, ids = micro
    reqs = requests_of(ids, u8)[:3]
    n = [r[0].shape[1] for r in reqs]
    plain = eng.generate_batch(reqs, max_new_tokens=10, eos_token_id=(), sampling=sampling)
    out = eng.generate_batch(reqs, max_new_tokens=10, eos_token_id=(), sampling=sampling, logprobs=2)
    check_output(out, plain, n, 2)
    eos = (int(plain[1][0, n[1] + 3]),)                                 # request 1 stops at its fourth token; the others ride on
    cut_plain = eng.generate_batch(reqs, max_new_tokens=10, eos_token_id=eos, sampling=sampling)
    cut = eng.generate_batch(reqs, max_new_tokens=10, eos_token_id=eos, sampling=sampling, logprobs=2)
    check_output(cut, cut_plain, n, 2)
    assert cut.token_logprobs[1].numel() <= 4
    for j in range(3):                                                  # the rows of the kept tokens are the rows of the uncut run
        m = cut.token_logprobs[j].numel()
        assert torch.equal(cut.token_logprobs[j], out.token_logprobs[j][:m]) and torch.equal(cut.top_ids[j], out.top_ids[j][:m])


@pytest.mark.parametrize("batch_size,sampling", [(2, None), (3, SP)], ids=["b2-greedy", "b3-sampled"])
def test_generate_stream(micro, batch_size, sampling):
    """Five requests over 2 / 3 slots, 10 new tokens: slots are re-admitted and a request's tokens span two windows.  The sampled run also
    stops requests early on an eos id (the greedy tokens of the micro model are one repeated id: no selective eos there)."""
    cfg, eng, u8, ids = micro
    reqs = requests_of(ids, u8)
    n = [r[0].shape[1] for r in reqs]
    plain = eng.generate_stream(reqs, batch_size=batch_size, max_new_tokens=10, eos_token_id=(), sampling=sampling)
    eos = ()
    if sampling is not None:
        eos = (int(plain[3][0, n[3] + 4]),)                             # request 3 stops at its fifth token at the latest
        plain = [torch.tensor([cut_at(p[0].tolist(), m, eos[0])]) for p, m in zip(plain, n)]       # the stop rule only truncates
    out = eng.generate_stream(reqs, batch_size=batch_size, max_new_tokens=10, eos_token_id=eos, sampling=sampling, logprobs=8)
    check_output(out, plain, n, 8)
    assert max(t.numel() for t in out.token_logprobs) == 10
    if sampling is not None:
        assert out.token_logprobs[3].numel() <= 5


def cut_at(seq, n_prompt, eos):
    new = seq[n_prompt:]
    return seq[:n_prompt] + (new[:new.index(eos) + 1] if eos in new else new)


@pytest.mark.parametrize("decode", ["copy", "shared"])
def test_generate_shared(micro, decode):
    cfg, eng, u8, ids = micro
    head = ids[:, :-48]
    sfx = [ids[:, -48:], ids[:, -48:-20], torch.tensor([[9, 8, 7, 6, 5]])]
    n = [head.shape[1] + s.shape[1] for s in sfx]
    for sampling in (None, SP):
        plain = eng.generate_shared(head, u8, sfx, max_new_tokens=4, eos_token_id=(), sampling=sampling, decode=decode)
        out = eng.generate_shared(head, u8, sfx, max_new_tokens=4, eos_token_id=(), sampling=sampling, decode=decode, logprobs=4)
        check_output(out, plain, n, 4)
        if sampling is None:
            for j in range(3):
                assert torch.equal(out.top_ids[j][:, 0], out.sequences[j][0, n[j]:])


def count_launches(ops, fn):
    n = []
    check = ops._check
    ops._check = lambda rc: (n.append(1), check(rc))[1]
    try:
        res = fn()
    finally:
        ops._check = check
    return len(n), res


# launches of these two calls counted on the commit before ``logprobs`` existed (same micro model, same requests, through ops._check)
LAUNCHES_BEFORE = {"generate": 66, "generate_batch": 74}


def test_default_call_is_unchanged(micro, ops):
    """Without ``logprobs`` a call launches exactly what it launched before the argument existed (the recorded counts); with it, exactly
    one more launch per generated token; the tokens are the same."""
    cfg, eng, u8, ids = micro
    T = 4
    n0, plain = count_launches(ops, lambda: eng.generate(ids, u8, max_new_tokens=T, eos_token_id=()))
    n1, none = count_launches(ops, lambda: eng.generate(ids, u8, max_new_tokens=T, eos_token_id=(), logprobs=None))
    n2, with_lp = count_launches(ops, lambda: eng.generate(ids, u8, max_new_tokens=T, eos_token_id=(), logprobs=8))
    assert n0 == n1 == LAUNCHES_BEFORE["generate"] and torch.equal(plain, none) and isinstance(none, torch.Tensor)
    assert n2 == n0 + T and torch.equal(with_lp.sequences, plain)
    reqs = requests_of(ids, u8)[:2]
    b0, bp = count_launches(ops, lambda: eng.generate_batch(reqs, max_new_tokens=T, eos_token_id=()))
    b1, bn = count_launches(ops, lambda: eng.generate_batch(reqs, max_new_tokens=T, eos_token_id=(), logprobs=None))
    b2, bl = count_launches(ops, lambda: eng.generate_batch(reqs, max_new_tokens=T, eos_token_id=(), logprobs=1))
    assert b0 == b1 == LAUNCHES_BEFORE["generate_batch"] and all(torch.equal(a, b) for a, b in zip(bp, bn)) and isinstance(bn, list)
    assert b2 == b0 + T and all(torch.equal(a, b) for a, b in zip(bp, bl.sequences))      # one eager launch for the first tokens + T - 1 steps


def test_refusals_before_any_launch(micro, ops):
    cfg, eng, u8, ids = micro
    head, sfx = ids[:, :-48], [ids[:, -48:], ids[:, -48:-20]]
    calls = [lambda k: eng.generate(ids, u8, max_new_tokens=2, logprobs=k),
             lambda k: eng.generate_batch([(ids, u8), (ids, u8)], max_new_tokens=2, logprobs=k),
             lambda k: eng.generate_stream([(ids, u8), (ids, u8)], batch_size=2, max_new_tokens=2, logprobs=k),
             lambda k: eng.generate_shared(head, u8, sfx, max_new_tokens=2, logprobs=k)]

    def refuse():
        for call in calls:
            for bad in (9, -1, 2.0, True):
                with pytest.raises(ValueError, match="logprobs"):
                    call(bad)
        eng.W.tp_size = 2
        try:
            for call in calls:
                with pytest.raises(NotImplementedError, match="tensor-parallel"):
                    call(2)
        finally:
            eng.W.tp_size = 1
    n, _ = count_launches(ops, refuse)
    assert n == 0


# ---- the surfaces --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(ops):
    from leopard_amd import compat
    from leopard_amd.weights import SynthSource
    from tests.test_emu_engine import micro_config
    cfg = micro_config()
    m = compat.LeopardForConditionalGeneration(cfg, lambda dev, dt: SynthSource(cfg, ops, dev, dt), torch.float16, ops, torch_dtype=torch.float16)
    return m.to("cpu").eval()


def test_compat_surfaces(model, ops):
    from leopard_amd import sampling
    from leopard_amd.synth import synth_prompt_ids
    cfg = model.config
    u8 = torch.from_numpy(np.random.default_rng(31).integers(0, 256, (2, 28, 28, 3), dtype=np.uint8))
    ids = torch.from_numpy(synth_prompt_ids([2], cfg, n_question=32)).reshape(1, -1)
    plain = model.generate(ids, pixel_values=u8, max_new_tokens=3, eos_token_id=[])
    out = model.generate(ids, pixel_values=u8, max_new_tokens=3, eos_token_id=[], logprobs=2)
    assert isinstance(plain, torch.Tensor) and isinstance(out, sampling.GenerationLogprobs) and torch.equal(out.sequences, plain)
    assert out.token_logprobs.shape == (3,) and out.top_token_ids.shape == (3, 2) and out.top_logprobs.shape == (3, 2)
    assert isinstance(out.sequence_logprob, float) and out.sequence_logprob == float(out.token_logprobs.to(torch.float64).sum())
    assert torch.equal(out.top_token_ids[:, 0], plain[0, ids.shape[1]:])
    reqs = [(ids, u8), (ids[:, :-4], u8)]
    head, sfx = ids[:, :-48], [ids[:, -48:], ids[:, -48:-20]]
    for got, want in ((model.generate_batch(reqs, max_new_tokens=3, eos_token_id=[], logprobs=1), model.generate_batch(reqs, max_new_tokens=3, eos_token_id=[])),
                      (model.generate_stream(reqs, batch_size=2, max_new_tokens=3, eos_token_id=[], logprobs=1),
                       model.generate_stream(reqs, batch_size=2, max_new_tokens=3, eos_token_id=[])),
                      (model.generate_shared(head, u8, sfx, max_new_tokens=3, eos_token_id=[], logprobs=1),
                       model.generate_shared(head, u8, sfx, max_new_tokens=3, eos_token_id=[]))):
        assert isinstance(got, list) and len(got) == 2 and all(isinstance(w, torch.Tensor) for w in want)
        for g, w in zip(got, want):
            assert isinstance(g, sampling.GenerationLogprobs) and torch.equal(g.sequences, w) and g.token_logprobs.shape == (3,)
            assert g.sequence_logprob == float(g.token_logprobs.to(torch.float64).sum()) and g.top_token_ids.shape == (3, 1)
    for bad in (9, -1):
        n, _ = count_launches(ops, lambda: _raises_value_error(lambda: model.generate(ids, pixel_values=u8, max_new_tokens=2, logprobs=bad)))
        assert n == 0
    with pytest.warns(UserWarning, match="output_scores"):
        sampling.warn_unsupported("generate", {"output_scores": True, "return_dict_in_generate": True})
    for key in ("output_scores", "output_logits", "output_attentions"):
        assert sampling.UNSUPPORTED[key] is False


def _raises_value_error(fn):
    with pytest.raises(ValueError, match="logprobs"):
        fn()


def test_run_inference_records(model, ops, tmp_path):
    from PIL import Image
    from leopard_amd import harness
    from leopard_amd.synth import synth_image_u8
    cfg = model.config

    class Tok:
        pad_token_id = 0

        def __call__(self, texts, **kw):
            ids = []
            for piece in texts[0].split(harness.TOK_IMG):
                ids += [1 + (ord(c) % 200) for c in piece[::9]] + [cfg.image_token_index]
            return {"input_ids": torch.tensor([ids[:-1]])}

        def batch_decode(self, ids, **kw):
            return [" ".join(str(int(i)) for i in ids[0])]

    p = str(tmp_path / "im.png")
    Image.fromarray(synth_image_u8(40, 300, 300)).save(p)
    recs = [{"images_path": [p], "question": "<image> which?", "answers": ["A"], "ques_type": "open-ended", "options": None}]
    gen_kw = harness.generate_kwargs
    harness.generate_kwargs = lambda pad: {**gen_kw(pad), "max_new_tokens": 3}
    try:
        plain = harness.run_inference(recs, model, Tok())
        rows = harness.run_inference(recs, model, Tok(), logprobs=2)
    finally:
        harness.generate_kwargs = gen_kw
    assert "answer_logprob" not in plain[0] and "token_logprobs" not in plain[0]
    extra = {k: rows[0].pop(k) for k in ("answer_logprob", "token_logprobs")}
    assert rows == plain                                                # the other fields are the default ones
    assert isinstance(extra["token_logprobs"], list) and 1 <= len(extra["token_logprobs"]) <= 3
    assert extra["answer_logprob"] == float(torch.tensor(extra["token_logprobs"], dtype=torch.float32).to(torch.float64).sum())
