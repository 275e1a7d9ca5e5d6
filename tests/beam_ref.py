"""Beam search: the cases the emulator (tests/test_emu_beam.py) and the device (tests/test_gpu_beam.py) share, and float64 restatements of
lmi_beam_step and lmi_beam_reorder.  The restatement of the select launch is ``leopard_amd.beams.walk_of``: it ranks ALL n_rows x V
candidates, so it does not rely on the argument that a row's best K suffice.  Nothing here needs a kernel to be imported."""
import itertools

import numpy as np
import torch

from leopard_amd import beams

NAN, INF = float("nan"), float("inf")
MAXB, MAX_EOS, WALK_WORDS = 8, 4, 1 + 40 * 5
GAP = 1e-3                                                             # neighbouring totals of a planted walk differ by at least this


# ---- lmi_beam_step ---------------------------------------------------------------------------------------------------------------------
def lse64(x64):
    m = x64.max(axis=1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (m + np.log(np.exp(x64 - m).sum(axis=1, keepdims=True)))[:, 0]


def ref_walk(case, dtype=np.float64, lse=None):
    """The walk list of a case from whole rows: float64 with its own lse (the reference), or float32 with the kernel's lse (its bits)."""
    x = case["logits"][:, :case["V"]].numpy().astype(dtype)
    l = lse64(x.astype(np.float64)).astype(dtype) if lse is None else np.asarray(lse, dtype=dtype)
    with np.errstate(invalid="ignore"):
        lp = x - l[:, None]
    return beams.walk_of(lp, np.asarray(case["scores"], dtype=dtype), case["K"], case["eos"], case["suppress"])


def min_gap(case):
    """The smallest difference of neighbouring totals over the float64 walk AND the first candidate past its end."""
    longer = dict(case, K=case["K"] + 1) if case["V"] - len(case["eos"]) - len(case["suppress"]) > case["K"] else case
    t = [c.total for c in ref_walk(longer) if np.isfinite(c.total)]
    return min((a - b for a, b in zip(t, t[1:])), default=INF)


def random_case(name, V, K, n_eos, n_sup=0, sup_eos=False, n_rows=None, ld=None, seed=0, pad=0.0):
    """Base logits N(0, 1); per row K + 2 planted non-eos ids well above them, every eos id planted in some rows, scores spread out —
    re-drawn (seed + 1000 n) until neighbouring totals of the walk differ by GAP (asserted: the restatement's order is then beyond the
    kernel's rounding, so ids and ranks must match exactly)."""
    n_rows = K if n_rows is None else n_rows
    ld = (V + 3) // 4 * 4 if ld is None else ld
    for attempt in range(200):
        g = np.random.default_rng(seed + 1000 * attempt)
        x = g.standard_normal((n_rows, ld)).astype(np.float32)
        x[:, V:] = pad                                                 # the row's padding: never read
        ids = g.permutation(V)
        eos = [int(i) for i in ids[:n_eos]]
        sup = [int(i) for i in ids[n_eos:n_eos + n_sup]] + (eos[:1] if sup_eos and eos else [])
        for b in range(n_rows):
            own = g.choice(ids[n_eos:], K + 2, replace=False)          # may hit a suppressed id: then it must not show up
            x[b, own] = (6.0 + 3.0 * g.random(K + 2)).astype(np.float32)
            for e in eos:
                if g.random() < 0.6:
                    x[b, e] = np.float32(6.0 + 3.0 * g.random())
        scores = [0.0] if n_rows == 1 else [float(v) for v in (-2.0 * g.random(n_rows)).astype(np.float32)]
        case = dict(name=name, V=V, K=K, eos=eos, suppress=sup, logits=torch.from_numpy(x), scores=scores, order_only=False)
        if min_gap(case) >= GAP:
            return case
    raise AssertionError(f"{name}: no draw with neighbouring totals {GAP} apart")


def step_cases():
    out = []
    for V in (1003, 1024):
        for K in (1, 2, 4, 8):
            out.append(random_case(f"V{V}-K{K}-eos2", V, K, 2, seed=V + K))
        out.append(random_case(f"V{V}-K4-eos0", V, 4, 0, seed=V + 11))
        out.append(random_case(f"V{V}-K4-eos4-suppress", V, 4, 4, n_sup=5, seed=V + 12))
        out.append(random_case(f"V{V}-K8-eos2-suppressed-eos", V, 8, 2, n_sup=3, sup_eos=True, seed=V + 13))
        out.append(random_case(f"V{V}-K4-first-step", V, 4, 2, n_rows=1, seed=V + 14))
        out.append(random_case(f"V{V}-K8-first-step", V, 8, 4, n_rows=1, seed=V + 15))
    # a row whose best 2 entries are eos
    c = random_case("best-two-are-eos", 1003, 4, 2, seed=21)
    c["logits"][1, c["eos"][0]], c["logits"][1, c["eos"][1]] = 11.0, 10.5
    assert min_gap(c) >= GAP
    out.append(c)
    # one beam owns all K survivors: its row's planted ids tower over the other rows' totals
    c = random_case("one-beam-owns-all", 1024, 4, 2, seed=22)
    c["scores"] = [-30.0, -30.0, 0.0, -30.0]
    assert min_gap(c) >= GAP and {w.parent for w in ref_walk(c) if not w.is_eos} == {2}
    out.append(c)
    # exact ties across beams and inside a row: equal rows, equal scores, pairs of equal logits — the restatement's ORDER only
    x = torch.zeros(4, 1024)
    x[:, [5, 9, 700, 701]] = 4.0
    x[:, [17, 18]] = 3.0
    x[:, 100] = 4.0                                                    # an eos id tied with the best
    out.append(dict(name="exact-ties", V=1024, K=4, eos=[100], suppress=[9], logits=x, scores=[-1.0, -1.0, -1.0, -1.0], order_only=True))
    # a -inf row and a NaN entry: neither row offers a candidate (lse -inf / NaN: every logit - lse is NaN); -inf entries elsewhere are
    # ordinary and come last.  The two live rows fill the K beams, and the draw keeps neighbouring totals GAP apart like every random case
    for seed in range(23, 223):
        c = random_case("inf-row-and-nan", 1003, 4, 2, seed=seed)
        c["logits"][0, :] = -INF
        c["logits"][2, 77] = NAN
        c["logits"][1, 3:900] = -INF
        if min_gap(c) >= GAP:
            break
    assert min_gap(c) >= GAP and {w.parent for w in ref_walk(c)} == {1, 3}
    out.append(c)
    return out


def big_case():
    """The production vocabulary, K = 8, rows at a padded stride whose padding holds huge values."""
    return random_case("V128256-K8", 128256, 8, 2, n_sup=2, ld=128256 + 64, seed=31, pad=1e30)


def run_beam_step(ops, dev, case, K=None):
    K = case["K"] if K is None else K
    x = case["logits"].clone().to(dev)
    n = x.shape[0]
    eos = torch.tensor(sorted(case["eos"]) + [-1] * (MAX_EOS - len(case["eos"])), dtype=torch.int64).to(dev)
    sup = torch.tensor(case["suppress"], dtype=torch.int64).to(dev) if case["suppress"] else None
    score = torch.full((MAXB,), 7.0)
    score[:n] = torch.tensor(case["scores"])
    o = dict(score=score.to(dev), tok=torch.full((MAXB,), -7, dtype=torch.int64).to(dev), parent=torch.full((MAXB,), -7, dtype=torch.int32).to(dev),
             walk=torch.full((WALK_WORDS,), -7, dtype=torch.int32).to(dev), row_lse=torch.full((n,), 7.0).to(dev),
             row_id=torch.full((n, MAXB), -7, dtype=torch.int32).to(dev), row_lp=torch.full((n, MAXB), 7.0).to(dev),
             row_eos_lp=torch.full((n, MAX_EOS), 7.0).to(dev), pos=torch.arange(10, 10 + MAXB, dtype=torch.int32).to(dev),
             k_len=torch.arange(20, 20 + MAXB, dtype=torch.int32).to(dev), rows_held=torch.tensor([5], dtype=torch.int32).to(dev))
    ops.beam_step(x, case["V"], K, eos, o["score"], o["tok"], o["parent"], o["walk"], o["row_lse"], o["row_id"], o["row_lp"], o["row_eos_lp"],
                  suppress=sup, pos=o["pos"], k_len=o["k_len"], rows_held=o["rows_held"])
    return dict({k: v.cpu() for k, v in o.items()}, logits=x.cpu())


def same_bits(a, b):
    a, b = torch.as_tensor(a, dtype=torch.float32), torch.as_tensor(b, dtype=torch.float32)
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(a[~na], b[~nb])


def check_beam_step(ops, dev, case):
    K, V, x = case["K"], case["V"], case["logits"]
    n = x.shape[0]
    o = run_beam_step(ops, dev, case)
    # the rows: lse = lmi_token_logprobs' bits; (id, logit - lse) of the best K non-eos, non-suppressed entries in TopList's order
    tgt = torch.zeros(n, dtype=torch.int64).to(dev)
    lp0, lse, am = torch.empty(n).to(dev), torch.empty(n).to(dev), torch.empty(n, dtype=torch.int64).to(dev)
    ops.token_logprobs(x.to(dev), V, tgt, lp0, lse, am)
    lse = lse.cpu()
    assert same_bits(o["row_lse"], lse), (case["name"], o["row_lse"], lse)
    barred = set(case["eos"]) | set(case["suppress"])
    for b in range(n):
        row = x[b, :V]
        nan = torch.isnan(row)
        order = torch.sort(torch.where(nan, torch.tensor(-INF), row), descending=True, stable=True).indices
        order = [int(i) for i in order if not nan[i] and int(i) not in barred][:K]
        assert o["row_id"][b, :len(order)].tolist() == order, (case["name"], b, o["row_id"][b], order)
        assert same_bits(o["row_lp"][b, :len(order)], row[order] - lse[b]), (case["name"], b)
        assert (o["row_id"][b, len(order):K] == -1).all() and (o["row_id"][b, K:] == -7).all() and (o["row_lp"][b, K:] == 7.0).all()
    if not barred:                                                     # the same row through lmi_decode_logprobs: bit for bit
        lp, ti, tl = torch.zeros(1, n).to(dev), torch.zeros(1, n, MAXB, dtype=torch.int32).to(dev), torch.zeros(1, n, MAXB).to(dev)
        ops.decode_logprobs(x.to(dev), V, tgt, MAXB, lp, ti, tl)
        assert torch.equal(ti[0, :, :K].cpu(), o["row_id"][:, :K]) and same_bits(tl[0, :, :K].cpu(), o["row_lp"][:, :K]), case["name"]
    eos_sorted = sorted(case["eos"])
    for b in range(n):
        for j in range(MAX_EOS):
            got = o["row_eos_lp"][b, j]
            if j >= len(eos_sorted):
                assert torch.isnan(got)
            elif eos_sorted[j] in case["suppress"]:
                assert float(got) == -INF
            else:
                assert same_bits(got, x[b, eos_sorted[j]] - lse[b])
    # the walk: exactly the fp32 restatement on the kernel's lse (order, ranks AND the totals' bits) ...
    got = beams.decode_walk(o["walk"].numpy())
    want32 = ref_walk(case, np.float32, lse.numpy())
    assert [(c.rank, c.parent, c.id, c.is_eos) for c in got] == [(c.rank, c.parent, c.id, c.is_eos) for c in want32], (case["name"], got, want32)
    assert same_bits([c.total for c in got], [c.total for c in want32]), case["name"]
    assert [c.rank for c in got] == list(range(len(got)))
    # ... and, where the draw keeps neighbouring totals GAP apart, the float64 reference to the scan's bound
    if not case["order_only"]:
        want = ref_walk(case)
        assert [(c.rank, c.parent, c.id, c.is_eos) for c in got] == [(c.rank, c.parent, c.id, c.is_eos) for c in want], (case["name"], got, want)
        tol = 1e-5 * max(1.0, float(lse[torch.isfinite(lse)].abs().max()))
        assert max(abs(a.total - b.total) for a, b in zip(got, want)) <= tol, case["name"]
    # the next beams = the walk's non-eos entries in order; fillers where the candidates run out; the rest untouched
    nxt = [c for c in got if not c.is_eos]
    assert len(nxt) <= K and (len(nxt) == K or case["order_only"])
    f = len(nxt)
    assert o["tok"][:f].tolist() == [c.id for c in nxt] and o["parent"][:f].tolist() == [c.parent for c in nxt]
    assert same_bits(o["score"][:f], [c.total for c in nxt])
    assert (o["tok"][f:K] == 0).all() and (o["parent"][f:K] == 0).all() and (o["score"][f:K] == -INF).all()
    assert (o["tok"][K:] == -7).all() and (o["parent"][K:] == -7).all() and (o["score"][max(K, n):] == 7.0).all()
    assert o["pos"].tolist() == [10 + j + (j < K) for j in range(MAXB)] and o["k_len"].tolist() == [20 + j + (j < K) for j in range(MAXB)]
    assert int(o["rows_held"][0]) == 6
    assert same_bits(o["logits"], x)                                   # the caller's logits are not modified
    return got


# ---- lmi_beam_reorder ------------------------------------------------------------------------------------------------------------------
def permutations_of(K):
    """identity, one swap, a K-cycle, all from slot 0, a mix of kept and replaced slots"""
    ident = list(range(K))
    swap = ident[:]
    swap[0], swap[K - 1] = swap[K - 1], swap[0]
    mix = [b if b % 2 == 0 else (b + 2) % K for b in range(K)]
    return {"identity": ident, "swap": swap, "cycle": [(b + 1) % K for b in range(K)], "all-from-0": [0] * K, "mix": mix}


REORDER_ROWS = list(itertools.product((0, 1, 5, 257), (0, 3)))        # (rows held, row0)
SLOT_ROWS = 600                                                        # a slot's capacity: beyond the 256 / 512 rows that size the grid


def check_beam_reorder(ops, dev, dtype, width, K, held, row0, parent, gen):
    """L = 2 (four tensors) of K slots x SLOT_ROWS rows x ``width`` elements: rows [row0, held) of slot b become those of slot parent[b],
    bit for bit ``index_select`` of a copy; every other byte of every slot stays."""
    n_t = 4
    bits = [torch.from_numpy(gen.integers(-32768, 32768, (K * SLOT_ROWS, width), dtype=np.int16)) for _ in range(n_t)]
    want = []
    for t in bits:
        w = t.clone().view(K, SLOT_ROWS, width)
        if held > row0:
            w[:, row0:held] = t.view(K, SLOT_ROWS, width)[:, row0:held].index_select(0, torch.tensor(parent))
        want.append(w.view(K * SLOT_ROWS, width))
    tens = [t.view(dtype).to(dev) for t in bits]
    ptrs = torch.tensor([t.data_ptr() for t in tens], dtype=torch.int64).to(dev)
    par = torch.tensor(parent + [-7] * (MAXB - K), dtype=torch.int32).to(dev)
    max_rows = (max(held - row0, 1) + 255) // 256 * 256
    ops.beam_reorder(ptrs, par, K, torch.tensor([row0], dtype=torch.int32).to(dev), torch.tensor([held], dtype=torch.int32).to(dev),
                     width * 2, SLOT_ROWS, max_rows)
    for i, (t, w) in enumerate(zip(tens, want)):
        assert torch.equal(t.cpu().view(torch.int16), w), (str(dtype), width, K, held, row0, parent, i)


# ---- the engine against a host loop ------------------------------------------------------------------------------------------------------
NOISE = 2e-3                            # the logit difference of the batch-1 and the batched decode path, relative to max |logit|: the
#                                         16-bit noise tests/test_gpu_shared_decode.py allows a greedy token to flip on, and the same rule here


class HostLoop:
    """generate_beams restated with ONE batch-1 cache per beam: ``decode_step``'s raw logits, float64 log-softmax, ``beams.walk_of`` over
    whole rows and ``beams.BeamSearch``.  ``cut`` is the first step >= 2 whose decisive gap — from the last kept candidate to the first
    dropped one — is within NOISE x max |logit| of that step's rows, the rule of tests/test_gpu_shared_decode.assert_equal_or_near_tie
    (step 1 reads the prefill row on both sides); ``eps[t]`` is that bound for step t + 1 (0 for step 1)."""

    def __init__(self, eng, cfg, ids, tiles, dtype, dev):
        self.eng, self.cfg, self.ids, self.tiles, self.dtype, self.dev = eng, cfg, ids, tiles, dtype, dev

    def run(self, K, T, eos=(), length_penalty=1.0, early_stopping=False, n_return=1):
        from leopard_amd.engine import KVCache
        eng, V = self.eng, self.cfg.text_config.vocab_size
        sup = [] if eng.suppress_tokens is None else [int(t) for t in eng.suppress_tokens.tolist()]
        P = eng.merged_len(self.ids)
        caches = [KVCache(self.cfg, P + T, self.dtype, self.dev) for _ in range(K)]
        rows = eng.prefill(self.ids, self.tiles, cache=caches[0]).logits_last.reshape(1, -1)[:, :V].double().cpu().numpy()
        for c in caches[1:]:
            for i in range(len(c.k)):
                c.k[i][:P].copy_(caches[0].k[i][:P]); c.v[i][:P].copy_(caches[0].v[i][:P])
            c.length = P
        search = beams.BeamSearch(K, T, length_penalty, early_stopping, n_return)
        scores, self.cut, self.eps = [0.0], None, [0.0]
        was, eng.use_graphs = eng.use_graphs, False                   # K caches: eager steps instead of K captures
        try:
            while True:
                lp = rows - lse64(rows)[:, None]
                walk = beams.walk_of(lp, scores, K, eos, sup)
                # the decisive gap: from the last kept candidate (the one that fills beam K - 1) to the first dropped one
                kept = [c.total for c in beams.walk_of(lp, scores, K + 1, eos, sup) if not c.is_eos]
                gap = kept[K - 1] - kept[K] if len(kept) > K else INF
                if search.generated >= 1 and self.cut is None and gap <= NOISE * float(np.abs(rows).max()):
                    self.cut = search.generated + 1
                if not search.step(walk):
                    break
                L = caches[0].length
                for i in range(len(caches[0].k)):
                    for which in ("k", "v"):
                        old = torch.stack([getattr(c, which)[i][P:L] for c in caches])
                        for b, c in enumerate(caches):
                            getattr(c, which)[i][P:L].copy_(old[search.parents[b]])
                scores = search.scores
                rows = np.stack([eng.decode_step(seq[-1], c)[:V].double().cpu().numpy() for seq, c in zip(search.beams, caches)])
                self.eps.append(NOISE * float(np.abs(rows).max()))
        finally:
            eng.use_graphs = was
        return search.results()


def engine_cases():
    """(K, decode, early_stopping, length_penalty): every early_stopping value meets every length_penalty once, and every K meets each of
    the two (a Latin square); both decode modes at every K."""
    return [(1, "shared", False, 0.0), (2, "copy", False, 1.0), (4, "shared", False, 2.0),
            (2, "shared", True, 0.0), (4, "copy", True, 1.0), (1, "copy", True, 2.0),
            (4, "copy", "never", 0.0), (1, "shared", "never", 1.0), (2, "copy", "never", 2.0)]


def engine_prompt(cfg, ids, seed):
    """The micro / mid prompt with its question ids re-drawn from ``seed`` (the seed is chosen so that the HOST LOOP's near-tie steps stay
    inside the cap of one case in eight; the images and the prompt's frame stay)."""
    g = np.random.default_rng(seed)
    out = ids.clone()
    q = torch.from_numpy(g.integers(3, min(cfg.text_config.vocab_size, 128000), 24))
    q[q == cfg.image_token_index] = 3
    out[0, -32:-8] = q.to(out.device)
    return out


def score_tol(host: HostLoop, T_i: int, length_penalty: float) -> float:
    """A hypothesis of T_i tokens: the log-probability of step t is logit - lse, and the lse moves by a softmax-weighted mean of its row's
    logit errors, so the step moves by at most 2 eps[t] between the two decode paths (eps = NOISE x max |logit| of that step's rows; 0 for
    step 1, whose row is the prefill's on both sides).  The score is the fp32 total (T_i adds of values below 2^5: 1e-5) over
    T_i ** length_penalty."""
    return (2 * sum(host.eps[:T_i]) + 1e-5) / (T_i ** length_penalty)


def compare_with_host(eng, host: HostLoop, K, decode, es, lp, T, eos):
    """generate_beams against the host loop with num_return_sequences = K.  Returns (whether the case agreed at its full length, the host
    loop's near-tie step or None, the host loop's hypotheses).  Where the outputs differ the host loop must have a near-tie step, and both
    are run again up to the step before it and must agree."""
    want = host.run(K, T, eos, lp, es, K)
    cut = host.cut

    def agree(got, want):
        return len(got.sequences) == len(want) and all(g[0, host.ids.numel():].tolist() == w[1] for g, w in zip(got.sequences, want))
    got = eng.generate_beams(host.ids, host.tiles, K, max_new_tokens=T, eos_token_id=eos, length_penalty=lp, early_stopping=es,
                             num_return_sequences=K, decode=decode)
    full = agree(got, want)
    if not full:
        assert cut is not None and cut > 1, (K, decode, es, lp, cut, [s.tolist() for s in got.sequences], want)
        T = cut - 1
        want = host.run(K, T, eos, lp, es, K)
        got = eng.generate_beams(host.ids, host.tiles, K, max_new_tokens=T, eos_token_id=eos, length_penalty=lp, early_stopping=es,
                                 num_return_sequences=K, decode=decode)
        assert agree(got, want), (K, decode, es, lp, cut, [s.tolist() for s in got.sequences], want)
    for g, s, (ws, wseq) in zip(got.sequences, got.scores, want):
        assert g.shape == (1, host.ids.numel() + len(wseq)) and g[0, :host.ids.numel()].tolist() == host.ids.reshape(-1).tolist()
        assert abs(s - ws) <= score_tol(host, len(wseq), lp), (K, decode, es, lp, s, ws)
    assert got.scores == sorted(got.scores, reverse=True)
    return full, cut, want


def pick_eos(host: HostLoop, K=4, T=8):
    """Two eos ids from what the unconstrained beams produce: the third token of the best hypothesis and a later token of the second."""
    res = host.run(K, T, (), 1.0, False, K)
    a = res[0][1][2]
    b = next((t for _, seq in res[1:] for t in seq[3:] if t != a), next(t for _, seq in res for t in seq if t != a))
    return (a, b)
