"""Beam search with logits processors: the cases the emulator (tests/test_emu_beam_rules.py) and the device (tests/test_gpu_beam_rules.py)
share, and restatements of lmi_beam_step_rules.  In beam search transformers applies the processors to the log-softmax scores:
s = logit - lse, then ``tests.logits_rules_ref.apply`` (penalty, n-gram ban, eos ban while min_left > 0) over ``prompt + that beam's
tokens``, then ``leopard_amd.beams.walk_of`` over the WHOLE processed rows.  ``rules64`` is apply's arithmetic in float64 (the reference);
the fp32 restatement on the kernel's own lse is ``apply`` itself and must match bit for bit.  Nothing here needs a kernel to be imported."""
import numpy as np
import torch

from leopard_amd import beams
from tests import beam_ref as R
from tests import logits_rules_ref as L

NAN, INF = float("nan"), float("inf")
MAXB, MAX_EOS, WALK_WORDS, GAP = R.MAXB, R.MAX_EOS, R.WALK_WORDS, R.GAP
RULESETS = ((1.3, 0, 0), (1.0, 2, 0), (1.0, 0, 5), (1.3, 2, 5), (0.8, 1, 3))       # (penalty, n-gram, min_left): the issue's five


def rules64(s, seq_ids, penalty, n, min_left, eos):
    """``logits_rules_ref.apply`` on a float64 row (a new array): the same three rules in the same order, in float64."""
    out = np.array(s, dtype=np.float64)
    V = out.shape[0]
    seq = [int(t) for t in seq_ids]
    if float(penalty) != 1.0:
        ids = sorted({t for t in seq if 0 <= t < V})
        if ids:
            l = out[ids]
            with np.errstate(invalid="ignore"):
                out[ids] = np.where(l < 0, l * float(penalty), l / float(penalty))
    n, Ln = int(n), len(seq)
    if n > 0 and Ln + 1 >= n:
        tail = seq[Ln - (n - 1):] if n > 1 else []
        for i in range(Ln - n + 1):
            if seq[i:i + n - 1] == tail and 0 <= seq[i + n - 1] < V:
                out[seq[i + n - 1]] = -INF
    if int(min_left) > 0:
        for e in eos:
            if 0 <= int(e) < V:
                out[int(e)] = -INF
    return out


def seen_ids(case, b):
    """The ids row b is judged against: its list before the call, with the appended token."""
    return list(case["seqs"][b]) + ([int(case["tok"][b])] if case["tok"] is not None else [])


def processed(case, dtype=np.float64, lse=None):
    """The processed rows s' [n_rows, V]: float64 with its own lse, or float32 (``apply``'s bits) on the kernel's lse."""
    x = case["logits"][:, :case["V"]].numpy().astype(dtype)
    l = R.lse64(x.astype(np.float64)).astype(dtype) if lse is None else np.asarray(lse, dtype=dtype)
    with np.errstate(invalid="ignore"):
        s = x - l[:, None]
    p, n, ml = case["rules"]
    out = np.empty_like(s)
    for b in range(s.shape[0]):
        if dtype == np.float32:
            out[b] = L.apply(torch.from_numpy(s[b]), seen_ids(case, b), p, n, ml, case["eos"]).numpy()
        else:
            out[b] = rules64(s[b], seen_ids(case, b), p, n, ml, case["eos"])
    return out


def ref_walk(case, dtype=np.float64, lse=None, K=None):
    return beams.walk_of(processed(case, dtype, lse), np.asarray(case["scores"], dtype=dtype), case["K"] if K is None else K, case["eos"],
                         case["suppress"])


def min_gap(case):
    """The smallest difference of neighbouring finite totals over the float64 PROCESSED walk and the first candidate past its end."""
    more = case["V"] - len(case["eos"]) - len(case["suppress"]) > case["K"]
    t = [c.total for c in ref_walk(case, K=case["K"] + (1 if more else 0)) if np.isfinite(c.total)]
    return min((a - b for a, b in zip(t, t[1:])), default=INF)


def raw_order(case, b):
    """Row b's ids that are neither eos nor suppressed, raw logit descending, id ascending (NaN left out)."""
    row = case["logits"][b, :case["V"]]
    nan = torch.isnan(row)
    order = torch.sort(torch.where(nan, torch.tensor(-INF), row), descending=True, stable=True).indices
    barred = set(case["eos"]) | set(case["suppress"])
    return [int(i) for i in order if not nan[i] and int(i) not in barred]


def random_case(name, V, K, n_eos, length, rules, n_sup=0, n_rows=None, ld=None, seed=0, pad=0.0, append=True, plant=None):
    """beam_ref.random_case's rows (K + 2 planted non-eos ids per row, eos ids planted in some rows, spread scores) and per row an id list of
    ``length`` ids AFTER the append: heavy duplicates drawn from a pool that holds the row's raw best id, its K-th and (K + 1)-th, an eos
    id, a suppressed id and two ids >= V.  ``plant(case, b)`` -> (ids forced to the front of the list, the appended token) builds the named
    situations.  Re-drawn until neighbouring totals of the PROCESSED walk are GAP apart."""
    n_rows = K if n_rows is None else n_rows
    ld = (V + 3) // 4 * 4 if ld is None else ld
    for attempt in range(200):
        g = np.random.default_rng(seed + 1000 * attempt)
        x = g.standard_normal((n_rows, ld)).astype(np.float32)
        x[:, V:] = pad
        ids = g.permutation(V)
        eos = [int(i) for i in ids[:n_eos]]
        sup = [int(i) for i in ids[n_eos:n_eos + n_sup]]
        for b in range(n_rows):
            own = g.choice(ids[n_eos:], K + 2, replace=False)
            x[b, own] = (6.0 + 3.0 * g.random(K + 2)).astype(np.float32)
            for e in eos:
                if g.random() < 0.6:
                    x[b, e] = np.float32(6.0 + 3.0 * g.random())
        scores = [0.0] if n_rows == 1 else [float(v) for v in (-2.0 * g.random(n_rows)).astype(np.float32)]
        case = dict(name=name, V=V, K=K, eos=eos, suppress=sup, logits=torch.from_numpy(x), scores=scores, order_only=False, rules=rules,
                    seqs=[], tok=[] if append else None)
        before = length - 1 if append else length
        for b in range(n_rows):
            raw = raw_order(case, b)
            pool = [raw[0], raw[K - 1], raw[K], L.IMAGE_ID, V + 31] + eos[:1] + sup[:1]
            seq = L.heavy_seq(before, V, seed=seed + 7 * b + attempt, extra=pool) if before > 0 else []
            front, tok = plant(case, b) if plant else ([], pool[int(g.integers(len(pool)))])
            seq[:len(front)] = front[:len(seq)]
            case["seqs"].append(seq)
            if append:
                case["tok"].append(int(tok))
        case["cap"] = (length + 2 + 3) // 4 * 4                       # a multiple of four ids: the id reorder moves 16-byte chunks
        if min_gap(case) >= GAP:
            return case
    raise AssertionError(f"{name}: no draw with neighbouring totals {GAP} apart")


# ---- the named situations: plant(case, b) -> (front of the id list, appended token) -----------------------------------------------------
def plant_kth(case, b):            # the raw K-th best id is seen: a penalty > 1 moves it down and out of the list
    raw = raw_order(case, b)
    return [raw[case["K"] - 1]], raw[-1]


def plant_next(case, b):           # the raw (K + 1)-th best id is seen: p = 0.5 lifts it into the list
    raw = raw_order(case, b)
    return [raw[case["K"]]], raw[-1]


def plant_bigram_best(case, b):    # .. a, best .. then a appended: n = 2 bans the raw best id
    raw = raw_order(case, b)
    return [raw[-1], raw[0]], raw[-1]


def plant_all_best(case, b):       # every raw best-K id is seen: n = 1 bans them all
    raw = raw_order(case, b)
    return raw[:case["K"]], raw[0]


def plant_eos_and_suppressed(case, b):   # an eos id and a suppressed id are seen
    raw = raw_order(case, b)
    return [case["eos"][0], case["suppress"][0], raw[0]], case["eos"][0]


def step_cases():
    out = []
    lengths = iter(L.LENGTHS * 4)
    k = 0
    for V in (1003, 1024):
        for K in (1, 2, 4, 8):
            out.append(random_case(f"V{V}-K{K}-rules{k % 5}", V, K, 2, next(lengths), RULESETS[k % 5], n_sup=2, seed=V + K))
            k += 1
        out.append(random_case(f"V{V}-K4-first-step", V, 4, 2, next(lengths), RULESETS[3], n_rows=1, seed=V + 14, append=False))
        out.append(random_case(f"V{V}-K8-first-step", V, 8, 4, next(lengths), RULESETS[4], n_rows=1, seed=V + 15, append=False))
    out.append(random_case("penalty-moves-out", 1003, 4, 2, 40, (2.0, 0, 0), seed=41, plant=plant_kth))
    out.append(random_case("half-penalty-lifts-in", 1024, 4, 2, 40, (0.5, 0, 0), seed=42, plant=plant_next))
    out.append(random_case("bigram-bans-best", 1003, 4, 2, 1025, (1.0, 2, 0), seed=43, plant=plant_bigram_best))
    out.append(random_case("all-best-banned", 1024, 4, 2, 40, (1.0, 1, 0), seed=44, plant=plant_all_best))
    out.append(random_case("seen-eos-and-suppressed", 1003, 4, 2, 40, (1.3, 0, 0), n_sup=2, seed=45, plant=plant_eos_and_suppressed))
    out.append(random_case("seen-eos-min-left", 1003, 2, 2, 40, (1.3, 3, 2), n_sup=2, seed=46, plant=plant_eos_and_suppressed))
    # exact ties across beams and inside a row, some of them seen (penalised alike) and one banned: the restatement's ORDER only
    x = torch.zeros(4, 1024)
    x[:, [5, 9, 700, 701]] = 4.0
    x[:, [17, 18]] = 3.0
    x[:, 100] = 4.0
    out.append(dict(name="exact-ties", V=1024, K=4, eos=[100], suppress=[9], logits=x, scores=[-1.0] * 4, order_only=True, rules=(1.5, 2, 0),
                    seqs=[[5, 700, 33, 701, 33]] * 4, tok=[33] * 4, cap=8))
    # a -inf row and a NaN entry offer nothing; -inf entries elsewhere are ordinary and come last
    for seed in range(47, 247):
        c = random_case("inf-row-and-nan", 1003, 4, 2, 40, RULESETS[3], seed=seed)
        c["logits"][0, :] = -INF
        c["logits"][2, 77] = NAN
        c["logits"][1, 3:900] = -INF
        if min_gap(c) >= GAP and {w.parent for w in ref_walk(c)} == {1, 3}:
            break
    assert min_gap(c) >= GAP and {w.parent for w in ref_walk(c)} == {1, 3}
    out.append(c)
    return out


def big_case():
    """The production vocabulary, K = 8, 7200 ids per row, rows at a padded stride whose padding holds huge values."""
    return random_case("V128256-K8", 128256, 8, 2, 7200, (1.3, 3, 1), n_sup=2, ld=128256 + 64, seed=31, pad=1e30)


# ---- one call --------------------------------------------------------------------------------------------------------------------------------
def seq_buffer(case):
    n = case["logits"].shape[0]
    seq = torch.full((n, case["cap"]), -77, dtype=torch.int32)
    for b, s in enumerate(case["seqs"]):
        seq[b, :len(s)] = torch.tensor(s, dtype=torch.int32)
    return seq


def buffers(case, dev, scores=None):
    n, (p, ng, ml) = case["logits"].shape[0], case["rules"]
    score = torch.full((MAXB,), 7.0)
    score[:n] = torch.tensor(case["scores"] if scores is None else scores)
    tok = torch.full((MAXB,), -7, dtype=torch.int64)
    if case["tok"] is not None:
        tok[:n] = torch.tensor(case["tok"], dtype=torch.int64)
    o = dict(score=score, tok=tok, parent=torch.full((MAXB,), -7, dtype=torch.int32), walk=torch.full((WALK_WORDS,), -7, dtype=torch.int32),
             row_lse=torch.full((n,), 7.0), row_id=torch.full((n, MAXB), -7, dtype=torch.int32), row_lp=torch.full((n, MAXB), 7.0),
             row_eos_lp=torch.full((n, MAX_EOS), 7.0), pos=torch.arange(10, 10 + MAXB, dtype=torch.int32),
             k_len=torch.arange(20, 20 + MAXB, dtype=torch.int32), rows_held=torch.tensor([5], dtype=torch.int32),
             seq=seq_buffer(case), seq_len=torch.tensor([len(s) for s in case["seqs"]], dtype=torch.int32),
             penalty=torch.full((n,), float(p)), ngram=torch.full((n,), int(ng), dtype=torch.int32),
             min_left=torch.full((n,), int(ml), dtype=torch.int32))
    return {k: v.to(dev) for k, v in o.items()}


def id_chunks(case):
    """(first chunk, chunks held) of the id reorder: every 16-byte chunk of four ids up to the longest list after the append."""
    return 0, (max(len(seen_ids(case, b)) for b in range(len(case["seqs"]))) + 3) // 4


def launch(ops, case, x, eos, sup, o, row0, held, ptrs=None):
    """The entry (the token to append is read from the ``tok`` buffer the select launch then overwrites) and, for K rows, the id reorder."""
    K = case["K"]
    ops.beam_step_rules(x, case["V"], K, eos, o["score"], o["tok"], o["parent"], o["walk"], o["row_lse"], o["row_id"], o["row_lp"], o["row_eos_lp"],
                        o["seq"], o["seq_len"], o["penalty"], o["ngram"], o["min_left"], append=None if case["tok"] is None else o["tok"],
                        suppress=sup, pos=o["pos"], k_len=o["k_len"], rows_held=o["rows_held"])
    if x.shape[0] == K:
        ptrs = torch.tensor([o["seq"].data_ptr()], dtype=torch.int64).to(x.device) if ptrs is None else ptrs
        ops.beam_reorder(ptrs, o["parent"], K, row0, held, 16, case["cap"] // 4, (case["cap"] // 4 + 255) // 256 * 256)


def device_args(case, dev):
    x = case["logits"].clone().to(dev)
    eos = torch.tensor(sorted(case["eos"]) + [-1] * (MAX_EOS - len(case["eos"])), dtype=torch.int64).to(dev)
    sup = torch.tensor(case["suppress"], dtype=torch.int64).to(dev) if case["suppress"] else None
    c0, held = id_chunks(case)
    return x, eos, sup, torch.tensor([c0], dtype=torch.int32).to(dev), torch.tensor([held], dtype=torch.int32).to(dev)


def run_step(ops, dev, case):
    x, eos, sup, row0, held = device_args(case, dev)
    o = buffers(case, dev)
    launch(ops, case, x, eos, sup, o, row0, held)
    return dict({k: v.cpu() for k, v in o.items()}, logits=x.cpu())


def expected_ids(case, parent):
    """The id buffer and the lengths after the call: the append, then — for K rows — whole chunks [first, held) of slot b from slot parent[b]."""
    seq, n = seq_buffer(case), len(case["seqs"])
    sl = torch.tensor([len(s) for s in case["seqs"]], dtype=torch.int32)
    if case["tok"] is not None:
        for b in range(n):
            seq[b, len(case["seqs"][b])] = int(case["tok"][b])
        sl += 1
    if n == case["K"] and n > 1:
        c0, held = id_chunks(case)
        seq[:, 4 * c0:4 * held] = seq[:, 4 * c0:4 * held].index_select(0, torch.tensor(parent, dtype=torch.int64))
    return seq, sl


def check_step(ops, dev, case):
    K, V, x = case["K"], case["V"], case["logits"]
    n, (p, ng, ml) = x.shape[0], case["rules"]
    o = run_step(ops, dev, case)
    # the rows: lse = lmi_token_logprobs' bits
    tgt = torch.zeros(n, dtype=torch.int64).to(dev)
    lp0, lse, am = torch.empty(n).to(dev), torch.empty(n).to(dev), torch.empty(n, dtype=torch.int64).to(dev)
    ops.token_logprobs(x.to(dev), V, tgt, lp0, lse, am)
    lse = lse.cpu()
    assert R.same_bits(o["row_lse"], lse), (case["name"], o["row_lse"], lse)
    # candidates: bit for bit apply() on fp32(logit - the kernel's lse), best K that are neither eos nor suppressed, s' descending, id ascending
    s32 = torch.from_numpy(processed(case, np.float32, lse.numpy()))
    barred = set(case["eos"]) | set(case["suppress"])
    eos_sorted = sorted(case["eos"])
    for b in range(n):
        row = s32[b]
        nan = torch.isnan(row)
        order = torch.sort(torch.where(nan, torch.tensor(-INF), row), descending=True, stable=True).indices
        order = [int(i) for i in order if not nan[i] and int(i) not in barred][:K]
        assert o["row_id"][b, :len(order)].tolist() == order, (case["name"], b, o["row_id"][b], order)
        assert R.same_bits(o["row_lp"][b, :len(order)], row[order]), (case["name"], b, o["row_lp"][b], row[order])
        assert (o["row_id"][b, len(order):K] == -1).all() and (o["row_id"][b, K:] == -7).all() and (o["row_lp"][b, K:] == 7.0).all()
        for j in range(MAX_EOS):
            got = o["row_eos_lp"][b, j]
            if j >= len(eos_sorted):
                assert torch.isnan(got)
            elif eos_sorted[j] in case["suppress"]:
                assert float(got) == -INF
            else:
                assert R.same_bits(got, row[eos_sorted[j]]), (case["name"], b, j, got, row[eos_sorted[j]])
    # the walk: exactly the fp32 restatement on the kernel's lse (order, ranks AND the totals' bits) ...
    key = lambda w: [(c.rank, c.parent, c.id, c.is_eos) for c in w]
    got = beams.decode_walk(o["walk"].numpy())
    want32 = ref_walk(case, np.float32, lse.numpy())
    assert key(got) == key(want32), (case["name"], got, want32)
    assert R.same_bits([c.total for c in got], [c.total for c in want32]), case["name"]
    assert [c.rank for c in got] == list(range(len(got)))
    # ... and the float64 reference: ids exact, totals to the scan's bound scaled by the one extra multiply or divide
    if not case["order_only"]:
        want = ref_walk(case)
        assert key(got) == key(want), (case["name"], got, want)
        tol = 1e-5 * max(1.0, float(lse[torch.isfinite(lse)].abs().max())) * max(p, 1.0 / p)
        for a, w in zip(got, want):
            assert a.total == w.total or abs(a.total - w.total) <= tol, (case["name"], a, w, tol)
    # the next beams = the walk's non-eos entries in order; fillers where the candidates run out; the rest untouched
    nxt = [c for c in got if not c.is_eos]
    assert len(nxt) <= K and (len(nxt) == K or case["order_only"])
    f = len(nxt)
    assert o["tok"][:f].tolist() == [c.id for c in nxt] and o["parent"][:f].tolist() == [c.parent for c in nxt]
    assert R.same_bits(o["score"][:f], [c.total for c in nxt])
    assert (o["tok"][f:K] == 0).all() and (o["parent"][f:K] == 0).all() and (o["score"][f:K] == -INF).all()
    assert (o["parent"][K:] == -7).all() and (o["score"][max(K, n):] == 7.0).all() and (o["tok"][max(K, n):] == -7).all()
    assert o["pos"].tolist() == [10 + j + (j < K) for j in range(MAXB)] and o["k_len"].tolist() == [20 + j + (j < K) for j in range(MAXB)]
    assert int(o["rows_held"][0]) == 6
    # the id lists: slot b holds what slot parent[b] held, the token it consumed appended; every other cell of the buffer is unchanged
    want_seq, want_len = expected_ids(case, o["parent"][:K].tolist())
    assert torch.equal(o["seq"], want_seq), (case["name"], (o["seq"] != want_seq).nonzero()[:8].tolist())
    assert torch.equal(o["seq_len"], want_len)
    if n == K:
        for b in range(K):
            src = o["parent"][b]
            assert o["seq"][b, :int(want_len[b])].tolist() == seen_ids(case, int(src))
    assert o["min_left"].tolist() == [max(ml - 1, 0)] * n
    assert R.same_bits(o["penalty"], torch.full((n,), float(p))) and o["ngram"].tolist() == [ng] * n
    assert R.same_bits(o["logits"], x)                                 # the caller's logits are not modified
    again = run_step(ops, dev, case)                                   # a second launch from the same inputs: identical bits
    for k in o:
        same = R.same_bits(o[k], again[k]) if o[k].dtype == torch.float32 else torch.equal(o[k], again[k])
        assert same, (case["name"], k)
    return got


def check_id_reorder(ops, dev, K, parent, first, held, cap=64):
    """lmi_beam_reorder over an id buffer: chunks [first, held) of four ids of slot b become those of slot parent[b], in place, for any
    parent (duplicates included); every other id stays."""
    g = torch.Generator().manual_seed(K * 100 + first + held)
    seq = torch.randint(0, 1 << 20, (K, cap), generator=g, dtype=torch.int32)
    want = seq.clone()
    if held > first:
        want[:, 4 * first:4 * held] = seq[:, 4 * first:4 * held].index_select(0, torch.tensor(parent))
    d = seq.to(dev)
    ops.beam_reorder(torch.tensor([d.data_ptr()], dtype=torch.int64).to(dev), torch.tensor(parent + [-7] * (MAXB - K), dtype=torch.int32).to(dev), K,
                     torch.tensor([first], dtype=torch.int32).to(dev), torch.tensor([held], dtype=torch.int32).to(dev), 16, cap // 4, 256)
    assert torch.equal(d.cpu(), want), (K, parent, first, held)


def check_rejects(ops, dev):
    """The argument checks raise before any launch: nothing is written."""
    import pytest
    z = lambda *s, dt=torch.int32: torch.zeros(*s, dtype=dt, device=dev)
    eos = torch.full((4,), -1, dtype=torch.int64, device=dev)
    mk = lambda: dict(score=z(8, dt=torch.float32), tok=z(8, dt=torch.int64), parent=z(8), walk=z(WALK_WORDS), row_lse=z(2, dt=torch.float32),
                      row_id=z(2, 8), row_lp=z(2, 8, dt=torch.float32), row_eos_lp=z(2, 4, dt=torch.float32), seq=z(2, 8), seq_len=z(2),
                      penalty=torch.ones(2, device=dev), ngram=z(2), min_left=z(2))
    rows = torch.zeros(2, 64, device=dev)
    ops.beam_step_rules(rows, 64, 2, eos, **mk())
    bad = mk()
    for kw, exc, match in ((dict(num_beams=9), ValueError, "num_beams"), (dict(logits=torch.zeros(3, 64, device=dev)), ValueError, "num_beams"),
                           (dict(eos=eos[:2]), TypeError, "eos"), (dict(walk=z(10)), TypeError, "walk"), (dict(logits=rows.half()), TypeError, "fp32"),
                           (dict(seq=z(2, 8, dt=torch.int64)), TypeError, "seq"), (dict(seq=z(1, 8)), TypeError, "seq"),
                           (dict(penalty=z(2)), TypeError, "penalty"), (dict(min_left=z(1)), TypeError, "min_left"),
                           (dict(append=z(2)), TypeError, "append"), (dict(vocab=65), RuntimeError, "lmi_beam_step_rules"),
                           (dict(logits=torch.zeros(2, 262148, device=dev), vocab=262145), ValueError, "vocab")):
        a = dict(dict(logits=rows, vocab=64, num_beams=2, eos=eos), **bad)
        a.update(kw)
        with pytest.raises(exc, match=match):
            ops.beam_step_rules(**a)
    with pytest.raises(RuntimeError, match="lmi_beam_step_rules"):
        ops._check(ops.lib.lmi_beam_step_rules(None, *([0] * 26)))    # null pointers
    assert all(not v.any() for k, v in bad.items() if k != "penalty")


# ---- the engine against a host loop ------------------------------------------------------------------------------------------------------
class HostLoop(R.HostLoop):
    """beam_ref.HostLoop with the processed rows: float64 log-softmax of ``decode_step``'s raw logits, ``rules64`` over the prompt ids as the
    caller passed them + that beam's tokens, eos banned while fewer than ``min_new_tokens`` tokens exist; then ``walk_of`` and
    ``BeamSearch`` as before.  ``cut`` / ``eps`` follow the same near-tie rule, on the processed totals."""

    def run(self, K, T, eos=(), length_penalty=1.0, early_stopping=False, n_return=1, rules=None):
        if rules is None:
            return super().run(K, T, eos, length_penalty, early_stopping, n_return)
        from leopard_amd.engine import KVCache
        eng, V = self.eng, self.cfg.text_config.vocab_size
        sup = [] if eng.suppress_tokens is None else [int(t) for t in eng.suppress_tokens.tolist()]
        prompt = [int(t) for t in self.ids.reshape(-1).tolist()]
        p, n, min_new = float(rules.repetition_penalty), int(rules.no_repeat_ngram_size), int(rules.min_new_tokens)
        P = eng.merged_len(self.ids)
        caches = [KVCache(self.cfg, P + T, self.dtype, self.dev) for _ in range(K)]
        rows = eng.prefill(self.ids, self.tiles, cache=caches[0]).logits_last.reshape(1, -1)[:, :V].double().cpu().numpy()
        for c in caches[1:]:
            for i in range(len(c.k)):
                c.k[i][:P].copy_(caches[0].k[i][:P]); c.v[i][:P].copy_(caches[0].v[i][:P])
            c.length = P
        search = beams.BeamSearch(K, T, length_penalty, early_stopping, n_return)
        scores, self.cut, self.eps, self.held_back = [0.0], None, [0.0], 0
        was, eng.use_graphs = eng.use_graphs, False
        try:
            while True:
                raw = rows - R.lse64(rows)[:, None]
                left = max(min_new - search.generated, 0)
                lp = np.stack([rules64(raw[b], prompt + search.beams[b], p, n, left, eos) for b in range(raw.shape[0])])
                walk = beams.walk_of(lp, scores, K, eos, sup)
                if left > 0 and eos:                                  # an eos the minimum length kept out of this step's first K ranks
                    free = beams.walk_of(np.stack([rules64(raw[b], prompt + search.beams[b], p, n, 0, eos) for b in range(raw.shape[0])]),
                                         scores, K, eos, sup)
                    self.held_back += any(c.is_eos and c.rank < K for c in free)
                kept = [c.total for c in beams.walk_of(lp, scores, K + 1, eos, sup) if not c.is_eos]
                gap = kept[K - 1] - kept[K] if len(kept) > K else INF
                if search.generated >= 1 and self.cut is None and gap <= R.NOISE * float(np.abs(rows).max()) * max(p, 1.0 / p):
                    self.cut = search.generated + 1
                if not search.step(walk):
                    break
                Lc = caches[0].length
                for i in range(len(caches[0].k)):
                    for which in ("k", "v"):
                        old = torch.stack([getattr(c, which)[i][P:Lc] for c in caches])
                        for b, c in enumerate(caches):
                            getattr(c, which)[i][P:Lc].copy_(old[search.parents[b]])
                scores = search.scores
                rows = np.stack([eng.decode_step(seq[-1], c)[:V].double().cpu().numpy() for seq, c in zip(search.beams, caches)])
                self.eps.append(R.NOISE * float(np.abs(rows).max()))
        finally:
            eng.use_graphs = was
        return search.results()


def engine_rules():
    from leopard_amd.engine import LogitsRules
    return dict(penalty=LogitsRules(repetition_penalty=1.3), ngram=LogitsRules(no_repeat_ngram_size=2), minimum=LogitsRules(min_new_tokens=4),
                all=LogitsRules(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=4))


def engine_cases():
    """(K, decode, early_stopping, length_penalty, rules): every rule alone and all three together at K = 1, 2, 4 in both decode modes."""
    return [(1, "shared", False, 1.0, "penalty"), (2, "copy", False, 1.0, "ngram"), (4, "shared", False, 1.0, "minimum"),
            (2, "shared", True, 0.0, "all"), (4, "copy", True, 1.0, "all"), (1, "copy", False, 2.0, "all"),
            (4, "copy", "never", 0.0, "penalty"), (2, "shared", False, 2.0, "minimum")]


def compare_with_host(eng, host: HostLoop, K, decode, es, lp, T, eos, rules):
    """beam_ref.compare_with_host with ``rules`` on both sides; the score tolerance is beam_ref.score_tol x max(p, 1 / p)."""
    want = host.run(K, T, eos, lp, es, K, rules)
    cut = host.cut
    n_ids = host.ids.numel()

    def agree(got, want):
        return len(got.sequences) == len(want) and all(g[0, n_ids:].tolist() == w[1] for g, w in zip(got.sequences, want))
    call = lambda T: eng.generate_beams(host.ids, host.tiles, K, max_new_tokens=T, eos_token_id=eos, length_penalty=lp, early_stopping=es,
                                        num_return_sequences=K, decode=decode, rules=rules)
    got = call(T)
    full = agree(got, want)
    if not full:
        assert cut is not None and cut > 1, (K, decode, es, lp, cut, [s.tolist() for s in got.sequences], want)
        want = host.run(K, cut - 1, eos, lp, es, K, rules)
        got = call(cut - 1)
        assert agree(got, want), (K, decode, es, lp, cut, [s.tolist() for s in got.sequences], want)
    p = float(rules.repetition_penalty)
    for g, s, (ws, wseq) in zip(got.sequences, got.scores, want):
        assert g.shape == (1, n_ids + len(wseq)) and g[0, :n_ids].tolist() == host.ids.reshape(-1).tolist()
        assert abs(s - ws) <= R.score_tol(host, len(wseq), lp) * max(p, 1.0 / p), (K, decode, es, lp, s, ws)
    assert got.scores == sorted(got.scores, reverse=True)
    return full, cut, want, got
