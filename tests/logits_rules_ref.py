"""Test helper: the torch-fp32 CPU restatement of lmi_decode_rules (leopard_amd/csrc/decode_rules.h) — repetition penalty, no-repeat
n-gram ban, min_new_tokens, in HF's processor order — and the device-agnostic kernel cases that tests/test_emu_logits_rules.py (emulator)
and tests/test_gpu_logits_rules.py (MI355X) both run.  The kernel's arithmetic is one IEEE fp32 multiply or divide per seen id and exact
-inf writes, so every comparison is bit for bit (``same_bits``: torch.equal that takes NaN == NaN)."""
import torch

NAN, INF = float("nan"), float("inf")


def apply(row, seq_ids, penalty, n, min_left, eos):
    """The three rules on one fp32 row [V] (a new tensor): ``seq_ids`` = every id seen so far (prompt + generated; ids outside [0, V) are
    compared in n-grams and never written), ``penalty`` (1 = off), ``n`` = no_repeat_ngram_size (0 = off), eos ids banned while
    ``min_left`` > 0 (entries < 0 unused)."""
    out = row.clone().to(torch.float32)
    V = out.numel()
    seq = [int(t) for t in seq_ids]
    L = len(seq)
    if float(penalty) != 1.0:
        ids = torch.tensor(sorted({t for t in seq if 0 <= t < V}), dtype=torch.int64)
        if ids.numel():
            p = torch.tensor(float(penalty), dtype=torch.float32)
            l = out[ids]
            out[ids] = torch.where(l < 0, l * p, l / p)
    n = int(n)
    if n > 0 and L + 1 >= n:
        tail = seq[L - (n - 1):] if n > 1 else []
        for i in range(L - n + 1):
            if seq[i:i + n - 1] == tail and 0 <= seq[i + n - 1] < V:
                out[seq[i + n - 1]] = -INF
    if int(min_left) > 0:
        for e in eos:
            if 0 <= int(e) < V:
                out[int(e)] = -INF
    return out


def same_bits(a, b):
    a, b = a.detach().cpu(), b.detach().cpu()
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and torch.equal(na, nb) and torch.equal(a[~na], b[~nb])


def random_rows(B, V, ld, seed, scale=4.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.full((B, ld), NAN)                                        # the padding columns hold NaN: they are never touched
    x[:, :V] = torch.randn(B, V, generator=g) * scale
    return x


class Case:
    """One launch: host tensors of every argument; ``seqs`` = the ids of each row BEFORE the append."""
    def __init__(self, x, V, seqs, penalty, ngram, min_left, eos=None, tok=None, live=None, seq_cap=None):
        B = x.shape[0]
        self.x, self.V, self.B = x, V, B
        self.seqs = [[int(t) for t in s] for s in seqs]
        self.cap = seq_cap if seq_cap is not None else max(max(len(s) for s in self.seqs) + 2, 4)
        self.seq = torch.full((B, self.cap), -77, dtype=torch.int32)   # the cells past seq_len hold a sentinel: never read, written by the append only
        for b, s in enumerate(self.seqs):
            self.seq[b, :len(s)] = torch.tensor(s, dtype=torch.int32)
        self.seq_len = torch.tensor([len(s) for s in self.seqs], dtype=torch.int32)
        self.penalty = torch.tensor([float(p) for p in penalty], dtype=torch.float32)
        self.ngram = torch.tensor([int(n) for n in ngram], dtype=torch.int32)
        self.min_left = torch.tensor([int(m) for m in min_left], dtype=torch.int32)
        self.eos = None if eos is None else torch.tensor([int(e) for e in eos], dtype=torch.int64)
        self.tok = None if tok is None else torch.tensor([int(t) for t in tok], dtype=torch.int64)
        self.live = None if live is None else torch.tensor([int(v) for v in live], dtype=torch.int32)

    def expected(self):
        """(logits, seq, seq_len, min_left) after the launch, from ``apply``."""
        x, seq, sl, ml = self.x.clone(), self.seq.clone(), self.seq_len.clone(), self.min_left.clone()
        for b in range(self.B):
            if self.live is not None and int(self.live[b]) == 0:
                continue
            s = list(self.seqs[b])
            if self.tok is not None and len(s) < self.cap:
                s.append(int(self.tok[b]))
                seq[b, len(s) - 1] = int(self.tok[b])
                sl[b] = len(s)
            x[b, :self.V] = apply(self.x[b, :self.V], s, float(self.penalty[b]), int(self.ngram[b]), int(ml[b]),
                                  [] if self.eos is None else self.eos.tolist())
            if int(ml[b]) > 0:
                ml[b] -= 1
        return x, seq, sl, ml

    def run(self, ops, dev):
        """One launch on ``dev``: (logits, seq, seq_len, min_left) on the host."""
        to = lambda t: None if t is None else t.clone().to(dev)
        x, seq, sl, ml = to(self.x), to(self.seq), to(self.seq_len), to(self.min_left)
        ops.decode_rules(x, self.V, seq, sl, to(self.penalty), to(self.ngram), ml, tok=to(self.tok), live=to(self.live), eos=to(self.eos))
        return x.cpu(), seq.cpu(), sl.cpu(), ml.cpu()

    def check(self, ops, dev, repeat=False):
        got, want = self.run(ops, dev), self.expected()
        assert same_bits(got[0], want[0]), self._diff(got[0], want[0])
        assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2]) and torch.equal(got[3], want[3]), (got[1:], want[1:])
        if repeat:                                                      # a second run from the same inputs: identical bits
            again = self.run(ops, dev)
            assert same_bits(again[0], got[0]) and all(torch.equal(a, g) for a, g in zip(again[1:], got[1:]))
        return got

    def _diff(self, got, want):
        bad = ~((got == want) | (torch.isnan(got) & torch.isnan(want)))
        idx = bad.nonzero()[:8].tolist()
        return [(i, float(got[i[0], i[1]]), float(want[i[0], i[1]])) for i in idx]


def heavy_seq(L, V, seed, extra=()):
    """L ids drawn from about sqrt(L) + 3 distinct ones (heavy duplicates; many repeated n-grams), with ``extra`` ids mixed in."""
    g = torch.Generator().manual_seed(seed)
    pool = torch.randint(0, V, (int(L ** 0.5) + 3,), generator=g).tolist() + list(extra)
    return [pool[i] for i in torch.randint(0, len(pool), (L,), generator=g).tolist()]


def special_row(x, b, seq, V):
    """Put zero, -0, +inf, -inf, NaN and a negative value on ids the sequence holds (and one of each on ids it does not)."""
    ids = [t for t in dict.fromkeys(seq) if 0 <= t < V]
    for k, v in enumerate((0.0, -0.0, INF, -INF, NAN, -3.25, 1e-30, -1e30)):
        if k < len(ids):
            x[b, ids[k]] = v
    free = [i for i in range(V) if i not in set(ids)][:5]
    for i, v in zip(free, (0.0, INF, -INF, NAN, -2.5)):
        x[b, i] = v


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
LENGTHS = (1, 2, 1023, 1024, 1025, 7200)                                # L after the append: below / at / above one 1024-thread stride, 8 strides
SMALL_V, SMALL_LD = 1000, 1024                                          # a vocabulary that is no multiple of 32, rows padded to 1024
BIG_V = 128256
IMAGE_ID = 128257                                                       # an id >= V that prompts hold (the image placeholder)


def check_lengths(ops, dev, V=SMALL_V, ld=SMALL_LD):
    """Every length of LENGTHS, all three rules on, heavy duplicates, out-of-range ids in the sequence, special values on seen ids."""
    for L in LENGTHS:
        seq = heavy_seq(L - 1, V, seed=L, extra=(-5, V, V + 31, IMAGE_ID))
        x = random_rows(1, V, ld, seed=100 + L)
        tok = [seq[L // 2]] if L > 2 else [7]
        special_row(x, 0, seq + tok, V)
        for n in (2, 3):
            Case(x, V, [seq], [1.3], [n], [2], eos=[3, -1, V - 1, V + 4], tok=tok, seq_cap=L + 3).check(ops, dev, repeat=L == 1025)


def check_batches(ops, dev, V=SMALL_V, ld=SMALL_LD):
    """B = 1, 3, 16 with different parameters per row; one row with everything off stays untouched while its seq grows."""
    for B in (1, 3, 16):
        seqs = [heavy_seq(5 + 37 * b, V, seed=B * 31 + b, extra=(V + b,)) for b in range(B)]
        x = random_rows(B, V, ld, seed=B)
        pens = [(0.7, 1.3, 2.0, 1.0)[b % 4] for b in range(B)]
        ns = [(0, 1, 2, 3)[(b + 1) % 4] for b in range(B)]
        mins = [(0, 1, 3)[b % 3] for b in range(B)]
        off = B - 1                                                     # the row with everything off
        pens[off], ns[off], mins[off] = 1.0, 0, 0
        for b in range(B):
            special_row(x, b, seqs[b], V)
        c = Case(x, V, seqs, pens, ns, mins, eos=[-1, 11, -1, 999], tok=[seqs[b][0] for b in range(B)])
        got = c.check(ops, dev, repeat=B == 3)
        assert same_bits(got[0][off], x[off]) and int(got[2][off]) == len(seqs[off]) + 1 and int(got[3][off]) == 0


def check_no_append(ops, dev, V=SMALL_V, ld=SMALL_LD):
    """tok = None: L = 0 (nothing seen: only the minimum-length rule acts) and L > 0 (the first-token form)."""
    x = random_rows(2, V, ld, seed=5)
    got = Case(x, V, [[], [4, 9, 4, 9, 4]], [2.0, 2.0], [1, 2], [1, 0], eos=[17, -1]).check(ops, dev)
    assert float(got[0][0, 17]) == -INF and got[2].tolist() == [0, 5] and got[3].tolist() == [0, 0]
    assert float(got[0][1, 9]) == -INF and float(got[0][1, 17]) == float(apply(x[1, :V], [4, 9, 4, 9, 4], 2.0, 0, 0, [])[17])


def check_one_id_repeated(ops, dev, V=SMALL_V, ld=SMALL_LD):
    """A sequence of one id: the penalty applies once, whatever the count."""
    for L, p in ((2, 0.7), (1500, 1.3), (1500, 2.0)):
        for val in (5.0, -5.0):
            x = random_rows(1, V, ld, seed=L)
            x[0, 42] = val
            got = Case(x, V, [[42] * (L - 1)], [p], [0], [0], tok=[42]).check(ops, dev)
            pt, vt = torch.tensor(p, dtype=torch.float32), torch.tensor(val, dtype=torch.float32)
            assert float(got[0][0, 42]) == float(vt * pt if val < 0 else vt / pt)


def banned(ops, dev, seq, n, V=64, ld=64):
    """The ids lmi_decode_rules sets to -inf for sequence ``seq`` (no append) under the n-gram rule alone, on a finite row."""
    x = random_rows(1, V, ld, seed=n)
    got = Case(x, V, [seq], [1.0], [n], [0]).check(ops, dev)
    return set((got[0][0, :V] == -INF).nonzero().reshape(-1).tolist())


def check_ngram_pins(ops, dev):
    """The cases pinned against transformers' NoRepeatNGramLogitsProcessor, and the edges of n."""
    s = [3, 5, 3, 7, 3, 5]
    assert banned(ops, dev, s, 1) == {3, 5, 7}
    assert banned(ops, dev, s, 2) == {3}
    assert banned(ops, dev, s, 3) == {3}
    assert banned(ops, dev, [4, 4, 4, 4], 3) == {4}
    assert banned(ops, dev, s, len(s) + 2) == set()                     # n = L + 2: no n-gram can be completed
    assert banned(ops, dev, s, len(s) + 1) == set()                     # n = L + 1: the rule runs over zero starts
    assert banned(ops, dev, [100, 5, 9, 100, 5], 3) == {9}              # an id >= V (100 >= 64) is compared ...
    assert banned(ops, dev, [5, 100, 5], 2) == set()                    # ... and never written


def check_min_left(ops, dev, V=SMALL_V, ld=SMALL_LD):
    """min_left 0, 1, 3 with unused (-1) and out-of-range eos entries; exactly one decrement per live step, none when frozen."""
    x = random_rows(4, V, ld, seed=9)
    seqs = [[1, 2], [1, 2], [1, 2], [1, 2]]
    c = Case(x, V, seqs, [1.0] * 4, [0] * 4, [0, 1, 3, 3], eos=[-1, 30, V, 31], tok=[8, 8, 8, 8], live=[1, 1, 1, 0])
    got = c.check(ops, dev)
    assert got[3].tolist() == [0, 0, 2, 3]
    assert same_bits(got[0][0], x[0]) and same_bits(got[0][3], x[3])
    for b in (1, 2):
        assert float(got[0][b, 30]) == -INF and float(got[0][b, 31]) == -INF
        keep = torch.ones(ld, dtype=torch.bool); keep[[30, 31]] = False
        assert same_bits(got[0][b][keep], x[b][keep])


def check_frozen_and_full(ops, dev, V=SMALL_V, ld=SMALL_LD):
    """live = 0: logits, seq, seq_len and min_left unchanged.  seq_len == seq_cap: nothing is written past the row (the next row's first
    cell and the sentinel after the last row stay), the rules still run over the full sequence."""
    x = random_rows(3, V, ld, seed=13)
    full = heavy_seq(6, V, seed=1)
    c = Case(x, V, [full, [9, 9, 9], full], [2.0, 2.0, 1.3], [1, 1, 2], [2, 2, 0], eos=[5], tok=[77, 78, 79], live=[1, 0, 1], seq_cap=6)
    c.seq[1, 3:] = -77
    got = c.check(ops, dev)
    assert got[2].tolist() == [6, 3, 6] and got[3].tolist() == [1, 2, 0]
    assert torch.equal(got[1], c.seq) and same_bits(got[0][1], x[1])
    assert 77 not in got[1].tolist()[0]


def check_production_vocab(ops, dev):
    """V = 128 256 (16 KB of bitmap), B = 3, a long sequence with an image id >= V in it."""
    V = BIG_V
    seqs = [heavy_seq(7199, V, seed=3, extra=(IMAGE_ID, V - 1, 0)), heavy_seq(40, V, seed=4, extra=(V - 1,)), [V - 1, 0, V - 1]]
    x = random_rows(3, V, V, seed=21)
    for b in range(3):
        special_row(x, b, seqs[b], V)
    Case(x, V, seqs, [1.3, 0.7, 2.0], [3, 2, 1], [1, 0, 2], eos=[128001, 128009, -1, -1], tok=[seqs[0][5], V - 1, 0]).check(ops, dev, repeat=True)


def check_rejects(ops, dev):
    """The argument checks: a vocabulary above 262 144, ld < vocab, wrong dtypes."""
    import pytest
    z = lambda *s, dt=torch.int32: torch.zeros(*s, dtype=dt, device=dev)
    x = torch.zeros(1, 64, device=dev)
    args = lambda: (z(1, 8), z(1), torch.ones(1, device=dev), z(1), z(1))
    ops.decode_rules(x, 64, *args())
    with pytest.raises(RuntimeError, match="lmi_decode_rules"):
        ops.decode_rules(x, 65, *args())                                # ld_logits < vocab
    with pytest.raises(RuntimeError, match="lmi_decode_rules: vocab"):
        ops.decode_rules(torch.zeros(1, 262145 + 3, device=dev), 262145, *args())
    with pytest.raises(TypeError):
        ops.decode_rules(x.half(), 64, *args())
    with pytest.raises(TypeError):
        ops.decode_rules(x, 64, z(1, 8, dt=torch.int64), *args()[1:])
    with pytest.raises(TypeError):
        ops.decode_rules(x, 64, *args(), tok=z(1))                      # tok must be int64
