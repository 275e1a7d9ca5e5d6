"""Test helper: the cases and plain references of the small row kernels that run in every layer or decode step — lmi_add_rmsnorm(_lo4),
lmi_rmsnorm_rows, lmi_decode_advance, the edges of lmi_decode_sample, lmi_split_hi_lo, rectangular lmi_preprocess_images and
lmi_gemm_bias_act.  Shared by tests/test_emu_row_kernels.py (emulator) and tests/test_gpu_row_kernels.py (MI355X): every case takes the
``Ops`` to drive and the device its tensors live on, builds its inputs on the CPU, and checks the kernel's output against float64 (the
tolerance checks) or against torch on the CPU (the bit-exact checks) — never against another launch of the kernel under test.  Identities
between sibling kernels are asserted on top of that.  Nothing is launched at import time."""
import numpy as np
import torch

from leopard_amd import _lib
from leopard_amd.ops import Lo4Act, lo4_k4
from tests.sampling_ref import draw_many, kept_set

DTYPES = [torch.float16, torch.bfloat16]
RMS_EPS = 1e-5
SENTINEL = 77.0                                  # exact in fp32, fp16 and bf16; no kernel here produces it
E2M1 = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


def eps(dtype) -> float:
    """One rounding of the 16-bit type (tests/test_gpu_kernels.py)."""
    return 2.0 ** -10 if dtype == torch.float16 else 2.0 ** -7


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Same shape, same dtype, same bytes (torch.equal would take -0.0 for +0.0)."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return bool(torch.equal(a.view(torch.uint8), b.view(torch.uint8)))


def sentinel_buf(rows: int, ld: int, dtype, dev, fill=SENTINEL) -> torch.Tensor:
    return torch.full((rows, ld), fill, dtype=dtype).to(dev)


def untouched(buf: torch.Tensor, M: int, D: int, fill=SENTINEL) -> bool:
    """The padding columns [D, ld) of the rows [0, M) and every row from M on still hold the sentinel."""
    b = buf.detach().cpu()
    return bool((b[:M, D:] == fill).all() and (b[M:] == fill).all())


def rel_err(out: torch.Tensor, ref64: torch.Tensor) -> float:
    """The project's measure (tests/test_gpu_kernels.py ``check``): max |out - ref| / (1 + |ref|)."""
    o = out.detach().cpu().double()
    return float(((o - ref64).abs() / (1.0 + ref64.abs())).max())


# ---- 1. / 2. the row norms ----------------------------------------------------------------------------------------------------------------
ADD_NORM_D = (8, 1152, 1536, 1544, 4096)         # one live lane; either side of the MAXV 3 / 8 dispatch; the limit
ADD_NORM_M = (1, 4, 5, 70)                       # four rows share a workgroup; 5 leaves three idle waves in the last one
LO4_D = (32, 96, 1152, 1536, 1568, 4096)         # K4 > D at 32, 96, 1152 and 1568
ROWS_D = (1152, 1544, 4096)
ROWS_N = (1, 3, 4, 5, 37)


def shaped_rows(M: int, D: int, seed: int) -> torch.Tensor:
    """fp32 [M, D] rows on which a kernel that loses part of a row shows up in the result: random rows alone hide a dropped 8-element
    chunk of the sum of squares below 2 eps.  Row 0 has most of its energy in its LAST chunk (x 30), row 1 in its FIRST, row 2 is all
    zeros (rstd = 1 / sqrt(eps)), row 3 has magnitude 1e3; the last three rows of a long stream repeat last / first / zero."""
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(M, D, generator=g) * 2.0 + 0.3
    kinds = {0: "last", 1: "first", 2: "zero", 3: "big"}
    if M > 8:
        kinds.update({M - 1: "last", M - 2: "first", M - 3: "zero"})
    for r, kind in kinds.items():
        if r >= M:
            continue
        if kind == "last":
            s[r, D - 8:] *= 30.0
        elif kind == "first":
            s[r, :8] *= 30.0
        elif kind == "zero":
            s[r] = 0.0
        else:
            s[r] *= 500.0
    return s


def norm_weight(D: int, seed: int = 4) -> torch.Tensor:
    return torch.rand(D, generator=torch.Generator().manual_seed(seed)) + 0.5


def rmsnorm_ref64(s: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """w * s * rsqrt(mean(s^2) + eps) in float64 on the CPU."""
    s64 = s.detach().cpu().double()
    return w.detach().cpu().double() * s64 * torch.rsqrt(s64.pow(2).mean(-1, keepdim=True) + RMS_EPS)


def add_inputs(M: int, D: int, delta_dtype, seed: int):
    """(x0 fp32, delta, the fp32 sum torch computes on the CPU): x0 + delta lands on shaped_rows (its zero row exactly)."""
    s = shaped_rows(M, D, seed)
    g = torch.Generator().manual_seed(seed + 1)
    delta = (torch.randn(M, D, generator=g) * 0.5).to(delta_dtype)
    x0 = s - delta.float()
    want = x0 + delta.float()
    assert (want[2] == 0).all() if M > 2 else True
    return x0, delta, want


def check_add_rmsnorm(ops, dev, dtype, delta_dtype, M: int, D: int) -> float:
    """lmi_add_rmsnorm on strided buffers with sentinels; returns the fp64 error of ``out`` (asserted <= 2 eps(T))."""
    x0, delta, want = add_inputs(M, D, delta_dtype, seed=1000 + D + M)
    w = norm_weight(D).to(dev)
    ldx, ldd, ldo = D + 12, D + 8, D + 24
    xbuf = sentinel_buf(M + 1, ldx, torch.float32, dev)
    dbuf = sentinel_buf(M + 1, ldd, delta_dtype, dev)
    obuf = sentinel_buf(M + 1, ldo, dtype, dev)
    xbuf[:M, :D] = x0.to(dev)
    dbuf[:M, :D] = delta.to(dev)
    x, out = xbuf[:M, :D], obuf[:M, :D]
    ops.add_rmsnorm(x, dbuf[:M, :D], w, out, RMS_EPS)
    assert bits_equal(x, want), "x after the call != x + float(delta) (torch, CPU)"
    assert untouched(xbuf, M, D) and untouched(obuf, M, D) and bits_equal(dbuf[:M, :D], delta) and untouched(dbuf, M, D)
    err = rel_err(out, rmsnorm_ref64(want, w))
    assert err <= 2 * eps(dtype), f"add_rmsnorm {dtype} M={M} D={D}: rel err {err:.3e} > {2 * eps(dtype):.3e}"
    # the sibling: the same rows through lmi_rmsnorm_rows, bit for bit (an identity on top of the reference above)
    sib = sentinel_buf(M, D, dtype, dev)
    ops.rmsnorm_rows(x, torch.arange(M, dtype=torch.int64).to(dev), w, sib, RMS_EPS)
    assert bits_equal(out, sib), "add_rmsnorm != rmsnorm_rows of the sum"
    return err


def check_add_only(ops, dev, delta_dtype, M: int, D: int):
    """out = None, w = None: the add alone."""
    x0, delta, want = add_inputs(M, D, delta_dtype, seed=2000 + D + M)
    ldx, ldd = D + 12, D + 8
    xbuf = sentinel_buf(M + 1, ldx, torch.float32, dev)
    dbuf = sentinel_buf(M + 1, ldd, delta_dtype, dev)
    xbuf[:M, :D] = x0.to(dev)
    dbuf[:M, :D] = delta.to(dev)
    ops.add_rmsnorm(xbuf[:M, :D], dbuf[:M, :D], None, None, RMS_EPS)
    assert bits_equal(xbuf[:M, :D], want) and untouched(xbuf, M, D) and bits_equal(dbuf[:M, :D], delta) and untouched(dbuf, M, D)


def decode_img(img: torch.Tensor, sc: torch.Tensor, K: int, per_row: bool = False) -> torch.Tensor:
    """fp4 image [M, K4 / 2] bytes + E8M0 scales ([M, K4 / 32] or [M] with per_row) -> fp32 [M, K] (independent of the kernels)."""
    M, half = img.shape
    b = img.to(torch.int64)
    codes = torch.stack([b & 15, b >> 4], dim=-1).reshape(M, half * 2)           # element k in nibble k & 1 of byte k >> 1
    val = E2M1[codes & 7] * torch.where((codes & 8) != 0, -1.0, 1.0)
    s = torch.exp2(sc.to(torch.float32) - 127.0)
    s = s[:, None].expand(M, half * 2) if per_row else s[:, :half * 2 // 32].repeat_interleave(32, dim=1)
    return (val * s)[:, :K]


def assert_lo4_norm_output(hi: torch.Tensor, img: torch.Tensor, sc: torch.Tensor, plain: torch.Tensor, y: torch.Tensor, D: int):
    """What a norm producer of a Lo4Act owes (CPU tensors): ``hi`` is the 16-bit operand the fast schedule hands over (``plain``), the
    decoded image (the oracle's e2m1 / E8M0 grid) carries most of the rounding residual y - hi of the fp32 norm ``y``, and the padding
    up to K4 reads as zero codes and zero scales."""
    assert torch.equal(hi, plain)                                         # the 16-bit operand is the one the fast schedule hands over
    lo = decode_img(img, sc, D)
    before = (y - hi.float()).pow(2).mean().sqrt().item()
    after = (y - hi.float() - lo).pow(2).mean().sqrt().item()
    assert after < 0.25 * before, (before, after)
    k4 = lo4_k4(D)
    if k4 > D:
        assert img[:, D // 2:].abs().max() == 0 and sc[:, D // 32:k4 // 32].abs().max() == 0


def _lo4_bufs(M: int, D: int, dtype, dev, ldo: int, ld4: int, lds: int, img_fill: int, sc_fill: int):
    k4 = lo4_k4(D)
    hbuf = sentinel_buf(M + 1, ldo, dtype, dev)
    ibuf = sentinel_buf(M + 1, ld4, torch.uint8, dev, img_fill)
    sbuf = sentinel_buf(M + 1, lds, torch.uint8, dev, sc_fill)
    return (hbuf, ibuf, sbuf), Lo4Act(hbuf[:M, :D], ibuf[:M, :k4 // 2], sbuf[:M, :k4 // 32])


def check_add_rmsnorm_lo4(ops, dev, dtype, delta_dtype, M: int, D: int) -> float:
    """lmi_add_rmsnorm_lo4: x as above, ``hi`` against fp64, the (hi, img, sc) triple against lmi_norm_lo4 of the sum byte for byte
    (padding up to K4 included; the two sides start from different garbage), and the producer's contract of assert_lo4_norm_output."""
    x0, delta, want = add_inputs(M, D, delta_dtype, seed=3000 + D + M)
    w = norm_weight(D).to(dev)
    k4 = lo4_k4(D)
    ldx, ldd = D + 12, D + 8
    xbuf = sentinel_buf(M + 1, ldx, torch.float32, dev)
    dbuf = sentinel_buf(M + 1, ldd, delta_dtype, dev)
    xbuf[:M, :D] = x0.to(dev)
    dbuf[:M, :D] = delta.to(dev)
    x = xbuf[:M, :D]
    (hbuf, ibuf, sbuf), act = _lo4_bufs(M, D, dtype, dev, D + 24, k4 // 2 + 16, k4 // 32 + 4, 0xAB, 0xCD)
    ops.add_rmsnorm_lo4(x, dbuf[:M, :D], w, act, RMS_EPS)
    assert bits_equal(x, want), "x after the call != x + float(delta) (torch, CPU)"
    assert untouched(xbuf, M, D) and untouched(hbuf, M, D) and untouched(ibuf, M, k4 // 2, 0xAB) and untouched(sbuf, M, k4 // 32, 0xCD)
    err = rel_err(act.hi, rmsnorm_ref64(want, w))
    assert err <= 2 * eps(dtype), f"add_rmsnorm_lo4 {dtype} M={M} D={D}: rel err {err:.3e} > {2 * eps(dtype):.3e}"
    # the sibling producer on the sum, other strides, other garbage
    (hbuf2, ibuf2, sbuf2), act2 = _lo4_bufs(M, D, dtype, dev, D + 8, k4 // 2 + 32, k4 // 32 + 8, 0x5A, 0x3C)
    ops.norm_lo4(x, w, None, act2, RMS_EPS)
    assert untouched(hbuf2, M, D) and untouched(ibuf2, M, k4 // 2, 0x5A) and untouched(sbuf2, M, k4 // 32, 0x3C)
    assert bits_equal(act.hi, act2.hi) and bits_equal(act.img, act2.img) and bits_equal(act.sc, act2.sc)
    # the 16-bit rows of the fast schedule, and the producer's contract against the fp32 norm
    plain = sentinel_buf(M, D, dtype, dev)
    ops.rmsnorm_rows(x, torch.arange(M, dtype=torch.int64).to(dev), w, plain, RMS_EPS)
    wc = w.cpu()
    y = wc * (want * torch.rsqrt(want.pow(2).mean(-1, keepdim=True) + RMS_EPS))
    for a in (act, act2):
        assert_lo4_norm_output(a.hi.cpu(), a.img.cpu(), a.sc.cpu(), plain.cpu(), y, D)
    return err


def gather_rows(n: int, S: int) -> torch.Tensor:
    """int64 [n] row indices into an S-row stream: out of order, with a repeat (n >= 3), row 0 and row S - 1 included (n >= 3)."""
    base = [v for v in (S - 1, 0, S - 1, 17, 3, 33, 32, 31, 64, 5) if v < S]
    rows = (base +[int(v) for v in torch.randperm(S, generator=torch.Generator().manual_seed(n)).tolist()])[:n]
    return torch.tensor(rows, dtype=torch.int64)


def check_rmsnorm_rows(ops, dev, dtype, n: int, D: int, S: int = 70) -> float:
    """lmi_rmsnorm_rows on a strided S-row stream: fp64 tolerance; for a stream of more than 32 rows also the bits of lmi_rmsnorm."""
    x0 = shaped_rows(S, D, seed=4000 + D)
    w = norm_weight(D).to(dev)
    rows = gather_rows(n, S)
    ldx, ldo = D + 12, D + 24
    xbuf = sentinel_buf(S + 1, ldx, torch.float32, dev)
    xbuf[:S, :D] = x0.to(dev)
    obuf = sentinel_buf(n + 1, ldo, dtype, dev)
    out = obuf[:n, :D]
    ops.rmsnorm_rows(xbuf[:S, :D], rows.to(dev), w, out, RMS_EPS)
    assert untouched(obuf, n, D) and bits_equal(xbuf[:S, :D], x0) and untouched(xbuf, S, D)
    err = rel_err(out, rmsnorm_ref64(x0[rows], w))
    assert err <= 2 * eps(dtype), f"rmsnorm_rows {dtype} n={n} D={D} S={S}: rel err {err:.3e} > {2 * eps(dtype):.3e}"
    if S > 32:                                                            # lmi_rmsnorm's one-wave-per-row kernel: the same bits
        full = sentinel_buf(S, D, dtype, dev)
        ops.rmsnorm(xbuf[:S, :D], w, full, RMS_EPS)
        assert bits_equal(out, full.cpu()[rows]), "rmsnorm_rows != rmsnorm(stream)[rows]"
    return err


# ---- 3. lmi_decode_advance ----------------------------------------------------------------------------------------------------------------
def check_decode_advance_stop_rule_and_history(ops, dev):
    """lmi_decode_advance: per-row argmax (lowest index on ties, suppressed ids excluded), history ring, stop rule (eos ids, budget) and the
    frozen state of stopped sequences, against a plain restatement."""
    B, V, ld, H = 5, 1003, 1024, 3                                  # 250 vector loads + a 3-element tail per row
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(B, ld, generator=g)
    logits[:, V:] = 100.0                                           # padding columns past the vocabulary must be ignored
    logits[1, 17] = logits[1, 400] = 50.0                           # a tie: the lower index wins
    logits[2, 5] = 60.0                                             # suppressed: the runner-up must be chosen
    suppress = torch.tensor([5], dtype=torch.int64).to(dev)
    want = []
    for b in range(B):
        row = logits[b, :V].clone()
        row[5] = float("-inf")
        want.append(int(row.argmax()))
    want[1] = 17
    logits_d = logits.to(dev)
    tok = torch.zeros(B, dtype=torch.int64).to(dev)
    pos = torch.tensor([10, 20, 30, 40, 50], dtype=torch.int32).to(dev)
    k_len = pos + 1
    live = torch.tensor([1, 1, 0, 1, 1], dtype=torch.int32).to(dev)         # sequence 2 already stopped
    budget = torch.tensor([5, 1, 9, 7, 3], dtype=torch.int32).to(dev)       # sequence 1 produces its last token now
    eos = torch.tensor([want[3], -1], dtype=torch.int64).to(dev)            # sequence 3 hits its eos
    hist = torch.full((H, B), -7, dtype=torch.int64).to(dev)
    hist_pos = torch.tensor([0, 1, 2, 3, 4], dtype=torch.int32).to(dev)
    ops.decode_advance(logits_d, V, tok, pos, k_len=k_len, live=live, budget=budget, eos=eos, hist=hist, hist_pos=hist_pos, suppress=suppress)
    assert tok.tolist() == want
    assert live.tolist() == [1, 0, 0, 0, 1] and budget.tolist() == [4, 0, 9, 6, 2]
    assert pos.tolist() == [11, 20, 30, 40, 51] and k_len.tolist() == [12, 21, 31, 41, 52]
    assert hist_pos.tolist() == [1, 2, 3, 4, 5]
    for b in range(B):
        assert int(hist[b % H, b]) == want[b]
    # the batch-1 form: no live / budget / history
    t1, p1, k1 = torch.zeros(1, dtype=torch.int64).to(dev), torch.tensor([7], dtype=torch.int32).to(dev), torch.tensor([8], dtype=torch.int32).to(dev)
    ops.decode_advance(logits_d[4:5], V, t1, p1, k_len=k1)
    assert int(t1) == int(logits[4, :V].argmax()) and int(p1) == 8 and int(k1) == 9


def advance_rows(V: int, ld: int):
    """(logits [B, ld] fp32, the token every row must give, the suppressed ids): rows whose answer is known by construction.  The scan
    gives thread t the elements 4 (t + 1024 u + 4096 trip) .. + 3: one trip of the four-loads-in-flight loop covers 16384 elements."""
    big = V > 20000
    sup = [7, 16390 if big else 900]
    g = torch.Generator().manual_seed(V + ld)
    rows, want = [], []

    def row(**at):
        r = torch.rand(V, generator=g) - 1.0                            # background in [-1, 0)
        for i, v in at.items():
            r[int(i[1:])] = v
        return r

    def add(r, tok):
        rows.append(r); want.append(tok)

    add(row(_0=5.0), 0)                                                 # the maximum at index 0
    add(row(**{f"_{V - 1}": 5.0}), V - 1)                               # ... at V - 1 (in the tail when V % 4 != 0)
    if big:
        add(row(_16383=5.0), 16383)                                     # the last element of the first trip
        add(row(_16384=5.0), 16384)                                     # the first element of the second
    add(row(_40=5.0, _200=5.0), 40)                                     # two equal maxima inside one wave's reach
    add(row(_41=5.0, _42=5.0), 41)                                      # ... inside one lane's four elements
    if big:
        add(row(_4000=5.0, _4104=5.0), 4000)                            # ... in two waves: the lower index sits in wave 15, the higher in wave 0
        add(row(_100=5.0, _16484=5.0), 100)                             # ... of one thread in two loop trips
        add(row(_20000=5.0, _120000=5.0, _128255=5.0), 20000)
    else:
        add(row(_40=5.0, _773=5.0), 40)                                 # ... in two waves
    add(row(_7=9.0, _500=5.0), 500)                                     # the maximum suppressed
    add(row(**{"_7": 9.0, f"_{sup[1]}": 8.0, "_600": 5.0}), 600)        # the two largest both suppressed
    add(row(_321=float("inf")), 321)                                    # +inf is a value like any other
    r = row(_556=5.0)
    r[::37] = float("nan")                                              # NaNs among finite values (index 0 included) are ignored
    add(r, 556)
    add(torch.full((V,), float("nan")), 0)                              # nothing to choose: token 0
    add(torch.full((V,), float("-inf")), 0)
    r = torch.full((V,), float("-inf"))
    r[7] = 1.0                                                          # the only finite entry is suppressed
    add(r, 0)
    logits = torch.full((len(rows), ld), 100.0)                         # padding columns past the vocabulary hold 100.0
    logits[:, :V] = torch.stack(rows)
    return logits, want, sup


def advance_tail_ref(tok, pos, k_len, live, budget, eos, hist, hist_pos):
    """decode_advance_tail restated on Python lists (in place): history ring, budget, eos, live mask, position / key-count advance."""
    H = len(hist)
    for b, t in enumerate(tok):
        lv = live[b]
        hist[hist_pos[b] % H][b] = t
        hist_pos[b] += 1
        budget[b] -= lv
        if budget[b] <= 0 or t in [e for e in eos if e >= 0]:
            lv = 0
        live[b] = lv
        pos[b] += lv
        k_len[b] += lv


def check_decode_advance_rows(ops, dev, V: int, ld: int):
    logits, want, sup = advance_rows(V, ld)
    B, H = len(want), 3
    pos = [10 * b + 3 for b in range(B)]
    k_len = [p + 1 for p in pos]
    live = [0 if b % 5 == 2 else 1 for b in range(B)]
    budget = [1 if b % 4 == 1 else 6 for b in range(B)]
    eos = [want[3], -1, V - 1]
    hist = [[-7] * B for _ in range(H)]
    hist_pos = [b for b in range(B)]
    i32 = lambda v: torch.tensor(v, dtype=torch.int32).to(dev)
    i64 = lambda v: torch.tensor(v, dtype=torch.int64).to(dev)
    d = dict(pos=i32(pos), k_len=i32(k_len), live=i32(live), budget=i32(budget), eos=i64(eos), hist=i64(hist), hist_pos=i32(hist_pos))
    tok = torch.full((B,), -1, dtype=torch.int64).to(dev)
    ops.decode_advance(logits.to(dev), V, tok, d["pos"], k_len=d["k_len"], live=d["live"], budget=d["budget"], eos=d["eos"], hist=d["hist"],
                       hist_pos=d["hist_pos"], suppress=i64(sup))
    assert tok.tolist() == want
    advance_tail_ref(want, pos, k_len, live, budget, eos, hist, hist_pos)
    got = {k: v.tolist() for k, v in d.items()}
    assert got == dict(pos=pos, k_len=k_len, live=live, budget=budget, eos=eos, hist=hist, hist_pos=hist_pos)
    assert 0 in live and 1 in live                                       # the case does stop some rows and keep others


def check_decode_advance_full_batch(ops, dev, B: int = 64, V: int = 128256):
    """One launch of B rows of the production vocabulary with distinct random maxima, against argmax on the CPU."""
    g = torch.Generator().manual_seed(9)
    logits = torch.randn(B, V, generator=g)
    where = torch.randperm(V, generator=g)[:B]
    logits[torch.arange(B), where] = 10.0 + torch.rand(B, generator=g)
    tok = torch.full((B,), -1, dtype=torch.int64).to(dev)
    pos = torch.zeros(B, dtype=torch.int32).to(dev)
    ops.decode_advance(logits.to(dev), V, tok, pos)
    assert tok.tolist() == logits.argmax(dim=1).tolist() == where.tolist() and pos.tolist() == [1] * B


# ---- 4. the edges of lmi_decode_sample ----------------------------------------------------------------------------------------------------
def gapped_row(V: int, head, seed: int = 0, ld: int = None) -> torch.Tensor:
    """A logits row whose top tokens sit at scattered indices with the given values; the rest far below."""
    g = torch.Generator().manual_seed(seed)
    row = torch.full((ld or V,), 100.0)                               # padding past the vocabulary must never be drawn
    row[:V] = -20.0 + torch.rand(V, generator=g)
    where = torch.randperm(V, generator=g)[:len(head)]
    for i, v in zip(where.tolist(), head):
        row[i] = v
    return row


HEAD = [4.0, 3.6, 3.5, 3.0, 2.9, 2.2, 2.0, 1.1, 1.0, 0.2, -0.5, -3.0]


def check_kept_set_ties_keep_the_lower_indices(ops, dev):
    V = 512
    row = torch.full((V,), -200.0)
    tie = [7, 40, 41, 300, 301, 450]
    row[tie] = 2.0
    row[100] = 3.0
    # top-k = 3: 100 plus the two lowest tied indices
    draws = draw_many(ops, row.to(dev), V, 1.0, 3, 1.0, n_rows=64, n_steps=6)
    assert set(draws.tolist()) == {100, 7, 40} == set(kept_set(row, V, 1.0, 3, 1.0))
    # top-p alone over six equal tokens: mass 1/2 -> exactly three, the lowest indices
    row2 = torch.full((V,), -200.0)                                 # (no mass outside the tie group: the cut lands exactly on 1/2)
    row2[tie] = 1.0
    draws = draw_many(ops, row2.to(dev), V, 1.0, 0, 0.5, n_rows=64, n_steps=6)
    assert set(draws.tolist()) == {7, 40, 41} == set(kept_set(row2, V, 1.0, 0, 0.5))
    # top-k and top-p together, the cut inside the tie group (0.375 of five: two)
    draws = draw_many(ops, row2.to(dev), V, 1.0, 5, 0.375, n_rows=64, n_steps=6)
    assert set(draws.tolist()) == {7, 40} == set(kept_set(row2, V, 1.0, 5, 0.375))


def check_suppressed_ids_are_never_drawn(ops, dev):
    V = 600
    row = gapped_row(V, HEAD, seed=2)
    top = kept_set(row, V, 1.0, 3, 1.0)
    sup = torch.tensor(top[:2], dtype=torch.int64).to(dev)
    draws = draw_many(ops, row.to(dev), V, 1.0, 4, 1.0, n_rows=64, n_steps=8, suppress=sup)
    want = kept_set(row, V, 1.0, 4, 1.0, suppress=top[:2])
    assert not (set(draws.tolist()) & set(top[:2])) and set(draws.tolist()) == set(want)


def check_top_k_1_is_decode_advance_and_shares_its_stop_rule(ops, dev):
    """top_k = 1 gives decode_advance's argmax (its tie and suppress rules), and the history ring, budget, eos, live mask and position
    advance are those of check_decode_advance_stop_rule_and_history; the step counter advances for live rows only."""
    B, V, ld, H = 5, 1003, 1024, 3
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(B, ld, generator=g)
    logits[:, V:] = 100.0
    logits[1, 17] = logits[1, 400] = 50.0
    logits[2, 5] = 60.0
    suppress = torch.tensor([5], dtype=torch.int64).to(dev)
    want = []
    for b in range(B):
        row = logits[b, :V].clone()
        row[5] = float("-inf")
        want.append(int(row.argmax()))
    want[1] = 17
    logits = logits.to(dev)
    outs = []
    for kernel in ("advance", "sample"):
        tok = torch.zeros(B, dtype=torch.int64).to(dev)
        pos = torch.tensor([10, 20, 30, 40, 50], dtype=torch.int32).to(dev)
        k_len = pos + 1
        live = torch.tensor([1, 1, 0, 1, 1], dtype=torch.int32).to(dev)
        budget = torch.tensor([5, 1, 9, 7, 3], dtype=torch.int32).to(dev)
        eos = torch.tensor([want[3], -1], dtype=torch.int64).to(dev)
        hist = torch.full((H, B), -7, dtype=torch.int64).to(dev)
        hist_pos = torch.tensor([0, 1, 2, 3, 4], dtype=torch.int32).to(dev)
        step = torch.tensor([3, 3, 3, 3, 3], dtype=torch.int32).to(dev)
        kw = dict(k_len=k_len, live=live, budget=budget, eos=eos, hist=hist, hist_pos=hist_pos, suppress=suppress)
        if kernel == "advance":
            ops.decode_advance(logits, V, tok, pos, **kw)
        else:
            ops.decode_sample(logits, V, torch.full((B,), 0.7).to(dev), torch.ones(B, dtype=torch.int32).to(dev), torch.full((B,), 0.9).to(dev),
                              torch.arange(B, dtype=torch.int64).to(dev), step, tok, pos, **kw)
            assert step.tolist() == [4, 4, 3, 4, 4]                  # the frozen row's counter stays
        outs.append([t.tolist() for t in (tok, pos, k_len, live, budget, hist, hist_pos)])
    assert outs[0] == outs[1]
    assert outs[1][0] == want
    assert outs[1][3] == [1, 0, 0, 0, 1] and outs[1][1] == [11, 20, 30, 40, 51]


def check_rows_without_a_drawable_token_give_token_zero(ops, dev):
    row = torch.full((2, 64), float("-inf"))
    row[1, :] = float("nan")
    tok = torch.full((2,), 9, dtype=torch.int64).to(dev)
    ops.decode_sample(row.to(dev), 64, torch.ones(2).to(dev), torch.zeros(2, dtype=torch.int32).to(dev), torch.full((2,), 0.5).to(dev),
                      torch.zeros(2, dtype=torch.int64).to(dev), torch.zeros(2, dtype=torch.int32).to(dev), tok, torch.zeros(2, dtype=torch.int32).to(dev))
    assert tok.tolist() == [0, 0]


def check_draw_depends_on_seed_step_and_row_only(ops, dev):
    V = 777
    g = torch.Generator().manual_seed(5)
    rows = (torch.randn(8, 800, generator=g) * 2).to(dev)

    def call(logits, seeds, steps, T=0.9, k=40, p=0.95):
        B = logits.shape[0]
        tok = torch.zeros(B, dtype=torch.int64).to(dev)
        st = torch.tensor(steps, dtype=torch.int32).to(dev)
        ops.decode_sample(logits, V, torch.full((B,), T).to(dev), torch.full((B,), k, dtype=torch.int32).to(dev), torch.full((B,), p).to(dev),
                          torch.tensor(seeds, dtype=torch.int64).to(dev), st, tok, torch.zeros(B, dtype=torch.int32).to(dev))
        return tok.tolist()
    alone = [call(rows[5:6].clone(), [123456789012345], [s])[0] for s in range(40)]
    seeds = [1, 2, 3, 4, 5, 123456789012345, 7, 8]
    batched = [call(rows.clone(), seeds, [s] * 8)[5] for s in range(40)]
    assert alone == batched
    other = [call(rows[5:6].clone(), [987654321], [s])[0] for s in range(40)]
    assert other != alone
    assert len(set(alone)) > 3                                        # it does sample


def check_kept_set_on_unaligned_rows(ops, dev, T: float, k: int, p: float):
    """V odd, ld_logits = V + 1: every odd row of the launch starts 8 bytes off a 16-byte boundary and takes sample_for_row's scalar
    path, every even row its vector path with a one-element tail; the draws of both are exactly the float64 kept set."""
    V = 1001
    row = gapped_row(V, HEAD, seed=7, ld=V + 1)
    kept = kept_set(row, V, T, k, p)
    rows = np.arange(64)
    draws = draw_many(ops, row.to(dev), V, T, k, p, n_rows=64, n_steps=12).reshape(12, 64)
    for parity in (0, 1):                                             # vector rows, scalar rows
        assert set(draws[:, rows % 2 == parity].reshape(-1).tolist()) == set(kept), parity


# ---- 5. lmi_split_hi_lo, rectangular lmi_preprocess_images, lmi_gemm_bias_act -------------------------------------------------------------
SPLIT_SHAPES = [(70, 128), (3, 8), (1, 4096)]


def split_input(M: int, K: int):
    """(x, tiny): normal-range random values; the second half of the last row near 1e-6 (``tiny``: its hi and lo are fp16 subnormals)."""
    g = torch.Generator().manual_seed(51 + M + K)
    x = torch.randn(M, K, generator=g)
    tiny = torch.zeros(M, K, dtype=torch.bool)
    tiny[M - 1, K // 2:] = True
    n = K - K // 2
    x[M - 1, K // 2:] = (torch.rand(n, generator=g) + 0.5) * 1e-6 * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    return x, tiny


def run_split_hi_lo(ops, dev, dtype, M: int, K: int):
    """(out [M, 2K] on the CPU, x, tiny): the launch on strided buffers, sentinels and the source checked here."""
    x, tiny = split_input(M, K)
    ldx, ldo = K + 4, 2 * K + 8
    xbuf = sentinel_buf(M + 1, ldx, torch.float32, dev)
    xbuf[:M, :K] = x.to(dev)
    obuf = sentinel_buf(M + 1, ldo, dtype, dev)
    ops.split_hi_lo(xbuf[:M, :K], obuf[:M, :2 * K])
    assert untouched(obuf, M, 2 * K) and bits_equal(xbuf[:M, :K], x) and untouched(xbuf, M, K)
    return obuf[:M, :2 * K].cpu(), x, tiny


def check_split_hi_lo(ops, dev, dtype, M: int, K: int):
    out, x, tiny = run_split_hi_lo(ops, dev, dtype, M, K)
    hi = x.to(dtype)
    lo = (x - hi.float()).to(dtype)
    if dtype == torch.float16:
        assert (hi[tiny].float().abs() < 2.0 ** -14).all() and (hi[tiny] != 0).all()          # those values do sit in the subnormal range
    got_hi, got_lo = out[:, :K], out[:, K:]
    assert bits_equal(got_hi[~tiny], hi[~tiny]) and bits_equal(got_lo[~tiny], lo[~tiny]), "normal-range values"
    assert bits_equal(got_hi[tiny], hi[tiny]) and bits_equal(got_lo[tiny], lo[tiny]), "the values near 1e-6 (gradual underflow)"


def check_preprocess_rectangular_image(ops, dev, dtype=torch.float16):
    n, H, W, P, ldo = 2, 45, 61, 14, 640                       # 3 x 4 patches, remainder pixels dropped
    pix = (torch.randn((n, 3, H, W), generator=torch.Generator().manual_seed(94))).to(torch.float32)
    out = torch.full((n * 12, ldo), 7.0, dtype=dtype).to(dev)
    ops.preprocess_images(pix.contiguous().to(dev), out, P)
    out = out.cpu()
    ref = torch.nn.functional.unfold(pix[:, :, :42, :56], kernel_size=P, stride=P).transpose(1, 2).reshape(n * 12, 588)
    assert torch.equal(out[:, :588].float(), ref.to(dtype).float()) and out[:, 588:].abs().max() == 0
    u8 = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (1, H, W, 3), dtype=np.uint8))
    out2 = torch.empty(12, ldo, dtype=dtype).to(dev)
    ops.preprocess_images(u8.to(dev), out2, P)
    out2 = out2.cpu()
    from leopard_amd.tiler import siglip_normalize
    ref2 = torch.nn.functional.unfold(torch.from_numpy(siglip_normalize(u8.numpy()))[:, :, :42, :56], kernel_size=P, stride=P)
    assert torch.equal(out2[:, :588].float(), ref2.transpose(1, 2).reshape(12, 588).to(dtype).float())
    assert out2[:, 588:].abs().max() == 0


def check_gemm_bias_act(ops, dev, dtype):
    """lmi_gemm_bias_act, bias + GELU-tanh and bias + residual, against fp32 on the CPU with test_gemm_store_bias's measure (4 eps(T))."""
    M, N, K = 70, 128, 64
    g = torch.Generator().manual_seed(31)
    a = torch.randn(M, K, generator=g).to(dtype)
    w = (torch.randn(N, K, generator=g) * 0.05).to(dtype)
    bias = torch.randn(N, generator=g)
    lin = a.float() @ w.float().T + bias
    out = torch.full((M, N), float("nan"), dtype=dtype).to(dev)
    ops.gemm_bias_act(a.to(dev), w.to(dev), out, bias=bias.to(dev), act=_lib.ACT_GELU_TANH)
    ref = torch.nn.functional.gelu(lin, approximate="tanh")
    err = rel_err(out, ref.double())
    assert err <= 4 * eps(dtype), f"gemm_bias_act gelu {dtype}: rel err {err:.3e}"
    x0 = torch.randn(M, N, generator=g)
    x = x0.clone().to(dev)
    ops.gemm_bias_act(a.to(dev), w.to(dev), x, bias=bias.to(dev), residual=True)
    err = rel_err(x, (x0 + lin).double())
    assert err <= 4 * eps(dtype), f"gemm_bias_act residual {dtype}: rel err {err:.3e}"
