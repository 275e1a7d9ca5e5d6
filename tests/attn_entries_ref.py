"""Test helper: what the calls of tests/attn_entries_case.py must COMPUTE.  Shared by tests/test_emu_attn_entries_values.py (the CPU emulator)
and tests/test_gpu_attn_entries.py (the device): every check takes the Ops object and the device its tensors live on.  No fixtures, no hooks.

VISIBILITY MODEL (``model``).  Per case and query row, the [lo, hi) key ranges the row sees, each in the buffer it lives in ("own": the packed
k / the pooled cache, "prefix": the shared prefix rows), written from the semantics include/leopard_amd.h documents and from nothing else:
bottom-right causal alignment (key j visible to query i iff j <= i + len_k - len_q), the sliding window (i + len_k - len_q - j < window), the
k_begin / k_len slots, the device prefix_len below max_prefix, prefix plus own rows.  ``d`` = {range name: (d_lo, d_hi)} moves every lo / hi of
that range: a deliberately wrong model (a "mutant").

REFERENCE (``reference``).  softmax(Q K^T scale) V in fp64 over exactly those ranges with the GQA head mapping, plain torch on the CPU.  A row
that sees no key gives zeros.

INPUTS.  *values*: the integer-hash tensors of the case, and the same with q and k times 4 (peaked softmax weights).  *edge probes*
(``probe_inputs``): key row j of a buffer carries a position code — NDIG one-hot digits of its index (prefix rows first, then own rows, so a
code is unique over everything a row of the case can see) at amplitude 12, exact in f16 and bf16 —, query row i carries the code of ONE target
key: a full match outscores every other key by at least 144 scale > 12 (head sizes 72 .. 128), so the row's output is its target's V row when
the target is visible and a flat average when it is not.  Four targets per range: its first visible key, the key before it, its last visible
key, the key after it; the keys before and after are real rows (the previous / next sequence or slot, the rows between prefix_len and
max_prefix).  A probe applies to a row iff its target key exists in the buffer (and, for first / last, the range is not empty).  Flipping the
visibility of the target (``MUTANT``) moves such a row by far more than any tolerance used here — asserted by ``sharpness``, on the CPU, for
every row."""
import functools
from types import SimpleNamespace

import torch

from tests import attn_entries_case as C
from tests.decode_hl_ref import pair_rows_checks

AMP = 12.0
TARGETS = ("first", "before", "last", "after")
MUTANT = {"first": (1, 0), "before": (-1, 0), "last": (0, -1), "after": (0, 1)}          # the (d_lo, d_hi) that flips the target key
FAMILIES = ("values", "values_x4")


def eps(dtype):
    return 2.0 ** -10 if dtype == "f16" else 2.0 ** -7          # one rounding of the 16-bit type (tests/test_gpu_kernels.py)


# ---- the visibility model ----------------------------------------------------------------------------------------------------------------------
def _causal_rows(q_lens, k_lens, k_begin, causal, window):
    """Rows of packed sequences: (lo, hi, lo kind, hi kind) of the own range per query row."""
    rows = []
    for Lq, Lk, k0 in zip(q_lens, k_lens, k_begin):
        shift = Lk - Lq
        for i in range(Lq):
            hi = min(Lk, i + shift + 1) if causal else Lk
            lo = max(0, i + shift - window + 1) if window else 0
            rows.append((k0 + lo, k0 + max(hi, lo), "window" if lo > 0 else "start", "causal" if hi < Lk else "end"))
    return rows


def model(fn, kw, d=None):
    """-> rows: per query row a list of ranges (name, lo, hi, lo kind, hi kind) clipped to their buffers; sizes: {name: rows of the buffer};
    H, KV, D.  ``d``: {name: (d_lo, d_hi)} added to every edge of that range before clipping."""
    d = d or {}
    H, KV, D = kw.get("H", 4), kw.get("KV", 1), kw.get("D", 128)
    cum = lambda lens: [sum(lens[:s]) for s in range(len(lens))]
    prefix = None
    if fn is C.varlen:
        k_lens = kw["q_lens"] if kw.get("k_lens") is None else kw["k_lens"]
        assert kw.get("causal", True) or not kw.get("window", 0)
        own, n_own = _causal_rows(kw["q_lens"], k_lens, cum(k_lens), kw.get("causal", True), kw.get("window", 0)), sum(k_lens)
    elif fn is C.decode:
        stride = max(kw["k_lens"]) + 3
        begin = [s * stride for s in range(len(kw["k_lens"]))] if kw.get("pooled") else cum(kw["k_lens"])
        own = _causal_rows(kw["q_lens"], kw["k_lens"], begin, True, kw.get("window", 0))
        n_own = len(kw["k_lens"]) * stride if kw.get("pooled") else sum(kw["k_lens"])
    elif fn is C.shared:
        stride = (max(kw["k_lens"]) if kw.get("max_k") is None else kw["max_k"]) + 3
        own = [(s * stride, s * stride + L, "start", "end") for s, L in enumerate(kw["k_lens"])]
        n_own = len(kw["k_lens"]) * stride
        prefix = (kw["max_prefix"] if kw.get("prefix") is None else kw["prefix"], kw["max_prefix"])
    elif fn is C.prefix_rows:
        own = [(2 * r, 2 * r + L, "start", "end") for r, L in enumerate(kw["k_lens"])]
        n_own = 2 * len(kw["k_lens"]) + max(max(kw["k_lens"]), 1)
        prefix = (kw["prefix"], kw["prefix"])
    elif fn is C.prefix_fwd:
        own, n_own = _causal_rows(kw["q_lens"], kw["q_lens"], cum(kw["q_lens"]), True, 0), sum(kw["q_lens"])
        prefix = (kw["prefix"], kw["prefix"])
    else:
        raise KeyError(fn)
    sizes = {"own": n_own}
    if prefix is not None:
        sizes["prefix"] = prefix[1]

    def clip(name, lo, hi, lk, hk):
        lo, hi = lo + d.get(name, (0, 0))[0], hi + d.get(name, (0, 0))[1]
        lo, hi = max(lo, 0), min(hi, sizes[name])
        return (name, lo, max(hi, lo), lk, hk)

    rows = []
    for lo, hi, lk, hk in own:
        ranges = [clip("prefix", 0, prefix[0], "start", "end")] if prefix is not None else []
        rows.append(ranges + [clip("own", lo, hi, lk, hk)])
    return SimpleNamespace(rows=rows, sizes=sizes, H=H, KV=KV, D=D)


def target_key(rng, target):
    """Index (in the range's buffer) of a probe's target key for the TRUE range ``rng``, None where first / last has no visible key."""
    _, lo, hi, _, _ = rng
    if target in ("first", "last") and hi <= lo:
        return None
    return {"first": lo, "before": lo - 1, "last": hi - 1, "after": hi}[target]


def probe_rows(m, name, target):
    """{query row: target key} of the rows the probe (range name, target) applies to: the target key exists in the buffer."""
    out = {}
    for r, ranges in enumerate(m.rows):
        for rng in ranges:
            t = target_key(rng, target) if rng[0] == name else None
            if t is not None and 0 <= t < m.sizes[name]:
                out[r] = t
    return out


def probes(m):
    """Every (range name, target) of the case with at least one applicable row."""
    return [(name, t) for name in ("prefix", "own") if name in m.sizes for t in TARGETS if probe_rows(m, name, t)]


def edge_kinds(m, name, target):
    """{edge kind: number of applicable rows} of a probe (the lo kind for first / before, the hi kind for last / after)."""
    rows, kinds = probe_rows(m, name, target), {}
    for r in rows:
        rng = next(g for g in m.rows[r] if g[0] == name)
        kind = rng[3] if target in ("first", "before") else rng[4]
        kinds[kind] = kinds.get(kind, 0) + 1
    return kinds


def expected_edges(fn, kw):
    """(range, edge kind, target) triples the case must have applicable rows for, from its arguments alone."""
    windowed = bool(kw.get("window", 0))          # every row of a windowed case may begin inside its sequence: no start edge is owed
    want = [("own", "end", "last")] + ([] if windowed else [("own", "start", "first")])
    many = len([L for L in kw.get("k_lens") or kw["q_lens"] if L > 0]) > 1 if fn is not C.prefix_rows else len(kw["k_lens"]) > 1
    if fn in (C.varlen, C.decode, C.prefix_fwd):
        if kw.get("causal", True) and max(kw["q_lens"]) > 1:
            want += [("own", "causal", "last"), ("own", "causal", "after")]
        if kw.get("window", 0) and kw["window"] < max(kw.get("k_lens") or kw["q_lens"]):
            want += [("own", "window", "first"), ("own", "window", "before")]
    if many:
        want += [("own", "end", "after")] + ([] if windowed else [("own", "start", "before")])
    if fn in (C.shared, C.prefix_rows, C.prefix_fwd):
        want += [("prefix", "start", "first"), ("prefix", "end", "last")]
        if fn is C.shared and kw.get("prefix") is not None and kw["prefix"] < kw["max_prefix"]:
            want.append(("prefix", "end", "after"))
    return want


# ---- the reference -----------------------------------------------------------------------------------------------------------------------------
def reference(m, inp, rows=None):
    """fp64 [n query rows, H D] of the model ``m`` over the CPU copies of the input tensors (``rows``: these query rows only, others zero)."""
    H, KV, D = m.H, m.KV, m.D
    q = inp["q"].cpu().double().view(-1, H, D)
    buf = {"own": (inp["k"].cpu().double().view(-1, KV, D), inp["v"].cpu().double().view(-1, KV, D))}
    if "prefix" in m.sizes:
        buf["prefix"] = (inp["kp"].cpu().double().view(-1, KV, D), inp["vp"].cpu().double().view(-1, KV, D))
    head_kv = torch.arange(H) // (H // KV)
    out = torch.zeros(q.shape[0], H * D, dtype=torch.float64)
    for r in (range(q.shape[0]) if rows is None else rows):
        ks = torch.cat([buf[name][0][lo:hi] for name, lo, hi, _, _ in m.rows[r]])
        vs = torch.cat([buf[name][1][lo:hi] for name, lo, hi, _, _ in m.rows[r]])
        if ks.shape[0] == 0:
            continue
        s = torch.einsum("hd,nhd->hn", q[r], ks[:, head_kv]) * D ** -0.5
        out[r] = torch.einsum("hn,nhd->hd", torch.softmax(s, -1), vs[:, head_kv]).reshape(-1)
    return out


# ---- the inputs --------------------------------------------------------------------------------------------------------------------------------
def _codes(idx, D, ndig):
    """[len(idx), D]: ``ndig`` one-hot digits (base D // ndig) of every index, amplitude AMP."""
    base = D // ndig
    idx = torch.as_tensor(idx, dtype=torch.int64)
    out = torch.zeros(len(idx), D)
    for k in range(ndig):
        out[torch.arange(len(idx)), k * base + (idx // base ** k) % base] = AMP
    return out


def code_digits(m):
    total = sum(m.sizes.values())
    ndig = 2 if total <= (m.D // 2) ** 2 else 3
    assert total <= (m.D // ndig) ** ndig
    return ndig


def values_inputs(fn, kw, dtype, dev, family):
    inp = C.make_inputs(fn, kw, dtype, dev)
    if family == "values_x4":
        inp = dict(inp, q=inp["q"] * 4, k=inp["k"] * 4, **({"kp": inp["kp"] * 4} if "kp" in inp else {}))
    return inp


def probe_inputs(fn, kw, dtype, dev, m, name, target):
    """The case's V rows, position codes as K rows and, per applicable query row, the code of the probe's target key in every head (other
    rows: zero, a flat softmax).  Returns (inputs, {row: target key})."""
    inp = C.make_inputs(fn, kw, dtype, dev)
    ndig, n_pre = code_digits(m), m.sizes.get("prefix", 0)
    rows = probe_rows(m, name, target)
    q = torch.zeros(inp["q"].shape[0], m.H, m.D)
    if rows:
        q[list(rows)] = _codes([t + (n_pre if name == "own" else 0) for t in rows.values()], m.D, ndig)[:, None, :]
    new = {"q": q.view(-1, m.H * m.D), "k": _codes(range(n_pre, n_pre + m.sizes["own"]), m.D, ndig).repeat(1, m.KV)}
    if n_pre:
        new["kp"] = _codes(range(n_pre), m.D, ndig).repeat(1, m.KV)
    for key, t in new.items():
        assert t.shape == inp[key].shape, (key, t.shape, inp[key].shape)
        inp[key] = t.to(inp[key].dtype).to(dev)
    return inp, rows


# ---- output forms ------------------------------------------------------------------------------------------------------------------------------
def form(fn, kw):
    if fn is C.varlen and kw.get("kind", "out") != "out":
        return kw["kind"]
    if kw.get("lo4"):
        return "lo4"
    return "hl" if kw.get("hl") else "f32" if kw.get("f32") else "out"


def decode_fp8(b):
    """e4m3 (fn) bytes -> fp64."""
    return b.cpu().view(torch.float8_e4m3fn).double()


def tolerance(fm, dtype, ref):
    """Elementwise bound of the checked rows of output form ``fm`` (module docstring of the tests): 3 eps(T); for the fp8 form (scale 16)
    plus half an e4m3 step of the value, normal or subnormal."""
    tol = torch.full_like(ref, 3 * eps(dtype))
    if fm == "fp8":
        tol = tol + torch.maximum(2.0 ** -4 * ref.abs(), torch.full_like(ref, 2.0 ** -10 / 16))
    return tol


def checked_rows(fm, outs, tq):
    """The rows a tolerance applies to, as fp64 [tq, H D]."""
    if fm == "fp8":
        return decode_fp8(outs["out_fp8"]) / 16.0
    if fm == "f32" and "out" not in outs:
        return outs["out_f32"].cpu().double()
    return outs["out"][:tq].cpu().double()


def decode_img(img, sc, K):
    """fp4 image [M, K4 / 2] bytes + E8M0 block scales -> fp32 [M, K] (tests/test_gpu_lowbit.py)."""
    grid = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
    M, half = img.shape
    b = img.to(torch.int64)
    codes = torch.stack([b & 15, b >> 4], dim=-1).reshape(M, half * 2)
    val = grid[codes & 7] * torch.where((codes & 8) != 0, -1.0, 1.0)
    s = torch.exp2(sc.to(torch.float32) - 127.0)[:, :half * 2 // 32].repeat_interleave(32, dim=1)
    return (val * s)[:, :K]


def _same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k].cpu(), b[k].cpu()) for k in a)


def _go(ops, spec, dtype, dev, inp, **more):
    """One guarded launch: (outputs, the allocation with its guard rows)."""
    mem = C.Guarded(dev)
    outs = C.launch(ops, *spec, dtype, dev, inp=inp, mem=mem, **more)[1]
    return outs, mem


LO4_TIE_CAP = 2e-3          # tests/test_gpu_lowbit.py: elements whose tie a fused multiply-subtract moved


def check_lo4(ops, spec, dtype, dev, inp, outs, ref, what):
    """The lo4 form as tests/test_gpu_lowbit.py defines it.  Returns the fraction of image elements that differ from the host rule (None where
    the entry has no fp32 form to take the residual from: the two-range prefill)."""
    from oracle import leopard_oracle as O
    fn, kw, _ = spec
    m = model(fn, kw)
    H, D = m.H, m.D
    nb = (D + 31) // 32 * 32
    tq = ref.shape[0]
    plain, mem = _go(ops, spec, dtype, dev, inp, **({"lo4": False} if fn is C.prefix_fwd else {"kind": "out"}), sel=None)
    assert mem.intact() and torch.equal(plain["out"].cpu(), outs["out"].cpu()), f"{what}: hi rows != the plain launch"
    hi, img, sc = outs["out"].cpu(), outs["img"].cpu(), outs["scales"].cpu()
    sel = torch.tensor([kw["sel"](r) for r in range(tq)]) if kw.get("sel") is not None else torch.ones(tq, dtype=torch.bool)
    assert not img[:, H * nb // 2:].any() and not sc[:, H * nb // 32:].any(), f"{what}: padding bytes written"
    assert not img[~sel].any() and not sc[~sel].any(), f"{what}: an unselected row's image or scales lost their initial (zero) bytes"
    got = decode_img(img, sc, H * nb).view(tq, H, nb)
    assert not got[:, :, D:].any(), f"{what}: codes in a head's padding"
    both = hi.double() + got[:, :, :D].reshape(tq, H * D).double()
    e_hi, e_both = (hi.double() - ref)[sel].abs().max().item(), (both - ref)[sel].abs().max().item()
    assert e_both <= e_hi, f"{what}: hi + image error {e_both:.3e} above hi alone {e_hi:.3e}"
    if fn is not C.varlen:
        return None
    o32 = _go(ops, spec, dtype, dev, inp, kind="f32", sel=None)[0]["out_f32"].cpu()
    lo = torch.zeros(tq, H, nb)
    lo[:, :, :D] = (o32 - hi.float()).view(tq, H, D)
    want = O._lo_round(lo.view(tq, H * nb)[sel], "e2m1", 32)
    moved = (got.view(tq, H * nb)[sel] != want).float().mean().item()
    assert moved <= LO4_TIE_CAP, f"{what}: {moved:.2e} of the image elements differ from the host rule"
    return moved


def check_form(ops, spec, dtype, dev, inp, outs, mem, ref, what):
    """Everything a launch of output form ``form(spec)`` owes beyond its values: guard rows, the bit-equalities with the plain launch."""
    fn, kw, _ = spec
    fm, tq = form(fn, kw), ref.shape[0]
    assert mem.intact(), f"{what}: a guard row was written"
    extra = {}
    if fm == "hl":
        plain, pmem = _go(ops, spec, dtype, dev, inp, hl=False)
        assert pmem.intact()
        two = mem.full[0].cpu()
        pair_rows_checks(two, plain["out"].cpu(), tq, C.DTYPES[dtype], what)
        hi, lo = two[:tq].double(), two[tq:2 * tq].double()
        e_two, e_one = (hi + lo - ref).abs().max().item(), (hi - ref).abs().max().item()
        assert e_two <= e_one, f"{what}: |hi + lo - ref| {e_two:.3e} above |hi - ref| {e_one:.3e}"
    if fm == "f32" and "out" in outs:                 # one launch writes both forms: the T rows are the plain launch's
        plain, pmem = _go(ops, spec, dtype, dev, inp, f32=False)
        assert pmem.intact() and torch.equal(plain["out"].cpu(), outs["out"].cpu()), f"{what}: T rows != the launch without out_f32"
        err32 = (outs["out_f32"].cpu().double() - ref).abs().max().item()
        assert err32 <= 3 * eps(dtype), f"{what}: out_f32 {err32 / eps(dtype):.2f} eps"
        extra["f32_eps"] = err32 / eps(dtype)
    if fm == "lo4":
        extra["lo4_moved"] = check_lo4(ops, spec, dtype, dev, inp, outs, ref, what)
    return extra


# ---- the checks --------------------------------------------------------------------------------------------------------------------------------
def check_values(ops, spec, dtype, dev, family):
    """One case on one value family.  Returns {"err_eps": max error of the checked rows in eps(T), ...} after asserting everything."""
    fn, kw, _ = spec
    fm, m = form(fn, kw), model(fn, kw)
    what = f"{fn.__name__} {kw} {dtype} {family}"
    inp = values_inputs(fn, kw, dtype, dev, family)
    ref = reference(m, inp)
    outs, mem = _go(ops, spec, dtype, dev, inp)
    again = _go(ops, spec, dtype, dev, inp)[0]
    assert _same(outs, again), f"{what}: two launches differ"
    got = checked_rows(fm, outs, ref.shape[0])
    assert torch.isfinite(got).all(), f"{what}: a non-finite output"
    over = ((got - ref).abs() - tolerance(fm, dtype, ref)).max().item() if got.numel() else 0.0
    err = (got - ref).abs().max().item() / eps(dtype) if got.numel() else 0.0
    print(f"{what}: max error {err:.3f} eps")
    assert over <= 0, f"{what}: over the bound by {over:.3e} (max error {err:.2f} eps)"
    rec = {"err_eps": err}
    rec.update(check_form(ops, spec, dtype, dev, inp, outs, mem, ref, what))
    return rec


def check_probes(ops, spec, dtype, dev):
    """Every probe of the case, every applicable row.  Returns {(range, target): (rows, max error in eps(T))}."""
    fn, kw, _ = spec
    fm, m = form(fn, kw), model(fn, kw)
    rec = {}
    for name, target in probes(m):
        what = f"{fn.__name__} {kw} {dtype} probe {name}/{target}"
        inp, rows = probe_inputs(fn, kw, dtype, dev, m, name, target)
        idx = sorted(rows)
        ref = reference(m, inp, rows=idx)[idx]
        outs, mem = _go(ops, spec, dtype, dev, inp)
        assert mem.intact(), f"{what}: a guard row was written"
        got_all = checked_rows(fm, outs, len(m.rows))
        assert torch.isfinite(got_all).all(), f"{what}: a non-finite output"
        got = got_all[idx]
        over = ((got - ref).abs() - tolerance(fm, dtype, ref)).amax(dim=1)
        err = (got - ref).abs().amax(dim=1) / eps(dtype)
        bad = [(idx[n], round(err[n].item(), 2)) for n in range(len(idx)) if over[n] > 0]
        print(f"{what}: {len(idx)} rows, max error {err.max().item():.3f} eps")
        assert not bad, f"{what}: rows over the bound (row, eps): {bad[:8]} of {len(bad)}"
        rec[(name, target)] = (len(idx), err.max().item())
    return rec


def sharpness(spec, dtype):
    """CPU only, no kernel.  For every probe of the case: the mutant reference (the model with the target key's visibility flipped) against the
    true one, at EVERY applicable row, in units of that row's tolerance — the smallest over the rows of max_elements |mutant - ref| / tol.
    Returns {(range, target): (rows, that minimum, the same minimum in eps(T))}."""
    fn, kw, _ = spec
    fm, m = form(fn, kw), model(fn, kw)
    out = {}
    for name, target in probes(m):
        inp, rows = probe_inputs(fn, kw, dtype, "cpu", m, name, target)
        idx = sorted(rows)
        ref = reference(m, inp, rows=idx)[idx]
        mut = reference(model(fn, kw, d={name: MUTANT[target]}), inp, rows=idx)[idx]
        ratio = ((mut - ref).abs() / tolerance(fm, dtype, ref)).amax(dim=1)
        out[(name, target)] = (len(idx), ratio.min().item(), ((mut - ref).abs().amax(dim=1) / eps(dtype)).min().item())
    return out


def check_edges_present(spec):
    """At least one row applies to each probe kind the case has an edge for."""
    fn, kw, _ = spec
    m = model(fn, kw)
    for name, kind, target in expected_edges(fn, kw):
        assert edge_kinds(m, name, target).get(kind, 0) > 0, f"{fn.__name__} {kw}: no row for the {target} key of a {name} {kind} edge"


@functools.lru_cache(maxsize=None)
def all_cases():
    return {**C.CASES, **C.EXTRA}


def stream_twins():
    """Cases launched with attn.stream_kv = 0: the streaming loads differ in cache policy only, so the bits must be those of the default."""
    return sorted(name for name, (_, _, opts) in all_cases().items() if opts.get("attn.stream_kv") == 0)


def check_same_bits(ops, dtype, dev, spec_a, spec_b):
    """Two specs of the same inputs must give the same bytes in every output."""
    inp = C.make_inputs(spec_a[0], spec_a[1], dtype, dev)
    a, mem_a = _go(ops, spec_a, dtype, dev, inp)
    b, mem_b = _go(ops, spec_b, dtype, dev, inp)
    assert mem_a.intact() and mem_b.intact() and _same(a, b), f"{spec_a[1]} {spec_a[2]} and {spec_b[1]} {spec_b[2]} differ"


def check_window_above_all(ops, dtype, dev):
    """A window longer than every sequence hides nothing: the bits of window 0."""
    fn, kw, opts = all_cases()["x_varlen_window_above_all"]
    check_same_bits(ops, dtype, dev, (fn, kw, opts), (fn, dict(kw, window=0), opts))


def check_window_one(ops, dtype, dev):
    """A window of 1: every row sees its own key alone and returns its own V row, exactly."""
    fn, kw, opts = all_cases()["x_varlen_window1"]
    inp = C.make_inputs(fn, kw, dtype, dev)
    outs, mem = _go(ops, (fn, kw, opts), dtype, dev, inp)
    assert mem.intact()
    v = inp["v"].cpu().view(-1, kw.get("KV", 1), 1, 128).expand(-1, -1, kw.get("H", 4) // kw.get("KV", 1), -1).reshape(outs["out"].shape)
    assert torch.equal(outs["out"].cpu(), v), "window 1: a row is not its own V row"


def record(ops, dev, out):
    """The table of profiles/attn_entries_values.txt for one platform: per case and dtype the maximum error of each value family and of the
    probes (in eps of the 16-bit type), the probe rows, and per probe the smallest mutant distance over its rows (CPU, no kernel)."""
    for name, spec in all_cases().items():
        for dtype in C.DTYPES:
            try:
                vals = {fam: check_values(ops, spec, dtype, dev, fam) for fam in FAMILIES}
                moved = vals["values"].get("lo4_moved")
                line = " ".join(f"{fam} {vals[fam]['err_eps']:.3f}" for fam in FAMILIES) + ("" if moved is None else f" lo4 ties moved {moved:.2e}")
            except AssertionError as e:
                line = "values FAILED: " + str(e).splitlines()[0][:200]
            sh = sharpness(spec, dtype)
            try:
                pr = check_probes(ops, spec, dtype, dev)
                line += f" probes {max(e for _, e in pr.values()):.3f} eps over {sum(n for n, _ in pr.values())} rows"
            except AssertionError as e:
                pr = {}
                line += " probes FAILED: " + str(e).splitlines()[0][:200]
            out.write(f"{name}/{dtype}: {line}\n")
            for key in sh:
                got = f"max {pr[key][1]:.3f} eps" if key in pr else "not run past the failure"
                out.write(f"    {key[0]}/{key[1]}: {sh[key][0]} rows, {got}; mutant at least {sh[key][2]:.1f} eps = {sh[key][1]:.1f} x tolerance\n")
            out.flush()


if __name__ == "__main__":          # python -m tests.attn_entries_ref [cuda] > table: the library LEOPARD_AMD_LIB names (cpu: an emulator build)
    import contextlib
    import sys

    from leopard_amd import _lib
    from leopard_amd.ops import Ops
    device = sys.argv[1] if len(sys.argv) > 1 else "cpu"
    with contextlib.redirect_stdout(sys.stderr):
        record(Ops(lib=_lib.bind(_lib.LIB_PATH), emulated=device == "cpu"), device, sys.__stdout__)
