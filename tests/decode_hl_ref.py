"""Inputs, fp64 references and the checks built on them for the hi + lo pair ("hl") decode kernels (csrc/skinny.h "hl", the lo_rows store of
attn_combine_kernel).  Shared by tests/test_gpu_decode_hl.py (the device) and tests/test_emu_decode_hl.py (the CPU emulator, which compiles
the same headers): every check takes the Ops object and the device its tensors live on.  No fixtures, no pytest hooks.

EXACT INPUTS.  hi rows are integers in [-2, 2], lo rows integers in [-3, 3] x 2^-7, weights are in {-1, 0, 1} x w_scale (w_scale a power of
two) and the residual base holds multiples of 2^-7 with |base| <= 64.  Every product is then a multiple of q = 2^-7 w_scale, and so is every
partial sum, whatever the order it is formed in; its magnitude is at most
    bound = max_n sum_k |w[n, k]| (|hi[m, k]| + |lo[m, k]|)  +  max |base|   <=   K (2 + 3 x 2^-7) w_scale + 64
which at K = 14336, w_scale = 1 is 29 072 < 2^17 = 2^24 q: every partial and final sum is an integer multiple of q below 2^24 q — exactly
representable in fp32.  The device result of a projection over these inputs therefore has ONE correct value, bit for bit, in any summation
order; ``exact_inputs`` asserts the bound on what it generated."""
import contextlib
import functools
from types import SimpleNamespace

import torch

from leopard_amd.weights import interleave_gate_up, rope_permute_rows, skinny_pack

GUARD = 7.0
DTYPES = [torch.float16, torch.bfloat16]
EPS_T = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}        # half an ulp of the 16-bit type, relative
# (name, skinny.coalesce, packed): the three weight layouts of skinny_gemm_kernel (LAYOUT 0, 2, 1)
LAYOUTS = (("row-major", 0, False), ("coalesced", 1, False), ("packed", None, True))


@contextlib.contextmanager
def option(ops, key, value):
    """Set a library option for the block; the value it had before comes back whatever happens inside."""
    before = ops.get_option(key)
    try:
        if value is not None:
            ops.set_option(key, value)
        yield
    finally:
        ops.set_option(key, before)


def sync(dev):
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()


def pair(x32, dtype):
    """[T(x); T(x - T(x))] of fp32 rows."""
    hi = x32.to(dtype)
    lo = (x32 - hi.float()).to(dtype)
    return torch.cat([hi, lo], 0).contiguous()


def strided_rows(x, dev, pad=8):
    """x on ``dev`` as a view whose row stride is its width + pad (the pad columns hold the guard value)."""
    buf = torch.full((x.shape[0], x.shape[1] + pad), GUARD, dtype=x.dtype)
    buf[:, :x.shape[1]] = x
    return buf.to(dev)[:, :x.shape[1]]


def guarded(rows, cols, dtype, dev, top=None):
    """[rows + 1, cols] filled with the guard value (``top``: the content of the first rows)."""
    t = torch.full((rows + 1, cols), GUARD, dtype=dtype)
    if top is not None:
        t[:top.shape[0]] = top
    return t.to(dev)


def intact(t, rows):
    return bool((t[rows:] == GUARD).all())


def exact_inputs(M, N, K, dtype, seed, w_scale=1.0):
    """The exact integer inputs (module docstring), CPU.  x: the pair [2 M, K] in ``dtype``; w [N, K] in ``dtype``; base fp32 [M, N];
    v fp64 [M, N] = (hi + lo) @ w^T, which is exact in fp32 too — asserted."""
    g = torch.Generator().manual_seed(seed)
    hi = torch.randint(-2, 3, (M, K), generator=g).double()
    lo = torch.randint(-3, 4, (M, K), generator=g).double() * 2.0 ** -7
    w = torch.randint(-1, 2, (N, K), generator=g).double() * w_scale
    base = torch.randint(-64 * 128, 64 * 128 + 1, (M, N), generator=g).double() * 2.0 ** -7
    return exact_from(hi, lo, w, base, dtype, w_scale)


def exact_from(hi, lo, w, base, dtype, w_scale):
    q = 2.0 ** -7 * w_scale
    assert hi.abs().max() <= 2 and torch.equal(hi, hi.round())
    assert (lo * 128).abs().max() <= 3 and torch.equal(lo * 128, (lo * 128).round())
    assert torch.equal(w / w_scale, (w / w_scale).round()) and (w / w_scale).abs().max() <= 1
    assert base.abs().max() <= 64 and torch.equal(base * 128, (base * 128).round())
    bound = ((hi.abs() + lo.abs()) @ w.abs().T).max().item() + base.abs().max().item()
    assert bound < 2.0 ** 24 * q, (bound, q)                             # every partial sum: a multiple of q below 2^24 q
    x = torch.cat([hi, lo], 0)
    x16, w16 = x.to(dtype), w.to(dtype)
    assert torch.equal(x16.double(), x) and torch.equal(w16.double(), w)    # the 16-bit operands hold them exactly
    v = (hi + lo) @ w.T
    assert torch.equal(v.float().double(), v) and torch.equal((v + base).float().double(), v + base)
    return SimpleNamespace(x=x16, w=w16, base=base.float(), v=v, M=hi.shape[0], N=w.shape[0], K=w.shape[1])


def layout_weight(w_dev, packed):
    return skinny_pack(w_dev) if packed else w_dev


# ---- 1. gemm_skinny(hl=True), exact ------------------------------------------------------------------------------------------------------------
def check_gemm_hl_exact(ops, dev, dtype, M, K, N=256, seed=1):
    """STORE_F32, RESIDUAL and STORE of lmi_gemm_skinny_hl on the exact inputs: equal to the fp64 reference bit for bit, in the three weight
    layouts and in two launches; X has a row stride > K, every output a guard below its rows."""
    inp = exact_inputs(M, N, K, dtype, seed + 1000 * M + K)
    X, w_dev = strided_rows(inp.x, dev), inp.w.to(dev)
    assert X.stride(0) > K
    v32 = inp.v.float()
    want = {"store_f32": v32, "residual": (inp.v + inp.base.double()).float(), "store": pair(v32, dtype)}
    seen = {}
    for name, co, packed in LAYOUTS:
        with option(ops, "skinny.coalesce", co):
            w = layout_weight(w_dev, packed)
            runs = []
            for _ in range(2):
                o32 = guarded(2 * M, N, torch.float32, dev)               # fp32 outputs have M rows: M guard rows + 1 below them
                acc = guarded(2 * M, N, torch.float32, dev, top=inp.base)
                o16 = guarded(2 * M, N, dtype, dev)
                ops.gemm_skinny(w, X, o32[:M], 3, packed=packed, hl=True)
                ops.gemm_skinny(w, X, acc[:M], 1, packed=packed, hl=True)
                ops.gemm_skinny(w, X, o16[:2 * M], 0, packed=packed, hl=True)
                runs.append({"store_f32": o32, "residual": acc, "store": o16})
            sync(dev)
        for key, rows in (("store_f32", M), ("residual", M), ("store", 2 * M)):
            a, b = runs[0][key].cpu(), runs[1][key].cpu()
            assert torch.equal(a, b), f"{name} {key}: two launches differ"
            assert intact(a, rows), f"{name} {key}: guard rows written"
            assert torch.equal(a[:rows], want[key]), f"{name} {key}: max diff {(a[:rows].double() - want[key].double()).abs().max().item():.3e}"
        seen[name] = runs[0]
    for name in ("coalesced", "packed"):
        for key in want:
            assert torch.equal(seen[name][key], seen["row-major"][key]), f"{name} != row-major: {key}"


def swiglu_ref(v):
    """fp64 SwiGLU of exact linear outputs v [M, N] whose columns are interleaved [32 gate | 32 up]: [M, N / 2], product column
    (N // 64 group) * 32 + j."""
    M, N = v.shape
    lv = v.view(M, N // 64, 2, 32)
    return (torch.nn.functional.silu(lv[:, :, 0]) * lv[:, :, 1]).reshape(M, N // 2)


def swiglu_tol(want, dtype):
    """The bound tests/test_emu_decode_hl.py uses for this epilogue: what a hi + lo pair leaves of one value (eps^2 relative, eps one ulp of
    the 16-bit type) plus the fp32 arithmetic of silu."""
    eps = 2.0 ** -10 if dtype == torch.float16 else 2.0 ** -7
    scale = max(1.0, want.abs().max().item())
    return 4 * eps * eps * scale + 2e-6 * scale


def run_swiglu_hl(ops, dev, dtype, inp, want, what):
    """The SwiGLU epilogue over the three layouts: out[:M] + out[M:] against ``want`` within swiglu_tol; layouts and launches agree bit for bit."""
    M, F = inp.M, inp.N // 2
    X, w_dev = strided_rows(inp.x, dev), inp.w.to(dev)
    tol, first = swiglu_tol(want, dtype), None
    for name, co, packed in LAYOUTS:
        with option(ops, "skinny.coalesce", co):
            w = layout_weight(w_dev, packed)
            outs = [guarded(2 * M, F, dtype, dev) for _ in range(2)]
            for o in outs:
                ops.gemm_skinny(w, X, o[:2 * M], 2, packed=packed, hl=True)
            sync(dev)
        a, b = outs[0].cpu(), outs[1].cpu()
        assert torch.equal(a, b) and intact(a, 2 * M), f"{what} {name}: launches differ or the guard row was written"
        got = a[:M].double() + a[M:2 * M].double()
        err = (got - want).abs().max().item()
        assert err <= tol, f"{what} {name}: |hi + lo - ref| {err:.3e} > {tol:.3e}"
        lo_cap = EPS_T[dtype] * a[:M].double().abs() + 1e-7                # the lo row is a rounding residual of ITS hi element
        assert (a[M:2 * M].double().abs() <= lo_cap).all(), f"{what} {name}: a lo element is no residual of its hi element"
        first = a if first is None else first
        assert torch.equal(a, first), f"{what} {name} != row-major"


def check_swiglu_hl(ops, dev, dtype, M, K, N=256, seed=2):
    """SwiGLU on the exact inputs (W x 2^-4: O(1) gate values): the linear outputs v are exact, so hi + lo is compared with the fp64 SwiGLU of v."""
    raw = exact_inputs(M, N, K, dtype, seed + 1000 * M + K, w_scale=2.0 ** -4)
    F = N // 2
    gu = interleave_gate_up(raw.w[:F].contiguous(), raw.w[F:].contiguous())
    inp = SimpleNamespace(x=raw.x, w=gu, M=M, N=N, K=K)
    v = (raw.x[:M].double() + raw.x[M:].double()) @ gu.double().T
    run_swiglu_hl(ops, dev, dtype, inp, swiglu_ref(v), f"swiglu M={M} K={K}")


def swiglu_mapping_inputs(M, dtype, seed=3):
    """K = 128, N = 256 (F = 128 products per row), built so that every gate / up pair of a row gives a DISTINCT product: gate_j is the same for
    every j of row m ((32 - m) / 16), up_j = (j + 1) / 16 — product j = silu(gate) (j + 1) / 16, steps of ~0.1 — plus the (small) lo rows'
    share.  A product stored in another column, or paired with another unit's up rows, then misses its reference by a whole step."""
    K, F = 128, 128
    g = torch.Generator().manual_seed(seed + M)
    hi = torch.zeros(M, K, dtype=torch.float64)
    for m in range(M):
        hi[m, :16] = 2.0
        hi[m, 16 - m:16] = 1.0                                             # sum of the first 16 = 32 - m
    hi[:, 16:80], hi[:, 80:] = 2.0, 1.0
    lo = torch.randint(-3, 4, (M, K), generator=g).double() * 2.0 ** -7
    gate, up = torch.zeros(F, K, dtype=torch.float64), torch.zeros(F, K, dtype=torch.float64)
    gate[:, :16] = 1.0
    for j in range(F):
        twos = min((j + 1) // 2, 64)
        ones = j + 1 - 2 * twos
        assert 0 <= ones <= 48
        up[j, 16:16 + twos] = 1.0
        up[j, 80:80 + ones] = 1.0                                          # hi . up_j = 2 twos + ones = j + 1
    ws = 2.0 ** -4
    raw = exact_from(hi, lo, torch.cat([gate, up]) * ws, torch.zeros(M, 2 * F, dtype=torch.float64), dtype, ws)
    gu = interleave_gate_up(raw.w[:F].contiguous(), raw.w[F:].contiguous())
    v = (hi + lo) @ gu.double().T
    want = swiglu_ref(v)
    gap = (want.sort(dim=1).values.diff(dim=1)).min().item()
    assert gap > 8 * swiglu_tol(want, dtype), (gap, swiglu_tol(want, dtype))       # distinct far beyond the tolerance
    return SimpleNamespace(x=raw.x, w=gu, M=M, N=2 * F, K=K), want


def check_swiglu_hl_column_mapping(ops, dev, dtype, M):
    inp, want = swiglu_mapping_inputs(M, dtype)
    run_swiglu_hl(ops, dev, dtype, inp, want, f"swiglu column mapping M={M}")


# ---- 2. folded norm: producer and consumer on pairs --------------------------------------------------------------------------------------------
def check_producer_hl(ops, dev, dtype, M, K, N=256, seed=4):
    """RESIDUAL + norm_out + rowsq_out on the exact inputs: residual bit-exact, norm_out = pair(x gamma) bit for bit (gamma = integer x power of
    two: the fp32 product is exact), row-square partials within 1e-5 of their maximum of fp64."""
    inp = exact_inputs(M, N, K, dtype, seed + 1000 * M + K)
    g = torch.Generator().manual_seed(seed)
    gamma = (torch.randint(1, 8, (N,), generator=g).double() * 2.0 ** torch.randint(-3, 2, (N,), generator=g).double())
    x_ref = inp.v + inp.base.double()
    y = x_ref * gamma
    assert torch.equal(y.float().double(), y)                            # x gamma needs no rounding in fp32
    want_h = pair(y.float(), dtype)
    want_sq = (x_ref ** 2).view(M, N // 16, 16).sum(-1)
    X, w_dev, gamma_dev = strided_rows(inp.x, dev), inp.w.to(dev), gamma.float().to(dev)
    first = None
    for name, co, packed in LAYOUTS:
        with option(ops, "skinny.coalesce", co):
            w = layout_weight(w_dev, packed)
            runs = []
            for _ in range(2):
                xs = guarded(2 * M, N, torch.float32, dev, top=inp.base)
                h = guarded(2 * M, N, dtype, dev)
                sq = guarded(M, N // 16, torch.float32, dev)
                ops.gemm_skinny(w, X, xs[:M], 1, packed=packed, norm_out=h[:2 * M], norm_gamma=gamma_dev, rowsq_out=sq[:M], hl=True)
                runs.append((xs, h, sq))
            sync(dev)
        (xs, h, sq), again = [t.cpu() for t in runs[0]], [t.cpu() for t in runs[1]]
        assert all(torch.equal(a, b) for a, b in zip((xs, h, sq), again)), f"producer {name}: two launches differ"
        assert intact(xs, M) and intact(h, 2 * M) and intact(sq, M), f"producer {name}: guard rows written"
        assert torch.equal(xs[:M], x_ref.float()), f"producer {name}: residual"
        assert torch.equal(h[:2 * M], want_h), f"producer {name}: norm_out pair"
        assert (sq[:M].double() - want_sq).abs().max() <= 1e-5 * want_sq.abs().max(), f"producer {name}: rowsq_out"
        first = (xs, h, sq) if first is None else first
        assert all(torch.equal(a, b) for a, b in zip((xs, h, sq), first)), f"producer {name} != row-major"


def rowsq_inputs(M, P, seed):
    """Row-square partials [M, P] (fp32, positive, O(1) mean square) with a guard row, and rstd of them in fp64 (eps as the fp32 the launch gets)."""
    g = torch.Generator().manual_seed(seed)
    sq = (torch.rand(M, P, generator=g) * 30.0 + 1.0).float()
    eps = 1e-5
    rstd = torch.rsqrt(sq.double().sum(-1, keepdim=True) / (16 * P) + float(torch.tensor(eps, dtype=torch.float32)))
    return sq, eps, rstd


def consumer_tol(P):
    """Relative bound of the consumer's row scale on an exact accumulator: the fixed-order fp32 sum of P positive partials (P / 32 per lane, then
    5 butterfly steps: at most P roundings of 2^-24, halved by the square root), the mean / eps / sqrt / reciprocal and one product."""
    return (P / 2 + 4) * 2.0 ** -24


def check_consumer_hl(ops, dev, dtype, M, P, N=256, seed=5):
    """rowsq_in with STORE_F32 on the exact inputs (K = norm_dim = 16 P): v rstd in fp64 within consumer_tol(P) |ref|, element by element."""
    K = 16 * P
    inp = exact_inputs(M, N, K, dtype, seed + 1000 * M + K)
    sq, eps, rstd = rowsq_inputs(M, P, seed + M)
    ref = inp.v * rstd
    X, w_dev = strided_rows(inp.x, dev), inp.w.to(dev)
    sq_dev = guarded(M, P, torch.float32, dev, top=sq)
    first = None
    for name, co, packed in LAYOUTS:
        with option(ops, "skinny.coalesce", co):
            w = layout_weight(w_dev, packed)
            outs = [guarded(2 * M, N, torch.float32, dev) for _ in range(2)]
            for o in outs:
                ops.gemm_skinny(w, X, o[:M], 3, packed=packed, rowsq_in=sq_dev[:M], norm_dim=K, norm_eps=eps, hl=True)
            sync(dev)
        a, b = outs[0].cpu(), outs[1].cpu()
        assert torch.equal(a, b) and intact(a, M), f"consumer {name}: launches differ or guard rows written"
        excess = ((a[:M].double() - ref).abs() - consumer_tol(P) * ref.abs()).max().item()
        assert excess <= 0, f"consumer {name} P={P}: over the bound by {excess:.3e}"
        first = a if first is None else first
        assert torch.equal(a, first), f"consumer {name} != row-major"


# ---- 3. rope_qkv_skinny(hl=True) ---------------------------------------------------------------------------------------------------------------
ROPE_CAP = 64
ROPE_POS = {1: ([0], [ROPE_CAP - 1]), 3: ([0, ROPE_CAP - 1, 17],), 8: ([5, 0, ROPE_CAP - 1, 31, 32, 1, 62, 40],)}


def rope_tables(cap, hd, dev, theta=10000.0):
    f = torch.arange(cap).float().reshape(-1, 1) * (1.0 / (theta ** (torch.arange(0, hd, 2).float() / hd))).reshape(1, -1)
    return f.cos().contiguous().to(dev), f.sin().contiguous().to(dev)


def check_rope_qkv_hl(ops, dev, dtype, M, K, H, KV, folded, seed=6):
    """lmi_rope_qkv_skinny_hl on the exact inputs, packed and row-major (both lane orders), for every position list of ROPE_POS[M].
    Reference in fp64 from the exact v (times rstd in fp64 when ``folded``) and the fp32 cos / sin the kernel reads:
        |got - ref| <= eps_T |ref| + (2^-22 + c) (|v0| + |v1|)
    — the output's rounding, the fp32 product and fma of the rotation, and c = consumer_tol(K / 16) for the folded row scale.  K / V cache rows
    m cap + pos[m] equal the qkv slices bit for bit, every other cache row and the guard row below qkv keep their fill."""
    hd, cap = 128, ROPE_CAP
    N, rot = (H + 2 * KV) * hd, (H + KV) * hd
    inp = exact_inputs(M, N, K, dtype, seed + 1000 * M + K + H)
    w_rope = torch.cat([rope_permute_rows(inp.w[:rot]), inp.w[rot:]]).contiguous().to(dev)
    X = strided_rows(inp.x, dev)
    cos, sin = rope_tables(cap, hd, dev)
    v, c = inp.v, 0.0
    sq_dev, eps = None, 0.0
    if folded:
        sq, eps, rstd = rowsq_inputs(M, K // 16, seed + M)
        v, c = v * rstd, consumer_tol(K // 16)
        sq_dev = guarded(M, K // 16, torch.float32, dev, top=sq)[:M]
    lin = v.view(M, H + 2 * KV, hd)
    for pos_list in ROPE_POS[M]:
        assert len(set(pos_list)) == M and max(pos_list) < cap
        pos = torch.tensor(pos_list, dtype=torch.int32)
        cs, sn = cos.cpu().double()[pos.long()].unsqueeze(1), sin.cpu().double()[pos.long()].unsqueeze(1)
        ref, mag = lin.clone(), lin.abs().clone()
        a, b = lin[:, :H + KV, :64], lin[:, :H + KV, 64:]
        ref[:, :H + KV, :64], ref[:, :H + KV, 64:] = a * cs - b * sn, b * cs + a * sn
        mag[:, :H + KV, :64] = mag[:, :H + KV, 64:] = a.abs() + b.abs()
        ref, mag = ref.reshape(M, N), mag.reshape(M, N)
        tol = EPS_T[dtype] * ref.abs() + (2.0 ** -22 + c) * mag
        rows = torch.arange(M) * cap + pos.long()
        first = None
        for name, co, packed in LAYOUTS:
            with option(ops, "skinny.coalesce", co):
                w = layout_weight(w_rope, packed)
                kp, vp = guarded(M * cap, KV * hd, dtype, dev), guarded(M * cap, KV * hd, dtype, dev)
                got = guarded(M, N, dtype, dev)
                ops.rope_qkv_skinny(w, X, got[:M], H, KV, hd, cos, sin, kp, vp, cap, pos.to(dev), packed=packed, rowsq_in=sq_dev, norm_eps=eps, hl=True)
                sync(dev)
            got, kp, vp = got.cpu(), kp.cpu(), vp.cpu()
            what = f"rope_qkv {name} M={M} K={K} H={H} pos={pos_list} folded={folded}"
            assert intact(got, M), f"{what}: guard row written"
            excess = ((got[:M].double() - ref).abs() - tol).max().item()
            assert excess <= 0, f"{what}: over the bound by {excess:.3e}"
            assert torch.equal(kp[rows], got[:M, H * hd:rot]) and torch.equal(vp[rows], got[:M, rot:]), f"{what}: cache rows"
            other = torch.ones(M * cap + 1, dtype=torch.bool)
            other[rows] = False
            assert bool((kp[other] == GUARD).all()) and bool((vp[other] == GUARD).all()), f"{what}: another cache row was written"
            first = (got, kp, vp) if first is None else first
            assert all(torch.equal(p, q) for p, q in zip((got, kp, vp), first)), f"{what} != row-major"


# ---- 4. Gaussian pairs -------------------------------------------------------------------------------------------------------------------------
def gaussian_pair_errors(ops, dev, dtype, M, K, N=256, seed=7):
    """Real pairs: max error of the hl launch and of the one-row launch against the fp64 product of the UNROUNDED operand, and — the yardstick
    of the fp32 accumulation alone — of the hl launch and of a plain torch fp32 matmul against the fp64 product of the hi + lo operand."""
    g = torch.Generator().manual_seed(seed + K + M)
    x32 = torch.randn(M, K, generator=g) * 2.0
    w = (torch.randn(N, K, generator=g) * 0.1).to(dtype)
    X = pair(x32, dtype)
    exact = x32.double() @ w.double().T
    seen = (X[:M].double() + X[M:].double()) @ w.double().T
    Xd, wd = X.to(dev), skinny_pack(w.to(dev))
    o_pair, o_one = guarded(M, N, torch.float32, dev), guarded(M, N, torch.float32, dev)
    ops.gemm_skinny(wd, Xd, o_pair[:M], 3, packed=True, hl=True)
    ops.gemm_skinny(wd, Xd[:M], o_one[:M], 3, packed=True)
    plain = ((Xd[:M].float() + Xd[M:].float()) @ w.to(dev).float().T).cpu()
    sync(dev)
    o_pair, o_one = o_pair.cpu(), o_one.cpu()
    assert intact(o_pair, M) and intact(o_one, M)
    return SimpleNamespace(pair=(o_pair[:M].double() - exact).abs().max().item(), one=(o_one[:M].double() - exact).abs().max().item(),
                           acc=(o_pair[:M].double() - seen).abs().max().item(), torch32=(plain.double() - seen).abs().max().item())


# ---- 5. decode attention writing pairs ---------------------------------------------------------------------------------------------------------
ATT_LENS = [1, 63, 64, 65, 700, 1023]                                   # tile edges of ATT_BKV = 64; splits past a sequence's end
ATT_CAP, ATT_HD = 1024, 128


@functools.lru_cache(maxsize=None)
def attention_case(H, KV, dtype, window=0, lens=tuple(ATT_LENS), seed=8):
    """q [B, H hd], pooled k / v [B cap, KV hd] (CPU, ``dtype``) and the fp64 output [B, H hd] of the last query of every sequence (``window``:
    it sees its last ``window`` keys only).  Computed once per case and shared: do not write to it."""
    B, hd, cap = len(lens), ATT_HD, ATT_CAP
    g = torch.Generator().manual_seed(seed + H)
    q = torch.randn(B, H * hd, generator=g).to(dtype)
    k, v = torch.randn(B * cap, KV * hd, generator=g).to(dtype), torch.randn(B * cap, KV * hd, generator=g).to(dtype)
    ref = torch.zeros(B, H * hd, dtype=torch.float64)
    for s, L in enumerate(lens):
        first = max(0, L - window) if window else 0
        ks, vs = k[s * cap + first:s * cap + L].double(), v[s * cap + first:s * cap + L].double()
        for h in range(H):
            kv = h // (H // KV)
            p = torch.softmax((q[s, h * hd:(h + 1) * hd].double() @ ks[:, kv * hd:(kv + 1) * hd].T) * hd ** -0.5, -1)
            ref[s, h * hd:(h + 1) * hd] = p @ vs[:, kv * hd:(kv + 1) * hd]
    return SimpleNamespace(q=q, k=k, v=v, ref=ref, lens=list(lens), B=B)


def pair_rows_checks(two, one, rows, dtype, what):
    """What every hl attention launch must satisfy whatever its content: hi rows == the plain launch, guard intact, lo a rounding residual."""
    assert torch.equal(two[:rows], one), f"{what}: hi rows != the plain launch"
    assert intact(two, 2 * rows), f"{what}: guard row written"
    hi, lo = two[:rows].double(), two[rows:2 * rows].double()
    assert (lo.abs() <= EPS_T[dtype] * hi.abs() + 1e-7).all(), f"{what}: a lo element is no residual of its hi element"


def pair_gain(two, rows, ref):
    hi, lo = two[:rows].double(), two[rows:2 * rows].double()
    return (hi + lo - ref).abs().max().item(), (hi - ref).abs().max().item()


def check_attention_pool_hl(ops, dev, dtype, H, KV, split_tiles, window=0, lens=tuple(ATT_LENS)):
    """lmi_attn_decode_pool_hl on ragged sequences of one pooled cache at one attn.decode_split_tiles setting."""
    case = attention_case(H, KV, dtype, window, lens)
    B, hd, cap = case.B, ATT_HD, ATT_CAP
    q, k, v = case.q.to(dev), case.k.to(dev), case.v.to(dev)
    cu_q = torch.arange(B + 1, dtype=torch.int32).to(dev)
    k_begin = (torch.arange(B, dtype=torch.int32) * cap).to(dev)
    k_len = torch.tensor(case.lens, dtype=torch.int32).to(dev)
    ws = torch.full((ops.decode_workspace_elems(B, H, hd, cap),), float("nan"), dtype=torch.float32).to(dev)
    what = f"decode_pool H={H} KV={KV} split_tiles={split_tiles} window={window}"
    with option(ops, "attn.decode_split_tiles", split_tiles):
        one = guarded(B, H * hd, dtype, dev)
        twos = [guarded(2 * B, H * hd, dtype, dev) for _ in range(2)]
        ops.attention_decode_pool(q, k, v, one[:B], cu_q, k_begin, k_len, cap, H, KV, hd, hd ** -0.5, ws, window=window)
        for t in twos:
            ops.attention_decode_pool(q, k, v, t[:2 * B], cu_q, k_begin, k_len, cap, H, KV, hd, hd ** -0.5, ws, window=window, hl=True)
        sync(dev)
    one, two, again = one.cpu(), twos[0].cpu(), twos[1].cpu()
    assert intact(one, B) and torch.equal(two, again), f"{what}: two launches differ"
    pair_rows_checks(two, one[:B], B, dtype, what)
    assert two[B:2 * B].double().abs().max() > 0, f"{what}: the lo rows are all zero"
    e_two, e_one = pair_gain(two, B, case.ref)
    assert e_two < 0.8 * e_one, f"{what}: hi + lo error {e_two:.3e} against hi alone {e_one:.3e}"
    return e_two, e_one


def check_attention_one_hl(ops, dev, dtype, H, KV, split_tiles, window=0, lens=tuple(ATT_LENS)):
    """lmi_attn_decode_fwd_hl, one sequence and one query row, at every length of ``lens``: the checks of the pooled entry per launch.  A
    query that sees ONE key returns that key's value row, a 16-bit row already: its lo row is rightly zero, so "lo is not all zero" is asked of
    every length above 1.  The gain (hi + lo error < 0.8 x hi error) is taken over the maximum of all lengths, as the pooled launch and the
    emulator test take it over their batch: for one long sequence alone it is no property of the kernel — the outputs are small there, and
    what is left in BOTH errors is P handed to the P.V MFMA in 16 bits (measured per length on the emulator: 0.29 .. 0.68, and 0.93 for
    fp16, 4 heads, 8 tiles per split, 700 keys)."""
    case = attention_case(H, KV, dtype, window, lens)
    hd, cap = ATT_HD, ATT_CAP
    cu_q = torch.tensor([0, 1], dtype=torch.int32).to(dev)
    ws = torch.full((ops.decode_workspace_elems(1, H, hd, cap),), float("nan"), dtype=torch.float32).to(dev)
    gains = []
    with option(ops, "attn.decode_split_tiles", split_tiles):
        for s, L in enumerate(case.lens):
            what = f"decode_fwd H={H} KV={KV} split_tiles={split_tiles} window={window} L={L}"
            q = case.q[s:s + 1].to(dev)
            k, v = case.k[s * cap:(s + 1) * cap].to(dev), case.v[s * cap:(s + 1) * cap].to(dev)
            cu_k = torch.tensor([0, L], dtype=torch.int32).to(dev)
            one = guarded(1, H * hd, dtype, dev)
            twos = [guarded(2, H * hd, dtype, dev) for _ in range(2)]
            ops.attention_decode(q, k, v, one[:1], cu_q, cu_k, 1, cap, H, KV, hd, hd ** -0.5, ws, window=window)
            for t in twos:
                ops.attention_decode(q, k, v, t[:2], cu_q, cu_k, 1, cap, H, KV, hd, hd ** -0.5, ws, window=window, hl=True)
            sync(dev)
            one, two, again = one.cpu(), twos[0].cpu(), twos[1].cpu()
            assert intact(one, 1) and torch.equal(two, again), f"{what}: two launches differ"
            pair_rows_checks(two, one[:1], 1, dtype, what)
            e_two, e_one = pair_gain(two, 1, case.ref[s:s + 1])
            gains.append((L, e_two, e_one))
            if L > 1:
                assert two[1].double().abs().max() > 0, f"{what}: the lo row is all zero"
    e_two, e_one = max(g[1] for g in gains), max(g[2] for g in gains)
    assert e_two < 0.8 * e_one, f"decode_fwd H={H} KV={KV} split_tiles={split_tiles} window={window}: hi + lo error {e_two:.3e} against hi alone {e_one:.3e}"
    return gains
