"""Wide batched decode (decode_batch_limit > 16): the cases and the row-group comparison shared by tests/test_emu_wide_decode.py (emulator)
and tests/test_gpu_wide_decode.py (device).

The contract under test is BIT EQUALITY, not a tolerance: row m of a launch over up to 64 rows equals row m of the existing launch over any
group of at most 16 rows that contains it (lmi_gemm_skinny_wide / lmi_rope_qkv_skinny_wide against lmi_gemm_skinny_ex / lmi_rope_qkv_skinny;
the choice, rules, logprobs and pooled-attention entries at 64 rows against themselves at 16).  ``row_groups`` cuts [0, M) into such groups;
every check fills the reference buffers group by group with the existing entry and compares whole buffers, guard rows included."""
import contextlib

import numpy as np
import torch

from leopard_amd.weights import interleave_gate_up, rope_permute_rows, skinny_pack

GUARD = 7.0
ROWS = 64                                                              # rows of every output buffer: rows >= M keep the guard value
DTYPES = [torch.float16, torch.bfloat16]
# (name, skinny.coalesce, packed): the three weight layouts (LAYOUT 0, 2, 1 of csrc/skinny.h)
LAYOUTS = (("row-major", 0, False), ("coalesced", 1, False), ("packed", None, True))
# 17: one live row in the second column block (the zero fill), 32: a full second block, 33: one row over two blocks (the four-block kernel),
# 48: three blocks, 64: the full width
WIDE_M = (17, 32, 33, 48, 64)
# 128: one k-step (seven waves hold zero partials), 1280: ten steps (uneven steps per wave), 1792: fourteen
WIDE_K = (128, 1280, 1792)


@contextlib.contextmanager
def option(ops, key, value):
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


def rnd(shape, dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def row_groups(M, first=16):
    """[0, M) cut into groups of at most 16 rows; ``first`` < 16 shifts every later boundary, so a row meets other neighbours and another
    lane of the 16-row kernel."""
    cuts = [0] + list(range(first, M, 16)) + [M]
    return [(a, b) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]


def guarded(rows, cols, dtype, dev, top=None):
    t = torch.full((rows, cols), GUARD, dtype=dtype)
    if top is not None:
        t[:top.shape[0]] = top
    return t.to(dev)


# ---- lmi_gemm_skinny_wide ---------------------------------------------------------------------------------------------------------------
def check_gemm_wide(ops, dev, dtype, layout, M, K, seed=0):
    """Every epilogue, the producer pair and the consumer (1 and 40 partials) of lmi_gemm_skinny_wide in one weight layout: whole output buffers
    equal those the 16-row entry fills group by group; rows >= M keep the guard; a second launch gives the same bits."""
    name, co, packed = layout
    lay = (lambda w: skinny_pack(w)) if packed else (lambda w: w)
    x = rnd((M, K), dtype, seed + 1).to(dev)
    with option(ops, "skinny.coalesce", co):
        def compare(make_out, call_wide, call_ref, firsts=(16,)):
            """make_out() -> tuple of fresh guarded buffers; call_*(outs, r0, r1) runs rows [r0, r1) into them."""
            wide = make_out()
            call_wide(wide, 0, M)
            again = make_out()
            call_wide(again, 0, M)
            sync(dev)
            for a, b in zip(wide, again):
                assert torch.equal(a, b), (name, M, K, "two launches differ")
            for first in firsts:
                ref = make_out()
                for r0, r1 in row_groups(M, first):
                    call_ref(ref, r0, r1)
                sync(dev)
                for t, (a, b) in enumerate(zip(wide, ref)):
                    assert torch.equal(a, b), (name, M, K, first, t, "row of the wide launch != row of its 16-row group")
                    assert bool((a[M:] == GUARD).all()), (name, M, K, t, "rows >= M were written")

        # N = 16 (one block: at M > 32 the workgroup's second block is dead), and 48 at the uneven K (one full workgroup + a half-dead one)
        for N in (16, 48) if K == 1280 else (16,):
            w = lay(rnd((N, K), dtype, seed + 2, 0.1).to(dev))
            base = rnd((M, N), torch.float32, seed + 3).to(dev)
            # STORE / STORE_F32 (also against a shifted grouping) / RESIDUAL
            compare(lambda: (guarded(ROWS, N, dtype, dev),),
                    lambda o, r0, r1: ops.gemm_skinny_wide(w, x[r0:r1], o[0][r0:r1], 0, packed),
                    lambda o, r0, r1: ops.gemm_skinny(w, x[r0:r1], o[0][r0:r1], 0, packed))
            compare(lambda: (guarded(ROWS, N, torch.float32, dev),),
                    lambda o, r0, r1: ops.gemm_skinny_wide(w, x[r0:r1], o[0][r0:r1], 3, packed),
                    lambda o, r0, r1: ops.gemm_skinny(w, x[r0:r1], o[0][r0:r1], 3, packed), firsts=(16, 7))
            compare(lambda: (guarded(ROWS, N, torch.float32, dev, top=base),),
                    lambda o, r0, r1: ops.gemm_skinny_wide(w, x[r0:r1], o[0][r0:r1], 1, packed),
                    lambda o, r0, r1: ops.gemm_skinny(w, x[r0:r1], o[0][r0:r1], 1, packed))
            # producer: residual + norm_out + rowsq_out
            gamma = (rnd((N,), torch.float32, seed + 4) + 1.0).to(dev)
            compare(lambda: (guarded(ROWS, N, torch.float32, dev, top=base), guarded(ROWS, N, dtype, dev), guarded(ROWS, N // 16, torch.float32, dev)),
                    lambda o, r0, r1: ops.gemm_skinny_wide(w, x[r0:r1], o[0][r0:r1], 1, packed, norm_out=o[1][r0:r1], norm_gamma=gamma,
                                                           rowsq_out=o[2][r0:r1]),
                    lambda o, r0, r1: ops.gemm_skinny(w, x[r0:r1], o[0][r0:r1], 1, packed, norm_out=o[1][r0:r1], norm_gamma=gamma,
                                                      rowsq_out=o[2][r0:r1]))
            # consumer: 1 partial (31 lanes of a row add zeros) and 40 (more than the 32 lanes)
            for parts in (1, 40):
                sq = (rnd((M, parts), torch.float32, seed + 5 + parts).abs() * 16.0 + 0.5).to(dev)
                kw = dict(norm_dim=16 * parts, norm_eps=1e-5)
                compare(lambda: (guarded(ROWS, N, dtype, dev),),
                        lambda o, r0, r1: ops.gemm_skinny_wide(w, x[r0:r1], o[0][r0:r1], 0, packed, rowsq_in=sq[r0:r1], **kw),
                        lambda o, r0, r1: ops.gemm_skinny(w, x[r0:r1], o[0][r0:r1], 0, packed, rowsq_in=sq[r0:r1], **kw))
        # SwiGLU, N = 64 (gate | up rows interleaved in 32s), plain and as a consumer
        N = 64
        wg = lay(interleave_gate_up(rnd((N // 2, K), dtype, seed + 6, 0.1), rnd((N // 2, K), dtype, seed + 7, 0.1)).contiguous().to(dev))
        sq = (rnd((M, 40), torch.float32, seed + 8).abs() * 16.0 + 0.5).to(dev)
        compare(lambda: (guarded(ROWS, N // 2, dtype, dev),),
                lambda o, r0, r1: ops.gemm_skinny_wide(wg, x[r0:r1], o[0][r0:r1], 2, packed),
                lambda o, r0, r1: ops.gemm_skinny(wg, x[r0:r1], o[0][r0:r1], 2, packed))
        compare(lambda: (guarded(ROWS, N // 2, dtype, dev),),
                lambda o, r0, r1: ops.gemm_skinny_wide(wg, x[r0:r1], o[0][r0:r1], 2, packed, rowsq_in=sq[r0:r1], norm_dim=640, norm_eps=1e-5),
                lambda o, r0, r1: ops.gemm_skinny(wg, x[r0:r1], o[0][r0:r1], 2, packed, rowsq_in=sq[r0:r1], norm_dim=640, norm_eps=1e-5))


def check_gemm_wide_rejects(ops, dev):
    """M = 65 is refused by the wide entry, M = 17 still by the 16-row one."""
    import pytest
    x, w = rnd((65, 128), torch.float16, 1).to(dev), rnd((16, 128), torch.float16, 2).to(dev)
    out = torch.zeros(65, 16, dtype=torch.float16, device=dev)
    with pytest.raises(RuntimeError):
        ops.gemm_skinny_wide(w, x, out, 0)
    with pytest.raises(RuntimeError):
        ops.gemm_skinny(w, x[:17], out[:17], 0)


# ---- lmi_rope_qkv_skinny_wide -----------------------------------------------------------------------------------------------------------
def rope_tables(cap, hd=128):
    f = torch.arange(cap).float().reshape(-1, 1) * (1.0 / (10000.0 ** (torch.arange(0, hd, 2).float() / hd))).reshape(1, -1)
    return f.cos().contiguous(), f.sin().contiguous()


def check_rope_qkv_wide(ops, dev, dtype, layout, M, folded, H=4, KV=1, hd=128, K=256, cap=6, seed=0):
    """qkv rows and the appended K / V rows of lmi_rope_qkv_skinny_wide equal those of lmi_rope_qkv_skinny on the rows' groups of 16 (distinct
    positions per row, slot stride ``cap``); every other cache row and every qkv row >= M keeps the guard."""
    name, co, packed = layout
    N = (H + 2 * KV) * hd
    w = rnd((N, K), dtype, seed + 1, 0.1)
    w = torch.cat([rope_permute_rows(w[:(H + KV) * hd]), w[(H + KV) * hd:]]).contiguous().to(dev)
    w = skinny_pack(w) if packed else w
    x = rnd((M, K), dtype, seed + 2).to(dev)
    cos, sin = (t.to(dev) for t in rope_tables(cap, hd))
    pos = torch.tensor([(5 * m + 3) % cap for m in range(M)], dtype=torch.int32).to(dev)
    sq = (rnd((M, K // 16), torch.float32, seed + 3).abs() * 16.0 + 0.5).to(dev) if folded else None

    def run(wide, groups):
        qkv = guarded(ROWS, N, dtype, dev)
        kc, vc = guarded(ROWS * cap, KV * hd, dtype, dev), guarded(ROWS * cap, KV * hd, dtype, dev)
        for r0, r1 in groups:
            args = (w, x[r0:r1], qkv[r0:r1], H, KV, hd, cos, sin, kc[r0 * cap:], vc[r0 * cap:], cap, pos[r0:r1], packed)
            kw = dict(rowsq_in=None if sq is None else sq[r0:r1], norm_eps=1e-5)
            if wide:
                ops.rope_qkv_skinny_wide(*args, **kw)
            else:
                ops.rope_qkv_skinny(*args, **kw)
        sync(dev)
        return qkv, kc, vc
    with option(ops, "skinny.coalesce", co):
        wide = run(True, [(0, M)])
        again = run(True, [(0, M)])
        ref = run(False, row_groups(M))
    for t, (a, b, c) in enumerate(zip(wide, again, ref)):
        assert torch.equal(a, b), (name, M, folded, t, "two launches differ")
        assert torch.equal(a, c), (name, M, folded, t, "wide launch != its 16-row groups")
    qkv, kc, vc = wide
    assert bool((qkv[M:] == GUARD).all())
    touched = torch.zeros(ROWS * cap, dtype=torch.bool)
    touched[[m * cap + (5 * m + 3) % cap for m in range(M)]] = True
    assert bool((kc.cpu()[~touched] == GUARD).all()) and bool((vc.cpu()[~touched] == GUARD).all())
    assert not bool((kc.cpu()[touched] == GUARD).all(dim=1).any())         # ... and every appended row was written


# ---- the choice, rules and logprobs kernels at 64 rows ----------------------------------------------------------------------------------
def _cut(t, r0, r1, col=False):
    """An own contiguous copy of rows (``col``: columns) [r0, r1) of ``t``."""
    return (t[:, r0:r1] if col else t[r0:r1]).clone().contiguous()


def check_choice_kernels(ops, dev, B=64, V=256, hist_len=8, seed=0):
    """decode_advance, decode_sample, decode_rules and decode_logprobs on B = 64 rows of a 256-id vocabulary: every row's outputs and state
    equal those of the same call on the row's group of 16."""
    g = np.random.default_rng(seed)
    logits = torch.from_numpy(g.standard_normal((B, V)).astype(np.float32) * 3.0)
    logits[5] = logits[4]                                             # two rows with the same content, and a row with a tie at the top
    logits[40, 17] = logits[40, 200] = 50.0
    state = dict(tok=torch.from_numpy(g.integers(0, V, B)), pos=torch.from_numpy(g.integers(1, 50, B).astype(np.int32)),
                 k_len=torch.from_numpy(g.integers(2, 51, B).astype(np.int32)), live=torch.from_numpy((g.random(B) < 0.8).astype(np.int32)),
                 budget=torch.from_numpy(g.integers(1, 4, B).astype(np.int32)), hist_pos=torch.from_numpy(g.integers(0, hist_len, B).astype(np.int32)))
    hist = torch.from_numpy(g.integers(0, V, (hist_len, B)))
    eos = torch.tensor([int(logits[9].argmax()), int(logits[33].argmax()), -1, -1], dtype=torch.int64)
    suppress = torch.tensor([int(logits[20].argmax())], dtype=torch.int64)
    samp = dict(temperature=torch.from_numpy((g.random(B) * 1.5 + 0.2).astype(np.float32)), top_k=torch.from_numpy(g.integers(0, 40, B).astype(np.int32)),
                top_p=torch.from_numpy((g.random(B) * 0.6 + 0.4).astype(np.float32)), seed=torch.from_numpy(g.integers(0, 1 << 40, B)),
                step=torch.from_numpy(g.integers(0, 9, B).astype(np.int32)))

    def choose(sampled, r0, r1):
        s = {k: _cut(v, r0, r1).to(dev) for k, v in state.items()}
        h = _cut(hist, r0, r1, col=True).to(dev)
        lg = _cut(logits, r0, r1).to(dev)
        if sampled:
            p = {k: _cut(v, r0, r1).to(dev) for k, v in samp.items()}
            ops.decode_sample(lg, V, p["temperature"], p["top_k"], p["top_p"], p["seed"], p["step"], s["tok"], s["pos"], s["k_len"], s["live"],
                              s["budget"], eos.to(dev), h, s["hist_pos"], suppress.to(dev))
            s["step"] = p["step"]
        else:
            ops.decode_advance(lg, V, s["tok"], s["pos"], s["k_len"], s["live"], s["budget"], eos.to(dev), h, s["hist_pos"], suppress.to(dev))
        sync(dev)
        return {k: v.cpu() for k, v in s.items()}, h.cpu()
    for sampled in (False, True):
        full, hfull = choose(sampled, 0, B)
        assert not torch.equal(full["tok"], state["tok"])
        for r0, r1 in row_groups(B):
            part, hpart = choose(sampled, r0, r1)
            for k in full:
                assert torch.equal(full[k][r0:r1], part[k]), (sampled, k, r0)
            assert torch.equal(hfull[:, r0:r1], hpart), (sampled, "hist", r0)

    # rules: append tok, repetition penalty, n-gram ban, min_new_tokens countdown
    cap = 24
    seq = torch.from_numpy(g.integers(0, 12, (B, cap)).astype(np.int32))
    rs = dict(seq_len=torch.from_numpy(g.integers(1, cap - 1, B).astype(np.int32)), penalty=torch.from_numpy((g.random(B) + 1.0).astype(np.float32)),
              ngram=torch.from_numpy(g.integers(0, 4, B).astype(np.int32)), min_left=torch.from_numpy(g.integers(0, 3, B).astype(np.int32)))
    rtok = torch.from_numpy(g.integers(0, 12, B))

    def rules(r0, r1):
        lg, sq = _cut(logits, r0, r1).to(dev), _cut(seq, r0, r1).to(dev)
        s = {k: _cut(v, r0, r1).to(dev) for k, v in rs.items()}
        ops.decode_rules(lg, V, sq, s["seq_len"], s["penalty"], s["ngram"], s["min_left"], tok=_cut(rtok, r0, r1).to(dev),
                         live=_cut(state["live"], r0, r1).to(dev), eos=eos[:2].to(dev))
        sync(dev)
        return [lg.cpu(), sq.cpu(), s["seq_len"].cpu(), s["min_left"].cpu()]
    full = rules(0, B)
    assert not torch.equal(full[0], logits)
    for r0, r1 in row_groups(B):
        for t, (a, b) in enumerate(zip(full, rules(r0, r1))):
            assert torch.equal(a[r0:r1], b), ("rules", t, r0)

    # logprobs: ring slot (hist_pos - 1) mod ring of [ring, B] tables
    K8 = ops.MAX_TOP_LOGPROBS

    def logprobs(r0, r1):
        n = r1 - r0
        lp = torch.full((hist_len, n), GUARD, device=dev)
        ti = torch.full((hist_len, n, K8), -5, dtype=torch.int32, device=dev)
        tl = torch.full((hist_len, n, K8), GUARD, device=dev)
        ops.decode_logprobs(_cut(logits, r0, r1).to(dev), V, _cut(state["tok"], r0, r1).to(dev), 3, lp, ti, tl,
                            hist_pos=_cut(state["hist_pos"], r0, r1).to(dev))
        sync(dev)
        return lp.cpu(), ti.cpu(), tl.cpu()
    full = logprobs(0, B)
    assert bool((full[0] != GUARD).any(dim=0).all())
    for r0, r1 in row_groups(B):
        for t, (a, b) in enumerate(zip(full, logprobs(r0, r1))):
            assert torch.equal(a[:, r0:r1], b), ("logprobs", t, r0)


# ---- lmi_attn_decode_pool at n_seq = 64 --------------------------------------------------------------------------------------------------
def check_attention_pool_wide(ops, dev, dtype, lens, H=4, KV=1, hd=128, cap=128, seed=0):
    """64 sequences in one pooled launch (``lens``: their key counts): every output row equals the launch over its group of 16 (the split
    geometry depends on the capacity and the heads, not on n_seq; the workspace is that of 64 query rows)."""
    B = len(lens)
    assert B == 64 and max(lens) <= cap
    q = rnd((B, H * hd), dtype, seed + 1).to(dev)
    k, v = rnd((B * cap, KV * hd), dtype, seed + 2).to(dev), rnd((B * cap, KV * hd), dtype, seed + 3).to(dev)
    k_len = torch.tensor(lens, dtype=torch.int32).to(dev)
    k_begin = (torch.arange(B, dtype=torch.int32) * cap).to(dev)

    def run(r0, r1, out):
        n = r1 - r0
        ws = torch.empty(ops.decode_workspace_elems(n, H, hd, cap), dtype=torch.float32, device=dev)
        ops.attention_decode_pool(q[r0:r1], k, v, out[r0:r1], torch.arange(n + 1, dtype=torch.int32).to(dev), k_begin[r0:r1].clone(),
                                  k_len[r0:r1].clone(), cap, H, KV, hd, hd ** -0.5, ws)
    wide, ref = guarded(B + 1, H * hd, dtype, dev), guarded(B + 1, H * hd, dtype, dev)
    run(0, B, wide)
    for r0, r1 in row_groups(B):
        run(r0, r1, ref)
    sync(dev)
    assert torch.equal(wide, ref) and bool((wide[B] == GUARD).all()) and not bool((wide[:B] == GUARD).all(dim=1).any())
    # ... and against fp64 on a few rows, so that "equal" is not "equally wrong"
    for s in (0, 17, 63):
        kk = k[s * cap:s * cap + lens[s]].double().cpu().view(-1, KV, hd)
        vv = v[s * cap:s * cap + lens[s]].double().cpu().view(-1, KV, hd)
        qq = q[s].double().cpu().view(H, hd)
        for h in range(H):
            p = torch.softmax((kk[:, h * KV // H] @ qq[h]) * hd ** -0.5, 0)
            want = p @ vv[:, h * KV // H]
            assert (wide[s, h * hd:(h + 1) * hd].double().cpu() - want).abs().max() <= 2.0 ** (-7 if dtype == torch.bfloat16 else -9) * max(1.0, want.abs().max().item())


ATTN_LENS = {"len1": [1] * 64, "len64": [64] * 64, "len65": [65] * 64,
             "ragged": [1 + (37 * s + 11 * (s % 5)) % 128 for s in range(64)]}


# ---- the engine -------------------------------------------------------------------------------------------------------------------------
def text_requests(n, vocab_hi, seed, dev, base_len=5):
    """n text-only requests of unequal lengths (base_len + 0 .. 6 tokens, ids in [3, vocab_hi))."""
    g = np.random.default_rng(seed)
    return [(torch.from_numpy(g.integers(3, vocab_hi, (1, base_len + (3 * j) % 7))).to(dev), None) for j in range(n)]


def early_eos(outs, reqs, n_new):
    """An eos id that some request emits early (before its last new token) and some request never emits, from eos-free outputs."""
    new = [o[0, r[0].shape[1]:].tolist() for o, r in zip(outs, reqs)]
    for cand in sorted({t for row in new for t in row[1:n_new // 2]}):
        if any(cand not in row for row in new):
            return cand
    raise AssertionError("no token serves as an early eos for these requests")


def assert_same_outputs(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), (i, x.tolist(), y.tolist())


def check_one_step_bitwise(eng, dev, wide_B=33, vocab_hi=200, n_keys=9, seed=0):
    """One eager step body on a pooled state of ``wide_B`` slots and on one of 16: slot j of the wide state and the slot of the 16-state that
    holds the same K / V rows, token and position get bit-equal logits — for a j in the first column block and one in the third (row 32:
    with 33 rows lmi_rmsnorm would switch kernels if the step called it on all rows at once)."""
    eng.decode_batch_limit = 64
    eng.release_batch_state()
    need = n_keys + 2
    wide, small = eng._batch_state(wide_B, need), eng._batch_state(16, need)
    assert wide.B == wide_B and small.B == 16 and not wide.hl and not small.hl
    slot_of = list(range(16))
    slot_of[5], slot_of[11] = wide_B - 1, 18                         # small slot s <- wide slot slot_of[s]: rows of the third and second block
    g = torch.Generator().manual_seed(seed)
    tok = torch.randint(3, vocab_hi, (wide_B,), generator=g)
    pos = torch.randint(1, n_keys, (wide_B,), generator=g).to(torch.int32)
    for st, slots in ((wide, list(range(wide_B))), (small, slot_of)):
        for i in range(len(st.k)):
            gk = torch.Generator().manual_seed(seed + 100 + i)
            rows_k = torch.randn(wide_B, n_keys, st.k[i].shape[1], generator=gk).to(st.k[i].dtype)
            rows_v = torch.randn(wide_B, n_keys, st.k[i].shape[1], generator=gk).to(st.k[i].dtype)
            for s, j in enumerate(slots):
                st.k[i][s * st.capacity:s * st.capacity + n_keys].copy_(rows_k[j].to(dev))
                st.v[i][s * st.capacity:s * st.capacity + n_keys].copy_(rows_v[j].to(dev))
        st.tok.copy_(tok[slots].to(dev))
        st.pos.copy_(pos[slots].to(dev))
        st.k_len.copy_((pos[slots] + 1).to(dev))
        st.live.fill_(1); st.budget.fill_(1 << 30); st.eos.fill_(-1); st.hist_pos.zero_()
        st.sampling, st.beams = False, 0
        eng._set_logprobs(st, None)
        eng._set_rules(st, None, ())
        eng._batch_decode_body(st)
    sync(dev)
    for s, j in enumerate(slot_of):
        assert torch.equal(small.logits[s], wide.logits[j]), (s, j)
    assert torch.equal(small.tok.cpu(), wide.tok.cpu()[slot_of])
    eng.release_batch_state()


# ---- device only: the Llama-3.1-8B projection shapes ------------------------------------------------------------------------------------
LLAMA_SHAPES = (("qkv", 6144, 4096, 0), ("o", 4096, 4096, 1), ("gate_up", 28672, 4096, 2), ("down", 4096, 14336, 1))


def check_gemm_wide_llama_shapes(ops, dev, dtype, M):
    """lmi_gemm_skinny_wide at the q|k|v, o, gate/up and down shapes of a Llama-3.1-8B step (packed weights, thousands of workgroups, K of
    32 and 112 steps): rows bit-equal to the 16-row kernel on their groups of 16, also against fp64 on one row."""
    for name, N, K, epi in LLAMA_SHAPES:
        x, w = rnd((M, K), dtype, 11).to(dev), rnd((N, K), dtype, 12, 0.02).to(dev)
        wp = skinny_pack(w)
        cols = N // 2 if epi == 2 else N
        odt = torch.float32 if epi == 1 else dtype
        base = rnd((M, cols), torch.float32, 13).to(dev) if epi == 1 else None
        wide, ref = guarded(ROWS, cols, odt, dev, top=base), guarded(ROWS, cols, odt, dev, top=base)
        ops.gemm_skinny_wide(wp, x, wide[:M], epi, True)
        for r0, r1 in row_groups(M):
            ops.gemm_skinny(wp, x[r0:r1], ref[r0:r1], epi, True)
        sync(dev)
        assert torch.equal(wide, ref), (name, M)
        assert bool((wide[M:] == GUARD).all()), (name, M)
        m = M - 1
        lin = x[m].double().cpu() @ w.double().cpu().T
        if epi == 2:
            lv = lin.view(N // 64, 2, 32)
            want = (torch.nn.functional.silu(lv[:, 0]) * lv[:, 1]).reshape(-1)
        else:
            want = lin + (base[m].double().cpu() if epi == 1 else 0.0)
        # fp32 sums of exact products: at most K 2^-24 sum |x_k w_nk| from the truth, whatever the order; then one rounding to the stored
        # type (half an ulp; none for the fp32 residual); SwiGLU passes the error of its two sums on with slopes <= 1.1 |up| and |silu(gate)|
        err = K * 2.0 ** -24 * (x[m].double().cpu().abs() @ w.double().cpu().abs().T).max().item()
        if epi == 2:
            err *= 1.1 * lin.abs().max().item() + 1.0
        half_ulp = 0.0 if epi == 1 else (2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11)
        assert (wide[m].double().cpu() - want).abs().max() <= half_ulp * want.abs().max().item() + err, (name, M)
