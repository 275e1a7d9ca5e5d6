"""Wide pair decode (decode_pair_limit > 8): the cases and the pair-group comparison shared by tests/test_emu_wide_pair.py (emulator) and
tests/test_gpu_wide_pair.py (device).

The contract under test is BIT EQUALITY, not a tolerance: pair m (its hi row m and its lo row m + M) of a launch over up to 32 pairs equals
pair m of the existing launch over any group of at most 8 pairs that contains it (lmi_gemm_skinny_wide_hl / lmi_rope_qkv_skinny_wide_hl
against lmi_gemm_skinny_hl / lmi_rope_qkv_skinny_hl; lmi_attn_decode_pool_hl at up to 32 sequences against itself at 8).  A group's X is the
hi rows [r0, r1) followed by the lo rows [M + r0, M + r1) of the wide X; its pair outputs are copied to the rows they have in the wide
layout, and whole buffers are compared, guard rows included.  The accuracy of the pair step is pinned by tests/decode_hl_ref.py and the
decode fixture; nothing here has a tolerance."""
import numpy as np
import torch

from leopard_amd.weights import interleave_gate_up, rope_permute_rows, skinny_pack
from tests import decode_hl_ref as H
from tests import wide_decode_ref as R

GUARD = R.GUARD
PAIRS = 32                                                             # single buffers hold PAIRS + 1 rows, pair buffers 2 PAIRS + 1
DTYPES = R.DTYPES
LAYOUTS = R.LAYOUTS
# 9: 18 rows — the lo rows start mid-block and cross the 16-row boundary of X; 16: hi and lo each fill one column block; 17: the four-block
# form with one live row in blocks 1 and 3; 24; 32: the full width
PAIR_M = (9, 16, 17, 24, 32)
# 128: one k-step (seven waves hold zero partials), 1280: ten steps (uneven steps per wave), 1792: fourteen
PAIR_K = (128, 1280, 1792)
sync, rnd, option = R.sync, R.rnd, R.option


def pair_groups(M, first=8):
    """[0, M) cut into groups of at most 8 pairs; ``first`` < 8 shifts every later boundary, so a pair meets other lanes of the 16-row kernel."""
    cuts = [0] + list(range(first, M, 8)) + [M]
    return [(a, b) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]


def group_x(X, M, r0, r1):
    """The [hi rows; lo rows] operand of pairs [r0, r1) of the wide operand X [2 M, K]."""
    return torch.cat([X[r0:r1], X[M + r0:M + r1]], 0).contiguous()


class Out:
    """One output buffer of a comparison: ``pair`` buffers hold rows m and m + M (2 PAIRS + 1 rows), single ones row m (PAIRS + 1 rows)."""
    def __init__(self, cols, dtype, dev, pair, top=None):
        self.pair = pair
        self.buf = R.guarded((2 if pair else 1) * PAIRS + 1, cols, dtype, dev, top=top)

    def wide(self, M):
        return self.buf[:2 * M] if self.pair else self.buf[:M]

    def group(self, r0, r1):
        """What the 8-pair entry writes for pairs [r0, r1): the rows themselves (single) or a scratch pair buffer (``put`` copies it back)."""
        if not self.pair:
            return self.buf[r0:r1]
        self.tmp = R.guarded(2 * (r1 - r0) + 1, self.buf.shape[1], self.buf.dtype, self.buf.device)
        return self.tmp[:2 * (r1 - r0)]

    def put(self, M, r0, r1):
        if self.pair:
            n = r1 - r0
            assert bool((self.tmp[2 * n:] == GUARD).all())
            self.buf[r0:r1] = self.tmp[:n]
            self.buf[M + r0:M + r1] = self.tmp[n:2 * n]

    def rows(self, M):
        return 2 * M if self.pair else M


def compare(dev, M, what, make, call_wide, call_ref, firsts=(8, 3)):
    """make() -> list of fresh Out; call_wide(views) launches all M pairs; call_ref(views, r0, r1) the 8-pair entry on pairs [r0, r1)."""
    wide, again = make(), make()
    call_wide([o.wide(M) for o in wide])
    call_wide([o.wide(M) for o in again])
    sync(dev)
    for a, b in zip(wide, again):
        assert torch.equal(a.buf, b.buf), (what, "two launches differ")
    for t, o in enumerate(wide):
        assert bool((o.buf[o.rows(M):] == GUARD).all()), (what, t, "rows past the pairs were written")
        assert not bool((o.buf[:o.rows(M)] == GUARD).all(dim=1).any()), (what, t, "a live row was not written")
    for first in firsts:
        ref = make()
        for r0, r1 in pair_groups(M, first):
            call_ref([o.group(r0, r1) for o in ref], r0, r1)
            for o in ref:
                o.put(M, r0, r1)
        sync(dev)
        for t, (a, b) in enumerate(zip(wide, ref)):
            assert torch.equal(a.buf, b.buf), (what, first, t, "pair of the wide launch != pair of its 8-pair group")


# ---- lmi_gemm_skinny_wide_hl ------------------------------------------------------------------------------------------------------------
def check_gemm_pair(ops, dev, dtype, layout, M, K, seed=0):
    """Every epilogue, the producer (residual + norm_out pair + rowsq_out) and the consumer (1 and 40 partials) of lmi_gemm_skinny_wide_hl in
    one weight layout against lmi_gemm_skinny_hl on groups of at most 8 pairs (two groupings)."""
    name, co, packed = layout
    lay = (lambda w: skinny_pack(w)) if packed else (lambda w: w)
    X = H.pair(rnd((M, K), torch.float32, seed + 1), dtype).to(dev)
    gx = lambda r0, r1: group_x(X, M, r0, r1)
    with option(ops, "skinny.coalesce", co):
        # N = 16 (one block: above 16 pairs the workgroup's second block is dead), and 48 at the uneven K (a full workgroup + a half-dead one)
        for N in (16, 48) if K == 1280 else (16,):
            w = lay(rnd((N, K), dtype, seed + 2, 0.1).to(dev))
            base = rnd((M, N), torch.float32, seed + 3)
            tag = (name, M, K, N)
            for epi, odt, pair, top in ((0, dtype, True, None), (3, torch.float32, False, None), (1, torch.float32, False, base)):
                compare(dev, M, tag + (epi,), lambda: [Out(N, odt, dev, pair, top)],
                        lambda o: ops.gemm_skinny_wide_hl(w, X, o[0], epi, packed),
                        lambda o, r0, r1: ops.gemm_skinny(w, gx(r0, r1), o[0], epi, packed, hl=True))
            gamma = (rnd((N,), torch.float32, seed + 4) + 1.0).to(dev)
            compare(dev, M, tag + ("producer",),
                    lambda: [Out(N, torch.float32, dev, False, base), Out(N, dtype, dev, True), Out(N // 16, torch.float32, dev, False)],
                    lambda o: ops.gemm_skinny_wide_hl(w, X, o[0], 1, packed, norm_out=o[1], norm_gamma=gamma, rowsq_out=o[2]),
                    lambda o, r0, r1: ops.gemm_skinny(w, gx(r0, r1), o[0], 1, packed, norm_out=o[1], norm_gamma=gamma, rowsq_out=o[2], hl=True))
            for parts in (1, 40):                                        # 1: 31 lanes of a row add zeros; 40: more than the 32 lanes
                sq = (rnd((M, parts), torch.float32, seed + 5 + parts).abs() * 16.0 + 0.5).to(dev)
                kw = dict(norm_dim=16 * parts, norm_eps=1e-5)
                compare(dev, M, tag + ("consumer", parts), lambda: [Out(N, dtype, dev, True)],
                        lambda o: ops.gemm_skinny_wide_hl(w, X, o[0], 0, packed, rowsq_in=sq, **kw),
                        lambda o, r0, r1: ops.gemm_skinny(w, gx(r0, r1), o[0], 0, packed, rowsq_in=sq[r0:r1], hl=True, **kw))
        N = 64                                                           # SwiGLU (gate | up rows interleaved in 32s), plain and as a consumer
        wg = lay(interleave_gate_up(rnd((N // 2, K), dtype, seed + 6, 0.1), rnd((N // 2, K), dtype, seed + 7, 0.1)).contiguous().to(dev))
        sq = (rnd((M, 40), torch.float32, seed + 8).abs() * 16.0 + 0.5).to(dev)
        for kw_of in (lambda r0, r1: {}, lambda r0, r1: dict(rowsq_in=sq[r0:r1], norm_dim=640, norm_eps=1e-5)):
            compare(dev, M, (name, M, K, "swiglu", bool(kw_of(0, M))), lambda: [Out(N // 2, dtype, dev, True)],
                    lambda o: ops.gemm_skinny_wide_hl(wg, X, o[0], 2, packed, **kw_of(0, M)),
                    lambda o, r0, r1: ops.gemm_skinny(wg, gx(r0, r1), o[0], 2, packed, hl=True, **kw_of(r0, r1)))


def check_pair_refusals(ops, dev):
    """M = 33 and a row_bias are refused by the entries themselves (an error return: nothing is launched, nothing written); M = 9 still by
    the 8-pair entry."""
    import pytest
    K, Hq, KV, hd, cap = 128, 4, 1, 128, 4
    x = rnd((66, K), torch.float16, 1).to(dev)
    w = rnd((16, K), torch.float16, 2).to(dev)
    out = torch.full((66, 16), GUARD, dtype=torch.float16, device=dev)
    with pytest.raises(RuntimeError):
        ops.gemm_skinny_wide_hl(w, x, out, 0)
    with pytest.raises(RuntimeError):
        ops.gemm_skinny(w, x[:18], out[:18], 0, hl=True)
    N = (Hq + 2 * KV) * hd
    wq = rnd((N, K), torch.float16, 3, 0.1).to(dev)
    qkv = torch.full((33, N), GUARD, dtype=torch.float16, device=dev)
    kc, vc = (torch.full((33 * cap, KV * hd), GUARD, dtype=torch.float16, device=dev) for _ in range(2))
    cos, sin = (t.to(dev) for t in R.rope_tables(cap, hd))
    pos = torch.zeros(33, dtype=torch.int32, device=dev)
    args = lambda M: (wq, x[:2 * M], qkv[:M], Hq, KV, hd, cos, sin, kc, vc, cap, pos[:M])
    with pytest.raises(RuntimeError):
        ops.rope_qkv_skinny_wide_hl(*args(33))
    with pytest.raises(RuntimeError):
        ops.rope_qkv_skinny_wide_hl(*args(9), row_bias=torch.zeros(1, dtype=torch.int32, device=dev))
    sync(dev)
    for t in (out, qkv, kc, vc):
        assert bool((t == GUARD).all())
    ops.rope_qkv_skinny_wide_hl(*args(9))                                # ... and the same call without the bias runs
    sync(dev)
    assert not bool((qkv[:9] == GUARD).all(dim=1).any()) and bool((qkv[9:] == GUARD).all())


# ---- lmi_rope_qkv_skinny_wide_hl --------------------------------------------------------------------------------------------------------
def check_rope_qkv_pair(ops, dev, dtype, layout, M, K, folded, Hq=4, KV=1, hd=128, cap=6, seed=0):
    """qkv rows and the appended K / V rows of lmi_rope_qkv_skinny_wide_hl equal those of lmi_rope_qkv_skinny_hl on the pairs' groups of 8
    (positions (5 m + 3) % cap: 0 and cap - 1 among them); every other cache row and every qkv row >= M keeps the guard."""
    name, co, packed = layout
    N = (Hq + 2 * KV) * hd
    w = rnd((N, K), dtype, seed + 1, 0.1)
    w = torch.cat([rope_permute_rows(w[:(Hq + KV) * hd]), w[(Hq + KV) * hd:]]).contiguous().to(dev)
    w = skinny_pack(w) if packed else w
    X = H.pair(rnd((M, K), torch.float32, seed + 2), dtype).to(dev)
    cos, sin = (t.to(dev) for t in R.rope_tables(cap, hd))
    where = [(5 * m + 3) % cap for m in range(M)]
    assert 0 in where and cap - 1 in where
    pos = torch.tensor(where, dtype=torch.int32).to(dev)
    sq = (rnd((M, K // 16), torch.float32, seed + 3).abs() * 16.0 + 0.5).to(dev) if folded else None

    def run(groups, wide=False):
        qkv = R.guarded(PAIRS + 1, N, dtype, dev)
        kc, vc = R.guarded(PAIRS * cap, KV * hd, dtype, dev), R.guarded(PAIRS * cap, KV * hd, dtype, dev)
        for r0, r1 in groups:
            kw = dict(rowsq_in=None if sq is None else sq[r0:r1], norm_eps=1e-5)
            if wide:
                ops.rope_qkv_skinny_wide_hl(w, X, qkv[:M], Hq, KV, hd, cos, sin, kc, vc, cap, pos, packed, **kw)
            else:
                ops.rope_qkv_skinny(w, group_x(X, M, r0, r1), qkv[r0:r1], Hq, KV, hd, cos, sin, kc[r0 * cap:], vc[r0 * cap:], cap, pos[r0:r1], packed,
                                    hl=True, **kw)
        sync(dev)
        return qkv, kc, vc
    with option(ops, "skinny.coalesce", co):
        wide, again = run([(0, M)], True), run([(0, M)], True)
        refs = [run(pair_groups(M, first)) for first in (8, 3)]
    for t, (a, b) in enumerate(zip(wide, again)):
        assert torch.equal(a, b), (name, M, K, folded, t, "two launches differ")
    for ref in refs:
        for t, (a, c) in enumerate(zip(wide, ref)):
            assert torch.equal(a, c), (name, M, K, folded, t, "wide pair launch != its 8-pair groups")
    qkv, kc, vc = wide
    assert bool((qkv[M:] == GUARD).all()) and not bool((qkv[:M] == GUARD).all(dim=1).any())
    touched = torch.zeros(PAIRS * cap, dtype=torch.bool)
    touched[[m * cap + p for m, p in enumerate(where)]] = True
    assert bool((kc.cpu()[~touched] == GUARD).all()) and bool((vc.cpu()[~touched] == GUARD).all())
    assert not bool((kc.cpu()[touched] == GUARD).all(dim=1).any()) and not bool((vc.cpu()[touched] == GUARD).all(dim=1).any())


# ---- lmi_attn_decode_pool_hl at 9 .. 32 sequences ---------------------------------------------------------------------------------------
ATT_SEQS = (9, 17, 32)


def check_attention_pool_pair(ops, dev, dtype, B, window, Hq=4, KV=1, seed=0):
    """B sequences in one pooled pair launch (lengths: decode_hl_ref.ATT_LENS, repeated): every sequence's hi and lo output row equals the
    launch over a group of at most 8 sequences that holds it (two groupings)."""
    hd, cap = H.ATT_HD, H.ATT_CAP
    lens = [H.ATT_LENS[(s + s // len(H.ATT_LENS)) % len(H.ATT_LENS)] for s in range(B)]
    q = rnd((B, Hq * hd), dtype, seed + 1).to(dev)
    k, v = rnd((B * cap, KV * hd), dtype, seed + 2).to(dev), rnd((B * cap, KV * hd), dtype, seed + 3).to(dev)
    k_len = torch.tensor(lens, dtype=torch.int32).to(dev)
    k_begin = (torch.arange(B, dtype=torch.int32) * cap).to(dev)

    def run(r0, r1, out):
        n = r1 - r0
        ws = torch.empty(ops.decode_workspace_elems(n, Hq, hd, cap), dtype=torch.float32, device=dev)
        ops.attention_decode_pool(q[r0:r1], k, v, out[:2 * n], torch.arange(n + 1, dtype=torch.int32).to(dev), k_begin[r0:r1].clone(),
                                  k_len[r0:r1].clone(), cap, Hq, KV, hd, hd ** -0.5, ws, window=window, hl=True)
    wide = R.guarded(2 * B + 1, Hq * hd, dtype, dev)
    run(0, B, wide)
    sync(dev)
    assert bool((wide[2 * B:] == GUARD).all()) and not bool((wide[:B] == GUARD).all(dim=1).any())
    assert wide[B:2 * B].double().abs().max() > 0
    for first in (8, 3):
        ref = R.guarded(2 * B + 1, Hq * hd, dtype, dev)
        for r0, r1 in pair_groups(B, first):
            n = r1 - r0
            tmp = R.guarded(2 * n + 1, Hq * hd, dtype, dev)
            run(r0, r1, tmp)
            ref[r0:r1], ref[B + r0:B + r1] = tmp[:n], tmp[n:2 * n]
        sync(dev)
        assert torch.equal(wide, ref), (B, window, first)


# ---- the engine -------------------------------------------------------------------------------------------------------------------------
T_NEW = 12


def set_limits(eng, pair, batch=32):
    eng.decode_batch_limit = batch
    eng.decode_pair_limit = pair


def same_logprob_outputs(a, b):
    R.assert_same_outputs(a.sequences, b.sequences)
    for ring in ("token_logprobs", "top_ids", "top_logprobs"):
        for i, (x, y) in enumerate(zip(getattr(a, ring), getattr(b, ring))):
            assert torch.equal(x, y), (ring, i)


def batch_in_groups_of_8(eng, reqs, **kw):
    """generate_batch of ``reqs`` under the default pair limit, at most 8 requests per call: every call decodes on the 8-pair step."""
    from leopard_amd.engine import GenerateOutput
    set_limits(eng, 8)
    assert len(reqs) % 8 != 1                                            # (a call with one request is generate(): the batch-1 step)
    outs = []
    for g0 in range(0, len(reqs), 8):
        outs.append(eng.generate_batch(reqs[g0:g0 + 8], max_new_tokens=T_NEW, eos_token_id=(), **kw))
        st = eng._batch_states[len(reqs[g0:g0 + 8])]
        assert st.hl
    return GenerateOutput.join(outs) if kw.get("logprobs") is not None else [o for part in outs for o in part]


def check_generate_batch_pair(eng, reqs, ref, n, captured):
    """generate_batch of the first n requests under decode_pair_limit = 32 with logprobs=2: one pooled pair state of n slots, one captured
    step, every request's tokens and log-prob tensors those of ``ref`` (batch_in_groups_of_8 of the same requests)."""
    from leopard_amd.engine import GenerateOutput
    set_limits(eng, 32)
    assert eng.decode_hl(n) and not eng.decode_hl(33)
    steps, body = [], eng._batch_decode_body
    eng._batch_decode_body = lambda st: (steps.append((st.B, st.hl)), body(st))[1]
    try:
        out = eng.generate_batch(reqs[:n], max_new_tokens=T_NEW, eos_token_id=(), logprobs=2)
    finally:
        eng._batch_decode_body = body
    st = eng._batch_states[n]
    assert st.hl and st.B == n and st.h.shape[0] == 2 * n and st.qkv.shape[0] == n
    if captured:                                                         # warm-up + capture, afterwards the ONE graph replays (no Python body)
        assert steps == [(n, True)] * 2, steps
        assert list(st.graphs) == [(False, True)] and st.graphs[(False, True)] is not None      # key: (sampling, with logprobs)
    else:
        assert steps == [(n, True)] * (T_NEW - 1)
    want = GenerateOutput(sequences=ref.sequences[:n], token_logprobs=ref.token_logprobs[:n], top_ids=ref.top_ids[:n],
                          top_logprobs=ref.top_logprobs[:n])
    same_logprob_outputs(out, want)


def check_stream_pair(eng, reqs, eos):
    """generate_stream(batch_size=16) with more requests than slots on the wide pair step against batch_size=8 on the 8-pair step."""
    set_limits(eng, 8)
    ref = eng.generate_stream(reqs, batch_size=8, max_new_tokens=T_NEW, eos_token_id=eos)
    assert eng._batch_states[8].hl
    assert any(o.shape[1] < r[0].shape[1] + T_NEW for o, r in zip(ref, reqs))       # slots are retired early and refilled
    set_limits(eng, 32)
    stats = {}
    out = eng.generate_stream(reqs, batch_size=16, max_new_tokens=T_NEW, eos_token_id=eos, stats=stats)
    assert stats["batch_size"] == 16 and eng._batch_states[16].hl and eng._batch_states[16].B == 16
    R.assert_same_outputs(out, ref)


def check_rules_pair(eng, reqs):
    from leopard_amd.engine import LogitsRules
    rules = LogitsRules(1.3, 3, 4)
    ref = batch_in_groups_of_8(eng, reqs, rules=rules)
    set_limits(eng, 32)
    out = eng.generate_batch(reqs, max_new_tokens=T_NEW, eos_token_id=(), rules=rules)
    assert eng._batch_states[len(reqs)].hl
    R.assert_same_outputs(out, ref)


def check_default_limit_keeps_the_fast_step(eng, reqs):
    """decode_pair_limit left at 8: 17 requests decode on the fast wide step (hl False) to the tokens the fast 16-row step gives them."""
    set_limits(eng, 8)
    assert eng.decode_pair_limit == 8 and eng.decode_hl(8) and not eng.decode_hl(9)
    stats = {}
    out = eng.generate_stream(reqs[:17], batch_size=17, max_new_tokens=6, eos_token_id=(), stats=stats)
    assert stats["batch_size"] == 17 and eng._batch_states[17].hl is False
    R.assert_same_outputs(out, eng.generate_stream(reqs[:17], batch_size=16, max_new_tokens=6, eos_token_id=()))
    batch = eng.generate_batch(reqs[:17], max_new_tokens=6, eos_token_id=())
    assert eng._batch_states[17].hl is False
    R.assert_same_outputs(batch, out)


def check_limit_values(eng):
    import pytest
    eng.decode_pair_limit = 8
    for bad in (7, 33, 0, -1, 16.0, "16", None, True):
        with pytest.raises(ValueError):
            eng.decode_pair_limit = bad
    assert eng.decode_pair_limit == 8
    for ok in (8, 9, 32):
        eng.decode_pair_limit = ok
        assert eng.decode_pair_limit == ok
    eng.decode_pair_limit = 8


def check_state_rebuilt_after_limit_change(eng, reqs):
    """A 9-slot state built under limit 8 (the fast step) is not replayed once the limit is 32: the next call builds the pair state."""
    set_limits(eng, 8)
    eng.generate_batch(reqs[:9], max_new_tokens=3, eos_token_id=())
    old = eng._batch_states[9]
    assert old.hl is False
    set_limits(eng, 32)
    assert 9 not in eng._batch_states or eng._batch_states[9] is not old
    eng.generate_batch(reqs[:9], max_new_tokens=3, eos_token_id=())
    new = eng._batch_states[9]
    assert new is not old and new.hl is True
    set_limits(eng, 32)                                                  # the same value again keeps the state
    assert eng._batch_states[9] is new


def reset(eng):
    eng.decode_pair_limit = 8
    eng.decode_batch_limit = eng.MAX_DECODE_BATCH
    eng.release_batch_state()
