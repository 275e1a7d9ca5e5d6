"""Scoring rows that continue a cached prefix, on the CPU emulator build: LeopardEngine.extend_score / score_shared and the
loglikelihood_shared / loglikelihood(share_prefix=True) surfaces on the micro model of tests/test_emu_prefix.py (hidden 512, 4 query heads on
1 KV head: the shape attention="rows" serves) against score_batch of the concatenated prompts, with both attention launches and both
schedules; the prefix cache is never written; every refusal comes before a launch."""
import os

import numpy as np
import pytest
import torch

from tests.emu_util import emu_ops
from tests.test_emu_prefix import _engine_setup, _prefilled

DTYPE = torch.float16
BOUND = 2e-3 * 2          # tests/test_emu_prefix.py: what extend's logits are held to (beside a from-scratch prefill, against the oracle)


@pytest.fixture(scope="module")
def ops():
    assert "HIPEMU_SYNC_DMA" not in os.environ, "the LDS-DMA asynchrony model must be on (unset HIPEMU_SYNC_DMA)"
    return emu_ops()


@pytest.fixture(scope="module")
def micro(ops):
    cfg, eng, u8, pix, ids, Wn = _engine_setup(ops, DTYPE, hidden=512, heads=4)
    return cfg, eng, u8, ids


def requests_of(ids):
    """(head, [(tail, continuation)]): the prompt without its last 48 ids, and four ways to go on — tails of 1 .. 3 ids, continuations of
    1 .. 6 ids."""
    head = ids[:, :-48]
    q = ids[0, -48:]
    reqs = [(q[:1], q[1:7]), (q[:3], q[3:4]), (q[:2], torch.tensor([9, 8, 7])), (q[:1], torch.tensor([11, 12]))]
    return head, [(t.reshape(1, -1), c.reshape(1, -1)) for t, c in reqs]


def as_extend(reqs):
    out = []
    for t, c in reqs:
        ign = torch.full((1, t.numel() - 1), -100, dtype=torch.int64)
        out.append((torch.cat([t, c[:, :-1]], dim=1), torch.cat([ign, c], dim=1)))
    return out


def as_full(head, u8, reqs):
    out = []
    for t, c in reqs:
        ctx = torch.cat([head, t], dim=1)
        out.append((torch.cat([ctx, c], dim=1), u8, torch.cat([torch.full_like(ctx, -100), c], dim=1)))
    return out


@pytest.mark.parametrize("precision", ["fast", "lo4"])
def test_extend_score_matches_score_batch_of_the_concatenated_prompts(micro, precision):
    """extend_score, both attention launches, against score_batch of [prefix ; suffix]: the same targets and (suffix-relative) rows, token
    log-probs within the bound tests/test_emu_prefix.py holds extend to; the prefix cache is bit-identical afterwards and a second call gives the
    same bits."""
    cfg, eng, u8, ids = micro
    eng.precision = precision
    try:
        head, reqs = requests_of(ids)
        full = eng.score_batch(as_full(head, u8, reqs))
        prefix = _prefilled(eng, cfg, head, u8, DTYPE)
        P = prefix.length
        k0, v0 = [t.clone() for t in prefix.k], [t.clone() for t in prefix.v]
        for attention in ("ranges", "rows"):
            got = eng.extend_score(prefix, as_extend(reqs), attention=attention)
            assert len(got) == len(reqs)
            worst = 0.0
            for (t, c), g, f in zip(reqs, got, full):
                assert g.seq_len == t.numel() + c.numel() - 1
                assert torch.equal(g.target_ids, f.target_ids) and torch.equal(g.rows, f.rows - P)
                worst = max(worst, (g.token_logprobs - f.token_logprobs).abs().max().item())
                assert g.loss.shape == () and abs(float(g.loss) - float(f.loss)) <= BOUND
            print(f"[{precision}, {attention}] max |token logprob - score_batch| = {worst:.3e} (bound {BOUND:.1e})")
            assert worst <= BOUND
            again = eng.extend_score(prefix, as_extend(reqs), attention=attention)
            for a, b in zip(got, again):
                assert torch.equal(a.token_logprobs, b.token_logprobs) and torch.equal(a.argmax, b.argmax)
            assert all(torch.equal(a, b) for a, b in zip(prefix.k, k0)) and all(torch.equal(a, b) for a, b in zip(prefix.v, v0))
            assert prefix.length == P
    finally:
        eng.precision = "fast"


def test_extend_score_empty_result_and_unscored_rows(micro):
    """A request without a scored row gives score()'s empty result; -100 rows inside a scored request are left out."""
    cfg, eng, u8, ids = micro
    head, reqs = requests_of(ids)
    prefix = _prefilled(eng, cfg, head, u8, DTYPE)
    sfx = torch.tensor([[5, 6, 7, 8]])
    none = eng.extend_score(prefix, [(sfx, torch.full((1, 4), -100))])
    assert none[0].seq_len == 4 and none[0].rows.numel() == 0 and bool(torch.isnan(none[0].loss))
    two = eng.extend_score(prefix, [(sfx, torch.tensor([[-100, 3, -100, 4]])), (sfx, torch.full((1, 4), -100))])
    assert two[0].rows.tolist() == [1, 3] and two[0].target_ids.tolist() == [3, 4] and two[1].rows.numel() == 0
    alone = eng.extend_score(prefix, [(sfx, torch.tensor([[-100, 3, -100, 4]]))])
    assert torch.equal(alone[0].token_logprobs, two[0].token_logprobs)


@pytest.mark.parametrize("attention", ["ranges", "rows"])
def test_score_shared_empty_tail_equals_the_last_prefix_id_as_tail(micro, attention):
    """score_shared moves the last prefix id into the suffixes when a tail is empty: the same call as passing it as the tail.  The vision tower
    runs once per call; the surface returns (sum, is_greedy) of the same numbers."""
    cfg, eng, u8, ids = micro
    head, _ = requests_of(ids)
    conts = [torch.tensor([[9, 8, 7]]), torch.tensor([[11]]), ids[:, -48:-44]]
    empty = torch.zeros(1, 0, dtype=torch.int64)
    towers = []
    enc = eng.encode_images
    eng.encode_images = lambda *a, **k: (towers.append(1), enc(*a, **k))[1]
    try:
        a = eng.score_shared(head, u8, [(empty, c) for c in conts], attention=attention)
        assert len(towers) == 1
        b = eng.score_shared(head[:, :-1], u8, [(head[:, -1:], c) for c in conts], attention=attention)
    finally:
        eng.encode_images = enc
    for x, y, c in zip(a, b, conts):
        assert torch.equal(x.token_logprobs, y.token_logprobs) and torch.equal(x.argmax, y.argmax) and torch.equal(x.rows, y.rows)
        assert x.rows.tolist() == list(range(c.numel())) and x.target_ids.tolist() == c.reshape(-1).tolist()
    # a mixed call: one empty tail moves the id into EVERY suffix
    mixed = eng.score_shared(head, u8, [(empty, conts[0]), (torch.tensor([[5]]), conts[1])], attention=attention)
    assert mixed[0].rows.tolist() == [0, 1, 2] and mixed[1].rows.tolist() == [1]
    prefix = _prefilled(eng, cfg, head[:, :-1], u8, DTYPE)
    c = eng.score_shared(head[:, :-1], None, [(head[:, -1:], x) for x in conts], prefix=prefix, attention=attention)
    for x, y in zip(b, c):
        assert torch.equal(x.token_logprobs, y.token_logprobs)


def test_score_shared_default_attention(ops, micro):
    """attention=None: the row-packed launch where it serves the model (4 query heads per KV head), the two-range launch where it does not —
    the explicit call's bits either way."""
    cfg, eng, u8, ids = micro
    head, reqs = requests_of(ids)
    assert eng.SCORE_SHARED_ATTENTION == "rows"
    for a, b in zip(eng.score_shared(head, u8, reqs), eng.score_shared(head, u8, reqs, attention="rows")):
        assert torch.equal(a.token_logprobs, b.token_logprobs)
    _, eng2, u8b, _, ids2, _ = _engine_setup(ops, DTYPE, hidden=256, heads=2)
    for a, b in zip(eng2.score_shared(ids2[:, :-48], u8b, reqs), eng2.score_shared(ids2[:, :-48], u8b, reqs, attention="ranges")):
        assert torch.equal(a.token_logprobs, b.token_logprobs)


def test_score_shared_errors_raise_before_any_launch(ops, micro):
    from leopard_amd.engine import KVCache
    cfg, eng, u8, ids = micro
    head, reqs = requests_of(ids)
    prefix = _prefilled(eng, cfg, head, u8, DTYPE)
    ext = as_extend(reqs)
    V = cfg.text_config.vocab_size
    empty = torch.zeros(1, 0, dtype=torch.int64)
    launches = []
    check = ops._check
    ops._check = lambda rc: (launches.append(1), check(rc))[1]
    try:
        with pytest.raises(ValueError, match="targets"):
            eng.extend_score(prefix, [(ext[0][0], torch.full_like(ext[0][1], V))])
        with pytest.raises(ValueError, match="targets"):
            eng.extend_score(prefix, [(ext[0][0], torch.full_like(ext[0][1], -5))])
        with pytest.raises(ValueError, match="targets"):
            eng.extend_score(prefix, [ext[1], (ext[0][0], ext[0][1][:, :-1])])
        with pytest.raises(ValueError, match="empty"):
            eng.extend_score(prefix, [(empty, empty)])
        with pytest.raises(ValueError, match="image token"):
            eng.extend_score(prefix, [(torch.tensor([[5, cfg.image_token_index]]), torch.tensor([[1, 2]]))])
        with pytest.raises(ValueError, match="empty"):
            eng.extend_score(KVCache(cfg, 16, DTYPE, "cpu"), ext)
        for fn in (lambda a: eng.extend_score(prefix, ext, attention=a), lambda a: eng.extend(prefix, [ext[0][0]], attention=a),
                   lambda a: eng.score_shared(head, u8, reqs, attention=a)):
            with pytest.raises(ValueError, match="attention"):
                fn("bogus")
        with pytest.raises(ValueError, match="empty continuation"):
            eng.score_shared(head, u8, [(reqs[0][0], empty)])
        with pytest.raises(ValueError, match="empty tail"):
            eng.score_shared(head, u8, [(empty, reqs[0][1])], prefix=prefix)
        with pytest.raises(ValueError, match="text token"):
            eng.score_shared(torch.tensor([[5, cfg.image_token_index]]), u8, [(empty, reqs[0][1])])
        with pytest.raises(ValueError, match="prefix is empty"):
            eng.score_shared(empty, u8, reqs)
        with pytest.raises(ValueError, match="image token"):
            eng.score_shared(head, u8, [(torch.tensor([[cfg.image_token_index]]), reqs[0][1])])
        with pytest.raises(ValueError, match="targets"):
            eng.score_shared(head, u8, [(reqs[0][0], torch.tensor([[V + 3]]))])
        # attention="rows": under lo4 every suffix must be corrected whole; a model with another head ratio is refused by name
        eng.precision = "lo4"
        eng.lo4_rows = 2
        with pytest.raises(NotImplementedError, match="LO4_FULL_BELOW"):
            eng.extend_score(prefix, ext, attention="rows")
        with pytest.raises(NotImplementedError, match="LO4_FULL_BELOW"):
            eng.extend(prefix, [ext[0][0]], attention="rows")
        eng.lo4_rows = "auto"
        eng.precision = "fast"
        eng.split_operands = True
        with pytest.raises(NotImplementedError, match="split"):
            eng.extend_score(prefix, ext)
        with pytest.raises(NotImplementedError, match="split"):
            eng.score_shared(head, u8, reqs)
        eng.split_operands = False
        eng._fp8 = object()
        with pytest.raises(NotImplementedError, match="fp8"):
            eng.extend_score(prefix, ext)
        eng._fp8 = None
        eng.W.tp_size = 2
        with pytest.raises(NotImplementedError, match="tensor-parallel"):
            eng.score_shared(head, u8, reqs)
        eng.W.tp_size = 1
        cfg.text_config.sliding_window = 16
        with pytest.raises(NotImplementedError, match="sliding_window"):
            eng.extend_score(prefix, ext)
        cfg.text_config.sliding_window = 0
        assert not launches
        _, eng2, u8b, _, ids2, _ = _engine_setup(ops, DTYPE, hidden=256, heads=2)
        launches.clear()
        with pytest.raises(NotImplementedError, match="ratio must be 4"):
            eng2.score_shared(ids2[:, :-48], u8b, reqs, attention="rows")
        assert not launches
    finally:
        ops._check = check
        eng.precision = "fast"
        eng.lo4_rows = "auto"
        eng.split_operands = False
        eng._fp8 = None
        eng.W.tp_size = 1
        cfg.text_config.sliding_window = 0


def test_extend_without_the_new_argument_keeps_its_bits(micro):
    """extend(...) as before == extend(..., attention="ranges"), bit for bit, on the suffixes of tests/test_emu_prefix.py's fan-out case (the
    default is the two-range launch: nothing existing changes); "rows" gives the same logits within extend's bound."""
    cfg, eng, u8, ids = micro
    head, tail = ids[:, :-48], ids[:, -48:]
    prefix = _prefilled(eng, cfg, head, u8, DTYPE)
    sfx = [tail, tail[:, :5], torch.tensor([[9, 8, 7, 6, 5, 4, 3, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20]])]
    was = eng.extend(prefix, sfx).logits
    assert torch.equal(was, eng.extend(prefix, sfx, attention="ranges").logits)
    rows = eng.extend(prefix, sfx, attention="rows").logits
    err = (rows - was).abs().max().item()
    print(f"extend: rows vs ranges max|logit diff| {err:.3e} (bound {BOUND:.1e})")
    assert err <= BOUND


def test_loglikelihood_share_prefix_groups_and_keeps_the_order(ops, micro):
    """loglikelihood(share_prefix=True): consecutive requests with the same pixel_values object share one prefill; the results come back in
    request order and agree with share_prefix=False within the bound; a group whose tail would hold an image token, and a group of one,
    take today's path: equal to share_prefix=False exactly."""
    from leopard_amd import compat
    from leopard_amd.weights import SynthSource
    cfg, eng, u8, ids = micro
    m = compat.LeopardForConditionalGeneration(cfg, lambda dev, dt: SynthSource(cfg, ops, dev, dt), DTYPE, ops, torch_dtype=DTYPE, precision="fast")
    m._engine, m.device = eng, torch.device("cpu")
    head, reqs = requests_of(ids)
    u8b = u8.clone()
    group = [(torch.cat([head, t], dim=1), c, u8) for t, c in reqs[:3]]
    img_pos = int((ids[0] == cfg.image_token_index).nonzero()[0])
    # the two contexts differ before their image tokens: every tail would hold them
    early = [(torch.cat([torch.tensor([[7 + j]]), ids[:, :-40]], dim=1), reqs[j][1], u8b) for j in range(2)]
    assert img_pos < ids.shape[1] - 40
    single = [(torch.cat([head, reqs[3][0]], dim=1), reqs[3][1], u8.clone())]
    allreq = group + early + single
    towers = []
    enc = eng.encode_images
    eng.encode_images = lambda *a, **k: (towers.append(1), enc(*a, **k))[1]
    try:
        shared = m.loglikelihood(allreq, share_prefix=True)
        n_shared = len(towers)
        plain = m.loglikelihood(allreq)
        assert m.loglikelihood(allreq, share_prefix=False) == plain
    finally:
        eng.encode_images = enc
    assert n_shared == 3                                           # one prefill for the group of three, one packed pass per other group
    assert len(shared) == len(allreq)
    for j in range(3):
        print(f"request {j}: shared {shared[j][0]:.5f} plain {plain[j][0]:.5f}")
        assert abs(shared[j][0] - plain[j][0]) <= BOUND * reqs[j][1].numel()
    assert shared[3:] == plain[3:]
    direct = m.loglikelihood_shared(head, u8, reqs[:3])
    assert direct == shared[:3]
    head2, tails = compat.shared_context_split([g[0] for g in group], cfg.image_token_index)
    assert head2.shape[1] == head.shape[1] and [t.numel() for t in tails] == [1, 3, 2]
