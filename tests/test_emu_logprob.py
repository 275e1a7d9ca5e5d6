"""Scoring on the CPU: lmi_token_logprobs through the kernel-logic emulator against float64, and LeopardEngine.score / score_batch
(label mapping, the shift, the ignore index) on a micro configuration against a float64 restatement of EVAL:333-348 over merged rows."""
import numpy as np
import pytest
import torch

from leopard_amd.config import LeopardConfig, RopeScaling, TextConfig, VisionConfig
from leopard_amd.engine import LeopardEngine
from leopard_amd.ops import Ops
from leopard_amd.weights import EngineWeights, SynthSource
from tests.emu_util import emu_ops


@pytest.fixture(scope="module")
def ops():
    return emu_ops()


def run_kernel(ops, x, V, targets, rows=None):
    n = targets.numel()
    lp, lse, am = torch.empty(n), torch.empty(n), torch.empty(n, dtype=torch.int64)
    ops.token_logprobs(x, V, targets, lp, lse, am, rows=rows)
    return lp, lse, am


def check_against_f64(x, V, targets, lp, lse, am, rows=None):
    d = (x if rows is None else x[rows])[:, :V].double()
    rl = torch.logsumexp(d, dim=-1)
    assert ((lse.double() - rl).abs() <= 1e-5 * rl.abs().clamp_min(1.0)).all(), (lse, rl)
    rp = d.gather(1, targets.reshape(-1, 1))[:, 0] - rl
    assert ((lp.double() - rp).abs() <= 1e-5 * rl.abs().clamp_min(1.0)).all()
    assert torch.equal(am, d.argmax(dim=-1))                          # torch: first occurrence of the maximum = the lowest index


@pytest.mark.parametrize("V", [8192, 32000, 128256])
@pytest.mark.parametrize("R,scale", [(1, 3e4), (300, 4.0), (7, 3e4)])
def test_token_logprobs_vs_float64(ops, V, R, scale):
    ld = V + 128                                                      # the head's padding: never read
    g = torch.Generator().manual_seed(V + R)
    x = torch.full((R, ld), 1e30)
    x[:, :V] = (torch.rand(R, V, generator=g) * 2 - 1) * scale
    t = torch.randint(0, V, (R,), generator=g)
    t[0] = 0
    t[-1] = V - 1
    if R > 2:
        x[1, 5] = x[1, V - 3] = x[1, 77] = float(scale) * 1.5        # tied maxima: the lowest index wins
        t[1] = 77
    lp, lse, am = run_kernel(ops, x, V, t)
    check_against_f64(x, V, t, lp, lse, am)
    if R > 2:
        assert int(am[1]) == 5
    # bit-identical reruns
    lp2, lse2, am2 = run_kernel(ops, x, V, t)
    assert torch.equal(lp, lp2) and torch.equal(lse, lse2) and torch.equal(am, am2)


def test_token_logprobs_row_index_and_odd_vocab(ops):
    V, ld = 1001, 1008                                                # V % 4 != 0: the scalar tail
    g = torch.Generator().manual_seed(5)
    x = torch.full((40, ld), 1e30)
    x[:, :V] = torch.randn(40, V, generator=g) * 3
    x[3, 1000] = 50.0                                                 # the maximum in the tail
    rows = torch.tensor([3, 0, 39, 3, 17])
    t = torch.tensor([1000, 0, 999, 4, 500])
    lp, lse, am = run_kernel(ops, x, V, t, rows=rows)
    check_against_f64(x, V, t, lp, lse, am, rows=rows)
    assert int(am[0]) == 1000 and torch.equal(lse[0], lse[3])          # the same source row twice: the same bits


def test_token_logprobs_bad_target_is_nan_and_arguments_checked(ops):
    x = torch.randn(2, 64)
    lp, lse, am = run_kernel(ops, x, 60, torch.tensor([-1, 60]))
    assert torch.isnan(lp).all() and torch.isfinite(lse).all()
    with pytest.raises(RuntimeError, match="lmi_token_logprobs"):
        run_kernel(ops, torch.randn(2, 63), 60, torch.tensor([0, 1]))  # ld % 4 != 0
    with pytest.raises(RuntimeError, match="lmi_token_logprobs"):
        run_kernel(ops, x, 65, torch.tensor([0, 1]))                   # vocab > ld


# ---- the engine ----------------------------------------------------------------------------------------------------------------------
def score_config():
    """Full ViT width (the kernels' shape rules), 1 + 2 layers, 56-pixel tiles: 4 visual rows per <image> token."""
    return LeopardConfig(
        vision_config=VisionConfig(hidden_size=1152, intermediate_size=100, num_hidden_layers=1, num_attention_heads=16,
                                   image_size=56, patch_size=14),
        text_config=TextConfig(hidden_size=128, intermediate_size=128, num_hidden_layers=2, num_attention_heads=1,
                               num_key_value_heads=1, vocab_size=256, rope_scaling=RopeScaling()),
        image_token_index=250)


@pytest.fixture(scope="module")
def engine(ops):
    cfg = score_config()
    assert cfg.tokens_per_tile == 4
    W = EngineWeights.build(cfg, SynthSource(cfg, ops, "cpu", torch.float16), torch.float16)
    return LeopardEngine(cfg, W, ops=ops, device="cpu")


def tiles(n, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (n, 56, 56, 3), dtype=np.uint8))


def reference_loss(logits: torch.Tensor, ids, labels, image_token_index: int, tpt: int):
    """EVAL:335-348 restated in float64 over the merged rows, with transformers-4.38's merge of the labels (a visual row is labelled -100,
    a text label moves with its token)."""
    merged = []
    for i, l in zip(ids, labels):
        merged += [-100] * tpt if i == image_token_index else [int(l)]
    merged = torch.tensor(merged)
    shift_logits, shift_labels = logits[:-1].double(), merged[1:]
    loss = torch.nn.functional.cross_entropy(shift_logits, shift_labels, ignore_index=-100)
    rows = torch.nonzero(shift_labels != -100)[:, 0]
    lp = torch.log_softmax(shift_logits, dim=-1)[rows, shift_labels[rows]]
    return loss, rows, shift_labels[rows], lp


# (every sequence longer than 32 rows: lmi_rmsnorm takes its few-rows kernel below that, so a short request alone and packed would differ)
TAIL = list(range(60, 80))
IDS = [5, 250, 9, 11, 250, 250, 17, 33, 40] + TAIL
LABELS = [-100, 250, 9, 11, 7, 250, 17, 33, 40] + [-100] * 10 + TAIL[10:]   # spans across the image tokens (their labels are dropped by the merge)


def test_score_matches_reference_semantics(engine):
    ids, lab = torch.tensor([IDS]), torch.tensor([LABELS])
    u8 = tiles(3, 1)
    all_logits = engine.prefill(ids, u8, all_logits=True).logits_all
    loss, rows, tgt, lp = reference_loss(all_logits, IDS, LABELS, 250, 4)
    res = engine.score(ids, u8, lab)
    assert res.seq_len == all_logits.shape[0] == len(IDS) + 3 * 3
    assert torch.equal(res.rows, rows) and torch.equal(res.target_ids, tgt)
    assert (res.token_logprobs.double() - lp).abs().max() <= 2e-5
    assert torch.equal(res.argmax, all_logits[rows].argmax(dim=-1))
    assert abs(float(res.loss) - float(loss)) <= 2e-5 and res.loss.dtype == torch.float32 and res.loss.dim() == 0
    # the row after an image span predicts the text token that follows it; the rows of the span predict nothing but its last one
    assert 1 + 4 - 1 in rows.tolist() and all(r not in rows.tolist() for r in (1, 2, 3))


def test_score_batch_equals_score(engine):
    text = list(range(3, 40))
    reqs = [(torch.tensor([IDS]), tiles(3, 1), torch.tensor([LABELS])),
            (torch.tensor([text]), None, torch.tensor([[-100] * 30 + text[30:]])),
            (torch.tensor([[250, 250, 250] + TAIL]), tiles(3, 2), torch.tensor([[-100, -100, -100] + TAIL]))]
    batch = engine.score_batch(reqs)
    for r, b in zip(reqs, batch):
        s = engine.score(*r)
        assert s.seq_len == b.seq_len and torch.equal(s.rows, b.rows) and torch.equal(s.target_ids, b.target_ids)
        assert torch.equal(s.token_logprobs, b.token_logprobs) and torch.equal(s.argmax, b.argmax) and torch.equal(s.loss, b.loss)


def test_score_chunking_is_bit_equal(engine):
    ids, lab, u8 = torch.tensor([IDS]), torch.tensor([[-100] * 25 + IDS[25:]]), tiles(3, 1)
    full = engine.score(ids, u8, lab)
    engine.score_chunk_rows = 3
    try:
        chunked = engine.score(ids, u8, lab)
    finally:
        engine.score_chunk_rows = 1024
    assert len(full.rows) == 4 and torch.equal(full.token_logprobs, chunked.token_logprobs) and torch.equal(full.argmax, chunked.argmax)


class _NoLaunch:
    """A library whose every entry point fails the test: nothing may be launched."""
    def __getattr__(self, name):
        raise AssertionError(f"{name} was launched")


def test_all_ignored_is_nan_without_a_launch(engine):
    real = engine.ops
    engine.ops = Ops(lib=_NoLaunch(), emulated=True)
    try:
        res = engine.score(torch.tensor([IDS]), tiles(3, 1), torch.full((1, len(IDS)), -100))
        only_image = engine.score(torch.tensor([IDS]), tiles(3, 1), torch.tensor([[9] + [-100] * (len(IDS) - 1)]))
    finally:
        engine.ops = real
    assert torch.isnan(res.loss) and res.token_logprobs.numel() == 0 and res.seq_len == len(IDS) + 9
    assert torch.isnan(only_image.loss)                               # the label of the first token is never a target (the shift)


@pytest.mark.parametrize("labels,match", [([[0] * 8], "shape"), ([[-100, 256] + [0] * (len(IDS) - 2)], r"\[0, 256\)"),
                                          ([[-100, -1] + [0] * (len(IDS) - 2)], "-100"), (None, "labels")])
def test_bad_labels_raise_before_launch(engine, labels, match):
    real = engine.ops
    engine.ops = Ops(lib=_NoLaunch(), emulated=True)
    try:
        with pytest.raises(ValueError, match=match):
            engine.score(torch.tensor([IDS]), tiles(3, 1), None if labels is None else torch.tensor(labels))
        with pytest.raises(ValueError, match=match):
            engine.score_batch([(torch.tensor([[1, 2]]), None, torch.tensor([[1, 2]])),
                                (torch.tensor([IDS]), tiles(3, 1), None if labels is None else torch.tensor(labels))])
    finally:
        engine.ops = real


def test_lo4_selection_unites_the_scored_rows(engine):
    """The host side of the row selection: tails of lo4_rows "auto" plus the scored rows; a cache key per set of extra rows."""
    eng = engine
    lens = [1100, 300, 2000]
    base = eng._lo4_selection(lens)
    assert base is not None and base[2].tolist() == [[1084, 1400], [3384, 3400]]
    extra = np.array([5, 6, 7, 1090, 1500, 3000], dtype=np.int64)
    row, unit, ranges = eng._lo4_selection(lens, extra)
    want = base[0].numpy().copy()
    want[extra] = 1
    assert np.array_equal(row.numpy(), want)
    assert ranges.tolist() == [[5, 8], [1084, 1400], [1500, 1501], [3000, 3001], [3384, 3400]]
    assert np.array_equal(unit.numpy(), np.pad(want, (0, -len(want) % 64)).reshape(-1, 64).max(axis=1))
    other = eng._lo4_selection(lens, extra[:-1])
    assert other[2].tolist() != ranges.tolist()                       # a different set of rows is a different cache entry
    assert eng._lo4_selection([1100], np.arange(1084, dtype=np.int64)) is None        # every row selected: the plain pass
    assert eng._lo4_selection([900], extra[:3]) is None              # <= LO4_FULL_BELOW rows: every row, as without scoring
