"""Pins tests/sampling_ext_ref.kept_set_ext — the float64 restatement lmi_decode_sample_ex is tested against — to transformers' own
MinPLogitsWarper, TypicalLogitsWarper, EpsilonLogitsWarper and EtaLogitsWarper, chained after Temperature, TopK and TopP in the order of
``generate(do_sample=True)``.  CPU only; skipped where transformers is not installed."""
import math

import pytest
import torch

from tests.row_kernels_ref import HEAD, gapped_row
from tests.sampling_ext_ref import BROAD_CASES, GAPPED_CASES, MIN_MARGIN, TIE_CASES, broad_row, kept_set_ext, tie_row

lp = pytest.importorskip("transformers.generation.logits_process")


def hf_kept(row: torch.Tensor, vocab: int, T=1.0, k=0, p=1.0, min_p=0.0, typ=1.0, eps=0.0, eta=0.0) -> set:
    """The ids HF leaves finite: the temperature division in fp32 (as the kernel's), everything after it in float64."""
    chain = []
    if k > 0:
        chain.append(lp.TopKLogitsWarper(top_k=k))
    if p < 1.0:
        chain.append(lp.TopPLogitsWarper(top_p=float(torch.tensor(p, dtype=torch.float32))))
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))       # the kernel's parameters are fp32
    if min_p > 0:
        chain.append(lp.MinPLogitsWarper(min_p=f32(min_p)))
    if typ < 1.0:
        chain.append(lp.TypicalLogitsWarper(mass=f32(typ)))
    if eps > 0:
        chain.append(lp.EpsilonLogitsWarper(epsilon=f32(eps)))
    if eta > 0:
        chain.append(lp.EtaLogitsWarper(epsilon=f32(eta)))
    scores = lp.TemperatureLogitsWarper(float(T))(None, row[:vocab].float().reshape(1, -1)) if T != 1.0 else row[:vocab].float().reshape(1, -1)
    scores = scores.double()
    for w in chain:
        scores = w(None, scores)
    return set(torch.nonzero(torch.isfinite(scores[0])).flatten().tolist())


def _check(row, vocab, c):
    kept, margin, notes = kept_set_ext(row, vocab, **c)
    assert margin >= MIN_MARGIN, (c, margin)                          # a condition on the inputs, not a tolerance
    assert set(kept) == hf_kept(row, vocab, **c), c
    return kept, notes


@pytest.mark.parametrize("V", [1000, 32000, 128256])
def test_gapped_rows_match_transformers(V):
    row = gapped_row(V, HEAD, seed=1)
    sizes = {len(_check(row, V, c)[0]) for c in GAPPED_CASES}
    assert len(GAPPED_CASES) == 19 and len(sizes) > 4                # the cases do cut at different places


def test_broad_row_matches_transformers_and_typical_removes_the_top_token():
    row = broad_row()
    removed = 0
    for c in BROAD_CASES:
        kept, notes = _check(row, row.numel(), c)
        removed += bool(notes.get("top_removed"))
        if notes.get("top_removed"):
            assert int(row.argmax()) not in kept
    assert len(BROAD_CASES) == 5 and removed >= 3


def test_tie_groups_on_the_boundaries_are_kept_whole():
    row = tie_row()
    seen = set()
    for c in TIE_CASES:
        kept, notes = _check(row, row.numel(), c)
        for key in ("typ_group", "eps_group", "eta_group"):
            if key in notes:
                assert notes[key] >= 2, (c, notes)                    # the boundary is a tie group, and the float64 set has all of it
                seen.add(key)
        levels = {float(row[i]) for i in kept}
        assert all(int((row == v).sum()) == sum(float(row[i]) == v for i in kept) for v in levels) or c["p"] < 1.0, c
    assert seen == {"typ_group", "eps_group", "eta_group"}


def test_edges_keep_what_hf_keeps():
    row = gapped_row(1000, HEAD, seed=1)
    top = int(row[:1000].argmax())
    assert kept_set_ext(row, 1000, min_p=1.0)[0] == [top]
    assert kept_set_ext(row, 1000, eps=0.99)[0] == [top]             # nothing has p >= 0.99: the top token stays
    assert kept_set_ext(row, 1000, eta=0.99)[0][0] == top             # (eta = min(h, sqrt(h) exp(-H)) is far below h here)
    kept, margin, notes = kept_set_ext(row, 1000, typ=1e-6)
    assert len(kept) == 1 and margin >= MIN_MARGIN                    # the token closest to the entropy, which need not be the top one
    assert kept_set_ext(row, 1000)[1] == math.inf                     # nothing on: no threshold, and the set is lmi_decode_sample's
