"""Beam search, the host side: everything transformers' ``_beam_search`` does AFTER candidate selection, restated on walk lists.

A walk list is what lmi_beam_step's select launch leaves for one step (and what ``walk_of`` builds on the CPU from whole rows): the
candidates of the step in the order total descending, beam ascending, id ascending, each with its rank, up to and including the one that
fills the last of the K next beams.  The non-eos entries ARE the next beams, in order; an entry that stops — an eos id, or any entry of
the step that reaches ``max_new_tokens`` — becomes a finished hypothesis when its rank is below K.

``BeamSearch`` follows transformers 5.x (``_get_running_beams_for_next_iteration``, ``_update_finished_beams``,
``_check_early_stop_heuristic``, ``_beam_search_has_unfinished_sequences``), including its fp32 arithmetic: a hypothesis' score is the fp32
total divided by ``generated_length ** length_penalty``, compared in fp32.  The -1e9 offsets transformers adds to keep unfinished entries
out of its static-shaped top-k are not restated: a finished list that is shorter than K says the same.  What is ours rather than HF's is
the order among EXACT ties of the total (torch.topk leaves it open): beam ascending, then id ascending.
"""
from __future__ import annotations

from typing import List, NamedTuple, Sequence, Tuple

import numpy as np
import torch

WALK_ENTRY = 5                         # LMI_BEAM_WALK_ENTRY: rank, total (fp32 bits), parent, id, is_eos


class Cand(NamedTuple):
    rank: int
    total: float
    parent: int
    id: int
    is_eos: bool


def decode_walk(words: np.ndarray) -> List[Cand]:
    """The walk buffer of lmi_beam_step (int32 words: n, then 5 per entry) as a list of ``Cand``."""
    words = np.ascontiguousarray(words, dtype=np.int32)
    n = int(words[0])
    body = words[1:1 + n * WALK_ENTRY].reshape(n, WALK_ENTRY)
    totals = body[:, 1].copy().view(np.float32)
    return [Cand(int(r[0]), float(t), int(r[2]), int(r[3]), bool(r[4])) for r, t in zip(body, totals)]


def walk_of(lp: np.ndarray, scores: Sequence[float], num_beams: int, eos: Sequence[int] = (), suppress: Sequence[int] = ()) -> List[Cand]:
    """The walk list of one step from WHOLE rows, on the CPU: ``lp`` [n_rows, V] holds logit - lse of every id, ``scores`` the rows'
    accumulated log-probabilities; total = score + lp in lp's dtype (float32 reproduces the kernel's and transformers' one fp32 add,
    float64 is the reference).  Every one of the n_rows x V candidates is ranked — nothing here relies on a row's best K — in the order
    total descending, beam ascending, id ascending; NaN totals never enter; a suppressed id is never a candidate, a suppressed eos id is
    one at -inf.  The walk ends with the candidate that fills beam ``num_beams`` - 1."""
    lp = np.asarray(lp)
    n_rows, V = lp.shape
    eos_ids = sorted(set(int(e) for e in eos if 0 <= int(e) < V))
    sup = set(int(s) for s in suppress)
    total = np.asarray(scores, dtype=lp.dtype).reshape(n_rows, 1) + lp
    is_eos = np.zeros(V, dtype=bool)
    is_eos[eos_ids] = True
    for s in sup:
        if 0 <= s < V:
            total[:, s] = -np.inf if is_eos[s] else np.nan
    flat = total.reshape(-1)
    live = np.flatnonzero(~np.isnan(flat))
    order = live[np.argsort(-flat[live], kind="stable")]           # flat index = beam * V + id: a stable sort keeps beam, then id, ascending
    out, filled = [], 0
    for r, c in enumerate(order.tolist()):
        b, i = divmod(c, V)
        out.append(Cand(r, float(flat[c]), b, i, bool(is_eos[i])))
        filled += 0 if is_eos[i] else 1
        if filled == num_beams:
            break
    return out


def _f32_div(x: float, d: float) -> float:
    """fp32 x / d as torch computes ``tensor_f32 / python_float`` (what transformers does to a finished hypothesis' total)."""
    return float(torch.tensor([x], dtype=torch.float32) / d)


class BeamSearch:
    """One beam search over walk lists.  ``step(walk)`` consumes the walk of one generated position and says whether the search goes on;
    ``beams`` are then the K running hypotheses (generated ids) and ``parents`` the beam each descends from; ``results()`` the finished
    hypotheses, best first."""

    def __init__(self, num_beams: int, max_new_tokens: int, length_penalty: float = 1.0, early_stopping=False, num_return_sequences: int = 1):
        if early_stopping not in (False, True, "never"):
            raise ValueError(f"early_stopping must be False, True or 'never', got {early_stopping!r}")
        if not 1 <= num_return_sequences <= num_beams:
            raise ValueError(f"num_return_sequences must be in [1, num_beams = {num_beams}], got {num_return_sequences}")
        if max_new_tokens < 1:
            raise ValueError(f"max_new_tokens must be at least 1, got {max_new_tokens}")
        self.K, self.max_new, self.length_penalty, self.early_stopping = int(num_beams), int(max_new_tokens), float(length_penalty), early_stopping
        self.n_return = int(num_return_sequences)
        self.beams: List[List[int]] = [[]]                            # before the first step: the prompt alone
        self.scores: List[float] = [0.0]
        self.parents: List[int] = [0]
        self.finished: List[Tuple[float, List[int]]] = []             # (length-penalised fp32 score, generated ids), best first, at most K
        self.generated = 0
        self.unsatisfied = True                                       # transformers' is_early_stop_heuristic_unsatisfied
        self.done = False

    def step(self, walk: Sequence[Cand]) -> bool:
        """Consume one walk list.  Returns True while another decode step is needed."""
        assert not self.done
        K = self.K
        self.generated += 1
        g = self.generated
        last = g >= self.max_new                                      # the length criterion: every candidate of this step stops
        full = len(self.finished) == K and self.early_stopping is True
        new_beams, new_scores, new_parents, just = [], [], [], []
        for c in walk:
            seq = self.beams[c.parent] + [c.id]
            if c.is_eos or last:
                if c.rank < K and not full:
                    just.append((_f32_div(c.total, g ** self.length_penalty), seq))
            elif len(new_beams) < K:
                new_beams.append(seq); new_scores.append(c.total); new_parents.append(c.parent)
        # keep the best K of (finished so far, then the ones that just finished): stable, so an equal score keeps the earlier one
        self.finished = sorted(self.finished + just, key=lambda h: -h[0])[:K]
        self.beams, self.scores, self.parents = new_beams, new_scores, new_parents
        if len(self.finished) == K and new_scores:
            if self.early_stopping == "never" and self.length_penalty > 0.0:
                best_len = self.max_new
            else:
                best_len = g
            best = _f32_div(new_scores[0], best_len ** self.length_penalty)
            self.unsatisfied = self.unsatisfied and best > self.finished[-1][0]
        go_on = self.unsatisfied and not (len(self.finished) == K and self.early_stopping is True) and not last and len(new_beams) > 0
        self.done = not go_on
        return go_on

    def results(self) -> List[Tuple[float, List[int]]]:
        """The ``num_return_sequences`` best finished hypotheses, best first.  Every search ends with K of them: the step that reaches
        ``max_new_tokens`` finishes its K best candidates, and no other stop condition holds before K have finished."""
        return self.finished[:self.n_return]
