"""tests/logits_rules_ref.apply — the restatement lmi_decode_rules is held to bit for bit — against transformers' own logits processors,
chained in HF's order (repetition penalty, no-repeat n-gram, minimum new tokens), on random rows and sequences, bit for bit.  Touches
neither the package nor the kernel."""
import pytest
import torch

from tests import logits_rules_ref as R

pytest.importorskip("transformers")
from transformers.generation.logits_process import (MinNewTokensLengthLogitsProcessor, NoRepeatNGramLogitsProcessor,  # noqa: E402
                                                    RepetitionPenaltyLogitsProcessor)

V = 97


def hf_chain(row, seq, penalty, n, prompt_len, min_new, eos):
    ids, scores = torch.tensor([seq], dtype=torch.long), row.clone().reshape(1, -1)
    if penalty != 1.0:
        scores = RepetitionPenaltyLogitsProcessor(penalty)(ids, scores)
    if n > 0:
        scores = NoRepeatNGramLogitsProcessor(n)(ids, scores)
    if min_new > 0:
        scores = MinNewTokensLengthLogitsProcessor(prompt_len, min_new, list(eos))(ids, scores)
    return scores[0]


@pytest.mark.parametrize("seed", range(6))
def test_apply_equals_the_hf_processors(seed):
    g = torch.Generator().manual_seed(seed)
    for L in (1, 2, 5, 40, 300):
        for penalty in (1.0, 0.7, 1.3, 2.0):
            for n in (0, 1, 2, 3, L + 2):
                row = torch.randn(V, generator=g) * 4
                row[torch.randint(0, V, (6,), generator=g)] = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), -2.5, 1e-30])
                pool = torch.randint(0, V, (int(L ** 0.5) + 2,), generator=g)           # heavy duplicates
                seq = pool[torch.randint(0, pool.numel(), (L,), generator=g)].tolist()
                prompt_len = int(torch.randint(0, L + 1, (1,), generator=g))
                for min_new in (0, L - prompt_len, L - prompt_len + 1, L - prompt_len + 3):
                    eos = (3, 11)
                    want = hf_chain(row, seq, penalty, n, prompt_len, min_new, eos)
                    min_left = max(min_new - (L - prompt_len), 0)                        # the countdown the kernel keeps: eos banned while > 0
                    got = R.apply(row, seq, penalty, n, min_left, eos)
                    assert R.same_bits(got, want), (L, penalty, n, min_new, seq[:8])


def test_the_pinned_ngram_cases():
    row = torch.zeros(16)
    ban = lambda seq, n: set((hf_chain(row, seq, 1.0, n, 0, 0, ()) == float("-inf")).nonzero().reshape(-1).tolist())
    s = [3, 5, 3, 7, 3, 5]
    assert ban(s, 1) == {3, 5, 7} and ban(s, 2) == {3} and ban(s, 3) == {3} and ban([4, 4, 4, 4], 3) == {4} and ban(s, 8) == set()
    for seq, n in ((s, 1), (s, 2), (s, 3), ([4, 4, 4, 4], 3), (s, 8), (s, 7)):
        assert set((R.apply(row, seq, 1.0, n, 0, ()) == float("-inf")).nonzero().reshape(-1).tolist()) == ban(seq, n)
