"""The host side of the generation calls that a launch trace does not see, on the CPU emulator (the micro configuration of
tests/test_emu_gen_logprobs.py): how often the logprob rings are copied to the host — per step for the batch-1 loop, once per HIST steps for
the pooled loops; a loop that drained per step would keep every output and every launch and still slow the step — and the sequential
continuation of shapes without a batched decode against the batched path."""
import pytest
import torch

from tests.emu_util import emu_ops
from tests.test_emu_gen_logprobs import SP, requests_of


@pytest.fixture(scope="module")
def micro():
    from tests.test_emu_shared_decode import _engine_setup
    cfg, eng, u8, ids = _engine_setup(emu_ops(), torch.float16)
    assert eng._batch_decode_supported()
    return eng, u8, ids


def text_requests(ids, u8):
    return requests_of(ids, u8)[1:]                                      # (the emulated vision tower is the slow part of a request)


def ring_reads(eng, monkeypatch, fn) -> int:
    """Calls of _rings_to_host during fn()."""
    calls = []
    real = eng._rings_to_host
    with monkeypatch.context() as m:
        m.setattr(eng, "_rings_to_host", lambda st: (calls.append(1), real(st))[1])
        fn()
    return len(calls)


def test_ring_reads_per_call(micro, monkeypatch):
    eng, u8, ids = micro
    reqs = text_requests(ids, u8)
    counted = lambda fn: ring_reads(eng, monkeypatch, fn)
    T = 6                                                               # batch-1 loop: the ring of one slot is read with every step's token
    assert counted(lambda: eng.generate(reqs[0][0], None, max_new_tokens=T, eos_token_id=(), sampling=SP, logprobs=2)) == T - 1
    assert counted(lambda: eng.generate(reqs[0][0], None, max_new_tokens=T, eos_token_id=())) == 0
    H = eng.HIST
    assert H == 8                                                       # 11 tokens = 10 steps: drained when full and once at the end
    assert counted(lambda: eng.generate_batch(reqs[:3], max_new_tokens=11, eos_token_id=(), sampling=SP, logprobs=3)) == -(-10 // H) == 2
    stats = {}                                                          # continuous batching: one read per window of HIST steps
    n = counted(lambda: eng.generate_stream(reqs, batch_size=2, max_new_tokens=9, eos_token_id=(), stats=stats, logprobs=1))
    assert stats["steps"] % H == 0 and stats["steps"] >= 2 * H and n == stats["steps"] // H
    head, sfx = reqs[3][0], [ids[:, -48:-20], torch.tensor([[9, 8, 7, 6, 5]])]
    for decode in ("copy", "shared"):
        assert counted(lambda: eng.generate_shared(head, None, sfx, max_new_tokens=11, eos_token_id=(), decode=decode, logprobs=2)) == 2


# Both paths hand lmi_decode_logprobs the logits row the token was chosen from, but not the same row: the pooled step's projections are
# lmi_gemm_skinny tiles over B rows, the batch-1 step's run one row (another summation order in 16-bit operands).  log-softmax moves by at
# most twice the largest change of a logit, so a value may differ by 2 * max_i |logit_i(sequential) - logit_i(batched)| of its own step,
# plus the kernel's own evaluation error: the 1e-5 that tests/test_emu_gen_logprobs.py holds lmi_decode_logprobs to against float64 (the
# only tolerance that file has; the form of the bound is that of tests/test_gpu_gen_logprobs.py between the prefill's and the step's row)
KERNEL_TOL = 1e-5


def step_rows(eng, monkeypatch, fn):
    """(what fn() returned, the [B, vocab] logits of every decode step it ran, in order)."""
    rows = []
    real, V = eng._choose, eng.cfg.text_config.vocab_size
    with monkeypatch.context() as m:
        m.setattr(eng, "_choose", lambda st, logits, **kw: (rows.append(logits[:, :V].clone()), real(st, logits, **kw))[1])
        return fn(), rows


def same_outputs(seq, bat, change):
    """``seq`` / ``bat``: GenerateOutputs of the sequential and the batched path; change[j][t]: the largest logit change of request j's
    step t (token t + 1; token 0 comes from the one prefill both share)."""
    assert len(seq.sequences) == len(bat.sequences) == len(change)
    for j, (s, t) in enumerate(zip(seq.sequences, bat.sequences)):
        assert torch.equal(s, t), (j, s.tolist(), t.tolist())
        assert torch.equal(seq.top_ids[j], bat.top_ids[j])
        bound = 2 * torch.tensor([0.0] + change[j], dtype=torch.float64) + KERNEL_TOL
        gap = (seq.token_logprobs[j].double() - bat.token_logprobs[j].double()).abs()
        top = (seq.top_logprobs[j].double() - bat.top_logprobs[j].double()).abs().max(dim=1).values
        print(f"[sequential vs batched] request {j}: largest |token logprob gap| {gap.max():.3e}, |top logprob gap| {top.max():.3e}, "
              f"largest logit change {max(change[j]):.3e}")
        assert gap[0] == 0 and top[0] == 0                              # the first token's row: one prefill, one eager launch
        assert (gap <= bound).all() and (top <= bound).all(), (gap, top, bound)


def test_sequential_fallback_gives_the_batched_result(micro, monkeypatch):
    """Shapes without a batched decode continue the requests one after another on the generation cache: the same sampled requests give the
    sequences and the logprob rows of the batched path."""
    eng, u8, ids = micro
    reqs = text_requests(ids, u8)[:3]
    head, sfx = text_requests(ids, u8)[3][0], [ids[:, -48:], ids[:, -48:-20], torch.tensor([[9, 8, 7, 6, 5]])]
    calls = {"generate_batch": (11, lambda: eng.generate_batch(reqs, max_new_tokens=11, eos_token_id=(), sampling=SP, logprobs=3)),
             "generate_shared": (6, lambda: eng.generate_shared(head, None, sfx, max_new_tokens=6, eos_token_id=(), sampling=SP, logprobs=3))}
    for name, (T, call) in calls.items():
        bat, bat_rows = step_rows(eng, monkeypatch, call)
        assert [tuple(r.shape[:1]) for r in bat_rows] == [(3,)] * (T - 1)                   # T - 1 steps of the three slots together
        with monkeypatch.context() as m:
            m.setattr(eng, "_batch_decode_supported", lambda: False)
            seq, seq_rows = step_rows(eng, monkeypatch, call)
        assert [tuple(r.shape[:1]) for r in seq_rows] == [(1,)] * (3 * (T - 1))             # request after request on the batch-1 step
        change = [[float((seq_rows[j * (T - 1) + t][0] - bat_rows[t][j]).abs().max()) for t in range(T - 1)] for j in range(3)]
        same_outputs(seq, bat, change)
