"""min_p, typical_p, epsilon_cutoff and eta_cutoff on the MI355X: lmi_decode_sample_ex on the case list shared with
tests/test_emu_sampling_ext.py, at V = 1000 / 1003 and at the real vocabulary sizes (the kept set is the set of the draws, chi-square, all
four off = lmi_decode_sample bit for bit, rows independent of slot and batch), and the engine / surfaces end to end on the mid model of
tests/test_gpu_sampling.py: reproducible under a seed, graph = eager, new values without a new capture, stream tokens independent of the
batch size, min_p = 1.0 = greedy, a call without the four launching what it launched before, generation_config.json, refusals, Idefics2."""
import json

import numpy as np
import pytest
import torch

from tests import sampling_ext_ref as X
from tests.row_kernels_ref import HEAD, gapped_row

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from leopard_amd.ops import Ops
    return Ops()


# ---- the kernel ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(X.GAPPED_CASES)))
def test_kept_set_is_the_set_of_draws_fewer_tokens_than_threads(ops, case):
    V = 1000                                                          # ld = 1024, 100.0 behind the vocabulary: never drawn
    X.check_kept_set_equals_draws(ops, gapped_row(V, HEAD, seed=1, ld=1024).to(DEV), V, X.GAPPED_CASES[case], 256, 8)


@pytest.mark.parametrize("case", [0, 4, 7, 9, 14])                    # each warper alone and all four: the scalar path
def test_kept_set_on_rows_that_are_not_16_byte_aligned(ops, case):
    V = 1003
    row = gapped_row(V, HEAD, seed=2)
    X.check_kept_set_equals_draws(ops, row, V, X.GAPPED_CASES[case], 256, 8, logits=X.unaligned_rows(row, 256, DEV))


@pytest.mark.parametrize("V", [32000, 128256])
def test_kept_set_at_the_real_vocabulary_sizes(ops, V):
    row = gapped_row(V, HEAD, seed=1)
    logits = row.to(DEV).reshape(1, -1).expand(64, -1).contiguous()   # one copy of the rows for every case
    for c in X.GAPPED_CASES:
        X.check_kept_set_equals_draws(ops, row, V, c, 64, 16, logits=logits)


@pytest.mark.parametrize("case", range(len(X.BROAD_CASES)))
def test_kept_set_on_the_broad_row_where_typical_p_removes_the_top_token(ops, case):
    row = X.broad_row()
    kept, notes = X.check_kept_set_equals_draws(ops, row.to(DEV), row.numel(), X.BROAD_CASES[case], 256, 8)
    if case < 3:
        assert notes["top_removed"] and int(row.argmax()) not in kept


@pytest.mark.parametrize("case", range(len(X.TIE_CASES)))
def test_tie_groups_on_the_boundaries_are_kept_whole(ops, case):
    row = X.tie_row()
    _, notes = X.check_kept_set_equals_draws(ops, row.to(DEV), row.numel(), X.TIE_CASES[case], 256, 4)
    assert max(notes.get(key, 0) for key in ("typ_group", "eps_group", "eta_group")) >= 2


def test_one_allowed_token_suppressed_ids_and_rows_without_a_drawable_token(ops):
    X.check_special_rows(ops, DEV)


@pytest.mark.parametrize("V", [1000, 32000, 128256])
def test_distribution_chi_square(ops, V):
    X.check_chi_square(ops, DEV, V, n_rows=128, n_steps=16)


@pytest.mark.parametrize("V", [1003, 128256])
def test_all_four_off_is_decode_sample(ops, V):
    X.check_all_off_equals_decode_sample(ops, DEV, V)


@pytest.mark.parametrize("V", [1003, 128256])
def test_rows_with_different_parameters_match_their_solo_launches(ops, V):
    X.check_rows_are_independent(ops, DEV, V)


# ---- end to end on a synthetic model (the mid model of tests/test_gpu_sampling.py) ---------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    from leopard_amd import compat
    from leopard_amd.config import full_config
    from leopard_amd.ops import Ops
    from leopard_amd.weights import SynthSource
    cfg = full_config()
    cfg.vision_config.num_hidden_layers = 1
    cfg.text_config.num_hidden_layers = 2
    cfg.text_config.vocab_size = 1024
    cfg.image_token_index = 1000
    ops = Ops()
    m = compat.LeopardForConditionalGeneration(cfg, lambda dev, dt: SynthSource(cfg, ops, dev, dt), torch.float16, ops,
                                               torch_dtype=torch.float16)
    return m.to(DEV)


def _prompts(n, seed=0):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(rng.integers(1, 900, (1, int(rng.integers(5, 20))))).to(DEV) for _ in range(n)]


HOT = dict(do_sample=True, temperature=4.0, top_k=0, top_p=0.98)          # the synthetic model's logits are flat enough to vary
EXT = dict(min_p=0.05, typical_p=0.9, epsilon_cutoff=2e-4, eta_cutoff=1e-3)


class _Spy:
    """Records the choice launches of an Ops without changing them."""

    def __init__(self, ops):
        self.ops, self.calls = ops, []
        self._saved = {name: getattr(ops, name) for name in ("decode_sample", "decode_sample_ex", "decode_advance")}

    def __enter__(self):
        for name, fn in self._saved.items():
            setattr(self.ops, name, (lambda *a, _n=name, _f=fn, **kw: (self.calls.append(_n), _f(*a, **kw))[1]))
        return self

    def __exit__(self, *exc):
        for name in self._saved:
            delattr(self.ops, name)


def test_a_call_without_the_four_launches_decode_sample_and_returns_the_tokens_of_before(model):
    """Runs first on the module's model: no _ex call has been made yet."""
    ids = _prompts(1, seed=21)[0]
    eng = model.engine
    with _Spy(eng.ops) as spy:
        before = model.generate(ids, max_new_tokens=10, seed=5, **HOT)
        assert "decode_sample_ex" not in spy.calls and "decode_sample" in spy.calls
        st = eng._gen_cache._decode_state
        assert (True, False) in st.graphs and (True, False, "ex") not in st.graphs
        plain_graph = st.graphs[(True, False)]
        del spy.calls[:]
        ext = model.generate(ids, max_new_tokens=10, seed=5, **HOT, **EXT)
        assert "decode_sample_ex" in spy.calls and "decode_sample" not in spy.calls and (True, False, "ex") in st.graphs
        assert model.last_decoding == "sample(temperature=4, top_k=0, top_p=0.98, min_p=0.05, typical_p=0.9, epsilon_cutoff=0.0002, eta_cutoff=0.001)"
        del spy.calls[:]
        after = model.generate(ids, max_new_tokens=10, seed=5, **HOT)
        assert "decode_sample_ex" not in spy.calls and st.graphs[(True, False)] is plain_graph
    assert torch.equal(before, after) and not torch.equal(before, ext)
    assert model.last_decoding == "sample(temperature=4, top_k=0, top_p=0.98)"


def test_reproducible_under_a_seed_and_graph_equals_eager(model):
    ids = _prompts(1)[0]
    torch.manual_seed(5)
    a = model.generate(ids, max_new_tokens=12, **HOT, **EXT)
    torch.manual_seed(5)
    b = model.generate(ids, max_new_tokens=12, **HOT, **EXT)
    assert torch.equal(a, b)
    eng = model.engine
    eng.use_graphs = False
    try:
        torch.manual_seed(5)
        c = model.generate(ids, max_new_tokens=12, **HOT, **EXT)
    finally:
        eng.use_graphs = True
    assert torch.equal(a, c)
    torch.manual_seed(6)
    assert not torch.equal(a, model.generate(ids, max_new_tokens=12, **HOT, **EXT))


def test_the_four_values_change_without_a_recapture(model):
    ids = _prompts(1, seed=4)[0]
    eng = model.engine
    model.generate(ids, max_new_tokens=4, seed=1, **HOT, min_p=0.1)
    st = eng._gen_cache._decode_state
    g = st.graphs[(True, False, "ex")]
    n_graphs = len(st.graphs)
    outs = []
    for kw in (dict(min_p=0.3), dict(typical_p=0.5), dict(epsilon_cutoff=1e-3), dict(eta_cutoff=0.05), EXT):
        outs.append(model.generate(ids, max_new_tokens=8, seed=2, **HOT, **kw))
        assert eng._gen_cache._decode_state is st and st.graphs[(True, False, "ex")] is g and len(st.graphs) == n_graphs
    assert len({tuple(o[0].tolist()) for o in outs}) > 1              # the new values were read
    reqs = [(p, None) for p in _prompts(4, seed=8)]
    model.generate_stream(reqs, batch_size=4, max_new_tokens=5, seed=3, **HOT, min_p=0.1)
    bst = eng._batch_states[4]
    bg = bst.graphs[(True, False, "ex")]
    model.generate_stream(reqs, batch_size=4, max_new_tokens=5, seed=3, **HOT, **EXT)
    assert eng._batch_states[4] is bst and bst.graphs[(True, False, "ex")] is bg


def test_stream_tokens_do_not_depend_on_batch_size(model):
    reqs = [(p, None) for p in _prompts(8, seed=11)]
    kw = dict(max_new_tokens=10, seed=2024, do_sample=True, temperature=0.9, top_k=20, top_p=0.95, min_p=0.05, typical_p=0.9, eta_cutoff=1e-3)
    eight = model.generate_stream(reqs, batch_size=8, **kw)
    two = model.generate_stream(reqs, batch_size=2, **kw)
    assert all(torch.equal(x, y) for x, y in zip(eight, two))
    batch = model.generate_batch(reqs, **kw)
    assert all(torch.equal(x, y) for x, y in zip(eight, batch))
    shared = model.generate_shared(reqs[0][0], None, [r[0] for r in reqs[1:4]], **kw)
    again = model.generate_shared(reqs[0][0], None, [r[0] for r in reqs[1:4]], decode="shared", **kw)
    assert len(shared) == 3 and len(again) == 3
    assert all(torch.equal(s, t) for s, t in zip(shared, model.generate_shared(reqs[0][0], None, [r[0] for r in reqs[1:4]], **kw)))
    assert all(torch.equal(s, t) for s, t in zip(again, model.generate_shared(reqs[0][0], None, [r[0] for r in reqs[1:4]], decode="shared", **kw)))


def test_min_p_one_is_greedy_with_rules_and_with_logprobs(model):
    ids = _prompts(1, seed=3)[0]
    greedy = model.generate(ids, max_new_tokens=12)
    assert torch.equal(model.generate(ids, max_new_tokens=12, seed=9, **HOT, min_p=1.0), greedy)
    assert torch.equal(model.generate(ids, max_new_tokens=12, seed=9, **HOT, epsilon_cutoff=0.99), greedy)
    ruled = model.generate(ids, max_new_tokens=12, repetition_penalty=1.3)
    assert torch.equal(model.generate(ids, max_new_tokens=12, seed=9, repetition_penalty=1.3, **HOT, min_p=1.0), ruled)
    out = model.generate(ids, max_new_tokens=12, seed=9, logprobs=2, **HOT, min_p=1.0)
    ref = model.generate(ids, max_new_tokens=12, logprobs=2)
    assert torch.equal(out.sequences, greedy) and torch.equal(out.token_logprobs, ref.token_logprobs)      # logprobs are of the raw row
    assert torch.equal(model.generate(ids, max_new_tokens=12), greedy) and model.last_decoding == "greedy"


def test_generation_config_values_are_picked_up_and_refusals_come_before_any_launch(model, tmp_path):
    from leopard_amd import sampling
    ids = _prompts(1, seed=6)[0]
    (tmp_path / "generation_config.json").write_text(json.dumps({"do_sample": True, "temperature": 4.0, "top_k": 0, "min_p": 0.07,
                                                                 "typical_p": 0.8}))
    saved = model.generation_defaults
    model.generation_defaults = sampling.read_generation_config(str(tmp_path))
    try:
        a = model.generate(ids, max_new_tokens=8, seed=4)
        assert model.last_decoding == "sample(temperature=4, top_k=0, top_p=1, min_p=0.07, typical_p=0.8)"
        assert torch.equal(a, model.generate(ids, max_new_tokens=8, seed=4, do_sample=True, temperature=4.0, top_k=0, min_p=0.07, typical_p=0.8))
        model.generate(ids, max_new_tokens=4, seed=4, min_p=0.0, typical_p=1.0)                            # the call's "off" wins
        assert model.last_decoding == "sample(temperature=4, top_k=0, top_p=1)"
    finally:
        model.generation_defaults = saved
    with _Spy(model.engine.ops) as spy:
        for kw in (dict(min_p=1.5), dict(typical_p=0.0), dict(epsilon_cutoff=1.0), dict(eta_cutoff=-0.1)):
            with pytest.raises(ValueError):
                model.generate(ids, max_new_tokens=4, **HOT, **kw)
            with pytest.raises(ValueError):
                model.generate_stream([(ids, None)], max_new_tokens=4, **HOT, **kw)
        model.engine.W.tp_size = 2                                    # what a tensor-parallel rank's weights say
        try:
            with pytest.raises(NotImplementedError):
                model.generate(ids, max_new_tokens=4, **HOT, min_p=0.1)
        finally:
            model.engine.W.tp_size = 1
        assert spy.calls == []
    assert model.generate(ids, max_new_tokens=4, do_sample=False, min_p=7.0).shape[1] == ids.shape[1] + 4      # greedy: ignored, as temperature


# ---- Idefics2 -------------------------------------------------------------------------------------------------------------------------
def test_idefics2_generate_with_its_suppress_list():
    from leopard_amd import idefics2_compat as IC
    from leopard_amd.idefics2 import Idefics2SynthSource
    from leopard_amd.ops import Ops
    from tests.test_emu_idefics2 import micro_idefics2
    ops = Ops()
    cfg = micro_idefics2()
    m = IC.Idefics2ForConditionalGeneration(cfg, lambda dev, dt: Idefics2SynthSource(cfg, ops, dev, dt), torch.float16, ops,
                                            eos_token_id=(2,)).to(DEV)
    ids = torch.from_numpy(np.random.default_rng(2).integers(3, 200, (1, 12))).to(DEV)
    greedy = m.generate(ids, max_new_tokens=8)
    kw = dict(max_new_tokens=8, do_sample=True, temperature=5.0, top_k=0, min_p=0.02, typical_p=0.95, eta_cutoff=1e-3)
    torch.manual_seed(3)
    a = m.generate(ids, **kw)
    torch.manual_seed(3)
    b = m.generate(ids, **kw)
    assert torch.equal(a, b) and not torch.equal(a, greedy) and "min_p=0.02" in m.last_decoding
    assert not (set(a[0, ids.shape[1]:].tolist()) & set(m.bad_words_ids))         # suppressed ids are never drawn
    assert torch.equal(m.generate(ids, max_new_tokens=8, do_sample=True, temperature=5.0, top_k=0, seed=1, min_p=1.0), greedy)
