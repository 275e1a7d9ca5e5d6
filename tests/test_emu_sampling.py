"""Sampled decoding on the CPU: lmi_decode_sample through the kernel-logic emulator (kept set, distribution, determinism, the stop rule
it shares with lmi_decode_advance), and the generate() surface's sampling arguments without a kernel launch."""
import json
import warnings

import numpy as np
import pytest
import torch

from tests.emu_util import emu_ops
from tests import row_kernels_ref as R
from tests.row_kernels_ref import HEAD, gapped_row
from tests.sampling_ref import chi2_ok, draw_many, kept_probs, kept_set


@pytest.fixture(scope="module")
def ops():
    return emu_ops()


@pytest.mark.parametrize("T,k,p", [(1.0, 5, 1.0), (1.0, 0, 0.8), (1.0, 6, 0.7), (0.5, 0, 0.9), (2.0, 8, 1.0), (1.0, 0, 0.0),
                                   (1.0, 3, 0.999)])
def test_kept_set_matches_float64_reference(ops, T, k, p):
    V = 1000
    row = gapped_row(V, HEAD, seed=1, ld=1024)
    kept = kept_set(row, V, T, k, p)
    draws = draw_many(ops, row, V, T, k, p, n_rows=64, n_steps=12)
    assert set(draws.tolist()) <= set(kept)
    probs = kept_probs(row, kept, T)
    assert all(q * len(draws) > 8 for q in probs)                     # every kept token is likely enough to show up
    assert set(draws.tolist()) == set(kept)
    if p == 0.0:
        assert len(kept) == 1                                         # top-p keeps at least one token


def test_kept_set_ties_keep_the_lower_indices(ops):
    R.check_kept_set_ties_keep_the_lower_indices(ops, "cpu")


@pytest.mark.parametrize("T", [0.5, 1.0, 2.0])
def test_distribution_chi_square(ops, T):
    V = 256
    g = torch.Generator().manual_seed(11)
    row = torch.randn(V, generator=g) * 1.5
    k, p = 24, 0.95
    kept = kept_set(row, V, T, k, p)
    draws = draw_many(ops, row, V, T, k, p, n_rows=128, n_steps=24, seed0=1000)
    assert set(draws.tolist()) <= set(kept)
    ok, stat, crit = chi2_ok(draws, kept, kept_probs(row, kept, T))
    assert ok, (T, stat, crit)


def test_draw_depends_on_seed_step_and_row_only(ops):
    R.check_draw_depends_on_seed_step_and_row_only(ops, "cpu")


def test_suppressed_ids_are_never_drawn(ops):
    R.check_suppressed_ids_are_never_drawn(ops, "cpu")


def test_top_k_1_is_decode_advance_and_shares_its_stop_rule(ops):
    R.check_top_k_1_is_decode_advance_and_shares_its_stop_rule(ops, "cpu")


def test_rows_without_a_drawable_token_give_token_zero(ops):
    R.check_rows_without_a_drawable_token_give_token_zero(ops, "cpu")


# ---- the generate() surface: arguments, defaults, warnings (no kernel launch) -----------------------------------------------------------
def test_resolve_follows_hf_semantics():
    from leopard_amd import sampling
    assert sampling.resolve({}, None) is None and sampling.resolve({}, False, temperature=0.3) is None      # absent / False: greedy
    sp = sampling.resolve({}, True, seed=7)
    assert (sp.temperature, sp.top_k, sp.top_p, sp.seed) == (1.0, 50, 1.0, 7)                             # HF defaults
    sp = sampling.resolve({"do_sample": True, "temperature": 0.6, "top_p": 0.9}, None, top_k=5, seed=1)
    assert (sp.temperature, sp.top_k, sp.top_p) == (0.6, 5, 0.9)                                          # call > generation_config > HF
    assert sampling.resolve({"do_sample": True}, False) is None
    for t in (0.0, -1.0):
        with pytest.raises(ValueError):
            sampling.resolve({}, True, temperature=t)
    with pytest.raises(ValueError):
        sampling.resolve({}, True, top_p=1.5)
    torch.manual_seed(123)
    a = sampling.resolve({}, True).seed
    torch.manual_seed(123)
    assert sampling.resolve({}, True).seed == a and sampling.resolve({}, True).seed != a                  # seeded from torch's CPU generator
    assert sampling.describe(None) == "greedy" and sampling.describe(sp).startswith("sample(temperature=0.6")


def test_unsupported_options_warn_once_naming_them():
    from leopard_amd import sampling
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        sampling.warn_unsupported("generate", {"num_beams": 4, "repetition_penalty": 1.2, "min_p": 0.1, "pad_token_id": 0})
        sampling.warn_unsupported("generate", {"num_beams": 1, "repetition_penalty": 1.0, "use_cache": True})
    assert len(w) == 1
    msg = str(w[0].message)
    assert "num_beams" in msg and "repetition_penalty" in msg and "min_p" in msg and "pad_token_id" not in msg


def test_generation_config_sampling_defaults_are_picked_up(tmp_path):
    from leopard_amd import compat, idefics2_compat as IC
    from leopard_amd.checkpoint import save_synthetic_checkpoint
    from tests.test_emu_engine import micro_config
    d = tmp_path / "llava"
    save_synthetic_checkpoint(str(d), micro_config())
    assert compat.from_pretrained(str(d)).generation_defaults == {}                 # no generation_config.json: nothing changes
    (d / "generation_config.json").write_text(json.dumps({"do_sample": True, "temperature": 0.6, "top_p": 0.9, "eos_token_id": 1}))
    m = compat.from_pretrained(str(d))
    assert m.generation_defaults == {"do_sample": True, "temperature": 0.6, "top_p": 0.9}
    from leopard_amd import reference_shim
    cls = reference_shim._llava_class()
    m2 = cls.from_pretrained(str(d), ops=object())
    assert m2.generation_defaults == m.generation_defaults
    # Idefics2: the loader that already reads eos / bad_words_ids from the same file
    from tests.test_emu_idefics2 import micro_idefics2
    import dataclasses
    di = tmp_path / "idefics2"
    di.mkdir()
    cfg = micro_idefics2()
    (di / "config.json").write_text(json.dumps(dataclasses.asdict(cfg)))
    (di / "generation_config.json").write_text(json.dumps({"do_sample": True, "top_k": 20, "eos_token_id": [2, 32002]}))
    mi = IC.Idefics2ForConditionalGeneration.from_pretrained(str(di))
    assert mi.generation_defaults == {"do_sample": True, "top_k": 20} and mi.eos_token_id == (2, 32002)


# ---- the engine over the emulated kernels -----------------------------------------------------------------------------------------------
def _micro_engine(ops):
    from leopard_amd.engine import LeopardEngine
    from leopard_amd.weights import EngineWeights, SynthSource
    from tests.test_emu_engine import micro_config
    cfg = micro_config()
    W = EngineWeights.build(cfg, SynthSource(cfg, ops, "cpu", torch.float16), torch.float16)
    return LeopardEngine(cfg, W, ops=ops, device="cpu")


def test_engine_sampled_generate_is_reproducible_and_top_k_1_is_greedy(ops):
    from leopard_amd.engine import SamplingParams
    eng = _micro_engine(ops)
    ids = torch.tensor([[7, 8, 9, 10]])
    greedy = eng.generate(ids, None, max_new_tokens=5, eos_token_id=())
    assert torch.equal(eng.generate(ids, None, max_new_tokens=5, eos_token_id=(), sampling=SamplingParams(0.8, 1, 1.0, 5)), greedy)
    hot = SamplingParams(temperature=50.0, top_k=0, top_p=1.0, seed=11)            # near-uniform over 256 tokens
    a = eng.generate(ids, None, max_new_tokens=5, eos_token_id=(), sampling=hot)
    b = eng.generate(ids, None, max_new_tokens=5, eos_token_id=(), sampling=hot)
    c = eng.generate(ids, None, max_new_tokens=5, eos_token_id=(), sampling=SamplingParams(50.0, 0, 1.0, 12))
    assert torch.equal(a, b) and not torch.equal(a, c) and not torch.equal(a, greedy)
    # greedy after sampling: the greedy step still runs decode_advance
    assert torch.equal(eng.generate(ids, None, max_new_tokens=5, eos_token_id=()), greedy)


def test_engine_sampled_stream_does_not_depend_on_batch_size(ops):
    from leopard_amd.engine import SamplingParams
    eng = _micro_engine(ops)
    eng.HIST = 2
    samples = [(torch.tensor([[5, 6, 7]]), None), (torch.tensor([[9, 3]]), None), (torch.tensor([[11, 12, 13, 14]]), None)]
    sp = SamplingParams(temperature=50.0, top_k=0, top_p=1.0, seed=99)
    one = eng.generate_stream(samples, batch_size=1, max_new_tokens=4, eos_token_id=(), sampling=sp)
    three = eng.generate_stream(samples, batch_size=3, max_new_tokens=4, eos_token_id=(), sampling=sp)
    assert all(torch.equal(x, y) for x, y in zip(one, three)), ([o.tolist() for o in one], [t.tolist() for t in three])
    assert len({tuple(o[0, -4:].tolist()) for o in one}) == 3
    batch = eng.generate_batch(samples, max_new_tokens=4, eos_token_id=(), sampling=sp)
    assert all(torch.equal(x, y) for x, y in zip(one, batch))
