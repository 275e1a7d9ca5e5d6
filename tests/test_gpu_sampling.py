"""Sampled decoding on the MI355X: lmi_decode_sample at the real vocabulary sizes (kept set, chi-square against torch), and the
engine / surface end to end — reproducible under torch.manual_seed, graph = eager, greedy unchanged, stream tokens independent of the
batch size, new parameters without a new capture, tensor-parallel ranks drawing the same tokens, Idefics2."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests.sampling_ref import chi2_ok, draw_many, kept_probs, kept_set

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from leopard_amd.ops import Ops
    return Ops()


def gapped_row(V: int, head, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    row = -20.0 + torch.rand(V, generator=g)
    where = torch.randperm(V, generator=g)[:len(head)]
    for i, v in zip(where.tolist(), head):
        row[i] = v
    return row.to(DEV)


@pytest.mark.parametrize("V", [128256, 32000])
@pytest.mark.parametrize("T,k,p", [(1.0, 5, 1.0), (1.0, 0, 0.8), (0.7, 6, 0.7), (2.0, 8, 1.0), (1.0, 0, 0.0)])
def test_full_vocabulary_kept_set(ops, V, T, k, p):
    row = gapped_row(V, [4.0, 3.6, 3.5, 3.0, 2.9, 2.2, 2.0, 1.1, 1.0, 0.2], seed=V % 97)
    kept = kept_set(row, V, T, k, p)
    draws = draw_many(ops, row, V, T, k, p, n_rows=256, n_steps=4)
    assert set(draws.tolist()) == set(kept)


@pytest.mark.parametrize("V", [128256, 32000])
@pytest.mark.parametrize("T", [0.5, 1.0, 2.0])
def test_full_vocabulary_chi_square(ops, V, T):
    g = torch.Generator().manual_seed(21)
    row = (torch.randn(V, generator=g) * 2.0).to(DEV)
    k, p = 50, 0.95
    kept = kept_set(row, V, T, k, p)
    draws = draw_many(ops, row, V, T, k, p, n_rows=512, n_steps=8, seed0=77)
    assert set(draws.tolist()) <= set(kept)
    ok, stat, crit = chi2_ok(draws, kept, kept_probs(row, kept, T))
    assert ok, (V, T, stat, crit)


# ---- end to end on a synthetic model -------------------------------------------------------------------------------------------------
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


def test_sampled_generate_is_reproducible_graph_equals_eager_and_seeds_differ(model):
    ids = _prompts(1)[0]
    torch.manual_seed(5)
    a = model.generate(ids, max_new_tokens=12, **HOT)
    torch.manual_seed(5)
    b = model.generate(ids, max_new_tokens=12, **HOT)
    assert torch.equal(a, b)
    eng = model.engine
    eng.use_graphs = False
    try:
        torch.manual_seed(5)
        c = model.generate(ids, max_new_tokens=12, **HOT)
    finally:
        eng.use_graphs = True
    assert torch.equal(a, c)
    torch.manual_seed(6)
    d = model.generate(ids, max_new_tokens=12, **HOT)
    assert not torch.equal(a, d)
    assert torch.equal(model.generate(ids, max_new_tokens=12, seed=1234, **HOT), model.generate(ids, max_new_tokens=12, seed=1234, **HOT))


def test_greedy_is_unchanged(model):
    ids = _prompts(1, seed=3)[0]
    eng = model.engine
    base = eng.generate(ids, None, max_new_tokens=12, eos_token_id=())           # the greedy engine path
    assert torch.equal(model.generate(ids, max_new_tokens=12, do_sample=False), base)
    assert torch.equal(model.generate(ids, max_new_tokens=12), base)
    model.generate(ids, max_new_tokens=6, **HOT)                                   # a sampled call in between ...
    assert torch.equal(model.generate(ids, max_new_tokens=12, do_sample=False), base)     # ... leaves the greedy step as it was
    assert model.last_decoding == "greedy"


def test_parameters_change_without_a_recapture(model):
    ids = _prompts(1, seed=4)[0]
    eng = model.engine
    model.generate(ids, max_new_tokens=4, do_sample=True, temperature=0.7, seed=1)
    st = eng._gen_cache._decode_state
    g_s, g = st.graphs.get((True, False)), st.graphs.get((False, False))
    assert g_s is not None
    for kw in (dict(temperature=1.5), dict(top_k=3), dict(top_p=0.5), dict(temperature=0.3, top_k=0, top_p=0.9)):
        model.generate(ids, max_new_tokens=4, do_sample=True, seed=2, **kw)
        assert eng._gen_cache._decode_state is st and st.graphs.get((True, False)) is g_s and st.graphs.get((False, False)) is g
    reqs = [(p, None) for p in _prompts(4, seed=8)]
    model.generate_stream(reqs, batch_size=4, max_new_tokens=5, seed=3, do_sample=True, temperature=0.8)
    bst = eng._batch_states[4]
    bg = bst.graphs.get((True, False))
    model.generate_stream(reqs, batch_size=4, max_new_tokens=5, seed=3, do_sample=True, temperature=2.0, top_k=7, top_p=0.6)
    assert eng._batch_states[4] is bst and bst.graphs.get((True, False)) is bg


def test_stream_tokens_do_not_depend_on_batch_size(model):
    reqs = [(p, None) for p in _prompts(8, seed=11)]
    kw = dict(max_new_tokens=10, seed=2024, do_sample=True, temperature=0.9, top_k=20, top_p=0.95)
    eight = model.generate_stream(reqs, batch_size=8, **kw)
    two = model.generate_stream(reqs, batch_size=2, **kw)
    one = model.generate_stream(reqs, batch_size=1, **kw)
    # batch sizes 2 and 8 run the same batched kernels: same tokens; batch 1 runs the batch-1 head (other summation order), where a draw
    # can only move on a near tie of two perturbed Gumbel scores
    assert all(torch.equal(x, y) for x, y in zip(eight, two))
    same = sum(bool(torch.equal(x, y)) for x, y in zip(eight, one))
    assert same == len(reqs), [(x.tolist(), y.tolist()) for x, y in zip(eight, one)]
    batch = model.generate_batch(reqs, **kw)
    assert all(torch.equal(x, y) for x, y in zip(eight, batch))


# ---- tensor parallel: every rank draws the same token ----------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _tp_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    from leopard_amd import dist as D
    from leopard_amd.config import mid_config
    from leopard_amd.engine import LeopardEngine, SamplingParams
    from leopard_amd.ops import Ops
    from leopard_amd.weights import EngineWeights, SynthSource
    torch.cuda.set_device(DEV)
    D.init(backend="gloo")
    ops, cfg, dtype = Ops(), mid_config(), torch.float16
    eng = LeopardEngine(cfg, EngineWeights.build(cfg, SynthSource(cfg, ops, DEV, dtype), dtype, tp_rank=rank, tp_size=world), ops=ops,
                        device=DEV)
    ids = torch.from_numpy(np.random.default_rng(1).integers(1, 1000, (1, 24))).to(DEV)
    outs = [eng.generate(ids, None, max_new_tokens=8, eos_token_id=(), sampling=SamplingParams(3.0, 0, 0.99, s))[0].tolist() for s in (7, 8)]
    torch.cuda.synchronize()
    out.put((rank, outs))
    D.barrier()


def test_tensor_parallel_ranks_draw_the_same_tokens():
    mp.set_start_method("spawn", force=True)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_tp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=900) for _ in procs)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    (_, o0), (_, o1) = res
    assert o0 == o1
    assert o0[0] != o0[1]                                                # the two seeds sample differently


# ---- Idefics2 -------------------------------------------------------------------------------------------------------------------------
def test_idefics2_sampled_generate():
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
    torch.manual_seed(3)
    a = m.generate(ids, max_new_tokens=8, do_sample=True, temperature=5.0, top_k=0)
    torch.manual_seed(3)
    b = m.generate(ids, max_new_tokens=8, do_sample=True, temperature=5.0, top_k=0)
    assert torch.equal(a, b) and not torch.equal(a, greedy) and m.last_decoding.startswith("sample(")
    assert not (set(a[0, ids.shape[1]:].tolist()) & set(m.bad_words_ids))         # suppressed ids are never drawn
    assert torch.equal(m.generate(ids, max_new_tokens=8), greedy)
