"""-m gpu: LeopardEngine.last_layer_rows at full depth and width (27 SigLIP + 32 Llama-3.1-8B layers) on the C2 (1 x 1344x896, S = 1242) and
C3 (6 x 1344x896, S = 7187: the benchmarked sample) inputs, fast and lo4 schedule: the last layer trimmed to the rows whose logits are read
("read", the default) gives bit for bit the last-position logits and the KV cache — every layer, every row: a superset of the rows
bench.py --dump-outputs samples — of the full last layer ("all").  The trimmed launches run other tile geometries (M <= 143 rows instead of
1242 / 7187) and a q-only / k|v-only split of the fused projection, so this is also the device check of the head-subset launches."""
import pytest
import torch

from leopard_amd.config import full_config
from leopard_amd.synth import synth_image_u8, synth_prompt_ids

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = {"c2": 1, "c3": 6}            # images of 1344 x 896


@pytest.fixture(scope="module")
def engine():
    from leopard_amd.engine import LeopardEngine
    from leopard_amd.ops import Ops
    from leopard_amd.weights import EngineWeights, SynthSource
    ops, cfg, dtype = Ops(), full_config(), torch.float16
    W = EngineWeights.build(cfg, SynthSource(cfg, ops, torch.device(DEV), dtype), dtype)
    eng = LeopardEngine(cfg, W, ops=ops, device=torch.device(DEV))
    yield eng
    del eng, W
    torch.cuda.empty_cache()


def sample_inputs(cfg, n_images, seed=0):
    from PIL import Image
    from leopard_amd.tiler import tile_sample, to_u8_tiles
    imgs = [Image.fromarray(synth_image_u8(seed + i, 1344, 896)) for i in range(n_images)]
    vit_inputs, plan = tile_sample(imgs)
    ids = synth_prompt_ids(plan.vit_inputs_per_image, cfg, seed=seed)
    return torch.from_numpy(to_u8_tiles(vit_inputs)).to(DEV), torch.from_numpy(ids).reshape(1, -1).to(DEV)


@pytest.mark.parametrize("precision", ["fast", "lo4"])
@pytest.mark.parametrize("case", ["c2", "c3"])
def test_read_rows_equal_all_rows_at_full_depth(engine, case, precision):
    from leopard_amd.engine import KVCache
    eng, cfg = engine, engine.cfg
    eng.precision = precision
    u8, ids = sample_inputs(cfg, CASES[case])
    S = eng.merged_len(ids, u8.shape[0])
    assert S == {"c2": 1242, "c3": 7187}[case]
    rows = []                                                    # query rows of the attention launches
    name = "attention_lo4" if precision == "lo4" else "attention"
    inner = getattr(eng.ops, name)
    qw = cfg.text_config.num_attention_heads * cfg.text_config.head_dim          # (the SigLIP tower's launches have another width)
    setattr(eng.ops, name, lambda q, *a, **k: (rows.append(q.shape[0]) if q.shape[1] == qw else None, inner(q, *a, **k))[1])
    out = {}
    try:
        for mode in ("all", "read"):
            eng.last_layer_rows = mode
            cache = KVCache(cfg, S, eng.dtype, torch.device(DEV))
            res = eng.prefill(ids, u8, cache=cache)
            torch.cuda.synchronize()
            assert res.seq_len == S and cache.length == S
            out[mode] = (res.logits_last.clone(), cache)
    finally:
        delattr(eng.ops, name)
        eng.last_layer_rows, eng.precision = "read", "fast"
    n = cfg.text_config.num_hidden_layers
    first_needed = S - 1 if precision == "fast" else S - eng.lo4_tail_rows(S)
    assert eng.lo4_tail_rows(S) == eng.LO4_TAIL_ROWS             # both samples are long: the tail policy, a real window
    assert rows[:n] == [S] * n and rows[n:] == [S] * (n - 1) + [S - first_needed // 128 * 128]
    (la, ca), (lr, cr) = out["all"], out["read"]
    assert bool(torch.isfinite(la).all()) and torch.equal(lr, la)
    for i in range(n):
        assert torch.equal(cr.k[i], ca.k[i]) and torch.equal(cr.v[i], ca.v[i]), i
    assert bool(ca.k[n - 1][S - 1].float().abs().sum() > 0) and bool(ca.v[n - 1][0].float().abs().sum() > 0)
