"""f1: the tensor names leopard_amd reads from a checkpoint are exactly the names the reference's converter
writes (toolkits/model_checkpoints_convertor/llava/hf2megatron_llava.py: the megatron -> HF direction, name map :168-175,
LLM layers :1150-1300, vision / projector / embeddings :1309-1455).  The string fragments the converter assembles keys
from, and its q / k / v index map, are stored data (tests/golden/converter_keys.json, written by oracle/gen_converter_keys.py,
which parses the converter's source without executing it)."""
import json
import os
import re


def test_engine_reads_exactly_the_converter_key_set(golden_dir):
    from leopard_amd.config import full_config
    from leopard_amd.synth import param_specs
    with open(os.path.join(golden_dir, "converter_keys.json")) as f:
        fx = json.load(f)
    lit = set(fx["name_literals"])
    # fragments of the name map (:168-175) and of the vision branch (:1309-1416)
    llm_ops = {".self_attn.o_proj.", ".mlp.gate_proj.", ".mlp.up_proj.", ".mlp.down_proj.", ".input_layernorm.", ".post_attention_layernorm."}
    assert llm_ops <= lit
    assert "language_model.model.layers.{layer_idx}" in lit and ".self_attn.{QKV[index]}.weight" in lit
    assert fx["qkv_index_map"] == ["q_proj", "k_proj", "v_proj"]
    vit_prefix = "vision_tower.vision_model.encoder.layers."
    vit_suffix = {".self_attn.out_proj.weight", ".self_attn.out_proj.bias", ".mlp.fc1.weight", ".mlp.fc1.bias", ".mlp.fc2.weight",
                  ".mlp.fc2.bias", ".layer_norm1.weight", ".layer_norm1.bias", ".layer_norm2.weight", ".layer_norm2.bias"}
    assert vit_prefix in lit and vit_suffix <= lit and ".self_attn.{QKV[index]}.{weight_or_bias}" in lit

    def written_by_converter(name: str) -> bool:
        if name in lit:                                               # embeddings, final norm, lm_head, projector, patch / position embedding, post LN
            return True
        m = re.fullmatch(r"language_model\.model\.layers\.(\d+)(\..+?\.)weight", name)
        if m:
            return m.group(2) in llm_ops or m.group(2) in {".self_attn.q_proj.", ".self_attn.k_proj.", ".self_attn.v_proj."}
        m = re.fullmatch(re.escape(vit_prefix) + r"(\d+)(\..+)", name)
        if m:
            return m.group(2) in vit_suffix or bool(re.fullmatch(r"\.self_attn\.[qkv]_proj\.(weight|bias)", m.group(2)))
        return False

    names = [n for n, _, _ in param_specs(full_config())]
    unknown = [n for n in names if not written_by_converter(n)]
    assert not unknown, unknown[:10]
    # and the other way round: every non-layer key the converter writes is consumed (or deliberately ignored, listed here)
    ignored = {"vision_tower.vision_model.pre_layrnorm.weight", "vision_tower.vision_model.pre_layrnorm.bias",      # CLIP tower only
               "vision_tower.vision_model.embeddings.cls_token", "vision_tower.vision_model.embeddings.class_embedding"}
    top = {l for l in lit if re.match(r"(language_model|multi_modal_projector|vision_tower\.vision_model)\.[a-z_.0-9]+\.(weight|bias)$", l)
           or l in ignored}
    assert top - ignored <= set(names), sorted(top - ignored - set(names))
    assert len(names) == 27 * 16 + 3 + 2 + 4 + 32 * 9 + 3            # SigLIP layers, patch/pos embeddings, post-LN, projector, Llama layers, embed/norm/head
