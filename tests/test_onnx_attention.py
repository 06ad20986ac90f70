"""The general graph path's host half on token models (nsg_inspect_onnx): the attention fixtures plan with one fused
launch per attention block, the FLOP count includes the two attention matmuls, and everything 4-D outside the
attention pattern of DESIGN.md section 13.3 is refused with the node's name.  No device needed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

ATT_MODELS = ["net_att_pre", "net_att_hybrid"]


def read(golden_dir, name):
    with open(f"{golden_dir}/{name}.onnx", "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def gen():
    import make_onnx_attention_golden
    return make_onnx_attention_golden


def export(gen, net, tmp_path, name="m.onnx"):
    import torch
    torch.manual_seed(1)
    return gen.export_model(net.eval(), str(tmp_path / name))


def refused(nsg, data, *needles):
    with pytest.raises(nsg.NsgError) as e:
        nsg.inspect_onnx(data, 86)
    assert e.value.code == -4, e.value
    for n in needles:
        assert n in str(e.value), str(e.value)


def test_the_pre_ln_transformer_plans_with_one_launch_per_attention_block(nsg, golden_dir):
    data = read(golden_dir, "net_att_pre")
    with pytest.raises(nsg.NsgError):  # the family reader refuses it
        nsg.convert_onnx(data)
    info = nsg.inspect_onnx(data, 86)
    assert info["path"] == "graph" and info["precision"] == "fp32"
    assert info["attention_launches"] == 2
    # stem conv, positional add; per block: LayerNorm, QKV, attention, projection (+ residual), LayerNorm, FFN 1
    # (+ GELU), FFN 2 (+ residual); final LayerNorm, policy Linear, token mean, three dense; planes and outputs.
    # The token views, the `chunk` slices, the head splits and the policy transpose cost nothing.
    assert info["launches"] == 1 + 1 + 2 * 7 + 1 + 1 + 1 + 3 + 2
    assert info["conv_launches"] == 1 + 2 * 4 + 1 + 3
    F, H, d, ffn, VH = 32, 4, 8, 64, 32
    flops = 2 * 81 * 9 * 86 * F
    flops += 2 * (2 * 81 * (F * 3 * F + F * F + 2 * F * ffn) + 2 * (2 * 81 * 81 * d) * H)
    flops += 2 * 81 * F * 27 + 2 * F * VH + 2 * 2 * VH
    assert info["flops_per_position"] == flops


def test_the_hybrid_plans_with_its_scale_folded_into_the_attention_launch(nsg, golden_dir):
    info = nsg.inspect_onnx(read(golden_dir, "net_att_hybrid"), 86)
    assert info["path"] == "graph" and info["attention_launches"] == 1
    # stem; q, k, v (q * scale is folded, no elementwise launch); attention; projection (+ residual); LayerNorm; FFN 1
    # (+ ReLU); FFN 2 (+ residual); LayerNorm; two 3x3 convs; policy conv; value conv, flatten, three dense
    assert info["launches"] == 1 + 3 + 1 + 1 + 1 + 1 + 1 + 1 + 2 + 1 + 2 + 3 + 2
    assert info["conv_launches"] == 14
    F, H, d, ffn, VC, VH = 48, 3, 16, 96, 4, 32
    flops = 2 * 81 * 9 * 86 * F + 2 * 81 * (4 * F * F + 2 * F * ffn) + 2 * (2 * 81 * 81 * d) * H
    flops += 2 * (2 * 81 * 9 * F * F) + 2 * 81 * F * 27 + 2 * 81 * F * VC + 2 * VC * 81 * VH + 2 * 2 * VH
    assert info["flops_per_position"] == flops


@pytest.mark.parametrize("F,H,kw", [(32, 4, dict(bias=True)), (64, 1, dict(fused=False, scale_on="k")),
                                    (48, 3, dict(scale_on="q", k_perm=True))])
def test_small_attention_models_plan(nsg, gen, tmp_path, F, H, kw):
    info = nsg.inspect_onnx(export(gen, gen.AttNet(F, H, **kw), tmp_path), 86)
    assert info["path"] == "graph" and info["attention_launches"] == 1
    # stem, QKV (1 or 3), attention, projection (+ residual), policy, mean, value, draw + planes + outputs: the scalar
    # on q or k is folded wherever it stands
    assert info["launches"] == 1 + (1 if kw.get("fused", True) else 3) + 1 + 1 + 1 + 1 + 2 + 2


def test_a_scale_computed_from_size_is_folded_on_the_host(nsg, gen, tmp_path):
    """`q.size(-1) ** -0.5` is exported as Shape / Gather / Cast / Pow: folded on the host into the launch's scale (the
    Shape node on q does not count as a second consumer of an interior tensor)."""
    data = export(gen, gen.AttNet(32, 4, tweak="size_scale"), tmp_path)
    assert b"Pow" in data
    info = nsg.inspect_onnx(data, 86)
    assert info["attention_launches"] == 1 and info["launches"] == 1 + 1 + 1 + 1 + 1 + 1 + 2 + 2


def test_layernorm_on_tokens_and_on_a_flat_tensor_plans(nsg, gen, tmp_path):
    info = nsg.inspect_onnx(export(gen, gen.LNNet(), tmp_path), 86)
    # stem, LayerNorm, policy, mean, fc1, LayerNorm, ReLU (behind the LayerNorm: its own launch), value, draw
    assert info["path"] == "graph" and info["attention_launches"] == 0 and info["launches"] == 9 + 2


def test_refusals_outside_the_attention_pattern_name_the_node(nsg, gen, tmp_path):
    # a head dimension of 6 (24 channels, 4 heads): named at the Reshape that splits the heads
    refused(nsg, export(gen, gen.AttNet(24, 4), tmp_path), "node '/att/Reshape", "head dimension 6")
    # Softmax over the heads, not the keys
    refused(nsg, export(gen, gen.AttNet(32, 4, tweak="softmax_axis1"), tmp_path), "node '/att/Softmax'", "axis 1")
    # a Softmax outside the pattern, on the flat value-head tensor
    refused(nsg, export(gen, gen.AttNet(32, 4, flat_softmax=True), tmp_path), "node '/Softmax'", "Softmax")
    # the 4-D scores consumed by something other than the pattern
    refused(nsg, export(gen, gen.AttNet(32, 4, tweak="relu_scores"), tmp_path), "node '/att/Relu'", "Relu", "[N,4,81,81]")


def test_a_softmax_swapped_into_the_fixture_is_refused(nsg, golden_dir):
    # byte patch: the value head's Sigmoid of net_att_pre becomes a Softmax on a flat [N,1] tensor
    data = read(golden_dir, "net_att_pre")
    patched = data.replace(b"\x22\x07Sigmoid", b"\x22\x07Softmax")
    assert patched != data
    refused(nsg, patched, "Softmax", "node '/Sigmoid")


@pytest.mark.parametrize("name", ATT_MODELS)
def test_truncated_attention_models_are_errors_not_crashes(nsg, golden_dir, name):
    data = read(golden_dir, name)
    for cut in np.linspace(1, len(data) - 1, 20).astype(int):
        with pytest.raises(nsg.NsgError):
            nsg.inspect_onnx(data[:cut], 86)
