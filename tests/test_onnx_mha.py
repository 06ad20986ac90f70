"""The general graph path's host half on PyTorch's stock transformer modules (nsg_inspect_onnx, no device):
nn.MultiheadAttention, nn.TransformerEncoderLayer and nn.TransformerEncoder plan with exactly the launches of the
hand-written form with the same weights (tests/mha_models.py), one kLaunchAttention per attention, and what stays
outside the pattern ("stock transformer modules") is refused with the node's name and a reason.

Before the pattern existed every model here stopped at the module's first shape assertion:
    node '/att/m/Mod' (Mod): op 'Mod' is outside the supported op set"""
import numpy as np
import pytest

import mha_models as mm

MHA_CASES = [dict(need_weights=nw, batch_first=bf, bias=b) for nw in (False, True) for bf in (True, False) for b in (True, False)]
ENC_CASES = [dict(norm_first=nf, activation=act) for nf in (True, False) for act in ("relu", "gelu")]


def ident(kw):
    return "-".join(f"{k}={v}" for k, v in kw.items())


def plans_like_its_twin(nsg, net, tmp_path, attentions):
    info = nsg.inspect_onnx(mm.export(net, tmp_path / "module.onnx"), 86)
    twin = nsg.inspect_onnx(mm.export(mm.twin(net), tmp_path / "twin.onnx"), 86)
    assert twin["path"] == "graph" and twin["attention_launches"] == attentions
    assert info["path"] == "graph" and info["precision"] == "fp32"
    assert info["attention_launches"] == attentions
    assert (info["launches"], info["conv_launches"]) == (twin["launches"], twin["conv_launches"])
    assert info["flops_per_position"] == twin["flops_per_position"]
    return info


def refused(nsg, data, *needles):
    with pytest.raises(nsg.NsgError) as e:
        nsg.inspect_onnx(data, 86)
    assert e.value.code == -4, e.value
    msg = str(e.value).split("general graph path: ")[-1]
    for n in needles:
        assert n in msg, msg


@pytest.mark.parametrize("kw", MHA_CASES, ids=ident)
def test_multihead_attention_plans_like_the_hand_written_form(nsg, tmp_path, kw):
    info = plans_like_its_twin(nsg, mm.make("mha", 32, 2, seed=1, **kw), tmp_path, 1)
    # stem, QKV, attention, projection (+ residual), policy, mean, value, draw + planes + outputs: the seq-first views,
    # the split of the packed projection and the (board x head) axis cost nothing
    assert info["launches"] == 8 + 2


@pytest.mark.parametrize("E,H", [(48, 3), (24, 2), (64, 1)])
@pytest.mark.parametrize("need_weights", [False, True])
def test_other_head_counts_and_one_head(nsg, tmp_path, E, H, need_weights):
    """One head: N*1 folds to N, so the head split's target [81,N,64] is the tensor's own shape."""
    plans_like_its_twin(nsg, mm.make("mha", E, H, seed=2, need_weights=need_weights), tmp_path, 1)


@pytest.mark.parametrize("kw", ENC_CASES, ids=ident)
def test_an_encoder_layer_plans_like_the_hand_written_block(nsg, tmp_path, kw):
    info = plans_like_its_twin(nsg, mm.make("enc", 32, 2, seed=3, ffn=64, **kw), tmp_path, 1)
    # stem; QKV, attention, projection (+ residual), FFN 1 (+ activation), FFN 2 (+ residual), two LayerNorms; four heads
    assert info["launches"] == 1 + 7 + 4 + 2


def test_a_two_layer_encoder_with_a_final_norm(nsg, tmp_path):
    info = plans_like_its_twin(nsg, mm.make("enc", 32, 2, seed=4, ffn=64, layers=2, final_norm=True), tmp_path, 2)
    assert info["launches"] == 1 + 2 * 7 + 1 + 4 + 2


# ---- what stays refused ---------------------------------------------------------------------------------------------------
def mask():
    import torch
    m = torch.zeros(81, 81)
    m[0, 1] = float("-inf")
    return m


@pytest.mark.parametrize("need_weights,scores", [(False, "[N,2,81,81]"), (True, "[N*2,81,81]")])
def test_attn_mask_is_refused(nsg, tmp_path, need_weights, scores):
    net = mm.make("mha", 32, 2, need_weights=need_weights, call=dict(attn_mask=mask()))
    refused(nsg, mm.export(net, tmp_path / "m.onnx"), "node '/att/m/Add_2' (Add)", "attn_mask", scores)


def test_key_padding_mask_is_refused(nsg, tmp_path):
    import torch
    net = mm.make("mha", 32, 2, call=dict(key_padding_mask=torch.zeros(1, 81, dtype=torch.bool)))
    refused(nsg, mm.export(net, tmp_path / "m.onnx"), "node '/att/m/ConstantOfShape' (ConstantOfShape)", "outside the supported op set")


@pytest.mark.parametrize("need_weights,node,why", [(False, "node '/att/m/Trilu' (Trilu)", "outside the supported op set"),
                                                   (True, "node '/att/m/Add_2' (Add)", "is_causal")])
def test_is_causal_is_refused(nsg, tmp_path, need_weights, node, why):
    import torch
    causal = torch.nn.Transformer.generate_square_subsequent_mask(81)
    net = mm.make("mha", 32, 2, need_weights=need_weights, call=dict(attn_mask=causal, is_causal=True))
    refused(nsg, mm.export(net, tmp_path / "m.onnx"), node, why)


def test_attention_weights_that_are_used_are_refused(nsg, tmp_path):
    net = mm.make("mha", 32, 2, need_weights=True, use_weights=True)
    refused(nsg, mm.export(net, tmp_path / "m.onnx"), "node '/att/m/", "interior tensor of the attention pattern", "more than one consumer")


def test_kdim_and_vdim_other_than_embed_dim_are_refused(nsg, tmp_path):
    net = mm.make("mha", 32, 2, cross=True, kdim=16, vdim=16)
    refused(nsg, mm.export(net, tmp_path / "m.onnx"), "node '/att/m/Reshape", "no part of a packed q / k / v projection", "kdim or vdim")


def test_cross_attention_is_refused(nsg, tmp_path):
    """Query from one tensor, key and value from another: the module slices in_proj_weight in the graph."""
    refused(nsg, mm.export(mm.make("mha", 32, 2, cross=True), tmp_path / "m.onnx"), "node '/att/m/Slice_1' (Slice)", "Slice of a constant")


@pytest.mark.parametrize("kw", [dict(add_bias_kv=True), dict(add_zero_attn=True)], ids=ident)
def test_add_bias_kv_and_add_zero_attn_are_refused(nsg, tmp_path, kw):
    refused(nsg, mm.export(mm.make("mha", 32, 2, **kw), tmp_path / "m.onnx"), "node '/att/m/ConstantOfShape' (ConstantOfShape)", "outside the supported op set")


def test_a_sequence_that_is_not_the_81_squares_is_refused(nsg, tmp_path):
    refused(nsg, mm.export(mm.make("mha", 32, 2, squares=40), tmp_path / "m.onnx"), "node '/Slice_1' (Slice)", "Slice along an axis other than the channels")


@pytest.mark.parametrize("need_weights", [False, True])
def test_a_head_dimension_outside_the_rule_keeps_its_wording(nsg, tmp_path, need_weights):
    refused(nsg, mm.export(mm.make("mha", 24, 4, need_weights=need_weights), tmp_path / "m.onnx"), "node '/att/m/Reshape_3' (Reshape)", "head dimension 6")


def test_the_seq_first_rows_feed_the_pattern_only(nsg, tmp_path):
    """A Relu on [81,N,E] (the module's input behind the caller's own transpose): refused with node, op and shape."""
    import torch

    class Net(mm.MhaNet):
        def forward(self, x0):
            x = mm.tokens(torch.tanh(self.stem(x0)))
            return self.heads(x + torch.relu(x.transpose(0, 1)).transpose(0, 1))

    torch.manual_seed(5)
    refused(nsg, mm.export(Net(32, 2).eval(), tmp_path / "m.onnx"), "node '/Relu' (Relu)", "[81,N,32]", "seq-first")


def test_mod_on_a_run_time_tensor_is_still_refused(nsg, tmp_path):
    """Mod folds on the host's shape values only: on a tensor it is refused in the words of an op outside the set."""
    import reduction_models as rm
    n = rm.RNet(nsg)
    n.stem(27, 0)
    n.node("Mod", ["s", n.const("three", [3.0])], "m", name="remainder", fmod=1)
    n.node("Flatten", ["m"], "policy", name="pflat", axis=1)
    n.node("GlobalMaxPool", ["s"], "gm4", name="gmax")
    g = n.node("Flatten", ["gm4"], "gm", name="gmflat", axis=1)
    for o in ("value", "draw"):
        n.node("Gemm", [g, n.const(o + "_w", np.ones((1, 27))), n.const(o + "_b", [0.0])], o, name=o + "_fc", transB=1)
    refused(nsg, n.data(), "node 'remainder' (Mod)", "op 'Mod' is outside the supported op set")
