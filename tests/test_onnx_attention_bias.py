"""The general graph path's host half on attention with a bias computed at run time (DESIGN.md section 13.3;
nsg_inspect_onnx): the three generator forms of tests/attention_bias_models.py plan with one attention launch per
block, the token -> flat, flat -> head rows and score-bias views cost no launch, the FLOP count includes the
generator's dense layers, and what the pattern does not take is refused with the node's name and the reason.  Before
this feature every model here was refused (NSG_E_FORMAT at the generator's Flatten, the first of the new views).  No
device needed."""
import numpy as np
import pytest

import attention_bias_models as abm

gen = abm.gen


def export(net, tmp_path, name="m.onnx"):
    return gen.export_model(net.eval(), str(tmp_path / name))


def refused(nsg, data, *needles):
    with pytest.raises(nsg.NsgError) as e:
        nsg.inspect_onnx(data, 86)
    assert e.value.code == -4, e.value
    for n in needles:
        assert n in str(e.value), str(e.value)


VARIANTS = [dict(), dict(bias=True), dict(bias=True, rt_first=True), dict(bias=True, swap=True), dict(scale_on="q"),
            dict(scale_on="k", bias=True), dict(mul_behind=0.5), dict(bias=True, mul_behind=0.5, rt_first=True, swap=True)]


@pytest.mark.parametrize("form", ["A", "B", "C"])
@pytest.mark.parametrize("kw", VARIANTS, ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()) or "plain")
def test_the_generator_forms_plan_with_one_attention_launch(nsg, tmp_path, form, kw):
    net = abm.build(32, 4, 7, form=form, **kw)
    info = nsg.inspect_onnx(export(net, tmp_path), 86)
    assert info["path"] == "graph" and info["precision"] == "fp32"
    assert info["attention_launches"] == 1
    # AttNet's launches (stem, QKV, attention, projection + residual, policy, mean, value, draw, planes, outputs), and
    # the generator's: the token Linear, Linear + swish, then A / B: one Linear; C: Linear, LayerNorm, the shared
    # Linear over the head rows.  The Flatten of the tokens, the Reshape to head rows and the Reshape to [N,H,81,81]
    # cost nothing, and neither do the scalar factors or the constant bias wherever they stand.
    generator = 1 + 1 + (1 if form in "AB" else 3)
    assert info["launches"] == 1 + 1 + 1 + 1 + 1 + 1 + 2 + 2 + generator == net.launches()
    assert info["conv_launches"] == 1 + 1 + 1 + 1 + 2 + generator - (1 if form == "C" else 0)
    F, H, d, comp, hidden, K = 32, 4, 8, 16, 32, 16
    flops = 2 * 81 * 9 * 86 * F + 2 * 81 * (F * 3 * F + F * F) + 2 * (2 * 81 * 81 * d) * H + 2 * 81 * F * 27 + 2 * 2 * F
    flops += 2 * 81 * F * comp + 2 * 81 * comp * hidden
    flops += {"A": 2 * hidden * 6561, "B": 2 * hidden * H * 6561, "C": 2 * hidden * H * K + 2 * H * K * 6561}[form]
    assert info["flops_per_position"] == flops == net.flops()


def test_one_head_of_width_64_plans(nsg, tmp_path):
    info = nsg.inspect_onnx(export(abm.build(64, 1, 8, form="C", bias=True), tmp_path), 86)
    assert info["path"] == "graph" and info["attention_launches"] == 1 and info["launches"] == 10 + 5


def test_two_blocks_are_two_attention_launches(nsg, tmp_path):
    import torch

    class Two(abm.BiasNet):
        def __init__(self):
            super().__init__(32, 4, form="C")
            self.att2 = abm.BiasAttention(32, 4, form="A", bias=True)

        def forward(self, x):
            x = gen.tokens(torch.tanh(self.stem(x)))
            x = x + self.att(x)
            x = x + self.att2(x)
            return self.p(x).transpose(1, 2).reshape(x.size(0), 2187), torch.sigmoid(self.fc_v(x.mean(dim=1))), \
                torch.sigmoid(self.fc_d(x.mean(dim=1)))

    torch.manual_seed(3)
    info = nsg.inspect_onnx(export(Two(), tmp_path), 86)
    assert info["path"] == "graph" and info["attention_launches"] == 2
    assert info["launches"] == 10 + 5 + (1 + 1 + 1) + 3  # the second block: QKV, attention, projection, and generator A


def test_refusals_name_the_node_and_the_reason(nsg, tmp_path):
    # a token flatten whose rows are not contiguous: C = 24
    refused(nsg, export(abm.build(32, 4, 1, form="A", gen_kw=dict(comp=24)), tmp_path), "node '/att/gen/Flatten'",
            "[N,81,24]", "multiple of 16")
    # head rows of K = 24
    refused(nsg, export(abm.build(32, 4, 1, form="C", gen_kw=dict(K=24)), tmp_path), "node '/att/gen/Reshape'",
            "[N,4,24]", "K = 24")
    # a second run-time Add
    refused(nsg, export(abm.build(32, 4, 1, form="B", tweak="second_rt"), tmp_path), "node '/att/Add_2'", "second run-time Add")
    # Relu on the 4-D bias view
    refused(nsg, export(abm.build(32, 4, 1, form="B", tweak="relu_bias"), tmp_path), "node '/att/Relu'", "Relu",
            "[N,4,81,81]", "run-time attention bias")
    # the bias view read by a second consumer
    refused(nsg, export(abm.build(32, 4, 1, form="B", tweak="bias_twice"), tmp_path), "node '/att/Add_1'", "more than one consumer")


def test_hand_built_refusals(nsg):
    # a bias of 2 heads on scores of 4
    refused(nsg, abm.RtAttCase(nsg, 64, 4, kind="flat", heads=2).data, "node 'rt_into_scores'", "2 heads", "[N,4,81,81]")
    refused(nsg, abm.RtAttCase(nsg, 64, 4, kind="rows", heads=2).data, "node 'rt_into_scores'", "2 heads")
    # the same bias view added twice: refused at the first Add, whose operand has a second consumer
    refused(nsg, abm.RtAttCase(nsg, 64, 4, kind="rows", second=True).data, "node 'rt_into_scores'", "more than one consumer")
    # a run-time tensor of another kind added to the scores: the flat generator output itself
    refused(nsg, abm.RtAttCase(nsg, 64, 1, kind="broadcast", other=True).data, "node 'rt_into_scores'", "run-time tensor [N,6561]",
            "[N,1,81,81]")
    # a factor that is not positive behind the run-time Add would turn a closed key's -inf into +inf or NaN
    refused(nsg, abm.RtAttCase(nsg, 64, 4, kind="flat", rt_scale=-0.5).data, "node 'rt_mul'", "positive factor")
    refused(nsg, abm.RtAttCase(nsg, 64, 4, kind="flat", rt_scale=0.0).data, "node 'rt_mul'", "positive factor")
    # the near-direct cases themselves plan: one attention launch, the views free
    for kind in abm.RT_KINDS:
        info = nsg.inspect_onnx(abm.RtAttCase(nsg, 64, 4, kind=kind, rt_scale=0.5).data, 86)
        assert info["path"] == "graph" and info["attention_launches"] == 1, kind
        # stem, global max, generator dense, attention, select, mean, value, draw + planes + outputs
        assert info["launches"] == 1 + 1 + 1 + 1 + 1 + 1 + 2 + 2, (kind, info["launches"])


def test_truncated_models_are_errors_not_crashes(nsg, tmp_path):
    data = export(abm.build(32, 4, 2, form="C", bias=True), tmp_path)
    assert nsg.inspect_onnx(data, 86)["path"] == "graph"
    for cut in np.linspace(1, len(data) - 1, 20).astype(int):
        with pytest.raises(nsg.NsgError):
            nsg.inspect_onnx(data[:cut], 86)
