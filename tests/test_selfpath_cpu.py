"""CPU: the interface of the SelAttention primitive (paif_amd.operations_m.SelfPath / Attention) -- module tree and state_dict layout of the
reference classes (10 entries), the registry and MixedOp's three-field name, the drop-in import path, the refusals of what is not built,
the calibration figures the fixtures record (tools/make_golden_selfpath.py), and the plain-torch restatement (tests/selfpath_eager.py)
against every fixture in float64.  No kernel is launched."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from paif_amd import ops, synthetic as S
from tests import selfpath_eager as E
from tests.helpers import t

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"1x3x5_k2": (1, 3, 5, 2), "1x13x17_k2": (1, 13, 17, 2), "2x9x20_k1": (2, 9, 20, 1), "1x19x29_k3": (1, 19, 29, 3),
         "1x16x32_k2": (1, 16, 32, 2)}
KEYS = ["conv.weight", "conv.bias", "conv2.weight", "conv2.bias", "cross_attn.to_qkv.weight", "cross_attn.to_out.0.weight",
        "cross_attn.to_out.0.bias", "norm1.weight", "norm1.bias", "prelu.weight"]


@pytest.mark.parametrize("heads", [1, 2, 3, 8])
def test_state_dict_is_the_reference_layout(golden, heads):
    from paif_amd.operations_m import Attention, SelfPath

    op = SelfPath(32, num_heads=heads)
    got = {k: tuple(v.shape) for k, v in op.state_dict().items()}
    assert list(got) == KEYS and got == S.selfpath_shapes(heads)
    assert got["cross_attn.to_qkv.weight"] == (192 * heads, 32) and got["cross_attn.to_out.0.weight"] == (32, 64 * heads)
    assert [n for n, _ in op.named_children()] == ["conv", "conv2", "act1", "cross_attn", "norm1", "prelu"]
    assert isinstance(op.cross_attn, Attention) and isinstance(op.cross_attn.to_out, nn.Sequential) and isinstance(op.act1, nn.ReLU)
    assert isinstance(op.norm1, nn.LayerNorm) and op.norm1.eps == 1e-5 and float(op.prelu.weight) == 0.25
    assert op.cross_attn.heads == heads and op.cross_attn.scale == 0.125
    gain = float(golden("gs_selfpath")["gain_k%d" % min(heads, 3)])
    sd = {k: t(v) for k, v in S.selfpath_state_dict(heads, gain).items()}
    op.load_state_dict(sd, strict=True)
    for k, v in op.state_dict().items():
        assert torch.equal(v, sd[k]), k
    # the expression: formula tensors of salt 13 under MixedOp's "_op." prefix, the q and k rows times the gain
    w = S.formula_tensor("_op.cross_attn.to_qkv.weight", (192 * heads, 32), 13)
    assert np.array_equal(sd["cross_attn.to_qkv.weight"][128 * heads:].numpy(), w[128 * heads:])
    assert np.array_equal(sd["cross_attn.to_qkv.weight"][:128 * heads].numpy(), w[:128 * heads] * np.float32(gain))


def test_registry_and_three_field_name():
    from paif_amd.core.model_fusion_auto import MixedOp
    from paif_amd.operations_m import OPS, SelfPath

    assert len(OPS) == 7
    op = OPS["SelAttention"](32, 4, 2, False)
    assert isinstance(op, SelfPath) and op.cross_attn.heads == 4
    m = MixedOp(32, "SelAttention_2_1")
    assert isinstance(m._op, SelfPath) and m._op.cross_attn.heads == 2 and len(m.state_dict()) == 10
    assert isinstance(MixedOp(32, "SelAttention_3_2")._op, SelfPath)          # the dilation field is parsed and ignored
    with pytest.raises(IndexError):
        MixedOp(32, "SelAttention_2")
    assert not getattr(m._op, "takes_out_f32", False) and not getattr(m._op, "takes_cpool", False) and not m.bwd_takes_res


def test_dropin_import():
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import operations_m as M\n"
            "ns = {}; exec('from operations_m import *', ns)\n"
            "assert M.__file__.startswith(%r)\n"
            "assert ns['SelfPath'] is M.SelfPath and ns['Attention'] is M.Attention\n"
            "assert isinstance(M.OPS['SelAttention'](32, 2, 1, False), M.SelfPath)\n"
            "print('OK')\n" % (ROOT, os.path.join(ROOT, "paif_amd", "dropin"), os.path.join(ROOT, "paif_amd")))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "OK" in out.stdout, out.stderr[-2000:]


def test_refusals():
    from paif_amd.operations_m import Attention, SelfPath

    for kw, name in ((dict(dim=64), "dim"), (dict(dim=32, reduction=2), "reduction"), (dict(dim=32, num_heads=0), "num_heads"),
                     (dict(dim=32, norm_layer=nn.BatchNorm1d), "norm_layer")):
        with pytest.raises(NotImplementedError, match=r"SelfPath\(%s=" % name):
            SelfPath(**kw)
    for kw, name in ((dict(dim=16), "dim"), (dict(dim=32, heads=0), "heads"), (dict(dim=32, dim_head=32), "dim_head"),
                     (dict(dim=32, dropout=0.1), "dropout")):
        with pytest.raises(NotImplementedError, match=r"Attention\(%s=" % name):
            Attention(**kw)
    op = SelfPath(32, num_heads=2).eval()
    x = torch.zeros(1, 32, 6, 7)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="no CPU path"):
            op(x)
        with pytest.raises(RuntimeError, match="no CPU path"):
            op.train()(x)
        op.eval()
    with pytest.raises(NotImplementedError, match="parameter gradients .* are not built -- freeze the parameters"):
        op(x)                            # autograd is recording and the parameters require grad: the training step's case
    with pytest.raises(NotImplementedError, match="parameter gradients .* are not built -- freeze the parameters"):
        op(x.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError, match="parameter gradients"):
        op.backward_nhwc(x, {}, wgrad=True)
    with ops.tape_mode("wgrad"), pytest.raises(NotImplementedError, match="parameter gradients"):
        op.forward_nhwc(x.permute(0, 2, 3, 1), (), [])
    with ops.no_param_grads():          # the attack path: reaches the kernels, which have no CPU path
        with pytest.raises(RuntimeError, match="no CPU path"):
            op(x.clone().requires_grad_(True))
        with torch.no_grad():
            op.prelu.weight.fill_(-0.1)
        with pytest.raises(NotImplementedError, match="negative PReLU slope"):
            op(x.clone().requires_grad_(True))
    with pytest.raises(RuntimeError):
        op.cross_attn(torch.zeros(1, 5, 32))


def test_fixtures_record_their_calibration(golden):
    g = golden("gs_selfpath")
    assert sorted(k for k in g if k.startswith("gain")) == ["gain_k1", "gain_k2", "gain_k3"]
    for name, (B, H, W, heads) in CASES.items():
        start, least, floor, std, smax, ent, vstd, tiles = g["case_" + name]
        assert 0 <= start <= 2000 and least >= 2e-5 and least >= 6 * floor
        assert 2.0 <= std <= 3.5 and smax >= 8
        assert (H, W) == (3, 5) or 0.25 <= ent <= 0.8
        assert vstd >= 0.1
        assert H * W < 96 or tiles >= 3
        c = golden("gs_selfpath_" + name)
        assert int(c["start"]) == int(start) and c["x"].shape == (B, 32, H, W) and c["x"].dtype == np.float32 and c["out64"].dtype == np.float64
        assert np.array_equal(c["x"], S.make_smooth_feature(11 + int(start), B, 32, H, W)) and np.array_equal(c["x64"], c["x"].astype(np.float64))
        for k in ("x", "out", "out64", "cot", "d_x", "d_x64"):
            assert c[k].shape == (B, 32, H, W)
        assert "conv.weight" not in c          # inputs, outputs and the gain: no weights
    m0, m1 = golden("gs_selfpath_1x13x17_k2_maps0"), golden("gs_selfpath_1x13x17_k2_maps1")
    assert list(m0["map_names"]) == ["tok", "qkv", "o", "lse", "v1", "ln"] and m0["map_floor"].shape == (6,)
    assert m0["qkv"].shape == (1, 221, 384) and m1["o"].shape == (1, 221, 128) and m1["lse"].shape == (1, 2, 221)


@pytest.mark.parametrize("case", list(CASES))
def test_eager_restatement_reproduces_the_fixtures(golden, case):
    B, H, W, heads = CASES[case]
    c = golden("gs_selfpath_" + case)
    sd = E.state(S.selfpath_state_dict(heads, float(golden("gs_selfpath")["gain_k%d" % heads])), torch.float64)
    x = t(c["x64"]).requires_grad_(True)
    taps = {}
    out = E.selfpath(x, sd, heads, taps)
    (out * t(c["cot"]).double()).sum().backward()
    for mine, ref in ((out.detach(), c["out64"]), (x.grad, c["d_x64"])):
        assert float((mine - t(ref)).abs().max()) <= 1e-11 * max(1.0, float(np.abs(ref).max()))
    if case == "1x13x17_k2":
        m0, m1 = golden("gs_selfpath_1x13x17_k2_maps0"), golden("gs_selfpath_1x13x17_k2_maps1")
        for k in ("tok", "qkv", "o", "lse", "v1", "ln"):
            ref = t(m0[k] if k in m0 else m1[k])
            assert float((taps[k].detach() - ref).abs().max()) <= 1e-11 * max(1.0, float(ref.abs().max())), k
