"""CPU: the SeAFusion baseline's interface -- state_dict layout of the reference class (72 entries, the decoder's unused BatchNorm
included), the fixture weights rebuilt from tests/golden/gs_seafusion.npz (thirty scales and one shift:
paif_amd.synthetic.seafusion_state_dict), the drop-in import path, and the refusals of what is not built.  No kernel is launched."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from paif_amd import ops, synthetic as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAD_CASES = ("1x4x5", "1x13x17", "2x9x20", "1x5x37", "1x19x18")


def _want_shapes():
    want = {}
    for s in ("vis", "inf"):
        want[s + "_conv.conv.weight"], want[s + "_conv.conv.bias"] = (16, 1, 3, 3), (16,)
        for r, c, co in ((1, 16, 32), (2, 32, 48)):
            p = "%s_rgbd%d." % (s, r)
            want[p + "dense.conv1.conv.weight"], want[p + "dense.conv1.conv.bias"] = (c, c, 3, 3), (c,)
            want[p + "dense.conv2.conv.weight"], want[p + "dense.conv2.conv.bias"] = (c, 2 * c, 3, 3), (c,)
            want[p + "convdown.conv.weight"], want[p + "convdown.conv.bias"] = (co, 3 * c, 1, 1), (co,)
            want[p + "sobelconv.convx.weight"] = want[p + "sobelconv.convy.weight"] = (c, 1, 3, 3)      # no bias
            want[p + "convup.conv.weight"], want[p + "convup.conv.bias"] = (co, c, 1, 1), (co,)
    for name, co, ci in (("decode4", 64, 96), ("decode3", 32, 64), ("decode2", 16, 32), ("decode1", 1, 16)):
        want[name + ".conv.weight"], want[name + ".conv.bias"] = (co, ci, 3, 3), (co,)
        for leaf in ("weight", "bias", "running_mean", "running_var"):
            want["%s.bn.%s" % (name, leaf)] = (co,)
        want[name + ".bn.num_batches_tracked"] = ()
    return want


def _fixture_sd(golden):
    g = golden("gs_seafusion")
    return {k: torch.from_numpy(np.asarray(v)) for k, v in S.seafusion_state_dict(g["scales"], g["shift"]).items()}


def test_state_dict_is_the_reference_layout():
    from paif_amd.fusion_model import seafusion as M

    net = M.SeaFusion()
    got = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    want = _want_shapes()
    assert len(got) == 72 and got == want and list(got) == list(net.state_dict())
    assert sum(p.numel() for p in net.parameters()) == 166883
    assert sum(v.numel() for k, v in net.state_dict().items() if ".conv" in k and k.endswith("weight")) == 166000
    assert len([k for k in got if ".bn." in k]) == 20
    assert isinstance(net.vis_rgbd1, M.RGBD) and isinstance(net.vis_rgbd1.dense, M.DenseBlock) and isinstance(net.inf_conv, M.ConvLeakyRelu2d)
    assert isinstance(net.vis_rgbd2.sobelconv, M.Sobelxy) and isinstance(net.inf_rgbd1.convup, M.Conv1)
    assert isinstance(net.decode4, M.ConvBnLeakyRelu2d) and isinstance(net.decode1, M.ConvBnTanh2d)
    # the reference's initialisation: trainable Sobel stencils
    sob = torch.tensor([[1., 0., -1.], [2., 0., -2.], [1., 0., -1.]])
    for blk, c in ((net.vis_rgbd1, 16), (net.inf_rgbd2, 32)):
        assert torch.equal(blk.sobelconv.convx.weight, sob.expand(c, 1, 3, 3)) and torch.equal(blk.sobelconv.convy.weight, sob.t().expand(c, 1, 3, 3))
        assert blk.sobelconv.convx.weight.requires_grad and blk.sobelconv.convx.bias is None
    # the order the kernels' pack takes the convs in is the table's
    assert [tuple(c.weight.shape) for c in net._convs()] == [(co, ci, k, k) for _, co, ci, k, _ in S.SEAFUSION_CONVS]
    assert [c.bias is not None for c in net._convs()] == [b for _, _, _, _, b in S.SEAFUSION_CONVS]


def test_rebuilt_fixture_weights_load_strictly(golden):
    from paif_amd.fusion_model.seafusion import SeaFusion

    g = golden("gs_seafusion")
    assert g["scales"].shape == (30,) and g["scales"].dtype == np.float32 and g["shift"].dtype == np.float32
    sd = _fixture_sd(golden)
    assert len(sd) == 72 and sum(v.numel() for k, v in sd.items() if ".conv" in k and k.endswith("weight")) == 166000
    net = SeaFusion()
    net.load_state_dict(sd, strict=True)
    for k, v in net.state_dict().items():
        assert v.dtype == sd[k].dtype and torch.equal(v, sd[k]), k
    # the expression: formula tensor times the conv's scale, weight and bias alike; the shift on the last bias only
    names = [n for n, _, _, _, _ in S.SEAFUSION_CONVS]
    k = names.index("inf_rgbd2.sobelconv.convy")
    w = S.formula_tensor("sea/inf_rgbd2.sobelconv.convy.weight", (32, 1, 3, 3)) * g["scales"][k]
    assert np.array_equal(sd["inf_rgbd2.sobelconv.convy.weight"].numpy(), w)
    sob = np.array([[1., 0., -1.], [2., 0., -2.], [1., 0., -1.]], dtype=np.float32)
    assert np.abs(w / np.abs(w).max() - sob.T / 2).max() > 0.1                      # a general depthwise filter, not the stencil
    b = S.formula_tensor("sea/decode1.conv.bias", (1,)) * g["scales"][29] + g["shift"]
    assert np.array_equal(sd["decode1.conv.bias"].numpy(), b)
    # the unused BatchNorm entries are not the identity: folding them in by mistake would show
    assert float((sd["decode3.bn.running_mean"]).abs().max()) > 0.01 and float(sd["decode3.bn.running_var"].min()) > 0
    assert float((sd["decode3.bn.weight"] - 1).abs().max()) > 0.01


def test_fixture_records_its_calibration_and_margins(golden):
    """What tools/make_golden_seafusion.py asserted when it wrote the fixtures: every conv's output has unit scale, both branches are taken
    at each of the 25 sign points, the tanh is neither linear nor saturated on the calibration planes, and in the five gradient cases none
    of the 688 sign points per pixel is close enough to zero for its fp32 sign to differ from the float64 sign."""
    g = golden("gs_seafusion")
    assert g["stats_std"].shape == (30,) and np.all((g["stats_std"] >= 0.8) & (g["stats_std"] <= 1.25))
    assert g["stats_negative_share"].shape == (25,) and np.all((g["stats_negative_share"] >= 0.2) & (g["stats_negative_share"] <= 0.8))
    assert 0.4 <= float(g["stats_inside"]) < 1.0
    for case in GRAD_CASES:
        start, least, floor = g["case_" + case][:3]
        assert 0 <= start <= 2000 and least >= 2e-5 and least >= 6 * floor, (case, start, least, floor)
        assert "d_i164" in golden("gs_seafusion_" + case)
    for case in ("1x37x53", "2x24x32"):       # forward only: the margin condition is out of reach at these sizes
        assert g["case_" + case][0] == 0 and "d_i1" not in golden("gs_seafusion_" + case)
        assert g["case_" + case][4] <= 0.01   # the share the taped-branch test leaves out, on the reference's own float32 run
    for case in ("1x4x5", "1x13x17"):
        keys = [k for p in (0, 1) for k in golden("gs_seafusion_%s_maps%d" % (case, p)) if k.startswith("map") and k != "map_floor"]
        assert sorted(keys, key=lambda k: int(k[3:])) == ["map%d" % k for k in range(21)]
    a = golden("gs_seafusion_attack")
    assert np.all(a["f32_vs_f64"] <= 1e-3) and 0 <= int(a["start"]) <= 2000


def test_drop_in_name_resolves_to_the_native_class():
    """`from fusion_model.SeaFusion import SeaFusion` with paif_amd/dropin first on the path."""
    code = ("import fusion_model.SeaFusion as M, paif_amd.fusion_model.seafusion as N;"
            "assert all(getattr(M, n) is getattr(N, n) for n in ('SeaFusion', 'RGBD', 'DenseBlock', 'Sobelxy', 'Conv1', 'ConvLeakyRelu2d', "
            "'ConvBnLeakyRelu2d', 'ConvBnTanh2d')); n = M.SeaFusion(); assert len(n.state_dict()) == 72; print('ok')")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "paif_amd", "dropin"), ROOT]))
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0 and b"ok" in r.stdout, r.stdout.decode(errors="replace")


def test_composite_accepts_the_baseline_and_orders_its_parameters():
    from paif_amd.core.model_fusion_auto import Network_MM_CompModel, grad_milestones
    from paif_amd.fusion_model.seafusion import SeaFusion

    m = Network_MM_CompModel(SeaFusion(), None, None, "mit_b0", num_classes=9)
    assert isinstance(m.enhance_net, SeaFusion)
    assert grad_milestones(m)[-1] is m.enhance_net        # they only walk parameters: the baseline is the last milestone
    assert all(hasattr(p, "_paif_order") for p in m.enhance_net.parameters())


def test_unsupported_requests_say_why():
    from paif_amd.fusion_model.seafusion import SeaFusion

    net = SeaFusion()
    z = torch.zeros(1, 1, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        with torch.no_grad():
            net(z, z)
    with pytest.raises(RuntimeError, match="no CPU path"):
        net.forward_impl(z, z)
    with pytest.raises(NotImplementedError, match="[Pp]arameter gradients"):    # a forward that wants parameter gradients
        net(z, z)
    with pytest.raises(RuntimeError, match="no CPU path"):                      # ... but not inside an attack: the planes are looked at
        with ops.no_param_grads():
            net(z, z)
    with pytest.raises(NotImplementedError, match="wgrad"):
        net.backward_impl(z, {}, wgrad=True)
    with pytest.raises(NotImplementedError, match="[Pp]arameter gradients"):    # a tape for the parameter-gradient kernels
        with ops.tape_mode("wgrad"):
            net.forward_impl(z, z, tape={})
    with pytest.raises(NotImplementedError, match="inter"):
        net.forward_impl(z, z, inter=[])


def test_wrong_dtypes_and_shapes_are_refused():
    """The plane checks come before any pointer is taken (tests/test_seafusion_gpu.py repeats them on device tensors)."""
    from paif_amd.fusion_model.seafusion import SeaFusion

    class _Dev:   # a stand-in that passes the device check only: dtype and shape are checked on it, nothing is launched
        def __init__(self, shape, dtype=torch.float32):
            self.is_cuda, self.dtype, self.shape, self.device = True, dtype, torch.Size(shape), "cuda:0"

        def dim(self):
            return len(self.shape)

    with pytest.raises(TypeError, match="fp32"):
        SeaFusion._check_planes(_Dev((1, 1, 8, 8), torch.float16), _Dev((1, 1, 8, 8), torch.float16))
    with pytest.raises(TypeError, match="fp32"):
        SeaFusion._check_planes(_Dev((1, 1, 8, 8)), _Dev((1, 1, 8, 8), torch.float64))
    with pytest.raises(ValueError, match=r"\[B,1,H,W\]"):
        SeaFusion._check_planes(_Dev((1, 3, 8, 8)), _Dev((1, 3, 8, 8)))
    with pytest.raises(ValueError, match=r"\[B,1,H,W\]"):
        SeaFusion._check_planes(_Dev((1, 1, 8, 8)), _Dev((1, 1, 8, 9)))
    with pytest.raises(ValueError, match=r"\[B,1,H,W\]"):
        SeaFusion._check_planes(_Dev((1, 8, 8)), _Dev((1, 8, 8)))
