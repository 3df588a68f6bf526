"""CPU: the interface of SKFF (paif_amd/operations_m.py) and Fusion_Network2 (paif_amd/fusion_model/skff.py) -- module tree and
state_dict layout as recorded from the reference classes (tests/golden/gk_index.npz), the fixture weights rebuilt from the 22 scales
(paif_amd.synthetic.fn2_state_dict), the drop-in import path, and the refusals of what is not built.  No kernel is launched."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from paif_amd import ops, synthetic as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAD_CASES = ("1x3x5", "1x13x17", "2x9x20", "1x19x18")
SKFF_CASES = [(c, h) for c in ("1x1x1", "1x3x5", "2x9x20", "1x37x53") for h in (2, 3)]


def _layout(module):
    sd = module.state_dict()
    return list(sd.keys()), [",".join(str(s) for s in v.shape) for v in sd.values()]


def test_state_dicts_are_the_recorded_reference_layouts(golden, capsys):
    from paif_amd.core.model_fusion_auto import SKFF, Fusion_Network2
    from paif_amd.fusion_model.drdb import DRDB

    g = golden("gk_index")
    net = Fusion_Network2()
    assert capsys.readouterr().out == ""
    names, shapes = _layout(net)
    assert len(names) == 41 and names == [str(n) for n in g["names_fn2"]] and shapes == [str(s) for s in g["shapes_fn2"]]
    names, shapes = _layout(SKFF(64, 3))
    assert names == [str(n) for n in g["names_skff3"]] and shapes == [str(s) for s in g["shapes_skff3"]]
    assert [n for n, _ in net.named_children()] == ["conv1", "DRDB1", "DRDB2", "conv2", "relu", "skff", "skff2", "conv3", "conv4"]
    assert [n for n, _ in net.skff.named_children()] == ["avg_pool", "conv_du", "fcs", "softmax"]
    assert isinstance(net.DRDB1, DRDB) and isinstance(net.skff, SKFF) and net.skff.height == 2 and len(net.skff2.fcs) == 2
    assert float(net.relu.weight) == 0.25 and float(net.skff.conv_du[1].weight) == 0.25
    # the reference's signature and its d = max(int(C / reduction), 4)
    assert SKFF(64).height == 3 and SKFF(64).conv_du[0].bias is None and tuple(SKFF(64).conv_du[0].weight.shape) == (8, 64, 1, 1)
    assert tuple(SKFF(64, 2, 32, True).fcs[1].weight.shape) == (64, 4, 1, 1) and SKFF(64, 2, 32, True).fcs[1].bias.shape == (64,)
    assert tuple(SKFF(64, 2, 1).conv_du[0].weight.shape) == (64, 64, 1, 1)
    # the order the kernels' pack takes the convs in is the table's
    assert [tuple(c.weight.shape) for c in net._convs()] == [(co, ci, k, k) for _, co, ci, k in S.FN2_CONVS]
    assert len(S.FN2_SCALED) == 22


def test_there_is_one_skff_class():
    import paif_amd.core.model_fusion_auto as C
    import paif_amd.fusion_model.skff as N
    import paif_amd.operations_m as M

    assert C.SKFF is M.SKFF and N.SKFF is M.SKFF and C.Fusion_Network2 is N.Fusion_Network2


def test_rebuilt_fixture_weights_load_strictly(golden):
    from paif_amd.core.model_fusion_auto import SKFF, Fusion_Network2

    g = golden("gk_index")
    assert g["scales"].shape == (22,) and g["scales"].dtype == np.float32
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in S.fn2_state_dict(g["scales"], float(g["shift"]), float(g["last_scale"])).items()}
    assert len(sd) == 41
    net = Fusion_Network2()
    net.load_state_dict(sd, strict=True)
    for k, v in net.state_dict().items():
        assert v.dtype == sd[k].dtype and torch.equal(v, sd[k]), k
    w = S.formula_tensor("hand2/skff2.fcs.1.weight", (64, 8, 1, 1)) * g["scales"][21]
    assert np.array_equal(sd["skff2.fcs.1.weight"].numpy(), w)
    for case, height in SKFF_CASES:
        f = golden("gk_skff_%s_h%d" % (case, height))
        m = SKFF(64, height, int(f["reduction"]), bool(f["bias"]))
        m.load_state_dict({k: torch.from_numpy(v) for k, v in S.skff_state_dict(f["scales"], height, int(f["reduction"]), bool(f["bias"])).items()},
                          strict=True)
    assert any(bool(golden("gk_skff_%s_h%d" % c)["bias"]) for c in SKFF_CASES)


def test_fixture_records_its_calibration_margins_and_coupling(golden):
    """What tools/make_golden_skff.py asserted when it wrote the fixtures."""
    g = golden("gk_index")
    assert g["stats_std"].shape == (22,) and np.all((g["stats_std"] >= 0.8) & (g["stats_std"] <= 1.25))
    assert g["stats_negative_share"].shape == (16,) and np.all((g["stats_negative_share"] >= 0.2) & (g["stats_negative_share"] <= 0.8))
    assert np.all(g["stats_attention_std"] >= 0.1)
    for case in GRAD_CASES:
        rec = g["case_" + case]
        start, least, floor, gap_mn, gap_mx = rec[:5]
        assert 0 <= start <= 2000 and least >= 2e-5 and least >= 6 * floor and gap_mn > 0 and gap_mx > 0
        cpl = rec[7:].reshape(4, 2)
        assert np.all(cpl[:, 0] >= 100 * cpl[:, 1]), (case, cpl)           # the coupling condition, per gradient
        f = golden("gk_fn2_" + case)
        assert int((f["fused64"] == 0).sum()) == 1 and int((f["fused64"] == 1).sum()) == 1
        assert f["d_out164"].dtype == np.float64 and f["floor_d_out2"].dtype == np.float32
    assert g["case_2x9x20"][5] != g["case_2x9x20"][6]                      # min and max in different images
    for case in ("1x37x53", "2x24x32"):
        assert "d_i1" not in golden("gk_fn2_" + case)
    for case in ("1x3x5", "1x13x17"):
        keys = [k for p in range(int(g["maps_parts_" + case][0])) for k in golden("gk_fn2_%s_maps%d" % (case, p))
                if k.startswith("map") and k != "map_floor"]
        assert sorted(keys, key=lambda k: int(k[3:])) == ["map%d" % k for k in range(20)]
    for case, height in SKFF_CASES:
        f = golden("gk_skff_%s_h%d" % (case, height))
        least, floor = f["stats"][1:3]
        cpl = f["stats"][3:].reshape(height, 2)
        assert least >= 2e-5 and least >= 6 * floor and np.all(cpl[:, 0] >= 100 * cpl[:, 1]), (case, height)
        assert "x0" not in f and len(f["seeds"]) == height              # the seeds are stored, not the maps


def test_drop_in_names_resolve_to_the_native_classes():
    """`from operations_m import SKFF` and `from core.model_fusion_auto import SKFF, Fusion_Network2` with paif_amd/dropin first on the
    path, in a fresh interpreter."""
    code = ("import operations_m as O, core.model_fusion_auto as M, paif_amd.operations_m as P, paif_amd.fusion_model.skff as N;"
            "from operations_m import SKFF;"
            "from core.model_fusion_auto import SKFF as S2, Fusion_Network2;"
            "assert SKFF is P.SKFF and S2 is P.SKFF and O.SKFF is P.SKFF and Fusion_Network2 is N.Fusion_Network2;"
            "assert len(Fusion_Network2().state_dict()) == 41; print('ok')")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "paif_amd", "dropin"), ROOT]))
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0 and b"ok" in r.stdout, r.stdout.decode(errors="replace")


def test_unbuilt_skff_arguments_name_the_argument():
    from paif_amd.operations_m import SKFF

    with pytest.raises(NotImplementedError, match="in_channels"):
        SKFF(32)
    with pytest.raises(NotImplementedError, match="height"):
        SKFF(64, height=4)
    with pytest.raises(NotImplementedError, match="height"):
        SKFF(64, height=1)
    with pytest.raises(NotImplementedError, match="reduction"):
        SKFF(64, 2, reduction=0.5)


def test_unsupported_requests_say_why():
    from paif_amd.core.model_fusion_auto import SKFF, Fusion_Network2

    m, x = SKFF(64, 2), torch.zeros(1, 64, 4, 4)
    with pytest.raises(NotImplementedError, match="[Pp]arameter gradients.*freeze the parameters"):
        m([x, x])
    with torch.no_grad():
        with pytest.raises(ValueError, match="list of 2"):
            m([x, x, x])
        with pytest.raises(ValueError, match="list of 2"):
            m(x)
        with pytest.raises(RuntimeError, match="no CPU path"):
            m([x, x])
    with pytest.raises(RuntimeError, match="no CPU path"):                       # inside an attack: the maps are looked at
        with ops.no_param_grads():
            m([x, x])
    net = Fusion_Network2()
    z, o1, o2 = torch.zeros(1, 1, 8, 8), torch.zeros(1, 64, 8, 8), torch.zeros(1, 128, 8, 8)
    with pytest.raises(NotImplementedError, match="[Pp]arameter gradients.*freeze the parameters"):
        net(z, z, o1, o2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        with torch.no_grad():
            net(z, z, o1, o2)
    assert not hasattr(net, "forward_impl")                                      # not a NativeFusion: no composite protocol


def test_checks_come_in_the_order_device_dtype_shape():
    from paif_amd.core.model_fusion_auto import SKFF, Fusion_Network2

    class _Dev:   # a stand-in that passes the device check only: dtype and shape are checked on it, nothing is launched
        def __init__(self, shape, dtype=torch.float32, is_cuda=True):
            self.is_cuda, self.dtype, self.shape, self.device = is_cuda, dtype, torch.Size(shape), "cuda:0" if is_cuda else "cpu"

        def dim(self):
            return len(self.shape)

    ok, o1, o2 = _Dev((1, 1, 8, 8)), _Dev((1, 64, 8, 8)), _Dev((1, 128, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU path"):                       # the device before the dtype
        Fusion_Network2._check(ok, ok, _Dev((1, 64, 8, 8), torch.float16), _Dev((1, 128, 8, 8), is_cuda=False))
    with pytest.raises(TypeError, match="fp32"):                                 # the dtype before the shape
        Fusion_Network2._check(ok, ok, _Dev((1, 64, 8, 9), torch.float16), o2)
    with pytest.raises(ValueError, match=r"\[B,1,H,W\]"):
        Fusion_Network2._check(ok, _Dev((1, 1, 8, 9)), o1, o2)
    with pytest.raises(ValueError, match=r"out1 \[B,64,H,W\]"):
        Fusion_Network2._check(ok, ok, _Dev((1, 32, 8, 8)), o2)
    with pytest.raises(ValueError, match=r"out2 \[B,128,H,W\]"):
        Fusion_Network2._check(ok, ok, o1, _Dev((1, 128, 8, 9)))
    Fusion_Network2._check(ok, ok, o1, o2)
    m = SKFF(64, 2)
    with pytest.raises(TypeError, match="fp32"):
        m._check([_Dev((1, 64, 4, 4), torch.float16), _Dev((1, 64, 4, 5))])
    with pytest.raises(ValueError, match="one shape"):
        m._check([_Dev((1, 64, 4, 4)), _Dev((1, 64, 4, 5))])
    with pytest.raises(ValueError, match="one shape"):
        m._check([_Dev((1, 32, 4, 4)), _Dev((1, 32, 4, 4))])


def test_a_negative_relu_slope_is_refused_before_anything_is_packed():
    """The reverse pass reads the branch of conv1's and conv2's PReLU off the taped output: right for slopes >= 0 only.  The check runs on
    the host value, before the first device call.  The gates' own slope may have any sign: their branch is read off the taped z."""
    convs = [(torch.zeros(co, ci, k, k), torch.zeros(co)) for _, co, ci, k in S.FN2_CONVS]
    with pytest.raises(ValueError, match="slope"):
        ops.fn2_pack(convs, torch.tensor([-0.1]), None, None)
    with pytest.raises(ValueError, match="slope"):
        ops.fn2_pack(convs, float("nan"), None, None)
    with pytest.raises(ValueError, match="sixteen"):
        ops.fn2_pack(convs[:15], 0.25, None, None)
