"""CPU: the SDNet baseline's interface -- state_dict layout of the reference class (tests/golden/gs_sdnet.npz holds the reference's
weights), the drop-in import path, and the refusals of what is not built.  No kernel is launched."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from paif_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ref_sd(golden):
    g = golden("gs_sdnet")
    return {k[3:]: torch.from_numpy(np.asarray(v)) for k, v in g.items() if k.startswith("sd/")}


def test_state_dict_is_the_reference_layout(golden):
    from paif_amd.fusion_model.sdnet import SDNet

    ref = _ref_sd(golden)
    net = SDNet()
    got = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert len(got) == 32
    assert got == {k: tuple(v.shape) for k, v in ref.items()}
    assert got["conv41.0.weight"] == (16, 48, 3, 3) and got["fuse.0.weight"] == (1, 128, 1, 1)
    assert "decom.0.bias" in got and "conv51.0.weight" in got and "conv72.0.bias" in got     # parameter containers only
    net.load_state_dict(ref, strict=True)
    for k, v in net.state_dict().items():
        assert torch.equal(v, ref[k]), k


def test_fixture_records_its_calibration_and_margins(golden):
    """What tools/make_golden_sdnet.py asserted when it wrote the fixtures: the weights leave the linear range, both LeakyReLU branches
    are taken in every map, the composite's clamp is active and inactive, and no pre-activation is close enough to zero for its fp32 sign
    to differ from the float64 sign."""
    g = golden("gs_sdnet")
    assert g["stats_std"].shape == (9,) and np.all((g["stats_std"] >= 0.8) & (g["stats_std"] <= 1.25))
    assert g["stats_negative_share"].shape == (8,) and np.all((g["stats_negative_share"] >= 0.2) & (g["stats_negative_share"] <= 0.8))
    for case, pixels in (("2x24x32", 1536), ("1x37x53", 1961), ("1x13x17", 221), ("1x4x5", 20)):
        start, least, floor, inside = g["case_" + case]
        assert 0 <= start <= 2000 and least >= 2e-5 and least >= 6 * floor, (case, start, least, floor)
        assert pixels < 100 or inside >= 0.4, (case, inside)


def test_drop_in_name_resolves_to_the_native_class():
    """`from fusion_model.SDNet import SDNet` with paif_amd/dropin first on the path."""
    code = ("import fusion_model.SDNet as M, paif_amd.fusion_model.sdnet as N;"
            "assert M.SDNet is N.SDNet; n = M.SDNet(); assert len(n.state_dict()) == 32; print('ok')")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "paif_amd", "dropin"), ROOT]))
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0 and b"ok" in r.stdout, r.stdout.decode(errors="replace")


def test_composite_accepts_the_baseline_and_orders_its_parameters():
    from paif_amd.core.model_fusion_auto import Network_MM_CompModel, grad_milestones
    from paif_amd.fusion_model.sdnet import SDNet

    m = Network_MM_CompModel(SDNet(), None, None, "mit_b0", num_classes=9)
    assert isinstance(m.enhance_net, SDNet)
    assert grad_milestones(m)[-1] is m.enhance_net        # they only walk parameters: the baseline is the last milestone
    assert all(hasattr(p, "_paif_order") for p in m.enhance_net.parameters())


def test_unsupported_requests_say_why():
    from paif_amd.fusion_model.sdnet import SDNet

    net = SDNet()
    z = torch.zeros(1, 1, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):                      # as tests/test_abi.py::test_cpu_tensor_is_refused
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
    """The plane checks come before any pointer is taken (tests/test_sdnet_gpu.py repeats them on device tensors)."""
    from paif_amd.fusion_model.sdnet import SDNet

    class _Dev:   # a stand-in that passes the device check only: dtype and shape are checked on it, nothing is launched
        def __init__(self, shape, dtype=torch.float32):
            self.is_cuda, self.dtype, self.shape, self.device = True, dtype, torch.Size(shape), "cuda:0"

        def dim(self):
            return len(self.shape)

    with pytest.raises(TypeError, match="fp32"):
        SDNet._check_planes(_Dev((1, 1, 8, 8), torch.float16), _Dev((1, 1, 8, 8), torch.float16))
    with pytest.raises(TypeError, match="fp32"):
        SDNet._check_planes(_Dev((1, 1, 8, 8)), _Dev((1, 1, 8, 8), torch.float64))
    with pytest.raises(ValueError, match=r"\[B,1,H,W\]"):
        SDNet._check_planes(_Dev((1, 3, 8, 8)), _Dev((1, 3, 8, 8)))
    with pytest.raises(ValueError, match=r"\[B,1,H,W\]"):
        SDNet._check_planes(_Dev((1, 1, 8, 8)), _Dev((1, 1, 8, 9)))
    with pytest.raises(ValueError, match=r"\[B,1,H,W\]"):
        SDNet._check_planes(_Dev((1, 8, 8)), _Dev((1, 8, 8)))
