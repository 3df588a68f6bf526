"""CPU: the ReCoNet baseline's interface -- state_dict layout of the reference class (tests/golden/gr_reconet.npz holds the reference's
weights), the drop-in import path, and the refusals of what is not built.  No kernel is launched."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {"d3c16": (3, 16, False), "d2c16bn": (2, 16, True), "d3c64": (3, 64, False)}


def _ref_sd(golden, key):
    g = golden("gr_reconet")
    pre = "sd_%s/" % key
    return {k[len(pre):]: torch.from_numpy(np.asarray(v)) for k, v in g.items() if k.startswith(pre)}   # 0-d entries stay 0-d


@pytest.mark.parametrize("key", sorted(CONFIGS))
def test_state_dict_is_the_reference_layout(golden, key):
    from paif_amd.fusion_model.reconet import ReCoNet

    ref = _ref_sd(golden, key)
    net = ReCoNet(*CONFIGS[key])
    got = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert got == {k: tuple(v.shape) for k, v in ref.items()}
    assert "att_a_conv.weight" in got and "decoder.conv_s.0.bias" in got and "decoder.conv_d.2.group.0.weight" in got
    assert ("decoder.conv_d.1.group.1.running_var" in got) == CONFIGS[key][2]
    net.load_state_dict(ref, strict=True)
    for k, v in net.state_dict().items():
        assert torch.equal(v, ref[k]), k


def test_drop_in_name_resolves_to_the_native_class():
    """`from fusion_model.Reconet import ReCoNet` with paif_amd/dropin first on the path (the reference's test_original.py:19)."""
    code = ("import fusion_model.Reconet as M, paif_amd.fusion_model.reconet as N;"
            "assert M.ReCoNet is N.ReCoNet; n = M.ReCoNet(3, 64, False); assert n.depth == 3; print('ok')")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "paif_amd", "dropin"), ROOT]))
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0 and b"ok" in r.stdout, r.stdout.decode(errors="replace")


def test_composite_accepts_the_baseline_and_orders_its_parameters():
    from paif_amd.core.model_fusion_auto import Network_MM_CompModel, grad_milestones
    from paif_amd.fusion_model.reconet import ReCoNet

    m = Network_MM_CompModel(ReCoNet(3, 16, False), None, None, "mit_b0", num_classes=9)
    assert isinstance(m.enhance_net, ReCoNet)
    assert grad_milestones(m)[-1] is m.enhance_net        # they only walk parameters: the baseline is the last milestone
    assert all(hasattr(p, "_paif_order") for p in m.enhance_net.parameters())


def test_unsupported_requests_say_why():
    from paif_amd.fusion_model.reconet import ReCoNet

    with pytest.raises(NotImplementedError, match="dim=24"):
        ReCoNet(3, 24, False)
    net = ReCoNet(2, 16, False)
    with pytest.raises(NotImplementedError, match="wgrad"):
        net.backward_impl(torch.zeros(1, 1, 4, 4), {}, wgrad=True)
    with pytest.raises(RuntimeError, match="no CPU path"):              # as tests/test_abi.py::test_cpu_tensor_is_refused
        with torch.no_grad():
            net(torch.zeros(1, 1, 8, 8), torch.zeros(1, 1, 8, 8))
    with pytest.raises(NotImplementedError, match="[Pp]arameter gradients"):   # a forward that wants parameter gradients
        net(torch.zeros(1, 1, 8, 8), torch.zeros(1, 1, 8, 8))
    bn = ReCoNet(2, 16, True).train()
    with pytest.raises(NotImplementedError, match="train-mode BatchNorm"):
        with torch.no_grad():
            bn._pack()
