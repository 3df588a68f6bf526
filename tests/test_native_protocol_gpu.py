"""GPU: the refusals paif_amd/fusion_model/_native.py raises for the seven native fusion networks on device tensors, message text
character for character as each network's module stated it before the base class existed; and the shared autograd node under
ops.no_param_grads().  The refusals launch no kernel."""
import pytest
import torch

from paif_amd import ops
from tests.baseline_common import dev
from tests.test_native_protocol_cpu import NETWORKS

pytestmark = pytest.mark.gpu

SHAPE_NOTE = {"SeaFusion": " (image_vis[:, :1] and a one-channel image_ir)", "Fusion_Network": " (channel 0 of ir and of vis)"}
TAKES_CHANNEL_0_ITSELF = ("SeaFusion", "Fusion_Network")


def _net(name):
    return NETWORKS[name]().eval().requires_grad_(False).to(dev())


@pytest.mark.parametrize("name", sorted(NETWORKS))
def test_wrong_planes_are_refused_with_the_network_s_own_message(name):
    net = _net(name)
    z = torch.zeros(1, 1, 8, 8, device=dev())
    with pytest.raises(TypeError) as e:
        net(z.half(), z.half())
    assert str(e.value) == "%s: fp32 planes are expected, got torch.float16" % name
    with pytest.raises(ValueError) as e:
        net(z, torch.zeros(1, 1, 8, 9, device=dev()))
    assert str(e.value) == ("%s: two [B,1,H,W] planes of one shape are expected%s, got (1, 1, 8, 8) and (1, 1, 8, 9)"
                            % (name, SHAPE_NOTE.get(name, "")))
    if name not in TAKES_CHANNEL_0_ITSELF:
        z3 = torch.zeros(1, 3, 8, 8, device=dev())
        with pytest.raises(ValueError) as e:
            net(z3, z3)
        assert str(e.value) == "%s: two [B,1,H,W] planes of one shape are expected, got (1, 3, 8, 8) and (1, 3, 8, 8)" % name


def test_the_remaining_messages_are_the_networks_own():
    z = torch.zeros(1, 1, 16, 16, device=dev())
    freeze = " -- freeze the parameters (requires_grad_(False)), or run under ops.no_param_grads() / torch.no_grad() for input gradients"
    for name, training in (("SDNet", "training the baseline"), ("ReCoNet", "training the baseline"), ("Fusion_Network", "training the network")):
        net = _net(name)
        with pytest.raises(NotImplementedError) as e:
            net.forward_impl(z, z, inter=object())
        assert str(e.value) == "%s: `inter` (the searched network's decomposition intermediates) does not apply" % name
        with pytest.raises(NotImplementedError) as e:
            net.requires_grad_(True)(z, z)
        assert str(e.value) == "%s: parameter gradients (%s) are not built" % (name, training) + freeze
    with pytest.raises(NotImplementedError) as e:
        _net("SDNet").backward_impl(None, {}, wgrad=True)
    assert str(e.value) == "SDNet: parameter gradients (training the baseline) are not built (wgrad=True)"
    with pytest.raises(NotImplementedError) as e:
        _net("ReCoNet").backward_impl(None, {}, wgrad=True)
    assert str(e.value) == "ReCoNet: parameter gradients (wgrad=True, training the baseline) are not built"
    with pytest.raises(ValueError) as e:
        _net("DIDFuse")(z[..., :1, :], z[..., :1, :])
    assert str(e.value) == "DIDFuse: reflection padding by 1 needs H, W >= 2 (as torch's ReflectionPad2d), got [B,1,H,W] = (1, 1, 1, 16)"
    with pytest.raises(ValueError) as e:
        _net("BFFusion")(z[..., :15], z[..., :15])
    assert str(e.value) == ("BFFusion: H, W >= 16 are needed (the level-4 map is (H // 8) x (W // 8) and takes reflection padding by 1), "
                            "got [B,1,H,W] = (1, 1, 16, 15)")


@pytest.mark.parametrize("name,extra", (("SDNet", {}), ("ReCoNet", {"init_f": "mean"})))
def test_an_attack_s_forward_gives_input_gradients_and_no_parameter_gradient(name, extra):
    """Under ops.no_param_grads() with trainable parameters the shared autograd node records the call: the input gradient arrives, no
    p.grad is set.  ReCoNet hands the node its `init_f` as well."""
    net = _net(name).requires_grad_(True)
    z = torch.zeros(1, 1, 8, 8, device=dev())
    with ops.no_param_grads():
        a = z.clone().requires_grad_(True)
        out = net(a, z, **extra)
        assert out.grad_fn is not None and out.shape == z.shape
        out.sum().backward()
    assert a.grad is not None and a.grad.shape == z.shape
    assert all(p.grad is None for p in net.parameters())
