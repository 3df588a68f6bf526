"""CPU: what paif_amd/fusion_model/_native.py owns for the seven native fusion networks -- the refusals that need no device, the base in
every class's MRO, and that the base adds nothing to a state_dict."""
import pytest
import torch

from paif_amd.fusion_model._native import NativeFusion


def _reconet():
    from paif_amd.fusion_model.reconet import ReCoNet
    return ReCoNet(1, 16, False)


def _sdnet():
    from paif_amd.fusion_model.sdnet import SDNet
    return SDNet()


def _u2fusion():
    from paif_amd.fusion_model.u2fusion import U2Fusion
    return U2Fusion()


def _seafusion():
    from paif_amd.fusion_model.seafusion import SeaFusion
    return SeaFusion()


def _didfuse():
    from paif_amd.fusion_model.didfuse import DID
    return DID()


def _bffusion():
    from paif_amd.fusion_model.bffusion import BFFR
    return BFFR()


def _drdb():
    from paif_amd.fusion_model.drdb import Fusion_Network
    return Fusion_Network()


# the name each network carries in its messages -> its constructor
NETWORKS = {"ReCoNet": _reconet, "SDNet": _sdnet, "U2Fusion": _u2fusion, "SeaFusion": _seafusion, "DIDFuse": _didfuse, "BFFusion": _bffusion,
            "Fusion_Network": _drdb}

# list(SDNet().state_dict()) of the commit before the base class existed
SDNET_KEYS = ['conv11.0.weight', 'conv11.0.bias', 'conv12.0.weight', 'conv12.0.bias', 'conv21.0.weight', 'conv21.0.bias', 'conv22.0.weight',
              'conv22.0.bias', 'conv31.0.weight', 'conv31.0.bias', 'conv32.0.weight', 'conv32.0.bias', 'conv41.0.weight', 'conv41.0.bias',
              'conv42.0.weight', 'conv42.0.bias', 'fuse.0.weight', 'fuse.0.bias', 'decom.0.weight', 'decom.0.bias', 'conv51.0.weight',
              'conv51.0.bias', 'conv52.0.weight', 'conv52.0.bias', 'conv61.0.weight', 'conv61.0.bias', 'conv62.0.weight', 'conv62.0.bias',
              'conv71.0.weight', 'conv71.0.bias', 'conv72.0.weight', 'conv72.0.bias']


@pytest.mark.parametrize("name", sorted(NETWORKS))
def test_the_protocol_refuses_what_is_not_built_without_a_device(name):
    net = NETWORKS[name]().eval().requires_grad_(False)
    assert NativeFusion in type(net).__mro__
    z = torch.zeros(1, 1, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        net(z, z)
    with pytest.raises(RuntimeError, match="no CPU path"):
        net.forward_impl(z, z)
    with pytest.raises(NotImplementedError, match="^%s: `inter`" % name):
        net.forward_impl(z, z, inter=object())
    with pytest.raises(NotImplementedError, match="^%s: parameter gradients" % name):
        net.backward_impl(None, {}, wgrad=True)
    with pytest.raises(NotImplementedError, match="^%s: parameter gradients .* -- freeze the parameters" % name):
        net.requires_grad_(True)(z, z)


def test_the_base_adds_no_state_dict_key():
    assert len(SDNET_KEYS) == 32
    assert list(NETWORKS["SDNet"]().state_dict()) == SDNET_KEYS
    for name in sorted(NETWORKS):
        net = NETWORKS[name]()
        own = {k.split(".")[0] for k in net.state_dict()}
        assert own <= {n for n, _ in net.named_children()} and "_packs" not in own, name
