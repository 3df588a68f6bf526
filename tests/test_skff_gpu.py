"""GPU: SKFF (paif_amd/operations_m.py) and Fusion_Network2 (paif_amd/fusion_model/skff.py; csrc/skff.hip, csrc/drdb.hip,
csrc/conv_slab.h) against the reference's own outputs and autograd (tests/golden/gk_*.npz, generated on the CPU by
tools/make_golden_skff.py).

Bound of the parity checks (tests/baseline_common.py: bound): with floor = max|ref32 - ref64| of the same tensor,
max|hip - ref64| <= 1.5 * floor + 1e-5 * max(1, max|ref64|).

The gate couples every pixel of an image to every other, forward (the pool) and in reverse (dS / (H W) at every pixel, the softmax term).
The tool kept only gradient cases whose float64 gradient differs from the one computed with the attention held constant by at least 100
floors, so a reverse pass that drops either term fails the gradient checks.  In the fixtures i1 is the infrared plane (`ir`), i2 the
visible Y plane (`vis`); the guidance maps and the SKFF inputs are S.make_feature(seed, shape) of the stored seeds."""
import numpy as np
import pytest
import torch

from paif_amd import ops, synthetic as S
from tests import skff_eager as E
from tests.baseline_common import bound, check, dev, floor  # noqa: F401
from tests.helpers import t

pytestmark = pytest.mark.gpu

GRAD_CASES = ("1x3x5", "1x13x17", "2x9x20", "1x19x18")
LARGE = ("1x37x53", "2x24x32")
SMALL = ("1x3x5", "1x13x17")
SKFF_CASES = [(c, h) for c in ("1x1x1", "1x3x5", "2x9x20", "1x37x53") for h in (2, 3)]
MAP_CHANNELS = [64] + [32] * 5 + [64, 64, 64, 64] + [32] * 5 + [64, 64, 64, 64, 1]
_SD = {}


def _net(golden):
    from paif_amd.core.model_fusion_auto import Fusion_Network2

    if "fn2" not in _SD:
        g = golden("gk_index")
        _SD["fn2"] = {k: torch.from_numpy(np.asarray(v)) for k, v in S.fn2_state_dict(g["scales"], float(g["shift"]), float(g["last_scale"])).items()}
    net = Fusion_Network2().eval()
    net.load_state_dict(_SD["fn2"], strict=True)
    return net.requires_grad_(False).to(dev())


def _inputs(golden, case):
    """-> (i1, i2, out1, out2, cot) on the device."""
    g = golden("gk_fn2_" + case)
    B, _, H, W = g["i1"].shape
    s1, s2 = (int(s) for s in g["guide_seeds"])
    cot = g["cot"] if "cot" in g else S.make_feature(900 + len(case), g["i1"].shape)
    return tuple(t(a).to(dev()) for a in (g["i1"], g["i2"], S.make_feature(s1, (B, 64, H, W)), S.make_feature(s2, (B, 128, H, W)), cot))


def _both(net, ins, cot, guides=True):
    """One taped forward and reverse -> (fused, tape, the four gradients)."""
    tape = {}
    with torch.no_grad():
        out = net._run(*ins, tape)
        grads = net._reverse(cot, tape, want_guides=guides)
    return out, tape, grads


def _flat(tape):
    m = tape["maps"]
    return m["slab"] + m["r6"] + [m[k] for k in ("f1", "c3", "f2", "c4", "v2", "f", "minmax")] + [m[g][k] for g in ("g1", "g2") for k in ("a", "z")]


# ---- SKFF alone --------------------------------------------------------------------------------------------------------------------
def _skff_case(golden, case, height):
    from paif_amd.operations_m import SKFF

    g = golden("gk_skff_%s_h%d" % (case, height))
    m = SKFF(64, height, int(g["reduction"]), bool(g["bias"])).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in S.skff_state_dict(g["scales"], height, int(g["reduction"]), bool(g["bias"])).items()},
                      strict=True)
    shape = tuple(int(s) for s in g["shape"])
    xs = [t(S.make_feature(int(s), shape)).to(dev()) for s in g["seeds"]]
    cot = t(S.make_feature(int(g["cot_seed"]), shape)).to(dev())

    def ref(key):   # a float64 map of the largest case lies in a file of its own
        return g[key] if key in g else golden("gk_skff_%s_h%d_%s" % (case, height, key))[key]

    return g, m.requires_grad_(False).to(dev()), xs, cot, ref


@pytest.mark.parametrize("case,height", SKFF_CASES)
def test_skff_alone_forward_and_reverse(golden, case, height):
    """1x1x1: the pool of one pixel is the pixel; 1x3x5; 2x9x20: a gate per image; 1x37x53: four pool workgroups of 512 pixels, the last
    one ragged (425).  Heights 2 and 3, reductions 4, 8 and 16, one case with biases.  Every input's gradient through .backward()."""
    g, m, xs, cot, ref = _skff_case(golden, case, height)
    with torch.no_grad():
        out = m(xs)
    assert out.grad_fn is None and out.shape == xs[0].shape
    check("skff", "%s h%d" % (case, height), "V", out, ref("out64"), float(g["floor_out"]))
    leaves = [x.clone().requires_grad_(True) for x in xs]
    out = m(leaves)
    assert out.grad_fn is not None
    (out * cot).sum().backward()
    for h, x in enumerate(leaves):
        check("skff", "%s h%d" % (case, height), "d_x%d" % h, x.grad, ref("d_x%d64" % h), float(g["floor_d_x%d" % h]))


def test_skff_gives_only_the_gradients_asked_for(golden):
    g, m, xs, cot, ref = _skff_case(golden, "1x3x5", 3)
    leaves = [xs[0], xs[1].clone().requires_grad_(True), xs[2]]
    (m(leaves) * cot).sum().backward()
    assert leaves[0].grad is None and leaves[2].grad is None
    check("skff", "1x3x5 h3", "d_x1 alone", leaves[1].grad, ref("d_x164"), float(g["floor_d_x1"]))


def test_skff_refusals_on_the_device(golden):
    _, m, xs, _, _ = _skff_case(golden, "1x3x5", 2)
    with torch.no_grad():
        with pytest.raises(ValueError, match="list of 2"):
            m(xs + xs[:1])
        with pytest.raises(ValueError, match="one shape"):
            m([xs[0], xs[1][:, :, :2]])
        with pytest.raises(TypeError, match="fp32"):
            m([xs[0].half(), xs[1].half()])
    with pytest.raises(NotImplementedError, match="[Pp]arameter gradients"):
        m.requires_grad_(True)(xs)


# ---- Fusion_Network2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GRAD_CASES + LARGE)
def test_fused_plane_matches_the_reference(golden, case):
    g = golden("gk_fn2_" + case)
    net = _net(golden)
    ins = _inputs(golden, case)[:4]
    with torch.no_grad():
        out = net(*ins)
    assert out.grad_fn is None and out.shape == ins[0].shape
    assert float(out.min()) == 0.0 and float(out.max()) == 1.0
    check("fused", case, "fused", out, g["fused64"], floor(g["fused"], g["fused64"]))


@pytest.mark.parametrize("case", SMALL)
def test_feature_maps_match_the_reference(golden, case):
    """The 20 taped maps (897 channels) and both gates' attention, each against its own floor."""
    parts = [golden("gk_fn2_%s_maps%d" % (case, p)) for p in range(int(golden("gk_index")["maps_parts_" + case][0]))]
    net = _net(golden)
    maps, att = net._features(*_inputs(golden, case)[:4])
    assert [m.shape[1] for m in maps] == MAP_CHANNELS and sum(MAP_CHANNELS) == 897
    for k, m in enumerate(maps):
        g = next(p for p in parts if "map%d" % k in p)
        check("maps", case, "map%d" % k, m, g["map%d" % k], float(g["map_floor"][k]))
    for k, a in enumerate(att):
        check("maps", case, "attention%d" % k, a, parts[0]["att%d" % k], float(parts[0]["att_floor"][k]))


@pytest.mark.parametrize("case", GRAD_CASES)
def test_input_gradients_match_float64_autograd(golden, case):
    """d_ir, d_vis, d_out1, d_out2 for the fixture's cotangent on the fused plane, through forward + .backward()."""
    g = golden("gk_fn2_" + case)
    net = _net(golden)
    *ins, cot = _inputs(golden, case)
    leaves = [x.clone().requires_grad_(True) for x in ins]
    out = net(*leaves)
    assert out.grad_fn is not None
    (out * cot).sum().backward()
    check("grad", case, "d_i1", leaves[0].grad, g["d_i164"], floor(g["d_i1"], g["d_i164"]))
    check("grad", case, "d_i2", leaves[1].grad, g["d_i264"], floor(g["d_i2"], g["d_i264"]))
    check("grad", case, "d_out1", leaves[2].grad, g["d_out164"], float(g["floor_d_out1"]))
    check("grad", case, "d_out2", leaves[3].grad, g["d_out264"], float(g["floor_d_out2"]))


def test_a_batch_is_normalised_as_one_tensor(golden):
    """2x9x20: min and max fall in different images (the tool searched for that), so the batch's plane is the reference's for the batch
    and NOT the two images run singly; the gradient of one image's output reaches the other image's input through the extrema."""
    g, idx = golden("gk_fn2_2x9x20"), golden("gk_index")["case_2x9x20"]
    assert idx[5] != idx[6]
    net = _net(golden)
    *ins, cot = _inputs(golden, "2x9x20")
    with torch.no_grad():
        both = net(*ins)
        single = torch.cat([net(*[x[k:k + 1] for x in ins]) for k in range(2)], 0)
    check("batch", "2x9x20", "fused", both, g["fused64"], floor(g["fused"], g["fused64"]))
    diff = float((both - single).abs().max())
    print("batch of two against the images run singly: %.3e" % diff)
    assert diff > 1e-2
    a = ins[0].clone().requires_grad_(True)
    out = net(a, *ins[1:])
    (out[0:1] * cot[0:1]).sum().backward()
    cross = float(a.grad[1].abs().max())
    print("gradient of image 0's output with respect to image 1's input: %.3e" % cross)
    assert cross > 0


def test_reverse_pass_is_linear_in_the_cotangent(golden):
    """reverse(g1) + reverse(g2) = reverse(g1 + g2) within 1e-4 of the largest gradient (tests/baseline_common.py says why)."""
    net = _net(golden)
    *ins, cot = _inputs(golden, "1x19x18")
    tape = {}
    with torch.no_grad():
        net._run(*ins, tape)
        g2 = t(S.make_feature(77, tuple(cot.shape))).to(dev())
        r1, r2, r12 = net._reverse(cot, tape), net._reverse(g2, tape), net._reverse(ops.add(cot, g2), tape)
    for x, y, z in zip(r1, r2, r12):
        scale = max(1.0, float(z.abs().max()))
        err = float((x + y - z).abs().max())
        print("linearity: err %.3e scale %.3e" % (err, scale))
        assert float(z.abs().max()) > 0
        assert err <= 1e-4 * scale


def test_two_runs_are_bit_identical(golden):
    net = _net(golden)
    *ins, cot = _inputs(golden, "2x24x32")
    runs = []
    for _ in range(2):
        out, tape, grads = _both(net, ins, cot)
        runs.append([out] + _flat(tape) + list(grads))
    for x, y in zip(*runs):
        assert torch.equal(x, y)


def test_channel_slices_are_taken_without_a_copy(golden):
    """ir[:, 0:1] of a multi-channel tensor and a multi-channel vis: planes addressed through their batch stride; forward itself takes
    channel 0 of both, as the reference does, and the other channels get a zero gradient."""
    net = _net(golden)
    i1, i2, o1, o2, cot = _inputs(golden, "2x24x32")
    wide1 = torch.cat([i1, i1 * 0.5, i1 * 0.25], 1).contiguous()
    wide2 = torch.cat([i2, i2 * 0.5], 1).contiguous()
    base, _, gbase = _both(net, (i1, i2, o1, o2), cot)
    view = wide1[:, 0:1]
    assert ops._plane(view)[0].data_ptr() == wide1.data_ptr()          # no copy is made of the slice
    got, _, gview = _both(net, (view, wide2[:, 0:1], o1, o2), cot)
    assert torch.equal(base, got)
    for x, y in zip(gbase, gview):
        assert torch.equal(x, y)
    with torch.no_grad():
        assert torch.equal(base, net(wide1, wide2, o1, o2))
    a = wide2.clone().requires_grad_(True)
    (net(wide1, a, o1, o2) * cot).sum().backward()
    assert torch.equal(a.grad[:, 0:1], gbase[1]) and float(a.grad[:, 1:].abs().max()) == 0.0


def test_forward_and_reverse_replayed_from_a_graph_are_bit_identical(golden):
    """Forward + reverse captured once with torch.cuda.graph and replayed = the eager run.  Single stream, no parallel branches; the eager
    pass comes first, so every weight pack is built (and every PReLU slope read) before the capture."""
    net = _net(golden)
    *ins, cot = _inputs(golden, "1x13x17")
    static = [x.clone() for x in ins] + [cot.clone()]
    eager_out, _, eager_grads = _both(net, ins, cot)
    eager = [eager_out] + list(eager_grads)
    gstream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(gstream):
        _both(net, static[:4], static[4])
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=gstream):
            out, _, grads = _both(net, static[:4], static[4])
    torch.cuda.synchronize()
    for x in [out] + list(grads):
        x.zero_()
    for s in static:
        s.zero_()
    for s, x in zip(static, ins + [cot]):
        s.copy_(x)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert float(eager[1].abs().max()) > 0
    for x, y in zip(eager, [out] + list(grads)):
        assert torch.equal(x, y)


def test_train_mode_equals_eval_mode_bit_for_bit(golden):
    """There is no norm layer and no dropout: the mode changes no bit."""
    net = _net(golden)
    *ins, cot = _inputs(golden, "1x13x17")
    out, _, grads = _both(net, ins, cot)
    net.train()
    out2, _, grads2 = _both(net, ins, cot)
    with torch.no_grad():
        out3 = net(*ins)
    for x, y in zip([out, out] + list(grads), [out2, out3] + list(grads2)):
        assert torch.equal(x, y)


def test_reference_initialisation_matches_torch_eager(golden):
    """A net as the constructor leaves it (torch's default initialisation, slopes 0.25) against tests/skff_eager.py on the device.  The
    bound is that restatement's own float32-vs-float64 difference on the same inputs, times 1.5, plus the scale term (check)."""
    from paif_amd.core.model_fusion_auto import Fusion_Network2

    torch.manual_seed(20)
    net = Fusion_Network2().eval().requires_grad_(False).to(dev())
    assert float(net.relu.weight) == 0.25
    ins = _inputs(golden, "1x13x17")[:4]
    with torch.no_grad():
        mine = net(*ins)
        ref32 = E.fusion_network2(net, *ins)
        ref64 = E.fusion_network2(net, *ins, dtype=torch.float64)
    check("reference initialisation", "1x13x17", "fused", mine, ref64.cpu().numpy(), floor(ref32.cpu().numpy(), ref64.cpu().numpy()))


def test_guidance_gradients_are_built_only_when_asked_for(golden, monkeypatch):
    """out1 / out2 without requires_grad: no d_out1 / d_out2, and the two transposed 1x1 launches are not made; d_ir and d_vis keep
    their bits."""
    net = _net(golden)
    *ins, cot = _inputs(golden, "1x3x5")
    L = ops.lib()
    calls = []
    real = L.paif_fn2_guide_bwd
    monkeypatch.setattr(L, "paif_fn2_guide_bwd", lambda *a: calls.append(a[1]) or real(*a))
    full = [x.clone().requires_grad_(True) for x in ins]
    (net(*full) * cot).sum().backward()
    assert calls == [0, 1] and full[2].grad is not None and full[3].grad is not None
    del calls[:]
    part = [ins[0].clone().requires_grad_(True), ins[1].clone().requires_grad_(True), ins[2], ins[3]]
    (net(*part) * cot).sum().backward()
    assert calls == [] and ins[2].grad is None and ins[3].grad is None
    assert torch.equal(part[0].grad, full[0].grad) and torch.equal(part[1].grad, full[1].grad)
    # one guidance map alone: both launches, one gradient handed out
    one = [ins[0], ins[1], ins[2], ins[3].clone().requires_grad_(True)]
    (net(*one) * cot).sum().backward()
    assert calls == [0, 1] and torch.equal(one[3].grad, full[3].grad)


def test_wrong_inputs_are_refused_on_the_device(golden):
    net = _net(golden)
    i1, i2, o1, o2, _ = _inputs(golden, "1x3x5")
    with pytest.raises(RuntimeError, match="no CPU path"):
        net(i1, i2, o1.cpu().half(), o2)                                  # the device before the dtype
    with pytest.raises(TypeError, match="fp32"):
        net(i1, i2, o1.half()[:, :, :2], o2)                              # the dtype before the shape
    with pytest.raises(ValueError, match=r"out1 \[B,64,H,W\]"):
        net(i1, i2, o1[:, :32], o2)
    with pytest.raises(ValueError, match=r"\[B,1,H,W\]"):
        net(i1, i2[:, :, :2], o1, o2)
    trainable = _net(golden).requires_grad_(True)
    with pytest.raises(NotImplementedError, match="[Pp]arameter gradients"):
        trainable(i1, i2, o1, o2)
    with ops.no_param_grads():                                            # an attack's forward: input gradients only
        a = i1.clone().requires_grad_(True)
        trainable(a, i2, o1, o2).sum().backward()
    assert a.grad is not None and all(p.grad is None for p in trainable.parameters())
    bad = _net(golden)
    with torch.no_grad():
        bad.relu.weight.fill_(-0.1)
    with pytest.raises(ValueError, match="slope"):
        bad(i1, i2, o1, o2)
    # the gates' own slope may be negative: their branch is read off the taped z
    neg = _net(golden)
    with torch.no_grad():
        neg.skff.conv_du[1].weight.fill_(-0.3)
        ref = E.fusion_network2(neg, i1, i2, o1, o2, dtype=torch.float64)
        ref32 = E.fusion_network2(neg, i1, i2, o1, o2)
        check("negative gate slope", "1x3x5", "fused", neg(i1, i2, o1, o2), ref.cpu().numpy(), floor(ref32.cpu().numpy(), ref.cpu().numpy()))
