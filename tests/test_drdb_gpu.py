"""GPU: the hand-designed fusion network (paif_amd/fusion_model/drdb.py, csrc/drdb.hip, csrc/conv_slab.h) against the reference's own
outputs and autograd (tests/golden/gr_drdb*.npz, generated on the CPU by tools/make_golden_drdb.py), and inside the composite model /
attack / harness flow of the searched network.

Bound of the kernel parity checks (tests/baseline_common.py: bound): with floor = max|ref32 - ref64| of the same tensor,
max|hip - ref64| <= 1.5 * floor + 1e-5 * max(1, max|ref64|).  One kernel form exists (exact fp32, the dilated 3x3, the 3x3 and the 1x1
convs on v_mfma_f32_16x16x4_f32); it is the default build.

Weight set A has both clamps active (min = 0 and max = 1 are attained by clamped pixels: the normalisation passes no gradient through
its extrema); set B has no clamped pixel and single extremal pixels: B is the test of the extremum terms.  In the fixtures i1 is the
infrared plane (`ir`), i2 the visible Y plane (`vis`).

The reference's autograd is the yardstick of the input gradients only where no sign point (the fifteen pre-activations, f against 0 and
1) is within fp32 reach of its jump (the five small cases, see the tool).  At 1x37x53 and 2x24x32 the reverse pass is tested as what it
is given its tape -- a linear map -- against a float64 restatement that takes EVERY branch from the tape: ReLU and PReLU masks off the
taped outputs, the clamp off the taped f, the extrema's positions and clamped flags off the taped f.  Nothing is recomputed, so no pixel
is excluded."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from paif_amd import ops, synthetic as S
from tests import drdb_eager as E
from tests import baseline_common as C
from tests.baseline_common import check, dev, exact_arithmetic, floor  # noqa: F401  (exact_arithmetic is a fixture)
from tests.helpers import t

pytestmark = pytest.mark.gpu

GRAD_CASES = ("1x3x5", "1x13x17", "2x9x20", "1x5x37", "1x19x18")
LARGE = ("1x37x53", "2x24x32")
SMALL = ("1x3x5", "1x13x17")
ALL = [(c, "A") for c in GRAD_CASES + LARGE] + [(c, "B") for c in GRAD_CASES]
GRADS = [(c, w) for w in ("A", "B") for c in GRAD_CASES]
MAP_CHANNELS = [64] + [32, 32, 32, 32, 32, 64, 64] * 2 + [32, 1]
HALO = 23            # conv1 1, ten dilated convs 2 each, conv2 1, conv21 1
EPS, ALPHA = 8 / 255., 2 / 255.
_SD = {}


def _sd(golden, which="A"):
    """The fixture weights, rebuilt once per set from the fifteen scales, the shift and the last scale."""
    if which not in _SD:
        g = golden("gr_drdb")
        shift, last = (0.0, 1.0) if which == "A" else (float(g["shift_B"]), float(g["last_scale_B"]))
        _SD[which] = {k: torch.from_numpy(np.asarray(v)) for k, v in S.drdb_state_dict(g["scales"], shift, last).items()}
    return _SD[which]


def _net(golden, which="A"):
    from paif_amd.fusion_model.drdb import Fusion_Network

    net = Fusion_Network().eval()
    net.load_state_dict(_sd(golden, which), strict=True)
    return net.requires_grad_(False).to(dev())


def _inputs(golden, case, which="A"):
    g = golden("gr_drdb_%s_%s" % (case, which))
    cot = g["cot"] if "cot" in g else S.make_feature(900 + len(case), g["i1"].shape)
    return t(g["i1"]).to(dev()), t(g["i2"]).to(dev()), t(cot).to(dev())


@pytest.mark.parametrize("case,which", ALL)
def test_fused_plane_matches_the_reference(golden, case, which):
    """1x3x5: most +-2-row taps fall outside the plane, smaller than the total halo of 23; 1x13x17 ragged in both directions with two tiles
    across; 2x9x20 two images under one batch min / max; 1x5x37 three tiles across; 1x19x18 2 x 2 ragged tiles; 1x37x53 and 2x24x32
    several tile rows and columns."""
    g = golden("gr_drdb_%s_%s" % (case, which))
    net = _net(golden, which)
    i1, i2, _ = _inputs(golden, case, which)
    with torch.no_grad():
        out = net(i1, i2)
    assert out.grad_fn is None and out.shape == i1.shape
    assert float(out.min()) == 0.0 and float(out.max()) == 1.0
    check("fused", case + which, "fused", out, g["fused64"], floor(g["fused"], g["fused64"]), halo=HALO if case in LARGE else None)


@pytest.mark.parametrize("case", SMALL)
def test_feature_maps_match_the_reference(golden, case):
    """The 17 taped maps (673 channels), each against its own floor: conv1, per DRDB x_1 .. x_5, relu(x6) and the output, conv2, f."""
    parts = [golden("gr_drdb_%s_maps%d" % (case, p)) for p in (0, 1)]
    net = _net(golden)
    i1, i2, _ = _inputs(golden, case)
    maps = net._features(i1, i2)
    assert [m.shape[1] for m in maps] == MAP_CHANNELS and sum(MAP_CHANNELS) == 673
    for k, m in enumerate(maps):
        g = parts[0 if k < 9 else 1]
        check("maps", case, "map%d" % k, m, g["map%d" % k], float(g["map_floor"][k]))


def _block(golden):
    from paif_amd.fusion_model.drdb import DRDB

    blk = DRDB().eval()
    blk.load_state_dict({k[len("DRDB1."):]: v for k, v in _sd(golden).items() if k.startswith("DRDB1.")}, strict=True)
    return blk.requires_grad_(False).to(dev())


@pytest.mark.parametrize("case", SMALL)
def test_a_block_alone_forward_and_reverse(golden, case):
    """DRDB as a module of its own, [B,64,H,W] -> [B,64,H,W], on the map conv1 + PReLU gave; its input gradient through .backward()."""
    g = golden("gr_drdb_%s_block" % case)
    blk = _block(golden)
    x = t(g["x"]).to(dev())
    with torch.no_grad():
        out = blk(x)
    assert out.grad_fn is None
    check("block", case, "out", out, g["out64"], floor(g["out"], g["out64"]))
    a = x.clone().requires_grad_(True)
    out = blk(a)
    assert out.grad_fn is not None
    (out * t(g["cot"]).to(dev())).sum().backward()
    check("block", case, "d_x", a.grad, g["d_x64"], floor(g["d_x"], g["d_x64"]))


@pytest.mark.parametrize("case,which", GRADS)
def test_input_gradients_match_float64_autograd(golden, case, which):
    """d_i1, d_i2 for the fixture's cotangent on the fused plane, through forward + .backward().  Set B carries the extremum terms."""
    g = golden("gr_drdb_%s_%s" % (case, which))
    net = _net(golden, which)
    i1, i2, cot = _inputs(golden, case, which)
    a, b = i1.clone().requires_grad_(True), i2.clone().requires_grad_(True)
    out = net(a, b)
    assert out.grad_fn is not None
    (out * cot).sum().backward()
    for name, mine in (("d_i1", a.grad), ("d_i2", b.grad)):
        check("grad", case + which, name, mine, g[name + "64"], floor(g[name], g[name + "64"]))


def test_a_batch_is_normalised_as_one_tensor(golden):
    """2x9x20, set B: min and max fall in different images (the tool searched for that), so the batch's plane is the reference's for the
    batch (test_fused_plane_matches_the_reference) and NOT the two images run singly; the gradient of one image's output reaches the other
    image's input through the extrema."""
    g, idx = golden("gr_drdb_2x9x20_B"), golden("gr_drdb")["case_2x9x20_B"]
    assert idx[5] != idx[6]
    net = _net(golden, "B")
    i1, i2, cot = _inputs(golden, "2x9x20", "B")
    with torch.no_grad():
        both = net(i1, i2)
        single = torch.cat([net(i1[k:k + 1], i2[k:k + 1]) for k in range(2)], 0)
    check("batch", "2x9x20B", "fused", both, g["fused64"], floor(g["fused"], g["fused64"]))
    diff = float((both - single).abs().max())
    print("batch of two against the images run singly: %.3e" % diff)
    assert diff > 1e-2
    a = i1.clone().requires_grad_(True)
    out = net(a, i2)
    (out[0:1] * cot[0:1]).sum().backward()
    cross = float(a.grad[1].abs().max())
    print("gradient of image 0's output with respect to image 1's input: %.3e" % cross)
    assert cross > 0


def _nchw(m):
    return m.permute(0, 3, 1, 2).contiguous()


def _taped_branches(maps, slope):
    """Every branch of the forward, read off the tape (on the CPU): the PReLU masks of conv1, conv2, conv21, the ReLU masks of the ten
    dilated convs and the two 1x1, the clamp's pass mask, the clamped plane, and per extremum (position, clamped flag)."""
    def prelu(m):
        return torch.where(m > 0, 1.0, slope)

    def relu(m):
        return (m > 0).double()

    br = {}
    s = [x.cpu() for x in maps["slab"]]
    br["conv1"] = prelu(_nchw(s[0][..., 0:64]))
    for d in range(2):
        for k in range(5):
            br["d%d.%d" % (d, k)] = relu(_nchw(s[d][..., 64 + 32 * k:96 + 32 * k]))
        br["d%d.r6" % d] = relu(_nchw(maps["r6"][d].cpu()))
    br["conv2"] = prelu(_nchw(maps["c2"].cpu()))
    f = maps["f"].cpu()
    br["conv21"] = prelu(f)
    br["pass"] = ((f >= 0) & (f <= 1)).double()
    c = f.clamp(0, 1).double()
    br["c"] = c
    for name, pos in (("min", int(torch.argmin(c))), ("max", int(torch.argmax(c)))):
        br[name] = (pos, float(br["pass"].reshape(-1)[pos]) == 0.0)
    return br


def _linearised(sd, br, i1, i2, cot, dtype):
    """The network with every activation replaced by the constant mask of its taped map, biases dropped, the clamp by its pass mask, and
    the normalisation by its differential at the taped (c, min, max): with r = max - min,
    d fused = (d c - d min) / r - (c - min) / r^2 (d max - d min), d c = pass * d f, and an extremum's differential is that of its pixel,
    or nothing where that pixel is clamped.  -> (d_i1, d_i2) for the cotangent, by torch's CPU autograd in `dtype`."""
    def w(name):
        return sd[name + ".weight"].to(dtype)

    def m(name):
        return br[name].to(dtype)

    a, b = i1.to(dtype).clone().requires_grad_(True), i2.to(dtype).clone().requires_grad_(True)
    x = F.conv2d(torch.cat((a, b), 1), w("conv1"), padding=1) * m("conv1")
    for d, name in enumerate(("DRDB1", "DRDB2")):
        cat = x
        for k in range(5):
            xk = F.conv2d(cat, w("%s.Dcov%d" % (name, k + 1)), padding=2, dilation=2) * m("d%d.%d" % (d, k))
            cat = torch.cat((cat, xk), 1)
        x = x + F.conv2d(cat, w(name + ".conv")) * m("d%d.r6" % d)
    x = F.conv2d(x, w("conv2"), padding=1) * m("conv2")
    dc = F.conv2d(x, w("conv21"), padding=1) * m("conv21") * m("pass")
    c = br["c"].to(dtype)
    mn, mx = c.min(), c.max()
    r = mx - mn
    (pmn, cmn), (pmx, cmx) = br["min"], br["max"]
    dmn = 0 if cmn else dc.reshape(-1)[pmn]
    dmx = 0 if cmx else dc.reshape(-1)[pmx]
    y = (dc - dmn) / r - (c - mn) / (r * r) * (dmx - dmn)
    (y * cot.to(dtype)).sum().backward()
    return a.grad.numpy(), b.grad.numpy()


@pytest.mark.parametrize("case", LARGE)
def test_reverse_pass_matches_its_float64_restatement_on_the_taped_branches(golden, case):
    """Sizes the margin condition cannot reach.  A sign the GPU forward decided differently from the reference cannot enter: the branches
    are the tape's, all of them.  A wrong tap, dilation, slice offset or mask shows at order 0.1.  The floor is the same restatement in
    float32."""
    net = _net(golden)
    i1, i2, cot = _inputs(golden, case)
    tape = {}
    with torch.no_grad():
        net.forward_impl(i1, i2, tape=tape)
        d1, d2 = net.backward_impl(cot, tape)
    sd = _sd(golden)
    br = _taped_branches(tape["maps"], float(sd["relu.weight"]))
    mm = tape["maps"]["minmax"].cpu()
    assert float(mm[0]) == float(br["c"].min()) and float(mm[1]) == float(br["c"].max())
    print("taped-mask reverse %s: extrema at %s (clamped %s) and %s (clamped %s), pass share %.3f"
          % (case, br["min"][0], br["min"][1], br["max"][0], br["max"][1], float(br["pass"].mean())))
    r64 = _linearised(sd, br, i1.cpu(), i2.cpu(), cot.cpu(), torch.float64)
    r32 = _linearised(sd, br, i1.cpu(), i2.cpu(), cot.cpu(), torch.float32)
    for name, mine, a64, a32 in (("d_i1", d1, r64[0], r32[0]), ("d_i2", d2, r64[1], r32[1])):
        assert float(np.abs(a64).max()) > 0
        check("taped-mask reverse", case, name, mine, a64, floor(a32, a64), halo=HALO)


def _flat(tape):
    m = tape["maps"]
    return [tape["out"]] + m["slab"] + m["r6"] + [m["f2"], m["c2"], m["f"], m["minmax"]]


@pytest.mark.parametrize("which", ("A", "B"))
def test_reverse_pass_is_linear_in_the_cotangent(golden, which):
    """backward_impl(g1) + backward_impl(g2) = backward_impl(g1 + g2) to fp32 rounding: within 1e-4 of the largest gradient
    (tests/baseline_common.py says why)."""
    C.reverse_pass_is_linear_in_the_cotangent(_net(golden, which), *_inputs(golden, "1x19x18", which), rtol=1e-4, label=" " + which)


def test_two_runs_are_bit_identical(golden):
    C.two_runs_are_bit_identical(_net(golden), *_inputs(golden, "2x24x32"), taped=_flat)


def test_channel_slices_are_taken_without_a_copy(golden):
    """The composite hands over ir[:, 0:1] and ycc of multi-channel tensors: planes addressed through their batch stride.  forward itself
    takes channel 0 of both inputs, as the reference does."""
    net = _net(golden)
    fa, wide1, wide2 = C.channel_slices_are_taken_without_a_copy(net, *_inputs(golden, "2x24x32"))
    with torch.no_grad():
        assert torch.equal(fa, net(wide1, wide2))


def test_settings_that_do_not_apply_change_nothing(golden):
    """One arithmetic: the storage mode, the conv / GEMM precision and two_stream leave every bit where it is."""
    C.settings_that_do_not_apply_change_nothing(_net(golden), *_inputs(golden, "1x13x17"), fp32_maps=_flat)


def test_wrong_planes_are_refused_on_the_device(golden):
    net = _net(golden)
    z = torch.zeros(1, 1, 8, 8, device=dev())
    with pytest.raises(TypeError, match="fp32"):
        net(z.half(), z.half())
    with pytest.raises(ValueError, match=r"\[B,1,H,W\]"):
        net(z, torch.zeros(1, 1, 8, 9, device=dev()))
    with pytest.raises(ValueError, match=r"\[B,1,H,W\]"):
        net(z[0], z[0])
    trainable = _net(golden).requires_grad_(True)
    with pytest.raises(NotImplementedError, match="[Pp]arameter gradients"):
        trainable(z, z)
    i1, i2, _ = _inputs(golden, "1x3x5")
    with ops.no_param_grads():                                  # an attack's forward: input gradients only
        a = i1.clone().requires_grad_(True)
        out = trainable(a, i2)
        out.sum().backward()
    assert a.grad is not None and all(p.grad is None for p in trainable.parameters())
    # a negative slope: refused when the weights are packed
    bad = _net(golden)
    with torch.no_grad():
        bad.relu.weight.fill_(-0.1)
    with pytest.raises(ValueError, match="slope"):
        bad(i1, i2)


def test_train_mode_equals_eval_mode_bit_for_bit(golden):
    """There is no norm layer and no dropout: the mode changes no bit."""
    net = _net(golden)
    i1, i2, cot = _inputs(golden, "1x13x17")
    with torch.no_grad():
        tape = {}
        base = (net.forward_impl(i1, i2, tape=tape),) + tuple(net.backward_impl(cot, tape))
        net.train()
        tape = {}
        got = (net.forward_impl(i1, i2, tape=tape),) + tuple(net.backward_impl(cot, tape)) + (net(i1, i2),)
    for x, y in zip(base + (base[0],), got):
        assert torch.equal(x, y)


def test_reference_initialisation_matches_torch_eager(golden):
    """A net as the constructor leaves it (torch's default conv initialisation, slope 0.25) against tests/drdb_eager.py on the device.
    f, before the clamp, within 1e-5 max(1, max|f|) (tests/test_seafusion_gpu.py's bound for this check); the normalised plane is
    (c - min) / r with r = max - min, and an error delta on f moves it by at most 4 delta / r (delta / r each from c and min, and
    (c - min) / r <= 1 times 2 delta / r from r), so its bound is 4 times f's over r."""
    from paif_amd.fusion_model.drdb import Fusion_Network

    torch.manual_seed(20)
    net = Fusion_Network().eval().requires_grad_(False).to(dev())
    assert float(net.relu.weight) == 0.25
    i1, i2, _ = _inputs(golden, "1x13x17")
    with torch.no_grad():
        tape = {}
        mine = net.forward_impl(i1, i2, tape=tape)
        f_ref = E.pre_clamp(net, i1, i2)
        ref = E.normalise(f_ref)
    f_mine = tape["maps"]["f"]
    r = float(f_ref.clamp(0, 1).max() - f_ref.clamp(0, 1).min())
    bound_f = 1e-5 * max(1.0, float(f_ref.abs().max()))
    err_f, err = float((f_mine - f_ref).abs().max()), float((mine - ref).abs().max())
    print("reference initialisation: f err %.3e bound %.3e; fused err %.3e bound %.3e (range of the clamped f %.3e)"
          % (err_f, bound_f, err, 4 * bound_f / r, r))
    assert r > 1e-3
    assert err_f <= bound_f
    assert err <= 4 * bound_f / r


# ---- inside the composite model ------------------------------------------------------------------------------------------------
def _in_composite(golden):
    """The network with the fixture's weights as the fusion module of Network_MM_CompModel."""
    from paif_amd.core.model_fusion_auto import Fusion_Network

    return C.composite(Fusion_Network(), _sd(golden))


def test_composite_clean_forward(golden):
    """fused within 1e-4, logits within 2e-4 x scale, argmax agreement 99.9 %: the tolerances of
    tests/test_seg_gpu.py::test_full_model_config1_4x64x96."""
    g = golden("gr_drdb_attack")
    C.composite_clean_forward(_in_composite(golden), g, start=int(g["start"]), fused_atol=1e-4, logits_rtol=2e-4, agreement=0.999)


def test_attack_both_pgd_through_the_network(golden, exact_arithmetic):
    """Losses rtol 1e-4, sign and delta mismatch <= 2e-3, against the reference's float32 trace."""
    g = golden("gr_drdb_attack")
    C.attack_both_pgd(_in_composite(golden), g, start=int(g["start"]), eps=EPS, alpha=ALPHA, loss_rtol=1e-4, frac=2e-3)


def test_pgd_iterations_replayed_from_a_graph_are_bit_identical(golden):
    """Three PGD iterations captured once with torch.cuda.graph and replayed = the eager loop.  Single stream, no parallel branches; every
    weight pack is built (and the PReLU slope read) before the capture."""
    g = golden("gr_drdb_attack")
    C.pgd_iterations_replayed_from_a_graph_are_bit_identical(_in_composite(golden), start=int(g["start"]),
                                                             delta0=lambda ir, vis: (t(g["d0_ir"]), t(g["d0_vis"])), eps=EPS, alpha=ALPHA)


def test_robustness_harnesses_run_with_the_network(golden):
    """val_segformer_robust2 (clean) and val_segformer_robust (PGD, 2 iterations) on two 2x64x96 batches: finite mIoU, and the clean one is
    what the confusion matrix of the model's own seg_map argmax gives."""
    C.robustness_harnesses_run(_in_composite(golden), miou_atol=1e-12, attack_iters=2)
