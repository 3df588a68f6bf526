"""GPU: the hand-designed fusion network (paif_amd/fusion_model/drdb.py, csrc/drdb.hip, csrc/conv_slab.h) against the reference's own
outputs and autograd (tests/golden/gr_drdb*.npz, generated on the CPU by tools/make_golden_drdb.py), and inside the composite model /
attack / harness flow of the searched network.

Bound of the kernel parity checks (tests/test_u2fusion_gpu.py): with floor = max|ref32 - ref64| of the same tensor,
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
from tests import helpers as Hh
from tests.helpers import t, maxabs

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


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


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
    return net.requires_grad_(False).to(_dev())


def _inputs(golden, case, which="A"):
    g = golden("gr_drdb_%s_%s" % (case, which))
    cot = g["cot"] if "cot" in g else S.make_feature(900 + len(case), g["i1"].shape)
    return t(g["i1"]).to(_dev()), t(g["i2"]).to(_dev()), t(cot).to(_dev())


def _bound(floor, ref64):
    return 1.5 * floor + 1e-5 * max(1.0, float(np.abs(ref64).max()))


def _floor(ref32, ref64):
    return float(np.abs(np.asarray(ref32).astype(np.float64) - ref64).max())


def _border(a):
    """The outermost HALO rows / columns of [..., H, W] (everything, where the plane is smaller than twice the halo)."""
    m = np.ones(a.shape[-2:], dtype=bool)
    m[HALO:-HALO, HALO:-HALO] = False
    return a[..., m]


def _check(what, case, name, mine, ref64, floor, border=False):
    got = mine.detach().cpu().numpy().astype(np.float64)
    assert got.shape == ref64.shape
    bound = _bound(floor, ref64)
    err = float(np.abs(got - ref64).max())
    print("%s %s %s: err %.3e bound %.3e ratio %.3f scale %.3e" % (what, case, name, err, bound, err / bound, float(np.abs(ref64).max())))
    assert err <= bound, (name, err, bound)
    if border:
        eb = float(np.abs(_border(got) - _border(ref64)).max())
        print("%s %s %s border: err %.3e bound %.3e ratio %.3f" % (what, case, name, eb, bound, eb / bound))
        assert eb <= bound, (name, "border", eb, bound)


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
    _check("fused", case + which, "fused", out, g["fused64"], _floor(g["fused"], g["fused64"]), border=case in LARGE)


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
        _check("maps", case, "map%d" % k, m, g["map%d" % k], float(g["map_floor"][k]))


def _block(golden):
    from paif_amd.fusion_model.drdb import DRDB

    blk = DRDB().eval()
    blk.load_state_dict({k[len("DRDB1."):]: v for k, v in _sd(golden).items() if k.startswith("DRDB1.")}, strict=True)
    return blk.requires_grad_(False).to(_dev())


@pytest.mark.parametrize("case", SMALL)
def test_a_block_alone_forward_and_reverse(golden, case):
    """DRDB as a module of its own, [B,64,H,W] -> [B,64,H,W], on the map conv1 + PReLU gave; its input gradient through .backward()."""
    g = golden("gr_drdb_%s_block" % case)
    blk = _block(golden)
    x = t(g["x"]).to(_dev())
    with torch.no_grad():
        out = blk(x)
    assert out.grad_fn is None
    _check("block", case, "out", out, g["out64"], _floor(g["out"], g["out64"]))
    a = x.clone().requires_grad_(True)
    out = blk(a)
    assert out.grad_fn is not None
    (out * t(g["cot"]).to(_dev())).sum().backward()
    _check("block", case, "d_x", a.grad, g["d_x64"], _floor(g["d_x"], g["d_x64"]))


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
        _check("grad", case + which, name, mine, g[name + "64"], _floor(g[name], g[name + "64"]))


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
    _check("batch", "2x9x20B", "fused", both, g["fused64"], _floor(g["fused"], g["fused64"]))
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
        _check("taped-mask reverse", case, name, mine, a64, _floor(a32, a64), border=True)


def _flat(tape):
    m = tape["maps"]
    return [tape["out"]] + m["slab"] + m["r6"] + [m["f2"], m["c2"], m["f"], m["minmax"]]


@pytest.mark.parametrize("which", ("A", "B"))
def test_reverse_pass_is_linear_in_the_cotangent(golden, which):
    """backward_impl(g1) + backward_impl(g2) = backward_impl(g1 + g2) to fp32 rounding (tests/test_u2fusion_gpu.py's check and bound)."""
    net = _net(golden, which)
    i1, i2, cot = _inputs(golden, "1x19x18", which)
    tape = {}
    with torch.no_grad():
        net.forward_impl(i1, i2, tape=tape)
        g2 = t(S.make_feature(77, tuple(cot.shape))).to(_dev())
        r1, r2, r12 = net.backward_impl(cot, tape), net.backward_impl(g2, tape), net.backward_impl(ops.add(cot, g2), tape)
    for x, y, z in zip(r1, r2, r12):
        scale = max(1.0, float(z.abs().max()))
        err = float((x + y - z).abs().max())
        print("linearity %s: err %.3e scale %.3e" % (which, err, scale))
        assert err <= 1e-4 * scale


def test_two_runs_are_bit_identical(golden):
    net = _net(golden)
    i1, i2, cot = _inputs(golden, "2x24x32")
    runs = []
    with torch.no_grad():
        for _ in range(2):
            tape = {}
            f = net.forward_impl(i1, i2, tape=tape)
            runs.append([f] + _flat(tape) + list(net.backward_impl(cot, tape)))
    for x, y in zip(*runs):
        assert torch.equal(x, y)


def test_channel_slices_are_taken_without_a_copy(golden):
    """The composite hands over ir[:, 0:1] and ycc of multi-channel tensors: planes addressed through their batch stride.  forward itself
    takes channel 0 of both inputs, as the reference does."""
    net = _net(golden)
    i1, i2, cot = _inputs(golden, "2x24x32")
    wide1 = torch.cat([i1, i1 * 0.5, i1 * 0.25], 1).contiguous()
    wide2 = torch.cat([i2, i2 * 0.5], 1).contiguous()
    with torch.no_grad():
        ta, tb = {}, {}
        fa = net.forward_impl(i1, i2, tape=ta)
        fb = net.forward_impl(wide1, wide2, tape=tb)
        assert torch.equal(fa, fb)
        assert torch.equal(fa, net(wide1, wide2))
        assert torch.equal(fa, net(wide1[:, 0:1], wide2[:, 0:1]))
        for x, y in zip(net.backward_impl(cot, ta), net.backward_impl(cot, tb)):
            assert torch.equal(x, y)


def test_settings_that_do_not_apply_change_nothing(golden):
    """One arithmetic: the storage mode, the conv / GEMM precision and two_stream leave every bit where it is."""
    net = _net(golden)
    i1, i2, cot = _inputs(golden, "1x13x17")
    with torch.no_grad():
        tape = {}
        base = (net.forward_impl(i1, i2, tape=tape),) + tuple(net.backward_impl(cot, tape))
    old = dict(ops.CONFIG)
    try:
        for storage, conv, gemm, two in (("bf16", "f32", "f32", True), ("f16", "bf16x3", "bf16x3", False)):
            ops.set_storage(storage), ops.set_conv_precision(conv), ops.set_gemm_precision(gemm)
            ops.CONFIG["two_stream"] = two
            with torch.no_grad():
                tape = {}
                got = (net.forward_impl(i1, i2, tape=tape),) + tuple(net.backward_impl(cot, tape))
            assert all(x.dtype == torch.float32 for x in _flat(tape))
            for x, y in zip(base, got):
                assert torch.equal(x, y)
    finally:
        ops.set_storage(old["storage"]), ops.set_conv_precision(old["conv_precision"]), ops.set_gemm_precision(old["gemm_precision"])
        ops.CONFIG["two_stream"] = old["two_stream"]


def test_wrong_planes_are_refused_on_the_device(golden):
    net = _net(golden)
    z = torch.zeros(1, 1, 8, 8, device=_dev())
    with pytest.raises(TypeError, match="fp32"):
        net(z.half(), z.half())
    with pytest.raises(ValueError, match=r"\[B,1,H,W\]"):
        net(z, torch.zeros(1, 1, 8, 9, device=_dev()))
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
    net = Fusion_Network().eval().requires_grad_(False).to(_dev())
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
@pytest.fixture
def exact_arithmetic():
    """The setting tests/test_attack_gpu.py asserts gradient parity under: exact-fp32 conv and GEMM kernels."""
    old, oldg = ops.CONFIG["conv_precision"], ops.CONFIG["gemm_precision"]
    ops.set_conv_precision("f32")
    ops.set_gemm_precision("f32")
    yield
    ops.set_conv_precision(old)
    ops.set_gemm_precision(oldg)


def _composite(golden):
    """As tests/test_u2fusion_gpu.py:_composite, with Fusion_Network as the fusion module; its weights are the fixture's set A."""
    from paif_amd.core.model_fusion_auto import Fusion_Network, Network_MM_CompModel

    m = Network_MM_CompModel(Fusion_Network(), None, None, "mit_b0", num_classes=9).eval()
    S.load_formula_weights(m, head=Hh.HEAD64["mit_b0"])
    m.enhance_net.load_state_dict(_sd(golden), strict=True)
    return m.to(_dev())


def _batch(start=0):
    ir, vis, lab = S.make_batch(2, 64, 96, start=start)
    return t(ir).to(_dev()), t(vis).to(_dev()), t(lab).to(_dev())


def _scale(a):
    return max(1.0, float(np.abs(a).max()))


def test_composite_clean_forward(golden):
    """Tolerances of tests/test_u2fusion_gpu.py::test_composite_clean_forward: fused 1e-4, logits 2e-4 x scale, argmax agreement 99.9 %."""
    g = golden("gr_drdb_attack")
    m = _composite(golden)
    ir, vis, lab = _batch(int(g["start"]))
    with torch.no_grad():
        fused, seg = m(ir, vis)
    print("composite: fused err %.3e logits err %.3e (scale %.3e)" % (maxabs(fused.cpu(), g["fused"]), maxabs(seg.cpu(), g["logits"]),
                                                                    _scale(g["logits"])))
    assert maxabs(fused.cpu(), g["fused"]) <= 1e-4
    assert maxabs(seg.cpu(), g["logits"]) <= 2e-4 * _scale(g["logits"])
    up = torch.nn.functional.interpolate(seg.cpu(), size=lab.shape[1:], mode="bilinear", align_corners=False)
    agree = (up.argmax(1).numpy() == g["pred"]).mean()
    print("composite: argmax agreement %.5f" % agree)
    assert agree >= 0.999


def _check_attack(g, d_ir, d_vis, trace, loss_rtol, frac):
    """tests/test_attack_gpu.py:_check_attack."""
    losses = np.array([s["loss"] for s in trace])
    np.testing.assert_allclose(losses, g["losses"], rtol=loss_rtol)
    for mine, ref in ((trace[-1]["g_ir"], g["gsum_ir"]), (trace[-1]["g_vis"], g["gsum_vis"])):
        mism = (np.sign(mine.cpu().numpy()) != np.sign(ref)).mean()
        print("attack: sign mismatch of the running sum %.2e" % mism)
        assert mism <= frac
    for mine, ref in ((d_ir, g["delta_ir"]), (d_vis, g["delta_vis"])):
        a = mine.detach().cpu().numpy()
        diff = (np.abs(a - ref) > 1e-6).mean()
        print("attack: share of differing delta elements %.2e" % diff)
        assert diff <= frac
        assert np.abs(a).max() <= 8 / 255. + 1e-7


def test_attack_both_pgd_through_the_network(golden, exact_arithmetic):
    from paif_amd.attack.attack import attack_both

    g = golden("gr_drdb_attack")
    m = _composite(golden)
    assert hasattr(m, "forward_taped")                       # the fast path of attack.py is the one taken
    ir, vis, lab = _batch(int(g["start"]))
    trace = []
    with torch.no_grad():
        d_ir, d_vis = attack_both(m, vis, ir, lab, epsilon=EPS, alpha=ALPHA, attack_iters=3, attack_loss='l_seg', attack_way='PGD',
                                  delta0_ir=t(g["d0_ir"]), delta0_vis=t(g["d0_vis"]), trace=trace)
    for s in trace:
        assert s["g_ir"].grad_fn is None and s["g_vis"].grad_fn is None and not s["g_ir"].requires_grad
    print("attack: losses %s reference %s" % ([s["loss"] for s in trace], list(g["losses"])))
    _check_attack(g, d_ir, d_vis, trace, 1e-4, 2e-3)


def _pgd_iterations(m, ir, vis, lab64, d_ir, d_vis, g_ir, g_vis, gs, iters):
    """The fast path of attack.py:_attack_loop, in place on d_*, g_* (so that it can be captured)."""
    for i in range(iters):
        with ops.attack_forward_arithmetic():
            _, logits, tape = m.forward_taped(ops.add(ir, d_ir), ops.add(vis, d_vis))
        way, wt, wf = ops.attack_loss_weights('PGD', i, iters)
        coef = ops.attack_loss_fwd(logits, lab64, way, wt, wf)
        d32 = ops.attack_loss_bwd(logits, lab64, coef, way, wt, wf, upstream=gs)
        with ops.attack_backward_arithmetic():
            gi, gv = m.backward_taped(d32, tape)
        ops.axpy_(g_ir, gi.contiguous(), 1.0 / gs)
        ops.pgd_step_(d_ir, g_ir, ir, ALPHA, EPS)
        ops.axpy_(g_vis, gv.contiguous(), 1.0 / gs)
        ops.pgd_step_(d_vis, g_vis, vis, ALPHA, EPS)


def test_pgd_iterations_replayed_from_a_graph_are_bit_identical(golden):
    """Three PGD iterations captured once with torch.cuda.graph and replayed = the eager loop.  Single stream, no parallel branches; every
    weight pack is built (and the PReLU slope read) before the capture."""
    g = golden("gr_drdb_attack")
    m = _composite(golden)
    ir, vis, lab = _batch(int(g["start"]))
    lab64 = lab.type(torch.long).contiguous()
    d0_ir, d0_vis = t(g["d0_ir"]).to(_dev()), t(g["d0_vis"]).to(_dev())
    state = [torch.zeros_like(x) for x in (ir, vis, ir, vis)]

    def reset():
        state[0].copy_(d0_ir), state[1].copy_(d0_vis), state[2].zero_(), state[3].zero_()

    gstream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), ops.attack_arithmetic():
        gs = ops.attack_grad_scale(lab64)
        reset()
        _pgd_iterations(m, ir, vis, lab64, *state, gs, 3)     # eager: also builds every weight pack outside the capture
        eager = [x.clone() for x in state]
        torch.cuda.synchronize()
        with torch.cuda.stream(gstream):
            reset()
            _pgd_iterations(m, ir, vis, lab64, *state, gs, 3)
            torch.cuda.synchronize()
            with torch.cuda.graph(graph, stream=gstream):
                _pgd_iterations(m, ir, vis, lab64, *state, gs, 3)
        torch.cuda.synchronize()
        reset()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
    assert float(eager[2].abs().max()) > 0
    for x, y in zip(eager, state):
        assert torch.equal(x, y)


def test_robustness_harnesses_run_with_the_network(golden):
    """val_segformer_robust2 (clean) and val_segformer_robust (PGD, 2 iterations) on two 2x64x96 batches: finite mIoU, and the clean one is
    what the confusion matrix of the model's own seg_map argmax gives."""
    from oracle import paif_oracle as O
    from paif_amd.harness import val_segformer_robust, val_segformer_robust2

    m = _composite(golden)
    batches = []
    for start in (0, 2):
        ir, vis, lab = _batch(start)
        batches.append((vis, ir, lab))
    clean = val_segformer_robust2(m, batches)
    conf = np.zeros((9, 9), dtype=np.int64)
    with torch.no_grad():
        for vis, ir, lab in batches:
            _, seg = m(ir, vis)
            up = torch.nn.functional.interpolate(seg.cpu(), size=lab.shape[1:], mode="bilinear", align_corners=False)
            conf += O.confusion_matrix(lab.cpu().numpy(), up.argmax(1).numpy())
    iou = O.compute_results(conf)[2]
    assert np.isfinite(clean["miou"])
    assert abs(clean["miou"] - float(np.mean(np.nan_to_num(iou)))) <= 1e-12
    rob = val_segformer_robust(m, batches, attack_iters=2)
    assert np.isfinite(rob["miou"])
