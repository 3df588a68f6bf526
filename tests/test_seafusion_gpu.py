"""GPU: the SeAFusion baseline (paif_amd/fusion_model/seafusion.py, csrc/seafusion.hip, csrc/conv_slab.h) against the reference's own
outputs and autograd (tests/golden/gs_seafusion*.npz, generated on the CPU by tools/make_golden_seafusion.py), and inside the composite
model / attack / harness flow of the searched network.

Bound of the kernel parity checks (tests/baseline_common.py: bound): with floor = max|ref32 - ref64| of the same tensor,
max|hip - ref64| <= 1.5 * floor + 1e-5 * max(1, max|ref64|).  One kernel form exists (exact fp32, the 3x3 and 1x1 convs on
v_mfma_f32_16x16x4_f32); it is the default build.

In the fixtures i1 is the infrared plane and enters image_vis, i2 is the visible Y plane and enters image_ir: the order inside the
composite model.

The reference's autograd is the yardstick of the input gradients only where none of the 688 sign points per pixel (LeakyReLU inputs at both
slopes, depthwise responses under abs) is within fp32 reach of zero (the five small cases, see the tool).  At 1x37x53 and 2x24x32 the
reverse pass is tested as what it is given its tape -- a linear map -- against a float64 restatement that takes its LeakyReLU branches and
tanh' from the tape itself and the signs of the depthwise responses from a float64 recomputation on the taped input map."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from paif_amd import ops, synthetic as S
from tests import baseline_common as C
from tests.baseline_common import check, dev, exact_arithmetic, floor  # noqa: F401  (exact_arithmetic is a fixture)
from tests.helpers import t

pytestmark = pytest.mark.gpu

GRAD_CASES = ("1x4x5", "1x13x17", "2x9x20", "1x5x37", "1x19x18")
LARGE = ("1x37x53", "2x24x32")
SMALL = ("1x4x5", "1x13x17")
MAP_CHANNELS = [16, 16, 16, 16, 32, 32, 32, 32, 48] * 2 + [64, 32, 16]
HALO = 10           # the ten 3 x 3 convs on the longest path
EPS, ALPHA = 8 / 255., 2 / 255.
_SD = {}


def _sd(golden):
    """The fixture weights, rebuilt once from the thirty scales and the shift."""
    if not _SD:
        g = golden("gs_seafusion")
        _SD.update({k: torch.from_numpy(np.asarray(v)) for k, v in S.seafusion_state_dict(g["scales"], g["shift"]).items()})
    return _SD


def _net(golden):
    from paif_amd.fusion_model.seafusion import SeaFusion

    net = SeaFusion().eval()
    net.load_state_dict(_sd(golden), strict=True)
    return net.requires_grad_(False).to(dev())


def _inputs(golden, case):
    g = golden("gs_seafusion_" + case)
    cot = g["cot"] if "cot" in g else S.make_feature(900 + len(case), g["i1"].shape)
    return t(g["i1"]).to(dev()), t(g["i2"]).to(dev()), t(cot).to(dev())


@pytest.mark.parametrize("case", GRAD_CASES + LARGE)
def test_fused_plane_matches_the_reference(golden, case):
    """1x4x5 is smaller than the total halo of 10 (all border), 1x13x17 is ragged in both directions with two tiles across, 2x9x20 has two
    images, 1x5x37 three tiles across with the last 5 pixels wide, 1x19x18 2 x 2 tiles ragged in both, 1x37x53 and 2x24x32 several tile
    rows and columns."""
    g = golden("gs_seafusion_" + case)
    net = _net(golden)
    i1, i2, _ = _inputs(golden, case)
    with torch.no_grad():
        out = net(i1, i2)
    assert out.grad_fn is None and out.shape == i1.shape
    check("fused", case, "fused", out, g["fused64"], floor(g["fused"], g["fused64"]), halo=HALO if case in LARGE else None)


@pytest.mark.parametrize("case", SMALL)
def test_feature_maps_match_the_reference(golden, case):
    """The 21 taped maps (592 channels: per stream the first conv, and per RGBD conv1, conv2, |convx| + |convy| and the output; decode4 ..
    decode2), each against its own floor."""
    parts = [golden("gs_seafusion_%s_maps%d" % (case, p)) for p in (0, 1)]
    net = _net(golden)
    i1, i2, _ = _inputs(golden, case)
    maps = net._features(i1, i2)
    assert [m.shape[1] for m in maps] == MAP_CHANNELS and sum(MAP_CHANNELS) == 592
    for k, m in enumerate(maps):
        g = parts[0 if k < 9 else 1]
        check("maps", case, "map%d" % k, m, g["map%d" % k], float(g["map_floor"][k]))


@pytest.mark.parametrize("case", GRAD_CASES)
def test_input_gradients_match_float64_autograd(golden, case):
    """d_i1, d_i2 for the fixture's cotangent on the fused plane, through forward + .backward()."""
    g = golden("gs_seafusion_" + case)
    net = _net(golden)
    i1, i2, cot = _inputs(golden, case)
    a, b = i1.clone().requires_grad_(True), i2.clone().requires_grad_(True)
    out = net(a, b)
    assert out.grad_fn is not None
    (out * cot).sum().backward()
    for name, mine in (("d_i1", a.grad), ("d_i2", b.grad)):
        check("grad", case, name, mine, g[name + "64"], floor(g[name], g[name + "64"]))


def _nchw(m):
    return m.permute(0, 3, 1, 2).contiguous()


def _taped_branches(sd, maps):
    """From the tape (on the CPU): per stream and RGBD the LeakyReLU masks and the signs of the two depthwise responses, recomputed in
    float64 from the taped input map -> (branches, keep): keep [B,1,H,W] is False where the 5 x 5 neighbourhood holds a response whose
    float64 magnitude is below the float32 floor of that response map (its sign is not decided at fp32)."""
    def mask(m, slope):
        return torch.where(_nchw(m) > 0, 1.0, slope)

    br, near = {}, None
    for s, name in enumerate(("vis", "inf")):
        s1, s2 = maps["slab1"][s].cpu(), maps["slab2"][s].cpu()
        br[name + "_conv"] = mask(s1[..., 0:16], 0.2)
        for r, slab, C, out in ((1, s1, 16, s2[..., 0:32]), (2, s2, 32, maps["enc"].cpu()[..., 48 * s:48 * s + 48])):
            p = "%s_rgbd%d" % (name, r)
            br[p + ".conv1"], br[p + ".conv2"], br[p + ".out"] = mask(slab[..., C:2 * C], 0.2), mask(slab[..., 2 * C:3 * C], 0.2), mask(out, 0.1)
            x = _nchw(slab[..., 0:C])
            for d in ("convx", "convy"):
                w = sd["%s.sobelconv.%s.weight" % (p, d)]
                r64 = F.conv2d(x.double(), w.double(), padding=1, groups=C)
                r32 = F.conv2d(x, w, padding=1, groups=C)
                floor = (r32.double() - r64).abs().max()
                br["%s.%s" % (p, d)] = torch.sign(r64)
                n = (r64.abs() < floor).double().amax(1, keepdim=True)
                near = n if near is None else torch.maximum(near, n)
    for k in ("dec4", "dec3", "dec2"):
        br[k] = mask(maps[k].cpu(), 0.2)
    keep = F.max_pool2d(near, 5, stride=1, padding=2) == 0
    return br, keep.numpy()


def _linearised(sd, br, dtanh, i1, i2, cot, dtype):
    """The network with every LeakyReLU replaced by the constant mask of its taped map, abs by the constant sign, the tanh by its taped
    derivative, biases dropped: what the reverse pass transposes.  -> (d_i1, d_i2) for the cotangent, by torch's CPU autograd in `dtype`."""
    def w(name):
        return sd[name + ".weight"].to(dtype)

    def m(name):
        return br[name].to(dtype)

    a, b = i1.to(dtype).clone().requires_grad_(True), i2.to(dtype).clone().requires_grad_(True)
    enc = []
    for name, plane in (("vis", a), ("inf", b)):
        x = F.conv2d(plane, w(name + "_conv.conv"), padding=1) * m(name + "_conv")
        for r in (1, 2):
            p = "%s_rgbd%d" % (name, r)
            C = x.shape[1]
            x1 = F.conv2d(x, w(p + ".dense.conv1.conv"), padding=1) * m(p + ".conv1")
            x2 = F.conv2d(torch.cat((x, x1), 1), w(p + ".dense.conv2.conv"), padding=1) * m(p + ".conv2")
            g = (F.conv2d(x, w(p + ".sobelconv.convx"), padding=1, groups=C) * m(p + ".convx")
                 + F.conv2d(x, w(p + ".sobelconv.convy"), padding=1, groups=C) * m(p + ".convy"))
            x = (F.conv2d(torch.cat((x, x1, x2), 1), w(p + ".convdown.conv")) + F.conv2d(g, w(p + ".convup.conv"))) * m(p + ".out")
        enc.append(x)
    x = torch.cat(enc, 1)
    for k, name in (("dec4", "decode4"), ("dec3", "decode3"), ("dec2", "decode2")):
        x = F.conv2d(x, w(name + ".conv"), padding=1) * m(k)
    y = F.conv2d(x, w("decode1.conv"), padding=1) * dtanh.to(dtype)
    (y * cot.to(dtype)).sum().backward()
    return a.grad.numpy(), b.grad.numpy()


@pytest.mark.parametrize("case", LARGE)
def test_reverse_pass_matches_its_float64_restatement_on_the_taped_branches(golden, case):
    """Sizes the margin condition cannot reach.  A LeakyReLU sign the GPU forward decided differently from the reference cannot enter: the
    branches are the tape's.  The sign under abs is recomputed in float64 from the taped input map; where the fp32 response is too close
    to zero for that (5 x 5 around it) the output pixel is left out, at most 1 % of them.  A wrong tap, slice offset or mask shows at order
    0.1.  The floor is the same restatement in float32."""
    net = _net(golden)
    i1, i2, cot = _inputs(golden, case)
    tape = {}
    with torch.no_grad():
        net.forward_impl(i1, i2, tape=tape)
        d1, d2 = net.backward_impl(cot, tape)
    br, keep = _taped_branches(_sd(golden), tape["maps"])
    share = 1.0 - float(keep.mean())
    print("taped-mask reverse %s: excluded share %.5f (the reference's own: %.5f)" % (case, share, float(golden("gs_seafusion")["case_" + case][4])))
    assert share <= 0.01
    tt = 2 * tape["out"].cpu().double() - 1
    dtanh = 0.5 * (1 - tt * tt)
    r64 = _linearised(_sd(golden), br, dtanh, i1.cpu(), i2.cpu(), cot.cpu(), torch.float64)
    r32 = _linearised(_sd(golden), br, dtanh, i1.cpu(), i2.cpu(), cot.cpu(), torch.float32)
    for name, mine, a64, a32 in (("d_i1", d1, r64[0], r32[0]), ("d_i2", d2, r64[1], r32[1])):
        check("taped-mask reverse", case, name, mine, a64, floor(a32, a64), halo=HALO, keep=keep)


def _flat(tape):
    m = tape["maps"]
    return [tape["out"]] + m["slab1"] + m["slab2"] + [m["enc"], m["dec4"], m["dec3"], m["dec2"]] + m["sgn"]


def test_reverse_pass_is_linear_in_the_cotangent(golden):
    """backward_impl(g1) + backward_impl(g2) = backward_impl(g1 + g2) to fp32 rounding: within 1e-4 of the largest gradient
    (tests/baseline_common.py says why)."""
    C.reverse_pass_is_linear_in_the_cotangent(_net(golden), *_inputs(golden, "1x19x18"), rtol=1e-4)


def test_two_runs_are_bit_identical(golden):
    C.two_runs_are_bit_identical(_net(golden), *_inputs(golden, "2x24x32"), taped=_flat)


def test_channel_slices_are_taken_without_a_copy(golden):
    """The composite hands over ir[:, 0:1] and ycc of multi-channel tensors: planes addressed through their batch stride.  forward itself
    takes image_vis[:, :1] of any channel count."""
    net = _net(golden)
    fa, wide1, wide2 = C.channel_slices_are_taken_without_a_copy(net, *_inputs(golden, "2x24x32"))
    with torch.no_grad():
        assert torch.equal(fa, net(wide1, wide2[:, 0:1]))


def test_settings_that_do_not_apply_change_nothing(golden):
    """One arithmetic: the storage mode, the conv / GEMM precision and two_stream leave every bit where it is."""
    C.settings_that_do_not_apply_change_nothing(_net(golden), *_inputs(golden, "1x13x17"), fp32_maps=lambda tape: _flat(tape)[:-4])


def test_wrong_planes_are_refused_on_the_device(golden):
    net = _net(golden)
    z = torch.zeros(1, 1, 8, 8, device=dev())
    with pytest.raises(TypeError, match="fp32"):
        net(z.half(), z.half())
    with pytest.raises(ValueError, match=r"\[B,1,H,W\]"):
        net(z, torch.zeros(1, 1, 8, 9, device=dev()))
    with pytest.raises(ValueError, match=r"\[B,1,H,W\]"):                      # image_ir has one channel
        net(torch.zeros(1, 3, 8, 8, device=dev()), torch.zeros(1, 3, 8, 8, device=dev()))
    trainable = _net(golden).requires_grad_(True)
    with pytest.raises(NotImplementedError, match="[Pp]arameter gradients"):
        trainable(z, z)
    with ops.no_param_grads():                                  # an attack's forward: input gradients only
        a = z.clone().requires_grad_(True)
        out = trainable(a, z)
        out.sum().backward()
    assert a.grad is not None and all(p.grad is None for p in trainable.parameters())


def test_train_mode_equals_eval_mode_bit_for_bit(golden):
    """The decoder's BatchNorm modules are owned and never applied: their (non-trivial) fixture values and the mode change no bit, and no
    running statistic moves."""
    net = _net(golden)
    i1, i2, cot = _inputs(golden, "1x13x17")
    before = {k: v.clone() for k, v in net.state_dict().items() if ".bn." in k}
    assert len(before) == 20 and float((before["decode4.bn.running_mean"]).abs().max()) > 0
    with torch.no_grad():
        tape = {}
        base = (net.forward_impl(i1, i2, tape=tape),) + tuple(net.backward_impl(cot, tape))
        net.train()
        tape = {}
        got = (net.forward_impl(i1, i2, tape=tape),) + tuple(net.backward_impl(cot, tape)) + (net(i1, i2),)
    for x, y in zip(base + (base[0],), got):
        assert torch.equal(x, y)
    for k, v in net.state_dict().items():
        if ".bn." in k:
            assert torch.equal(v, before[k]), k


def _eager(net, image_vis, image_ir):
    """fusion_model/SeaFusion.py:105-125 restated with torch's own convs on the module's parameters."""
    def cl(mod, x):
        return F.leaky_relu(F.conv2d(x, mod.conv.weight, mod.conv.bias, padding=1), 0.2)

    def rgbd(blk, x):
        C = x.shape[1]
        x1 = torch.cat((x, cl(blk.dense.conv1, x)), 1)
        x1 = torch.cat((x1, cl(blk.dense.conv2, x1)), 1)
        x1 = F.conv2d(x1, blk.convdown.conv.weight, blk.convdown.conv.bias)
        g = (F.conv2d(x, blk.sobelconv.convx.weight, None, padding=1, groups=C).abs()
             + F.conv2d(x, blk.sobelconv.convy.weight, None, padding=1, groups=C).abs())
        return F.leaky_relu(x1 + F.conv2d(g, blk.convup.conv.weight, blk.convup.conv.bias), 0.1)

    v = rgbd(net.vis_rgbd2, rgbd(net.vis_rgbd1, cl(net.vis_conv, image_vis[:, :1])))
    i = rgbd(net.inf_rgbd2, rgbd(net.inf_rgbd1, cl(net.inf_conv, image_ir)))
    x = cl(net.decode2, cl(net.decode3, cl(net.decode4, torch.cat((v, i), 1))))
    return torch.tanh(F.conv2d(x, net.decode1.conv.weight, net.decode1.conv.bias, padding=1)) / 2 + 0.5


def test_reference_initialisation_matches_torch_eager(golden):
    """A net as the constructor leaves it: torch's default conv initialisation and the Sobel stencils in convx / convy, the values a user's
    checkpoint is most likely to hold there (exact zeros among the taps, exact-zero responses on flat patches)."""
    from paif_amd.fusion_model.seafusion import SeaFusion

    torch.manual_seed(20)
    net = SeaFusion().eval().requires_grad_(False).to(dev())
    sob = torch.tensor([[1., 0., -1.], [2., 0., -2.], [1., 0., -1.]], device=dev())
    assert torch.equal(net.vis_rgbd2.sobelconv.convx.weight, sob.expand(32, 1, 3, 3))
    assert torch.equal(net.inf_rgbd1.sobelconv.convy.weight, sob.t().expand(16, 1, 3, 3))
    i1, i2, _ = _inputs(golden, "1x13x17")
    with torch.no_grad():
        mine, ref = net(i1, i2), _eager(net, i1, i2)
    err = float((mine - ref).abs().max())
    print("reference initialisation: err %.3e (fused in [%.3f, %.3f])" % (err, float(ref.min()), float(ref.max())))
    assert float(ref.max() - ref.min()) > 1e-3
    assert err <= 1e-5


# ---- inside the composite model ------------------------------------------------------------------------------------------------
def _in_composite(golden):
    """The network with the fixture's weights as the fusion module of Network_MM_CompModel."""
    from paif_amd.fusion_model.seafusion import SeaFusion

    return C.composite(SeaFusion(), _sd(golden))


def test_composite_clean_forward(golden):
    """fused within 1e-4, logits within 2e-4 x scale, argmax agreement 99.9 %: the tolerances of
    tests/test_seg_gpu.py::test_full_model_config1_4x64x96."""
    g = golden("gs_seafusion_attack")
    C.composite_clean_forward(_in_composite(golden), g, start=int(g["start"]), fused_atol=1e-4, logits_rtol=2e-4, agreement=0.999)


def test_attack_both_pgd_through_the_baseline(golden, exact_arithmetic):
    """Losses rtol 1e-4, sign and delta mismatch <= 2e-3, against the reference's float32 trace."""
    g = golden("gs_seafusion_attack")
    C.attack_both_pgd(_in_composite(golden), g, start=int(g["start"]), eps=EPS, alpha=ALPHA, loss_rtol=1e-4, frac=2e-3)


def test_pgd_iterations_replayed_from_a_graph_are_bit_identical(golden):
    """Three PGD iterations captured once with torch.cuda.graph and replayed = the eager loop.  Single stream, no parallel branches; every
    weight pack is built before the capture."""
    g = golden("gs_seafusion_attack")
    C.pgd_iterations_replayed_from_a_graph_are_bit_identical(_in_composite(golden), start=int(g["start"]),
                                                             delta0=lambda ir, vis: (t(g["d0_ir"]), t(g["d0_vis"])), eps=EPS, alpha=ALPHA)


def test_robustness_harnesses_run_with_the_baseline(golden):
    """val_segformer_robust2 (clean) and val_segformer_robust (PGD, 2 iterations) on two 2x64x96 batches: finite mIoU, and the clean one is
    what the confusion matrix of the model's own seg_map argmax gives."""
    C.robustness_harnesses_run(_in_composite(golden), miou_atol=1e-12, attack_iters=2)
