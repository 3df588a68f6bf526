"""GPU: the DIDFuse baseline (paif_amd/fusion_model/didfuse.py, csrc/didfuse.hip, csrc/conv_slab.h) against the reference's own outputs
and autograd (tests/golden/gd_didfuse*.npz, generated on the CPU by tools/make_golden_didfuse.py, the reference in .eval() mode), and
inside the composite model / attack / harness flow of the searched network.

Bound of the kernel parity checks (tests/baseline_common.py: bound): with floor = max|ref32 - ref64| of the same tensor,
max|hip - ref64| <= 1.5 * floor + 1e-5 * max(1, max|ref64|).  One kernel form exists (exact fp32, the 64- and 128-channel convs on
v_mfma_f32_16x16x4_f32, BatchNorm folded into the weights); it is the default build.

In the fixtures i1 is the infrared plane and enters x_over (AE_Encoder1), i2 is the visible Y plane and enters x_under (AE_Encoder2): the
order inside the composite model.

The reference's autograd is the yardstick of the input gradients only where none of the 384 sign points per pixel (the six PReLU inputs)
is within fp32 reach of zero (the six small cases, see the tool).  At 1x37x53 and 2x24x32 the reverse pass is tested as what it is given
its tape -- a linear map -- against a float64 restatement that takes its PReLU branches, tanh' and sigmoid' from the tape itself.  Nothing
there depends on a sign recomputed off the tape, so no pixel is excluded."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from paif_amd import ops, synthetic as S
from tests import baseline_common as C
from tests.baseline_common import check, dev, exact_arithmetic, floor  # noqa: F401  (exact_arithmetic is a fixture)
from tests.helpers import t

pytestmark = pytest.mark.gpu

GRAD_CASES = ("1x2x3", "1x4x5", "1x13x17", "2x9x20", "1x5x37", "1x19x18")
LARGE = ("1x37x53", "2x24x32")
SMALL = ("1x4x5", "1x13x17")
HALO = 6            # cov1, cov2, cov3 | cov4, cov5, cov6, cov7: the 3 x 3 convs on the longest path
EPS, ALPHA = 8 / 255., 2 / 255.
_SD = {}


def _sd(golden):
    """The fixture weights, rebuilt once from the eleven scales and the shift."""
    if not _SD:
        g = golden("gd_didfuse")
        _SD.update({k: torch.from_numpy(np.asarray(v)) for k, v in S.didfuse_state_dict(g["scales"], g["shift"]).items()})
    return _SD


def _net(golden):
    from paif_amd.fusion_model.didfuse import DID

    net = DID().eval()
    net.load_state_dict(_sd(golden), strict=True)
    return net.requires_grad_(False).to(dev())


def _inputs(golden, case):
    g = golden("gd_didfuse_" + case)
    cot = g["cot"] if "cot" in g else S.make_feature(900 + len(case), g["i1"].shape)
    return t(g["i1"]).to(dev()), t(g["i2"]).to(dev()), t(cot).to(dev())


@pytest.mark.parametrize("case", GRAD_CASES + LARGE)
def test_fused_plane_matches_the_reference(golden, case):
    """1x2x3 is reflection padding at its smallest size (every read of row -1 and row H lands on the other row), 1x4x5 is smaller than the
    total halo (all border), 1x13x17 is ragged in both directions with two tiles across, 2x9x20 has two images, 1x5x37 three tiles across
    with the last 5 pixels wide, 1x19x18 2 x 2 tiles ragged in both, 1x37x53 and 2x24x32 several tile rows and columns."""
    g = golden("gd_didfuse_" + case)
    net = _net(golden)
    i1, i2, _ = _inputs(golden, case)
    with torch.no_grad():
        out = net(i1, i2)
    assert out.grad_fn is None and out.shape == i1.shape
    check("fused", case, "fused", out, g["fused64"], floor(g["fused"], g["fused64"]), halo=HALO if case in LARGE else None)


@pytest.mark.parametrize("case", SMALL)
def test_feature_maps_match_the_reference(golden, case):
    """The 14 taped maps (896 channels: per stream f1, f2, fB, fD; the means F_1, F_2, F_b, F_d; Out1, Out2), each against its own floor."""
    parts = [golden("gd_didfuse_%s_maps%d" % (case, p)) for p in (0, 1)]
    net = _net(golden)
    i1, i2, _ = _inputs(golden, case)
    maps = net._features(i1, i2)
    assert [m.shape[1] for m in maps] == [64] * 14
    for k, m in enumerate(maps):
        g = parts[0 if k < 8 else 1]
        check("maps", case, "map%d" % k, m, g["map%d" % k], float(g["map_floor"][k]))


@pytest.mark.parametrize("case", GRAD_CASES)
def test_input_gradients_match_float64_autograd(golden, case):
    """d_i1, d_i2 for the fixture's cotangent on the fused plane, through forward + .backward()."""
    g = golden("gd_didfuse_" + case)
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


_BLOCKS = {name.split(".")[0][3:].replace("Encoder", "E").replace("Decoder1", "D") + "." + name.split(".")[1]: (name, k)
           for name, k, _, _, _ in S.DIDFUSE_CONVS}      # "E1.cov1" -> ("AE_Encoder1.cov1.cov1", 1)


def _bn_eps(net):
    """BatchNorm prefix ("AE_Encoder1.cov1.cov1.2.") -> that module's eps."""
    return {name + ".": m.eps for name, m in net.named_modules() if isinstance(m, torch.nn.BatchNorm2d)}


def _linearised(sd, eps, maps, fused, i1, i2, cot, dtype):
    """The network with every PReLU replaced by the constant mask of its taped map, tanh and sigmoid by their taped derivatives
    (1 - t^2, f (1 - f)), every BatchNorm by its constant scale gamma / sqrt(var + eps) with the module's eps (_bn_eps), biases and shifts
    dropped, reflection padding by F.pad: what the reverse pass transposes.  -> (d_i1, d_i2) for the cotangent, by torch's CPU autograd in `dtype`."""
    def conv(x, block, pad):
        name, k = _BLOCKS[block]
        bn = "%s.%d." % (name, k + 1)
        sc = sd[bn + "weight"].to(dtype) / torch.sqrt(sd[bn + "running_var"].to(dtype) + eps[bn])
        x = F.pad(x, (1, 1, 1, 1), mode="reflect") if pad == "reflect" else F.pad(x, (1, 1, 1, 1))
        return F.conv2d(x, sd["%s.%d.weight" % (name, k)].to(dtype)) * sc.view(1, -1, 1, 1)

    def prelu(block, taped):
        name, k = _BLOCKS[block]
        return torch.where(_nchw(taped) > 0, 1.0, float(sd["%s.%d.weight" % (name, k + 2)])).to(dtype)

    def dtanh(taped):
        tt = _nchw(taped).to(dtype)
        return 1 - tt * tt

    a, b = i1.to(dtype).clone().requires_grad_(True), i2.to(dtype).clone().requires_grad_(True)
    f = []
    for s, (e, plane) in enumerate((("E1", a), ("E2", b))):
        enc = maps["enc"][s]
        f1 = conv(plane, e + ".cov1", "reflect") * prelu(e + ".cov1", enc[..., 0:64])
        f2 = conv(f1, e + ".cov2", "zero") * prelu(e + ".cov2", enc[..., 64:128])
        fb = conv(f2, e + ".cov3", "zero") * dtanh(enc[..., 128:192])
        fd = conv(f2, e + ".cov4", "zero") * dtanh(enc[..., 192:256])
        f.append((f1, f2, fb, fd))
    F1, F2, Fb, Fd = ((x + y) / 2 for x, y in zip(*f))
    o1 = conv(torch.cat((Fb, Fd), 1), "D.cov5", "zero") * prelu("D.cov5", maps["d1"][..., 0:64])
    o2 = conv(torch.cat((o1, F2), 1), "D.cov6", "zero") * prelu("D.cov6", maps["d2"][..., 0:64])
    ff = fused.to(dtype)
    y = conv(torch.cat((o2, F1), 1), "D.cov7", "reflect") * (ff * (1 - ff))
    (y * cot.to(dtype)).sum().backward()
    return a.grad.numpy(), b.grad.numpy()


def _cpu_maps(maps):
    return dict(enc=[m.cpu() for m in maps["enc"]], bd=maps["bd"].cpu(), d1=maps["d1"].cpu(), d2=maps["d2"].cpu())


@pytest.mark.parametrize("case", LARGE)
def test_reverse_pass_matches_its_float64_restatement_on_the_taped_branches(golden, case):
    """Sizes the margin condition cannot reach.  A PReLU sign the GPU forward decided differently from the reference cannot enter: the
    branches are the tape's, and so are tanh' and sigmoid'.  No pixel is excluded.  A wrong tap, slice offset, mask, missing 0.5 of a mean
    or a wrong reflected row shows at order 0.1.  The floor is the same restatement in float32."""
    assert _BLOCKS["E2.cov4"] == ("AE_Encoder2.cov4.cov4", 0) and _BLOCKS["D.cov7"] == ("AE_Decoder1.cov7.cov7", 1) and len(_BLOCKS) == 11
    net = _net(golden)
    i1, i2, cot = _inputs(golden, case)
    tape = {}
    with torch.no_grad():
        net.forward_impl(i1, i2, tape=tape)
        d1, d2 = net.backward_impl(cot, tape)
    maps, fused = _cpu_maps(tape["maps"]), tape["out"].cpu()
    r64 = _linearised(_sd(golden), _bn_eps(net), maps, fused, i1.cpu(), i2.cpu(), cot.cpu(), torch.float64)
    r32 = _linearised(_sd(golden), _bn_eps(net), maps, fused, i1.cpu(), i2.cpu(), cot.cpu(), torch.float32)
    for name, mine, a64, a32 in (("d_i1", d1, r64[0], r32[0]), ("d_i2", d2, r64[1], r32[1])):
        assert float(np.abs(a64).max()) > 1e-3
        check("taped-mask reverse", case, name, mine, a64, floor(a32, a64), halo=HALO)


def _flat(tape):
    m = tape["maps"]
    return [tape["out"]] + m["enc"] + [m["bd"], m["d1"], m["d2"]]


def test_reverse_pass_is_linear_in_the_cotangent(golden):
    """backward_impl(g1) + backward_impl(g2) = backward_impl(g1 + g2) to fp32 rounding: within 1e-4 of the largest gradient
    (tests/baseline_common.py says why)."""
    C.reverse_pass_is_linear_in_the_cotangent(_net(golden), *_inputs(golden, "1x19x18"), rtol=1e-4)


def test_two_runs_are_bit_identical(golden):
    C.two_runs_are_bit_identical(_net(golden), *_inputs(golden, "2x24x32"), taped=_flat)


def test_channel_slices_are_taken_without_a_copy(golden):
    """The composite hands over ir[:, 0:1] and ycc of multi-channel tensors: planes addressed through their batch stride."""
    C.channel_slices_are_taken_without_a_copy(_net(golden), *_inputs(golden, "2x24x32"))


def test_settings_that_do_not_apply_change_nothing(golden):
    """One arithmetic: the storage mode, the conv / GEMM precision and two_stream leave every bit where it is."""
    C.settings_that_do_not_apply_change_nothing(_net(golden), *_inputs(golden, "1x13x17"), fp32_maps=_flat)


def test_wrong_planes_and_modes_are_refused_on_the_device(golden):
    net = _net(golden)
    z = torch.zeros(1, 1, 8, 8, device=dev())
    with pytest.raises(TypeError, match="fp32"):
        net(z.half(), z.half())
    with pytest.raises(ValueError, match=r"\[B,1,H,W\]"):
        net(z, torch.zeros(1, 1, 8, 9, device=dev()))
    with pytest.raises(ValueError, match=r"\[B,1,H,W\]"):
        net(torch.zeros(1, 3, 8, 8, device=dev()), torch.zeros(1, 3, 8, 8, device=dev()))
    for shape in ((1, 1, 1, 8), (1, 1, 8, 1)):                   # as torch's ReflectionPad2d(1)
        with pytest.raises(ValueError, match="H, W >= 2"):
            net(torch.zeros(shape, device=dev()), torch.zeros(shape, device=dev()))
    trainable = _net(golden).requires_grad_(True)
    with pytest.raises(NotImplementedError, match="[Pp]arameter gradients"):
        trainable(z, z)
    with ops.no_param_grads():                                  # an attack's forward: input gradients only
        a = z.clone().requires_grad_(True)
        out = trainable(a, z)
        out.sum().backward()
    assert a.grad is not None and all(p.grad is None for p in trainable.parameters())
    # .train(): batch statistics are not built, and the running statistics are neither used in their place nor moved
    before = {k: v.clone() for k, v in net.state_dict().items()}
    net.train()
    with pytest.raises(NotImplementedError, match="BatchNorm"):
        with torch.no_grad():
            net(z, z)
    with pytest.raises(NotImplementedError, match="BatchNorm"):
        net.forward_impl(z, z, tape={})
    for k, v in net.state_dict().items():
        assert torch.equal(v, before[k]), k


def _eager(net, x_over, x_under):
    """fusion_model/AUIF.py restated with torch's own ops on the module's parameters and buffers (eval-mode BatchNorm)."""
    def block(seq, x):
        for m in seq:
            if isinstance(m, torch.nn.ReflectionPad2d):
                x = F.pad(x, (1, 1, 1, 1), mode="reflect")
            elif isinstance(m, torch.nn.Conv2d):
                x = F.conv2d(x, m.weight, m.bias, padding=m.padding)
            elif isinstance(m, torch.nn.BatchNorm2d):
                x = F.batch_norm(x, m.running_mean, m.running_var, m.weight, m.bias, training=False, eps=m.eps)
            elif isinstance(m, torch.nn.PReLU):
                x = F.prelu(x, m.weight)
            else:
                x = torch.tanh(x) if isinstance(m, torch.nn.Tanh) else torch.sigmoid(x)
        return x

    f = []
    for e, x in ((net.AE_Encoder1, x_over), (net.AE_Encoder2, x_under)):
        f1 = block(e.cov1.cov1, x)
        f2 = block(e.cov2.cov2, f1)
        f.append((f1, f2, block(e.cov3.cov3, f2), block(e.cov4.cov4, f2)))
    F1, F2, Fb, Fd = ((x + y) / 2 for x, y in zip(*f))
    d = net.AE_Decoder1
    o1 = block(d.cov5.cov5, torch.cat((Fb, Fd), 1))
    o2 = block(d.cov6.cov6, torch.cat((o1, F2), 1))
    return block(d.cov7.cov7, torch.cat((o2, F1), 1))


def test_reference_initialisation_matches_torch_eager(golden):
    """A net as the constructor leaves it: torch's default conv initialisation, identity BatchNorm, slopes 0.25."""
    from paif_amd.fusion_model.didfuse import DID

    torch.manual_seed(20)
    net = DID().eval().requires_grad_(False).to(dev())
    i1, i2, _ = _inputs(golden, "1x13x17")
    with torch.no_grad():
        mine, ref = net(i1, i2), _eager(net, i1, i2)
    err = float((mine - ref).abs().max())
    print("reference initialisation: err %.3e (fused in [%.3f, %.3f])" % (err, float(ref.min()), float(ref.max())))
    assert float(ref.max() - ref.min()) > 1e-3
    assert err <= 1e-5


def test_in_place_changes_of_buffers_and_slopes_rebuild_the_pack(golden):
    """The pack's key holds the BatchNorm buffers and the PReLU slopes: an in-place change of one running_var, then of one slope, changes
    the output, and it is torch eager's again (1e-5, the bound of the test above)."""
    net = _net(golden)
    i1, i2, _ = _inputs(golden, "1x13x17")
    with torch.no_grad():
        base = net(i1, i2)
        assert float((base - _eager(net, i1, i2)).abs().max()) <= 1e-5
        net.AE_Decoder1.cov5.cov5[1].running_var[::2].mul_(4.0)
        second = net(i1, i2)
        err = float((second - _eager(net, i1, i2)).abs().max())
        print("running_var changed: moved %.3e, err %.3e" % (float((second - base).abs().max()), err))
        assert float((second - base).abs().max()) > 1e-3 and err <= 1e-5
        net.AE_Encoder2.cov2.cov2[2].weight.fill_(0.6)
        third = net(i1, i2)
        err = float((third - _eager(net, i1, i2)).abs().max())
        print("slope changed: moved %.3e, err %.3e" % (float((third - second).abs().max()), err))
        assert float((third - second).abs().max()) > 1e-3 and err <= 1e-5
        net.AE_Encoder1.cov1.cov1[3].weight.fill_(-0.1)          # a negative slope: refused when the pack is rebuilt
        with pytest.raises(ValueError, match="slope"):
            net(i1, i2)


def test_batchnorm_eps_is_taken_from_each_module(golden):
    """Eleven different eps, none the default (0.05, 0.10, ... in module order: against running variances of order 1 each moves its
    scale by percents).  Forward against torch eager (1e-5, the bound of the two tests above), the reverse pass against its float64
    restatement on the taped branches with the bound of that test -- both read m.eps.  Then one eps changed on a net whose pack exists:
    eps is a Python float, no tensor version tells of it, and the pack still follows."""
    net, plain = _net(golden), _net(golden)
    bns = [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert len(bns) == 11 and all(m.eps == 1e-5 for m in bns)
    for k, m in enumerate(bns):
        m.eps = 0.05 * (k + 1)
    i1, i2, cot = _inputs(golden, "1x13x17")
    tape = {}
    with torch.no_grad():
        base = plain(i1, i2)
        out = net.forward_impl(i1, i2, tape=tape)
        d1, d2 = net.backward_impl(cot, tape)
        err = float((out - _eager(net, i1, i2)).abs().max())
        print("eps per module: moved %.3e, err %.3e" % (float((out - base).abs().max()), err))
        assert float((out - base).abs().max()) > 1e-3 and err <= 1e-5
    maps, fused = _cpu_maps(tape["maps"]), tape["out"].cpu()
    r64 = _linearised(_sd(golden), _bn_eps(net), maps, fused, i1.cpu(), i2.cpu(), cot.cpu(), torch.float64)
    r32 = _linearised(_sd(golden), _bn_eps(net), maps, fused, i1.cpu(), i2.cpu(), cot.cpu(), torch.float32)
    for name, mine, a64, a32 in (("d_i1", d1, r64[0], r32[0]), ("d_i2", d2, r64[1], r32[1])):
        check("eps reverse", "1x13x17", name, mine, a64, floor(a32, a64))
    with torch.no_grad():
        bns[4].eps = 2.0
        second = net(i1, i2)
        err = float((second - _eager(net, i1, i2)).abs().max())
        print("one eps changed: moved %.3e, err %.3e" % (float((second - out).abs().max()), err))
        assert float((second - out).abs().max()) > 1e-3 and err <= 1e-5


# ---- inside the composite model ------------------------------------------------------------------------------------------------
def _in_composite(golden):
    """The network with the fixture's weights as the fusion module of Network_MM_CompModel."""
    from paif_amd.fusion_model.didfuse import DID

    return C.composite(DID(), _sd(golden))


def test_composite_clean_forward(golden):
    """fused within 1e-4, logits within 2e-4 x scale, argmax agreement 99.9 %: the tolerances of
    tests/test_seg_gpu.py::test_full_model_config1_4x64x96."""
    g = golden("gd_didfuse_attack")
    C.composite_clean_forward(_in_composite(golden), g, start=int(g["start"]), fused_atol=1e-4, logits_rtol=2e-4, agreement=0.999)


def test_attack_both_pgd_through_the_baseline(golden, exact_arithmetic):
    """Limits: losses rtol 1e-4, sign and delta mismatch <= 2e-3, against the reference's float32 trace.

    The batch is the first on which that trace is stable under a perturbation of the fused plane and takes exactly the steps of the
    reference's float64 trace (tools/make_golden_didfuse.py, THE ATTACK BATCH; chosen on the reference alone), so the whole of the limit
    is the implementation's.  On one MI355X: losses within 2.0e-7, one infrared element of 12,288 different in sign and delta (8.1e-5),
    none of the visible ones."""
    g = golden("gd_didfuse_attack")
    C.attack_both_pgd(_in_composite(golden), g, start=int(g["start"]), eps=EPS, alpha=ALPHA, loss_rtol=1e-4, frac=2e-3)


def test_pgd_iterations_replayed_from_a_graph_are_bit_identical(golden):
    """Three PGD iterations captured once with torch.cuda.graph and replayed = the eager loop.  Single stream, no parallel branches; every
    weight pack is built (and the six slopes are read to the host) before the capture."""
    g = golden("gd_didfuse_attack")
    C.pgd_iterations_replayed_from_a_graph_are_bit_identical(_in_composite(golden), start=int(g["start"]),
                                                             delta0=lambda ir, vis: (t(g["d0_ir"]), t(g["d0_vis"])), eps=EPS, alpha=ALPHA)


def test_robustness_harnesses_run_with_the_baseline(golden):
    """val_segformer_robust2 (clean) and val_segformer_robust (PGD, 2 iterations) on two 2x64x96 batches: finite mIoU, and the clean one is
    what the confusion matrix of the model's own seg_map argmax gives."""
    C.robustness_harnesses_run(_in_composite(golden), miou_atol=1e-12, attack_iters=2)
