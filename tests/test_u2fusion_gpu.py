"""GPU: the U2Fusion baseline (paif_amd/fusion_model/u2fusion.py, csrc/u2fusion.hip) against the reference's own outputs and autograd
(tests/golden/gu_u2fusion*.npz, generated on the CPU by tools/make_golden_u2fusion.py), and inside the composite model / attack / harness
flow of the searched network.

Bound of the kernel parity checks (tests/baseline_common.py: bound): with floor = max|ref32 - ref64| of the same tensor,
max|hip - ref64| <= 1.5 * floor + 1e-5 * max(1, max|ref64|).  One kernel form exists (exact fp32, the wide convs on
v_mfma_f32_16x16x4_f32); it is the default build.

The reference's autograd is the yardstick of the input gradients only where no pre-activation is within fp32 reach of zero (the five
small cases, see the tool).  At 1x37x53 and 2x24x32 the reverse pass is tested as what it is given its tape -- a linear map -- against a
float64 restatement that takes its LeakyReLU branches and tanh' from the tape itself."""
import pytest
import torch
import torch.nn.functional as F

from paif_amd import ops, synthetic as S
from tests import baseline_common as C
from tests.baseline_common import check, dev, exact_arithmetic, floor  # noqa: F401  (exact_arithmetic is a fixture)
from tests.helpers import t

pytestmark = pytest.mark.gpu

GRAD_CASES = ("1x4x5", "1x13x17", "2x9x20", "1x11x37", "1x19x35")
LARGE = ("1x37x53", "2x24x32")
SMALL = ("1x4x5", "1x13x17")
HALO = 10           # the ten 3 x 3 convs
EPS, ALPHA = 8 / 255., 2 / 255.
_SD = {}


def _sd(golden):
    """The fixture weights, rebuilt once from the ten scales and the shift."""
    if not _SD:
        g = golden("gu_u2fusion")
        _SD.update({k: torch.from_numpy(v) for k, v in S.u2fusion_state_dict(g["scales"], g["shift"]).items()})
    return _SD


def _net(golden):
    from paif_amd.fusion_model.u2fusion import U2Fusion

    net = U2Fusion().eval()
    net.load_state_dict(_sd(golden), strict=True)
    return net.requires_grad_(False).to(dev())


def _inputs(golden, case):
    g = golden("gu_u2fusion_" + case)
    cot = g["cot"] if "cot" in g else S.make_feature(900 + len(case), g["i1"].shape)
    return t(g["i1"]).to(dev()), t(g["i2"]).to(dev()), t(cot).to(dev())


@pytest.mark.parametrize("case", GRAD_CASES + LARGE)
def test_fused_plane_matches_the_reference(golden, case):
    """1x4x5 is smaller than the total halo of 10 (all border), 1x13x17 is ragged in both directions with two tiles across, 2x9x20 has two
    images, 1x11x37 three tiles across with the last 5 pixels wide, 1x19x35 and 1x37x53 several tile rows and columns, ragged in both."""
    g = golden("gu_u2fusion_" + case)
    net = _net(golden)
    i1, i2, _ = _inputs(golden, case)
    with torch.no_grad():
        out = net(i1, i2)
    assert out.grad_fn is None and out.shape == i1.shape
    check("fused", case, "fused", out, g["fused64"], floor(g["fused"], g["fused64"]), halo=HALO if case in LARGE else None)


@pytest.mark.parametrize("case", SMALL)
def test_feature_maps_match_the_reference(golden, case):
    """The nine LeakyReLU maps (conv_1, the five dense layers, sub.0 .. sub.2), each against its own floor."""
    g = golden("gu_u2fusion_" + case)
    net = _net(golden)
    i1, i2, _ = _inputs(golden, case)
    maps = net._features(i1, i2)
    assert [m.shape[1] for m in maps] == [44] * 6 + [128, 64, 32]
    for k, m in enumerate(maps):
        check("maps", case, "map%d" % k, m, g["map%d" % k], float(g["map_floor"][k]))


@pytest.mark.parametrize("case", GRAD_CASES)
def test_input_gradients_match_float64_autograd(golden, case):
    """d_i1, d_i2 for the fixture's cotangent on the fused plane, through forward + .backward()."""
    g = golden("gu_u2fusion_" + case)
    net = _net(golden)
    i1, i2, cot = _inputs(golden, case)
    a, b = i1.clone().requires_grad_(True), i2.clone().requires_grad_(True)
    out = net(a, b)
    assert out.grad_fn is not None
    (out * cot).sum().backward()
    for name, mine in (("d_i1", a.grad), ("d_i2", b.grad)):
        check("grad", case, name, mine, g[name + "64"], floor(g[name], g[name + "64"]))


def _linearised(sd, masks, dtanh, i1, i2, cot, dtype):
    """The network with every LeakyReLU replaced by the constant mask of its taped map and the tanh by its taped derivative, biases
    dropped: what the reverse pass transposes.  -> (d_i1, d_i2) for the cotangent, by torch's CPU autograd in `dtype`."""
    w = [sd[name + ".weight"].to(dtype) for name, _, _ in S.U2FUSION_CONVS]
    m = [x.to(dtype) for x in masks]
    a, b = i1.to(dtype).clone().requires_grad_(True), i2.to(dtype).clone().requires_grad_(True)
    x = F.conv2d(torch.cat((a, b), 1), w[0], padding=1) * m[0]
    for i in range(1, 6):
        x = torch.cat((x, F.conv2d(x, w[i], padding=1) * m[i]), 1)
    for i in range(6, 9):
        x = F.conv2d(x, w[i], padding=1) * m[i]
    y = F.conv2d(x, w[9], padding=1) * dtanh.to(dtype)
    (y * cot.to(dtype)).sum().backward()
    return a.grad.numpy(), b.grad.numpy()


@pytest.mark.parametrize("case", LARGE)
def test_reverse_pass_matches_its_float64_restatement_on_the_taped_branches(golden, case):
    """Sizes the margin condition cannot reach.  A sign the GPU forward decided differently from the reference cannot enter: the branches
    are the tape's.  A wrong tap, slice offset or mask shows at order 0.1.  The floor is the same restatement in float32."""
    net = _net(golden)
    i1, i2, cot = _inputs(golden, case)
    tape = {}
    with torch.no_grad():
        net.forward_impl(i1, i2, tape=tape)
        d1, d2 = net.backward_impl(cot, tape)
    cat = tape["cat"].cpu()
    maps = [cat[..., 44 * k:44 * (k + 1)] for k in range(6)] + [tape[k].cpu() for k in ("s1", "s2", "s3")]
    masks = [torch.where(m > 0, 1.0, 0.2).permute(0, 3, 1, 2).contiguous() for m in maps]
    out = tape["out"].cpu().double()
    dtanh = 1 - out * out
    r64 = _linearised(_sd(golden), masks, dtanh, i1.cpu(), i2.cpu(), cot.cpu(), torch.float64)
    r32 = _linearised(_sd(golden), masks, dtanh, i1.cpu(), i2.cpu(), cot.cpu(), torch.float32)
    for name, mine, a64, a32 in (("d_i1", d1, r64[0], r32[0]), ("d_i2", d2, r64[1], r32[1])):
        check("taped-mask reverse", case, name, mine, a64, floor(a32, a64), halo=HALO)


def _flat(tape):
    return [tape[k] for k in ("cat", "s1", "s2", "s3", "out")]


def test_reverse_pass_is_linear_in_the_cotangent(golden):
    """backward_impl(g1) + backward_impl(g2) = backward_impl(g1 + g2) to fp32 rounding: within 1e-4 of the largest gradient
    (tests/baseline_common.py says why)."""
    C.reverse_pass_is_linear_in_the_cotangent(_net(golden), *_inputs(golden, "1x19x35"), rtol=1e-4)


def test_two_runs_are_bit_identical(golden):
    C.two_runs_are_bit_identical(_net(golden), *_inputs(golden, "2x24x32"), taped=_flat)


def test_channel_slices_are_taken_without_a_copy(golden):
    """The composite hands over ir[:, 0:1] and ycc of multi-channel tensors: planes addressed through their batch stride."""
    C.channel_slices_are_taken_without_a_copy(_net(golden), *_inputs(golden, "2x24x32"))


def test_settings_that_do_not_apply_change_nothing(golden):
    """One arithmetic: the storage mode, the conv / GEMM precision and two_stream leave every bit where it is."""
    C.settings_that_do_not_apply_change_nothing(_net(golden), *_inputs(golden, "1x13x17"), fp32_maps=_flat)


@pytest.mark.parametrize("shape", ((1, 13, 17), (2, 9, 20)))
@pytest.mark.parametrize("layer", (7, 8))
def test_sub_convs_equal_the_generic_slab_conv_bit_for_bit(golden, layer, shape):
    """sub.1 (128 -> 64, four blocks per workgroup) and sub.2 (64 -> 32, two) are the two layers whose channel counts the generic entry
    point onto csrc/conv_slab.h (paif_bffusion_conv) accepts: paif_u2fusion_conv_fwd / _bwd and that entry point run one kernel on one
    operand order, so the same weights give the same bits, forward and transposed.  The generic transpose has the add form only: it
    adds onto a zeroed map.  1x13x17: two tiles across, ragged both ways; 2x9x20: two images."""
    B, H, W = shape
    L, dev = ops.lib(), C.dev()
    sd = _sd(golden)
    convs = [(sd[n + ".weight"].to(dev), sd[n + ".bias"].to(dev)) for n, _, _ in S.U2FUSION_CONVS]
    pack = ops.u2fusion_pack(convs)
    w, b = convs[layer]
    cout, cin = w.shape[:2]
    cv = ops._BffConv([(w, 0)], cout, cin, 9, b, 0.2, 0)
    x = t(S.make_feature(310 + layer, (B, H, W, cin))).to(dev)
    taped = t(S.make_feature(320 + layer, (B, H, W, cout))).to(dev)
    d_out = t(S.make_feature(330 + layer, (B, H, W, cout))).to(dev)
    assert float(taped.min()) < 0 < float(taped.max()) and float(x.min()) < 0 < float(x.max())
    mine, other = torch.empty_like(taped), torch.empty_like(taped)
    ops._lib.check(L.paif_u2fusion_conv_fwd(ops._p(pack), layer, ops._p(x), ops._p(mine), B, H, W, ops._stream()), "u2fusion_conv_fwd")
    ops._bff_conv(cv, x, 0, other, 0, B, H, W)
    assert float(mine.min()) < 0 < float(mine.max())
    assert torch.equal(mine, other)
    d_mine, d_other = torch.empty_like(x), torch.zeros_like(x)
    ops._lib.check(L.paif_u2fusion_conv_bwd(ops._p(pack), layer, ops._p(taped), ops._p(d_out), ops._p(d_mine), B, H, W, ops._stream()),
                   "u2fusion_conv_bwd")
    ops._bff_conv_t(cv, taped, d_out, 0, d_other, 0, None, True, 0, B, H, W)
    assert float(d_mine.abs().max()) > 0
    assert torch.equal(d_mine, d_other)


def test_wrong_planes_are_refused_on_the_device(golden):
    net = _net(golden)
    z = torch.zeros(1, 1, 8, 8, device=dev())
    with pytest.raises(TypeError, match="fp32"):
        net(z.half(), z.half())
    with pytest.raises(ValueError, match=r"\[B,1,H,W\]"):
        net(z, torch.zeros(1, 1, 8, 9, device=dev()))
    with pytest.raises(ValueError, match=r"\[B,1,H,W\]"):
        net(torch.zeros(1, 3, 8, 8, device=dev()), torch.zeros(1, 3, 8, 8, device=dev()))
    trainable = _net(golden).requires_grad_(True)
    with pytest.raises(NotImplementedError, match="[Pp]arameter gradients"):
        trainable(z, z)
    with ops.no_param_grads():                                  # an attack's forward: input gradients only
        a = z.clone().requires_grad_(True)
        out = trainable(a, z)
        out.sum().backward()
    assert a.grad is not None and all(p.grad is None for p in trainable.parameters())


# ---- inside the composite model ------------------------------------------------------------------------------------------------
def _in_composite(golden):
    """The network with the fixture's weights as the fusion module of Network_MM_CompModel."""
    from paif_amd.fusion_model.u2fusion import U2Fusion

    return C.composite(U2Fusion(), _sd(golden))


def test_composite_clean_forward(golden):
    """fused within 1e-4, logits within 2e-4 x scale, argmax agreement 99.9 %: the tolerances of
    tests/test_seg_gpu.py::test_full_model_config1_4x64x96."""
    g = golden("gu_u2fusion_attack")
    C.composite_clean_forward(_in_composite(golden), g, start=int(g["start"]), fused_atol=1e-4, logits_rtol=2e-4, agreement=0.999)


def test_attack_both_pgd_through_the_baseline(golden, exact_arithmetic):
    """Losses rtol 1e-4, sign and delta mismatch <= 2e-3, against the reference's float32 trace."""
    g = golden("gu_u2fusion_attack")
    C.attack_both_pgd(_in_composite(golden), g, start=int(g["start"]), eps=EPS, alpha=ALPHA, loss_rtol=1e-4, frac=2e-3)


def test_pgd_iterations_replayed_from_a_graph_are_bit_identical(golden):
    """Three PGD iterations captured once with torch.cuda.graph and replayed = the eager loop.  Single stream, no parallel branches; every
    weight pack is built before the capture."""
    g = golden("gu_u2fusion_attack")
    C.pgd_iterations_replayed_from_a_graph_are_bit_identical(_in_composite(golden), start=int(g["start"]),
                                                             delta0=lambda ir, vis: (t(g["d0_ir"]), t(g["d0_vis"])), eps=EPS, alpha=ALPHA)


def test_robustness_harnesses_run_with_the_baseline(golden):
    """val_segformer_robust2 (clean) and val_segformer_robust (PGD, 2 iterations) on two 2x64x96 batches: finite mIoU, and the clean one is
    what the confusion matrix of the model's own seg_map argmax gives."""
    C.robustness_harnesses_run(_in_composite(golden), miou_atol=1e-12, attack_iters=2)
