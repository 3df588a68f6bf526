"""GPU: the BFFusion baseline (paif_amd/fusion_model/bffusion.py, csrc/bffusion.hip, csrc/conv_slab.h) against the reference's own outputs
and autograd (tests/golden/gb_bffusion*.npz, generated on the CPU by tools/make_golden_bffusion.py, the reference in .eval() mode), and
inside the composite model / attack / harness flow of the searched network.

Bound of the kernel parity checks (tests/test_didfuse_gpu.py): with floor = max|ref32 - ref64| of the same tensor,
max|hip - ref64| <= 1.5 * floor + 1e-5 * max(1, max|ref64|).  One kernel form exists (exact fp32, the convs on v_mfma_f32_16x16x4_f32,
BatchNorm folded into the weights, the context reduction accumulated in float64); it is the default build.

In the fixtures i1 is the infrared plane and enters image_vis_y (the `_vi` modules and attn2), i2 is the visible Y plane and enters
image_ir: the order inside the composite model.

Cases: 1x16x16 is the smallest input (level 4 is 2 x 2: every reflected read and every fold lands on a border row, no fringe); 1x17x23 has
two ragged tiles each way at level 1, a pool that drops a row at level 1 and a column at levels 1-3, every upsample pads a column and the
top one a row; 1x22x16 is odd at levels 2 and 3 only; 2x16x20 has two images (per-image context matrices, batch strides); 1x40x56 and
2x35x50 have several tile rows and columns at level 1, more than one at level 2, and three chunks of the context reduction.

The reference's autograd is the yardstick of the input gradients only where no sign point (62 activation inputs, every pooling window's
gap between its two largest entries) is within fp32 reach of its switch (the gradient cases, see the tool).  At the large cases the
reverse pass is tested against a float64 restatement (tests/bffusion_eager.py) that takes every LeakyReLU / ReLU branch and every pool
choice from the tape and nothing else: softmax, LayerNorm, tanh and the gate are torch's own.  No pixel is excluded."""
import numpy as np
import pytest
import torch

from paif_amd import ops, synthetic as S
from tests import helpers as Hh
from tests.bffusion_eager import eager, taped_maps
from tests.helpers import t, maxabs

pytestmark = pytest.mark.gpu

GRAD_CASES = ("1x16x16", "1x17x23", "1x22x16")
TWO_IMAGES = "2x16x20"
LARGE = ("1x40x56", "2x35x50")
RESTATED = (TWO_IMAGES,) + LARGE
SMALL = ("1x16x16", "1x17x23")
HALO = 8            # full-resolution pixels the border check covers: one level-4 pixel
EPS, ALPHA = 8 / 255., 2 / 255.
_SD = {}


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _sd(golden):
    """The fixture weights, rebuilt once from the 97 scales and shifts."""
    if not _SD:
        g = golden("gb_bffusion")
        _SD.update({k: torch.from_numpy(np.asarray(v)) for k, v in S.bffusion_state_dict(g["scales"], g["shift"]).items()})
    return _SD


def _net(golden):
    from paif_amd.fusion_model.bffusion import BFFR

    net = BFFR().eval()
    net.load_state_dict(_sd(golden), strict=True)
    return net.requires_grad_(False).to(_dev())


def _inputs(golden, case):
    g = golden("gb_bffusion_" + case)
    cot = g["cot"] if "cot" in g else S.make_feature(900 + len(case), g["i1"].shape)
    return t(g["i1"]).to(_dev()), t(g["i2"]).to(_dev()), t(cot).to(_dev())


def _bound(floor, ref64):
    return 1.5 * floor + 1e-5 * max(1.0, float(np.abs(ref64).max()))


def _floor(ref32, ref64):
    return float(np.abs(ref32.astype(np.float64) - ref64).max())


def _border(a):
    m = np.ones(a.shape[-2:], dtype=bool)
    m[HALO:-HALO, HALO:-HALO] = False
    return a[..., m]


def _check(what, case, name, mine, ref64, floor, border=False):
    got = mine.detach().cpu().numpy().astype(np.float64)
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    bound = _bound(floor, ref64)
    err = float(np.abs(got - ref64).max())
    print("%s %s %s: err %.3e bound %.3e ratio %.3f scale %.3e" % (what, case, name, err, bound, err / bound, float(np.abs(ref64).max())))
    assert err <= bound, (name, err, bound)
    if border:
        eb = float(np.abs(_border(got) - _border(ref64)).max())
        print("%s %s %s border: err %.3e bound %.3e ratio %.3f" % (what, case, name, eb, bound, eb / bound))
        assert eb <= bound, (name, "border", eb, bound)


@pytest.mark.parametrize("case", GRAD_CASES + RESTATED)
def test_fused_plane_matches_the_reference(golden, case):
    g = golden("gb_bffusion_" + case)
    net = _net(golden)
    i1, i2, _ = _inputs(golden, case)
    with torch.no_grad():
        out = net(i1, i2)
    assert out.grad_fn is None and out.shape == i1.shape
    _check("fused", case, "fused", out, g["fused64"], _floor(g["fused"], g["fused64"]), border=case in LARGE)


@pytest.mark.parametrize("case", SMALL)
def test_feature_maps_match_the_reference(golden, case):
    """The 98 taped maps (BFFR._map_list), each against its own floor."""
    parts = [golden("gb_bffusion_%s_maps%d" % (case, p)) for p in range(int(golden("gb_bffusion")["maps_" + case]))]
    ref = {k: v for p in parts for k, v in p.items()}
    net = _net(golden)
    i1, i2, _ = _inputs(golden, case)
    maps = net._features(i1, i2)
    assert len(maps) == 98
    for k, m in enumerate(maps):
        _check("maps", case, "map%d" % k, m, ref["map%d" % k], float(ref["map_floor"][k]))


def _gradient_parity(golden, case):
    g = golden("gb_bffusion_" + case)
    net = _net(golden)
    i1, i2, cot = _inputs(golden, case)
    a, b = i1.clone().requires_grad_(True), i2.clone().requires_grad_(True)
    out = net(a, b)
    assert out.grad_fn is not None
    (out * cot).sum().backward()
    for name, mine in (("d_i1", a.grad), ("d_i2", b.grad)):
        assert float(np.abs(g[name + "64"]).max()) > 1e-4
        _check("grad", case, name, mine, g[name + "64"], _floor(g[name], g[name + "64"]))


@pytest.mark.parametrize("case", GRAD_CASES)
def test_input_gradients_match_float64_autograd(golden, case):
    """d_i1, d_i2 for the fixture's cotangent on the fused plane, through forward + .backward()."""
    _gradient_parity(golden, case)


def test_input_gradients_of_two_images_match_float64_autograd(golden):
    """2x16x20 where the tool found a start that meets the margin condition (the fixture says which)."""
    assert bool(golden("gb_bffusion")["case_" + TWO_IMAGES][7]) == ("d_i164" in golden("gb_bffusion_" + TWO_IMAGES))
    if "d_i164" in golden("gb_bffusion_" + TWO_IMAGES):
        _gradient_parity(golden, TWO_IMAGES)


def _restated(net, taped, i1, i2, cot, dtype):
    a, b = i1.to(dtype).clone().requires_grad_(True), i2.to(dtype).clone().requires_grad_(True)
    out = eager(net, a, b, taped=taped, dtype=dtype)
    (out * cot.to(dtype)).sum().backward()
    return out.detach(), a.grad.cpu().numpy(), b.grad.cpu().numpy()


@pytest.mark.parametrize("case", RESTATED)
def test_reverse_pass_matches_its_float64_restatement_on_the_taped_branches(golden, case):
    """Sizes the margin condition cannot reach.  Only what is discontinuous is frozen from the tape; the floor is the same restatement in
    float32.  A wrong tap, slice offset, fold, pool choice, per-image index or a missing 0.5 shows at order 0.1.  The restatement runs
    through torch's own float64 ops and autograd on the device the maps are on."""
    net = _net(golden)
    i1, i2, cot = _inputs(golden, case)
    tape = {}
    with torch.no_grad():
        net.forward_impl(i1, i2, tape=tape)
        d1, d2 = net.backward_impl(cot, tape)
    taped = taped_maps(tape["maps"], _dev())
    f64, a64, b64 = _restated(net, taped, i1, i2, cot, torch.float64)
    _, a32, b32 = _restated(net, taped, i1, i2, cot, torch.float32)
    assert float((f64 - tape["out"].double()).abs().max()) <= 1e-5      # the frozen forward is the taped one
    for name, mine, r64, r32 in (("d_i1", d1, a64, a32), ("d_i2", d2, b64, b32)):
        assert float(np.abs(r64).max()) > 1e-4
        _check("taped-branch reverse", case, name, mine, r64, _floor(r32, r64), border=case in LARGE)


def _flat(tape):
    m = tape["maps"]
    out = [tape["out"]] + [x for s in range(2) for x in m["E"][s] + m["EN"][s]] + m["D"]
    return out + [a[k] for row in m["A"] for a in row for k in ("p1", "p2", "qkv", "ctx", "y", "z", "f1", "f2")]


def test_reverse_pass_is_linear_in_the_cotangent(golden):
    net = _net(golden)
    i1, i2, cot = _inputs(golden, "1x22x16")
    tape = {}
    with torch.no_grad():
        net.forward_impl(i1, i2, tape=tape)
        g2 = t(S.make_feature(77, tuple(cot.shape))).to(_dev())
        r1, r2, r12 = net.backward_impl(cot, tape), net.backward_impl(g2, tape), net.backward_impl(ops.add(cot, g2), tape)
    for x, y, z in zip(r1, r2, r12):
        scale = max(1.0, float(z.abs().max()))
        err = float((x + y - z).abs().max())
        print("linearity: err %.3e scale %.3e" % (err, scale))
        assert float(z.abs().max()) > 0
        assert err <= 1e-4 * scale


def test_two_runs_are_bit_identical(golden):
    """The whole tape and both gradients, at a size with three chunks of the context reduction."""
    net = _net(golden)
    i1, i2, cot = _inputs(golden, "2x35x50")
    runs = []
    with torch.no_grad():
        for _ in range(2):
            tape = {}
            f = net.forward_impl(i1, i2, tape=tape)
            runs.append([f] + _flat(tape) + list(net.backward_impl(cot, tape)))
    assert len(runs[0]) == 1 + (1 + 16 + 4 + 64) + 2
    for x, y in zip(*runs):
        assert torch.equal(x, y)


def test_channel_slices_are_taken_without_a_copy(golden):
    net = _net(golden)
    i1, i2, cot = _inputs(golden, TWO_IMAGES)
    wide1 = torch.cat([i1, i1 * 0.5, i1 * 0.25], 1).contiguous()
    wide2 = torch.cat([i2, i2 * 0.5], 1).contiguous()
    with torch.no_grad():
        ta, tb = {}, {}
        fa = net.forward_impl(i1, i2, tape=ta)
        fb = net.forward_impl(wide1, wide2, tape=tb)
        assert torch.equal(fa, fb)
        assert torch.equal(fa, net(wide1[:, 0:1], wide2[:, 0:1]))
        for x, y in zip(net.backward_impl(cot, ta), net.backward_impl(cot, tb)):
            assert torch.equal(x, y)


def test_settings_that_do_not_apply_change_nothing(golden):
    net = _net(golden)
    i1, i2, cot = _inputs(golden, "1x17x23")
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


def test_wrong_planes_and_modes_are_refused_on_the_device(golden):
    net = _net(golden)
    z = torch.zeros(1, 1, 16, 16, device=_dev())
    with pytest.raises(TypeError, match="fp32"):
        net(z.half(), z.half())
    with pytest.raises(ValueError, match=r"\[B,1,H,W\]"):
        net(z, torch.zeros(1, 1, 16, 17, device=_dev()))
    with pytest.raises(ValueError, match=r"\[B,1,H,W\]"):
        net(torch.zeros(1, 3, 16, 16, device=_dev()), torch.zeros(1, 3, 16, 16, device=_dev()))
    for shape in ((1, 1, 15, 16), (1, 1, 16, 15)):
        with pytest.raises(ValueError, match="16"):
            net(torch.zeros(shape, device=_dev()), torch.zeros(shape, device=_dev()))
    trainable = _net(golden).requires_grad_(True)
    with pytest.raises(NotImplementedError, match="[Pp]arameter gradients"):
        trainable(z, z)
    with ops.no_param_grads():                                  # an attack's forward: input gradients only
        a = z.clone().requires_grad_(True)
        out = trainable(a, z)
        out.sum().backward()
    assert a.grad is not None and all(p.grad is None for p in trainable.parameters())
    before = {k: v.clone() for k, v in net.state_dict().items()}
    net.train()
    with pytest.raises(NotImplementedError, match="BatchNorm"):
        with torch.no_grad():
            net(z, z)
    with pytest.raises(NotImplementedError, match="BatchNorm"):
        net.forward_impl(z, z, tape={})
    for k, v in net.state_dict().items():
        assert torch.equal(v, before[k]), k


def test_reference_initialisation_matches_torch_eager(golden):
    """A net as the constructor leaves it: torch's default conv and linear initialisation, identity BatchNorm and LayerNorm."""
    from paif_amd.fusion_model.bffusion import BFFR

    torch.manual_seed(20)
    net = BFFR().eval().requires_grad_(False).to(_dev())
    i1, i2, _ = _inputs(golden, "1x17x23")
    with torch.no_grad():
        mine, ref = net(i1, i2), eager(net, i1, i2)
    err = float((mine - ref).abs().max())
    print("reference initialisation: err %.3e (fused in [%.3f, %.3f])" % (err, float(ref.min()), float(ref.max())))
    assert float(ref.max() - ref.min()) > 1e-3
    assert err <= 1e-5


def test_in_place_changes_and_eps_rebuild_the_pack(golden):
    """The pack's key holds the used BatchNorm buffers and the LayerNorm affine, and the eps floats are compared per call: a change of a
    used running_var, a LayerNorm weight, a BatchNorm eps and the LayerNorm eps each changes the output, and it is torch eager's again
    (1e-5, the bound of the test above).  A change of a ConvLayer.bn buffer -- never applied -- changes no bit."""
    net = _net(golden)
    i1, i2, _ = _inputs(golden, "1x17x23")
    at = net.fusion_block1.attn2
    steps = (("running_var", lambda: at.conv_pre[1].batch_norm.running_var[::2].mul_(4.0)),
             ("LayerNorm weight", lambda: net.fusion_block2.attn1.norm1.weight[::2].mul_(-1.5)),
             ("BatchNorm eps", lambda: setattr(net.fusion_block1.attn1.ffn[0].batch_norm, "eps", 1.0)),
             ("LayerNorm eps", lambda: setattr(net.fusion_block3.attn2.norm1, "eps", 2.0)))
    with torch.no_grad():
        last = net(i1, i2)
        assert float((last - eager(net, i1, i2)).abs().max()) <= 1e-5
        for what, change in steps:
            change()
            out = net(i1, i2)
            err, moved = float((out - eager(net, i1, i2)).abs().max()), float((out - last).abs().max())
            print("%s changed: moved %.3e, err %.3e" % (what, moved, err))
            assert moved > 1e-4 and err <= 1e-5, what
            last = out
        net.DB1_2.bn.running_var.mul_(9.0), net.conv1_ir.bn.weight.fill_(7.0), net.DB3_1.bn.running_mean.add_(1.0)
        net.DB2_2.bn.eps = 3.0
        assert torch.equal(net(i1, i2), last)


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
    from paif_amd.core.model_fusion_auto import Network_MM_CompModel
    from paif_amd.fusion_model.bffusion import BFFR

    m = Network_MM_CompModel(BFFR(), None, None, "mit_b0", num_classes=9).eval()
    S.load_formula_weights(m, head=Hh.HEAD64["mit_b0"])
    m.enhance_net.load_state_dict(_sd(golden), strict=True)
    return m.to(_dev())


def _batch(start=0):
    ir, vis, lab = S.make_batch(2, 64, 96, start=start)
    return t(ir).to(_dev()), t(vis).to(_dev()), t(lab).to(_dev())


def _scale(a):
    return max(1.0, float(np.abs(a).max()))


def test_composite_clean_forward(golden):
    """Tolerances of tests/test_didfuse_gpu.py::test_composite_clean_forward: fused 1e-4, logits 2e-4 x scale, argmax agreement 99.9 %."""
    g = golden("gb_bffusion_attack")
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
    """tests/test_attack_gpu.py:_check_attack, with every figure printed before the first assertion."""
    losses = np.array([s["loss"] for s in trace])
    print("attack: largest relative loss difference %.2e" % float(np.abs(losses / g["losses"] - 1).max()))
    signs = [(np.sign(mine.cpu().numpy()) != np.sign(ref)).mean() for mine, ref in ((trace[-1]["g_ir"], g["gsum_ir"]),
                                                                                     (trace[-1]["g_vis"], g["gsum_vis"]))]
    deltas = [mine.detach().cpu().numpy() for mine in (d_ir, d_vis)]
    diffs = [(np.abs(a - ref) > 1e-6).mean() for a, ref in zip(deltas, (g["delta_ir"], g["delta_vis"]))]
    print("attack: sign mismatch of the running sums %.2e %.2e" % tuple(signs))
    print("attack: share of differing delta elements %.2e %.2e" % tuple(diffs))
    np.testing.assert_allclose(losses, g["losses"], rtol=loss_rtol)
    for mism in signs:
        assert mism <= frac
    for a, diff in zip(deltas, diffs):
        assert diff <= frac
        assert np.abs(a).max() <= 8 / 255. + 1e-7


def test_attack_both_pgd_through_the_baseline(golden, exact_arithmetic):
    """Limits of tests/test_didfuse_gpu.py: losses rtol 1e-4, sign and delta mismatch <= 2e-3, against the reference's float32 trace on
    the batch the tool chose on the reference alone (tools/make_golden_didfuse.py, THE ATTACK BATCH)."""
    from paif_amd.attack.attack import attack_both

    g = golden("gb_bffusion_attack")
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
    weight pack is built before the capture."""
    m = _composite(golden)
    ir, vis, lab = _batch(0)
    lab64 = lab.type(torch.long).contiguous()
    d0_ir, d0_vis = (t(S.make_delta0(k, tuple(x.shape), EPS)).to(_dev()) for k, x in enumerate((ir, vis)))
    state = [torch.zeros_like(x) for x in (ir, vis, ir, vis)]

    def reset():
        state[0].copy_(d0_ir), state[1].copy_(d0_vis), state[2].zero_(), state[3].zero_()

    gstream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), ops.attack_arithmetic():
        gs = ops.attack_grad_scale(lab64)
        reset()
        _pgd_iterations(m, ir, vis, lab64, *state, gs, 3)     # eager: also builds every weight pack outside the capture
        first = [x.clone() for x in state]
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
    assert float(first[2].abs().max()) > 0
    for x, y in zip(first, state):
        assert torch.equal(x, y)


def test_robustness_harnesses_run_with_the_baseline(golden):
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
