"""What the GPU tests of the native fusion networks (tests/test_{reconet,sdnet,u2fusion,seafusion,didfuse,bffusion,drdb}_gpu.py) share:
the parity check against a float64 reference, and one body per test of the protocol every network implements
(paif_amd/fusion_model/_native.py) -- alone and inside the composite model / attack / harness flow of the searched network.

Every function takes the network's particulars -- the net or the composite model, its inputs, the halo, the tape's tensors, the start
batch and delta0, every tolerance -- as arguments: the limits of a network stand in its own test file."""
import numpy as np
import pytest
import torch

from paif_amd import ops, synthetic as S
from tests import helpers as Hh
from tests.helpers import t, maxabs


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ---- parity against a float64 reference ------------------------------------------------------------------------------------------
def floor(ref32, ref64):
    """max|ref32 - ref64|: what the reference itself loses in float32."""
    return float(np.abs(np.asarray(ref32).astype(np.float64) - ref64).max())


def bound(floor, ref64):
    """1.5 * floor + 1e-5 * max(1, max|ref64|) (the form of tests/test_training_gpu.py's stage-gradient bound): the scale term allows
    fp32 reordering of sums whose terms are of the size of the result, a wrong tap or a dropped term shows at order 0.1."""
    return 1.5 * floor + 1e-5 * max(1.0, float(np.abs(ref64).max()))


def border(a, halo):
    """The outermost `halo` rows / columns of [..., H, W] (everything, where the plane is smaller than twice the halo)."""
    m = np.ones(a.shape[-2:], dtype=bool)
    m[halo:-halo, halo:-halo] = False
    return a[..., m]


def check(what, case, name, mine, ref64, floor, halo=None, keep=None):
    """max|mine - ref64| <= bound(floor, ref64); with `halo`, the border taken alone against the same bound.  keep (bool array):
    excluded elements take no part, neither in the error nor in the border check."""
    got = mine.detach().cpu().numpy().astype(np.float64)
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    if keep is not None:
        got = np.where(keep, got, ref64)
    lim = bound(floor, ref64)
    err = float(np.abs(got - ref64).max())
    print("%s %s %s: err %.3e bound %.3e ratio %.3f scale %.3e" % (what, case, name, err, lim, err / lim, float(np.abs(ref64).max())))
    assert err <= lim, (name, err, lim)
    if halo is not None:
        eb = float(np.abs(border(got, halo) - border(ref64, halo)).max())
        print("%s %s %s border: err %.3e bound %.3e ratio %.3f" % (what, case, name, eb, lim, eb / lim))
        assert eb <= lim, (name, "border", eb, lim)


# ---- the network alone ------------------------------------------------------------------------------------------------------------
def _both(net, i1, i2, cot):
    """-> ((fused, d_1, d_2), tape) of one forward_impl / backward_impl."""
    tape = {}
    return (net.forward_impl(i1, i2, tape=tape),) + tuple(net.backward_impl(cot, tape)), tape


def reverse_pass_is_linear_in_the_cotangent(net, i1, i2, cot, rtol, label=""):
    """backward_impl(g1) + backward_impl(g2) = backward_impl(g1 + g2) within rtol * max(1, max|gradient|).  Every output is a sum of a few
    thousand fp32 products with cancellation, so the three results differ by accumulated rounding; a dropped or doubled term shows at
    order 1."""
    tape = {}
    with torch.no_grad():
        net.forward_impl(i1, i2, tape=tape)
        g2 = t(S.make_feature(77, tuple(cot.shape))).to(dev())
        r1, r2, r12 = net.backward_impl(cot, tape), net.backward_impl(g2, tape), net.backward_impl(ops.add(cot, g2), tape)
    for x, y, z in zip(r1, r2, r12):
        scale = max(1.0, float(z.abs().max()))
        err = float((x + y - z).abs().max())
        print("linearity%s: err %.3e scale %.3e" % (label, err, scale))
        assert float(z.abs().max()) > 0
        assert err <= rtol * scale


def two_runs_are_bit_identical(net, i1, i2, cot, taped):
    """The fused plane, taped(tape) and both gradients of two runs; -> the list one run gave."""
    runs = []
    with torch.no_grad():
        for _ in range(2):
            out, tape = _both(net, i1, i2, cot)
            runs.append([out[0]] + list(taped(tape)) + list(out[1:]))
    for x, y in zip(*runs):
        assert torch.equal(x, y)
    return runs[0]


def channel_slices_are_taken_without_a_copy(net, i1, i2, cot):
    """The composite hands over ir[:, 0:1] and ycc of multi-channel tensors: planes addressed through their batch stride.
    -> (fused, wide1, wide2) for what a network's own `forward` accepts beyond that."""
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
    return fa, wide1, wide2


def settings_that_do_not_apply_change_nothing(net, i1, i2, cot, fp32_maps):
    """One arithmetic: the storage mode, the conv / GEMM precision and two_stream leave every bit where it is, and fp32_maps(tape) fp32."""
    with torch.no_grad():
        base, _ = _both(net, i1, i2, cot)
    old = dict(ops.CONFIG)
    try:
        for storage, conv, gemm, two in (("bf16", "f32", "f32", True), ("f16", "bf16x3", "bf16x3", False)):
            ops.set_storage(storage), ops.set_conv_precision(conv), ops.set_gemm_precision(gemm)
            ops.CONFIG["two_stream"] = two
            with torch.no_grad():
                got, tape = _both(net, i1, i2, cot)
            assert all(x.dtype == torch.float32 for x in fp32_maps(tape))
            for x, y in zip(base, got):
                assert torch.equal(x, y)
    finally:
        ops.set_storage(old["storage"]), ops.set_conv_precision(old["conv_precision"]), ops.set_gemm_precision(old["gemm_precision"])
        ops.CONFIG["two_stream"] = old["two_stream"]


# ---- inside the composite model ---------------------------------------------------------------------------------------------------
@pytest.fixture
def exact_arithmetic():
    """The setting tests/test_attack_gpu.py asserts gradient parity under: exact-fp32 conv and GEMM kernels."""
    old, oldg = ops.CONFIG["conv_precision"], ops.CONFIG["gemm_precision"]
    ops.set_conv_precision("f32")
    ops.set_gemm_precision("f32")
    yield
    ops.set_conv_precision(old)
    ops.set_gemm_precision(oldg)


def composite(fusion, sd):
    """As tests/test_attack_gpu.py:_model, with `fusion` as the fusion module and `sd` (the fixture's weights) loaded into it."""
    from paif_amd.core.model_fusion_auto import Network_MM_CompModel

    m = Network_MM_CompModel(fusion, None, None, "mit_b0", num_classes=9).eval()
    S.load_formula_weights(m, head=Hh.HEAD64["mit_b0"])
    m.enhance_net.load_state_dict(sd, strict=True)
    return m.to(dev())


def batch(start=0):
    ir, vis, lab = S.make_batch(2, 64, 96, start=start)
    return t(ir).to(dev()), t(vis).to(dev()), t(lab).to(dev())


def scale(a):
    return max(1.0, float(np.abs(a).max()))


def composite_clean_forward(m, g, start, fused_atol, logits_rtol, agreement):
    """fused within fused_atol, logits within logits_rtol x scale, argmax agreement with the reference's prediction."""
    ir, vis, lab = batch(start)
    with torch.no_grad():
        fused, seg = m(ir, vis)
    print("composite: fused err %.3e logits err %.3e (scale %.3e)" % (maxabs(fused.cpu(), g["fused"]), maxabs(seg.cpu(), g["logits"]),
                                                                    scale(g["logits"])))
    up = torch.nn.functional.interpolate(seg.cpu(), size=lab.shape[1:], mode="bilinear", align_corners=False)
    agree = (up.argmax(1).numpy() == g["pred"]).mean()
    print("composite: argmax agreement %.5f" % agree)
    assert maxabs(fused.cpu(), g["fused"]) <= fused_atol
    assert maxabs(seg.cpu(), g["logits"]) <= logits_rtol * scale(g["logits"])
    assert agree >= agreement


def check_attack(g, d_ir, d_vis, trace, loss_rtol, frac, eps):
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
        assert np.abs(a).max() <= eps + 1e-7


def attack_both_pgd(m, g, start, eps, alpha, loss_rtol, frac):
    """Three PGD iterations of attack_both from the fixture's delta0 against the reference's float32 trace (check_attack)."""
    from paif_amd.attack.attack import attack_both

    assert hasattr(m, "forward_taped")                       # the fast path of attack.py is the one taken
    ir, vis, lab = batch(start)
    trace = []
    with torch.no_grad():
        d_ir, d_vis = attack_both(m, vis, ir, lab, epsilon=eps, alpha=alpha, attack_iters=3, attack_loss='l_seg', attack_way='PGD',
                                  delta0_ir=t(g["d0_ir"]), delta0_vis=t(g["d0_vis"]), trace=trace)
    for s in trace:
        assert s["g_ir"].grad_fn is None and s["g_vis"].grad_fn is None and not s["g_ir"].requires_grad
    print("attack: losses %s reference %s" % ([s["loss"] for s in trace], list(g["losses"])))
    check_attack(g, d_ir, d_vis, trace, loss_rtol, frac, eps)


def pgd_iterations(m, ir, vis, lab64, d_ir, d_vis, g_ir, g_vis, gs, iters, eps, alpha):
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
        ops.pgd_step_(d_ir, g_ir, ir, alpha, eps)
        ops.axpy_(g_vis, gv.contiguous(), 1.0 / gs)
        ops.pgd_step_(d_vis, g_vis, vis, alpha, eps)


def pgd_iterations_replayed_from_a_graph_are_bit_identical(m, start, delta0, eps, alpha):
    """Three PGD iterations captured once with torch.cuda.graph and replayed = the eager loop.  Single stream, no parallel branches; the
    eager pass comes first, so every weight pack is built (and whatever it reads to the host is read) before the capture.
    delta0(ir, vis) -> the two start perturbations on the CPU."""
    ir, vis, lab = batch(start)
    lab64 = lab.type(torch.long).contiguous()
    d0_ir, d0_vis = (x.to(dev()) for x in delta0(ir, vis))
    state = [torch.zeros_like(x) for x in (ir, vis, ir, vis)]

    def reset():
        state[0].copy_(d0_ir), state[1].copy_(d0_vis), state[2].zero_(), state[3].zero_()

    gstream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), ops.attack_arithmetic():
        gs = ops.attack_grad_scale(lab64)
        reset()
        pgd_iterations(m, ir, vis, lab64, *state, gs, 3, eps, alpha)     # eager: also builds every weight pack outside the capture
        eager = [x.clone() for x in state]
        torch.cuda.synchronize()
        with torch.cuda.stream(gstream):
            reset()
            pgd_iterations(m, ir, vis, lab64, *state, gs, 3, eps, alpha)
            torch.cuda.synchronize()
            with torch.cuda.graph(graph, stream=gstream):
                pgd_iterations(m, ir, vis, lab64, *state, gs, 3, eps, alpha)
        torch.cuda.synchronize()
        reset()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
    assert float(eager[2].abs().max()) > 0
    for x, y in zip(eager, state):
        assert torch.equal(x, y)


def robustness_harnesses_run(m, miou_atol, attack_iters):
    """val_segformer_robust2 (clean) and val_segformer_robust (PGD) on two 2x64x96 batches: finite mIoU, and the clean one is what the
    confusion matrix of the model's own seg_map argmax gives."""
    from oracle import paif_oracle as O
    from paif_amd.harness import val_segformer_robust, val_segformer_robust2

    batches = []
    for start in (0, 2):
        ir, vis, lab = batch(start)
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
    assert abs(clean["miou"] - float(np.mean(np.nan_to_num(iou)))) <= miou_atol
    rob = val_segformer_robust(m, batches, attack_iters=attack_iters)
    assert np.isfinite(rob["miou"])
