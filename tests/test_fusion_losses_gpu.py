"""GPU: the Sobel fusion criteria and Sobelxy (csrc/sobel_loss.hip, paif_amd/core/loss.py) against the float64 results of the reference
recorded in tests/golden/gl_fusion_losses_*.npz (tools/make_golden_fusion_losses.py).

Inputs are integer multiples of 1/256, so every Sobel sum, max, difference and comparison is exact in float32 in any summation order:
no sign decision can differ between the kernels and the reference and no pixel is left out.  The fixtures hold deliberate ties (half of
`gen` equals the mask, a quadrant equals max(Y, ir)) and a constant block, where sign(0) = 0 decides the gradient.

Bounds (w_i / v_j: the criterion's intensity / gradient weights; planes lie in [0, 2], S <= 8; N = B*H*W):
  value     |d| <= 2^-20 * (sum_i w_i * 2 + 8 * sum_j v_j)         16 ulp per pixel term
  gradient  |d| <= 2^-20 * (sum_i w_i + 8 * sum_j v_j) / N         per element; at most 13 addends of magnitude <= 2 k
Fusionloss_grad3 runs on the SSIM kernels and is held to what Fusionloss_grad2 is: value 2e-5 (tests/test_attack_gpu.py), gradient
2e-5 * max|ref| (tests/test_reverse_kernels_gpu.py).  Every test prints the error it measured before it asserts.

The last case, 2x1x33x65, is one pixel more than the kernels' 32 x 64 tile in both dimensions: ragged tiles, tile seams and the seam
between two images are all crossed."""
import numpy as np
import pytest
import torch

from paif_amd import ops, synthetic as S
from paif_amd.core import loss as L
from tests import fusion_loss_eager as E
from tests.helpers import t
from tests.kernel_check import dev, err, exact

pytestmark = pytest.mark.gpu

TILE = (32, 64)
CASES = ("1x1x1x1", "1x1x1x7", "1x1x7x1", "1x1x3x5", "2x1x19x29", "2x1x%dx%d" % (TILE[0] + 1, TILE[1] + 1))
SOBEL = [n for n, c in E.CRITERIA.items() if c[2] is not None]


def _planes(fx, ir_channels=3, rows=slice(None)):
    """Device tensors of a fixture: ir with 1 or 3 channels, vis as the 3-channel YCrCb tensor, mask, gen."""
    p = {k: t(np.ascontiguousarray(fx[k][rows])).to(dev()) for k in ("ir", "vis", "mask", "gen")}
    if ir_channels == 1:
        p["ir"] = p["ir"][:, :1].contiguous()
    return p


def _run(name, p, grad=True):
    """-> (value, d value / d gen) of the HIP criterion."""
    crit = getattr(L, name)()
    a = dict(p)
    if grad:
        a["gen"] = p["gen"].clone().requires_grad_(True)
    v = crit(*[a[k] for k in E.CRITERIA[name][1]])
    assert v.dim() == 0 and v.is_cuda and v.dtype == torch.float32, name
    if not grad:
        return v, None
    v.backward()
    return v.detach(), a["gen"].grad


@pytest.mark.parametrize("ir_channels", [1, 3])
@pytest.mark.parametrize("case", CASES)
def test_value_and_gradient_against_float64(golden, case, ir_channels):
    fx = golden("gl_fusion_losses_" + case)
    p = _planes(fx, ir_channels)
    n = fx["gen"].size
    for name in SOBEL:
        v, g = _run(name, p)
        print("floor | %s %s | value %.3e | gradient %.3e" % (name, case, fx[name + "/floor"][0], fx[name + "/floor"][1]))
        err("%s value %s" % (name, case), v, torch.tensor(float(fx[name + "/value64"]), dtype=torch.float64), E.value_bound(name))
        err("%s d gen %s" % (name, case), g, t(fx[name + "/dgen64"]), E.grad_bound(name, n))
        v0, _ = _run(name, p, grad=False)                       # the route without an autograd node
        exact("%s value without autograd %s" % (name, case), v0, v.cpu())


@pytest.mark.parametrize("case", CASES)
def test_fusionloss_grad3_against_float64(golden, case):
    fx = golden("gl_fusion_losses_" + case)
    v, g = _run("Fusionloss_grad3", _planes(fx))
    ref = t(fx["Fusionloss_grad3/dgen64"])
    err("Fusionloss_grad3 value " + case, v, torch.tensor(float(fx["Fusionloss_grad3/value64"]), dtype=torch.float64), 2e-5)
    err("Fusionloss_grad3 d gen " + case, g, ref, 2e-5 * float(ref.abs().max()))


@pytest.mark.parametrize("case", CASES)
def test_sobelxy_map_and_input_gradient(golden, case):
    """S <= 8 and |cotangent| <= 1: the two rules with one gradient weight 1 and N = 1 (a map, not a mean)."""
    fx = golden("gl_fusion_losses_" + case)
    x = t(fx["gen"]).to(dev()).requires_grad_(True)
    s = L.Sobelxy()(x)
    s.backward(t(fx["cot"]).to(dev()))
    err("Sobelxy " + case, s, t(fx["Sobelxy/out64"]), 2.0 ** -20 * 8)
    err("Sobelxy d x " + case, x.grad, t(fx["Sobelxy/dx64"]), 2.0 ** -20 * 8)
    with torch.no_grad():
        exact("Sobelxy without autograd " + case, L.Sobelxy()(x), s.detach().cpu())
    # a plane inside a wider tensor is read in place
    wide = t(np.ascontiguousarray(fx["vis"])).to(dev())
    wide[:, 1:2] = x.detach()
    exact("Sobelxy of a channel view " + case, ops.sobelxy(wide[:, 1:2]), s.detach().cpu())


def test_second_call_is_bit_identical(golden):
    fx = golden("gl_fusion_losses_" + CASES[-1])
    p = _planes(fx)
    for name in E.CRITERIA:
        (v1, g1), (v2, g2) = _run(name, p), _run(name, p)
        exact(name + " value, second call", v2, v1.cpu())
        exact(name + " d gen, second call", g2, g1.cpu())


def test_two_copies_of_one_image_against_batch_of_one(golden):
    """The images of a batch are padded and reduced on their own: a batch of two copies gives each copy the B = 1 gradient bit for bit
    (times N1 / N2 = 1/2, exact), and the B = 1 value within the value bound."""
    fx = golden("gl_fusion_losses_" + CASES[-1])
    one = _planes(fx, rows=slice(0, 1))
    two = {k: torch.cat([v, v]).contiguous() for k, v in one.items()}
    for name in SOBEL:
        (v1, g1), (v2, g2) = _run(name, one), _run(name, two)
        exact(name + " d gen, copy 0", g2[0:1] * 2, g1.cpu())
        exact(name + " d gen, copy 1", g2[1:2] * 2, g1.cpu())
        err(name + " value, two copies", v2, v1.cpu().double(), E.value_bound(name))
    s1, s2 = ops.sobelxy(one["gen"]), ops.sobelxy(two["gen"])
    exact("Sobelxy, copy 0", s2[0:1], s1.cpu())
    exact("Sobelxy, copy 1", s2[1:2], s1.cpu())


def test_value_on_non_dyadic_planes():
    """Random float32 planes (no exactness): the value only, against the float64 restatement on the host."""
    B, H, W = 2, TILE[0] + 1, TILE[1] + 1
    p = {k: S.make_feature(900 + i, (B, c, H, W), 0.0, 1.0) for i, (k, c) in enumerate((("ir", 3), ("vis", 3), ("mask", 1), ("gen", 1)))}
    d = {k: t(v).to(dev()) for k, v in p.items()}
    for name in SOBEL:
        v, _ = _run(name, d, grad=False)
        err(name + " value, non-dyadic", v, E.call(name, p, dtype=torch.float64), E.value_bound(name))


def test_forward_and_backward_inside_a_captured_graph(golden):
    """No host synchronisation and no host read of the upstream gradient: value and gradient are captured in one graph and replayed
    on new inputs with the bits of the eager run."""
    fx = golden("gl_fusion_losses_" + CASES[-1])
    p = _planes(fx)
    other = {k: v.flip(0).contiguous() for k, v in p.items()}           # the two images swapped: new data of the same shape
    for name in ("Fusionloss", "Fusionloss6"):
        crit = getattr(L, name)()
        static = {k: v.clone() for k, v in p.items()}
        static["gen"].requires_grad_(True)
        args = [static[k] for k in E.CRITERIA[name][1]]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            torch.autograd.grad(crit(*args), static["gen"])              # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            value = crit(*args)
            grad, = torch.autograd.grad(value, static["gen"])
        with torch.no_grad():
            for k in static:
                static[k].copy_(other[k])
        graph.replay()
        torch.cuda.synchronize()
        v_e, g_e = _run(name, other)
        exact(name + " value, replayed", value.detach(), v_e.cpu())
        exact(name + " d gen, replayed", grad, g_e.cpu())


# ---- inside the composite models (mit_b0 at 2x64x96) ----------------------------------------------------------------------------
def _batch():
    ir, vis, lab = S.make_batch(2, 64, 96)
    mask = np.maximum(ir, vis[:, :1]).astype(np.float32)
    return tuple(t(a).to(dev()) for a in (ir, vis, mask, lab))


def _searched(crit):
    from paif_amd.core.model_fusion_auto import Network_MM_Searched
    from paif_amd.genotypes import FUSION_AT

    m = Network_MM_Searched(32, FUSION_AT, crit, torch.nn.CrossEntropyLoss(ignore_index=255), "mit_b0", num_classes=9).eval()
    S.load_formula_weights(m)
    return m.to(dev())


def test_searched_model_with_fusionloss6():
    m = _searched(L.Fusionloss6())
    ir, vis, mask, lab = _batch()
    with torch.no_grad():
        loss = m._loss(ir, vis, mask, lab)
        fused, seg = m(ir, vis)
        ycc = ops.rgb2ycrcb(vis)
        ref = m._criterion(ir, ycc, fused, mask) * 0.1 + m._seg_term(seg, lab) * 4
        print("Network_MM_Searched._loss with Fusionloss6: %.6f (criterion %.6f)" % (float(loss), float(m._criterion(ir, ycc, fused, mask))))
        exact("_loss = 0.1 criterion + 4 seg term", loss, ref.cpu())
        exact("_fusion_loss", m._fusion_loss(ir, vis, mask), m._criterion(ir, ycc, m.forward_fusion(ir, vis), mask).cpu())
    # parameter gradients: the model's loss method against the two steps taken by hand
    m._fusion_loss_lower(ir, vis, mask).backward()
    got = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    m.zero_grad(set_to_none=True)
    fused, _ = m(ir, vis)
    m._criterion(ir, ops.rgb2ycrcb(vis), fused, mask).backward()
    ref = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    assert sorted(got) == sorted(ref) and len(got) > 50
    assert any(float(v.abs().max()) > 0 for k, v in got.items() if k.startswith("enhance_net."))
    diff = [k for k in got if not torch.equal(got[k], ref[k])]
    print("param.grad of %d tensors, %d differ" % (len(got), len(diff)))
    assert not diff, diff[:8]
    with pytest.raises(NotImplementedError, match="reads its image arguments"):
        m._fusion_loss_lower(ir.clone().requires_grad_(True), vis, mask)
    with pytest.raises(NotImplementedError, match="reads its image arguments"):
        m._fusion_loss_lower(ir, vis.clone().requires_grad_(True), mask)


def test_compmodel_seafusion_with_its_own_loss(golden):
    from paif_amd.core.model_fusion_auto import Network_MM_CompModel
    from paif_amd.fusion_model.seafusion import SeaFusion

    g = golden("gs_seafusion")
    m = Network_MM_CompModel(SeaFusion(), L.Fusionloss(), torch.nn.CrossEntropyLoss(ignore_index=255), "mit_b0", num_classes=9).eval()
    S.load_formula_weights(m)
    m.enhance_net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in S.seafusion_state_dict(g["scales"], g["shift"]).items()},
                                  strict=True)
    m = m.to(dev())
    ir, vis, mask, lab = _batch()
    with torch.no_grad():
        loss = m._loss(ir, vis, mask, lab)
        fused, seg = m(ir, vis)
        crit = m._criterion(ir, ops.rgb2ycrcb(vis), fused)
        print("Network_MM_CompModel(SeaFusion)._loss with Fusionloss: %.6f (criterion %.6f)" % (float(loss), float(crit)))
        exact("_loss = 0.1 criterion + 4 seg term", loss, (crit * 0.1 + m._seg_term(seg, lab) * 4).cpu())
        v64 = E.call("Fusionloss", dict(ir=ir.cpu(), vis=ops.rgb2ycrcb(vis).cpu(), gen=fused.cpu()), dtype=torch.float64)
        err("Fusionloss on the fused image", crit, v64, E.value_bound("Fusionloss"))
