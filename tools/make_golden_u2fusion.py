"""TEST INFRASTRUCTURE -- fixtures of the U2Fusion baseline.  Build container only (CPU):

    python tools/make_golden_u2fusion.py <reference tree>

Imports the reference's own fusion_model.U2Fusion.U2Fusion, core.model_fusion_auto.Network_MM_CompModel and attack.attack from the tree
given on the command line (through the shims of oracle/ref_import.py) and stores what they compute under tests/golden/:

gu_u2fusion.npz           the ten conv scales and the shift of sub.3.bias (the weights are paif_amd.synthetic.u2fusion_state_dict(scales,
                          shift): 658,728 floats would not fit a committed file), the achieved calibration figures, and per case the kept
                          start and its margins
gu_u2fusion_<case>.npz    inputs and the fused plane in float32 and float64; for the five gradient cases also the cotangent and d_i1 /
                          d_i2 from float32 and float64 autograd; for 1x4x5 and 1x13x17 the nine LeakyReLU maps in float64 with one
                          scalar floor max|ref32 - ref64| per map (both precisions in full would pass 1 MiB)
gu_u2fusion_attack.npz    Network_MM_CompModel(U2Fusion(), mit_b0) with those weights: clean forward and a PGD-3 trace of attack_both, in
                          the layout of gs_sdnet_attack.npz, float32 and float64

CALIBRATION.  Formula weights (S.formula_tensor("u2/" + key)), then two sweeps that rescale each conv, weight and bias, to a
pre-activation standard deviation of 1 on the planes of S.make_batch(2, 48, 64, 0); sub.3.bias is then shifted so that the pre-tanh mean
is 0.55 (the composite clamps the fused plane to [0, 1]).  Asserted and stored: the share of negative pre-activations of each of the nine
maps lies in [0.2, 0.8], and at least 40 % of the fused pixels of the calibration planes lie strictly inside (0, 1).  The same share is
recorded per case without a condition: the cases are at most 37 x 53 and as much border as interior.

THE MARGIN CONDITION (tools/make_golden_sdnet.py).  LeakyReLU's gradient jumps at zero: one element whose fp32 sign differs from the
float64 sign puts an order-0.1 error into a 21 x 21 patch of the input gradient.  Per gradient case the inputs are
S.make_batch(B, H, W, start=s) for the first s = 0, 1, 2, ... at which, in float64, min|pre-activation| over the nine maps is >= 2e-5 and
>= 6 * max|pre32 - pre64|.  With 488 pre-activations per pixel only small cases meet it; 1x37x53 and 2x24x32 are forward-only cases
(start 0): the forward is continuous and needs no margin.

The reference's LeakyReLU is in place, so every hook stores a clone of what it sees.
"""
import copy
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_import  # noqa: E402
from oracle import paif_oracle as O  # noqa: E402
from paif_amd import synthetic as S  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
GRAD_CASES = {"1x4x5": (1, 4, 5), "1x13x17": (1, 13, 17), "2x9x20": (2, 9, 20), "1x11x37": (1, 11, 37), "1x19x35": (1, 19, 35)}
FWD_CASES = {"1x37x53": (1, 37, 53), "2x24x32": (2, 24, 32)}
WITH_MAPS = ("1x4x5", "1x13x17")
EPS, ALPHA, ITERS = 8 / 255.0, 2 / 255.0, 3
MARGIN_ABS, MARGIN_REL, MAX_START = 2e-5, 6.0, 2000
ATTACK_CAP = 1e-3


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def npy(x):
    return x.detach().cpu().numpy()


def save(name, **arrays):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    print("wrote %-40s %8.1f KB" % (name + ".npz", size / 1024), flush=True)
    assert size < (1 << 20), "a committed file stays under 1 MiB"


def planes(B, H, W, start):
    """x_over = infrared, x_under = visible Y of the synthetic pairs, in [0,1] (as tools/make_golden_sdnet.py)."""
    ir, vis, _ = S.make_batch(B, H, W, start=start)
    i1 = t(ir)[:, 0:1].clone()
    i2 = O.rgb2ycrcb(t(vis))[:, 0:1].clamp(0, 1).clone()
    return i1.contiguous(), i2.contiguous()


def convs_of(net):
    """The ten Conv2d modules in S.U2FUSION_CONVS order."""
    return [net.conv_1[0]] + [d.conv[0] for d in net.dense_layers] + [net.sub[0][0], net.sub[1][0], net.sub[2][0], net.sub[3]]


def acts_of(net):
    """The nine LeakyReLU modules, in layer order."""
    return [net.conv_1[1]] + [d.conv[1] for d in net.dense_layers] + [net.sub[0][1], net.sub[1][1], net.sub[2][1]]


def loaded(Ref, scales, shift):
    net = Ref().eval()
    net.load_state_dict({k: t(v) for k, v in S.u2fusion_state_dict(scales, shift).items()}, strict=True)
    return net


def probe(net, i1, i2):
    """-> (the pre-activations of the ten convs, the fused plane).  The hooks clone: the activation that follows works in place."""
    got = {}
    handles = [c.register_forward_hook(lambda m, i, o, k=k: got.__setitem__(k, o.detach().clone())) for k, c in enumerate(convs_of(net))]
    with torch.no_grad():
        fused = net(i1, i2)
    for h in handles:
        h.remove()
    return [got[k] for k in range(10)], fused


def calibrated(Ref):
    i1, i2 = planes(2, 48, 64, 0)
    scales, shift = np.ones(10, dtype=np.float32), np.float32(0)
    for _ in range(2):
        for k in range(10):
            pre, _ = probe(loaded(Ref, scales, shift), i1, i2)
            scales[k] = np.float32(scales[k] / pre[k].std().item())
    pre, _ = probe(loaded(Ref, scales, shift), i1, i2)
    shift = np.float32(0.55 - pre[9].mean().item())
    net = loaded(Ref, scales, shift)
    pre, fused = probe(net, i1, i2)
    inside = float(((fused > 0) & (fused < 1)).float().mean())
    stds = [p.std().item() for p in pre]
    neg = [(p < 0).float().mean().item() for p in pre[:9]]
    assert all(0.8 <= s <= 1.25 for s in stds), stds
    assert abs(pre[9].mean().item() - 0.55) <= 1e-3, pre[9].mean().item()
    assert all(0.2 <= n <= 0.8 for n in neg), neg
    assert inside >= 0.4, inside
    print("pre-activation std %s\nnegative share %s  pre-tanh mean %.3f  fused inside (0,1): %.2f"
          % (["%.3f" % s for s in stds], ["%.2f" % n for n in neg], pre[9].mean().item(), inside), flush=True)
    return net, scales, shift, np.array(stds, dtype=np.float64), np.array(neg, dtype=np.float64), inside


def margins(net, net64, i1, i2):
    p32, _ = probe(net, i1, i2)
    p64, _ = probe(net64, i1.double(), i2.double())
    least = min(p.abs().min().item() for p in p64[:9])
    floor = max((a.double() - b).abs().max().item() for a, b in zip(p32[:9], p64[:9]))
    return least, floor


def run(net, i1, i2, cot, dtype, with_maps):
    m = copy.deepcopy(net).to(dtype)
    a = i1.to(dtype).clone().requires_grad_(True)
    b = i2.to(dtype).clone().requires_grad_(True)
    got = {}
    handles = [act.register_forward_hook(lambda mod, i, o, k=k: got.__setitem__(k, o.detach().clone())) for k, act in enumerate(acts_of(m))]
    fused = m(a, b)
    for h in handles:
        h.remove()
    res = dict(fused=npy(fused))
    if cot is not None:
        (fused * cot.to(dtype)).sum().backward()
        res.update(d_i1=npy(a.grad), d_i2=npy(b.grad))
    if with_maps:
        res["maps"] = [npy(got[k]) for k in range(9)]      # [B, C, H, W] each
    return res


def u2fusion_fixtures(Ref):
    net, scales, shift, stds, neg, inside0 = calibrated(Ref)
    net64 = copy.deepcopy(net).double()
    index = {"scales": scales, "shift": np.array(shift, dtype=np.float32), "stats_std": stds, "stats_negative_share": neg,
             "stats_inside": np.array(inside0)}
    for name, (B, H, W) in list(GRAD_CASES.items()) + list(FWD_CASES.items()):
        grad = name in GRAD_CASES
        if grad:
            for start in range(MAX_START + 1):
                i1, i2 = planes(B, H, W, start)
                least, floor = margins(net, net64, i1, i2)
                if least >= MARGIN_ABS and least >= MARGIN_REL * floor:
                    break
            else:
                raise RuntimeError("%s: no start up to %d meets the margin condition" % (name, MAX_START))
            assert least >= MARGIN_ABS and least >= MARGIN_REL * floor
            cot = t(S.make_feature(900 + len(name) + H, (B, 1, H, W)))
        else:
            start, cot = 0, None
            i1, i2 = planes(B, H, W, start)
            least, floor = margins(net, net64, i1, i2)     # recorded, not a condition: the forward is continuous
        r32 = run(net, i1, i2, cot, torch.float32, name in WITH_MAPS)
        r64 = run(net, i1, i2, cot, torch.float64, name in WITH_MAPS)
        inside = float(((r64["fused"] > 0) & (r64["fused"] < 1)).mean())
        print("%-8s %s start %4d  min|pre| %.2e  fp32 floor of the pre-activations %.2e  fused inside (0,1): %.2f"
              % (name, "gradient" if grad else "forward ", start, least, floor, inside), flush=True)
        index["case_%s" % name] = np.array([start, least, floor, inside], dtype=np.float64)
        arrays = dict(i1=npy(i1), i2=npy(i2), fused=r32["fused"], fused64=r64["fused"])
        if grad:
            arrays.update(cot=npy(cot), d_i1=r32["d_i1"], d_i2=r32["d_i2"], d_i164=r64["d_i1"], d_i264=r64["d_i2"])
        if name in WITH_MAPS:
            for k in range(9):
                arrays["map%d" % k] = r64["maps"][k]
            arrays["map_floor"] = np.array([np.abs(r32["maps"][k].astype(np.float64) - r64["maps"][k]).max() for k in range(9)])
        save("gu_u2fusion_" + name, **arrays)
    save("gu_u2fusion", **index)
    return net


def attack_run(R, m, net, start):
    """tools/make_golden_sdnet.py:attack_fixture with U2Fusion as the fusion module, on S.make_batch(2, 64, 96, start)."""
    ir, vis, lab = (t(a) for a in S.make_batch(2, 64, 96, start=start))
    torch.manual_seed(1234)
    d0_ir = torch.zeros_like(ir).uniform_(-EPS, EPS)
    d0_vis = torch.zeros_like(vis).uniform_(-EPS, EPS)

    with torch.no_grad():
        fused, seg = m(ir, vis)
    # the reference's own attack_both: it draws delta0 from the global RNG (attack/attack.py:434,439), ir first
    for p_ in m.parameters():
        p_.grad = None
    seg_maps = []

    def recording(a, b):
        fz, sg = m(a, b)
        seg_maps.append(sg.detach().clone())
        return fz, sg

    torch.manual_seed(1234)
    with torch.no_grad():
        d_ir, d_vis = R["attack"].attack_both(recording, vis, ir, lab, epsilon=EPS, alpha=ALPHA, attack_iters=ITERS, attack_loss="l_seg",
                                              attack_way="PGD")
    losses = []
    for sg in seg_maps:
        outp = torch.nn.functional.interpolate(sg, size=lab.shape[1:], mode="bilinear", align_corners=False)
        losses.append(float(R["attack"].Seg_loss()(outp, lab)))
    # the per-iteration running sums: the loop restated (oracle.paif_oracle.attack_both) around the reference's model, pinned to the run above
    tr32 = []
    O.attack_both(lambda a, b: m(a, b), vis, ir, lab, d0_ir, d0_vis, EPS, ALPHA, ITERS, "PGD", trace=tr32)
    assert np.allclose([s["loss"] for s in tr32], losses, rtol=1e-5), ([s["loss"] for s in tr32], losses)
    assert float((torch.sign(tr32[-1]["g_ir"]) != torch.sign(d_ir.grad)).float().mean()) <= 1e-3

    # float64: the reference's U2Fusion in double between the restated colour glue and segmentation network (the reference's own colour
    # transform builds float32 constants), from the SAME float32 delta0
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in m.state_dict().items()}
    u64 = copy.deepcopy(m.enhance_net).double()

    def fwd64(a, b):
        ycc = O.rgb2ycrcb(b)
        fz = u64(a[:, 0:1], ycc[:, 0:1])
        return fz, O.wetr_forward(O.seg_input_from_fused(fz, ycc), sd64, "denoise_net.", "mit_b0")

    with torch.no_grad():
        fused64, seg64 = fwd64(ir.double(), vis.double())
    assert float((fused64 - fused.double()).abs().max()) <= 1e-5, "the float64 composition must be the float32 model's"
    tr64 = []
    O.attack_both(fwd64, vis.double(), ir.double(), lab, d0_ir.double(), d0_vis.double(), EPS, ALPHA, ITERS, "PGD", trace=tr64)
    up = torch.nn.functional.interpolate(seg, size=lab.shape[1:], mode="bilinear", align_corners=False)
    pred = up.argmax(1).numpy()
    losses64 = np.array([s["loss"] for s in tr64])
    rel = float(np.abs(np.array(losses) / losses64 - 1).max())
    mism = [float((torch.sign(tr32[-1][k]).double() != torch.sign(tr64[-1][k])).double().mean()) for k in ("g_ir", "g_vis")]
    arrays = dict(start=np.array(start), fused=npy(fused), logits=npy(seg), fused64=npy(fused64), logits64=npy(seg64), pred=pred.astype(np.uint8),
                  conf=O.confusion_matrix(lab.numpy(), pred),
                  d0_ir=npy(d0_ir), d0_vis=npy(d0_vis), delta_ir=npy(d_ir), delta_vis=npy(d_vis),
                  gsum_ir=npy(d_ir.grad), gsum_vis=npy(d_vis.grad), losses=np.array(losses),
                  gsum_ir64=npy(tr64[-1]["g_ir"]).astype(np.float32), gsum_vis64=npy(tr64[-1]["g_vis"]).astype(np.float32),
                  losses64=losses64, f32_vs_f64=np.array([rel] + mism))
    print("attack start %d: losses %s (float64 %s), loss relative difference %.1e, sign mismatch float32 / float64 %s, classes in the clean map: %s"
          % (start, losses, losses64, rel, mism, np.bincount(pred.ravel(), minlength=9)), flush=True)
    return arrays, rel, mism


def attack_fixture(R, Ref, net):
    with ref_import.quiet():
        m = R["mfa"].Network_MM_CompModel(Ref(), None, None, "mit_b0", num_classes=9)
    m.eval()
    S.load_formula_weights(m, head=S.head_tag("mit_b0", 2, 64, 96))
    m.enhance_net.load_state_dict(net.state_dict(), strict=True)
    for start in range(MAX_START + 1):      # the first batch whose float32 run stays within the cap of its float64 run
        arrays, rel, mism = attack_run(R, m, net, start)
        if rel <= ATTACK_CAP and max(mism) <= ATTACK_CAP:
            break
    else:
        raise RuntimeError("no attack batch up to start %d keeps float32 within %g of float64" % (MAX_START, ATTACK_CAP))
    assert rel <= ATTACK_CAP and max(mism) <= ATTACK_CAP
    # the weights are gu_u2fusion.npz's scales and shift: no second copy
    save("gu_u2fusion_attack", **arrays)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref_import.REF_ROOT = os.path.abspath(sys.argv[1])
    R = ref_import.load()
    import fusion_model.U2Fusion as ref_u2
    assert os.path.abspath(ref_u2.__file__).startswith(ref_import.REF_ROOT), ref_u2.__file__
    torch.set_num_threads(8)
    os.makedirs(OUT, exist_ok=True)
    net = u2fusion_fixtures(ref_u2.U2Fusion)
    attack_fixture(R, ref_u2.U2Fusion, net)


if __name__ == "__main__":
    main()
