"""TEST INFRASTRUCTURE -- fixtures of the SeAFusion baseline.  Build container only (CPU):

    python tools/make_golden_seafusion.py <reference tree>

Imports the reference's own fusion_model.SeaFusion.SeaFusion, core.model_fusion_auto.Network_MM_CompModel and attack.attack from the tree
given on the command line (through the shims of oracle/ref_import.py) and stores what they compute under tests/golden/:

gs_seafusion.npz                 the thirty conv scales and the shift of decode1.conv.bias (the weights are
                                 paif_amd.synthetic.seafusion_state_dict(scales, shift)), the achieved calibration figures, and per case
                                 the kept start and its margins
gs_seafusion_<case>.npz          inputs and the fused plane in float32 and float64; for the five gradient cases also the cotangent and
                                 d_i1 / d_i2 from float32 and float64 autograd; for the two forward-only cases the share of output pixels
                                 the taped-branch test would exclude on the reference's own float32 / float64 depthwise responses
gs_seafusion_<case>_maps<n>.npz  for 1x4x5 and 1x13x17: the 21 taped maps (592 channels, SeaFusion._map_list order) in float64 with one
                                 scalar floor max|ref32 - ref64| per map, maps 0..8 (the image_vis stream) in file 0, 9..20 in file 1
gs_seafusion_attack.npz          Network_MM_CompModel(SeaFusion(), mit_b0) with those weights: clean forward and a PGD-3 trace of
                                 attack_both, in the layout of gu_u2fusion_attack.npz, float32 and float64

i1 is the infrared plane and enters image_vis, i2 is the visible Y plane and enters image_ir: the order inside the composite model.

CALIBRATION.  Formula weights (S.formula_tensor("sea/" + key)), the eight depthwise convs included, then two sweeps that rescale each of
the thirty convs, weight and bias, to an output standard deviation of 1 on the planes of S.make_batch(2, 48, 64, 0);
decode1.conv.bias is then shifted to a pre-tanh mean of 0.  Asserted and stored: every conv's std in [0.8, 1.25]; a negative share in
[0.2, 0.8] at each of the 25 sign points (the 13 LeakyReLU(0.2) inputs, the 4 convdown + convup sums, the 8 depthwise responses); at
least 40 % of the fused pixels in (0.1, 0.9).

THE MARGIN CONDITION (tools/make_golden_u2fusion.py).  LeakyReLU's and abs's gradients jump at zero.  Per gradient case the inputs are
S.make_batch(B, H, W, start=s) for the first s = 0, 1, 2, ... at which, in float64, min|.| over all 688 sign points per pixel is >= 2e-5
and >= 6 * max|pre32 - pre64|.  Only cases of up to about 360 pixels meet it; 1x37x53 and 2x24x32 are forward-only cases (start 0).
"""
import copy
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_import  # noqa: E402
from oracle import paif_oracle as O  # noqa: E402
from paif_amd import synthetic as S  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
GRAD_CASES = {"1x4x5": (1, 4, 5), "1x13x17": (1, 13, 17), "2x9x20": (2, 9, 20), "1x5x37": (1, 5, 37), "1x19x18": (1, 19, 18)}
SPARES = {"1x35x6": (1, 35, 6), "1x17x19": (1, 17, 19), "1x7x35": (1, 7, 35)}   # for a gradient case without a start up to MAX_START
FWD_CASES = {"1x37x53": (1, 37, 53), "2x24x32": (2, 24, 32)}
WITH_MAPS = ("1x4x5", "1x13x17")
EPS, ALPHA, ITERS = 8 / 255.0, 2 / 255.0, 3
MARGIN_ABS, MARGIN_REL, MAX_START = 2e-5, 6.0, 2000
ATTACK_CAP = 1e-3
NCONV = len(S.SEAFUSION_CONVS)
STREAMS = ("vis", "inf")


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
    """i1 = infrared, i2 = visible Y of the synthetic pairs, in [0,1] (as tools/make_golden_u2fusion.py)."""
    ir, vis, _ = S.make_batch(B, H, W, start=start)
    i1 = t(ir)[:, 0:1].clone()
    i2 = O.rgb2ycrcb(t(vis))[:, 0:1].clamp(0, 1).clone()
    return i1.contiguous(), i2.contiguous()


def convs_of(net):
    """The thirty Conv2d modules in S.SEAFUSION_CONVS order."""
    return [net.get_submodule(name) for name, _, _, _, _ in S.SEAFUSION_CONVS]


def map_modules(net):
    """The 21 modules whose outputs are the taped maps, in SeaFusion._map_list order."""
    out = []
    for s in STREAMS:
        out.append(getattr(net, s + "_conv"))
        for r in ("_rgbd1", "_rgbd2"):
            blk = getattr(net, s + r)
            out += [blk.dense.conv1, blk.dense.conv2, blk.sobelconv, blk]
    return out + [net.decode4, net.decode3, net.decode2]


def loaded(Ref, scales, shift):
    net = Ref().eval()
    net.load_state_dict({k: t(v) for k, v in S.seafusion_state_dict(scales, shift).items()}, strict=True)
    return net


def probe(net, i1, i2):
    """-> (the outputs of the thirty convs, the fused plane)."""
    got = {}
    handles = [c.register_forward_hook(lambda m, i, o, k=k: got.__setitem__(k, o.detach().clone())) for k, c in enumerate(convs_of(net))]
    with torch.no_grad():
        fused = net(i1, i2)
    for h in handles:
        h.remove()
    return [got[k] for k in range(NCONV)], fused


def sign_points(pre):
    """The 25 tensors whose sign selects a branch: the 13 LeakyReLU(0.2) inputs, the 4 convdown + convup sums (the reference's x1 + x2), the
    8 depthwise responses.  688 channels."""
    lrelu, sums, dw = [], [], []
    for k, (name, _, _, _, _) in enumerate(S.SEAFUSION_CONVS):
        if name.endswith(("_conv.conv", "dense.conv1.conv", "dense.conv2.conv")) or name in ("decode4.conv", "decode3.conv", "decode2.conv"):
            lrelu.append(pre[k])
        elif name.endswith("convdown.conv"):
            sums.append(pre[k] + pre[k + 3])      # convup follows convx, convy
        elif name.endswith(("convx", "convy")):
            dw.append(pre[k])
    assert (len(lrelu), len(sums), len(dw)) == (13, 4, 8) and sum(p.shape[1] for p in lrelu + sums + dw) == 688
    return lrelu + sums + dw


def calibrated(Ref):
    i1, i2 = planes(2, 48, 64, 0)
    scales, shift = np.ones(NCONV, dtype=np.float32), np.float32(0)
    for _ in range(2):
        for k in range(NCONV):
            pre, _ = probe(loaded(Ref, scales, shift), i1, i2)
            scales[k] = np.float32(scales[k] / pre[k].std().item())
    pre, _ = probe(loaded(Ref, scales, shift), i1, i2)
    shift = np.float32(-pre[NCONV - 1].mean().item())
    net = loaded(Ref, scales, shift)
    pre, fused = probe(net, i1, i2)
    inside = float(((fused > 0.1) & (fused < 0.9)).float().mean())
    stds = [p.std().item() for p in pre]
    neg = [(p < 0).float().mean().item() for p in sign_points(pre)]
    assert all(0.8 <= s <= 1.25 for s in stds), stds
    assert abs(pre[NCONV - 1].mean().item()) <= 1e-3, pre[NCONV - 1].mean().item()
    assert all(0.2 <= n <= 0.8 for n in neg), neg
    assert inside >= 0.4, inside
    print("conv output std %s\nnegative share %s  pre-tanh mean %.3f  fused inside (0.1,0.9): %.2f"
          % (["%.3f" % s for s in stds], ["%.2f" % n for n in neg], pre[NCONV - 1].mean().item(), inside), flush=True)
    return net, scales, shift, np.array(stds, dtype=np.float64), np.array(neg, dtype=np.float64), inside


def margins(net, net64, i1, i2):
    p32 = sign_points(probe(net, i1, i2)[0])
    p64 = sign_points(probe(net64, i1.double(), i2.double())[0])
    least = min(p.abs().min().item() for p in p64)
    floor = max((a.double() - b).abs().max().item() for a, b in zip(p32, p64))
    return least, floor


def excluded_share(net, net64, i1, i2):
    """tests/test_seafusion_gpu.py's exclusion rule on the reference's own float32 run: each depthwise conv's float32 response beside the
    float64 response to the SAME (float32) input map; the share of output pixels whose 5 x 5 neighbourhood holds a response with
    |float64 value| < max|float32 - float64| of that response map."""
    seen = {}
    names = [name for name, _, _, _, _ in S.SEAFUSION_CONVS if name.endswith(("convx", "convy"))]
    handles = [net.get_submodule(n).register_forward_hook(lambda m, i, o, n=n: seen.__setitem__(n, (i[0].detach().clone(), o.detach().clone())))
               for n in names]
    with torch.no_grad():
        net(i1, i2)
        for h in handles:
            h.remove()
        near = torch.zeros(i1.shape, dtype=torch.float64)
        for n in names:
            x32, r32 = seen[n]
            r64 = net64.get_submodule(n)(x32.double())
            floor = (r32.double() - r64).abs().max()
            near = torch.maximum(near, (r64.abs() < floor).double().amax(1, keepdim=True))
    return float((F.max_pool2d(near, 5, stride=1, padding=2) > 0).double().mean())


def run(net, i1, i2, cot, dtype, with_maps):
    m = copy.deepcopy(net).to(dtype)
    a = i1.to(dtype).clone().requires_grad_(True)
    b = i2.to(dtype).clone().requires_grad_(True)
    got = {}
    handles = [mod.register_forward_hook(lambda mod, i, o, k=k: got.__setitem__(k, o.detach().clone())) for k, mod in enumerate(map_modules(m))]
    fused = m(a, b)
    for h in handles:
        h.remove()
    res = dict(fused=npy(fused))
    if cot is not None:
        (fused * cot.to(dtype)).sum().backward()
        res.update(d_i1=npy(a.grad), d_i2=npy(b.grad))
    if with_maps:
        res["maps"] = [npy(got[k]) for k in range(21)]      # [B, C, H, W] each
        assert sum(x.shape[1] for x in res["maps"]) == 592
    return res


def first_start(net, net64, B, H, W):
    for start in range(MAX_START + 1):
        i1, i2 = planes(B, H, W, start)
        least, floor = margins(net, net64, i1, i2)
        if least >= MARGIN_ABS and least >= MARGIN_REL * floor:
            return start, i1, i2, least, floor
    return None


def seafusion_fixtures(Ref):
    net, scales, shift, stds, neg, inside0 = calibrated(Ref)
    net64 = copy.deepcopy(net).double()
    index = {"scales": scales, "shift": np.array(shift, dtype=np.float32), "stats_std": stds, "stats_negative_share": neg,
             "stats_inside": np.array(inside0)}
    for name, (B, H, W) in list(GRAD_CASES.items()) + list(FWD_CASES.items()):
        grad = name in GRAD_CASES
        if grad:
            found = first_start(net, net64, B, H, W)
            if found is None:
                raise RuntimeError("%s: no start up to %d meets the margin condition; take the nearest of %s in GRAD_CASES, here and in the "
                                   "tests" % (name, MAX_START, sorted(SPARES)))
            start, i1, i2, least, floor = found
            assert least >= MARGIN_ABS and least >= MARGIN_REL * floor
            cot = t(S.make_feature(900 + len(name) + H, (B, 1, H, W)))
            share = 0.0
        else:
            start, cot = 0, None
            i1, i2 = planes(B, H, W, start)
            least, floor = margins(net, net64, i1, i2)     # recorded, not a condition: the forward is continuous
            share = excluded_share(net, net64, i1, i2)
            assert share <= 0.01, (name, share)
        r32 = run(net, i1, i2, cot, torch.float32, name in WITH_MAPS)
        r64 = run(net, i1, i2, cot, torch.float64, name in WITH_MAPS)
        inside = float(((r64["fused"] > 0.1) & (r64["fused"] < 0.9)).mean())
        print("%-8s %s start %4d  min|sign point| %.2e  fp32 floor of the sign points %.2e  fused inside (0.1,0.9): %.2f  excluded share %.4f"
              % (name, "gradient" if grad else "forward ", start, least, floor, inside, share), flush=True)
        index["case_%s" % name] = np.array([start, least, floor, inside, share], dtype=np.float64)
        arrays = dict(i1=npy(i1), i2=npy(i2), fused=r32["fused"], fused64=r64["fused"])
        if grad:
            arrays.update(cot=npy(cot), d_i1=r32["d_i1"], d_i2=r32["d_i2"], d_i164=r64["d_i1"], d_i264=r64["d_i2"])
        save("gs_seafusion_" + name, **arrays)
        if name in WITH_MAPS:
            floors = np.array([np.abs(r32["maps"][k].astype(np.float64) - r64["maps"][k]).max() for k in range(21)])
            for part, ks in enumerate((range(0, 9), range(9, 21))):
                save("gs_seafusion_%s_maps%d" % (name, part), map_floor=floors, **{"map%d" % k: r64["maps"][k] for k in ks})
    save("gs_seafusion", **index)
    return net


def attack_run(R, m, net, start):
    """tools/make_golden_u2fusion.py:attack_run with SeaFusion as the fusion module, on S.make_batch(2, 64, 96, start)."""
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

    # float64: the reference's SeaFusion in double between the restated colour glue and segmentation network (the reference's own colour
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
    # the weights are gs_seafusion.npz's scales and shift: no second copy
    save("gs_seafusion_attack", **arrays)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref_import.REF_ROOT = os.path.abspath(sys.argv[1])
    R = ref_import.load()
    import fusion_model.SeaFusion as ref_sea
    assert os.path.abspath(ref_sea.__file__).startswith(ref_import.REF_ROOT), ref_sea.__file__
    torch.set_num_threads(8)
    os.makedirs(OUT, exist_ok=True)
    net = seafusion_fixtures(ref_sea.SeaFusion)
    attack_fixture(R, ref_sea.SeaFusion, net)


if __name__ == "__main__":
    main()
