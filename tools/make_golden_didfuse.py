"""TEST INFRASTRUCTURE -- fixtures of the DIDFuse baseline.  Build container only (CPU):

    python tools/make_golden_didfuse.py <reference tree>

Imports the reference's own fusion_model.AUIF.DID, core.model_fusion_auto.Network_MM_CompModel and attack.attack from the tree given on
the command line (through the shims of oracle/ref_import.py) and stores what they compute, in .eval() mode, under tests/golden/:

gd_didfuse.npz                  the eleven conv scales and the shift of cov7's conv bias (the weights are
                                paif_amd.synthetic.didfuse_state_dict(scales, shift)), the achieved calibration figures, and per case
                                the kept start and its margins
gd_didfuse_<case>.npz           inputs and the fused plane in float32 and float64; for the six gradient cases also the cotangent and
                                d_i1 / d_i2 from float32 and float64 autograd
gd_didfuse_<case>_maps<n>.npz   for 1x4x5 and 1x13x17: the 14 taped maps (896 channels, DID._map_list order) in float64 with one scalar
                                floor max|ref32 - ref64| per map, maps 0..7 (the two encoders) in file 0, 8..13 in file 1
gd_didfuse_attack.npz           Network_MM_CompModel(DID(), mit_b0) with those weights: clean forward and a PGD-3 trace of attack_both,
                                in the layout of gs_seafusion_attack.npz, float32 and float64 (`f32_vs_f64`: losses, signs of the last
                                running sums ir / vis, delta elements ir / vis), plus `stability` (see THE ATTACK BATCH below); DIDFUSE_ATTACK_ONLY=1 in the environment rewrites this file alone from the stored scales

i1 is the infrared plane and enters x_over (AE_Encoder1), i2 is the visible Y plane and enters x_under (AE_Encoder2): the order inside the
composite model.

CALIBRATION.  Formula weights (S.didfuse_state_dict: BatchNorm entries that are not the identity, the six PReLU slopes 0.10 .. 0.35), then
two sweeps that rescale each of the eleven convs, weight and bias, to a post-BatchNorm standard deviation of 1 on the planes of
S.make_batch(2, 48, 64, 0); cov7's conv bias is then shifted to a pre-sigmoid mean of 0.  Asserted and stored: every post-BatchNorm
pre-activation's std in [0.8, 1.25]; a negative share in [0.2, 0.8] at each of the 6 PReLU inputs; at least 40 % of the tanh outputs with
|tanh| < 0.9 and at least 40 % of the fused pixels in (0.1, 0.9).

THE MARGIN CONDITION (tools/make_golden_u2fusion.py).  PReLU's gradient jumps at zero.  Per gradient case the inputs are
S.make_batch(B, H, W, start=s) for the first s = 0, 1, 2, ... at which, in float64, min|.| over all 384 sign points per pixel (the six
PReLU inputs, 64 channels each) is >= 2e-5 and >= 6 * max|pre32 - pre64|.  1x37x53 and 2x24x32 are forward-only cases (start 0).
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
GRAD_CASES = {"1x2x3": (1, 2, 3), "1x4x5": (1, 4, 5), "1x13x17": (1, 13, 17), "2x9x20": (2, 9, 20), "1x5x37": (1, 5, 37),
              "1x19x18": (1, 19, 18)}
SPARES = {"1x35x6": (1, 35, 6), "1x17x19": (1, 17, 19), "1x7x35": (1, 7, 35)}   # for a gradient case without a start up to MAX_START
FWD_CASES = {"1x37x53": (1, 37, 53), "2x24x32": (2, 24, 32)}
WITH_MAPS = ("1x4x5", "1x13x17")
EPS, ALPHA, ITERS = 8 / 255.0, 2 / 255.0, 3
MARGIN_ABS, MARGIN_REL, MAX_START = 2e-5, 6.0, 2000
ATTACK_CAP = 1e-3
# THE ATTACK BATCH.  PGD takes the sign of a gradient and amplifies a single branch flipped upstream (a ReLU of the segmentation head, a
# clamp of the colour glue, a PReLU here) from iteration to iteration, and a batch can sit within fp32 reach of such a flip without the
# reference's own float32 and float64 runs showing it.  So a batch is kept only if the reference's float32 trace is also STABLE under a
# perturbation of the fused plane of the size the kernel parity bound allows an implementation (1.5 * floor + 1e-5, about 1.2e-5: uniform
# noise of amplitude PERTURB, the same at every iteration): losses within 5e-5, sign and delta mismatch within 1e-3 of the unperturbed
# trace -- half of what tests/test_didfuse_gpu.py allows.  Only the reference is run for this choice.
#
# The running sums also have elements of every size down to 1e-8 of their largest (at 2x64x96 about ten of the 49,152 lie below 1e-6 of
# it), so in ANY batch a few PGD sign points are within fp32 reach of zero; one that falls the other way at the first iteration moves an
# input by 2 * ALPHA and grows to about 1.5e-3 of the deltas by the third.  The test's 2e-3 has room for one such cascade, and it compares
# with the FLOAT32 trace: whatever that trace differs from the float64 one is taken from the implementation's share.  So the float32
# trace kept here takes exactly the float64 trace's steps -- no delta element differs (ATTACK_DELTA_CAP) -- besides the cap on the signs of
# the last running sum.
PERTURB, STABLE_LOSS, STABLE_FRAC = 1.2e-5, 5e-5, 1e-3
ATTACK_DELTA_CAP = 0.0
NCONV = len(S.DIDFUSE_CONVS)
LAST = NCONV - 1


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


def bns_of(net):
    """The eleven BatchNorm2d modules in S.DIDFUSE_CONVS order: their outputs are the pre-activations."""
    return [net.get_submodule("%s.%d" % (prefix, k + 1)) for prefix, k, _, _, _ in S.DIDFUSE_CONVS]


def map_modules(net):
    """The ten modules whose outputs are taped maps: per encoder Cov1 .. Cov4, then Cov5, Cov6."""
    out = []
    for e in (net.AE_Encoder1, net.AE_Encoder2):
        out += [e.cov1, e.cov2, e.cov3, e.cov4]
    return out + [net.AE_Decoder1.cov5, net.AE_Decoder1.cov6]


def loaded(Ref, scales, shift):
    net = Ref().eval()
    net.load_state_dict({k: t(v) for k, v in S.didfuse_state_dict(scales, shift).items()}, strict=True)
    return net


def probe(net, i1, i2):
    """-> (the eleven post-BatchNorm pre-activations, the fused plane)."""
    got = {}
    handles = [c.register_forward_hook(lambda m, i, o, k=k: got.__setitem__(k, o.detach().clone())) for k, c in enumerate(bns_of(net))]
    with torch.no_grad():
        fused = net(i1, i2)
    for h in handles:
        h.remove()
    return [got[k] for k in range(NCONV)], fused


def sign_points(pre):
    """The 6 PReLU inputs: 384 channels."""
    pts = [pre[k] for k, (_, _, _, _, prelu) in enumerate(S.DIDFUSE_CONVS) if prelu]
    assert len(pts) == 6 and sum(p.shape[1] for p in pts) == 384
    return pts


def tanh_inputs(pre):
    return [pre[k] for k, (prefix, _, _, _, _) in enumerate(S.DIDFUSE_CONVS) if prefix.endswith(("cov3", "cov4"))]


def calibrated(Ref):
    i1, i2 = planes(2, 48, 64, 0)
    scales, shift = np.ones(NCONV, dtype=np.float32), np.float32(0)
    for _ in range(2):
        for k in range(NCONV):
            pre, _ = probe(loaded(Ref, scales, shift), i1, i2)
            scales[k] = np.float32(scales[k] / pre[k].std().item())
    net = loaded(Ref, scales, shift)
    pre, _ = probe(net, i1, i2)
    bn = bns_of(net)[LAST]
    gain = float((bn.weight[0] / torch.sqrt(bn.running_var[0] + bn.eps)).detach())     # d(post-BN) / d(conv bias)
    shift = np.float32(-pre[LAST].mean().item() / gain)
    net = loaded(Ref, scales, shift)
    pre, fused = probe(net, i1, i2)
    inside = float(((fused > 0.1) & (fused < 0.9)).float().mean())
    stds = [p.std().item() for p in pre]
    neg = [(p < 0).float().mean().item() for p in sign_points(pre)]
    soft = float(np.mean([(torch.tanh(p).abs() < 0.9).float().mean().item() for p in tanh_inputs(pre)]))
    assert len(tanh_inputs(pre)) == 4
    assert all(0.8 <= s <= 1.25 for s in stds), stds
    assert abs(pre[LAST].mean().item()) <= 1e-3, pre[LAST].mean().item()
    assert all(0.2 <= n <= 0.8 for n in neg), neg
    assert soft >= 0.4 and inside >= 0.4, (soft, inside)
    print("post-BN std %s\nnegative share %s  pre-sigmoid mean %.3f  |tanh| < 0.9: %.2f  fused inside (0.1,0.9): %.2f"
          % (["%.3f" % s for s in stds], ["%.2f" % n for n in neg], pre[LAST].mean().item(), soft, inside), flush=True)
    return net, scales, shift, np.array(stds, dtype=np.float64), np.array(neg, dtype=np.float64), soft, inside


def margins(net, net64, i1, i2):
    p32 = sign_points(probe(net, i1, i2)[0])
    p64 = sign_points(probe(net64, i1.double(), i2.double())[0])
    least = min(p.abs().min().item() for p in p64)
    floor = max((a.double() - b).abs().max().item() for a, b in zip(p32, p64))
    return least, floor


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
        # DID._map_list order: the eight encoder maps, the means F_1, F_2, F_b, F_d as the reference forms them, Out1, Out2
        means = [(got[k] + got[4 + k]) / 2 for k in range(4)]
        res["maps"] = [npy(x) for x in [got[k] for k in range(8)] + means + [got[8], got[9]]]      # [B, 64, H, W] each
        assert len(res["maps"]) == 14 and sum(x.shape[1] for x in res["maps"]) == 896
    return res


def first_start(net, net64, B, H, W):
    for start in range(MAX_START + 1):
        i1, i2 = planes(B, H, W, start)
        least, floor = margins(net, net64, i1, i2)
        if least >= MARGIN_ABS and least >= MARGIN_REL * floor:
            return start, i1, i2, least, floor
    return None


def didfuse_fixtures(Ref):
    net, scales, shift, stds, neg, soft, inside0 = calibrated(Ref)
    net64 = copy.deepcopy(net).double()
    index = {"scales": scales, "shift": np.array(shift, dtype=np.float32), "stats_std": stds, "stats_negative_share": neg,
             "stats_tanh_soft": np.array(soft), "stats_inside": np.array(inside0)}
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
        else:
            start, cot = 0, None
            i1, i2 = planes(B, H, W, start)
            least, floor = margins(net, net64, i1, i2)     # recorded, not a condition: the forward is continuous
        r32 = run(net, i1, i2, cot, torch.float32, name in WITH_MAPS)
        r64 = run(net, i1, i2, cot, torch.float64, name in WITH_MAPS)
        inside = float(((r64["fused"] > 0.1) & (r64["fused"] < 0.9)).mean())
        print("%-8s %s start %4d  min|sign point| %.2e  fp32 floor of the sign points %.2e  fused inside (0.1,0.9): %.2f"
              % (name, "gradient" if grad else "forward ", start, least, floor, inside), flush=True)
        index["case_%s" % name] = np.array([start, least, floor, inside], dtype=np.float64)
        arrays = dict(i1=npy(i1), i2=npy(i2), fused=r32["fused"], fused64=r64["fused"])
        if grad:
            arrays.update(cot=npy(cot), d_i1=r32["d_i1"], d_i2=r32["d_i2"], d_i164=r64["d_i1"], d_i264=r64["d_i2"])
        save("gd_didfuse_" + name, **arrays)
        if name in WITH_MAPS:
            floors = np.array([np.abs(r32["maps"][k].astype(np.float64) - r64["maps"][k]).max() for k in range(14)])
            for part, ks in enumerate((range(0, 8), range(8, 14))):
                save("gd_didfuse_%s_maps%d" % (name, part), map_floor=floors, **{"map%d" % k: r64["maps"][k] for k in ks})
    save("gd_didfuse", **index)
    return net


def attack_run(R, m, start):
    """tools/make_golden_seafusion.py:attack_run with DID as the fusion module, on S.make_batch(2, 64, 96, start)."""
    ir, vis, lab = (t(a) for a in S.make_batch(2, 64, 96, start=start))
    torch.manual_seed(1234)
    d0_ir = torch.zeros_like(ir).uniform_(-EPS, EPS)
    d0_vis = torch.zeros_like(vis).uniform_(-EPS, EPS)

    with torch.no_grad():
        fused, seg = m(ir, vis)
    # the reference's own attack_both: it draws delta0 from the global RNG, ir first
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

    # float64: the reference's DID in double between the restated colour glue and segmentation network (the reference's own colour
    # transform builds float32 constants), from the SAME float32 delta0
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in m.state_dict().items()}
    u64 = copy.deepcopy(m.enhance_net).double().eval()

    def fwd64(a, b):
        ycc = O.rgb2ycrcb(b)
        fz = u64(a[:, 0:1], ycc[:, 0:1])
        return fz, O.wetr_forward(O.seg_input_from_fused(fz, ycc), sd64, "denoise_net.", "mit_b0")

    with torch.no_grad():
        fused64, seg64 = fwd64(ir.double(), vis.double())
    assert float((fused64 - fused.double()).abs().max()) <= 1e-5, "the float64 composition must be the float32 model's"
    tr64 = []
    d64 = O.attack_both(fwd64, vis.double(), ir.double(), lab, d0_ir.double(), d0_vis.double(), EPS, ALPHA, ITERS, "PGD", trace=tr64)
    up = torch.nn.functional.interpolate(seg, size=lab.shape[1:], mode="bilinear", align_corners=False)
    pred = up.argmax(1).numpy()
    losses64 = np.array([s["loss"] for s in tr64])
    rel = float(np.abs(np.array(losses) / losses64 - 1).max())
    mism = [float((torch.sign(tr32[-1][k]).double() != torch.sign(tr64[-1][k])).double().mean()) for k in ("g_ir", "g_vis")]
    # the third figure of tests/test_didfuse_gpu.py:_check_attack, the share of delta elements further than 1e-6 apart: an element differs
    # if the sign of the running sum differed at ANY of the three iterations, so it is larger than the sign mismatch of the last one
    mism += [float(((a.double() - b).abs() > 1e-6).double().mean()) for a, b in zip((d_ir, d_vis), d64)]
    arrays = dict(start=np.array(start), fused=npy(fused), logits=npy(seg), fused64=npy(fused64), logits64=npy(seg64), pred=pred.astype(np.uint8),
                  conf=O.confusion_matrix(lab.numpy(), pred),
                  d0_ir=npy(d0_ir), d0_vis=npy(d0_vis), delta_ir=npy(d_ir), delta_vis=npy(d_vis),
                  gsum_ir=npy(d_ir.grad), gsum_vis=npy(d_vis.grad), losses=np.array(losses),
                  gsum_ir64=npy(tr64[-1]["g_ir"]).astype(np.float32), gsum_vis64=npy(tr64[-1]["g_vis"]).astype(np.float32),
                  losses64=losses64, f32_vs_f64=np.array([rel] + mism))
    print("attack start %d: losses %s (float64 %s), loss relative difference %.1e, sign (ir, vis) and delta (ir, vis) mismatch float32 / float64 %s, classes in the clean map: %s"
          % (start, losses, losses64, rel, mism, np.bincount(pred.ravel(), minlength=9)), flush=True)
    return arrays, rel, mism


def stability(m, start):
    """-> (largest relative loss difference, largest sign / delta mismatch) of the reference's float32 PGD trace under the perturbation."""
    ir, vis, lab = (t(a) for a in S.make_batch(2, 64, 96, start=start))
    torch.manual_seed(1234)
    d0_ir = torch.zeros_like(ir).uniform_(-EPS, EPS)
    d0_vis = torch.zeros_like(vis).uniform_(-EPS, EPS)
    noise = t(S.make_feature(4242, (2, 1, 64, 96))) * PERTURB
    runs = []
    for perturbed in (False, True):
        plain = m.enhance_net.forward          # the composite calls .forward itself: a forward hook would not be run
        if perturbed:
            m.enhance_net.forward = lambda a, b: plain(a, b) + noise
        tr = []
        try:
            d = O.attack_both(lambda a, b: m(a, b), vis, ir, lab, d0_ir, d0_vis, EPS, ALPHA, ITERS, "PGD", trace=tr)
        finally:
            if perturbed:
                del m.enhance_net.forward
        runs.append((tr, d))
    (ta, da), (tb, db) = runs
    rel = max(abs(x["loss"] / y["loss"] - 1) for x, y in zip(ta, tb))
    frac = max([float((torch.sign(ta[-1][k]) != torch.sign(tb[-1][k])).float().mean()) for k in ("g_ir", "g_vis")]
               + [float(((x - y).abs() > 1e-6).float().mean()) for x, y in zip(da, db)])
    print("attack start %d: under the perturbation the losses move by %.1e, signs / deltas differ at %.1e" % (start, rel, frac), flush=True)
    return rel, frac


def attack_fixture(R, Ref, net):
    with ref_import.quiet():
        m = R["mfa"].Network_MM_CompModel(Ref(), None, None, "mit_b0", num_classes=9)
    m.eval()
    S.load_formula_weights(m, head=S.head_tag("mit_b0", 2, 64, 96))
    m.enhance_net.load_state_dict(net.state_dict(), strict=True)
    assert not m.enhance_net.training
    for start in range(MAX_START + 1):      # the first stable batch whose float32 run stays within the cap of its float64 run
        srel, sfrac = stability(m, start)
        if srel > STABLE_LOSS or sfrac > STABLE_FRAC:
            continue
        arrays, rel, mism = attack_run(R, m, start)
        if rel <= ATTACK_CAP and max(mism) <= ATTACK_CAP and max(mism[2:]) <= ATTACK_DELTA_CAP:
            break
    else:
        raise RuntimeError("no attack batch up to start %d keeps float32 within %g of float64" % (MAX_START, ATTACK_CAP))
    assert rel <= ATTACK_CAP and max(mism) <= ATTACK_CAP and max(mism[2:]) <= ATTACK_DELTA_CAP and srel <= STABLE_LOSS and sfrac <= STABLE_FRAC
    arrays["stability"] = np.array([PERTURB, srel, sfrac])
    # the weights are gd_didfuse.npz's scales and shift: no second copy
    save("gd_didfuse_attack", **arrays)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref_import.REF_ROOT = os.path.abspath(sys.argv[1])
    R = ref_import.load()
    import fusion_model.AUIF as ref_did
    assert os.path.abspath(ref_did.__file__).startswith(ref_import.REF_ROOT), ref_did.__file__
    torch.set_num_threads(8)
    os.makedirs(OUT, exist_ok=True)
    if os.environ.get("DIDFUSE_ATTACK_ONLY"):      # the attack fixture alone, from the stored scales and shift
        g = np.load(os.path.join(OUT, "gd_didfuse.npz"))
        net = loaded(ref_did.DID, g["scales"], g["shift"])
    else:
        net = didfuse_fixtures(ref_did.DID)
    attack_fixture(R, ref_did.DID, net)


if __name__ == "__main__":
    main()
