"""TEST INFRASTRUCTURE -- fixtures of the hand-designed fusion network (Fusion_Network over two DRDB).  Build container only (CPU):

    python tools/make_golden_drdb.py <reference tree>

Imports the reference's own core.model_fusion_auto.Fusion_Network / DRDB / Network_MM_CompModel and attack.attack from the tree given on
the command line (through the shims of oracle/ref_import.py) and stores what they compute under tests/golden/:

gr_drdb.npz                      the fifteen conv scales, shift and last scale of weight set B (the weights are
                                 paif_amd.synthetic.drdb_state_dict(scales, shift, last_scale)), the achieved calibration figures, and per
                                 case and weight set the kept start, its margins and where the extrema sit
gr_drdb_<case>_<A|B>.npz         inputs and the fused plane in float32 and float64; for the five gradient cases also the cotangent and
                                 d_i1 / d_i2 from float32 and float64 autograd (forward-only cases: set A only)
gr_drdb_<case>_maps<n>.npz       for 1x3x5 and 1x13x17, set A: the 17 taped maps (673 channels, Fusion_Network._map_list order) in float64
                                 with one scalar floor max|ref32 - ref64| per map, maps 0..8 in file 0, 9..16 in file 1
gr_drdb_<case>_block.npz         for 1x3x5 and 1x13x17, set A: DRDB1 ALONE on the float32 map conv1 + PReLU gave: its output and, for the
                                 stored cotangent, d_x, float32 and float64
gr_drdb_attack.npz               Network_MM_CompModel(Fusion_Network(), mit_b0) with weight set A: clean forward and a PGD-3 trace of
                                 attack_both, in the layout of gu_u2fusion_attack.npz, float32 and float64

i1 is the infrared plane (the reference's `ir`), i2 the visible Y plane (`vis`): the order inside the composite model.

CALIBRATION.  Formula weights (S.formula_tensor(S.DRDB_PREFIX + key)), then two sweeps that rescale each of the fifteen convs, weight and bias,
to an output standard deviation of 1 on the planes of S.make_batch(2, 48, 64, 0).  That is weight set A: both clamps are active, so
min = 0 and max = 1 are attained by clamped pixels and the normalisation passes no gradient through its extrema.  Set B is A with conv21's
weight and bias times 0.1 and its bias + 0.5: no pixel is clamped, min and max are attained by single pixels and the extremum terms carry
gradient.  Asserted and stored: every conv's std in [0.8, 1.25]; a negative share in [0.2, 0.8] at each conv; on set A at least 5 % of
the pre-clamp pixels above 1 and at least 5 % below 0, min = 0, max = 1; on set B at most 1 % of the calibration pixels clamped (the
tails beyond five standard deviations; every CASE of set B has none, see below).

THE MARGIN CONDITION (tools/make_golden_u2fusion.py).  ReLU's, PReLU's and the clamp's gradients jump.  Per gradient case and weight set
the inputs are S.make_batch(B, H, W, start=s) for the first s = 0, 1, 2, ... at which, in float64, min|.| over all sign points -- the
pre-activations of the fifteen convs and the distance of f (conv21's PReLU output) to 0 and to 1 -- is >= 2e-5 and
>= 6 * max|pre32 - pre64|.  Set B additionally: no clamped pixel; the gap between each extremum of f and its runner-up >= 6 * the fp32
floor of f (so no exact tie, and float32 picks the same pixel); at 2x9x20 min and max fall in different images.  1x37x53 and 2x24x32 are
forward-only cases (start 0).
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
GRAD_CASES = {"1x3x5": (1, 3, 5), "1x13x17": (1, 13, 17), "2x9x20": (2, 9, 20), "1x5x37": (1, 5, 37), "1x19x18": (1, 19, 18)}
FWD_CASES = {"1x37x53": (1, 37, 53), "2x24x32": (2, 24, 32)}
WITH_MAPS = ("1x3x5", "1x13x17")
SETS = {"A": (0.0, 1.0), "B": (0.5, 0.1)}       # (shift, last_scale)
EPS, ALPHA, ITERS = 8 / 255.0, 2 / 255.0, 3
MARGIN_ABS, MARGIN_REL, MAX_START = 2e-5, 6.0, 2000
ATTACK_CAP = 1e-3
NCONV = len(S.DRDB_CONVS)
NMAPS = 17


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def npy(x):
    return x.detach().cpu().numpy()


def largest_committed():
    return max(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT) if not f.startswith("gr_drdb"))


def save(name, **arrays):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    print("wrote %-40s %8.1f KB" % (name + ".npz", size / 1024), flush=True)
    assert size < (1 << 20) and size <= largest_committed(), "a fixture stays under 1 MiB and under the largest one already committed"


def planes(B, H, W, start):
    """i1 = infrared, i2 = visible Y of the synthetic pairs, in [0,1] (as tools/make_golden_u2fusion.py)."""
    ir, vis, _ = S.make_batch(B, H, W, start=start)
    i1 = t(ir)[:, 0:1].clone()
    i2 = O.rgb2ycrcb(t(vis))[:, 0:1].clamp(0, 1).clone()
    return i1.contiguous(), i2.contiguous()


def convs_of(net):
    return [net.get_submodule(name) for name, _, _, _ in S.DRDB_CONVS]


def loaded(Ref, scales, which="A"):
    shift, last = SETS[which]
    with ref_import.quiet():
        net = Ref().eval()
    net.load_state_dict({k: t(v) for k, v in S.drdb_state_dict(scales, shift, last).items()}, strict=True)
    return net


def probe(net, i1, i2):
    """-> (the outputs of the fifteen convs, f = conv21's PReLU output before the clamp, the fused plane)."""
    got = {}
    handles = [c.register_forward_hook(lambda m, i, o, k=k: got.__setitem__(k, o.detach().clone())) for k, c in enumerate(convs_of(net))]
    with torch.no_grad():
        fused = net(i1, i2)
        f = net.relu(got[NCONV - 1])
    for h in handles:
        h.remove()
    return [got[k] for k in range(NCONV)], f, fused


def sign_points(pre, f):
    """The tensors whose sign selects a branch: the fifteen pre-activations, f - 0 and f - 1 (the clamp as torch.where decides it)."""
    return list(pre) + [f, f - 1]


def calibrated(Ref):
    i1, i2 = planes(2, 48, 64, 0)
    scales = np.ones(NCONV, dtype=np.float32)
    for _ in range(2):
        for k in range(NCONV):
            pre, _, _ = probe(loaded(Ref, scales), i1, i2)
            scales[k] = np.float32(scales[k] / pre[k].std().item())
    net = loaded(Ref, scales)
    pre, f, fused = probe(net, i1, i2)
    stds = [p.std().item() for p in pre]
    neg = [(p < 0).float().mean().item() for p in pre]
    above, below = float((f > 1).float().mean()), float((f < 0).float().mean())
    c = f.clamp(0, 1)
    assert all(0.8 <= s <= 1.25 for s in stds), stds
    assert all(0.2 <= n <= 0.8 for n in neg), neg
    assert above >= 0.05 and below >= 0.05, (above, below)
    assert float(c.min()) == 0.0 and float(c.max()) == 1.0
    _, fb, _ = probe(loaded(Ref, scales, "B"), i1, i2)
    clamped_b = float(((fb < 0) | (fb > 1)).float().mean())      # the tails of these 6144 pixels; every CASE of set B has none (margins)
    assert clamped_b <= 0.01, clamped_b
    print("conv output std %s\nnegative share %s\nset A: %.3f of the pre-clamp pixels above 1, %.3f below 0; set B: f in [%.3f, %.3f], %.4f clamped"
          % (["%.3f" % s for s in stds], ["%.2f" % n for n in neg], above, below, float(fb.min()), float(fb.max()), clamped_b), flush=True)
    return scales, np.array(stds), np.array(neg), np.array([above, below, float(fb.min()), float(fb.max()), clamped_b])


def extrema(f64):
    """-> (gap of the minimum to its runner-up, gap of the maximum, image of the minimum, image of the maximum) of f [B,1,H,W]."""
    flat = f64.reshape(-1)
    srt = torch.sort(flat).values
    per = flat.numel() // f64.shape[0]
    return (float(srt[1] - srt[0]), float(srt[-1] - srt[-2]), int(torch.argmin(flat)) // per, int(torch.argmax(flat)) // per)


def margins(net, net64, i1, i2, which):
    """-> (min|sign point| in float64, fp32 floor of the sign points, ok): ok holds the extra conditions of set B."""
    pre32, f32, _ = probe(net, i1, i2)
    pre64, f64, _ = probe(net64, i1.double(), i2.double())
    p64 = sign_points(pre64, f64)
    least = min(p.abs().min().item() for p in p64)
    floor = max((a.double() - b).abs().max().item() for a, b in zip(sign_points(pre32, f32), p64))
    ok, ext = True, extrema(f64)
    if which == "B":
        ffloor = float((f32.double() - f64).abs().max())
        ok = bool(((f64 > 0) & (f64 < 1)).all()) and min(ext[0], ext[1]) >= MARGIN_REL * ffloor and min(ext[0], ext[1]) > 0
        if f64.shape[0] > 1:
            ok = ok and ext[2] != ext[3]
    return least, floor, ok, ext


def first_start(net, net64, B, H, W, which):
    for start in range(MAX_START + 1):
        i1, i2 = planes(B, H, W, start)
        least, floor, ok, ext = margins(net, net64, i1, i2, which)
        if ok and least >= MARGIN_ABS and least >= MARGIN_REL * floor:
            return start, i1, i2, least, floor, ext
    return None


def map_outputs(net, a, b):
    """The 17 taped maps in Fusion_Network._map_list order, read off the reference's own modules."""
    got = {}
    mods = {"conv1": net.conv1, "conv2": net.conv2, "conv21": net.conv21, "DRDB1": net.DRDB1, "DRDB2": net.DRDB2}
    for d in ("DRDB1", "DRDB2"):
        blk = getattr(net, d)
        for k in range(1, 6):
            mods["%s.Dcov%d" % (d, k)] = getattr(blk, "Dcov%d" % k)
        mods[d + ".conv"] = blk.conv
    handles = [m.register_forward_hook(lambda mod, i, o, k=k: got.__setitem__(k, o.detach().clone())) for k, m in mods.items()]
    fused = net(a, b)
    for h in handles:
        h.remove()
    maps = [net.relu(got["conv1"]).detach()]
    for d in ("DRDB1", "DRDB2"):
        maps += [torch.relu(got["%s.Dcov%d" % (d, k)]) for k in range(1, 6)] + [torch.relu(got[d + ".conv"]), got[d]]
    maps += [net.relu(got["conv2"]).detach(), net.relu(got["conv21"]).detach()]
    assert len(maps) == NMAPS and sum(m.shape[1] for m in maps) == 673
    return fused, maps


def run(net, i1, i2, cot, dtype, with_maps):
    m = copy.deepcopy(net).to(dtype)
    a = i1.to(dtype).clone().requires_grad_(True)
    b = i2.to(dtype).clone().requires_grad_(True)
    fused, maps = map_outputs(m, a, b)
    res = dict(fused=npy(fused))
    if cot is not None:
        (fused * cot.to(dtype)).sum().backward()
        res.update(d_i1=npy(a.grad), d_i2=npy(b.grad))
    if with_maps:
        res["maps"] = [npy(x) for x in maps]
    return res


def block_run(net, x32, cot, dtype):
    blk = copy.deepcopy(net.DRDB1).to(dtype)
    x = x32.to(dtype).clone().requires_grad_(True)
    out = blk(x)
    (out * cot.to(dtype)).sum().backward()
    return npy(out), npy(x.grad)


def drdb_fixtures(Ref):
    scales, stds, neg, clampstats = calibrated(Ref)
    index = {"scales": scales, "shift_B": np.float32(SETS["B"][0]), "last_scale_B": np.float32(SETS["B"][1]), "stats_std": stds,
             "stats_negative_share": neg, "stats_clamp": clampstats}
    nets = {}
    for which in SETS:
        net = loaded(Ref, scales, which)
        nets[which] = net
        net64 = copy.deepcopy(net).double()
        for name, (B, H, W) in list(GRAD_CASES.items()) + (list(FWD_CASES.items()) if which == "A" else []):
            grad = name in GRAD_CASES
            if grad:
                found = first_start(net, net64, B, H, W, which)
                if found is None:
                    raise RuntimeError("%s set %s: no start up to %d meets the margin condition" % (name, which, MAX_START))
                start, i1, i2, least, floor, ext = found
                cot = t(S.make_feature(900 + len(name) + H, (B, 1, H, W)))
            else:
                start, cot = 0, None
                i1, i2 = planes(B, H, W, start)
                least, floor, _, ext = margins(net, net64, i1, i2, which)     # recorded, not a condition: the forward is continuous
            with_maps = which == "A" and name in WITH_MAPS
            r32 = run(net, i1, i2, cot, torch.float32, with_maps)
            r64 = run(net, i1, i2, cot, torch.float64, with_maps)
            print("%-8s set %s %s start %4d  min|sign point| %.2e  fp32 floor %.2e  extremum gaps %.2e %.2e in images %d %d"
                  % (name, which, "gradient" if grad else "forward ", start, least, floor, ext[0], ext[1], ext[2], ext[3]), flush=True)
            index["case_%s_%s" % (name, which)] = np.array([start, least, floor, ext[0], ext[1], ext[2], ext[3]], dtype=np.float64)
            arrays = dict(i1=npy(i1), i2=npy(i2), fused=r32["fused"], fused64=r64["fused"])
            if grad:
                arrays.update(cot=npy(cot), d_i1=r32["d_i1"], d_i2=r32["d_i2"], d_i164=r64["d_i1"], d_i264=r64["d_i2"])
            save("gr_drdb_%s_%s" % (name, which), **arrays)
            if with_maps:
                floors = np.array([np.abs(r32["maps"][k].astype(np.float64) - r64["maps"][k]).max() for k in range(NMAPS)])
                for part, ks in enumerate((range(0, 9), range(9, NMAPS))):
                    save("gr_drdb_%s_maps%d" % (name, part), map_floor=floors, **{"map%d" % k: r64["maps"][k] for k in ks})
                x32 = t(r32["maps"][0])
                cotb = t(S.make_feature(700 + H, (B, 64, H, W)))
                o32, g32 = block_run(net, x32, cotb, torch.float32)
                o64, g64 = block_run(net, x32, cotb, torch.float64)
                save("gr_drdb_%s_block" % name, x=npy(x32), cot=npy(cotb), out=o32, out64=o64, d_x=g32, d_x64=g64)
    save("gr_drdb", **index)
    return nets["A"]


def attack_run(R, m, start):
    """tools/make_golden_u2fusion.py:attack_run with Fusion_Network as the fusion module, on S.make_batch(2, 64, 96, start)."""
    ir, vis, lab = (t(a) for a in S.make_batch(2, 64, 96, start=start))
    torch.manual_seed(1234)
    d0_ir = torch.zeros_like(ir).uniform_(-EPS, EPS)
    d0_vis = torch.zeros_like(vis).uniform_(-EPS, EPS)

    with torch.no_grad():
        fused, seg = m(ir, vis)
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
    tr32 = []
    O.attack_both(lambda a, b: m(a, b), vis, ir, lab, d0_ir, d0_vis, EPS, ALPHA, ITERS, "PGD", trace=tr32)
    assert np.allclose([s["loss"] for s in tr32], losses, rtol=1e-5), ([s["loss"] for s in tr32], losses)
    assert float((torch.sign(tr32[-1]["g_ir"]) != torch.sign(d_ir.grad)).float().mean()) <= 1e-3

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
        arrays, rel, mism = attack_run(R, m, start)
        if rel <= ATTACK_CAP and max(mism) <= ATTACK_CAP:
            break
    else:
        raise RuntimeError("no attack batch up to start %d keeps float32 within %g of float64" % (MAX_START, ATTACK_CAP))
    assert rel <= ATTACK_CAP and max(mism) <= ATTACK_CAP
    save("gr_drdb_attack", **arrays)      # the weights are gr_drdb.npz's scales, set A: no second copy


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref_import.REF_ROOT = os.path.abspath(sys.argv[1])
    R = ref_import.load()
    Ref = R["mfa"].Fusion_Network
    assert os.path.abspath(R["mfa"].__file__).startswith(ref_import.REF_ROOT), R["mfa"].__file__
    torch.set_num_threads(8)
    os.makedirs(OUT, exist_ok=True)
    net = drdb_fixtures(Ref)
    attack_fixture(R, Ref, net)


if __name__ == "__main__":
    main()
