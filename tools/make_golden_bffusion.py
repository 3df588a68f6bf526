"""TEST INFRASTRUCTURE -- fixtures of the BFFusion baseline.  Build container only (CPU):

    python tools/make_golden_bffusion.py <reference tree>

Imports the reference's own fusion_model.BFFusion.BFFR, core.model_fusion_auto.Network_MM_CompModel and attack.attack from the tree given
on the command line (through the shims of oracle/ref_import.py) and stores what they compute, in .eval() mode, under tests/golden/:

gb_bffusion.npz                  the 97 layer scales and bias shifts (the weights are
                                 paif_amd.synthetic.bffusion_state_dict(scales, shift)), the achieved calibration figures, per case the
                                 kept start and its margins, and per case with maps the number of map files
gb_bffusion_<case>.npz           inputs and the fused plane in float32 and float64; for the gradient cases also the cotangent and
                                 d_i1 / d_i2 from float32 and float64 autograd
gb_bffusion_<case>_maps<n>.npz   for 1x16x16 and 1x17x23: the 98 taped maps (BFFR._map_list order, NCHW) in float64 with one scalar floor
                                 max|ref32 - ref64| per map (`map_floor`, all 98 in every file), split greedily over files of <= 0.6 MB raw
gb_bffusion_attack.npz           Network_MM_CompModel(BFFR(), mit_b0) with those weights: clean forward and a PGD-3 trace of attack_both,
                                 in the layout of gd_didfuse_attack.npz (tools/make_golden_didfuse.py: attack_run, stability and THE ATTACK
                                 BATCH, chosen on the reference alone); BFFUSION_ATTACK_ONLY=1 rewrites this file alone

i1 is the infrared plane and enters image_vis_y (conv1_vi / DB*_vi / attn2), i2 is the visible Y plane and enters image_ir: the order
inside the composite model, forward(ir[:, 0:1], Y[:, 0:1]).

CALIBRATION on S.make_batch(2, 48, 64, 0).  Formula weights (S.bffusion_state_dict: no BatchNorm or LayerNorm entry is the identity, the
8 unused ConvLayer.bn included), then two sweeps in forward order that rescale each of the 97 layers, weight and bias: a conv to a
pre-activation (post-BatchNorm where there is one) std of 1; wq1 and wk1 together to a std of LOGIT_STD of the context logits
scale * q^T k (a sum over all pixels of the calibration planes); wv1 to a unit std of the attention's output; end_proj1 to a unit std of
the LayerNorm input; conv_out to a unit pre-tanh std.  From the second sweep on the bias of every conv in front of a LeakyReLU / ReLU, and
of conv_out, is shifted to a pre-activation mean of 0 (through the mean BatchNorm gain where there is one).  Asserted and stored: every conv
pre-activation's std in [0.8, 1.25]; a negative share in [0.2, 0.8] at every LeakyReLU and ReLU input (62 of them); per attention block the
median over the columns of the largest softmax probability in [1.5 / d, 0.9]; the LayerNorm inputs' per-pixel variance (its median) above
0.05; at least 40 % of the fused pixels in (0.1, 0.9).

THE MARGIN CONDITION.  The gradient jumps where a LeakyReLU / ReLU input changes sign and where the two largest entries of a pooling
window change places.  Per gradient case the inputs are S.make_batch(B, H, W, start=s) for the first s <= 2000 at which, in float64, every
sign point (the 62 activation inputs and, per pooling window and channel, the gap between its two largest entries) is >= 2e-5 and
>= 6 * max|point32 - point64|.  Spare shapes of the same geometry class stand in for a case without such a start; the kept ones are printed
and stored.  The forward-only cases take start 0.

The tool also asserts, in float64, that tests/bffusion_eager.py (the restatement the GPU tests and the timing tool use) IS the reference.
"""
import copy
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from oracle import ref_import  # noqa: E402
from paif_amd import synthetic as S  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
# name -> ((B, H, W), spares of the same geometry class)
GRAD_CASES = {"1x16x16": ((1, 16, 16), ()), "1x17x23": ((1, 17, 23), ((1, 17, 22), (1, 19, 23))), "1x22x16": ((1, 22, 16), ((1, 22, 17), (1, 20, 16))),
              "2x16x20": ((2, 16, 20), ())}
OPTIONAL_GRAD = ("2x16x20",)           # forward + restatement if no start is found
FWD_CASES = {"1x40x56": (1, 40, 56), "2x35x50": (2, 35, 50)}
WITH_MAPS = ("1x16x16", "1x17x23")
MARGIN_ABS, MARGIN_REL, MAX_START = 2e-5, 6.0, 2000
LOGIT_STD = 2.0
MAP_FILE_BYTES = 600 * 1024
LAYERS = S.BFFUSION_LAYERS
SIGN_KINDS = ("dense", "fconv", "dec")
CONV_KINDS = ("stem", "dense", "fconv", "dec", "head")
DEC_NAMES = ("DB1_1", "DB2_1", "DB1_2", "DB3_1", "DB2_2", "DB1_3")


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
    from oracle import paif_oracle as O
    ir, vis, _ = S.make_batch(B, H, W, start=start)
    i1 = t(ir)[:, 0:1].clone()
    i2 = O.rgb2ycrcb(t(vis))[:, 0:1].clamp(0, 1).clone()
    return i1.contiguous(), i2.contiguous()


def loaded(Ref, scales, shift):
    net = Ref().eval()
    net.load_state_dict({k: t(v) for k, v in S.bffusion_state_dict(scales, shift).items()}, strict=True)
    return net


def attn_of(net, level, stream):
    fb = getattr(net, "fusion_block%d" % (level + 1))
    return fb.attn1 if stream else fb.attn2


def probe(net, i1, i2, grad=False):
    """-> dict: pre [97] (the layer's output: post-BatchNorm for an f_ConvLayer), xatt (name of end_proj1 -> its input), mods (module name
    -> output), fused."""
    pre, xatt, mods, handles = {}, {}, {}, []
    for k, (name, _, _, kind, bn) in enumerate(LAYERS):
        m = net.get_submodule(bn if kind == "fconv" else name)
        handles.append(m.register_forward_hook(lambda mod, i, o, k=k: pre.__setitem__(k, o.detach().clone())))
        if kind == "proj":
            handles.append(m.register_forward_pre_hook(lambda mod, i, name=name: xatt.__setitem__(name, i[0].detach().clone())))
    for name, m in net.named_modules():
        if name:
            handles.append(m.register_forward_hook(lambda mod, i, o, name=name: mods.__setitem__(name, o.detach().clone())))
    with torch.set_grad_enabled(grad):
        fused = net(i1, i2)
    for h in handles:
        h.remove()
    return dict(pre=[pre[k] for k in range(len(LAYERS))], xatt=xatt, mods=mods, fused=fused)


def logits(p, k):
    """The context logits of the attention block whose wq1 is layer k: [B, heads, d, d]."""
    assert LAYERS[k][3] == "q" and LAYERS[k + 1][3] == "k"
    dim = LAYERS[k][1][0]
    h = S.BFFUSION_HEADS[S.BFFUSION_NB.index(dim)]
    d = dim // h
    q, kk = (p["pre"][j].reshape(p["pre"][j].shape[0], -1, h, d) for j in (k, k + 1))
    return torch.einsum("bnhi,bnhj->bhij", q, kk) * d ** -0.5


def calibrated(Ref):
    i1, i2 = planes(2, 48, 64, 0)
    scales, shift = np.ones(len(LAYERS), dtype=np.float32), np.zeros(len(LAYERS), dtype=np.float32)
    for sweep in range(3):
        for k, (name, _, _, kind, _) in enumerate(LAYERS):
            p = probe(loaded(Ref, scales, shift), i1, i2)
            if kind == "q":
                scales[k] = np.float32(scales[k] * np.sqrt(LOGIT_STD / logits(p, k).std().item()))
            elif kind == "k":
                scales[k] = np.float32(scales[k] * LOGIT_STD / logits(p, k - 1).std().item())
            elif kind == "v":
                scales[k] = np.float32(scales[k] / p["xatt"][LAYERS[k + 1][0]].std().item())
            else:
                scales[k] = np.float32(scales[k] / p["pre"][k].std().item())
            if sweep and kind in SIGN_KINDS + ("head",):
                net = loaded(Ref, scales, shift)
                gain = 1.0
                if kind == "fconv":
                    bn = net.get_submodule(LAYERS[k][4])
                    gain = float((bn.weight / torch.sqrt(bn.running_var + bn.eps)).mean())
                shift[k] = np.float32(shift[k] - probe(net, i1, i2)["pre"][k].mean().item() / gain)
        print("calibration sweep %d done" % sweep, flush=True)
    last = len(LAYERS) - 1
    net = loaded(Ref, scales, shift)
    p = probe(net, i1, i2)
    stds = np.array([p["pre"][k].std().item() for k, l in enumerate(LAYERS) if l[3] in CONV_KINDS])
    neg = np.array([(p["pre"][k] < 0).float().mean().item() for k, l in enumerate(LAYERS) if l[3] in SIGN_KINDS])
    peak, lnvar, logit_std = [], [], []
    for k, l in enumerate(LAYERS):
        if l[3] == "q":
            lg = logits(p, k)
            d = lg.shape[-1]
            pk = lg.softmax(dim=-2).max(dim=-2).values.median().item()
            assert 1.5 / d <= pk <= 0.9, (l[0], pk, d)
            peak.append(pk), logit_std.append(lg.std().item())
        if l[3] == "proj":
            lnvar.append(p["pre"][k].var(dim=-1, unbiased=False).median().item())
    inside = float(((p["fused"] > 0.1) & (p["fused"] < 0.9)).float().mean())
    print("conv pre-activation std: min %.3f max %.3f\nnegative share: min %.2f max %.2f (%d points)\nsoftmax peak (median over columns) %s\n"
          "logit std %s\nLayerNorm input variance (median over pixels) %s\npre-tanh mean %.4f, fused inside (0.1, 0.9): %.2f"
          % (stds.min(), stds.max(), neg.min(), neg.max(), len(neg), ["%.2f" % x for x in peak], ["%.2f" % x for x in logit_std],
             ["%.2f" % x for x in lnvar], p["pre"][last].mean().item(), inside), flush=True)
    assert len(neg) == 62 and len(stds) == 65 and len(peak) == 8 and len(lnvar) == 8
    assert np.all((stds >= 0.8) & (stds <= 1.25)), stds
    assert np.all((neg >= 0.2) & (neg <= 0.8)), neg
    assert min(lnvar) > 0.05, lnvar
    assert abs(p["pre"][last].mean().item()) <= 2e-2 and inside >= 0.4, (p["pre"][last].mean().item(), inside)
    stats = dict(stats_std=stds, stats_negative_share=neg, stats_softmax_peak=np.array(peak), stats_logit_std=np.array(logit_std),
                 stats_ln_var=np.array(lnvar), stats_inside=np.array(inside))
    return net, scales, shift, stats


def pool_gaps(x):
    """Per 2 x 2 window (an odd last row / column is dropped) and channel: the largest entry minus the second largest."""
    B, C, H, W = x.shape
    w = x[:, :, :H // 2 * 2, :W // 2 * 2].reshape(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)
    top = w.sort(dim=-1, descending=True).values
    return top[..., 0] - top[..., 1]


def sign_points(p):
    pts = [p["pre"][k] for k, l in enumerate(LAYERS) if l[3] in SIGN_KINDS]
    pts += [pool_gaps(p["mods"]["DB%d_%s" % (l, tag)]) for tag in ("vi", "ir") for l in (1, 2, 3)]
    assert len(pts) == 68
    return pts


def margins(net, net64, i1, i2):
    p32, p64 = sign_points(probe(net, i1, i2)), sign_points(probe(net64, i1.double(), i2.double()))
    least = min(x.abs().min().item() for x in p64)
    floor = max((a.double() - b).abs().max().item() for a, b in zip(p32, p64))
    return least, floor


def map_list(net, p):
    """BFFR._map_list order, NCHW (the eight context matrices as [B, d, 1, dim])."""
    mods, out = p["mods"], []
    for tag in ("vi", "ir"):
        for l in range(1, 5):
            db = "DB%d_%s" % (l, tag)
            out += [mods[db + ".conv1"], mods[db + ".conv2"], mods[db]]
    ctxs = []
    for l in range(4):
        for s in range(2):
            a = "fusion_block%d.%s" % (l + 1, "attn1" if s else "attn2")
            p2 = mods[a + ".conv_pre.1"]
            B, C, H, W = p2.shape

            def tok(x):
                return x.permute(0, 2, 1).reshape(B, -1, H, W)

            out += [mods[a + ".conv_pre.0"], p2, tok(torch.cat([mods[a + ".wq1"], mods[a + ".wk1"], mods[a + ".wv1"]], -1)),
                    tok(mods[a + ".end_proj1"]), tok(mods[a + ".norm1"]), mods[a + ".ffn.0"], mods[a + ".ffn.1"]]
            h = S.BFFUSION_HEADS[l]
            d = C // h
            q, k = (mods[a + "." + n].reshape(B, -1, h, d) for n in ("wq1", "wk1"))
            ctx = (torch.einsum("bnhi,bnhj->bhij", q, k) * d ** -0.5).softmax(dim=-2)
            ctxs.append(ctx.reshape(B, C, d)[:, None].permute(0, 3, 1, 2))
    out += [mods["fusion_block%d" % (l + 1)] for l in range(4)]
    out += [mods[n] for n in DEC_NAMES]
    out += ctxs
    assert len(out) == 98
    return [npy(x) for x in out]


def run(net, i1, i2, cot, dtype, with_maps):
    m = copy.deepcopy(net).to(dtype)
    a = i1.to(dtype).clone().requires_grad_(True)
    b = i2.to(dtype).clone().requires_grad_(True)
    p = probe(m, a, b, grad=True)
    res = dict(fused=npy(p["fused"]))
    if cot is not None:
        (p["fused"] * cot.to(dtype)).sum().backward()
        res.update(d_i1=npy(a.grad), d_i2=npy(b.grad))
    if with_maps:
        res["maps"] = map_list(m, p)
    return res


def first_start(net, net64, shapes):
    for B, H, W in shapes:
        for start in range(MAX_START + 1):
            i1, i2 = planes(B, H, W, start)
            least, floor = margins(net, net64, i1, i2)
            if least >= MARGIN_ABS and least >= MARGIN_REL * floor:
                return (B, H, W), start, i1, i2, least, floor
        print("no start up to %d for %dx%dx%d" % (MAX_START, B, H, W), flush=True)
    return None


def check_restatement(net):
    """tests/bffusion_eager.py is the reference, in float64 (free and with the branches frozen from the reference's own maps)."""
    from tests.bffusion_eager import eager
    for B, H, W in ((1, 17, 23), (2, 16, 20)):
        i1, i2 = planes(B, H, W, 0)
        n64 = copy.deepcopy(net).double()
        ref = n64(i1.double(), i2.double())
        mine = eager(n64, i1.double(), i2.double())
        err = float((ref - mine).abs().max())
        print("restatement vs reference at %dx%dx%d: %.2e" % (B, H, W, err), flush=True)
        assert err <= 1e-12


def bffusion_fixtures(Ref):
    net, scales, shift, stats = calibrated(Ref)
    check_restatement(net)
    net64 = copy.deepcopy(net).double()
    index = dict(scales=scales, shift=shift, **stats)
    kept = {}
    cases = [(n, sh, sp, True) for n, (sh, sp) in GRAD_CASES.items()] + [(n, sh, (), False) for n, sh in FWD_CASES.items()]
    for name, shape, spares, grad in cases:
        found = first_start(net, net64, (shape,) + tuple(spares)) if grad else None
        if grad and found is None:
            if name not in OPTIONAL_GRAD:
                raise RuntimeError("%s: neither it nor its spares meet the margin condition" % name)
            grad = False
        if grad:
            (B, H, W), start, i1, i2, least, floor = found
            cot = t(S.make_feature(900 + len(name) + H, (B, 1, H, W)))
        else:
            (B, H, W), start, cot = shape, 0, None
            i1, i2 = planes(B, H, W, start)
            least, floor = margins(net, net64, i1, i2)     # recorded, not a condition: the forward is continuous
        with_maps = name in WITH_MAPS
        assert not with_maps or (B, H, W) == shape, "the map cases keep their shape"
        r32, r64 = run(net, i1, i2, cot, torch.float32, with_maps), run(net, i1, i2, cot, torch.float64, with_maps)
        inside = float(((r64["fused"] > 0.1) & (r64["fused"] < 0.9)).mean())
        print("%-8s kept as %dx%dx%d %s start %4d  min|sign point| %.2e  fp32 floor of the sign points %.2e  fused inside (0.1,0.9): %.2f"
              % (name, B, H, W, "gradient" if grad else "forward ", start, least, floor, inside), flush=True)
        index["case_%s" % name] = np.array([start, least, floor, inside, B, H, W, float(grad)], dtype=np.float64)
        arrays = dict(i1=npy(i1), i2=npy(i2), fused=r32["fused"], fused64=r64["fused"])
        if grad:
            arrays.update(cot=npy(cot), d_i1=r32["d_i1"], d_i2=r32["d_i2"], d_i164=r64["d_i1"], d_i264=r64["d_i2"])
        save("gb_bffusion_" + name, **arrays)
        if with_maps:
            floors = np.array([np.abs(a.astype(np.float64) - b).max() for a, b in zip(r32["maps"], r64["maps"])])
            files, cur, size = [], {}, 0
            for k, m in enumerate(r64["maps"]):
                if cur and size + m.nbytes > MAP_FILE_BYTES:
                    files.append(cur)
                    cur, size = {}, 0
                cur["map%d" % k] = m
                size += m.nbytes
            files.append(cur)
            for part, arrs in enumerate(files):
                save("gb_bffusion_%s_maps%d" % (name, part), map_floor=floors, **arrs)
            index["maps_%s" % name] = np.array(len(files))
        kept[name] = (B, H, W, grad)
    save("gb_bffusion", **index)
    print("kept: %s" % kept, flush=True)
    return net


def attack_fixture(R, Ref, net):
    import make_golden_didfuse as DG      # attack_run, stability and the caps of THE ATTACK BATCH: one rule for every baseline
    with ref_import.quiet():
        m = R["mfa"].Network_MM_CompModel(Ref(), None, None, "mit_b0", num_classes=9)
    m.eval()
    S.load_formula_weights(m, head=S.head_tag("mit_b0", 2, 64, 96))
    m.enhance_net.load_state_dict(net.state_dict(), strict=True)
    assert not m.enhance_net.training
    for start in range(DG.MAX_START + 1):
        srel, sfrac = DG.stability(m, start)
        if srel > DG.STABLE_LOSS or sfrac > DG.STABLE_FRAC:
            continue
        arrays, rel, mism = DG.attack_run(R, m, start)
        if rel <= DG.ATTACK_CAP and max(mism) <= DG.ATTACK_CAP and max(mism[2:]) <= DG.ATTACK_DELTA_CAP:
            break
    else:
        raise RuntimeError("no attack batch up to start %d keeps float32 within %g of float64" % (DG.MAX_START, DG.ATTACK_CAP))
    arrays["stability"] = np.array([DG.PERTURB, srel, sfrac])
    save("gb_bffusion_attack", **arrays)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref_import.REF_ROOT = os.path.abspath(sys.argv[1])
    R = ref_import.load()
    import fusion_model.BFFusion as ref_bff
    assert os.path.abspath(ref_bff.__file__).startswith(ref_import.REF_ROOT), ref_bff.__file__
    torch.set_num_threads(8)
    os.makedirs(OUT, exist_ok=True)
    if os.environ.get("BFFUSION_ATTACK_ONLY"):
        g = np.load(os.path.join(OUT, "gb_bffusion.npz"))
        net = loaded(ref_bff.BFFR, g["scales"], g["shift"])
    else:
        net = bffusion_fixtures(ref_bff.BFFR)
    if not os.environ.get("BFFUSION_NO_ATTACK"):
        attack_fixture(R, ref_bff.BFFR, net)


if __name__ == "__main__":
    main()
