"""TEST INFRASTRUCTURE -- fixtures of the ReCoNet baseline.  Build container only (CPU):

    python tools/make_golden_reconet.py <reference tree>

Imports the reference's own fusion_model.Reconet.ReCoNet, core.model_fusion_auto.Network_MM_CompModel and attack.attack from the tree
given on the command line (through the shims of oracle/ref_import.py) and stores what they compute under tests/golden/:

gr_reconet.npz            the three configurations' weights, the inputs, the cotangents, the achieved calibration figures
gr_reconet_<cfg>_<case>_<init>.npz
                          the reference's show_detail outputs (every i_f, att_a, att_b) in float32 and float64, and d_i1 / d_i2 for the
                          fixed cotangent on the last i_f from float32 and from float64 autograd (one file per combination: a committed
                          file stays under 1 MiB)
gr_reconet_attack.npz     Network_MM_CompModel(ReCoNet(3, 16, False), mit_b0): clean forward and a PGD-3 trace of attack_both, in the
                          layout of gg_attack_PGD, float32 and float64

The default initialisation is useless as a test (outputs within [-0.02, 0.15], every sigmoid ~ 0.5, tanh and GELU in their linear
range), so the drawn weights are rescaled until, on the fixture's own inputs, the pre-GELU and the pre-tanh values have a standard
deviation of about 1 and both attention maps span at least [0.2, 0.8]; the three conditions are asserted and the figures stored.
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
CONFIGS = {"d3c16": (3, 16, False), "d2c16bn": (2, 16, True), "d3c64": (3, 64, False)}
CASES = {"2x48x64": (2, 48, 64), "1x37x53": (1, 37, 53), "1x4x5": (1, 4, 5)}
INITS = ("max", "mean")
EPS, ALPHA, ITERS = 8 / 255.0, 2 / 255.0, 3


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def npy(x):
    return x.detach().cpu().numpy()


def save(name, **arrays):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    print("wrote %-40s %8.1f KB" % (name + ".npz", size / 1024))
    assert size < (1 << 20), "a committed file stays under 1 MiB"


def make_inputs():
    """i_1 = infrared, i_2 = visible Y of the synthetic pairs, in [0,1].  In the 2x48x64 case the second sample has i_2 = i_1 on the
    left half of the image: with init_f='max' every max of the network then ties there, so both tie rules carry gradient."""
    out = {}
    for ci, (name, (B, H, W)) in enumerate(CASES.items()):
        ir, vis, _ = S.make_batch(B, H, W, start=10 * ci)
        i1 = t(ir)[:, 0:1].clone()
        i2 = O.rgb2ycrcb(t(vis))[:, 0:1].clamp(0, 1).clone()
        if name == "2x48x64":
            i2[1, :, :, : W // 2] = i1[1, :, :, : W // 2]
        out[name] = (i1.contiguous(), i2.contiguous())
    return out


class Probe:
    """Forward hooks on the reference module: pre-GELU values, pre-tanh values, the attention maps."""

    def __init__(self, net):
        self.z, self.y, self.att = [], [], []
        self.handles = [cg.group[1].register_forward_hook(lambda m, i, o: self.z.append(o.detach())) for cg in net.decoder.conv_d]
        self.handles.append(net.decoder.conv_s[0].register_forward_hook(lambda m, i, o: self.y.append(o.detach())))

    def run(self, net, inputs):
        self.z, self.y, self.att = [], [], []
        with torch.no_grad():
            for i1, i2 in inputs.values():
                for init in INITS:
                    _, a, b = net(i1, i2, init_f=init, show_detail=True)
                    self.att += [(x.min().item(), x.max().item()) for x in a + b]
        cat = lambda xs: torch.cat([x.reshape(-1) for x in xs])
        depth = net.depth
        zs = [cat(self.z[g::3]).std().item() for g in range(3)]
        return zs, cat(self.y).std().item(), min(a for a, _ in self.att), max(b for _, b in self.att), depth

    def close(self):
        for h in self.handles:
            h.remove()


def calibrated(Ref, key, inputs):
    depth, dim, use_bn = CONFIGS[key]
    torch.manual_seed(20240 + len(key) * 7 + dim)
    net = Ref(depth, dim, use_bn).eval()
    gen = torch.Generator().manual_seed(77 + dim)
    if use_bn:   # away from the defaults, so that folding is tested
        for cg in net.decoder.conv_d:
            bn = cg.group[1]
            with torch.no_grad():
                bn.running_mean.copy_(0.3 * torch.randn(dim, generator=gen))
                bn.running_var.copy_(0.5 + 1.5 * torch.rand(dim, generator=gen))
                bn.weight.copy_(0.5 + torch.rand(dim, generator=gen))
                bn.bias.copy_(0.3 * torch.randn(dim, generator=gen))
    probe = Probe(net)
    for _ in range(12):
        zs, ys, amin, amax, _ = probe.run(net, inputs)
        with torch.no_grad():
            for g, cg in enumerate(net.decoder.conv_d):
                if use_bn:   # the value GELU sees is the BatchNorm's output
                    cg.group[1].weight.mul_(1.0 / zs[g]), cg.group[1].bias.mul_(1.0 / zs[g])
                else:
                    cg.group[0].weight.mul_(1.0 / zs[g]), cg.group[0].bias.mul_(1.0 / zs[g])
            cs = net.decoder.conv_s[0]
            cs.weight.mul_(1.0 / ys), cs.bias.mul_(1.0 / ys)
            if amin > 0.18 or amax < 0.82:
                net.att_a_conv.weight.mul_(1.5), net.att_b_conv.weight.mul_(1.5)
    zs, ys, amin, amax, _ = probe.run(net, inputs)
    probe.close()
    assert all(0.8 <= z <= 1.25 for z in zs), zs
    assert 0.8 <= ys <= 1.25, ys
    assert amin <= 0.2 and amax >= 0.8, (amin, amax)
    print("%-8s pre-GELU std %s  pre-tanh std %.3f  attention in [%.3f, %.3f]" % (key, ["%.3f" % z for z in zs], ys, amin, amax))
    return net, np.array(zs + [ys, amin, amax], dtype=np.float64)


def detail_and_grads(net, i1, i2, init, cot, dtype):
    m = copy.deepcopy(net).to(dtype)
    a = i1.to(dtype).clone().requires_grad_(True)
    b = i2.to(dtype).clone().requires_grad_(True)
    fs, aa, ab = m(a, b, init_f=init, show_detail=True)
    (fs[-1] * cot.to(dtype)).sum().backward()
    det = lambda xs: np.stack([npy(x) for x in xs])
    return dict(i_f=det(fs), att_a=det(aa), att_b=det(ab), d_i1=npy(a.grad), d_i2=npy(b.grad))


def reconet_fixtures(Ref):
    inputs = make_inputs()
    index = {}
    for name, (i1, i2) in inputs.items():
        index["i1_" + name], index["i2_" + name] = npy(i1), npy(i2)
        index["cot_" + name] = S.make_feature(900 + len(name) + i1.shape[2], tuple(i1.shape))
    nets = {}
    for key in CONFIGS:
        net, stats = calibrated(Ref, key, inputs)
        nets[key] = net
        index["stats_" + key] = stats   # pre-GELU std per dilation, pre-tanh std, attention min, attention max
        for k, v in net.state_dict().items():
            index["sd_%s/%s" % (key, k)] = npy(v)
        for name, (i1, i2) in inputs.items():
            for init in INITS:
                cot = t(index["cot_" + name])
                r32 = detail_and_grads(net, i1, i2, init, cot, torch.float32)
                r64 = detail_and_grads(net, i1, i2, init, cot, torch.float64)
                arrays = {k: v for k, v in r32.items()}
                arrays.update({k + "64": v for k, v in r64.items()})
                save("gr_reconet_%s_%s_%s" % (key, name, init), **arrays)
    save("gr_reconet", **index)
    return nets


def attack_fixture(R, Ref, net16):
    with ref_import.quiet():
        m = R["mfa"].Network_MM_CompModel(Ref(3, 16, False), None, None, "mit_b0", num_classes=9)
    m.eval()
    S.load_formula_weights(m, head=S.head_tag("mit_b0", 2, 64, 96))
    m.enhance_net.load_state_dict(net16.state_dict(), strict=True)
    ir, vis, lab = (t(a) for a in S.make_batch(2, 64, 96))
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

    # float64: the reference's ReCoNet in double between the restated colour glue and segmentation network (the reference's own
    # colour transform builds float32 constants), from the SAME float32 delta0
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in m.state_dict().items()}
    rec64 = copy.deepcopy(m.enhance_net).double()

    def fwd64(a, b):
        ycc = O.rgb2ycrcb(b)
        fz = rec64(a[:, 0:1], ycc[:, 0:1])
        return fz, O.wetr_forward(O.seg_input_from_fused(fz, ycc), sd64, "denoise_net.", "mit_b0")

    with torch.no_grad():
        fused64, seg64 = fwd64(ir.double(), vis.double())
    assert float((fused64 - fused.double()).abs().max()) <= 1e-5, "the float64 composition must be the float32 model's"
    tr64 = []
    O.attack_both(fwd64, vis.double(), ir.double(), lab, d0_ir.double(), d0_vis.double(), EPS, ALPHA, ITERS, "PGD", trace=tr64)
    up = torch.nn.functional.interpolate(seg, size=lab.shape[1:], mode="bilinear", align_corners=False)
    pred = up.argmax(1).numpy()
    arrays = dict(fused=npy(fused), logits=npy(seg), fused64=npy(fused64), logits64=npy(seg64), pred=pred.astype(np.uint8),
                  conf=O.confusion_matrix(lab.numpy(), pred),
                  d0_ir=npy(d0_ir), d0_vis=npy(d0_vis), delta_ir=npy(d_ir), delta_vis=npy(d_vis),
                  gsum_ir=npy(d_ir.grad), gsum_vis=npy(d_vis.grad), losses=np.array(losses),
                  gsum_ir64=npy(tr64[-1]["g_ir"]).astype(np.float32), gsum_vis64=npy(tr64[-1]["g_vis"]).astype(np.float32),
                  losses64=np.array([s["loss"] for s in tr64]))
    for k, v in net16.state_dict().items():
        arrays["sd/" + k] = npy(v)
    print("attack losses %s (float64 %s), classes in the clean map: %s" % (losses, arrays["losses64"], np.bincount(pred.ravel(), minlength=9)))
    save("gr_reconet_attack", **arrays)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref_import.REF_ROOT = os.path.abspath(sys.argv[1])
    R = ref_import.load()
    import fusion_model.Reconet as ref_reconet
    assert os.path.abspath(ref_reconet.__file__).startswith(ref_import.REF_ROOT), ref_reconet.__file__
    torch.set_num_threads(8)
    os.makedirs(OUT, exist_ok=True)
    nets = reconet_fixtures(ref_reconet.ReCoNet)
    attack_fixture(R, ref_reconet.ReCoNet, nets["d3c16"])


if __name__ == "__main__":
    main()
