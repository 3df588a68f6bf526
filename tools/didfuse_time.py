"""DIDFuse baseline: time of one forward and one reverse pass (input gradients) of the kernels of csrc/didfuse.hip beside a torch-eager
restatement of the same arithmetic (F.pad(reflect), conv2d, F.batch_norm(training=False), prelu, cat, autograd for the reverse pass) on
the same GPU in the same process.

    python tools/didfuse_time.py [--batch 8] [--height 480] [--width 640] [--iters 20] [--no-eager]

Warm-up, then `iters` launches between two events; prints one JSON line and writes it to profiles/didfuse_time.json (not under
--no-eager: that form is for profiler runs)."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from paif_amd import synthetic as S  # noqa: E402
from paif_amd.fusion_model.didfuse import DID  # noqa: E402

MACS_PER_PIXEL = sum(9 * co * ci for _, _, co, ci, _ in S.DIDFUSE_CONVS)      # 370,944


def eager_forward(sd, x_over, x_under, eps):
    """The reference's arithmetic (fusion_model/AUIF.py) in .eval() mode from torch.nn.functional calls; eps: BatchNorm prefix -> the
    module's eps."""
    def block(prefix, k, x, act):
        if k == 1:
            x = F.pad(x, (1, 1, 1, 1), mode="reflect")
        x = F.conv2d(x, sd["%s.%d.weight" % (prefix, k)], sd["%s.%d.bias" % (prefix, k)], padding=1 - k)
        bn = "%s.%d." % (prefix, k + 1)
        x = F.batch_norm(x, sd[bn + "running_mean"], sd[bn + "running_var"], sd[bn + "weight"], sd[bn + "bias"], training=False,
                         eps=eps[bn])
        return F.prelu(x, sd["%s.%d.weight" % (prefix, k + 2)]) if act == "prelu" else act(x)

    f = []
    for e, x in (("AE_Encoder1", x_over), ("AE_Encoder2", x_under)):
        f1 = block(e + ".cov1.cov1", 1, x, "prelu")
        f2 = block(e + ".cov2.cov2", 0, f1, "prelu")
        f.append((f1, f2, block(e + ".cov3.cov3", 0, f2, torch.tanh), block(e + ".cov4.cov4", 0, f2, torch.tanh)))
    F1, F2, Fb, Fd = ((a + b) / 2 for a, b in zip(*f))
    o1 = block("AE_Decoder1.cov5.cov5", 0, torch.cat((Fb, Fd), 1), "prelu")
    o2 = block("AE_Decoder1.cov6.cov6", 0, torch.cat((o1, F2), 1), "prelu")
    return block("AE_Decoder1.cov7.cov7", 1, torch.cat((o2, F1), 1), torch.sigmoid)


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-eager", action="store_true", help="the HIP kernels only (profiler runs)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ir, vis, _ = S.make_batch(a.batch, a.height, a.width)
    x1 = torch.from_numpy(ir).to(dev)
    x2 = torch.from_numpy(vis[:, 0:1].copy()).to(dev)
    cot = torch.from_numpy(S.make_feature(5, tuple(x1.shape))).to(dev)
    net = DID().eval()
    # formula weights: BatchNorm entries that are not the identity, the six slopes of the fixtures
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in S.didfuse_state_dict(np.ones(len(S.DIDFUSE_CONVS)), 0.0).items()},
                        strict=True)
    net = net.requires_grad_(False).to(dev)
    eps = {name + ".": m.eps for name, m in net.named_modules() if isinstance(m, torch.nn.BatchNorm2d)}
    sd = {k: v.detach() for k, v in net.state_dict().items()}
    gflop = 2e-9 * MACS_PER_PIXEL * a.batch * a.height * a.width
    r = {"tool": "didfuse_time", "device": torch.cuda.get_device_name(0), "batch": a.batch, "height": a.height, "width": a.width, "iters": a.iters,
         "kernel_form": "fp32, BatchNorm folded, 64- and 128-channel 3x3 convs on v_mfma_f32_16x16x4_f32", "forward_gflop": gflop}
    with torch.no_grad():
        r["hip_forward_ms"] = timed(lambda: net(x1, x2), a.iters)
        r["hip_forward_tflops"] = gflop / r["hip_forward_ms"]
        tape = {}
        net.forward_impl(x1, x2, tape=tape)
        r["hip_reverse_ms"] = timed(lambda: net.backward_impl(cot, tape), a.iters)
        del tape

        def hip_both():
            tp = {}
            net.forward_impl(x1, x2, tape=tp)
            net.backward_impl(cot, tp)

        r["hip_forward_plus_reverse_ms"] = timed(hip_both, a.iters)
        if not a.no_eager:
            r["eager_forward_ms"] = timed(lambda: eager_forward(sd, x1, x2, eps), a.iters)
            r["max_abs_hip_minus_eager"] = float((net(x1, x2) - eager_forward(sd, x1, x2, eps)).abs().max())
    if not a.no_eager:
        def eager_both():
            x, y = x1.clone().requires_grad_(True), x2.clone().requires_grad_(True)
            torch.autograd.grad((eager_forward(sd, x, y, eps) * cot).sum(), [x, y])

        r["eager_forward_plus_reverse_ms"] = timed(eager_both, a.iters)
        r["forward_speedup_vs_eager"] = r["eager_forward_ms"] / r["hip_forward_ms"]
        r["forward_plus_reverse_speedup_vs_eager"] = r["eager_forward_plus_reverse_ms"] / r["hip_forward_plus_reverse_ms"]
        r["not_slower_than_eager"] = bool(r["forward_speedup_vs_eager"] >= 1.0 and r["forward_plus_reverse_speedup_vs_eager"] >= 1.0)
    line = json.dumps(r)
    print(line)
    if not a.no_eager:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "didfuse_time.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
