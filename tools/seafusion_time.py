"""SeAFusion baseline: time of one forward and one reverse pass (input gradients) of the kernels of csrc/seafusion.hip beside a torch-eager
restatement of the same arithmetic (torch.nn.functional.conv2d, cat, abs, autograd for the reverse pass) on the same GPU in the same
process.

    python tools/seafusion_time.py [--batch 8] [--height 480] [--width 640] [--iters 20] [--no-eager]

Warm-up, then `iters` launches between two events; prints one JSON line and writes it to profiles/seafusion_time.json (not under
--no-eager: that form is for profiler runs)."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from paif_amd import synthetic as S  # noqa: E402
from paif_amd.fusion_model.seafusion import SeaFusion  # noqa: E402

MACS_PER_PIXEL = sum(k * k * co * ci for _, co, ci, k, _ in S.SEAFUSION_CONVS)      # 166,000


def eager_forward(sd, image_vis, image_ir):
    """The reference's arithmetic (fusion_model/SeaFusion.py:105-125) from torch.nn.functional calls."""
    def cl(name, x):
        return F.leaky_relu(F.conv2d(x, sd[name + ".conv.weight"], sd[name + ".conv.bias"], padding=1), 0.2)

    def rgbd(p, x):
        c = x.shape[1]
        x1 = torch.cat((x, cl(p + ".dense.conv1", x)), 1)
        x1 = torch.cat((x1, cl(p + ".dense.conv2", x1)), 1)
        x1 = F.conv2d(x1, sd[p + ".convdown.conv.weight"], sd[p + ".convdown.conv.bias"])
        g = (F.conv2d(x, sd[p + ".sobelconv.convx.weight"], None, padding=1, groups=c).abs()
             + F.conv2d(x, sd[p + ".sobelconv.convy.weight"], None, padding=1, groups=c).abs())
        return F.leaky_relu(x1 + F.conv2d(g, sd[p + ".convup.conv.weight"], sd[p + ".convup.conv.bias"]), 0.1)

    v = rgbd("vis_rgbd2", rgbd("vis_rgbd1", cl("vis_conv", image_vis[:, :1])))
    i = rgbd("inf_rgbd2", rgbd("inf_rgbd1", cl("inf_conv", image_ir)))
    x = cl("decode2", cl("decode3", cl("decode4", torch.cat((v, i), 1))))
    return torch.tanh(F.conv2d(x, sd["decode1.conv.weight"], sd["decode1.conv.bias"], padding=1)) / 2 + 0.5


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
    torch.manual_seed(0)
    net = SeaFusion().eval().requires_grad_(False).to(dev)
    sd = {k: v.detach() for k, v in net.state_dict().items()}
    gflop = 2e-9 * MACS_PER_PIXEL * a.batch * a.height * a.width
    r = {"tool": "seafusion_time", "device": torch.cuda.get_device_name(0), "batch": a.batch, "height": a.height, "width": a.width, "iters": a.iters,
         "kernel_form": "fp32, 3x3 and 1x1 convs on v_mfma_f32_16x16x4_f32", "forward_gflop": gflop}
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
            r["eager_forward_ms"] = timed(lambda: eager_forward(sd, x1, x2), a.iters)
            r["max_abs_hip_minus_eager"] = float((net(x1, x2) - eager_forward(sd, x1, x2)).abs().max())
    if not a.no_eager:
        def eager_both():
            x, y = x1.clone().requires_grad_(True), x2.clone().requires_grad_(True)
            torch.autograd.grad((eager_forward(sd, x, y) * cot).sum(), [x, y])

        r["eager_forward_plus_reverse_ms"] = timed(eager_both, a.iters)
        r["forward_speedup_vs_eager"] = r["eager_forward_ms"] / r["hip_forward_ms"]
        r["forward_plus_reverse_speedup_vs_eager"] = r["eager_forward_plus_reverse_ms"] / r["hip_forward_plus_reverse_ms"]
        r["not_slower_than_eager"] = bool(r["forward_speedup_vs_eager"] >= 1.0 and r["forward_plus_reverse_speedup_vs_eager"] >= 1.0)
    line = json.dumps(r)
    print(line)
    if not a.no_eager:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "seafusion_time.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
