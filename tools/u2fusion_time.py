"""U2Fusion baseline: time of one forward and one reverse pass (input gradients) of the kernels of csrc/u2fusion.hip beside a torch-eager
restatement of the same arithmetic (torch.nn.functional.conv2d, cat, autograd for the reverse pass) on the same GPU in the same process.

    python tools/u2fusion_time.py [--batch 8] [--height 480] [--width 640] [--iters 20] [--no-eager]

Warm-up, then `iters` launches between two events; prints one JSON line and writes it to profiles/u2fusion_time.json (not under
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
from paif_amd.fusion_model.u2fusion import U2Fusion  # noqa: E402

MACS_PER_PIXEL = 9 * sum(co * ci for _, co, ci in S.U2FUSION_CONVS)      # 658,728


def eager_forward(sd, x_over, x_under):
    """The reference's arithmetic (fusion_model/U2Fusion.py:120-125) from torch.nn.functional calls."""
    def conv(name, x):
        return F.conv2d(x, sd[name + ".weight"], sd[name + ".bias"], padding=1)

    x = F.leaky_relu(conv("conv_1.0", torch.cat((x_over, x_under), 1)), 0.2)
    for i in range(5):
        x = torch.cat((x, F.leaky_relu(conv("dense_layers.%d.conv.0" % i, x), 0.2)), 1)
    for i in range(3):
        x = F.leaky_relu(conv("sub.%d.0" % i, x), 0.2)
    return torch.tanh(conv("sub.3", x))


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
    net = U2Fusion().eval().requires_grad_(False).to(dev)
    sd = {k: v.detach() for k, v in net.state_dict().items()}
    gflop = 2e-9 * MACS_PER_PIXEL * a.batch * a.height * a.width
    r = {"tool": "u2fusion_time", "device": torch.cuda.get_device_name(0), "batch": a.batch, "height": a.height, "width": a.width, "iters": a.iters,
         "kernel_form": "fp32, layers 1..8 on v_mfma_f32_16x16x4_f32", "forward_gflop": gflop}
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
        with open(os.path.join(ROOT, "profiles", "u2fusion_time.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
