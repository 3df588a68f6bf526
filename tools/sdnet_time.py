"""SDNet baseline: time of one forward and one reverse pass (input gradients) of the kernels of csrc/sdnet.hip beside a torch-eager
restatement of the same arithmetic (torch.nn.functional calls, autograd for the reverse pass) on the same GPU in the same process.

    python tools/sdnet_time.py [--batch 8] [--height 480] [--width 640] [--iters 20] [--no-eager]

Warm-up, then `iters` launches between two events; prints one JSON line."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from paif_amd import synthetic as S  # noqa: E402
from paif_amd.fusion_model.sdnet import SDNet  # noqa: E402

MACS_PER_PIXEL = 2 * (25 * 16 + 9 * 16 * 16 * (1 + 2 + 3)) + 128      # both encoders and the fuse: 28.6 k


def eager_forward(sd, x1, x2):
    """The reference's arithmetic (fusion_model/SDNet.py:33-47) from torch.nn.functional calls."""
    def conv(name, x, pad):
        return F.leaky_relu(F.conv2d(x, sd[name + ".0.weight"], sd[name + ".0.bias"], padding=pad))

    maps = []
    for e, x in (("1", x1), ("2", x2)):
        a = conv("conv1" + e, x, 2)
        b = conv("conv2" + e, a, 1)
        c = conv("conv3" + e, torch.cat([a, b], 1), 1)
        d = conv("conv4" + e, torch.cat([a, b, c], 1), 1)
        maps += [a, b, c, d]
    return torch.tanh(F.conv2d(torch.cat(maps, 1), sd["fuse.0.weight"], sd["fuse.0.bias"]))


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
    net = SDNet().eval().requires_grad_(False).to(dev)
    sd = {k: v.detach() for k, v in net.state_dict().items()}
    gflop = 2e-9 * MACS_PER_PIXEL * a.batch * a.height * a.width
    r = {"tool": "sdnet_time", "device": torch.cuda.get_device_name(0), "batch": a.batch, "height": a.height, "width": a.width, "iters": a.iters,
         "kernel_form": "fp32, dense convs on v_mfma_f32_16x16x4_f32", "forward_gflop": gflop}
    with torch.no_grad():
        r["hip_forward_ms"] = timed(lambda: net(x1, x2), a.iters)
        r["hip_forward_tflops"] = gflop / r["hip_forward_ms"]
        tape = {}
        net.forward_impl(x1, x2, tape=tape)
        r["hip_reverse_ms"] = timed(lambda: net.backward_impl(cot, tape), a.iters)
        del tape
        if not a.no_eager:
            r["eager_forward_ms"] = timed(lambda: eager_forward(sd, x1, x2), a.iters)
            r["max_abs_hip_minus_eager"] = float((net(x1, x2) - eager_forward(sd, x1, x2)).abs().max())
    if not a.no_eager:
        def eager_both():
            x, y = x1.clone().requires_grad_(True), x2.clone().requires_grad_(True)
            torch.autograd.grad((eager_forward(sd, x, y) * cot).sum(), [x, y])

        def hip_both():
            tp = {}
            with torch.no_grad():
                net.forward_impl(x1, x2, tape=tp)
                net.backward_impl(cot, tp)

        r["eager_forward_plus_reverse_ms"] = timed(eager_both, max(3, a.iters // 4), warmup=2)
        r["hip_forward_plus_reverse_ms"] = timed(hip_both, a.iters)
        r["forward_speedup_vs_eager"] = r["eager_forward_ms"] / r["hip_forward_ms"]
        r["forward_plus_reverse_speedup_vs_eager"] = r["eager_forward_plus_reverse_ms"] / r["hip_forward_plus_reverse_ms"]
    print(json.dumps(r))


if __name__ == "__main__":
    main()
