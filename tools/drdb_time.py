"""The hand-designed fusion network (Fusion_Network over two DRDB): time of one forward and one reverse pass (input gradients) of the
kernels of csrc/drdb.hip beside the torch-eager restatement of the same arithmetic (tests/drdb_eager.py: torch.nn.functional.conv2d, cat,
where, min / max, autograd for the reverse pass) on the same GPU in the same process.

    python tools/drdb_time.py [--batch 8] [--height 480] [--width 640] [--iters 20] [--no-eager]

Warm-up, then `iters` launches between two events (the timing helper of tools/seafusion_time.py); prints one JSON line and writes it to
profiles/drdb_time.json (not under --no-eager: that form is for profiler runs)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from paif_amd import synthetic as S  # noqa: E402
from paif_amd.fusion_model.drdb import Fusion_Network  # noqa: E402
from seafusion_time import timed  # noqa: E402
from tests import drdb_eager as E  # noqa: E402

MACS_PER_PIXEL = sum(k * k * co * ci for _, co, ci, k in S.DRDB_CONVS)      # 417,184
TAPE_FLOATS_PER_PIXEL = 2 * 224 + 2 * 64 + 64 + 32 + 1 + 1                  # two slabs, two r6, f2, c2, f, fused
REVERSE_FLOATS_PER_PIXEL = 2 * 224 + 64 + 32 + 1 + 2                       # two d_slab, d_f2, d_c2, d_f, d_ir and d_vis


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
    net = Fusion_Network().eval().requires_grad_(False).to(dev)
    pixels = a.batch * a.height * a.width
    gflop = 2e-9 * MACS_PER_PIXEL * pixels
    r = {"tool": "drdb_time", "device": torch.cuda.get_device_name(0), "batch": a.batch, "height": a.height, "width": a.width, "iters": a.iters,
         "kernel_form": "fp32, dilation-2 3x3, 3x3 and 1x1 convs on v_mfma_f32_16x16x4_f32", "forward_gflop": gflop,
         "forward_launches": 17, "reverse_launches": 19, "tape_bytes": 4 * TAPE_FLOATS_PER_PIXEL * pixels,
         "reverse_buffer_bytes": 4 * REVERSE_FLOATS_PER_PIXEL * pixels}
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
            r["eager_forward_ms"] = timed(lambda: E.fusion_network(net, x1, x2), a.iters)
            r["max_abs_hip_minus_eager"] = float((net(x1, x2) - E.fusion_network(net, x1, x2)).abs().max())
    if not a.no_eager:
        def eager_both():
            x, y = x1.clone().requires_grad_(True), x2.clone().requires_grad_(True)
            torch.autograd.grad((E.fusion_network(net, x, y) * cot).sum(), [x, y])

        r["eager_forward_plus_reverse_ms"] = timed(eager_both, a.iters)
        r["forward_speedup_vs_eager"] = r["eager_forward_ms"] / r["hip_forward_ms"]
        r["forward_plus_reverse_speedup_vs_eager"] = r["eager_forward_plus_reverse_ms"] / r["hip_forward_plus_reverse_ms"]
        r["not_slower_than_eager"] = bool(r["forward_speedup_vs_eager"] >= 1.0 and r["forward_plus_reverse_speedup_vs_eager"] >= 1.0)
    line = json.dumps(r)
    print(line)
    if not a.no_eager:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "drdb_time.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
