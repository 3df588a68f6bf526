"""BFFusion baseline: time of one forward and one reverse pass (input gradients) of the kernels of csrc/bffusion.hip beside a torch-eager
restatement of the same arithmetic (tests/bffusion_eager.py: F.pad(reflect), conv2d, F.batch_norm(training=False), max_pool2d,
interpolate, linear, softmax, layer_norm, cat; autograd for the reverse pass) on the same GPU in the same process.

    python tools/bffusion_time.py [--batch 8] [--height 480] [--width 640] [--iters 10] [--no-eager]

Warm-up, then `iters` launches between two events; prints one JSON line and writes it to profiles/bffusion_time.json (not under
--no-eager: that form is for profiler runs).  The line also holds the bytes of the tape and of the reverse pass's gradient buffers."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from paif_amd import synthetic as S  # noqa: E402
from paif_amd.fusion_model.bffusion import BFFR  # noqa: E402
from tests.bffusion_eager import eager  # noqa: E402


def macs(H, W):
    """Multiply-adds of the convs and linears of one image (the attention's reduction and application are not counted)."""
    total = 0
    for name, shape, _, kind, _ in S.BFFUSION_LAYERS:
        if kind in ("stem", "head"):
            level = 0
        elif kind in ("dense",):
            level = int(name[2]) - 1
        elif kind == "dec":
            level = int(name[2]) - 1
        else:
            level = int(name[len("fusion_block")]) - 1
        total += int(np.prod(shape)) * (H >> level) * (W >> level)
    return total


def tensors(x):
    if torch.is_tensor(x):
        return [x]
    if isinstance(x, dict):
        x = list(x.values())
    return [t for y in x for t in tensors(y)] if isinstance(x, (list, tuple)) else []


def timed(fn, iters, warmup=2):
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
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no-eager", action="store_true", help="the HIP kernels only (profiler runs)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ir, vis, _ = S.make_batch(a.batch, a.height, a.width)
    x1 = torch.from_numpy(ir).to(dev)
    x2 = torch.from_numpy(vis[:, 0:1].copy()).to(dev)
    cot = torch.from_numpy(S.make_feature(5, tuple(x1.shape))).to(dev)
    net = BFFR().eval()
    # the fixture weights where they are at hand (calibrated: the attention is neither uniform nor one-hot), else formula weights
    path = os.path.join(ROOT, "tests", "golden", "gb_bffusion.npz")
    scales, shifts = (lambda g: (g["scales"], g["shift"]))(np.load(path)) if os.path.exists(path) else (np.ones(len(S.BFFUSION_LAYERS)), 0.0)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in S.bffusion_state_dict(scales, shifts).items()}, strict=True)
    net = net.requires_grad_(False).to(dev)
    gflop = 2e-9 * macs(a.height, a.width) * a.batch
    r = {"tool": "bffusion_time", "device": torch.cuda.get_device_name(0), "batch": a.batch, "height": a.height, "width": a.width, "iters": a.iters,
         "kernel_form": "fp32, BatchNorm folded, slab convs on v_mfma_f32_16x16x4_f32, context reduction in float64", "forward_gflop": gflop}
    with torch.no_grad():
        r["hip_forward_ms"] = timed(lambda: net(x1, x2), a.iters)
        r["hip_forward_tflops"] = gflop / r["hip_forward_ms"]
        tape = {}
        net.forward_impl(x1, x2, tape=tape)
        r["tape_bytes"] = sum(t.numel() * t.element_size() for t in tensors(tape))
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        net.backward_impl(cot, tape)
        torch.cuda.synchronize()
        r["reverse_peak_extra_bytes"] = torch.cuda.max_memory_allocated() - before      # gradient buffers and the ring map
        r["hip_reverse_ms"] = timed(lambda: net.backward_impl(cot, tape), a.iters)
        del tape

        def hip_both():
            tp = {}
            net.forward_impl(x1, x2, tape=tp)
            net.backward_impl(cot, tp)

        r["hip_forward_plus_reverse_ms"] = timed(hip_both, a.iters)
        if not a.no_eager:
            r["eager_forward_ms"] = timed(lambda: eager(net, x1, x2), a.iters)
            r["max_abs_hip_minus_eager"] = float((net(x1, x2) - eager(net, x1, x2)).abs().max())
    if not a.no_eager:
        def eager_both():
            x, y = x1.clone().requires_grad_(True), x2.clone().requires_grad_(True)
            torch.autograd.grad((eager(net, x, y) * cot).sum(), [x, y])

        r["eager_forward_plus_reverse_ms"] = timed(eager_both, a.iters)
        r["forward_speedup_vs_eager"] = r["eager_forward_ms"] / r["hip_forward_ms"]
        r["forward_plus_reverse_speedup_vs_eager"] = r["eager_forward_plus_reverse_ms"] / r["hip_forward_plus_reverse_ms"]
        r["not_slower_than_eager"] = bool(r["forward_speedup_vs_eager"] >= 1.0 and r["forward_plus_reverse_speedup_vs_eager"] >= 1.0)
    line = json.dumps(r)
    print(line)
    if not a.no_eager:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "bffusion_time.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
