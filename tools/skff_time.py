"""Timing of SKFF and Fusion_Network2 on the GPU at B = 8, 480x640: SKFF alone (height 2 and 3, channel-last maps: ops.skff_forward_nhwc /
ops.skff_backward_nhwc, three launches each way) and the whole network (ops.fn2_forward / ops.fn2_backward), forward and
forward + reverse, beside the torch-eager restatement (tests/skff_eager.py), and a 630 MB device copy as the HBM yardstick of
tools/hbm_rates.py.

    python tools/skff_time.py [--batch 8] [--size 480x640] [--steps skff2_fwd,...] [--repeats 5] [--step-timeout 300] [--json out.json]

Method: fence-less HIP events on the launch stream (ops.KernelTimer) around one call, one warm-up run, then the median of --repeats
runs: the times include the host's launch work where the GPU waits for it (HOST-INCLUSIVE).  Every step runs in a child process of its
own under its own time limit; the first step that fails, faults or runs out of time ends the whole script -- nothing more is started on
the GPU after it.

Bytes are derived, not measured: per launch what it MUST move (each input map read once, each output map written once; the gate's
partials and parameters are a few KB).  With M = 4 B H W 64 bytes, one 64-channel map, and n inputs: pool reads n M; gate ~0; apply reads
n M and writes M; reduce reads (n + 1) M; gate-reverse ~0; apply-reverse reads M and writes n M."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = ("copy", "skff2_fwd", "skff2_fwdbwd", "skff3_fwd", "skff3_fwdbwd", "fn2_fwd", "fn2_fwdbwd", "eager_skff2_fwd", "eager_skff2_fwdbwd",
         "eager_fn2_fwd", "eager_fn2_fwdbwd")


def launch_bytes(n, B, H, W):
    """-> [(launch, bytes it must move)] of one SKFF forward and reverse with n inputs."""
    M = 4 * B * H * W * 64
    return [("pool", n * M), ("gate", 0), ("apply", (n + 1) * M), ("reduce", (n + 1) * M), ("gate-reverse", 0), ("apply-reverse", (n + 1) * M)]


def _timed(fn, repeats):
    import torch
    from paif_amd import ops

    tm = ops.KernelTimer(lambda tag: False)
    fn()
    torch.cuda.synchronize()
    pairs = []
    for _ in range(repeats):
        e0 = tm.mark()
        fn()
        pairs.append((e0, tm.mark()))
    torch.cuda.synchronize()
    return statistics.median(tm.elapsed_ms(a, b) for a, b in pairs)


def run_step(step, B, H, W, repeats):
    import torch
    from paif_amd import ops
    from paif_amd.core.model_fusion_auto import SKFF, Fusion_Network2
    from tests import skff_eager as E

    dev = torch.device("cuda:0")
    torch.manual_seed(5)
    res = {"step": step, "B": B, "H": H, "W": W}
    eager = step.startswith("eager_")
    name = step[6:] if eager else step
    if name == "copy":
        a = torch.empty(630 * 1000000 // 4, device=dev)
        b = torch.empty_like(a)
        res["ms"] = _timed(lambda: b.copy_(a), repeats)
        res["bytes"] = 2 * a.numel() * 4
    elif name.startswith("skff"):
        n = int(name[4])
        m = SKFF(64, n).eval().requires_grad_(False).to(dev)
        by = launch_bytes(n, B, H, W)
        both = name.endswith("fwdbwd")
        res["launch_bytes"] = by if both else by[:3]
        res["bytes"] = sum(v for _, v in res["launch_bytes"])
        if eager:
            xs = [torch.randn(B, 64, H, W, device=dev) for _ in range(n)]
            cot = torch.randn(B, 64, H, W, device=dev)
            if both:
                def fn():
                    leaves = [x.clone().requires_grad_(True) for x in xs]      # (the clones are part of the eager figure: n M read + written)
                    (E.skff(m, leaves) * cot).sum().backward()
            else:
                def fn():
                    with torch.no_grad():
                        E.skff(m, xs)
        else:
            xs = [torch.randn(B, H, W, 64, device=dev) for _ in range(n)]
            cot = torch.randn(B, H, W, 64, device=dev)
            pack = m._pack()
            if both:
                def fn():
                    tape, _ = ops.skff_forward_nhwc(xs, pack)
                    ops.skff_backward_nhwc(xs, tape, cot, pack)
            else:
                def fn():
                    ops.skff_forward_nhwc(xs, pack)
        res["ms"] = _timed(fn, repeats)
    elif name.startswith("fn2"):
        net = Fusion_Network2().eval().requires_grad_(False).to(dev)
        ins = [torch.rand(B, 1, H, W, device=dev), torch.rand(B, 1, H, W, device=dev), torch.randn(B, 64, H, W, device=dev),
               torch.randn(B, 128, H, W, device=dev)]
        cot = torch.randn(B, 1, H, W, device=dev)
        both = name.endswith("fwdbwd")
        if eager and both:
            def fn():
                leaves = [x.clone().requires_grad_(True) for x in ins]
                (E.fusion_network2(net, *leaves) * cot).sum().backward()
        elif eager:
            def fn():
                with torch.no_grad():
                    E.fusion_network2(net, *ins)
        elif both:
            def fn():
                with torch.no_grad():
                    tape = {}
                    net._run(*ins, tape)
                    net._reverse(cot, tape)
        else:
            def fn():
                with torch.no_grad():
                    net(*ins)
        res["ms"] = _timed(fn, repeats)
    else:
        raise SystemExit("unknown step " + step)
    if "bytes" in res:
        res["tb_per_s"] = res["bytes"] / res["ms"] / 1e9
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", default="480x640")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--json", default=None)
    ap.add_argument("--steps", default=",".join(STEPS), help="which of %s to run" % (STEPS,))
    ap.add_argument("--step", default=None, help="(internal) run one step in this process")
    a = ap.parse_args()
    H, W = (int(v) for v in a.size.split("x"))
    if a.step:
        return run_step(a.step, a.batch, H, W, a.repeats)
    for n in (2, 3):
        print("SKFF, %d inputs, B = %d, %dx%d: bytes each launch must move: %s" % (
            n, a.batch, H, W, ", ".join("%s %.0f MB" % (k, v / 1e6) for k, v in launch_bytes(n, a.batch, H, W))), flush=True)
    results = []
    for st in a.steps.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", st, "--batch", str(a.batch), "--size", a.size, "--repeats", str(a.repeats)]
        try:
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            results.append({"step": st, "did_not_finish_within_s": a.step_timeout})
            print("%s: did not finish within %d s -- stopping" % (st, a.step_timeout), flush=True)
            break
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
        if out.returncode != 0 or not line:
            print("%s failed (exit %d) -- stopping\n%s" % (st, out.returncode, out.stderr[-2000:]), flush=True)
            results.append({"step": st, "failed": out.returncode})
            break
        r = json.loads(line[0][7:])
        results.append(r)
        print("%-20s %10.3f ms" % (st, r["ms"]) + (("  %6.0f MB  %5.2f TB/s" % (r["bytes"] / 1e6, r["tb_per_s"])) if "bytes" in r else ""), flush=True)
    by = {r["step"]: r for r in results if "ms" in r}
    if "copy" in by:
        for st, r in by.items():
            if "tb_per_s" in r and st != "copy":
                print("%-20s %.2f of the copy's rate (%.2f TB/s read + write)" % (st, r["tb_per_s"] / by["copy"]["tb_per_s"], by["copy"]["tb_per_s"]), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)
    return 1 if any("failed" in r or "did_not_finish_within_s" in r for r in results) else 0


if __name__ == "__main__":
    sys.exit(main())
