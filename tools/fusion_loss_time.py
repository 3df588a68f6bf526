"""Timing of the fusion criteria of paif_amd/core/loss.py on the GPU at B = 8, 480x640: each criterion's forward and forward + backward
(d/d generated image) on the HIP kernels (csrc/sobel_loss.hip; Fusionloss_grad3: the MSE and SSIM kernels), beside the torch-eager
restatement (tests/fusion_loss_eager.py) on the same device.

    python tools/fusion_loss_time.py [--size 8x480x640] [--criteria Fusionloss,Fusionloss6] [--repeats 9] [--step-timeout 120] [--json out.json]

Method: fence-less HIP events on the launch stream (ops.KernelTimer), two warm-up runs, then the median of --repeats runs.  Every step
(one criterion on one side) runs in a child process of its own under its own time limit; the first step that fails, faults or runs out of
time ends the whole script -- nothing more is started on the GPU after it.

Bytes are derived, not measured: a Sobel criterion's forward must read each plane its terms use once (4 B per pixel and plane), its
backward the same planes plus one write of d gen; the rate is that over the time, as a fraction of the 6.29 TB/s a float4 copy reaches
on this chip (bench.py: HBM_PEAK_GBS).  The forward figure includes the one-block finish launch; forward + backward includes what autograd
adds around the two kernels (the clone of the value, ones_like for the upstream gradient)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_GBS = 6290.0
# planes a criterion's terms read besides `gen`
PLANES = {"Fusionloss": 2, "Fusionloss2": 1, "Fusionloss3": 1, "Fusionloss4": 2, "Fusionloss6": 3, "Fusionloss_add": 2, "Total_fusion_loss3": 2,
          "Fusionloss_grad3": None}


def _timed(fn, repeats):
    import torch
    from paif_amd import ops

    tm = ops.KernelTimer(lambda tag: False)
    fn()
    fn()
    torch.cuda.synchronize()
    pairs = []
    for _ in range(repeats):
        e0 = tm.mark()
        fn()
        pairs.append((e0, tm.mark()))
    torch.cuda.synchronize()
    return statistics.median(tm.elapsed_ms(a, b) for a, b in pairs)


def run_step(name, side, B, H, W, repeats):
    import torch
    from paif_amd import synthetic as S
    from paif_amd.core import loss as L
    from tests import fusion_loss_eager as E

    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(S.make_feature(40 + i, (B, c, H, W), 0.0, 1.0)).to(dev)
         for i, (k, c) in enumerate((("ir", 1), ("vis", 3), ("mask", 1), ("gen", 1)))}
    order = E.CRITERIA[name][1]
    crit = getattr(L, name)() if side == "hip" else E.CRITERIA[name][0]

    def fwd():
        with torch.no_grad():
            crit(*[t[k] for k in order])

    def fwd_bwd():
        a = dict(t, gen=t["gen"].detach().requires_grad_(True))
        crit(*[a[k] for k in order]).backward()

    n = B * H * W
    res = {"criterion": name, "side": side, "B": B, "H": H, "W": W, "fwd_ms": _timed(fwd, repeats), "fwd_bwd_ms": _timed(fwd_bwd, repeats)}
    if side == "hip" and PLANES[name] is not None:
        res["fwd_bytes"] = 4 * n * (PLANES[name] + 1)
        res["bwd_bytes"] = 4 * n * (PLANES[name] + 2)
        res["fwd_fraction_of_copy_rate"] = res["fwd_bytes"] / (res["fwd_ms"] * 1e-3) / (COPY_GBS * 1e9)
        res["fwd_bwd_fraction_of_copy_rate"] = (res["fwd_bytes"] + res["bwd_bytes"]) / (res["fwd_bwd_ms"] * 1e-3) / (COPY_GBS * 1e9)
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="8x480x640")
    ap.add_argument("--criteria", default=",".join(PLANES))
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--step-timeout", type=int, default=120)
    ap.add_argument("--json", default=None)
    ap.add_argument("--step", default=None, help="(internal) run one step, <criterion>:<hip|eager>, in this process")
    a = ap.parse_args()
    B, H, W = (int(v) for v in a.size.split("x"))
    if a.step:
        name, side = a.step.split(":")
        return run_step(name, side, B, H, W, a.repeats)
    results = []
    for name in a.criteria.split(","):
        for side in ("hip", "eager"):
            cmd = [sys.executable, os.path.abspath(__file__), "--step", "%s:%s" % (name, side), "--size", a.size, "--repeats", str(a.repeats)]
            try:
                out = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
            except subprocess.TimeoutExpired:
                results.append({"criterion": name, "side": side, "did_not_finish_within_s": a.step_timeout})
                print("%s %s: did not finish within %d s -- stopping" % (name, side, a.step_timeout), flush=True)
                break
            line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
            if out.returncode != 0 or not line:
                print("%s %s failed (exit %d) -- stopping\n%s" % (name, side, out.returncode, out.stderr[-2000:]), flush=True)
                results.append({"criterion": name, "side": side, "failed": out.returncode})
                break
            r = json.loads(line[0][7:])
            results.append(r)
            print("%-18s %-5s forward %8.3f ms   forward + backward %8.3f ms" % (name, side, r["fwd_ms"], r["fwd_bwd_ms"]) +
                  (("   %5.1f MB / %5.1f MB, %4.1f %% / %4.1f %% of the float4-copy rate" % (
                      r["fwd_bytes"] / 1e6, (r["fwd_bytes"] + r["bwd_bytes"]) / 1e6, 100 * r["fwd_fraction_of_copy_rate"],
                      100 * r["fwd_bwd_fraction_of_copy_rate"])) if "fwd_bytes" in r else ""), flush=True)
        else:
            continue
        break
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)
    return 1 if any("failed" in r or "did_not_finish_within_s" in r for r in results) else 0


if __name__ == "__main__":
    sys.exit(main())
