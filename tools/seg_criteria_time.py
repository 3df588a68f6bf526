"""Timing of the segmentation criteria of paif_amd/core/loss.py on the GPU at the training shape (seg_map [8,9,120,160], labels 480x640):
forward and forward + backward (d/d seg_map) of NormalLoss, SoftmaxFocalLoss(2) and OhemCELoss in both modes on the HIP kernels
(csrc/seg_criteria.hip), beside the torch-eager restatement (F.interpolate + the criterion of tests/seg_criteria_eager.py, float32, same
device; its OHEM is sort-free -- the reference's own sort is timed as `ohem_sort`) and beside ops.upsample_ce.

    python tools/seg_criteria_time.py [--size 8x9x120x160] [--labels 480x640] [--repeats 9] [--step-timeout 120] [--json out.json]

Method: fence-less HIP events on the launch stream (ops.KernelTimer), two warm-up runs, then the median of --repeats runs.  Every step (one
criterion on one side) runs in a child process of its own under `timeout -k 10`; the first step that fails, faults or runs out of time
ends the whole script -- nothing more is started on the GPU after it.

Bytes are derived, not measured: what each launch must move once, with n = B*OH*OW pixels, S = 4*B*IH*IW*C bytes of logits and CP = C
rounded up to 4: pixel kernel S + 8n (labels) + 8n (the l and lse planes); each of OHEM's two histogram passes and its sum pass 4n (mode
B only: in mode A they return at once); gradient kernel S + 8n + 8n + 4n*CP; resize adjoint 4n*CP + S*CP/C.  The rate is that over the
time, as a fraction of the 6.29 TB/s a float4 copy reaches on this chip (bench.py: HBM_PEAK_GBS).  The forward + backward figure includes
what autograd adds around the kernels (NCHW <-> NHWC copies of the seg_map, the clone of the value)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_GBS = 6290.0
STEPS = ("normal", "focal", "ohem_a", "ohem_b", "ohem_sort", "upsample_ce")


def derived_bytes(step, B, C, IH, IW, OH, OW):
    n, S, cp = B * OH * OW, 4 * B * IH * IW * C, (C + 3) // 4 * 4
    launches = {"pixel": S + 16 * n, "grad": S + 16 * n + 4 * n * cp, "adjoint": 4 * n * cp + S * cp // C}
    if step == "ohem_b":
        launches.update(hist1=4 * n, hist2=4 * n, select_sum=4 * n)
    fwd = sum(v for k, v in launches.items() if k not in ("grad", "adjoint"))
    return launches, fwd, sum(launches.values())


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


def run_step(step, side, shape, size, repeats):
    import torch
    from paif_amd import ops
    from paif_amd.core import loss as L
    from tests import seg_criteria_eager as E

    dev = torch.device("cuda:0")
    B, C = shape[:2]
    g = torch.Generator().manual_seed(11)
    seg = (2.0 * torch.randn(shape, generator=g)).to(dev)
    lab = torch.randint(0, C, (B,) + size, generator=g)
    lab[torch.rand(lab.shape, generator=g) < 0.15] = 255
    lab = lab.to(dev)
    n = lab.numel()
    # mode A: most pixels lie above T(0.7) = 0.357; mode B: few lie above T(0.02) = 3.9 and n_min asks for half of all
    ohem = {"ohem_a": (0.7, n // 16), "ohem_b": (0.02, n // 2), "ohem_sort": (0.7, n // 16)}
    if side == "hip":
        crit = {"normal": lambda: L.NormalLoss().from_seg_map, "focal": lambda: L.SoftmaxFocalLoss(2.0).from_seg_map,
                "upsample_ce": lambda: ops.upsample_ce}.get(step, lambda: L.OhemCELoss(*ohem[step]).from_seg_map)()
    elif step == "ohem_sort":
        def crit(s, l, T=E.ohem_T(0.7), k=ohem[step][1]):     # the reference's formulation: a full descending sort
            v = torch.sort(E.per_pixel(E.upsample(s, l.shape[1:]), l).flatten(), descending=True).values
            return v[v > T].mean() if v[k - 1] > T else v[:k].mean()
    elif step == "upsample_ce":
        crit = lambda s, l: torch.nn.functional.cross_entropy(E.upsample(s, l.shape[1:]), l, ignore_index=255)
    else:
        kind = step if step in ("normal", "focal") else "ohem"
        kw = dict(T=E.ohem_T(ohem[step][0]), n_min=ohem[step][1]) if kind == "ohem" else (dict(gamma=2.0) if kind == "focal" else {})
        crit = lambda s, l: E.criterion(s, l, kind, **kw)

    def fwd():
        with torch.no_grad():
            crit(seg, lab)

    def fwd_bwd():
        crit(seg.detach().requires_grad_(True), lab).backward()

    res = {"step": step, "side": side, "seg_map": list(shape), "labels": list(size), "fwd_ms": _timed(fwd, repeats),
           "fwd_bwd_ms": _timed(fwd_bwd, repeats)}
    if side == "hip" and step in ("normal", "focal", "ohem_a", "ohem_b"):
        launches, fb, ab = derived_bytes(step, B, C, shape[2], shape[3], size[0], size[1])
        res.update(launch_bytes=launches, fwd_bytes=fb, fwd_bwd_bytes=ab,
                   fwd_fraction_of_copy_rate=fb / (res["fwd_ms"] * 1e-3) / (COPY_GBS * 1e9),
                   fwd_bwd_fraction_of_copy_rate=ab / (res["fwd_bwd_ms"] * 1e-3) / (COPY_GBS * 1e9))
        if step.startswith("ohem"):
            coef = ops.seg_criterion_fwd(ops.to_nhwc(seg), lab, "ohem", T=E.ohem_T(ohem[step][0]), n_min=ohem[step][1])[0]
            res["mode"] = int(coef[1])
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="8x9x120x160")
    ap.add_argument("--labels", default="480x640")
    ap.add_argument("--steps", default=",".join(STEPS))
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--step-timeout", type=int, default=120)
    ap.add_argument("--json", default=None)
    ap.add_argument("--step", default=None, help="(internal) run one step, <step>:<hip|eager>, in this process")
    a = ap.parse_args()
    shape = tuple(int(v) for v in a.size.split("x"))
    size = tuple(int(v) for v in a.labels.split("x"))
    if a.step:
        step, side = a.step.split(":")
        return run_step(step, side, shape, size, a.repeats)
    results = []
    for step in a.steps.split(","):
        for side in (("eager",) if step == "ohem_sort" else ("hip", "eager")):
            cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--step", "%s:%s" % (step, side),
                   "--size", a.size, "--labels", a.labels, "--repeats", str(a.repeats)]
            out = subprocess.run(cmd, capture_output=True, text=True)
            line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
            if out.returncode != 0 or not line:
                print("%s %s failed or ran out of time (exit %d) -- stopping\n%s" % (step, side, out.returncode, out.stderr[-2000:]), flush=True)
                results.append({"step": step, "side": side, "failed": out.returncode})
                break
            r = json.loads(line[0][7:])
            results.append(r)
            print("%-12s %-5s forward %8.3f ms   forward + backward %8.3f ms" % (step, side, r["fwd_ms"], r["fwd_bwd_ms"]) +
                  (("   %6.1f MB / %6.1f MB, %4.1f %% / %4.1f %% of the float4-copy rate%s" % (
                      r["fwd_bytes"] / 1e6, r["fwd_bwd_bytes"] / 1e6, 100 * r["fwd_fraction_of_copy_rate"],
                      100 * r["fwd_bwd_fraction_of_copy_rate"], "   mode %s" % " AB"[r["mode"]] if "mode" in r else ""))
                   if "fwd_bytes" in r else ""), flush=True)
        else:
            continue
        break
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)
    return 1 if any("failed" in r for r in results) else 0


if __name__ == "__main__":
    sys.exit(main())
