"""Timing of the SelAttention primitive on the GPU: the flash attention core (ops.self_attention / ops.self_attention_bwd) and the whole
primitive (MixedOp(32, 'SelAttention_2_1'), forward and input gradient) at B = 1, heads = 2, N = 96x128, 240x320 and 480x640, beside

  * paif_sr_attention_split_fwd(precision 6 = fp16 pairs) on the same q / k / v with Nk = N -- the only kernel from before the primitive
    that can run the problem at all (it re-stages and re-splits K / V in every 256-query workgroup);
  * the torch-eager restatement (tests/selfpath_eager.py) where its N x N scores fit in memory.

    python tools/selfpath_time.py [--sizes 96x128,240x320,480x640] [--steps core_fwd,split_fwd] [--repeats 5] [--step-timeout 300] [--json out.json]

Method: fence-less HIP events on the launch stream (ops.KernelTimer), one warm-up run, then the median of --repeats runs.  Every step
(one kernel family at one size) runs in a child process of its own under its own time limit; the first step that fails, faults or runs
out of time ends the whole script -- nothing more is started on the GPU after it.  A step that is EXPECTED to be slow (the split kernel
at 480x640) is marked so: its time-out is recorded as "did not finish", and the script still stops there (it is the last step).

FLOP counts are derived, not measured: forward 4 N^2 64 heads, reverse 16 N^2 64 heads (eight N x N x 64 products: DESIGN 4), times the
MFMA instructions per product of the arithmetic (3 for fp16 pairs, 1 for the exact fp32 MFMA) for the matrix-pipe rate."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEADS = 2
STEPS = ("core_fwd", "core_bwd", "prim_fwd", "prim_bwd", "eager_fwd", "split_fwd")     # per size; split_fwd of the largest size runs last


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


def run_step(step, H, W, repeats):
    import torch
    from paif_amd import _lib, ops, synthetic as S
    from paif_amd.core.model_fusion_auto import MixedOp

    dev = torch.device("cuda:0")
    N = H * W
    g = torch.Generator().manual_seed(N)
    qkv = torch.randn(1, N, 192 * HEADS, generator=g)
    qkv[..., :128 * HEADS] *= 2.5 ** 0.5                      # score standard deviation 2.5
    qkv = qkv.to(dev)
    res = {"step": step, "H": H, "W": W, "N": N}
    if step == "core_fwd":
        res["ms"] = _timed(lambda: ops.self_attention(qkv, HEADS, want_lse=True), repeats)
        res["flop"], res["mfma_per_product"] = 4 * N * N * 64 * HEADS, 3
    elif step == "core_bwd":
        out, lse = ops.self_attention(qkv, HEADS, want_lse=True)
        dout = torch.randn(1, N, 64 * HEADS, generator=g).to(dev)
        res["ms"] = _timed(lambda: ops.self_attention_bwd(qkv, out, dout, lse, HEADS), repeats)
        res["flop"], res["mfma_per_product"] = 16 * N * N * 64 * HEADS, 1
    elif step in ("prim_fwd", "prim_bwd"):
        op = MixedOp(32, "SelAttention_%d_1" % HEADS).eval()
        op._op.load_state_dict({k: torch.from_numpy(v) for k, v in S.selfpath_state_dict(HEADS, 10.0).items()}, strict=True)
        op.to(dev)
        x = torch.from_numpy(S.make_smooth_feature(11, 1, 32, H, W)).to(dev)
        if step == "prim_fwd":
            def fn():
                with torch.no_grad():
                    op(x)
        else:
            cot = torch.from_numpy(S.make_feature(12, (1, 32, H, W))).to(dev)

            def fn():
                xx = x.clone().requires_grad_(True)
                with ops.no_param_grads():
                    (op(xx) * cot).sum().backward()
        res["ms"] = _timed(fn, repeats)
    elif step == "eager_fwd":
        from tests import selfpath_eager as E

        need = 3 * HEADS * N * N * 4          # scores, exp, and one temporary
        free = torch.cuda.mem_get_info()[0]
        if need > 0.5 * free:
            res["skipped"] = "N x N scores need %.1f GB" % (need / 1e9)
        else:
            res["ms"] = _timed(lambda: E.attention_core(qkv, HEADS), repeats)
    elif step == "split_fwd":
        C = 64 * HEADS
        q, kv = qkv[..., :C].contiguous(), qkv[..., C:].contiguous()
        out = torch.empty_like(q)
        L = ops.lib()

        def fn():
            _lib.check(L.paif_sr_attention_split_fwd(ops._p(q), ops._p(kv), ops._p(out), None, 1, N, N, C, HEADS, 6, ops._stream()), "split")
        res["ms"] = _timed(fn, repeats)
        res["flop"], res["mfma_per_product"] = 4 * N * N * 64 * HEADS, 3
        mine = ops.self_attention(qkv, HEADS)
        res["max_abs_difference_to_the_flash_kernel"] = float((mine - out).abs().max())
    else:
        raise SystemExit("unknown step " + step)
    if "ms" in res and "flop" in res:
        res["tflops"] = res["flop"] / res["ms"] / 1e9
        res["mfma_tflops"] = res["tflops"] * res["mfma_per_product"]
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="96x128,240x320,480x640")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--json", default=None)
    ap.add_argument("--steps", default=",".join(STEPS), help="which of %s to run" % (STEPS,))
    ap.add_argument("--step", default=None, help="(internal) run one step in this process")
    ap.add_argument("--hw", default=None)
    a = ap.parse_args()
    if a.step:
        H, W = (int(v) for v in a.hw.split("x"))
        return run_step(a.step, H, W, a.repeats)
    sizes = [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")]
    plan = [(st, H, W) for H, W in sizes for st in a.steps.split(",")]
    plan.sort(key=lambda p: (p[0] == "split_fwd" and (p[1], p[2]) == sizes[-1]))       # the step that may not finish goes last
    results = []
    for st, H, W in plan:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", st, "--hw", "%dx%d" % (H, W), "--repeats", str(a.repeats)]
        try:
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            results.append({"step": st, "H": H, "W": W, "did_not_finish_within_s": a.step_timeout})
            print("%s %dx%d: did not finish within %d s -- stopping" % (st, H, W, a.step_timeout), flush=True)
            break
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
        if out.returncode != 0 or not line:
            print("%s %dx%d failed (exit %d) -- stopping\n%s" % (st, H, W, out.returncode, out.stderr[-2000:]), flush=True)
            results.append({"step": st, "H": H, "W": W, "failed": out.returncode})
            break
        r = json.loads(line[0][7:])
        results.append(r)
        print("%-9s %3dx%-3d %s" % (st, H, W, ("%10.3f ms" % r["ms"]) if "ms" in r else r.get("skipped", "")) +
              (("  %7.1f TFLOP/s (%.1f on the matrix pipe)" % (r["tflops"], r["mfma_tflops"])) if "tflops" in r else ""), flush=True)
    by = {(r["step"], r["H"], r["W"]): r for r in results}
    for H, W in sizes:
        new, old = by.get(("core_fwd", H, W), {}), by.get(("split_fwd", H, W), {})
        if "ms" in new and "ms" in old:
            print("%dx%d: flash forward %.3f ms, split kernel %.3f ms, ratio %.2f" % (H, W, new["ms"], old["ms"], old["ms"] / new["ms"]), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)
    bad = [r for r in results if "failed" in r]
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
