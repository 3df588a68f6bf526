"""TEST INFRASTRUCTURE -- fixtures of the SelAttention primitive (SelfPath).  Build container only (CPU):

    python tools/make_golden_selfpath.py <reference tree>

Imports the reference's own MixedOp through the shims of oracle/ref_import.py, builds MixedOp(32, 'SelAttention_<k>_1') and stores under
tests/golden/:

gs_selfpath.npz                 the gain per head count and the calibration figures per case
gs_selfpath_<case>.npz          x, out (float32 and float64), a cotangent, d_x from float32 and float64 autograd, the kept start
gs_selfpath_1x13x17_k2_maps<n>.npz  tok, qkv, o, lse, v1, ln in float64 with one floor max|ref32 - ref64| each (map_floor, in that
                                order): qkv and the floors in file 0, the rest in file 1

WEIGHTS.  S.load_formula_weights(op, salt=13), then the q and k rows of to_qkv.weight times one gain per head count
(S.selfpath_state_dict(heads, gain); the fixtures hold the gain, not weights).  The bare formula weights give scaled scores of standard
deviation 0.03 -- a flat softmax that tests nothing.  Asserted and stored per case: mean over queries of the score standard deviation in
[2, 3.5]; max|score| >= 8; entropy / ln N in [0.25, 0.8] (not at 3x5: 15 keys, near one-hot by design); the per-token standard
deviation of the LayerNorm input >= 0.1; row maxima in at least three different 32-key tiles where N >= 96.

THE MARGIN CONDITION (tools/make_golden_u2fusion.py).  PReLU's gradient jumps at 0.  The input of a case is
S.make_smooth_feature(11 + s, B, 32, H, W) for the first s <= 2000 at which, in float64, min|pre-activation| of conv and conv2 is
>= 2e-5 and >= 6 * max|pre32 - pre64|.  The softmax and the LayerNorm have no sign points.
"""
import copy
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_import  # noqa: E402
from paif_amd import synthetic as S  # noqa: E402
from tests import selfpath_eager as E  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
CASES = {"1x3x5_k2": (1, 3, 5, 2), "1x13x17_k2": (1, 13, 17, 2), "2x9x20_k1": (2, 9, 20, 1), "1x19x29_k3": (1, 19, 29, 3),
         "1x16x32_k2": (1, 16, 32, 2)}
WITH_MAPS = "1x13x17_k2"
SEED = 11
MARGIN_ABS, MARGIN_REL, MAX_START = 2e-5, 6.0, 2000
GAINS = (10.0, 9.0, 11.0, 8.0, 12.0, 7.0, 13.0, 6.0, 14.0, 5.0, 16.0)


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def npy(x):
    return x.detach().cpu().numpy()


def largest_committed():
    return max(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT) if not f.startswith("gs_selfpath"))


def save(name, **arrays):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    print("wrote %-40s %8.1f KB" % (name + ".npz", size / 1024), flush=True)
    assert size < (1 << 20) and size <= largest_committed(), "a fixture stays under 1 MiB and under the largest one already committed"


def build(R, heads, gain):
    with ref_import.quiet():
        op = R["mfa"].MixedOp(32, "SelAttention_%d_1" % heads).eval()
    S.load_formula_weights(op, salt=13)
    with torch.no_grad():
        op._op.cross_attn.to_qkv.weight[:128 * heads] *= np.float32(gain)
    mine = S.selfpath_state_dict(heads, gain)
    assert list(op._op.state_dict()) == list(mine), "state_dict order"
    for k, v in op._op.state_dict().items():
        assert np.array_equal(npy(v), mine[k]), k
    return op


def probe(op, x):
    """The reference's own intermediates, read off its modules by hooks."""
    sp, got = op._op, {}

    def tap(mod, name_in, name_out):
        def hook(m, i, o):          # returns None: the output passes unchanged
            if name_in:
                got[name_in] = i[0].detach()
            got[name_out] = o.detach()
        return mod.register_forward_hook(hook)

    hooks = [tap(sp.conv, None, "z1"), tap(sp.conv2, None, "z2"), tap(sp.cross_attn.to_qkv, "tok", "qkv"),
             tap(sp.cross_attn.to_out[0], "o", "v1"), tap(sp.norm1, None, "ln")]
    with torch.no_grad():
        got["out"] = op(x)
    for h in hooks:
        h.remove()
    got["lse"] = torch.logsumexp(E.scores(got["qkv"], sp.cross_attn.heads), dim=-1)
    return got


def figures(g64, heads, N):
    s = E.scores(g64["qkv"], heads)
    p = torch.softmax(s, dim=-1)
    ent = float((-(p * torch.log(p.clamp_min(1e-300))).sum(-1)).mean() / np.log(N))
    tiles = len(torch.unique(s.argmax(-1) // 32))
    return np.array([float(s.std(dim=-1).mean()), float(s.abs().max()), ent, float(g64["v1"].std(dim=-1).min()), tiles], dtype=np.float64)


def figures_ok(f, H, W):
    N = H * W
    return (2.0 <= f[0] <= 3.5 and f[1] >= 8.0 and ((H, W) == (3, 5) or 0.25 <= f[2] <= 0.8) and f[3] >= 0.1 and (N < 96 or f[4] >= 3))


def first_start(op, op64, B, H, W):
    for s in range(MAX_START + 1):
        x = t(S.make_smooth_feature(SEED + s, B, 32, H, W))
        g32, g64 = probe(op, x), probe(op64, x.double())
        least = min(float(g64[k].abs().min()) for k in ("z1", "z2"))
        floor = max(float((g32[k].double() - g64[k]).abs().max()) for k in ("z1", "z2"))
        if least >= MARGIN_ABS and least >= MARGIN_REL * floor:
            return s, x, least, floor, g32, g64
    raise RuntimeError("no start up to %d meets the margin condition" % MAX_START)


def grad_run(op, x, cot, dtype):
    m = copy.deepcopy(op).to(dtype)
    xx = x.to(dtype).clone().requires_grad_(True)
    out = m(xx)
    (out * cot.to(dtype)).sum().backward()
    return npy(out), npy(xx.grad)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref_import.REF_ROOT = os.path.abspath(sys.argv[1])
    R = ref_import.load()
    torch.set_num_threads(8)
    os.makedirs(OUT, exist_ok=True)
    index = {}
    for heads in sorted({c[3] for c in CASES.values()}):
        for gain in GAINS:
            op = build(R, heads, gain)
            op64 = copy.deepcopy(op).double()
            found = {name: first_start(op, op64, B, H, W) for name, (B, H, W, k) in CASES.items() if k == heads}
            figs = {name: figures(found[name][5], heads, CASES[name][1] * CASES[name][2]) for name in found}
            if all(figures_ok(figs[name], CASES[name][1], CASES[name][2]) for name in found):
                break
        else:
            raise RuntimeError("heads %d: no gain of %s meets the calibration ranges: %s" % (heads, GAINS, figs))
        index["gain_k%d" % heads] = np.float32(gain)
        for name, (s, x, least, floor, g32, g64) in found.items():
            B, H, W, _ = CASES[name]
            f = figs[name]
            assert figures_ok(f, H, W), (name, f)
            print("%-11s gain %.1f start %3d min|pre| %.2e floor %.2e | score std %.2f max|s| %.1f entropy/lnN %.2f min std(v1) %.2f argmax tiles %d"
                  % (name, gain, s, least, floor, f[0], f[1], f[2], f[3], int(f[4])), flush=True)
            index["case_" + name] = np.concatenate([[s, least, floor], f])
            cot = t(S.make_feature(900 + H, (B, 32, H, W)))
            o32, d32 = grad_run(op, x, cot, torch.float32)
            o64, d64 = grad_run(op, x, cot, torch.float64)
            assert np.array_equal(o32, npy(g32["out"])) and np.array_equal(o64, npy(g64["out"]))
            # the restatement the GPU tests use must be the reference's function
            sd64 = E.state(S.selfpath_state_dict(heads, gain), torch.float64)
            assert float((E.selfpath(x.double(), sd64, heads) - g64["out"]).abs().max()) <= 1e-11 * max(1.0, float(g64["out"].abs().max()))
            save("gs_selfpath_" + name, start=np.array(s), x=npy(x), x64=npy(x.double()), out=o32, out64=o64, cot=npy(cot), d_x=d32, d_x64=d64)
            if name == WITH_MAPS:
                keys = ("tok", "qkv", "o", "lse", "v1", "ln")
                floors = np.array([float((g32[k].double() - g64[k]).abs().max()) for k in keys])
                save("gs_selfpath_%s_maps0" % name, map_floor=floors, map_names=np.array(keys), qkv=npy(g64["qkv"]))
                save("gs_selfpath_%s_maps1" % name, **{k: npy(g64[k]) for k in keys if k != "qkv"})
    save("gs_selfpath", **index)


if __name__ == "__main__":
    main()
