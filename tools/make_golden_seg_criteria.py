"""TEST INFRASTRUCTURE -- fixtures of the segmentation criteria (OhemCELoss, SoftmaxFocalLoss, NormalLoss).  Build container only (CPU):

    python tools/make_golden_seg_criteria.py <reference tree>

Runs the reference's own three classes (core/loss.py) through the shims of oracle/ref_import.py on
F.interpolate(seg_map, labels.shape[1:], bilinear, align_corners=False), in float32 and in float64, asserts the restatement
tests/seg_criteria_eager.py equal to the float64 results, and stores three files per shape under tests/golden/,
gc_seg_<family>_<B>x<C>x<IH>x<IW>_<OH>x<OW>[_ign<k>].npz with family = ohem | focal | normal:

seg_map [B,C,IH,IW] float32 (2 x standard normal), labels [B,OH,OW] int64, ignore_lb, l64 [B,OH,OW] (the per-pixel cross entropy in
float64, 0 on ignored pixels), floor_l = max|l32 - l64|, margin = max(1e-4, 6 * floor_l), cases = the names of the cases, and per case
<case>/value32, value64, dseg32, dseg64 (d value / d seg_map from float32 and float64 autograd of the reference) plus
  ohem    <case>/thresh, T (float32(-log(float32(thresh)))), n_min, mode (1 = A: mean{l > T}, 2 = B: the n_min largest), v (mode B),
          margin_T = min over the valid pixels of |l - T|, margin_v = l_(n_min) - l_(n_min+1) (mode B with v > 0; -1 otherwise)
  focal   <case>/gamma

LABELS.  Uniform classes; about 15 % of the pixels carry ignore_lb, among them one whole row (where there is more than one row).
OHEM REGIMES, from the float64 l:  A (thresh 0.7, n_min = max(1, cnt // 2));  Bpos (thresh 0.02, n_min = max(1, cnt + (#valid - cnt) // 2):
mode B with v > 0);  Bzero (thresh 0.02, n_min = #valid + (n - #valid) // 2: the zeros of ignored pixels enter the top n_min);  nmin1;
nminN (n_min = n);  thresh1 (thresh 1.0, T = 0, n_min = max(1, #valid // 2)).
MARGINS.  A float32 evaluation must make every selection the float64 one makes, so every case needs margin_T >= margin, and mode B with
v > 0 also margin_v >= margin.  Ignored pixels are left out of margin_T: their l is exactly 0 in any arithmetic and 0 > T is false for
every T >= 0.  The seed is the first of 100, 101, ... whose inputs satisfy this for every case of the shape.

Only data is stored."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_import  # noqa: E402
from tests import seg_criteria_eager as E  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
# (seg_map shape, label size, ignore_lb)
SHAPES = (((1, 9, 1, 1), (1, 1), 255), ((1, 9, 3, 5), (12, 20), 255), ((2, 9, 6, 8), (24, 32), 255), ((1, 19, 5, 7), (13, 29), 255),
          ((2, 3, 8, 8), (8, 8), 255), ((1, 32, 4, 4), (16, 16), 255), ((2, 9, 17, 33), (68, 132), 255), ((2, 9, 6, 8), (24, 32), 7))
GAMMAS = (("g0", 0.0), ("g1", 1.0), ("g2", 2.0), ("g0.5", 0.5))
MAX_BYTES = 1 << 20


def tag(shape, size, ignore_lb):
    return "%dx%dx%dx%d_%dx%d" % (shape + size) + ("" if ignore_lb == 255 else "_ign%d" % ignore_lb)


def make_inputs(seed, shape, size, ignore_lb):
    rng = np.random.RandomState(seed)
    B, C = shape[:2]
    seg = (2.0 * rng.standard_normal(shape)).astype(np.float32)
    lab = rng.randint(0, C, size=(B,) + size).astype(np.int64)
    if ignore_lb != 255:
        lab[lab == ignore_lb] = (ignore_lb + 1) % C          # the class that serves as ignore_lb appears only as such
    lab[rng.random_sample(lab.shape) < 0.15] = ignore_lb
    if size[0] > 1:
        lab[0, size[0] // 2, :] = ignore_lb
    return seg, lab


def ohem_regimes(l64, valid):
    n, nv = l64.size, int(valid.sum())
    out = []
    for name, thresh in (("A", 0.7), ("Bpos", 0.02), ("Bzero", 0.02), ("nmin1", 0.7), ("nminN", 0.7), ("thresh1", 1.0)):
        T = E.ohem_T(thresh)
        cnt = int((l64 > T).sum())
        n_min = {"A": max(1, cnt // 2), "Bpos": max(1, cnt + (nv - cnt) // 2), "Bzero": max(1, nv + (n - nv) // 2), "nmin1": 1,
                 "nminN": n, "thresh1": max(1, nv // 2)}[name]
        out.append((name, thresh, T, n_min))
    return out


def margins(l64, valid, T, n_min):
    s = np.sort(l64.ravel())[::-1]
    cnt = int((l64 > T).sum())
    m_T = float(np.abs(l64[valid] - T).min()) if valid.any() else float("inf")
    if cnt >= n_min:
        return 1, 0.0, m_T, -1.0
    v = float(s[n_min - 1])
    m_v = float(s[n_min - 1] - s[n_min]) if (v > 0 and n_min < s.size) else -1.0
    return 2, v, m_T, m_v


def run_ref(make, seg, lab, dtype):
    x = torch.from_numpy(seg).to(dtype).requires_grad_(True)
    with ref_import.quiet():
        crit = make()
    val = crit(E.upsample(x, lab.shape[1:]), torch.from_numpy(lab))
    assert val.dtype == dtype
    val.backward()
    return val.detach().numpy(), x.grad.numpy()


def build(L, shape, size, ignore_lb):
    """-> (seed, {family: dict}) for the first seed whose inputs satisfy the margin condition in every OHEM case."""
    for seed in range(100, 200):
        seg, lab = make_inputs(seed, shape, size, ignore_lb)
        tl = torch.from_numpy(lab)
        valid = lab != ignore_lb
        if not valid.any():
            continue
        l64 = E.per_pixel(E.upsample(torch.from_numpy(seg).double(), size), tl, ignore_lb).numpy()
        l32 = E.per_pixel(E.upsample(torch.from_numpy(seg), size), tl, ignore_lb).numpy()
        # the reference's own per-pixel criterion gives the same l
        ref_l = L.NormalLoss(ignore_lb=ignore_lb).criteria(E.upsample(torch.from_numpy(seg).double(), size), tl).numpy()
        assert np.array_equal(ref_l, l64)
        floor_l = float(np.abs(l32.astype(np.float64) - l64).max())
        m = max(1e-4, 6.0 * floor_l)
        regs = ohem_regimes(l64, valid)
        marg = {name: margins(l64, valid, T, n_min) for name, _, T, n_min in regs}
        if all(mt >= m and (mv < 0 or mv >= m) for _, _, mt, mv in marg.values()):
            break
    else:
        raise RuntimeError("no seed in 100..199 satisfies the margins for %s" % (tag(shape, size, ignore_lb),))
    common = dict(seg_map=seg, labels=lab, ignore_lb=np.int64(ignore_lb), l64=l64, floor_l=np.float64(floor_l), margin=np.float64(m),
                  seed=np.int64(seed))
    fam = {"ohem": dict(common, cases=np.array([r[0] for r in regs])), "focal": dict(common, cases=np.array([g[0] for g in GAMMAS])),
           "normal": dict(common, cases=np.array(["n"]))}

    def both(make, kind, **kw):
        v32, g32 = run_ref(make, seg, lab, torch.float32)
        v64, g64 = run_ref(make, seg, lab, torch.float64)
        ev, eg = E.value_and_grad(torch.from_numpy(seg), tl, kind, ignore_lb=ignore_lb, **kw)
        # the restatement against the reference in float64: equal up to the order of the float64 sums
        assert abs(float(ev) - float(v64)) <= 1e-12 * max(1.0, abs(float(v64))), (kind, kw, float(ev), float(v64))
        assert np.abs(eg.numpy() - g64).max() <= 1e-12 * max(np.abs(g64).max(), 1e-300), (kind, kw)
        return {"value32": v32, "value64": v64, "dseg32": g32, "dseg64": g64}

    for name, thresh, T, n_min in regs:
        mode, v, m_T, m_v = marg[name]
        r = both(lambda: L.OhemCELoss(thresh, n_min, ignore_lb=ignore_lb), "ohem", T=T, n_min=n_min)
        r.update(thresh=np.float64(thresh), T=np.float32(T), n_min=np.int64(n_min), mode=np.int64(mode), v=np.float64(v),
                 margin_T=np.float64(m_T), margin_v=np.float64(m_v))
        fam["ohem"].update({name + "/" + k: a for k, a in r.items()})
    for name, gamma in GAMMAS:
        r = both(lambda: L.SoftmaxFocalLoss(gamma, ignore_lb=ignore_lb), "focal", gamma=gamma)
        r.update(gamma=np.float64(gamma))
        fam["focal"].update({name + "/" + k: a for k, a in r.items()})
    r = both(lambda: L.NormalLoss(ignore_lb=ignore_lb), "normal")
    fam["normal"].update({"n/" + k: a for k, a in r.items()})
    return seed, fam


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "core")):
        sys.exit(__doc__)
    ref_import.REF_ROOT = os.path.abspath(sys.argv[1])
    L = ref_import.load()["loss"]
    for shape, size, ignore_lb in SHAPES:
        seed, fam = build(L, shape, size, ignore_lb)
        for name, d in fam.items():
            path = os.path.join(OUT, "gc_seg_%s_%s.npz" % (name, tag(shape, size, ignore_lb)))
            np.savez_compressed(path, **d)
            assert os.path.getsize(path) < MAX_BYTES, (path, os.path.getsize(path))
        o = fam["ohem"]
        print("%-28s seed %d  floor_l %.2e  margin %.2e  modes %s  min margin_T %.2e  bytes %s" % (
            tag(shape, size, ignore_lb), seed, float(o["floor_l"]), float(o["margin"]),
            "".join("AB"[int(o[c + "/mode"]) - 1] for c in o["cases"]), min(float(o[c + "/margin_T"]) for c in o["cases"]),
            [os.path.getsize(os.path.join(OUT, "gc_seg_%s_%s.npz" % (n, tag(shape, size, ignore_lb)))) for n in fam]))


if __name__ == "__main__":
    main()
