"""Shared pieces of the direct kernel tests (tests/test_reverse_kernels_gpu.py, tests/test_small_kernels_gpu.py): device
placement, seeded generators and the error checks, which print every measured error next to its bound before they assert.

Bounds (fp32 kernels against float64 on the CPU), the ones the suite already holds these classes of kernel to:
  REV  max|err| <= 2e-5 * max|ref|          reverse kernels (tests/test_train_kernels_gpu.py)
  PW   max|err| <= 2e-6 * max(1, max|ref|)  pointwise and interpolation kernels (tests/test_seg_gpu.py)
  bit equality for the data movers."""
import torch

REV, PW = 2e-5, 2e-6


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def gen(*key, base=17):
    """A generator seeded from the case's parameters (base: one stream per test module)."""
    seed = base
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def to_dev(x):
    """CPU tensor (any float dtype) -> dense fp32 tensor on the device."""
    return x.detach().float().contiguous().to(dev())


def err(name, got, ref, bound, keep=None):
    """Print the measured error next to its bound, then assert.  keep: boolean mask of the elements that are compared."""
    got, ref = got.detach().cpu().double(), ref.detach().double()
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), name
    d = (got - ref).abs()
    if keep is not None:
        d = d[keep]
    e = float(d.max()) if d.numel() else 0.0
    print("ERR | %s | %.3e | %.3e" % (name, e, bound))
    assert e <= bound, (name, e, bound)


def rev(name, got, ref, keep=None, rel=REV, scale_over_keep=False):
    """scale_over_keep: take max|ref| over the compared elements only."""
    r = ref.detach()
    err(name, got, ref, rel * float((r[keep] if scale_over_keep else r).abs().max()), keep)


def pw(name, got, ref):
    err(name, got, ref, PW * max(1.0, float(ref.detach().abs().max())))


def h16(name, got, ref, eps16, bound32, keep=None):
    """A 16-bit stored output (tests/test_forward_kernels_gpu.py), per element:
    |got - ref| <= 1.01 * eps16 * |ref| + bound32, eps16 = 2^-8 (bf16) or 2^-11 (fp16) for the rounding of the stored value
    and bound32 the bound the fp32 form of the same kernel has at that case.  Prints the element that comes closest to (or
    exceeds by most) its own bound."""
    got, ref = got.detach().float().cpu().double(), ref.detach().double()
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), name
    d, tol = (got - ref).abs(), 1.01 * eps16 * ref.abs() + bound32
    if keep is not None:
        d, tol = d[keep], tol[keep]
    d, tol = d.reshape(-1), tol.reshape(-1)
    i = int(torch.where(d > tol, d - tol + 1.0, d / tol.clamp_min(1e-300)).argmax())     # an element over its bound, else the closest
    e, b = float(d[i]), float(tol[i])
    print("ERR | %s | %.3e | %.3e" % (name, e, b))
    assert bool((d <= tol).all()), (name, e, b)


def exact(name, got, ref):
    got = got.cpu()
    assert got.shape == ref.shape and got.dtype == ref.dtype, (name, tuple(got.shape), tuple(ref.shape))
    same = torch.equal(got, ref)
    print("ERR | %s | %s | bit equality" % (name, "0" if same else "differs"))
    assert same, name
