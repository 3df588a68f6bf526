"""Shared pieces of the direct kernel tests (tests/test_reverse_kernels_gpu.py, tests/test_small_kernels_gpu.py): device
placement, seeded generators and the error checks, which print every measured error next to its bound before they assert.

Bounds (fp32 kernels against float64 on the CPU), the ones the suite already holds these classes of kernel to:
  REV  max|err| <= 2e-5 * max|ref|          reverse kernels (tests/test_train_kernels_gpu.py)
  PW   max|err| <= 2e-6 * max(1, max|ref|)  pointwise and interpolation kernels (tests/test_seg_gpu.py)
  bit equality for the data movers.
16-bit stored outputs (tests/test_forward_kernels_gpu.py, tests/test_dense_conv16_gpu.py): `h16` per element, and `flips` for the
share of elements that are not the RNE cast (`rne16`) of the float64 reference."""
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


def rne16(x, dt):
    """float64 -> the nearest value of a 16-bit format (torch.bfloat16 / torch.float16), ties to even, in ONE rounding
    (torch's own cast from float64 goes through fp32 and so rounds twice)."""
    p, emin = (8, -126) if dt is torch.bfloat16 else (11, -14)          # significant bits, exponent of the smallest normal value
    x = x.detach().double()
    e = torch.frexp(x)[1]                                                 # x = m * 2^e, 0.5 <= |m| < 1
    ulp = torch.ldexp(torch.ones_like(x), (e - p).clamp_min(emin - p + 1))
    return (torch.round(x / ulp) * ulp).to(dt)                            # torch.round: halves to even; the cast is exact


def flips(name, got, cpu16, ref16, factor=4.0, floor=1e-4, check=True):
    """Rounding flips of a 16-bit stored output: the share of elements that are not RNE16 of the float64 reference (ref16), held
    to `factor` x the share of the fp32 CPU evaluation of the same reference (cpu16) + `floor`.  A summation error moves a value
    across a rounding boundary with a probability proportional to it, so a small systematic error shows here long before it
    reaches half an ulp.  Returns the counts (kernel, CPU, elements); check=False only prints and returns them, for a caller
    that pools maps too small for a share of 1e-4 to mean anything (`flips_pooled`)."""
    r = ref16.float()
    n = r.numel()
    g, c = int((got.detach().cpu().float() != r).sum()), int((cpu16.float() != r).sum())
    print("ERR | %s flips%s | %.3e | %.3e | cpu fp32 %.3e" % (name, "" if check else " (pooled)", g / n, factor * c / n + floor, c / n))
    assert not check or g <= factor * c + floor * n, (name, g, c, n)
    return g, c, n


def flips_pooled(name, counts, factor=4.0, floor=1e-4):
    """The same bound over the summed counts of several cases of one kernel."""
    g, c, n = (sum(x[i] for x in counts) for i in range(3))
    print("ERR | %s flips over %d cases | %.3e | %.3e | cpu fp32 %.3e" % (name, len(counts), g / n, factor * c / n + floor, c / n))
    assert g <= factor * c + floor * n, (name, g, c, n)


def exact(name, got, ref):
    got = got.cpu()
    assert got.shape == ref.shape and got.dtype == ref.dtype, (name, tuple(got.shape), tuple(ref.shape))
    same = torch.equal(got, ref)
    print("ERR | %s | %s | bit equality" % (name, "0" if same else "differs"))
    assert same, name
