"""CPU: the dense conv's host-side dispatch, pinned row by row against a recorded table.

paif_conv2d_kernel_name, paif_conv2d_can_cpool and paif_conv2d_is_persistent are host-only logic: they dereference nothing and need no
GPU.  Over a grid of descriptor x shape (the shapes sit on every size rule's edge) the test asserts

1. the kernel name and the can_cpool answer of every row equal tests/golden/conv_dispatch_table.npz;
2. the contract of the pool query: where a descriptor without `cpool` answers can_cpool == 1, the same descriptor WITH `cpool` is still
   accepted and runs a kernel that writes the pool (every kernel but conv3x3_h16_dma_rows does);
3. the contract of paif_conv2d_is_persistent: 1 exactly where the name is the persistent wave-specialised kernel (conv_bf16x3_ws*).

The default environment runs in-process; every PAIF_CONV_* switch gets one fresh child process (most switches are read once per process).

`python tests/test_conv_dispatch_table.py --write` records the fixture from the library that is built in the tree.
"""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "conv_dispatch_table.npz")

F32, BF16X3, BF16, BF16X6, F16, F16X2, F16X3 = range(7)        # PAIF_CONV_*
SPLIT = (BF16X3, BF16, F16, F16X2)                              # the split-arithmetic family: the one whose kernel depends on the shape

# (B, H, W); a tile is 8 x 32, a strip-row of the row-streaming kernel one image row of 32 columns
SHAPES = [
    (8, 480, 640), (2, 64, 96), (1, 97, 131), (2, 333, 517),                # the shapes of the GPU tests
    (1, 8, 32 * 1023), (1, 8, 32 * 1024),                                   # 1023 / 1024 tiles: lower bound of the ws and dma forms
    (1, 16, 32 * 1023), (1, 16, 32 * 1023 + 1), (1, 16, 32 * 1024),         # 2046 / 2048 / 2048 tiles: the resident form's bound
    (8, 512, 2048), (8, 512, 2049),                                         # 32768 tiles = 128 x 256, the dma tile table; one column past it
    (8, 63, 2112), (8, 64, 2112),                                           # > 32768 strip-rows with H = 63 / 64: the rows kernel's H >= 64
    (7, 151, 992), (8, 64, 2048),                                           # 32767 / 32768 strip-rows with H >= 64: its size rule
    (1, 4095, 8192), (1, 4096, 8192),                                       # 2^31 bytes at 64 B per pixel; H * W * 128 = 2^32 (ws)
    (1, 2047, 8192), (1, 2048, 8192),                                       # 2^31 bytes at 128 B per pixel (res; fp32 output of rows)
    (1023, 8, 64), (1024, 8, 64),                                           # B < 1024 of the dma tile table
]
SHAPES_BLIND = [(8, 480, 640), (1, 97, 131)]      # for the families whose dispatch reads no shape (exact fp32, bf16x6, f16x3, gradient hooks)

KH_DIL = [(1, 1), (3, 1), (3, 2), (5, 1), (5, 2), (7, 1), (7, 2)]
CIN_COUT = [(32, 32), (32, 16), (16, 16)]

# one fresh child process per switch, in this order
ENVS = [("PAIF_CONV_WS", "0"), ("PAIF_CONV_RES", "0"), ("PAIF_CONV_MS", "0"), ("PAIF_CONV_DMA", "0"), ("PAIF_CONV_DMA_D2", "0"),
        ("PAIF_CONV_DMA1X1", "0"), ("PAIF_CONV_DMA_ROWS", "0"), ("PAIF_CONV_DMA_ROWS", "1"), ("PAIF_CONV_RES_NSRC", "3")]


def env_tag(var, val):
    return var[len("PAIF_CONV_"):] + "_" + val


def descriptors(split_only=False):
    """The grid: a plain product in a fixed order.  Yields (precision, storage, kh, dil, nsrc, nres, in_act, aux, pool, cpool, cin, cout, alpha).
    alpha is read by one rule only (the LDS-DMA tile kernels fold it through the activation: plain 16-bit weights), so 0.0 goes to those
    precisions alone."""
    for prec, st, (kh, dil), nsrc, nres, in_act, aux, pool, cpool, (cin, cout), alpha in itertools.product(
            range(7), range(5), KH_DIL, (1, 2, 3), range(4), (0, 1, 2), (0, 1), (0, 1), (0, 1), CIN_COUT, (1.0, 0.0)):
        if split_only and (prec not in SPLIT or cin != 32):
            continue
        if alpha == 0.0 and prec not in (BF16, F16):
            continue
        yield prec, st, kh, dil, nsrc, nres, in_act, aux, pool, cpool, cin, cout, alpha


def storage_code(st, wl0, in_act):
    """The kernels' storage template argument of a split-arithmetic launch (conv_mfma.hip kernel_st)."""
    if st == 4:
        return 15
    s = 1 if st == 3 else st
    base = (3 if in_act == 1 else 1) if s == 1 else s
    code = base + 3 if (wl0 and base) else base
    return code + 8 if st >= 3 else code


def accepted_sans_pool(prec, st, kh, dil, nsrc, nres, in_act, aux, pool, cpool, cin, cout, alpha):
    """paif_conv2d_fwd's PAIF_REQUIRE chain and the instantiations built, restated (all but the `cpool` line: that one is
    paif_conv2d_can_cpool itself).  The grid always passes the pointers and slopes a descriptor needs."""
    st_bf, st_hf = st in (1, 2), st in (3, 4)
    if st_bf and not (prec in (BF16X3, BF16) and cin == 32):
        return False
    if st_hf and not (prec in (F16, F16X2) and cin == 32):
        return False
    if prec == BF16 and not st_bf:
        return False
    if prec in (F16, F16X2) and not st_hf:
        return False
    if st == 4 and prec != F16:
        return False
    if prec in (BF16X6, F16X3):
        return cin == 32 and (kh, dil) in ((1, 1), (3, 1), (3, 2), (5, 1), (7, 1))      # (fp32 storage: the lines above)
    if prec == F32:
        return cin == 32 or (kh, dil) == (3, 1)
    if cin != 32:
        return False
    code = storage_code(st, prec in (BF16, F16), in_act)
    if aux:
        return code == 0                                # gradient hooks: fp32 storage only
    if code == 0:
        return True
    if not ((kh in (1, 3, 7) and dil == 1) or (kh, dil) == (3, 2)):
        return False
    return code in (1, 3, 4, 6, 12, 14) or (kh == 1 and code in (2, 5, 9)) or ((kh, dil) == (3, 2) and code == 15)


def evaluate(L, split_only=False):
    """Query every accepted row.  Returns (names, name index per row, can_cpool per row, is_persistent per row, contract-2 violations)."""
    one = ctypes.c_void_p(16)          # any non-null pointer: nothing is dereferenced
    buf = ctypes.create_string_buffer(96)
    names, index = [], {}
    idx, cp, pers, bad = [], [], [], []
    kname, can, isp = L.paif_conv2d_kernel_name, L.paif_conv2d_can_cpool, L.paif_conv2d_is_persistent
    from paif_amd import _lib

    for row in descriptors(split_only):
        if not accepted_sans_pool(*row):
            continue
        prec, st, kh, dil, nsrc, nres, in_act, aux, pool, cpool, cin, cout, alpha = row
        d = _lib.ConvDesc()
        for i in range(3):
            d.src[i] = one if i < nsrc else None
            d.res[i] = one if i < nres else None
        d.nsrc, d.cin, d.cout, d.kh, d.dil, d.in_act, d.precision, d.storage, d.alpha = nsrc, cin, cout, kh, dil, in_act, prec, st, alpha
        d.wpk, d.out, d.in_prelu = one, one, one
        d.pool_partial = one if pool else None
        d.aux_out = one if aux else None
        d.cpool = one if cpool else None
        ref = ctypes.byref(d)
        for B, H, W in (SHAPES if prec in SPLIT and cin == 32 and not aux else SHAPES_BLIND):
            c = can(ref, B, H, W)
            if cpool and not c:
                continue                                 # "conv2d: no fused ChannelPool for this descriptor": refused
            assert kname(ref, B, H, W, buf, 96) == 0
            n = buf.value
            k = index.get(n)
            if k is None:
                k = index[n] = len(names)
                names.append(n.decode())
            idx.append(k)
            cp.append(c)
            pers.append(isp(ref, B, H, W))
            if c and not cpool:
                d.cpool = one
                ok = can(ref, B, H, W) == 1 and kname(ref, B, H, W, buf, 96) == 0 and not buf.value.startswith(b"conv3x3_h16_dma_rows")
                d.cpool = None
                if not ok:
                    bad.append((row, (B, H, W), n.decode(), buf.value.decode()))
    return names, np.asarray(idx, np.uint16), np.asarray(cp, np.uint8), np.asarray(pers, np.uint8), bad


def run_child(var, val, out):
    """One fresh process with the switch set: evaluates the split-arithmetic rows and leaves them in `out`."""
    env = dict(os.environ)
    for v, _ in ENVS:
        env.pop(v, None)
    env[var] = val
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors="replace")
    z = np.load(out)
    return [str(s) for s in z["names"]], z["idx"], z["cpool"], z["pers"], int(z["nbad"]), str(z["bad"])


def check(tag, names, idx, cp, pers, nbad, bad):
    z = np.load(FIXTURE)
    want_names, want_idx, want_cp = [str(s) for s in z["names"]], z["idx_" + tag], z["cpool_" + tag]
    assert len(idx) == len(want_idx), "%s: the grid has %d accepted rows, the fixture %d" % (tag, len(idx), len(want_idx))
    got = np.asarray(names, dtype=object)[idx]
    want = np.asarray(want_names, dtype=object)[want_idx]
    diff = np.flatnonzero(got != want)
    assert diff.size == 0, "%s: %d rows changed their kernel, the first: row %d runs %s, recorded %s" % (
        tag, diff.size, diff[0], got[diff[0]], want[diff[0]])
    diff = np.flatnonzero(cp != want_cp)
    assert diff.size == 0, "%s: %d rows changed paif_conv2d_can_cpool, the first: row %d (%s)" % (tag, diff.size, diff[0], got[diff[0]])
    assert nbad == 0, "%s: can_cpool == 1 without `cpool`, but with it the descriptor is refused or runs a kernel without the pool: %s" % (tag, bad)
    is_ws = np.asarray([n.startswith("conv_bf16x3_ws") for n in names], np.uint8)[idx]
    diff = np.flatnonzero(pers != is_ws)
    assert diff.size == 0, "%s: paif_conv2d_is_persistent contradicts the kernel name on %d rows, the first: row %d answers %d for %s" % (
        tag, diff.size, diff[0], pers[diff[0]], got[diff[0]])


def test_dispatch_table_default_environment(monkeypatch):
    from paif_amd import _lib

    for v, _ in ENVS:
        monkeypatch.delenv(v, raising=False)        # (PAIF_CONV_DMA_ROWS is read per call)
    names, idx, cp, pers, bad = evaluate(_lib.load())
    check("default", names, idx, cp, pers, len(bad), bad[:3])


@pytest.mark.parametrize("var,val", ENVS, ids=[env_tag(*e) for e in ENVS])
def test_dispatch_table_with_switch(var, val, tmp_path):
    check(env_tag(var, val), *run_child(var, val, str(tmp_path / "rows.npz")))


def _write():
    import tempfile

    from paif_amd import _lib

    names, idx, cp, _, bad = evaluate(_lib.load())
    assert not bad, bad[:3]
    index = {n: i for i, n in enumerate(names)}
    out = {"idx_default": idx, "cpool_default": cp}
    with tempfile.TemporaryDirectory() as tmp:
        for var, val in ENVS:
            cn, cidx, ccp, _, nbad, cbad = run_child(var, val, os.path.join(tmp, "rows.npz"))
            assert nbad == 0, cbad
            for n in cn:
                if n not in index:
                    index[n] = len(names)
                    names.append(n)
            remap = np.asarray([index[n] for n in cn], np.uint16)
            out["idx_" + env_tag(var, val)] = remap[cidx]
            out["cpool_" + env_tag(var, val)] = ccp
    np.savez_compressed(FIXTURE, names=np.asarray(names), **out)
    print("wrote %s: %d names, %d + %d x %d rows, %d bytes" % (
        FIXTURE, len(names), len(idx), len(ENVS), len(out["idx_" + env_tag(*ENVS[0])]), os.path.getsize(FIXTURE)))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        from paif_amd import _lib

        names, idx, cp, pers, bad = evaluate(_lib.load(), split_only=True)
        np.savez(sys.argv[2], names=np.asarray(names), idx=idx, cpool=cp, pers=pers, nbad=len(bad), bad=str(bad[:3]))
    elif sys.argv[1:] == ["--write"]:
        _write()
    else:
        sys.exit("usage: test_conv_dispatch_table.py --write")
