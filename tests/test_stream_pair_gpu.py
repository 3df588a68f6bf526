"""The pair form of the two image streams' shared prefix (ops.CONFIG["stream_pair"]): the stems of both streams as one launch
(`paif_stem_fwd_pair`), their guided filters as one joint batch of 2B images (`paif_guided_filter_fused_fwd_joint`, the f16-range
fallback decided per problem).  Same kernels, same arithmetic, fewer launches: EVERY comparison here is bitwise, against the two single
launches of the path that stays in place.  The last tests need no GPU: the rules that switch the pair path off."""
import pytest
import torch

from paif_amd import ops, synthetic as S
from tests.helpers import t

gpu = pytest.mark.gpu
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _default_arithmetic():
    old = dict(ops.CONFIG)
    ops.set_conv_precision("bf16x3")
    ops.set_storage("f32")
    yield
    ops.CONFIG.clear()
    ops.CONFIG.update(old)
    ops._ACT_BF16[0] = False
    ops._TWINS.clear()


def _bits(x):
    return x.contiguous().view(torch.int16 if x.dtype in (F16, BF16) else torch.int32)


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, tuple(a.shape), tuple(b.shape))
    assert torch.equal(_bits(a), _bits(b)), (what, int((_bits(a) != _bits(b)).sum()))


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(shape, generator=g) * 2 - 1) * scale).to(_dev())


# ---- 1. stem pair ----
@gpu
@pytest.mark.parametrize("storage", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("shape", [(1, 5, 7), (2, 11, 131)])       # ragged; past one 128-pixel chunk
def test_stem_pair_is_two_stems(shape, storage):
    B, H, W = shape
    ir = _rand((B, 1, H, W), 1) * 0.5 + 0.5
    vis = (_rand((B, 3, H, W), 2) * 0.5 + 0.5)[:, 0:1]              # channel 0 of a 3-plane tensor: its own batch stride
    w0, w1 = _rand((32, 1, 3, 3), 3), _rand((32, 1, 3, 3), 4)
    a0, a1 = torch.full((1,), 0.25, device=_dev()), torch.full((1,), 0.1, device=_dev())
    ops.set_storage(storage)
    with ops.bf16_activations():
        f0, g0 = ops.stem(ir, w0, a0)
        f1, g1 = ops.stem(vis, w1, a1)
        feat, guide, (h0, h1) = ops.stem_pair(ir, w0, a0, vis, w1, a1)
        assert feat.shape == (2 * B, H, W, 32) and feat.dtype == F32 and guide.shape == (2 * B, H, W)
        _same(h0, f0, "map 0"), _same(h1, f1, "map 1")
        _same(feat[:B], f0, "joint map 0"), _same(feat[B:], f1, "joint map 1")
        _same(guide[:B], g0, "guide 0"), _same(guide[B:], g1, "guide 1")
        if storage != "f32":                                        # the 16-bit twins: both half-views find their halves
            for h, f in ((h0, f0), (h1, f1)):
                tw, ref = ops.cast_storage(h, True), ops.cast_storage(f, True)
                assert tw.dtype == (F16 if storage == "f16" else BF16) and ops._TWINS[h.data_ptr()][1] is tw
                _same(tw, ref, "twin")
        else:
            assert not ops._TWINS
    torch.cuda.synchronize()


@gpu
def test_stem_pair_fp16_only_map():
    """CONFIG["gf_in_f16"]: no fp32 map at all, the joint fp16 map is the stem's output."""
    B, H, W = 2, 11, 131
    ir, vis = _rand((B, 1, H, W), 5), _rand((B, 3, H, W), 6)[:, 0:1]
    w0, w1 = _rand((32, 1, 3, 3), 3), _rand((32, 1, 3, 3), 4)
    a0, a1 = torch.full((1,), 0.25, device=_dev()), torch.full((1,), 0.1, device=_dev())
    ops.set_storage("f16")
    ops.CONFIG["gf_in_f16"] = True
    with ops.bf16_activations():
        f0, g0 = ops.stem(ir, w0, a0)
        f1, g1 = ops.stem(vis, w1, a1)
        feat, guide, (h0, h1) = ops.stem_pair(ir, w0, a0, vis, w1, a1)
    assert feat.dtype == F16
    _same(h0, f0, "map 0"), _same(h1, f1, "map 1"), _same(guide[:B], g0, "guide 0"), _same(guide[B:], g1, "guide 1")


# ---- 2. guided filter on the joint batch ----
def _gf_inputs(B, H, W, seed):
    y = _rand((B, H, W, 32), seed)
    return ops.channel_residue(y), y


@gpu
@pytest.mark.parametrize("mode", ["hf16", "hf16_y16", "bf16", "f32"])
@pytest.mark.parametrize("shape", [(1, 24, 100), (2, 70, 170)])
def test_guided_filter_joint_batch_is_two_calls(shape, mode):
    """(2+2, 70, 170): three 80-column strips (the last 10 wide) in the 12-wave build, slots of rows that cross strip, image and
    problem boundaries."""
    B, H, W = shape
    g0, y0 = _gf_inputs(B, H, W, 10)
    g1, y1 = _gf_inputs(B, H, W, 11)
    if mode == "hf16_y16":
        y0, y1 = y0.to(F16), y1.to(F16)
    ob = {"hf16": F16, "hf16_y16": F16, "bf16": True, "f32": False}[mode]
    assert ops.guided_filter_joint_fits(2 * B, H, W)
    r0, r1 = ops.guided_filter_pair(g0, y0, out_bf16=ob), ops.guided_filter_pair(g1, y1, out_bf16=ob)
    j = ops.guided_filter_pair(torch.cat([g0, g1]), torch.cat([y0, y1]), out_bf16=ob, bsplit=B)
    assert j.shape == (2, 2 * B, H, W, 32)
    for e in range(2):
        _same(j[e][:B], r0[e], "problem 0, eps %d" % e)
        _same(j[e][B:], r1[e], "problem 1, eps %d" % e)


@gpu
@pytest.mark.parametrize("which", [0, 1])
def test_guided_filter_joint_batch_overflow_stays_in_its_problem(which, monkeypatch):
    """Only one problem's data leaves the f16 range of the matrix-core engine's split sums: that problem's half must be its own single
    call's result (which takes the VALU fallback), the other half its own single call's matrix-core result."""
    B, H, W = 2, 70, 170
    g, y = [None, None], [None, None]
    for p in range(2):
        g[p], y[p] = _gf_inputs(B, H, W, 20 + p)
    y[which] = y[which] * 3.0e4                                  # 9-row sums ~ 1e5: beyond 65,000
    r = [ops.guided_filter_pair(g[p], y[p]) for p in range(2)]
    j = ops.guided_filter_pair(torch.cat(g), torch.cat(y), bsplit=B)
    for e in range(2):
        _same(j[e][:B], r[0][e], "problem 0, eps %d" % e)
        _same(j[e][B:], r[1][e], "problem 1, eps %d" % e)
    # the single call of the overflowing problem did take the VALU fallback, and the two engines differ in bits on the other problem's
    # in-range data: the comparison above tells them apart
    monkeypatch.setenv("PAIF_GF_ENGINE", "valu")
    v = [ops.guided_filter_pair(g[p], y[p]) for p in range(2)]
    _same(v[which], r[which], "the overflowing problem's single call")
    assert not torch.equal(_bits(v[1 - which]), _bits(r[1 - which]))


# ---- 3. / 4. conv pairs ----
def _h16(shape, seed, dt):
    return _rand(shape, seed).to(dt)


def _pair_name(kw0, kw1):
    """-> (return code, kernel name) of paif_conv2d_pair_kernel_name for the descriptors conv2d builds from kw0 / kw1 (nothing is launched)."""
    import ctypes
    pend = []
    ops.conv2d(_defer=pend, **kw0)
    ops.conv2d(_defer=pend, **kw1)
    assert len(pend) == 2
    (d0, (B, H, W), _, _), (d1, _, _, _) = pend
    buf = ctypes.create_string_buffer(96)
    rc = ops.lib().paif_conv2d_pair_kernel_name(ctypes.byref(d0), ctypes.byref(d1), B, H, W, buf, len(buf))
    return rc, buf.value.decode()


def _storage(dt):
    ops.set_storage("f16" if dt is F16 else "bf16")
    return ops.bf16_activations()


@gpu
@pytest.mark.parametrize("dt", [F16, BF16])
def test_conv1x1_pair_is_two_launches(dt):
    """The folded decomposition 1x1 at the ragged shape above the size rule, different weights and biases per problem."""
    B, H, W = 2, 333, 517
    with _storage(dt):
        kws = []
        for p in range(2):
            w = _rand((32, 96, 1, 1), 30 + p, 0.2)
            kws.append(dict(srcs=[_h16((B, H, W, 32), 40 + 3 * p + i, dt) for i in range(3)], wpk=ops.pack_conv_weight(w, 3, 32, 1), kh=1, dil=1,
                            shift=_rand((32,), 50 + p)))
        rc, name = _pair_name(*kws)
        assert rc == 0 and name == "conv_h16_dma_1x1<%d>" % (2 if dt is F16 else 1), (rc, name)
        r0, r1 = ops.conv2d(**kws[0]), ops.conv2d(**kws[1])
        o0, o1 = ops.conv2d_pair(*kws)
        _same(o0, r0, "problem 0"), _same(o1, r1, "problem 1")


@gpu
@pytest.mark.parametrize("dt", [F16, BF16])
@pytest.mark.parametrize("shape", [(1, 261, 1001), (2, 333, 517), (1, 320, 1024)])     # 1,056 / 1,428 / 1,280 tiles per problem
@pytest.mark.parametrize("form", [(1, 0), (2, 0), (3, 1)])
def test_tile_conv_pair_is_two_launches(form, shape, dt):
    """128 workgroups per problem (16 of every XCD's 32): 8-9, 11-12 and 10 tiles per workgroup -- every residue of the unroll factors."""
    nsrc, nres = form
    B, H, W = shape
    with _storage(dt):
        kws = []
        for p in range(2):
            srcs = [_h16((B, H, W, 32), 60 + 3 * p + i, dt) for i in range(nsrc)]
            w = _rand((32, 32 * nsrc, 3, 3), 70 + p, 0.1)
            kw = dict(srcs=srcs, wpk=ops.pack_conv_weight(w, nsrc, 32, 3), kh=3, dil=1, act=ops.ACT_PRELU,
                      prelu=torch.full((1,), 0.25 - 0.15 * p, device=_dev()))
            if nres:
                kw.update(alpha=0.333333, res=(srcs[0],))
            kws.append(kw)
        rc, name = _pair_name(*kws)
        assert rc == 0 and name == "conv3x3_h16_dma<%d, %d, %d, false, 1, 0>" % (nsrc, nres, 2 if dt is F16 else 1), (rc, name)
        r0, r1 = ops.conv2d(**kws[0]), ops.conv2d(**kws[1])
        o0, o1 = ops.conv2d_pair(*kws)
        _same(o0, r0, "problem 0"), _same(o1, r1, "problem 1")


@gpu
def test_conv_pair_not_supported_falls_back_to_two_launches():
    """A pool-epilogue descriptor and two descriptors of different forms have no pair form: the query says so (PAIF_ENOSUP = -2) and
    conv2d_pair issues the two single launches."""
    B, H, W = 2, 333, 517
    with _storage(F16):
        x = [_h16((B, H, W, 32), 80 + i, F16) for i in range(3)]
        w3 = ops.pack_conv_weight(_rand((32, 96, 3, 3), 90, 0.1), 3, 32, 3)
        w1 = ops.pack_conv_weight(_rand((32, 32, 3, 3), 91, 0.1), 1, 32, 3)
        a = torch.full((1,), 0.25, device=_dev())
        comp = torch.empty((B, H, W, 4), device=_dev(), dtype=F32)
        pool = dict(srcs=x, wpk=w3, kh=3, dil=1, act=ops.ACT_PRELU, prelu=a, alpha=0.333333, res=(x[0],), cpool=(comp, 0))
        assert _pair_name(pool, dict(pool, cpool=(comp, 2)))[0] == -2
        three = dict(pool, cpool=None)
        one = dict(srcs=x[:1], wpk=w1, kh=3, dil=1, act=ops.ACT_PRELU, prelu=a)
        assert _pair_name(three, one)[0] == -2
        assert _pair_name(three, three)[0] == 0
        r0, r1 = ops.conv2d(**three), ops.conv2d(**one)
        o0, o1 = ops.conv2d_pair(three, one)
        _same(o0, r0, "three sources"), _same(o1, r1, "one source")


# ---- 5. whole forward ----
def _fusion_net(dev=None):
    from paif_amd.core.model_fusion_auto import Network_Fusion_Searched
    from paif_amd.genotypes import FUSION_AT

    net = Network_Fusion_Searched(32, None, FUSION_AT).eval()
    net.load_state_dict({k: t(S.formula_tensor("enhance_net." + k, tuple(v.shape))).to(v.dtype) for k, v in net.state_dict().items()},
                        strict=True)
    return net if dev is None else net.to(dev)


def _forward(net, ir, ycc, pair):
    ops.CONFIG["stream_pair"] = pair
    with torch.no_grad():
        return net(ir, ycc).clone()


@gpu
@pytest.mark.parametrize("shape,storage", [((2, 72, 200), "f16"), ((2, 333, 517), "f16"), ((2, 333, 517), "bf16")])
def test_forward_with_and_without_the_pair_path(shape, storage, monkeypatch):
    """(2, 72, 200) lies below the size rules of the LDS-DMA convs: there the conv pair calls fall back to single launches (the stem and
    guided-filter pairs have no size rule and run); at (2, 333, 517) the 1x1 and the three tile convs run as pairs."""
    net = _fusion_net(_dev())
    ir, vis, _ = S.make_batch(*shape)
    irt, ycc = t(ir).to(_dev()), ops.rgb2ycrcb(t(vis).to(_dev()))
    calls = []
    real = ops.stem_pair
    monkeypatch.setattr(ops, "stem_pair", lambda *a: (calls.append(1), real(*a))[1])
    ops.set_storage(storage)
    off = _forward(net, irt, ycc, False)
    assert not calls
    paired = []
    real_launch = ops._launch_convs
    monkeypatch.setattr(ops, "_launch_convs", lambda pend: (paired.append(real_launch(pend)), paired[-1])[1])
    on = _forward(net, irt, ycc, True)
    assert calls == [1]
    assert sum(1 for x in paired if x) == (0 if shape == (2, 72, 200) else 4), paired
    _same(on, off, "fused image")
    ops.check_f16_overflow()


@gpu
def test_forward_pair_path_replayed_from_a_graph():
    net = _fusion_net(_dev())
    ir, vis, _ = S.make_batch(2, 333, 517)
    irt, ycc = t(ir).to(_dev()), ops.rgb2ycrcb(t(vis).to(_dev()))
    ops.set_storage("f16")
    eager = _forward(net, irt, ycc, True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _forward(net, irt, ycc, True)                            # warm-up on the capture stream: packs, workspaces
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with torch.no_grad():
            out = net(irt, ycc)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    _same(out, eager, "fused image from the graph")
    ops.check_f16_overflow()


# ---- 6. no GPU: the rules that switch the pair path off, the twin table ----
def test_pair_path_rules():
    from paif_amd.operations_m import ResidualDenseBlock

    net = _fusion_net()
    dec = net.decompation
    assert isinstance(dec.chain._ops[0]._op, ResidualDenseBlock) and isinstance(dec.chain2._ops[0]._op, ResidualDenseBlock)
    assert dec.pair_capable()
    ops._ACT_BF16[0] = F16
    assert net._pair_path(None, None, True)
    assert not net._pair_path({}, None, True)                     # a taped pass
    assert not net._pair_path(None, {}, True)                     # a forward that returns intermediates
    assert not net._pair_path(None, None, False)                  # no device
    ops.CONFIG["two_stream"] = True
    assert not net._pair_path(None, None, True)
    ops.CONFIG["two_stream"] = False
    ops.CONFIG["stream_pair"] = False
    assert not net._pair_path(None, None, True)
    ops.CONFIG["stream_pair"] = True
    ops._ACT_BF16[0] = False                                      # fp32 storage
    assert not net._pair_path(None, None, True)
    ops._ACT_BF16[0] = BF16
    assert net._pair_path(None, None, True)
    # chains whose first ops differ: looked up on the modules
    first = dec.chain2._ops[0]
    keep = first._op
    first._op = torch.nn.Identity()
    assert not dec.pair_capable() and not net._pair_path(None, None, True)
    first._op = keep
    keep.d = 2                                                    # the same block at dilation 2
    assert not dec.pair_capable()
    keep.d = 1
    assert dec.pair_capable()


def test_twin_table_resolves_both_half_views():
    B = 2
    feat = torch.arange(2 * B * 3 * 4 * 32, dtype=F32).reshape(2 * B, 3, 4, 32)
    twin = feat.to(F16)
    h0, h1 = ops.register_twin_halves(feat, twin, B)
    assert h0.data_ptr() == feat.data_ptr() and h1.data_ptr() != h0.data_ptr()
    for h, lo in ((h0, 0), (h1, B)):
        got = ops.cast_storage(h, F16)                            # found in the table: no kernel runs (these are CPU tensors)
        assert got.data_ptr() == twin[lo:lo + B].data_ptr() and got.is_contiguous() and torch.equal(got, twin[lo:lo + B])
