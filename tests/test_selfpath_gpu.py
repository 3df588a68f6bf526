"""GPU: the SelAttention primitive (paif_amd.operations_m.SelfPath / Attention, csrc/attention_full.hip) -- the flash attention core against
a float64 eager softmax on the device, the whole primitive against the reference's own outputs and autograd (tests/golden/gs_selfpath*.npz,
tools/make_golden_selfpath.py), and the op inside a chain, the searched network, the attack and a captured graph.

Bound F (fp32-level arithmetic, tests/test_drdb_gpu.py): max|hip - ref64| <= 1.5 * floor + 1e-5 * max(1, max|ref64|), floor = max|ref32 - ref64|
of the same tensor.  Bound D (default precisions, tests/test_attack_gpu.py): <= 1e-4 * max(1, max|ref|)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from paif_amd import ops, synthetic as S
from tests import selfpath_eager as E
from tests.helpers import t

pytestmark = pytest.mark.gpu

CASES = {"1x3x5_k2": 2, "1x13x17_k2": 2, "2x9x20_k1": 1, "1x19x29_k3": 3, "1x16x32_k2": 2}
CORE_SIZES = [(1, 1, 15), (1, 2, 221), (2, 1, 180), (1, 3, 551), (1, 2, 512), (1, 2, 1025), (1, 1, 5120)]
CONSTRUCTED = [(kind, n) for kind in "abcd" for n in (221, 551)]
SEL_GENOTYPE = dict(normal_1=[("Denseblocks_3_1", 0), ("DilConv_3_2", 1)], normal_1_concat=[1, 2],
                    normal_2=[("Denseblocks_3_1", 0), ("Denseblocks_3_1", 1)], normal_2_concat=[1, 2],
                    normal_3=[("SelAttention_2_1", 0), ("Residualblocks_7_1", 1)], normal_3_concat=[1, 2])
_REF = {}


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bound_f(floor, ref64):
    return 1.5 * floor + 1e-5 * max(1.0, float(ref64.abs().max()))


def _check_f(what, mine, ref32, ref64):
    floor = float((ref32.double() - ref64).abs().max())
    err = float((mine.double() - ref64).abs().max())
    bound = _bound_f(floor, ref64)
    print("%s: err %.3e floor %.3e bound %.3e ratio %.3f scale %.3e" % (what, err, floor, bound, err / bound, float(ref64.abs().max())))
    assert err <= bound, (what, err, bound)


def _check_d(what, mine, ref):
    ref = ref.double()
    err = float((mine.double() - ref).abs().max())
    bound = 1e-4 * max(1.0, float(ref.abs().max()))
    print("%s: err %.3e bound %.3e ratio %.3f" % (what, err, bound, err / bound))
    assert err <= bound, (what, err, bound)


class _exact:
    def __enter__(self):
        self.old = (ops.CONFIG["conv_precision"], ops.CONFIG["gemm_precision"])
        ops.set_conv_precision("f32"), ops.set_gemm_precision("f32")

    def __exit__(self, *a):
        ops.set_conv_precision(self.old[0]), ops.set_gemm_precision(self.old[1])


# ------------------------------------------------------------------------------------------------------------------------------
# inputs of the core tests
# ------------------------------------------------------------------------------------------------------------------------------
def _randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _random_qkv(B, heads, N):
    """q, k ~ N(0, sigma^2) per element: the scaled score q.k / 8 has standard deviation sigma^2 (2.5; 0.3 on the long flat row)."""
    sd = 0.3 if N == 5120 else 2.5
    qkv = _randn(1000 + N + heads, B, N, 192 * heads)
    qkv[..., :128 * heads] *= sd ** 0.5
    return qkv, sd


def _constructed_qkv(kind, N, heads=2):
    """Four constructed inputs (the module docstring of the issue's cases): q | k | v [1, N, 192 heads] in float64."""
    u = F.normalize(_randn(7, 64), dim=0)
    q, k = torch.zeros(1, N, heads, 64, dtype=torch.float64), torch.zeros(1, N, heads, 64, dtype=torch.float64)
    v = _randn(11 + N, 1, N, heads, 64)
    noise_q, noise_k = _randn(12 + N, 1, N, heads, 64), _randn(13 + N, 1, N, heads, 64)
    noise_q -= (noise_q @ u)[..., None] * u          # orthogonal to u: the constructed part of the score is exact
    noise_k -= (noise_k @ u)[..., None] * u
    if kind == "a":      # late maximum: score = a_j + noise, a_j rising from -60 to 60 with the key index
        a = torch.linspace(-60.0, 60.0, N, dtype=torch.float64)
        q[:] = 8.0 * u + 0.3 * noise_q
        k[:] = a[None, :, None, None] * u + 0.3 * noise_k
    elif kind == "b":    # every score <= -40
        q[:] = 20.0 * u + 0.3 * noise_q
        k[:] = -20.0 * u + 0.3 * noise_k
    elif kind == "c":    # identical keys: p exactly uniform
        q[:] = 1.5 * _randn(14 + N, 1, N, heads, 64)
        k[:] = 1.5 * _randn(15, 64)
    else:                # one-hot: query i points at key (7 i) mod N
        kk = F.normalize(_randn(16 + N, 1, N, heads, 64), dim=-1)
        k[:] = 29.0 * kk
        q[:] = 29.0 * kk[:, (7 * torch.arange(N)) % N]
    return torch.cat([q.reshape(1, N, -1), k.reshape(1, N, -1), v.reshape(1, N, -1)], dim=-1).contiguous(), heads


def _core_case(key):
    """-> dict(qkv32 on device, heads, out / lse from float64 and float32 eager, cot, dqkv from float64 / float32 autograd), computed once."""
    if key not in _REF:
        if key[0] == "random":
            _, B, heads, N = key
            qkv64, sd = _random_qkv(B, heads, N)
        else:
            (qkv64, heads), sd = _constructed_qkv(key[1], key[2]), None
        qkv32 = qkv64.float().to(_dev())
        r = dict(qkv=qkv32, heads=heads, sd=sd)
        cot = _randn(99, *qkv64.shape[:2], 64 * heads).float().to(_dev())
        r["cot"] = cot
        for name, dt in (("64", torch.float64), ("32", torch.float32)):
            x = qkv32.to(dt).requires_grad_(True)          # both references start from the SAME float32 values
            out, lse = E.attention_core(x, heads)
            r["out" + name], r["lse" + name] = out.detach(), lse.detach()
            if qkv64.shape[1] <= 1025:
                (out * cot.to(dt)).sum().backward()
                r["dqkv" + name] = x.grad
            if dt == torch.float64:
                r["scores"] = E.scores(x.detach(), heads)
        _REF[key] = r
    return _REF[key]


# ------------------------------------------------------------------------------------------------------------------------------
# 1 / 2 / 3: the attention core
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,heads,N", CORE_SIZES)
def test_core_forward_random(B, heads, N):
    r = _core_case(("random", B, heads, N))
    std = float(r["scores"].std(dim=-1).mean())
    print("score std %.3f (wanted %.1f)" % (std, r["sd"]))
    assert abs(std / r["sd"] - 1) <= 0.2
    out, lse = ops.self_attention(r["qkv"], heads, want_lse=True)
    assert out.shape == (B, N, 64 * heads) and lse.shape == (B, heads, N)
    _check_f("out", out, r["out32"], r["out64"])
    _check_f("lse", lse, r["lse32"], r["lse64"])
    assert torch.equal(ops.self_attention(r["qkv"], heads), out)


@pytest.mark.parametrize("kind,N", CONSTRUCTED)
def test_core_forward_constructed(kind, N):
    r = _core_case(("constructed", kind, N))
    s = r["scores"]
    if kind == "a":
        assert int(s.argmax(-1).min()) >= (N - 1) // 64 * 64 and float(s.max()) >= 55 and float(s.min()) <= -55
    elif kind == "b":
        assert float(s.max()) <= -40
    elif kind == "c":
        assert float((s.max(-1).values - s.min(-1).values).max()) <= 1e-4
    else:
        top = s.topk(2, dim=-1).values
        assert float((top[..., 0] - top[..., 1]).min()) >= 30
    out, lse = ops.self_attention(r["qkv"], r["heads"], want_lse=True)
    _check_f("out", out, r["out32"], r["out64"])
    _check_f("lse", lse, r["lse32"], r["lse64"])
    if kind == "c":
        v = r["qkv"][..., 128 * r["heads"]:].double().mean(dim=1, keepdim=True)
        assert float((out.double() - v).abs().max()) <= 1e-5


@pytest.mark.parametrize("key", [("random",) + s for s in CORE_SIZES if s[2] != 5120] + [("constructed", k, n) for k in "ad" for n in (221, 551)],
                         ids=lambda k: "-".join(str(x) for x in k))
def test_core_reverse(key):
    r = _core_case(key)
    heads = r["heads"]
    out, lse = ops.self_attention(r["qkv"], heads, want_lse=True)
    dqkv = ops.self_attention_bwd(r["qkv"], out, r["cot"], lse, heads)
    again = ops.self_attention_bwd(r["qkv"], out, r["cot"], lse, heads)
    for i, name in enumerate(("dq", "dk", "dv")):
        sl = slice(64 * heads * i, 64 * heads * (i + 1))
        _check_f(name, dqkv[..., sl], r["dqkv32"][..., sl], r["dqkv64"][..., sl])
    assert torch.equal(dqkv, again), "no atomics: the same inputs give the same bits"


def test_core_reads_only_its_own_columns():
    """Head 1 of a three-head tensor: the same q / k / v blocks with other filler in the other heads' columns give the same bits."""
    B, N, heads = 2, 221, 3
    a = _randn(5, B, N, 192 * heads).float().to(_dev())
    b = _randn(6, B, N, 192 * heads).float().to(_dev()) * 3
    cot_a, cot_b = _randn(7, B, N, 64 * heads).float().to(_dev()), _randn(8, B, N, 64 * heads).float().to(_dev())
    for blk in range(3):
        c0 = 64 * heads * blk + 64
        b[..., c0:c0 + 64] = a[..., c0:c0 + 64]
    cot_b[..., 64:128] = cot_a[..., 64:128]
    oa, la = ops.self_attention(a, heads, want_lse=True)
    ob, lb = ops.self_attention(b, heads, want_lse=True)
    assert torch.equal(oa[..., 64:128], ob[..., 64:128]) and torch.equal(la[:, 1], lb[:, 1])
    assert not torch.equal(oa[..., :64], ob[..., :64])
    da, db = ops.self_attention_bwd(a, oa, cot_a, la, heads), ops.self_attention_bwd(b, ob, cot_b, lb, heads)
    for blk in range(3):
        c0 = 64 * heads * blk + 64
        assert torch.equal(da[..., c0:c0 + 64], db[..., c0:c0 + 64])


# ------------------------------------------------------------------------------------------------------------------------------
# 4 / 5: the whole primitive
# ------------------------------------------------------------------------------------------------------------------------------
def _op(golden, heads, grad=False):
    from paif_amd.core.model_fusion_auto import MixedOp

    op = MixedOp(32, "SelAttention_%d_1" % heads).eval()
    gain = float(golden("gs_selfpath")["gain_k%d" % heads])
    op._op.load_state_dict({k: t(v) for k, v in S.selfpath_state_dict(heads, gain).items()}, strict=True)
    return op.to(_dev())


@pytest.mark.parametrize("case", list(CASES))
def test_primitive_forward(golden, case):
    g = golden("gs_selfpath_" + case)
    op = _op(golden, CASES[case])
    x = t(g["x"]).to(_dev())
    with torch.no_grad():
        y = op(x)
        _check_d("default " + case, y.cpu(), t(g["out64"]))
        assert torch.equal(op.train()(x), y), ".train() computes what .eval() does"
        op.eval()
        with _exact():
            _check_f("exact " + case, op(x).cpu(), t(g["out"]), t(g["out64"]))


def test_primitive_taped_intermediates(golden):
    case = "1x13x17_k2"
    g, m0, m1 = golden("gs_selfpath_" + case), golden("gs_selfpath_%s_maps0" % case), golden("gs_selfpath_%s_maps1" % case)
    op = _op(golden, 2)._op
    tape = []
    with torch.no_grad(), _exact():
        op.forward_nhwc(ops.to_nhwc(t(g["x"]).to(_dev())), (), tape)
        e = tape[0]
        ln = ops.layernorm(e["v1"], op.norm1.weight, op.norm1.bias, op.norm1.eps)
        o = ops.self_attention(e["qkv"], 2)       # not on the tape (the reverse kernels do not read it): the same launch on the taped qkv
    assert "o" not in e
    mine = dict(tok=e["r"].reshape(1, 221, 32), qkv=e["qkv"], o=o, lse=e["lse"], v1=e["v1"], ln=ln)
    for name, floor in zip(m0["map_names"], m0["map_floor"]):
        ref = t(m0[name] if name in m0 else m1[name])
        err = float((mine[str(name)].cpu().double() - ref).abs().max())
        bound = _bound_f(float(floor), ref)
        print("%s: err %.3e floor %.3e bound %.3e ratio %.3f" % (name, err, floor, bound, err / bound))
        assert err <= bound, (name, err, bound)


@pytest.mark.parametrize("case", list(CASES))
def test_primitive_input_gradient(golden, case):
    g = golden("gs_selfpath_" + case)
    op = _op(golden, CASES[case])
    cot = t(g["cot"]).to(_dev())

    def grad():
        x = t(g["x"]).to(_dev()).requires_grad_(True)
        with ops.no_param_grads():
            (op(x) * cot).sum().backward()
        return x.grad.cpu()

    _check_d("default " + case, grad(), t(g["d_x64"]))
    with _exact():
        _check_f("exact " + case, grad(), t(g["d_x"]), t(g["d_x64"]))
    assert all(p.grad is None for p in op.parameters())


def _rdb_eager(x, sd, k, taps):
    a, pad = sd["lrelu.weight"], k // 2
    z1 = F.conv2d(x, sd["conv1.conv.weight"], padding=pad)
    x1 = E.prelu(z1, a)
    z2 = F.conv2d(torch.cat([x, x1], 1), sd["conv2.conv.weight"], padding=pad)
    x2 = E.prelu(z2, a)
    z3 = F.conv2d(torch.cat([x, x1, x2], 1), sd["conv3.conv.weight"], padding=pad)
    taps += [z1, z2, z3]
    return E.prelu(z3, a) * 0.333333 + x


@pytest.mark.parametrize("order", ["first", "last"])
def test_primitive_inside_a_chain(golden, order):
    """Cell_Chain = inp + ops(inp) with the op as first member (bwd_takes_res = False: the chain adds g itself) and as last member (the
    chain's residual rides in conv2's epilogue, behind the PReLU), at exact settings under bound F: against the float64 eager restatement of
    the chain, with the float32 run of the same restatement as the floor.
    The input is the first smooth feature that meets the margin rule of the fixtures: in float64 the pre-activations (two of SelfPath,
    three of the dense block) all keep 2e-5 and six times their own float32 error from zero -- PReLU's gradient jumps there."""
    from paif_amd.core.model_fusion_auto import Cell_Chain

    names = ["SelAttention_2_1", "Denseblocks_3_1"]
    if order == "last":
        names.reverse()
    chain = Cell_Chain(32, [(names[0], 0), (names[1], 1)], [1, 2]).eval()
    S.load_formula_weights(chain, salt=5)
    sel = [m._op for m in chain._ops if type(m._op).__name__ == "SelfPath"][0]
    gain = float(golden("gs_selfpath")["gain_k2"])
    sel.load_state_dict({k: t(v) for k, v in S.selfpath_state_dict(2, gain).items()}, strict=True)
    chain.to(_dev())
    sds = [{k: v.detach().double() for k, v in m._op.state_dict().items()} for m in chain._ops]
    sds32 = [{k: v.float() for k, v in sd.items()} for sd in sds]

    def eager(x, pre, sds=sds):
        y = x
        for name, sd in zip(names, sds):
            if name.startswith("Sel"):
                taps = {}
                y = E.selfpath(y, sd, 2, taps)
                pre += [taps["z1"], taps["z2"]]
            else:
                y = _rdb_eager(y, sd, 3, pre)
        return x + y

    B, H, W = 1, 9, 12
    for s in range(200):
        x64 = t(S.make_smooth_feature(40 + s, B, 32, H, W)).to(_dev()).double().requires_grad_(True)
        pre, pre32 = [], []
        ref = eager(x64, pre)
        with torch.no_grad():
            eager(x64.detach().float(), pre32, sds32)
        least = min(float(p.abs().min()) for p in pre)
        floor = max(float((a.double() - b).abs().max()) for a, b in zip(pre32, pre))
        if least >= 2e-5 and least >= 6 * floor:
            break
    else:
        raise AssertionError("no input with a margin")
    cot = t(S.make_feature(77, (B, 32, H, W))).to(_dev())
    (ref * cot.double()).sum().backward()
    x = x64.detach().float().requires_grad_(True)
    x32 = x64.detach().float().requires_grad_(True)
    ref32 = eager(x32, [], sds32)
    (ref32 * cot).sum().backward()
    with _exact(), ops.no_param_grads():
        y = chain(x)
        (y * cot).sum().backward()
    _check_f("chain out (%s)" % order, y.detach(), ref32.detach(), ref.detach())
    _check_f("chain d_x (%s)" % order, x.grad, x32.grad, x64.grad)


# ------------------------------------------------------------------------------------------------------------------------------
# 6: in the network
# ------------------------------------------------------------------------------------------------------------------------------
def _genotype():
    from paif_amd.genotypes import Genotype

    return Genotype(**SEL_GENOTYPE)


def _fusion_net():
    from paif_amd.core.model_fusion_auto import Network_Fusion_Searched

    net = Network_Fusion_Searched(32, None, _genotype()).eval()
    S.load_formula_weights(net)
    sel = net.chain._ops[0]._op
    assert type(sel).__name__ == "SelfPath"
    sel.load_state_dict({k: t(v) for k, v in S.selfpath_state_dict(2, 10.0).items()}, strict=True)
    return net.to(_dev()), sel


def test_network_forward_and_f16_storage():
    from oracle import paif_oracle as O

    net, sel = _fusion_net()
    ir, vis, _ = S.make_batch(1, 24, 32)
    irt, yt = t(ir).to(_dev()), O.rgb2ycrcb(t(vis))[:, 0:1].contiguous().to(_dev())
    with torch.no_grad():
        mine = net(irt, yt)
        ops.set_storage("f16")
        try:
            f16 = net(irt, yt)
        finally:
            ops.set_storage("f32")
    sd64 = {k: v.detach().double() for k, v in sel.state_dict().items()}

    def eager_nhwc(x, res=(), tape=None):
        y = E.selfpath(x.permute(0, 3, 1, 2).double(), sd64, 2).float().permute(0, 2, 3, 1).contiguous()
        for r in res:
            y = y + r
        return y

    sel.forward_nhwc = eager_nhwc
    try:
        with torch.no_grad():
            ref = net(irt, yt)
    finally:
        del sel.forward_nhwc
    _check_d("fused, op replaced by the eager restatement", mine, ref)
    err = float((f16.float() - mine).abs().max())
    print("f16 storage vs f32 storage: %.3e" % err)
    assert err <= 1.8e-3


def _mm_model():
    from paif_amd.core.model_fusion_auto import Network_MM_Searched

    m = Network_MM_Searched(32, _genotype(), None, None, "mit_b0", num_classes=9).eval()
    S.load_formula_weights(m)
    m.enhance_net.chain._ops[0]._op.load_state_dict({k: t(v) for k, v in S.selfpath_state_dict(2, 10.0).items()}, strict=True)
    return m.to(_dev())


def test_attack_iteration_runs_through_the_op():
    from paif_amd.attack.attack import attack_both

    m = _mm_model()
    ir, vis, lab = S.make_batch(1, 64, 96)          # (mit_b0's spatial reduction needs H, W >= 32)
    eps = 8 / 255.
    with torch.no_grad():
        d_ir, d_vis = attack_both(m, t(vis).to(_dev()), t(ir).to(_dev()), t(lab).to(_dev()), epsilon=eps, alpha=2 / 255., attack_iters=1,
                                  attack_loss='l_seg', attack_way='PGD')
    for d in (d_ir, d_vis):
        assert bool(torch.isfinite(d).all()) and float(d.abs().max()) <= eps + 1e-7
    assert float(d_ir.abs().max()) > 0 and float(d_vis.abs().max()) > 0


def test_graph_replay_is_bit_identical():
    from paif_amd.graph import GraphedForward

    m = _mm_model()
    ir, vis, _ = S.make_batch(1, 64, 96)
    g = GraphedForward(m, t(ir).to(_dev()), t(vis).to(_dev()))
    ir2, vis2, _ = S.make_batch(1, 64, 96, start=3)
    ir2, vis2 = t(ir2).to(_dev()), t(vis2).to(_dev())
    with torch.no_grad():
        f_e, s_e = m(ir2, vis2)
    f_g, s_g = g(ir2, vis2)
    assert torch.equal(f_e, f_g) and torch.equal(s_e, s_g)


# ------------------------------------------------------------------------------------------------------------------------------
# 7: refusals on device tensors
# ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_on_device(golden):
    op = _op(golden, 2)
    x = t(S.make_smooth_feature(11, 1, 32, 6, 7)).to(_dev()).requires_grad_(True)
    with pytest.raises(NotImplementedError, match="parameter gradients .* are not built -- freeze the parameters"):
        op(x)
    qkv = torch.zeros(1, 15, 384, device=_dev())
    with pytest.raises(TypeError, match="expected float32"):
        ops.self_attention(qkv.half(), 2)
    with pytest.raises(ValueError, match="192 \\* heads"):
        ops.self_attention(qkv, 3)
    L = ops.lib()
    assert L.paif_self_attention_workspace_bytes(1, (1 << 30) + 1, 1) == 0 and L.paif_self_attention_workspace_bytes(70000, 15, 2) == 0
    assert L.paif_self_attention_bwd_workspace_bytes(1, 15, 70000) == 0
    out = torch.zeros(1, 15, 128, device=_dev())
    p = lambda z: ctypes.c_void_p(z.data_ptr())
    rc = L.paif_self_attention_fwd(p(qkv), p(out), None, p(out), 70000, 15, 2, ops._stream())      # refused before any launch
    assert rc == -2 and b"not built" in L.paif_last_error()
