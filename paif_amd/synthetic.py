"""Deterministic synthetic inputs and formula weights (numpy only, portable).

No checkpoint or dataset of the reference is available (reference README.md:34-43 gives
Drive links only), so every parity case runs on inputs and weights produced by the
integer formulas below.  The same functions are used by the oracle's golden-vector
script (this container), by the GPU parity tests and by bench.py (GPU box), so both
sides see bit-identical float32 data without shipping any tensor files.

Input contract mirrored from the reference dataset class (TaskFusion_dataset2.py:74-104):
vis = RGB uint8 / 255 -> float32 [3,H,W]; ir = gray uint8 / 255 -> float32 [1,H,W];
label = int64 [H,W] in {0..8} (255 = ignore).
"""
import os
import zlib

import numpy as np

_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def splitmix64(x):
    """Vectorised splitmix64 finaliser on uint64 arrays."""
    with np.errstate(over="ignore"):
        x = (x + np.uint64(0x9E3779B97F4A7C15)) & _M64
        z = x
        z = ((z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & _M64
        z = ((z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & _M64
        z = z ^ (z >> np.uint64(31))
    return z


def hash_uniform(seed, n, offset=0):
    """n float64 values in [0,1) from a counter-based hash of (seed, index)."""
    idx = np.arange(offset, offset + n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        key = splitmix64(np.uint64(seed) * np.uint64(0x100000001B3) + idx)
    return (key >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def key_seed(name):
    """Stable 32-bit seed of a state_dict key (crc32 of its utf-8 name)."""
    return zlib.crc32(name.encode("utf-8")) & 0xFFFFFFFF


def formula_tensor(name, shape, salt=0):
    """Formula value for one state_dict entry, chosen by the key's suffix.

    * ``num_batches_tracked``           -> 0 (int64)
    * ``running_var``                   -> uniform [0.5, 1.5)
    * ``running_mean``                  -> uniform [-0.1, 0.1)
    * norm ``weight`` (1-D, LayerNorm/BatchNorm)  -> uniform [0.8, 1.2)
    * PReLU ``weight`` (shape (1,))     -> uniform [0.1, 0.3)
    * ``bias``                          -> uniform [-0.05, 0.05)
    * conv / linear ``weight``          -> uniform [-1, 1) * sqrt(3 / fan_in)   (unit-gain)
    """
    shape = tuple(int(s) for s in shape)
    n = int(np.prod(shape)) if len(shape) else 1
    seed = (key_seed(name) + 0x9E3779B1 * salt) & 0xFFFFFFFF
    if name.endswith("num_batches_tracked"):
        return np.zeros(shape, dtype=np.int64)
    u = hash_uniform(seed, n)
    if name.endswith("running_var"):
        v = 0.5 + u
    elif name.endswith("running_mean"):
        v = (u - 0.5) * 0.2
    elif name.endswith("bias"):
        v = (u - 0.5) * 0.1
    elif len(shape) == 1 and shape[0] == 1:
        v = 0.1 + 0.2 * u  # PReLU slope
    elif len(shape) == 1:
        v = 0.8 + 0.4 * u  # norm gain
    else:
        fan_in = int(np.prod(shape[1:]))
        v = (2.0 * u - 1.0) * np.sqrt(3.0 / fan_in)
    return v.astype(np.float32).reshape(shape)


def formula_state_dict(shapes, salt=0):
    """shapes: mapping key -> shape.  Returns key -> numpy array."""
    return {k: formula_tensor(k, s, salt) for k, s in shapes.items()}


# Calibrated segmentation head ---------------------------------------------------------------------------------------
# With formula weights everywhere the SegFormer head predicts ONE class on every pixel (the class means of its last layer
# swamp the spatial variation), which makes argmax / confusion-matrix / mIoU parity checks vacuous.  oracle/calibrate_head.py
# therefore fits `decoder.linear_pred.{weight,bias}` (core/segformer_head.py:57) per parity case by ridge regression of the
# synthetic labels on the REFERENCE's own head feature and stores the float32 table in synthetic_head.npz: with it the
# reference's argmax has all 9 classes (>= 5 % each), near-ties along every class boundary and a label-correlated map.
HEAD_KEYS = ("decoder.linear_pred.weight", "decoder.linear_pred.bias")
_HEAD_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "synthetic_head.npz")
_head_cache = {}


def head_tag(backbone, B, H, W):
    """Name of a calibration case: the backbone and the batch it was fitted on, e.g. 'mit_b3_1x480x640'."""
    return "%s_%dx%dx%d" % (backbone, B, H, W)


def calibrated_head(tag):
    """(weight [9,256,1,1], bias [9]) float32 of a calibration case, plus the reference's class shares on its inputs."""
    if not _head_cache:
        _head_cache.update(dict(np.load(_HEAD_FILE)))
    if tag + ".weight" not in _head_cache:
        raise KeyError("no calibrated head %r (have: %s)" % (tag, sorted(k[:-7] for k in _head_cache if k.endswith(".weight"))))
    return _head_cache[tag + ".weight"], _head_cache[tag + ".bias"], _head_cache[tag + ".class_share"]


def apply_head(state_dict, tag):
    """Overwrite the `...decoder.linear_pred.{weight,bias}` entries of a (numpy or torch) state_dict with a calibrated head."""
    w, b, _ = calibrated_head(tag)
    hit = 0
    for k in list(state_dict):
        for suffix, val in zip(HEAD_KEYS, (w, b)):
            if k.endswith(suffix):
                old = state_dict[k]
                if isinstance(old, np.ndarray):
                    state_dict[k] = val.copy()
                else:
                    import torch

                    state_dict[k] = torch.from_numpy(val.copy()).to(old.dtype)
                hit += 1
    if hit != 2:
        raise KeyError("state_dict has no decoder.linear_pred entries to calibrate")
    return state_dict


def load_formula_weights(module, salt=0, strict=True, head=None):
    """Fill a torch module's state_dict from the formula (strict key check); `head` = a calibration tag (head_tag(...))
    replaces the segmentation head's last layer by the fitted table."""
    import torch

    sd = module.state_dict()
    new = {k: torch.from_numpy(formula_tensor(k, tuple(v.shape), salt)).to(v.dtype) for k, v in sd.items()}
    if head is not None:
        apply_head(new, head)
    module.load_state_dict(new, strict=strict)
    return module


def selfpath_shapes(heads):
    """The ten state_dict entries of SelfPath(dim=32, num_heads=heads) (reference operations_m.py:90-112), in module order."""
    return {"conv.weight": (32, 32, 3, 3), "conv.bias": (32,), "conv2.weight": (32, 32, 3, 3), "conv2.bias": (32,),
            "cross_attn.to_qkv.weight": (192 * heads, 32), "cross_attn.to_out.0.weight": (32, 64 * heads),
            "cross_attn.to_out.0.bias": (32,), "norm1.weight": (32,), "norm1.bias": (32,), "prelu.weight": (1,)}


def selfpath_state_dict(heads, gain):
    """key -> float32 numpy array: what load_formula_weights(MixedOp(32, 'SelAttention_<heads>_1'), salt=13) gives its `_op`, with the q and
    k rows of to_qkv.weight (the first 128 * heads) times `gain` -- the bare formula weights leave the softmax flat (max p ~ 1 / N), so
    the fixtures of tools/make_golden_selfpath.py store one calibrated gain per head count."""
    sd = {k: formula_tensor("_op." + k, s, 13) for k, s in selfpath_shapes(heads).items()}
    sd["cross_attn.to_qkv.weight"][:128 * heads] *= np.float32(gain)
    return sd


# The ten convs of the U2Fusion baseline (reference fusion_model/U2Fusion.py:102-118) as (state_dict prefix, out channels, in channels):
# its 658,728 weights would not fit a committed fixture, so the fixtures store one fp32 scale per conv and one shift of the last bias.
U2FUSION_CONVS = ((("conv_1.0", 44, 2),) + tuple(("dense_layers.%d.conv.0" % i, 44, 44 * (i + 1)) for i in range(5))
                  + (("sub.0.0", 128, 264), ("sub.1.0", 64, 128), ("sub.2.0", 32, 64), ("sub.3", 1, 32)))


def u2fusion_state_dict(scales, shift):
    """key -> float32 numpy array: formula_tensor("u2/" + key) times the conv's scale (weight and bias alike), `shift` added to
    sub.3.bias.  tools/make_golden_u2fusion.py and the tests rebuild the fixture weights with this one expression."""
    scales = np.asarray(scales, dtype=np.float32)
    assert scales.shape == (len(U2FUSION_CONVS),)
    sd = {}
    for (name, cout, cin), s in zip(U2FUSION_CONVS, scales):
        sd[name + ".weight"] = formula_tensor("u2/" + name + ".weight", (cout, cin, 3, 3)) * s
        sd[name + ".bias"] = formula_tensor("u2/" + name + ".bias", (cout,)) * s
    sd["sub.3.bias"] = sd["sub.3.bias"] + np.float32(shift)
    return sd


# The thirty convs of the SeAFusion baseline (reference fusion_model/SeaFusion.py:86-104) in module order, as (state_dict prefix, out
# channels, in channels per group, kernel size, has a bias): the order of ops.seafusion_pack.  The depthwise pair of an RGBD has one
# input channel per group and no bias.
def _rgbd_convs(prefix, c, cout):
    return ((prefix + ".dense.conv1.conv", c, c, 3, True), (prefix + ".dense.conv2.conv", c, 2 * c, 3, True),
            (prefix + ".convdown.conv", cout, 3 * c, 1, True), (prefix + ".sobelconv.convx", c, 1, 3, False),
            (prefix + ".sobelconv.convy", c, 1, 3, False), (prefix + ".convup.conv", cout, c, 1, True))


SEAFUSION_CONVS = (sum((((s + "_conv.conv", 16, 1, 3, True),) + _rgbd_convs(s + "_rgbd1", 16, 32) + _rgbd_convs(s + "_rgbd2", 32, 48)
                        for s in ("vis", "inf")), ())
                   + (("decode4.conv", 64, 96, 3, True), ("decode3.conv", 32, 64, 3, True), ("decode2.conv", 16, 32, 3, True),
                      ("decode1.conv", 1, 16, 3, True)))
SEAFUSION_BN = (("decode4.bn", 64), ("decode3.bn", 32), ("decode2.bn", 16), ("decode1.bn", 1))   # owned, never applied


def seafusion_state_dict(scales, shift):
    """key -> numpy array (72 entries): formula_tensor("sea/" + key) times the conv's scale (weight and bias alike, the eight depthwise
    convs included: they are NOT the Sobel stencil), `shift` added to decode1.conv.bias, and formula values for the decoder's unused
    BatchNorm entries.  tools/make_golden_seafusion.py and the tests rebuild the fixture weights with this one expression."""
    scales = np.asarray(scales, dtype=np.float32)
    assert scales.shape == (len(SEAFUSION_CONVS),)
    sd = {}
    for (name, cout, cin, k, bias), s in zip(SEAFUSION_CONVS, scales):
        sd[name + ".weight"] = formula_tensor("sea/" + name + ".weight", (cout, cin, k, k)) * s
        if bias:
            sd[name + ".bias"] = formula_tensor("sea/" + name + ".bias", (cout,)) * s
    sd["decode1.conv.bias"] = sd["decode1.conv.bias"] + np.float32(shift)
    for name, c in SEAFUSION_BN:
        for leaf in ("weight", "bias", "running_mean", "running_var"):
            sd["%s.%s" % (name, leaf)] = formula_tensor("sea/%s.%s" % (name, leaf), (c,))
        sd[name + ".num_batches_tracked"] = formula_tensor("sea/" + name + ".num_batches_tracked", ())
    return sd


# The eleven Conv2d + BatchNorm2d blocks of the DIDFuse baseline (reference fusion_model/AUIF.py, class DID) in module order, as
# (nn.Sequential prefix, index of the conv in it, out channels, in channels, has a PReLU): the order of ops.didfuse_pack.  The conv is
# followed by its BatchNorm and, where there is one, the PReLU; cov1 and cov7 start with the ReflectionPad2d.
def _did_encoder(prefix):
    return ((prefix + ".cov1.cov1", 1, 64, 1, True), (prefix + ".cov2.cov2", 0, 64, 64, True), (prefix + ".cov3.cov3", 0, 64, 64, False),
            (prefix + ".cov4.cov4", 0, 64, 64, False))


DIDFUSE_CONVS = (_did_encoder("AE_Encoder1") + _did_encoder("AE_Encoder2")
                 + (("AE_Decoder1.cov5.cov5", 0, 64, 128, True), ("AE_Decoder1.cov6.cov6", 0, 64, 128, True),
                    ("AE_Decoder1.cov7.cov7", 1, 1, 128, False)))
DIDFUSE_SLOPES = (0.10, 0.15, 0.20, 0.25, 0.30, 0.35)   # the six PReLU slopes in module order


def didfuse_state_dict(scales, shift):
    """key -> numpy array (83 entries): formula_tensor("did/" + key) times the conv's scale (weight and bias alike), `shift` added to
    cov7's conv bias, formula values (not the identity) for the BatchNorm entries, and the six PReLU slopes set to DIDFUSE_SLOPES in module
    order (formula_tensor would take a one-element `weight` for a slope in [0.1, 0.3): the listed values are told apart more easily).
    tools/make_golden_didfuse.py and the tests rebuild the fixture weights with this one expression."""
    scales = np.asarray(scales, dtype=np.float32)
    assert scales.shape == (len(DIDFUSE_CONVS),)
    sd, slopes = {}, iter(DIDFUSE_SLOPES)
    for (prefix, k, cout, cin, prelu), s in zip(DIDFUSE_CONVS, scales):
        conv, bn = "%s.%d" % (prefix, k), "%s.%d" % (prefix, k + 1)
        sd[conv + ".weight"] = formula_tensor("did/" + conv + ".weight", (cout, cin, 3, 3)) * s
        sd[conv + ".bias"] = formula_tensor("did/" + conv + ".bias", (cout,)) * s
        for leaf in ("weight", "bias", "running_mean", "running_var"):
            sd["%s.%s" % (bn, leaf)] = formula_tensor("did/%s.%s" % (bn, leaf), (cout,))
        if cout == 1:   # BatchNorm2d(1): a one-element `weight` is a norm gain here, not a slope
            sd[bn + ".weight"] = (0.8 + 0.4 * hash_uniform(key_seed("did/" + bn + ".weight"), 1)).astype(np.float32)
        sd[bn + ".num_batches_tracked"] = formula_tensor("did/" + bn + ".num_batches_tracked", ())
        if prelu:
            sd["%s.%d.weight" % (prefix, k + 2)] = np.array([next(slopes)], dtype=np.float32)
    last = "AE_Decoder1.cov7.cov7.1.bias"
    sd[last] = sd[last] + np.float32(shift)
    return sd


# The fifteen Conv2d of the hand-designed Fusion_Network (reference core/model_fusion_auto.py:159-188, its two DRDB :118-158) in
# state_dict order, as (name, out channels, in channels, kernel size): the order of ops.drdb_pack.
def _drdb_convs(prefix):
    return tuple(("%s.Dcov%d" % (prefix, k), 32, 64 + 32 * (k - 1), 3) for k in range(1, 6)) + ((prefix + ".conv", 64, 224, 1),)


DRDB_CONVS = (("conv1", 64, 2, 3),) + _drdb_convs("DRDB1") + _drdb_convs("DRDB2") + (("conv2", 32, 64, 3), ("conv21", 1, 32, 3))
# Prefix of the formula keys.  The draw matters to the fixture tool: with most prefixes conv21's output is one-signed on the calibration planes
# (negative share under 0.2 or over 0.8), which tools/make_golden_drdb.py refuses; "hand/" (the hand-designed network) calibrates.
DRDB_PREFIX = "hand/"


def drdb_state_dict(scales, shift=0.0, last_scale=1.0):
    """key -> numpy array (31 entries, the reference's state_dict order): formula_tensor(DRDB_PREFIX + key) times the conv's scale (weight and
    bias alike); conv21's weight and bias are further multiplied by `last_scale` and `shift` is then added to its bias; relu.weight (the
    one PReLU slope) is the formula value, in [0.1, 0.3).  (shift, last_scale) = (0, 1) is weight set A of tools/make_golden_drdb.py (both
    clamps active), (0.5, 0.1) is set B (no pixel clamped).  The tool and the tests rebuild the fixture weights with this one expression."""
    scales = np.asarray(scales, dtype=np.float32)
    assert scales.shape == (len(DRDB_CONVS),)
    sd = {}
    for (name, cout, cin, k), s in zip(DRDB_CONVS, scales):
        sd[name + ".weight"] = formula_tensor(DRDB_PREFIX + name + ".weight", (cout, cin, k, k)) * s
        sd[name + ".bias"] = formula_tensor(DRDB_PREFIX + name + ".bias", (cout,)) * s
    sd["conv21.weight"] = sd["conv21.weight"] * np.float32(last_scale)
    sd["conv21.bias"] = sd["conv21.bias"] * np.float32(last_scale) + np.float32(shift)
    sd["relu.weight"] = formula_tensor(DRDB_PREFIX + "relu.weight", (1,))
    return sd


# Fusion_Network2 (reference core/model_fusion_auto.py:227-260).  FN2_CONVS: its sixteen Conv2d outside the gates, as DRDB_CONVS (the order
# of ops.fn2_pack); FN2_GATE_CONVS: per gate conv_du.0 and the two fcs (1x1, no bias).  FN2_SCALED: the 22 convs a calibration rescales.
FN2_CONVS = DRDB_CONVS[:13] + (("conv2", 1, 64, 3), ("conv3", 64, 64, 1), ("conv4", 64, 128, 1))
SKFF_D = 8       # max(int(64 / 8), 4)


def skff_convs(prefix, height=2, d=SKFF_D):
    return ((prefix + "conv_du.0", d, 64, 1),) + tuple(("%sfcs.%d" % (prefix, h), 64, d, 1) for h in range(height))


FN2_GATE_CONVS = skff_convs("skff.") + skff_convs("skff2.")
FN2_SCALED = FN2_CONVS + FN2_GATE_CONVS
FN2_PREFIX = "hand2/"


def skff_state_dict(scales, height=2, reduction=8, bias=False, prefix="", formula_prefix=FN2_PREFIX):
    """key -> numpy array of one SKFF(64, height, reduction, bias) in the reference's state_dict order: formula tensors, conv_du.0 times
    scales[0], fcs.h times scales[1 + h] (weight and bias alike); conv_du.1.weight (the PReLU slope) is the formula value."""
    d = max(int(64 / reduction), 4)
    sd = {}

    def conv(name, cout, cin, s):
        sd[prefix + name + ".weight"] = formula_tensor(formula_prefix + prefix + name + ".weight", (cout, cin, 1, 1)) * np.float32(s)
        if bias:
            sd[prefix + name + ".bias"] = formula_tensor(formula_prefix + prefix + name + ".bias", (cout,)) * np.float32(s)

    conv("conv_du.0", d, 64, scales[0])
    sd[prefix + "conv_du.1.weight"] = formula_tensor(formula_prefix + prefix + "conv_du.1.weight", (1,))
    for h in range(height):
        conv("fcs.%d" % h, 64, d, scales[1 + h])
    return sd


def fn2_state_dict(scales, shift=0.0, last_scale=1.0):
    """key -> numpy array (41 entries, the reference's state_dict order): formula_tensor(FN2_PREFIX + key) times the conv's scale (weight
    and bias alike; `scales` in FN2_SCALED order); conv2's weight and bias are further multiplied by `last_scale` and `shift` is then added
    to its bias; relu.weight and the gates' PReLU slopes are the formula values, in [0.1, 0.3).  The tool and the tests rebuild the fixture
    weights with this one expression."""
    scales = np.asarray(scales, dtype=np.float32)
    assert scales.shape == (len(FN2_SCALED),)
    by = {name: s for (name, _, _, _), s in zip(FN2_SCALED, scales)}

    def conv(sd, name, cout, cin, k):
        sd[name + ".weight"] = formula_tensor(FN2_PREFIX + name + ".weight", (cout, cin, k, k)) * by[name]
        sd[name + ".bias"] = formula_tensor(FN2_PREFIX + name + ".bias", (cout,)) * by[name]

    sd = {}
    for name, cout, cin, k in FN2_CONVS[:14]:
        conv(sd, name, cout, cin, k)
    sd["conv2.weight"] = sd["conv2.weight"] * np.float32(last_scale)
    sd["conv2.bias"] = sd["conv2.bias"] * np.float32(last_scale) + np.float32(shift)
    sd["relu.weight"] = formula_tensor(FN2_PREFIX + "relu.weight", (1,))
    for g in ("skff.", "skff2."):
        sd.update(skff_state_dict([by[g + "conv_du.0"], by[g + "fcs.0"], by[g + "fcs.1"]], prefix=g))
    for name, cout, cin, k in FN2_CONVS[14:]:
        conv(sd, name, cout, cin, k)
    return sd


# The BFFusion baseline (reference fusion_model/BFFusion.py, class BFFR).  BFFUSION_LAYERS: its 97 convs and linears in state_dict order,
# as (state_dict prefix of `.weight`, weight shape, has a bias, kind, BatchNorm prefix or None).  kind: "stem" (1 x 1, no activation),
# "dense" (LeakyReLU 0.2 / 0.1), "fconv" (BatchNorm + ReLU: the 32 BatchNorms that ARE applied), "q", "k", "v", "proj" (the attention's
# linears), "dec" (LeakyReLU 0.01; its `bn` is a member the reference never applies), "head" (tanh / 2 + 0.5).
BFFUSION_NB, BFFUSION_CIN, BFFUSION_HEADS = (16, 32, 64, 96), (16, 16, 32, 64), (4, 8, 8, 16)


def _bffusion_layers():
    out = []
    for tag in ("vi", "ir"):
        out.append(("conv1_%s.conv2d" % tag, (16, 1, 1, 1), True, "stem", "conv1_%s.bn" % tag))
        for l, (c, nb) in enumerate(zip(BFFUSION_CIN, BFFUSION_NB)):
            db = "DB%d_%s" % (l + 1, tag)
            out += [(db + ".conv1.conv", (c, c, 3, 3), True, "dense", None), (db + ".conv2.conv", (c, 2 * c, 3, 3), True, "dense", None),
                    (db + ".conv_down", (nb, 3 * c, 1, 1), True, "dense", None)]
    for l, dim in enumerate(BFFUSION_NB):
        for at in ("attn1", "attn2"):
            p = "fusion_block%d.%s" % (l + 1, at)
            for seq in ("conv_pre", "ffn"):
                for k in range(2):
                    f = "%s.%s.%d" % (p, seq, k)
                    out.append((f + ".conv2d", (dim, dim, 3, 3), True, "fconv", f + ".batch_norm"))
            out += [(p + ".wq1", (dim, dim), False, "q", None), (p + ".wk1", (dim, dim), False, "k", None),
                    (p + ".wv1", (dim, dim), False, "v", None), (p + ".end_proj1", (dim, dim), True, "proj", None)]
    nb = BFFUSION_NB
    for name, cin, cout in (("DB1_1", nb[0] + nb[1], nb[0]), ("DB2_1", nb[1] + nb[2], nb[1]), ("DB3_1", nb[2] + nb[3], nb[2]),
                            ("DB1_2", 2 * nb[0] + nb[1], nb[0]), ("DB2_2", 2 * nb[1] + nb[2], nb[1]), ("DB1_3", 3 * nb[0] + nb[1], nb[0])):
        out.append((name + ".conv2d", (cout, cin, 3, 3), True, "dec", name + ".bn"))
    out.append(("conv_out.conv2d", (1, nb[0], 1, 1), True, "head", None))
    return tuple(out)


BFFUSION_LAYERS = _bffusion_layers()


def bffusion_state_dict(scales, shifts=0.0):
    """key -> numpy array (386 entries, the reference's state_dict order): formula_tensor("bff/" + key) times the layer's scale (weight
    and bias alike), the layer's shift (one per layer, or one scalar for all) added to every element of its bias, and formula values -- not the identity -- for every BatchNorm (the 32 applied
    ones and the 8 `ConvLayer.bn` that are never applied) and LayerNorm entry.  tools/make_golden_bffusion.py and the tests rebuild the
    fixture weights with this one expression."""
    scales = np.asarray(scales, dtype=np.float32)
    shifts = np.broadcast_to(np.asarray(shifts, dtype=np.float32), scales.shape)
    assert scales.shape == (len(BFFUSION_LAYERS),)
    sd = {}

    def norm(prefix, c, batch):
        leaves = ("weight", "bias", "running_mean", "running_var") if batch else ("weight", "bias")
        for leaf in leaves:
            sd["%s.%s" % (prefix, leaf)] = formula_tensor("bff/%s.%s" % (prefix, leaf), (c,))
        if c == 1:      # a one-element `weight` is a norm gain here, not a slope
            sd[prefix + ".weight"] = (0.8 + 0.4 * hash_uniform(key_seed("bff/" + prefix + ".weight"), 1)).astype(np.float32)
        if batch:
            sd[prefix + ".num_batches_tracked"] = formula_tensor("bff/" + prefix + ".num_batches_tracked", ())

    for (name, shape, bias, kind, bn), s, sh in zip(BFFUSION_LAYERS, scales, shifts):
        if kind == "q":     # LayerNorm sits before the three linears in the state_dict
            norm(name[:-len("wq1")] + "norm1", shape[0], False)
        sd[name + ".weight"] = formula_tensor("bff/" + name + ".weight", shape) * s
        if bias:
            sd[name + ".bias"] = formula_tensor("bff/" + name + ".bias", (shape[0],)) * s + sh
        if bn is not None:
            norm(bn, shape[0], True)
    return sd


# --------------------------------------------------------------------------------------
# inputs
# --------------------------------------------------------------------------------------
def _smooth_field(seed, H, W, freqs=((1, 1), (2, 3), (5, 2), (3, 7))):
    """Natural-image-like smooth uint8 field + hash noise (guided-filter sensitivity grows in
    flat regions, so plain white noise would be the wrong test signal)."""
    yy = np.arange(H, dtype=np.float64)[:, None] / H
    xx = np.arange(W, dtype=np.float64)[None, :] / W
    ph = hash_uniform(seed, 3 * len(freqs))
    f = np.zeros((H, W), dtype=np.float64)
    for i, (fy, fx) in enumerate(freqs):
        amp = 0.5 + ph[3 * i]
        f += amp * np.sin(2 * np.pi * (fy * yy + ph[3 * i + 1])) * np.cos(2 * np.pi * (fx * xx + ph[3 * i + 2]))
    f = (f - f.min()) / (f.max() - f.min() + 1e-12)
    # blocky objects (edges) + noise
    by = (np.arange(H)[:, None] * 7 // max(H, 1)) % 2
    bx = (np.arange(W)[None, :] * 9 // max(W, 1)) % 2
    f = 0.70 * f + 0.18 * (by ^ bx)
    noise = hash_uniform(seed ^ 0x5BD1E995, H * W).reshape(H, W)
    f = f + 0.12 * (noise - 0.5)
    f = np.clip(f, 0.0, 1.0)
    return np.floor(f * 255.0 + 0.5).astype(np.uint8)


def make_pair(index, H=480, W=640):
    """One (ir [1,H,W], vis [3,H,W]) float32 pair in [0,1] = uint8/255, seeded by sample index."""
    ir = _smooth_field(1000 + 17 * index, H, W).astype(np.float32) / np.float32(255.0)
    vis = np.stack(
        [_smooth_field(2000 + 17 * index + c, H, W, freqs=((1, 2), (3, 1), (4, 5), (2, 6))) for c in range(3)], 0
    ).astype(np.float32) / np.float32(255.0)
    return ir[None], vis


def make_label(index, H=480, W=640, n_class=9, ignore=255):
    """Blocky 9-class label map, a few px = 255 to exercise ignore_index."""
    yy = np.arange(H)[:, None]
    xx = np.arange(W)[None, :]
    by = yy * 6 // H
    bx = xx * 8 // W
    lab = ((by * 5 + bx * 3 + index) % n_class).astype(np.int64)
    # a diagonal stripe of ignore pixels
    lab[((yy + xx + index) % 97) == 0] = ignore
    return lab


def make_batch(B, H=480, W=640, start=0):
    """Returns ir [B,1,H,W], vis [B,3,H,W] float32, label [B,H,W] int64."""
    irs, viss, labs = [], [], []
    for i in range(start, start + B):
        ir, vis = make_pair(i, H, W)
        irs.append(ir)
        viss.append(vis)
        labs.append(make_label(i, H, W))
    return np.stack(irs), np.stack(viss), np.stack(labs)


def make_delta0(index, shape, epsilon):
    """PGD start perturbation: counter-hash uniform in [-eps, eps) (replaces the reference's
    global-RNG ``uniform_`` at attack/attack.py:434,439 so both sides start identically)."""
    n = int(np.prod(shape))
    u = hash_uniform(0xD17A0000 + index, n)
    return ((2.0 * u - 1.0) * epsilon).astype(np.float32).reshape(shape)


def make_feature(seed, shape, lo=-1.0, hi=1.0):
    """Generic float32 feature tensor for per-operator tests."""
    n = int(np.prod(shape))
    return (lo + (hi - lo) * hash_uniform(seed, n)).astype(np.float32).reshape(shape)


def make_smooth_feature(seed, B, C, H, W):
    """Smooth multi-channel feature (uint8-quantised field per channel, affine-mixed)."""
    out = np.zeros((B, C, H, W), dtype=np.float32)
    for b in range(B):
        for c in range(C):
            f = _smooth_field(seed + 131 * b + 7 * c, H, W).astype(np.float32) / np.float32(255.0)
            out[b, c] = f * np.float32(0.5 + 0.03 * c) - np.float32(0.1 * (c % 5))
    return out


def sample_indices(n, k=512):
    """Up to k evenly spaced flat indices into a tensor of n elements (golden fixtures keep a sample of the big
    gradient / parameter tensors, not all 4 M values)."""
    if n <= k:
        return np.arange(n, dtype=np.int64)
    return np.unique(np.linspace(0, n - 1, k).astype(np.int64))
