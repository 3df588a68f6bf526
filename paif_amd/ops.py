"""Thin host wrappers: torch CUDA tensors -> raw pointers -> libpaif_hip.so (include/paif_hip.h).

torch supplies device memory (caching allocator, zero fills / memsets, copies), the current HIP stream and the autograd
graph nodes; the arithmetic of the path -- forward, input gradients, parameter gradients, optimizer -- runs in the
hand-written gfx950 kernels of libpaif_hip.so.  What is left to torch ops, all outside the hot loops:
  * scalar bookkeeping on 1-2 element device tensors (1/#valid pixels of the CE, stacking two loss weights, the
    BatchNorm `num_batches_tracked` counter, the optional 2-float global min/max exchange);
  * the loss glue of the attack variants neither entry script uses by default (segPGD / cosPGD / newPGD masks and cosine
    similarity, `trans_format` of the never-called single-modality attacks): torch ops on top of the HIP autograd nodes;
  * a user-supplied seg_loss that is not a plain CrossEntropyLoss.
Internal activation layout is NHWC ([B,H,W,C] contiguous float32).  `to_nhwc` / `to_nchw_view` convert at the module
boundary: an NHWC tensor viewed as [B,C,H,W] is exactly torch's channels_last format, so the reference's NCHW operator API
is kept without copies between our own ops.
"""
import ctypes
import weakref
import os

import torch

from . import _lib

ACT_NONE, ACT_PRELU, ACT_RELU = 0, 1, 2
ACT_GELU = 1  # paif_gemm_fwd's act code 1 is GELU (the conv's code 1 is PReLU)

# Arithmetic of the dense k x k convs (cin = 32):
#   "f32"    -- v_mfma_f32_32x32x2_f32, bit-exact fp32 products (parity ~1e-6 vs the fp32 reference)
#   "bf16x3" -- split-bf16: hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_bf16, fp32 accumulate
#               (~1e-5 relative; 5.3x less matrix-pipe time -> the convs become HBM-bound)
# Arithmetic of the SegFormer GEMMs: "f32" | "bf16x3" | "auto" (default): split-bf16 only for the shapes whose exact-fp32 GEMM is
# matrix-pipe bound (K >= 256: MiT stages 3-4, fc2, SR convs), exact fp32 for the others; the attention products follow (split-bf16
# unless "f32").  Measured on the 480x640 mit_b3 golden (tools/gpu_check_gemm_auto.py): logits max|d| from the reference's fp64 run
# 1.8e-5 (f32) / 2.2e-5 (auto) / 4.2e-5 (bf16x3) against the reference's own fp32 floor of 3.8e-5, argmax agreement 100 % in all three.
# With the round-2 kernels split-bf16 is the faster GEMM for every shape without split-K (tools/gemm_shapes_b16.py: another ~2 % on
# configs[2]); "auto" keeps K < 256 exact because that is what keeps the default inside the reference's own fp32 noise floor.
#
# Arithmetic of the ATTACKS (attack_both / attack_vis / attack_ir and the single-modality variants), CONFIG["attack_precision"]:
#   "bf16x6" (DEFAULT) -- the whole attack loop (taped forward AND input-gradient reverse pass) at fp32-level precision, whatever the two
#              settings above say.  Reverse pass: convs, the K >= 256 GEMMs and (round 5) the attention products as three-piece bf16
#              splits (six MFMAs per product, 2^-25 per product).  Forward pass (round 5, CONFIG["attack_fwd_f16x3"]): the convs and those
#              GEMMs as fp16 PAIRS -- two 11-bit pieces per operand, three fp16 MFMAs per product, the weight side pre-scaled by 2^8 --
#              whose error against float64 measures at or below the exact fp32 MFMA's on O(1) data (tools/f16x3_check.py); attention
#              three-piece.  The other GEMMs on the exact-fp32 kernel.  SURVEY 8(a) A1 (sign mismatch <= 1e-3 per iteration) HOLDS:
#              measured sign mismatch against the reference's float64 run 0 in every iteration through PGD-10 (also with the split
#              GEMMs forced at the test's small size: tests/test_parity_default_gpu.py);
#   "exact"  -- opt-in: every kernel of the loop fp32-exact (fp32 MFMA, 157 TF): A1 holds (0 ... 8e-5 at iteration 10), 20 % slower;
#   "fast"   -- opt-in: the settings above stay in force inside the loop (split-bf16 conv products, ~1e-5 relative): sign(running
#              gradient sum) is a chaotic map and 2.4e-4 of the elements sit on the other side of zero in iteration 1, 2.5e-2 by
#              iteration 10 (differing delta elements 5.3 %, loss trajectory 3.3e-3; the reference's own float32-vs-float64
#              disagreement: 0 / 4.1e-4 / 0.13 % / 6e-5) -- A1 holds for the first three iterations only.
# Measured in round 3 (tests/test_parity_default_gpu.py, tools/pgd_precision_sweep.py; PGD-10, 2x64x96, mit_b0).
#
# Activation STORAGE of the fusion network's inference forward (BASELINE configs[1] names "bf16"): "f32" (default: every map
# fp32, parity at the fp32 tolerance) or "bf16": the 32-channel maps behind the guided-filter block (everything from the two
# decomposition 1x1 convs to the tail) are held as bf16 -- half the HBM bytes of a pipeline that is bandwidth / latency bound --
# with fp32 accumulation and split-bf16 weights unchanged; the stems, the guided filter (statistics, A = cov/(var+eps), b, LF)
# and every 1-channel plane stay fp32 (SURVEY hard part 1).  Taped (gradient) passes always run fp32 storage.  Tolerance of this
# mode: SURVEY 8(d) bf16 clause (max / mean |fused - reference| reported, argmax agreement >= 99.9 %, mIoU within 0.1 pt):
# tests/test_bf16_storage_gpu.py.
def _env_switch(name, default="1"):
    """A/B switch from the environment: 0 / 1, or "gemm" (the GEMMs only) for the attack loops' fp16-pair arithmetic."""
    v = os.environ.get(name, default)
    if v not in ("0", "1", "gemm"):
        raise ValueError("%s=%r: expected 0, 1 or gemm" % (name, v))
    return {"0": False, "1": True, "gemm": "gemm"}[v]


GEMM_PRECISIONS = ("f32", "bf16x3", "auto", "bf16x6", "auto6", "f16x3", "auto6h")


def _env_gemm_precision():
    v = os.environ.get("PAIF_GEMM_PRECISION", "auto")
    if v not in GEMM_PRECISIONS:
        raise ValueError("PAIF_GEMM_PRECISION=%r: expected one of %s" % (v, GEMM_PRECISIONS))
    return v


CONFIG = {"conv_precision": "bf16x3", "gemm_precision": _env_gemm_precision(), "serpentine": True, "attack_precision": "bf16x6", "storage": "f32",
          # inference forward of the fusion network: run the infrared and the visible stream on two HIP streams (identical results; off by
          # default because per-launch timings -- bench.py's roofline blocks, rocprofv3 averages -- then measure CU sharing, not kernels)
          "two_stream": False,
          # inference forward, 16-bit storage, single-stream mode: the two streams' stems run as ONE launch (stem_pair) and their guided
          # filters as one joint batch of 2B images (guided_filter_pair(bsplit=B)) -- identical bits, fewer launches; False = two launches each
          "stream_pair": True,
          # round 5: ChannelPool(ir_feature, vis_feature) from the producing convs' epilogues (paif_conv_desc.cpool) instead of a pass of its own;
          # fp16 storage: the forward's last 32-channel map as fp32 / the folded 1x1 with fp16 hi + lo weights (ablation switches)
          "cpool_fused": True, "f16_last_f32": True, "f16_decomp_split": False,
          # round 6, fp16 storage, OPT-IN: the stem writes its map as fp16 only and the guided filter reads that (no fp32 stem map).  Measured:
          # +1.3 % pairs/s (2,330 -> 2,360) for argmax agreement 99.942 % -> 99.920 % over 32 samples, the lower end of the bootstrap interval
          # 99.928 % -> 99.897 % (profiles/r06_f16_storage_report*.json): it would spend the clause's margin, so it stays off
          "gf_in_f16": os.environ.get("PAIF_GF_IN_F16", "0") == "1",
          # 16-bit inference forward: a ResidualDenseBlock (k = 3, dilation 1) as ONE kernel (csrc/rdb_fused.hip) on maps of >= 512 tiles.
          # OFF by default: correct (tests/test_f16_storage_gpu.py) and 2 map passes instead of 9, but matrix-pipe bound at the clock the chip
          # sustains under that load -- 400 us per block inside the forward against 355 for the three bandwidth-bound launches
          "rdb_fused": False, "gemm2": False, "timer_torch_events": os.environ.get("PAIF_TIMER_TORCH_EVENTS", "0") == "1", "infer_f16x3": os.environ.get("PAIF_INFER_F16X3", "1") != "0", "wgrad_f16x3": os.environ.get("PAIF_WGRAD_F16X3", "1") != "0", "_wgrad_scale": None, "gemm_split_min_m": 2048, "f16x3_min_k": int(os.environ.get("PAIF_F16X3_MIN_K", "32")), "attack_bwd_f16x3": _env_switch("PAIF_ATTACK_BWD_F16X3"),
          "attack_grad_scale_log2": (int(os.environ["PAIF_ATTACK_GSCALE"]) if "PAIF_ATTACK_GSCALE" in os.environ else None),
          "attack_fwd_f16x3": _env_switch("PAIF_ATTACK_FWD_F16X3"), "attn_x6": os.environ.get("PAIF_ATTN_X6", "1") != "0", "attn_f16x3": os.environ.get("PAIF_ATTN_F16X3", "1") != "0", "gemm_gather": os.environ.get("PAIF_GEMM_GATHER", "1") != "0"}
# falsy, or the torch dtype (torch.bfloat16 / torch.float16) of the 32-channel maps while an inference forward of the fusion network
# runs in a 16-bit storage mode (set by the model through `bf16_activations`)
_ACT_BF16 = [False]
H16 = (torch.bfloat16, torch.float16)     # dtypes of 16-bit-stored maps


STORAGE_MODES = ("f32", "bf16", "bf16_split", "f16")


def set_storage(mode):
    """Activation storage of the fusion network's inference forward.
    "f32":        fp32 maps, split-bf16 products (3 bf16 MFMAs, fp32-level parity) -- the API default.
    "bf16":       BASELINE configs[1]: bf16 maps AND bf16 weights, one bf16 MFMA per product, fp32 accumulate (PAIF_CONV_BF16).
    "bf16_split": bf16 maps, weights kept as split-bf16 hi + lo (2 MFMAs per product: only the maps are rounded).
    "f16":        round 5 -- the 16-bit configuration that meets SURVEY 8(d)'s argmax clause: IEEE fp16 maps (11 significant bits where
                  bf16 has 8) and fp16 weights, one fp16 MFMA per product, fp32 accumulate; the guided filter writes HF = x - LF (small
                  magnitudes) and the 1x1 behind it folds over [x, HF1, HF2]; the forward's last 32-channel map (the input of
                  stem_out) stays fp32.  Why: tools/storage_sensitivity.py, tools/f16_ablation.py, DESIGN section 2."""
    if mode not in STORAGE_MODES:
        raise ValueError("storage must be one of %s" % (STORAGE_MODES,))
    CONFIG["storage"] = mode


def pack_precision():
    """Arithmetic a weight pack built NOW is for: "f16" inside an fp16-storage inference forward, else CONFIG['conv_precision']."""
    return "f16" if _ACT_BF16[0] is torch.float16 else CONFIG["conv_precision"]


class bf16_activations:
    """Context of the fusion network's inference forward: conv outputs (and what is computed from them) are bf16 maps."""

    def __init__(self, enable=True):
        self.enable = enable

    def __enter__(self):
        self.old = _ACT_BF16[0]
        on = self.enable and CONFIG["storage"] in ("bf16", "bf16_split", "f16") and CONFIG["conv_precision"] == "bf16x3"
        _ACT_BF16[0] = (torch.float16 if CONFIG["storage"] == "f16" else torch.bfloat16) if on else False

    def __exit__(self, et, *a):
        was_f16 = _ACT_BF16[0] is torch.float16
        _ACT_BF16[0] = self.old
        if not self.old:
            _TWINS.clear()
        if was_f16 and et is None and _F16_GUARD and not torch.cuda.is_current_stream_capturing():
            _f16_guard_poll(torch.cuda.current_device())


# ---- range guard of the fp16 storage mode ----
# IEEE fp16 stores |v| >= 65520 as inf.  Every 16-bit map of the inference forward reaches the forward's last map through convs and
# residual adds (`inp + ops(inp)` in every chain), which keep a non-finite value non-finite; the forward ends in tanh, which would turn it
# into a finite, wrong +-1.  The kernel in front of that tanh (stem_out) ORs one device word when its pre-activation is inf / NaN.
# The word is read WITHOUT stalling the stream: a forward leaves an async copy + event behind, the next forward (or check_f16_overflow())
# looks at it.  Formula weights keep every map O(1); a real checkpoint is not known to.
_F16_GUARD = {}     # device index -> dict(flag=int32[1] device, host=int32[1] pinned, event=Event or None)


def f16_guard_flag(device):
    g = _F16_GUARD.get(device.index)
    if g is None:
        g = _F16_GUARD[device.index] = dict(flag=torch.zeros(1, device=device, dtype=torch.int32),
                                            host=torch.zeros(1, dtype=torch.int32).pin_memory(), event=None, dirty=False)
    g["dirty"] = True
    return g["flag"]


def _f16_overflow_error():
    return FloatingPointError("fp16 storage: a 16-bit map of the fusion network's inference forward overflowed IEEE fp16's range (|v| >= 65520 "
                              "is stored as inf): the fused image of that forward is wrong.  Run this model with ops.set_storage(\"f32\") "
                              "(or \"bf16\": fp32's exponent range at 8 significant bits)")


def _f16_guard_poll(device_index):
    """End of an fp16-storage forward (not under graph capture): look at the previous forward's copy if it has landed, leave a new one."""
    g = _F16_GUARD.get(device_index)
    if g is None or not g["dirty"]:
        return
    ev = g["event"]
    if ev is not None:
        if not ev.query():
            return                       # the previous copy is still in flight: no second one queued behind it
        g["event"] = None
        if int(g["host"][0]) != 0:
            g["flag"].zero_()
            g["host"].zero_()
            raise _f16_overflow_error()
    g["host"].copy_(g["flag"], non_blocking=True)
    g["event"] = torch.cuda.Event()
    g["event"].record()
    g["dirty"] = False


def check_f16_overflow(device=None):
    """Synchronous form of the fp16 storage mode's range guard: waits for the stream, raises FloatingPointError if any fp16-storage forward
    since the last check overflowed (and clears the word).  Call it after a hipGraph replay, at the end of an evaluation loop, in tests."""
    idx = torch.cuda.current_device() if device is None else torch.device(device).index
    g = _F16_GUARD.get(idx)
    if g is None:
        return
    torch.cuda.synchronize(idx)
    g["event"] = None
    bad = int(g["flag"].item()) != 0 or int(g["host"][0]) != 0
    g["flag"].zero_()
    g["host"].zero_()
    g["dirty"] = False
    if bad:
        raise _f16_overflow_error()


_TWINS = {}    # data_ptr of an fp32 map -> (the map, its bf16 twin written by the producing kernel); lives for one bf16 forward
_SERP = [0]    # tile-direction parity of the next dense-conv launch
F16X3_WSCALE = 256.0    # csrc/gemm_mfma.hip / conv_mfma.hip: the exact power of two on the weight side of the fp16-pair arithmetic
_PREC_CODE = {"f32": 0, "bf16x3": 1, "bf16x6": 3, "f16": 4, "f16x2": 5, "f16x3": 6}    # include/paif_hip.h PAIF_CONV_*
PREC_BF16 = 2          # include/paif_hip.h PAIF_CONV_BF16 (conv descriptors with bf16-stored maps only)


def set_gemm_precision(mode):
    """Arithmetic of the SegFormer GEMMs: "f32" (exact fp32 MFMA), "bf16x3" (split-bf16: 3 bf16 MFMAs, ~1e-5 relative),
    or "auto": split-bf16 where the GEMM is matrix-pipe bound at fp32 (K >= 256 and M >= CONFIG["gemm_split_min_m"]), exact fp32 elsewhere."""
    if mode not in GEMM_PRECISIONS:
        raise ValueError("gemm precision must be one of %s" % (GEMM_PRECISIONS,))
    CONFIG["gemm_precision"] = mode


def set_conv_precision(mode):
    if mode not in _PREC_CODE:
        raise ValueError("conv precision must be one of %s" % sorted(_PREC_CODE))
    CONFIG["conv_precision"] = mode


def set_attack_precision(mode):
    """Arithmetic of the attack loops:
    "fp32level" (the default; stored as its pre-round-6 name "bf16x6", which is still accepted): fp32-level parity at a fraction of the
        exact kernels' matrix time -- the 32-channel convs, the GEMMs from 2,048 rows up and the attention products on fp16 PAIRS (two
        fp16 pieces per operand, 3 fp16 MFMAs per product, ~2^-21.5; CONFIG["attack_fwd_f16x3" / "attack_bwd_f16x3" / "attn_f16x3"];
        with those switches off: three-piece bf16 splits, 6 MFMAs, 2^-25), the smaller GEMMs on the exact fp32 MFMA;
    "exact": fp32-exact MFMA kernels everywhere;
    "fast": whatever set_conv_precision / set_gemm_precision select -- split-bf16 by default; ~1.25x faster, the trajectory diverges."""
    if mode == "fp32level":
        mode = "bf16x6"
    if mode not in ("exact", "bf16x6", "fast"):
        raise ValueError("attack precision must be 'exact', 'fp32level' (alias 'bf16x6') or 'fast'")
    CONFIG["attack_precision"] = mode


class attack_arithmetic:
    """Context of an attack loop: switches the conv / GEMM arithmetic to CONFIG['attack_precision'] -- "bf16x6" (the DEFAULT:
    three-piece bf16 splits for the convs and the K >= 256 GEMMs, exact fp32 MFMA for the rest; fp32-level parity), "exact" (opt-in:
    fp32-exact kernels everywhere) or "fast" (opt-in: leave set_conv_precision / set_gemm_precision in force)."""

    def __enter__(self):
        self.old = (CONFIG["conv_precision"], CONFIG["gemm_precision"])
        mode = CONFIG.get("attack_precision", "bf16x6")
        if mode == "exact":
            CONFIG["conv_precision"], CONFIG["gemm_precision"] = "f32", "f32"
        elif mode == "bf16x6":
            CONFIG["conv_precision"], CONFIG["gemm_precision"] = "bf16x6", "auto6"

    def __exit__(self, *a):
        CONFIG["conv_precision"], CONFIG["gemm_precision"] = self.old


class attack_forward_arithmetic:
    """Inside an attack loop, around the FORWARD pass only (CONFIG["attack_fwd_f16x3"]): the 32-channel convs and the K >= 256 GEMMs as fp16
    pairs (two 11-bit pieces per operand, three fp16 MFMAs per product, ~2^-21.5) instead of three bf16 pieces (six MFMAs, 2^-25).  The
    backward keeps the three-piece form: gradients span the bf16 exponent range."""

    def __enter__(self):
        self.old = (CONFIG["gemm_precision"], CONFIG["conv_precision"])
        if CONFIG["attack_fwd_f16x3"] and self.old[0] == "auto6":
            CONFIG["gemm_precision"] = "auto6h"
        if CONFIG["attack_fwd_f16x3"] in (True, "conv") and self.old[1] == "bf16x6":
            CONFIG["conv_precision"] = "f16x3"

    def __exit__(self, *a):
        CONFIG["gemm_precision"], CONFIG["conv_precision"] = self.old


class inference_gemm_arithmetic:
    """Around the segmentation network's inference forward (no tape; CONFIG["infer_f16x3"]): the "auto" rule of the GEMMs / attention /
    strided convs becomes "auto6h" -- fp16 pairs (two 11-bit pieces per operand, three fp16 MFMAs per product) from 2,048 rows up, for every
    k extent, instead of split-bf16 for K >= 256 and the exact fp32 MFMA below.  Error against float64 at the exact kernels' level (20x
    below split-bf16) at the same speed (configs[2] 746 vs 747 pairs/s on one box).  Activations of the path are O(1)-O(100), orders of
    magnitude inside fp16's range.  Taped forwards / reverse passes outside an attack loop keep "auto": unscaled gradients
    need the bf16 exponent range."""

    def __enter__(self):
        self.old = CONFIG["gemm_precision"]
        if CONFIG["infer_f16x3"] and self.old == "auto":
            CONFIG["gemm_precision"] = "auto6h"

    def __exit__(self, *a):
        CONFIG["gemm_precision"] = self.old


class attack_backward_arithmetic:
    """Inside an attack loop, around the REVERSE pass (CONFIG["attack_bwd_f16x3"]): fp16 pairs there too.  The reverse pass is linear in
    the upstream gradient, so the loop multiplies d(loss)/d(logits) by an exact power of two (attack_grad_scale: ~ the number of
    pixels the loss averages over, which brings the gradients to O(1)) and divides the input gradient by it -- bit-neutral in fp32
    arithmetic, and what puts the gradients inside fp16's exponent range."""

    def __enter__(self):
        self.old = (CONFIG["gemm_precision"], CONFIG["conv_precision"])
        if CONFIG["attack_bwd_f16x3"] and self.old[0] == "auto6":
            CONFIG["gemm_precision"] = "auto6h"
        if CONFIG["attack_bwd_f16x3"] in (True, "conv") and self.old[1] == "bf16x6":
            CONFIG["conv_precision"] = "f16x3"

    def __exit__(self, *a):
        CONFIG["gemm_precision"], CONFIG["conv_precision"] = self.old


def check_attack_range(*grads):
    """The fp16-pair arithmetic of the attack loops needs every matrix operand inside fp16's exponent range (|v| < 65504): activations
    are, by orders of magnitude, and the scaled gradients are for any sane model -- but nothing in the kernels enforces it, and an
    overflow becomes inf / NaN in the accumulated input gradient.  One reduction + host read per attack call (skipped while a hipGraph
    is being captured: run one eager call first); raises with the way out instead of returning a garbage perturbation."""
    if not (CONFIG["attack_fwd_f16x3"] or CONFIG["attack_bwd_f16x3"]) or CONFIG.get("attack_precision", "bf16x6") != "bf16x6":
        return
    if torch.cuda.is_current_stream_capturing():
        return
    ok = None
    for g in grads:
        f = torch.isfinite(g).all()
        ok = f if ok is None else ok & f
    if ok is not None and not bool(ok):
        raise FloatingPointError("attack loop: non-finite input gradient -- an operand left fp16's exponent range in the fp16-pair arithmetic "
                                 "(CONFIG['attack_grad_scale_log2'] = %r).  Lower that scale, or run the loop on three-piece bf16 splits: "
                                 "ops.CONFIG.update(attack_fwd_f16x3=False, attack_bwd_f16x3=False, attn_f16x3=False)"
                                 % (CONFIG["attack_grad_scale_log2"],))


_VALID_PIXELS = {}     # (data_ptr, numel, version) of a label tensor -> pixels that are not ignore_index (one host read per label tensor)


def attack_grad_scale(label, ignore_index=255):
    """The power of two the attack loops scale the reverse pass by (1.0 when the reverse pass stays on three-piece bf16 splits):
    2^(floor(log2 V) - 4) with V = the pixels the cross-entropy AVERAGES over -- the label's valid pixels, not its size (with
    most labels at ignore_index the mean over the valid pixels makes d(logits) 1 / V, not 1 / numel; scaling by numel would overflow).
    One small reduction + host read per label tensor (cached; while a hipGraph is being captured the cached value of the eager call that
    must precede a capture is used, the label's size if there is none)."""
    if not CONFIG["attack_bwd_f16x3"] or CONFIG.get("attack_precision", "bf16x6") != "bf16x6":
        return 1.0
    k = CONFIG["attack_grad_scale_log2"]
    if k is None:
        key = (label.data_ptr(), label.numel(), label._version)
        v = _VALID_PIXELS.get(key)
        if v is None:
            if torch.cuda.is_current_stream_capturing():
                v = label.numel()
            else:
                if len(_VALID_PIXELS) > 64:
                    _VALID_PIXELS.clear()
                v = _VALID_PIXELS[key] = max(1, int((label != ignore_index).sum()))
        k = max(0, int(v).bit_length() - 1 - 4)      # 2^floor(log2 V) / 16: |d logits| <= 1/16 after scaling
    return float(2 ** k)


# ---- what a taped forward records: "dgrad" = enough for the input-gradient pass (PGD attacks); "wgrad" = also what the
# parameter-gradient kernels need (layer inputs, pre-activations, BatchNorm statistics).  Set by the autograd nodes.
_TAPE_MODE = ["dgrad"]


class tape_mode:
    def __init__(self, mode):
        assert mode in ("dgrad", "wgrad")
        self.mode = mode

    def __enter__(self):
        self.old = _TAPE_MODE[0]
        _TAPE_MODE[0] = self.mode

    def __exit__(self, *a):
        _TAPE_MODE[0] = self.old


def taping_wgrad():
    return _TAPE_MODE[0] == "wgrad"


# attacks differentiate w.r.t. the INPUT only: inside this context the autograd nodes skip the parameter gradients
_NO_PARAM_GRADS = [0]


class no_param_grads:
    def __enter__(self):
        _NO_PARAM_GRADS[0] += 1

    def __exit__(self, *a):
        _NO_PARAM_GRADS[0] -= 1


def want_param_grads(module):
    """Parameter gradients are produced when autograd is recording, the caller is not an attack, and some parameter of
    the module requires grad."""
    return torch.is_grad_enabled() and _NO_PARAM_GRADS[0] == 0 and any(p.requires_grad for p in module.parameters())


# called by the reverse passes when a sub-module's parameter gradients are final (bucketed all-reduce hooks in here)
GRAD_READY = [None]


def grads_ready(module):
    if GRAD_READY[0] is not None:
        GRAD_READY[0](module)


class PackedWeight:
    """Packed MFMA B-operand stream + the precision it was packed for."""

    __slots__ = ("data", "precision")

    def __init__(self, data, precision):
        self.data, self.precision = data, precision


def lib():
    return _lib.load()


class KernelTimer:
    """HIP-event timing of selected kernel launches on the CURRENT stream (the stream every paif_amd
    kernel is launched on).  Used by bench.py for the live roofline figure; off by default."""

    def __init__(self, match, every=1):
        self.match = match          # predicate on the kernel tag
        self.every = max(1, int(every))   # time one matching launch in `every` (a pair of event records between two kernels costs
        self.seen = 0                     # ~3 us of idle GPU: 22 of them are ~2-3 % of a 3.5 ms step)
        self.records = []           # (tag, start_event, end_event, flops, bytes)
        self._events = []           # fence-less HIP events owned by this timer
        self.extra = {}             # tag -> bytes of residual-map reads (not part of the SURVEY 8(d) byte model)

    def start(self, tag):
        if not self.match(tag):
            return None
        self.seen += 1
        if (self.seen - 1) % self.every:
            return None
        return self._record()

    def _record(self):
        """One timing event on the current stream: a fence-less HIP event (csrc/timing.hip) unless CONFIG["timer_torch_events"]."""
        if CONFIG["timer_torch_events"]:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            return e
        ev = ctypes.c_void_p()
        _lib.check(lib().paif_timing_event_create(ctypes.byref(ev)), "timing_event_create")
        _lib.check(lib().paif_timing_event_record(ev, _stream()), "timing_event_record")
        self._events.append(ev)
        return ev

    def mark(self):
        """A timing event on the current stream, whatever the tag predicate says (tools that time a span of launches of their own)."""
        return self._record()

    @classmethod
    def elapsed_ms(cls, e0, e1):
        """Milliseconds between two mark()s; call after a synchronize."""
        return cls._elapsed(e0, e1)

    @staticmethod
    def _elapsed(e0, e1):
        if isinstance(e0, torch.cuda.Event):
            return e0.elapsed_time(e1)
        ms = ctypes.c_float()
        _lib.check(lib().paif_timing_event_elapsed_ms(e0, e1, ctypes.byref(ms)), "timing_event_elapsed_ms")
        return ms.value

    def __del__(self):
        try:
            for ev in self._events:
                lib().paif_timing_event_destroy(ev)
        except Exception:
            pass

    def stop(self, tag, e0, flops, nbytes, extra_bytes=0):
        """nbytes: algorithmic bytes on SURVEY 8(d)'s model (each distinct input map read once, the output written once; residual adds
        free); extra_bytes: what the launch moves on top of that by construction (residual maps read in the epilogue)."""
        if e0 is None:
            return
        e1 = self._record()
        self.records.append((tag, e0, e1, flops, nbytes))
        self.extra[tag] = self.extra.get(tag, 0) + extra_bytes

    def summary(self):
        """-> dict tag -> (launches, total_ms, total_flops, total_bytes); call after a synchronize."""
        out = {}
        for tag, e0, e1, fl, nb in self.records:
            n, ms, f, b = out.get(tag, (0, 0.0, 0, 0))
            out[tag] = (n + 1, ms + self._elapsed(e0, e1), f + fl, b + nb)
        return out


TIMER = None  # set to a KernelTimer to instrument launches


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    """Device pointer of a dense float32 CUDA tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("paif_amd ops need CUDA(HIP) tensors; got a %s tensor -- there is no CPU path" % t.device)
    if t.dtype != torch.float32:
        raise TypeError("expected float32, got %s" % t.dtype)
    if not t.is_contiguous():
        raise RuntimeError("expected a dense (contiguous) tensor, got strides %s for shape %s" % (t.stride(), tuple(t.shape)))
    return ctypes.c_void_p(t.data_ptr())


def _pa(t):
    """Device pointer of an activation map: dense float32, bfloat16 or float16 CUDA tensor (None -> NULL)."""
    if t is None:
        return None
    if t.dtype in H16:
        if not t.is_cuda or not t.is_contiguous():
            raise RuntimeError("expected a dense CUDA tensor")
        return ctypes.c_void_p(t.data_ptr())
    return _p(t)


def cast_storage(x, to):
    """Convert a map between fp32 and a 16-bit storage format (round to nearest even on the way down), as a HIP kernel.
    to: a torch dtype (float32 / bfloat16 / float16); True = the running forward's 16-bit dtype (bf16 outside one); False = float32."""
    want = to if isinstance(to, torch.dtype) else ((_ACT_BF16[0] or torch.bfloat16) if to else torch.float32)
    if x.dtype == want:
        return x
    if want in H16 and x.dtype == torch.float32:
        tw = _TWINS.get(x.data_ptr())
        if tw is not None and tw[0] is x and tw[1].dtype == want:     # the producer already wrote this map's 16-bit twin
            return tw[1]
    if x.dtype in H16 and want in H16:
        raise TypeError("cast_storage: %s -> %s is not built (one 16-bit format per forward)" % (x.dtype, want))
    assert x.numel() % 4 == 0
    out = torch.empty(x.shape, device=x.device, dtype=want)
    mode = {torch.bfloat16: 1, torch.float16: 2}[want] if want in H16 else (0 if x.dtype == torch.bfloat16 else 3)
    _lib.check(lib().paif_cast_storage_fwd(_pa(x.contiguous()), _pa(out), x.numel(), mode, _stream()), "cast_storage")
    return out


def require_no_grad(*tensors):
    """Entry points that are forward-only (no autograd node of their own): fail loudly rather than silently
    dropping gradients.  The differentiable entry points are the models' / operators' forward() (autograd nodes
    with hand-written reverse passes) and the loss functions."""
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise NotImplementedError(
            "paif_amd: this entry point is forward-only (it has no autograd node); call it under torch.no_grad(), or go "
            "through the model / operator forward().  There is deliberately no autograd/eager fallback.")


def to_nhwc(x):
    """[B,C,H,W] (any strides) -> dense [B,H,W,C]; free when x is already channels_last."""
    return x.permute(0, 2, 3, 1).contiguous()


def to_nchw_view(x):
    """dense [B,H,W,C] -> [B,C,H,W] view (channels_last strides), no copy."""
    return x.permute(0, 3, 1, 2)


# ---------------------------------------------------------------------------------------------
# colour / glue
# ---------------------------------------------------------------------------------------------
def rgb2ycrcb(rgb):
    rgb = rgb.contiguous()
    B, C, H, W = rgb.shape
    assert C == 3
    out = torch.empty_like(rgb)
    _lib.check(lib().paif_rgb2ycrcb_fwd(_p(rgb), _p(out), B, H, W, _stream()), "rgb2ycrcb")
    return out


def ycrcb2rgb(ycc):
    ycc = ycc.contiguous()
    B, C, H, W = ycc.shape
    assert C == 3
    out = torch.empty_like(ycc)
    _lib.check(lib().paif_ycrcb2rgb_fwd(_p(ycc), _p(out), B, H, W, _stream()), "ycrcb2rgb")
    return out


def recompose_clamp(fused, ycc):
    """fused [B,1,H,W] + chroma of ycc [B,3,H,W] -> (RGB clamped to [0,1] [B,3,H,W], per-block (min, max) partials)."""
    fused = fused.contiguous()
    ycc = ycc.contiguous()
    B, _, H, W = ycc.shape
    L = lib()
    partial = torch.empty(2 * L.paif_minmax_blocks(B, H, W), device=ycc.device, dtype=torch.float32)
    rgb = torch.empty_like(ycc)
    _lib.check(L.paif_recompose_clamp_fwd(_p(fused), _p(ycc), _p(rgb), _p(partial), B, H, W, _stream()), "recompose_clamp")
    return rgb, partial


def fused_to_uint8(fused, ycc):
    """fused [B,1,H,W], ycc [B,3,H,W] -> uint8 NHWC [B,H,W,3]: the reference's fused-image post-processing
    (test_original.py:181-197: recomposition, clamp, uint8, batch-global min-max in float64, uint8)."""
    rgb, partial = recompose_clamp(fused, ycc)
    B, _, H, W = rgb.shape
    out = torch.empty((B, H, W, 3), device=rgb.device, dtype=torch.uint8)
    _lib.check(lib().paif_fused_uint8_fwd(_p(rgb), _p(partial), partial.numel() // 2, ctypes.c_void_p(out.data_ptr()), B, H, W, _stream()),
               "fused_uint8")
    return out


def seg_input_from_fused(fused, ycc, return_minmax=False, minmax_sync=None):
    """fused [B,1,H,W], ycc [B,3,H,W] -> normalised SegFormer input [B,3,H,W] (batch-global min-max).
    minmax_sync (optional): callable (mn, mx) -> (mn, mx) on 0-d device tensors, e.g. dist_utils.global_minmax for the
    all-ranks min/max of the `global_minmax=True` mode."""
    fused = fused.contiguous()
    ycc = ycc.contiguous()
    B, _, H, W = ycc.shape
    L = lib()
    nblk = L.paif_minmax_blocks(B, H, W)
    partial = torch.empty(2 * nblk, device=ycc.device, dtype=torch.float32)
    rgb = torch.empty_like(ycc)
    _lib.check(L.paif_recompose_clamp_fwd(_p(fused), _p(ycc), _p(rgb), _p(partial), B, H, W, _stream()), "recompose_clamp")
    if minmax_sync is not None:
        mn, mx = minmax_sync(partial[:nblk].min(), partial[nblk:].max())    # two scalars cross the ranks
        partial, nblk = torch.stack([mn.reshape(()), mx.reshape(())]).contiguous(), 1
    mm = torch.empty(2, device=ycc.device, dtype=torch.float32)
    _lib.check(L.paif_minmax_normalize_fwd(_p(rgb), _p(partial), nblk, _p(rgb), _p(mm), B, H, W, _stream()),
               "minmax_normalize")
    return (rgb, mm) if return_minmax else rgb


def u8_to_planes(src):
    """uint8 [B,H,W,C] (or [B,H,W]) device bytes -> float32 [B,C,H,W] = src / 255."""
    if src.dim() == 3:
        src = src.unsqueeze(-1)
    assert src.dtype == torch.uint8 and src.is_cuda and src.is_contiguous()
    B, H, W, C = src.shape
    out = torch.empty((B, C, H, W), device=src.device, dtype=torch.float32)
    _lib.check(lib().paif_u8_to_planes_fwd(ctypes.c_void_p(src.data_ptr()), _p(out), B, H * W, C, _stream()), "u8_to_planes")
    return out


def u8_to_i64(src):
    assert src.dtype == torch.uint8 and src.is_cuda and src.is_contiguous()
    out = torch.empty(src.shape, device=src.device, dtype=torch.int64)
    _lib.check(lib().paif_u8_to_i64_fwd(ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(out.data_ptr()), src.numel(), _stream()), "u8_to_i64")
    return out


# ---------------------------------------------------------------------------------------------
# fusion network pieces (all NHWC)
# ---------------------------------------------------------------------------------------------
def _plane_view(img):
    """-> (img with dense planes, its batch stride in floats) for the stem kernels."""
    B, _, H, W = img.shape
    if img.dtype != torch.float32 or not img.is_cuda:
        raise RuntimeError("stem: need a float32 CUDA tensor")
    if img.stride(3) != 1 or img.stride(2) != W:
        img = img.contiguous()
    return img, (img.stride(0) if B > 1 else H * W)


def stem(img, w, prelu, want_guide=True):
    """img: [B,1,H,W] or a channel-0 view of [B,C,H,W] (dense planes, arbitrary batch stride)."""
    B, _, H, W = img.shape
    img, bstride = _plane_view(img)
    feat = None if (_ACT_BF16[0] is torch.float16 and CONFIG["gf_in_f16"]) else torch.empty((B, H, W, 32), device=img.device, dtype=torch.float32)
    guide = torch.empty((B, H, W), device=img.device, dtype=torch.float32) if want_guide else None
    if _ACT_BF16[0] is torch.float16 and CONFIG["gf_in_f16"]:
        # fp16 storage, round 6: the stem writes its map as fp16 ONLY (the guide still comes from the fp32 values); the guided filter reads
        # that map (HF = x16 - LF(x16), the x16 the folded 1x1 takes as its first source anyway) -- no fp32 stem map exists in this forward
        twin = torch.empty((B, H, W, 32), device=img.device, dtype=torch.float16)
        _lib.check(lib().paif_stem_fwd_twin_f16(ctypes.c_void_p(img.data_ptr()), bstride, _p(w), _p(prelu), None, _pa(twin), _p(guide),
                                                B, H, W, _stream()), "stem")
        return twin, guide
    if _ACT_BF16[0]:     # 16-bit storage: the bf16 / fp16 twin of the map, for the layers that take it as a residual input (cast_storage finds it)
        twin = torch.empty((B, H, W, 32), device=img.device, dtype=_ACT_BF16[0])
        fn = lib().paif_stem_fwd_twin_f16 if _ACT_BF16[0] is torch.float16 else lib().paif_stem_fwd_twin
        _lib.check(fn(ctypes.c_void_p(img.data_ptr()), bstride, _p(w), _p(prelu), _p(feat), _pa(twin), _p(guide),
                      B, H, W, _stream()), "stem")
        _TWINS[feat.data_ptr()] = (feat, twin)
        return feat, guide
    _lib.check(lib().paif_stem_fwd(ctypes.c_void_p(img.data_ptr()), bstride, _p(w), _p(prelu), _p(feat), _p(guide),
                                   B, H, W, _stream()), "stem")
    return feat, guide


def pair_halves(joint, B):
    """The two problems' halves of a joint [2B,...] tensor of a pair launch: dense views (problem 0 = images 0..B-1)."""
    return joint[:B], joint[B:]


def register_twin_halves(feat, twin, B):
    """_TWINS is keyed by data_ptr and checked by identity: the two half-views of a joint fp32 map must each find their half of the
    joint 16-bit twin (cast_storage).  -> the two registered half-views of feat."""
    halves = pair_halves(feat, B)
    for h, t in zip(halves, pair_halves(twin, B)):
        _TWINS[h.data_ptr()] = (h, t)
    return halves


def stem_pair(img0, w0, prelu0, img1, w1, prelu1):
    """stem(img0, w0, prelu0) and stem(img1, w1, prelu1) of one geometry as ONE launch.  -> (feat [2B,H,W,32], guide [2B,H,W], (f0, f1)):
    the joint map (fp32; the fp16 twin alone under CONFIG["gf_in_f16"]) and guide, problem p in images p*B .. p*B + B - 1, and the map's
    two half-views (registered with their 16-bit twins' halves in a 16-bit storage forward).  Bits of two stem() calls."""
    if img0.shape != img1.shape:
        raise ValueError("stem_pair: the two images differ in shape: %s / %s" % (tuple(img0.shape), tuple(img1.shape)))
    B, _, H, W = img0.shape
    img0, bs0 = _plane_view(img0)
    img1, bs1 = _plane_view(img1)
    dev, st = img0.device, _ACT_BF16[0]
    only16 = st is torch.float16 and CONFIG["gf_in_f16"]
    feat = None if only16 else torch.empty((2 * B, H, W, 32), device=dev, dtype=torch.float32)
    twin = torch.empty((2 * B, H, W, 32), device=dev, dtype=st) if st else None
    guide = torch.empty((2 * B, H, W), device=dev, dtype=torch.float32)
    _lib.check(lib().paif_stem_fwd_pair(ctypes.c_void_p(img0.data_ptr()), bs0, _p(w0), _p(prelu0), ctypes.c_void_p(img1.data_ptr()), bs1,
                                        _p(w1), _p(prelu1), _p(feat), _pa(twin), 0 if twin is None else 2 if st is torch.float16 else 1,
                                        _p(guide), B, H, W, _stream()), "stem_pair")
    if only16:
        return twin, guide, pair_halves(twin, B)
    return feat, guide, (register_twin_halves(feat, twin, B) if twin is not None else pair_halves(feat, B))


def channel_residue(x):
    B, H, W, C = x.shape
    assert C == 32
    g = torch.empty((B, H, W), device=x.device, dtype=torch.float32)
    _lib.check(lib().paif_channel_residue_fwd(_p(x), _p(g), B, H, W, _stream()), "channel_residue")
    return g


class GfTape:
    """What the guided filter's taped forward leaves for its reverse pass: mc [2,B,H,W,32] = (mean_y, cov) and the per-pixel guide
    statistics workspace (csrc/gf_taped.hip).  The round-1 kernels' tape is a plain [4,B,H,W,32] tensor (A_0, b_0, A_1, b_1)."""
    __slots__ = ("mc", "stats")

    def __init__(self, mc, stats):
        self.mc, self.stats = mc, stats


def guided_filter_joint_fits(B2, H, W):
    """True if guided_filter_pair(bsplit=...) takes a joint batch of B2 images on the engine the single calls run on."""
    return H > 9 and W > 9 and bool(lib().paif_guided_filter_fused_joint_fits(B2, H, W))


def guided_filter_pair(guide, y, eps=(0.001, 0.0001), want_ab=False, out_bf16=False, tape=None, bsplit=None):
    """Returns lf [2,B,H,W,32] for the two eps (r = 4) (and the coefficient maps ab [4,B,H,W,32] for the
    backward pass).  AssertionError if H or W <= 9, like the reference's guided_filter_pytorch.
    out_bf16 (inference, fused form): the two maps as bf16 -- the bf16 configuration's storage of the maps behind this block;
    out_bf16 = torch.float16 (the fp16 configuration): the two HIGH-frequency maps y - LF as fp16 instead (paif_hip.h
    paif_guided_filter_fused_fwd_hf16).
    bsplit (inference, fused form): guide / y are the JOINT tensors of two problems of one geometry (images 0..bsplit-1 and bsplit..B-1,
    the two streams of the fusion forward): one launch sequence for both, the f16-range fallback decided per problem -- each half of
    lf[e] holds the bits of its own call (one qualification: include/paif_hip.h)."""
    hf16 = out_bf16 is torch.float16
    out_bf16 = bool(out_bf16)
    B, H, W, C = y.shape
    assert C == 32
    assert H > 9 and W > 9, "guided filter needs H, W > 2r+1 = 9"
    L = lib()
    if not want_ab and CONFIG.get("gf_fused", True):
        lf = torch.empty((2, B, H, W, 32), device=y.device, dtype=torch.float16 if hf16 else torch.bfloat16 if out_bf16 else torch.float32)
        ws = torch.empty(L.paif_guided_filter_fused_workspace_floats(B, H, W), device=y.device, dtype=torch.float32)
        import os
        eng = os.environ.get("PAIF_GF_ENGINE")
        tag = ("gf_fused_kernel" if eng == "valu" else "gf2_kernel") + " (+ gf_guide_stats_kernel)"
        e0 = TIMER.start(tag) if TIMER is not None else None
        y16 = y.dtype == torch.float16
        if y16 and not hf16:
            raise NotImplementedError("guided filter: an fp16 target map is built for the fp16 configuration's high-frequency output only")
        fn = (L.paif_guided_filter_fused_fwd_hf16_y16 if y16 else L.paif_guided_filter_fused_fwd_hf16 if hf16 else
              L.paif_guided_filter_fused_fwd_bf16 if out_bf16 else L.paif_guided_filter_fused_fwd)
        if bsplit is not None:
            _lib.check(L.paif_guided_filter_fused_fwd_joint(_p(guide), _pa(y) if y16 else _p(y), _pa(lf), eps[0], eps[1], _p(ws), B, bsplit, H, W,
                                                            3 if y16 else 2 if hf16 else 1 if out_bf16 else 0, _stream()), "guided_filter_fused")
        else:
            _lib.check(fn(_p(guide), _pa(y) if y16 else _p(y), _pa(lf), eps[0], eps[1], _p(ws), B, H, W, _stream()), "guided_filter_fused")
        if e0 is not None:   # algorithmic traffic: guide + y read once, the two low-frequency maps written once; ~650 FLOP per pixel-channel
            TIMER.stop(tag, e0, 650 * B * H * W * 32, B * H * W * (4 + (2 if y16 else 4) * 32 + (2 if out_bf16 else 4) * 64))
        return lf
    assert not out_bf16, "bf16 low-frequency maps are an inference (fused-form) output"
    assert bsplit is None, "the joint batch of two problems is an inference (fused-form) call"
    lf = torch.empty((2, B, H, W, 32), device=y.device, dtype=torch.float32)
    import os
    # tape: "mc" / "ab" force the round-6 streaming pair / the round-1 pair (tests, A/B runs); default: streaming wherever it fits
    assert tape in (None, "mc", "ab"), tape
    if tape is None:
        tape = os.environ.get("PAIF_GF_TAPE")        # A/B knob: the round-1 pair and its four-map tape under the streaming reverse pass
        if tape not in (None, "mc", "ab"):
            raise ValueError("PAIF_GF_TAPE must be 'mc' or 'ab', got %r" % tape)
    if tape is None:
        tape = "mc" if os.environ.get("PAIF_GF_BWD") != "v1" and L.paif_guided_filter_taped_fits(B, H, W) else "ab"
    if want_ab and tape == "mc":
        # round 6: the streaming taped forward and its two-map tape (mean_y, cov) + the per-pixel guide statistics (csrc/gf_taped.hip)
        mc = torch.empty((2, B, H, W, 32), device=y.device, dtype=torch.float32)
        stats = torch.empty(L.paif_guided_filter_fused_workspace_floats(B, H, W), device=y.device, dtype=torch.float32)
        _lib.check(L.paif_guided_filter_taped_fwd(_p(guide), _p(y), _p(mc), _p(lf), eps[0], eps[1], _p(stats), B, H, W, _stream()),
                   "guided_filter_taped")
        return lf, GfTape(mc, stats)
    ab = torch.empty((4, B, H, W, 32), device=y.device, dtype=torch.float32)
    _lib.check(L.paif_guided_filter_ab_fwd(_p(guide), _p(y), _p(ab), eps[0], eps[1], B, H, W, _stream()), "guided_filter_ab")
    _lib.check(L.paif_guided_filter_lf_fwd(_p(guide), _p(ab), _p(lf), B, H, W, _stream()), "guided_filter_lf")
    return (lf, ab) if want_ab else lf


def pack_conv_weight(w, nsrc, cin, kh, precision=None):
    """w: [cout, nsrc*cin, kh, kh] -> packed MFMA B-operand stream (PackedWeight)."""
    cout = w.shape[0]
    assert tuple(w.shape) == (cout, nsrc * cin, kh, kh), (tuple(w.shape), nsrc, cin, kh)
    precision = precision or pack_precision()
    if cin != 32:
        precision = "f32"  # the split-bf16 kernel is built for 32-channel sources
    L = lib()
    nfl = L.paif_conv_wpk_floats(nsrc, cin, kh)
    wpk = torch.empty(nfl * 3 // 2 if precision == "bf16x6" else nfl, device=w.device, dtype=torch.float32)
    wc = w.detach().contiguous()
    if precision in ("f16", "f16x2"):      # fp16 hi | lo pieces; "f16" reads the hi pieces only (one MFMA per product)
        _lib.check(L.paif_pack_conv_weight_f16x2(_p(wc), _p(wpk), cout, nsrc, kh, _stream()), "pack_conv_weight_f16x2")
    elif precision == "f16x3":             # fp16 pairs on fp32 maps: the pieces of 2^8 * w (exact scale; the kernel undoes it on the accumulators)
        _lib.check(L.paif_pack_conv_weight_f16x2(_p(wc * F16X3_WSCALE), _p(wpk), cout, nsrc, kh, _stream()), "pack_conv_weight_f16x2")
    elif precision == "bf16x6":
        _lib.check(L.paif_pack_conv_weight_bf16x6(_p(wc), _p(wpk), cout, nsrc, kh, _stream()), "pack_conv_weight_bf16x6")
    elif precision == "bf16x3":
        _lib.check(L.paif_pack_conv_weight_bf16x3(_p(wc), _p(wpk), cout, nsrc, kh, _stream()), "pack_conv_weight_bf16x3")
    else:
        _lib.check(L.paif_pack_conv_weight(_p(wc), _p(wpk), cout, nsrc, cin, kh, _stream()), "pack_conv_weight")
    return PackedWeight(wpk, precision)


def compose_dw_pw_weight(dw, pw):
    """dw [C,1,k,k] (depthwise), pw [Co,C,1,1] -> [Co,C,k,k]: the dense kernel of conv1x1(dwconv(.)) (operations_m.py:494-506)."""
    C, _, k, _ = dw.shape
    Co = pw.shape[0]
    assert tuple(dw.shape) == (C, 1, k, k) and tuple(pw.shape) == (Co, C, 1, 1)
    out = torch.empty((Co, C, k, k), device=dw.device, dtype=torch.float32)
    _lib.check(lib().paif_compose_dw_pw_weight(_p(dw.detach().contiguous()), _p(pw.detach().contiguous()), _p(out), Co, C, k, _stream()),
               "compose_dw_pw_weight")
    return out


def compose_pw_conv_weight(pw, w):
    """w [Cm,Ci,k,k] (dense conv), pw [Co,Cm,1,1] (the 1x1 behind it) -> [Co,Ci,k,k]: the dense kernel of conv1x1(conv_kxk(.))
    (operations_m.py:451-464 ResidualModule)."""
    Cm, Ci, k, _ = w.shape
    Co = pw.shape[0]
    assert tuple(pw.shape) == (Co, Cm, 1, 1)
    out = torch.empty((Co, Ci, k, k), device=w.device, dtype=torch.float32)
    _lib.check(lib().paif_compose_pw_conv_weight(_p(pw.detach().contiguous()), _p(w.detach().contiguous()), _p(out), Co, Cm, Ci, k, _stream()),
               "compose_pw_conv_weight")
    return out


def pack_decomp1x1_weight(w, precision=None):
    assert tuple(w.shape) == (32, 128, 1, 1)
    precision = precision or CONFIG["conv_precision"]
    L = lib()
    nfl = L.paif_conv_wpk_floats(3, 32, 1)
    wpk = torch.empty(nfl * 3 // 2 if precision == "bf16x6" else nfl, device=w.device, dtype=torch.float32)
    wc = w.detach().contiguous()
    if precision == "f16x3":
        # the same fold as paif_pack_decomp1x1_weight_bf16x3 (one fp32 add / subtract per weight), then the fp16 pieces of 2^8 * w
        w2 = wc.view(32, 128)
        fold = torch.cat([w2[:, 64:96] + w2[:, 96:128], w2[:, 0:32] - w2[:, 64:96], w2[:, 32:64] - w2[:, 96:128]], dim=1).contiguous()
        _lib.check(L.paif_pack_conv_weight_f16x2(_p(fold * F16X3_WSCALE), _p(wpk), 32, 3, 1, _stream()), "pack_conv_weight_f16x2")
    elif precision == "bf16x6":
        _lib.check(L.paif_pack_decomp1x1_weight_bf16x6(_p(wc), _p(wpk), _stream()), "pack_decomp1x1_weight_bf16x6")
    elif precision == "bf16x3":
        _lib.check(L.paif_pack_decomp1x1_weight_bf16x3(_p(wc), _p(wpk), _stream()), "pack_decomp1x1_weight_bf16x3")
    else:
        _lib.check(L.paif_pack_decomp1x1_weight(_p(wc), _p(wpk), _stream()), "pack_decomp1x1_weight")
    return PackedWeight(wpk, precision)


def rdb_fused_pack(w1, w2, w3, dtype):
    """Weights of a ResidualDenseBlock (k = 3) for the one-kernel form (paif_rdb_fused_fwd): 16-bit 16x16x32-MFMA operands."""
    assert tuple(w1.shape) == (32, 32, 3, 3) and tuple(w2.shape) == (32, 64, 3, 3) and tuple(w3.shape) == (32, 96, 3, 3) and dtype in H16
    L = lib()
    wpk = torch.empty(L.paif_rdb_fused_wpk_floats(), device=w1.device, dtype=torch.float32)
    _lib.check(L.paif_rdb_fused_pack(_p(w1.detach().contiguous()), _p(w2.detach().contiguous()), _p(w3.detach().contiguous()), _p(wpk),
                                     int(dtype == torch.float16), _stream()), "rdb_fused_pack")
    return PackedWeight(wpk, "rdb_f16" if dtype == torch.float16 else "rdb_bf16")


def rdb_fused(x, wpk, prelu, alpha=0.333333, res=(), cpool=None):
    """ResidualDenseBlock forward on a 16-bit NHWC-32 map as ONE launch: out = P(c3([x, P(c1(x)), P(c2([x, x1]))])) * alpha + x + res...
    (operations_m.py:435-449); res: up to two more residual maps; cpool = (comp, offset) as in conv2d."""
    B, H, W, C = x.shape
    assert C == 32 and x.dtype in H16 and x.is_contiguous() and len(res) <= 2
    assert wpk.precision == ("rdb_f16" if x.dtype == torch.float16 else "rdb_bf16")
    res = [cast_storage(r, x.dtype) for r in res]
    out = torch.empty_like(x)
    cp = None
    if cpool is not None:
        comp, coff = cpool
        assert comp.dtype == torch.float32 and tuple(comp.shape) == (B, H, W, 4) and comp.is_contiguous() and coff in (0, 2)
        cp = ctypes.c_void_p(comp.data_ptr() + 4 * coff)
    if CONFIG.get("serpentine", True):
        _SERP[0] ^= 1
    tag = "rdb_fused_kernel"
    e0 = TIMER.start(tag) if TIMER is not None else None
    _lib.check(lib().paif_rdb_fused_fwd(_pa(x), _p(wpk.data), _p(prelu), float(alpha), _pa(res[0]) if len(res) > 0 else None,
                                        _pa(res[1]) if len(res) > 1 else None, _pa(out), cp, int(x.dtype == torch.float16),
                                        _SERP[0] if CONFIG.get("serpentine", True) else 0, B, H, W, _stream()), "rdb_fused")
    if e0 is not None:     # SURVEY 8(d) bytes of the three convs it replaces: x read by each (3), x1 twice, x2 once, three maps written
        px = B * H * W
        TIMER.stop(tag, e0, 2 * px * 9 * 32 * 32 * 6, px * 2 * 32 * 9, px * 2 * 32 * len(res))
    return out


def pack_decomp1x1_hf_weight(w):
    """The folded decomposition 1x1 of the fp16 forward: over [x, HF1, HF2] (the guided filter writes HF = x - LF), fp16 hi + lo
    pieces (precision "f16x2": two MFMAs per product -- this conv's weight rounding is the one that moves the segmentation argmax)."""
    assert tuple(w.shape) == (32, 128, 1, 1)
    L = lib()
    wpk = torch.empty(L.paif_conv_wpk_floats(3, 32, 1), device=w.device, dtype=torch.float32)
    _lib.check(L.paif_pack_decomp1x1_hf_weight_f16x2(_p(w.detach().contiguous()), _p(wpk), _stream()), "pack_decomp1x1_hf_weight_f16x2")
    # one fp16 MFMA per product like every other conv of the mode: on the real kernels the hi + lo form ("f16x2", CONFIG
    # "f16_decomp_split") buys nothing once the filter stores HF (tools/f16_ablation.py: 99.928 % vs 99.931 % over 8 samples, 23 us)
    return PackedWeight(wpk, "f16x2" if CONFIG.get("f16_decomp_split", False) else "f16")


def bn_fold(weight, bias, mean, var, eps):
    C = weight.shape[0]
    scale = torch.empty(C, device=weight.device, dtype=torch.float32)
    shift = torch.empty(C, device=weight.device, dtype=torch.float32)
    _lib.check(lib().paif_bn_fold(_p(weight.detach()), _p(bias.detach()), _p(mean), _p(var), eps, _p(scale), _p(shift), C, _stream()),
               "bn_fold")
    return scale, shift


IN_DPRELU, IN_DRELU, IN_SCALE = 3, 4, 5   # dgrad staging modes of paif_conv_desc.in_act


def conv2d_kernel_name(desc, B, H, W):
    """Kernel paif_conv2d_fwd runs for this descriptor / shape, as rocprofv3 lists it (e.g. 'conv_bf16x3_ms<3, 1, 2>')."""
    buf = ctypes.create_string_buffer(96)
    _lib.check(lib().paif_conv2d_kernel_name(ctypes.byref(desc), B, H, W, buf, len(buf)), "conv2d_kernel_name")
    return buf.value.decode()


def _launch_convs(pend):
    """Launch prepared conv descriptors [(desc, (B, H, W), (flops, bytes, residual bytes), keep-alive)]: two of one shape as ONE pair launch
    where paif_conv2d_fwd_pair has the form (and CONFIG["stream_pair"] is on), else one launch each.  KernelTimer: one start / stop per
    launch, a pair launch with the work of both problems."""
    L = lib()
    if len(pend) == 2 and pend[0][1] == pend[1][1] and CONFIG.get("stream_pair", True):
        (d0, (B, H, W), w0, _), (d1, _, w1, _) = pend
        buf = ctypes.create_string_buffer(96)
        if L.paif_conv2d_pair_kernel_name(ctypes.byref(d0), ctypes.byref(d1), B, H, W, buf, len(buf)) == 0:
            tag = buf.value.decode()
            e0 = TIMER.start(tag) if TIMER is not None else None
            _lib.check(L.paif_conv2d_fwd_pair(ctypes.byref(d0), ctypes.byref(d1), B, H, W, _stream()), "conv2d_pair")
            if e0 is not None:
                TIMER.stop(tag, e0, w0[0] + w1[0], w0[1] + w1[1], w0[2] + w1[2])
            return True
    for d, (B, H, W), work, _ in pend:
        e0 = None
        if TIMER is not None:   # name the kernel this launch takes, as rocprofv3 will list it
            tag = conv2d_kernel_name(d, B, H, W)
            e0 = TIMER.start(tag)
        _lib.check(L.paif_conv2d_fwd(ctypes.byref(d), B, H, W, _stream()), "conv2d")
        if e0 is not None:
            TIMER.stop(tag, e0, *work)
    return False


def conv2d_pair(kw0, kw1):
    """conv2d(**kw0) and conv2d(**kw1) -- two problems of one geometry, e.g. the same layer of the two image streams -- as ONE launch where
    the pair form exists (paif_conv2d_fwd_pair: the LDS-DMA 1x1, the LDS-DMA 3x3 tile kernel for 1, 2 sources or 3 sources + 1
    residual map); otherwise as the two single launches.  Same bits either way.  -> (out0, out1)."""
    pend = []
    o0 = conv2d(_defer=pend, **kw0)
    n0 = len(pend)
    o1 = conv2d(_defer=pend, **kw1)
    if n0 == 1 and len(pend) == 2:
        _launch_convs(pend)
    elif pend:          # one of the two was launched by conv2d itself (a request the pair form has not): the other one alone
        _launch_convs(pend)
    return o0, o1


def conv2d(srcs, wpk, kh, dil=1, cin=32, cout=32, in_act=ACT_NONE, in_prelu=None, scale=None, shift=None,
           act=ACT_NONE, prelu=None, alpha=1.0, res=(), pool=False, want_aux=False, in_aux=None, in_scale=None,
           in_alpha=1.0, epi_dact=0, epi_aux=None, out=None, out_f32=False, cpool=None, _defer=None):
    """Dense conv over the virtual concat of `srcs` (NHWC).  Returns out (and the per-tile pool partials /
    the saved pre-activation when asked).  in_act 3/4/5 + in_aux/in_scale/in_alpha and epi_dact/epi_aux are the
    activation-derivative hooks used when the same kernel runs a dgrad (include/paif_hip.h).
    cpool = (comp [B,H,W,4] fp32, offset 0 | 2): also write ChannelPool(out) = (max_c, mean_c) into comp[..., offset:offset+2] -- fused into
    the conv's epilogue where the kernel can (paif_conv2d_can_cpool), by the stand-alone pass behind it otherwise."""
    B, H, W, C = srcs[0].shape
    assert C == cin and 1 <= len(srcs) <= 3
    res = [r for r in res if r is not None]
    extra = res[3:]
    res = res[:3]
    # activation storage (include/paif_hip.h PAIF_ST_*): 16-bit sources (bf16 / fp16) -> output in the same format; fp32 sources -> bf16
    # output only for the 1x1 behind the guided-filter block while a bf16 inference forward is running; otherwise fp32.
    # out_f32 (a request, honoured where the kernel exists: fp16 sources, 3x3 dilation 2, one source): fp32 output from 16-bit sources
    # and residual maps -- the forward's last 32-channel map
    sdt = srcs[0].dtype
    src16 = sdt in H16
    assert all(s_.dtype == sdt for s_ in srcs), "mixed source storage"
    if out is not None:
        odt = out.dtype
    elif src16:
        want32 = (out_f32 and sdt == torch.float16 and kh == 3 and dil == 2 and len(srcs) == 1 and in_act == ACT_NONE and not pool and cout == 32
                  and wpk.precision == "f16")
        odt = torch.float32 if want32 else sdt
    else:
        odt = torch.bfloat16 if (_ACT_BF16[0] is torch.bfloat16 and kh == 1 and not want_aux and in_act < 3 and not epi_dact) else torch.float32
    out16 = odt in H16
    if src16:
        storage = (3 if out16 else 4) if sdt == torch.float16 else 1
        if not out16 and sdt != torch.float16:
            raise NotImplementedError("bf16 sources with an fp32 output are not built")
    else:
        storage = 0 if not out16 else 2
        if odt == torch.float16:
            raise NotImplementedError("fp32 sources with an fp16 output are not built (the fp16 forward hands the 1x1 fp16 maps)")
    if storage and (want_aux or in_act >= 3 or epi_dact or in_aux is not None):
        raise NotImplementedError("16-bit activation storage is built for the inference forward (no gradient hooks)")
    if wpk.precision == "f16x3" and storage:
        raise NotImplementedError("the fp16-pair conv arithmetic is built for fp32 maps")
    if (sdt == torch.float16) != (wpk.precision in ("f16", "f16x2")):
        raise RuntimeError("conv2d: fp16 maps need an fp16 weight pack and vice versa (sources %s, pack %s)" % (sdt, wpk.precision))
    if out is None:
        out = torch.empty((B, H, W, cout), device=srcs[0].device, dtype=odt)
    else:
        assert tuple(out.shape) == (B, H, W, cout) and out.is_contiguous()
    rdt = sdt if storage == 4 else odt                 # residual maps share the output's storage (fp16 in / fp32 out: the sources')
    res = [cast_storage(r, rdt) for r in res]
    extra = [cast_storage(r, odt) for r in extra]
    src_bf, out_bf = src16, out16                       # (byte accounting below)
    L = lib()
    d = _lib.ConvDesc()
    d.storage = storage
    for i in range(3):
        d.src[i] = _pa(srcs[i]) if i < len(srcs) else None
        d.res[i] = _pa(res[i]) if i < len(res) else None
    for r in res:
        assert tuple(r.shape) == (B, H, W, cout)
    d.nsrc, d.cin, d.wpk, d.kh, d.dil = len(srcs), cin, _p(wpk.data), kh, dil
    d.precision = _PREC_CODE[wpk.precision]
    if storage in (1, 2) and wpk.precision == "bf16x3" and CONFIG["storage"] == "bf16":
        d.precision = PREC_BF16            # plain bf16 weights: the hi half of the split-bf16 pack
    d.in_act, d.in_prelu = in_act, _p(in_prelu)
    d.scale, d.shift = _p(scale), _p(shift)
    d.act, d.prelu, d.alpha = act, _p(prelu), alpha
    d.out, d.cout = _pa(out), cout
    partial = None
    if pool:
        partial = torch.empty((L.paif_conv2d_blocks(B, H, W), 32), device=out.device, dtype=torch.float32)
    d.pool_partial = _p(partial)
    aux = torch.empty_like(out) if want_aux else None
    d.aux_out, d.in_aux, d.in_scale, d.in_alpha = _p(aux), _p(in_aux), _p(in_scale), in_alpha
    d.epi_aux, d.epi_dact = _p(epi_aux), epi_dact
    pool_after = None
    if cpool is not None:
        comp, coff = cpool
        assert cout == 32 and comp.dtype == torch.float32 and tuple(comp.shape) == (B, H, W, 4) and comp.is_contiguous() and coff in (0, 2)
        if not extra and CONFIG.get("cpool_fused", True) and L.paif_conv2d_can_cpool(ctypes.byref(d), B, H, W):
            d.cpool = ctypes.c_void_p(comp.data_ptr() + 4 * coff)
        else:
            pool_after = (comp, coff)
    if CONFIG.get("serpentine", True):     # consecutive dense-conv launches walk their tiles in opposite directions (paif_hip.h)
        _SERP[0] ^= 1
        d.reverse_tiles = _SERP[0]
    px = B * H * W
    # algorithmic work: 2*K*cout FLOP per output pixel; each source map read once, output written once
    eb_in, eb_out = (2 if src_bf else 4), (2 if out_bf else 4)
    eb_res = 2 if (res and res[0].dtype in H16) else 4
    work = (2 * px * kh * kh * cin * len(srcs) * cout, px * (eb_in * cin * len(srcs) + eb_out * cout), px * eb_res * cout * len(res))
    if _defer is not None and not extra and pool_after is None and not pool and not want_aux:
        # conv2d_pair: the descriptor is complete, the launch is the caller's (the tensors it points into travel with it)
        _defer.append((d, (B, H, W), work, (srcs, res, out, wpk, scale, shift, prelu, in_prelu)))
        return out
    _launch_convs([(d, (B, H, W), work, None)])
    for r in extra:  # more than 3 fused residuals: plain adds
        out = add(out, r)
    if pool_after is not None:
        channel_pool1(out, *pool_after)
    if pool and want_aux:
        return out, partial, aux
    if want_aux:
        return out, aux
    return (out, partial) if pool else out


def pack_conv_dgrad_weight(w, coff, cs, precision=None):
    """Forward weight w [Co, Ctot, k, k] -> packed weights of the dgrad conv w.r.t. source channels
    [coff, coff+cs): a k x k conv with cin = Co, cout = cs, rotated taps."""
    Co, Ctot, k, _ = w.shape
    wt = torch.empty((cs, Co, k, k), device=w.device, dtype=torch.float32)
    _lib.check(lib().paif_conv_weight_dgrad(_p(w.detach().contiguous()), _p(wt), Co, Ctot, k, coff, cs, _stream()), "conv_weight_dgrad")
    return pack_conv_weight(wt, 1, Co, k, precision)


def fold_decomp1x1_weight(w):
    wf = torch.empty((32, 96, 1, 1), device=w.device, dtype=torch.float32)
    _lib.check(lib().paif_fold_decomp1x1_weight(_p(w.detach().contiguous()), _p(wf), _stream()), "fold_decomp1x1_weight")
    return wf


def dwconv(x, w, k, dil, in_relu):
    B, H, W, C = x.shape
    assert C == 32
    out = torch.empty_like(x)
    fn = {torch.bfloat16: lib().paif_dwconv_fwd_bf16, torch.float16: lib().paif_dwconv_fwd_f16}.get(x.dtype, lib().paif_dwconv_fwd)
    _lib.check(fn(_pa(x), _p(w.detach().contiguous()), _pa(out), k, dil, int(in_relu), B, H, W, _stream()), "dwconv")
    return out


def channel_pool2(ir, vis):
    B, H, W, _ = ir.shape
    comp = torch.empty((B, H, W, 4), device=ir.device, dtype=torch.float32)
    assert ir.dtype == vis.dtype
    fn = {torch.bfloat16: lib().paif_channel_pool2_fwd_bf16, torch.float16: lib().paif_channel_pool2_fwd_f16}.get(ir.dtype, lib().paif_channel_pool2_fwd)
    _lib.check(fn(_pa(ir), _pa(vis), _p(comp), B, H, W, _stream()), "channel_pool2")
    return comp


def channel_pool1(x, comp, coff):
    """ChannelPool of ONE map into comp[..., coff:coff+2] (comp [B,H,W,4] fp32; coff 0 = the infrared half, 2 = the visible half)."""
    B, H, W, C = x.shape
    assert C == 32 and tuple(comp.shape) == (B, H, W, 4) and comp.dtype == torch.float32 and coff in (0, 2)
    fn = {torch.bfloat16: lib().paif_channel_pool1_fwd_bf16, torch.float16: lib().paif_channel_pool1_fwd_f16}.get(x.dtype, lib().paif_channel_pool1_fwd)
    _lib.check(fn(_pa(x), ctypes.c_void_p(comp.data_ptr() + 4 * coff), B, H, W, _stream()), "channel_pool1")
    return comp


def spa_blend(comp, w, ir, vis, want_scale=False):
    B, H, W, _ = ir.shape
    agg = torch.empty_like(ir)
    if ir.dtype in H16:
        assert not want_scale and vis.dtype == ir.dtype
        fn = lib().paif_spa_blend_fwd_f16 if ir.dtype == torch.float16 else lib().paif_spa_blend_fwd_bf16
        _lib.check(fn(_p(comp), _p(w.detach().contiguous()), _pa(ir), _pa(vis), _pa(agg), B, H, W, _stream()), "spa_blend")
        return agg
    scale = torch.empty((B, H, W), device=ir.device, dtype=torch.float32) if want_scale else None
    _lib.check(lib().paif_spa_blend_fwd(_p(comp), _p(w.detach().contiguous()), _p(ir), _p(vis), _p(agg), _p(scale), B, H, W, _stream()),
               "spa_blend")
    return (agg, scale) if want_scale else agg


def eca_finish(o, r, partial, w1d, k, prelu, save=False):
    B, H, W, _ = o.shape
    out = torch.empty_like(o)
    gate = torch.empty((B, 32), device=o.device, dtype=torch.float32)
    if o.dtype in H16:
        assert not save and r.dtype == o.dtype
        fn = lib().paif_eca_finish_fwd_f16 if o.dtype == torch.float16 else lib().paif_eca_finish_fwd_bf16
        _lib.check(fn(_pa(o), _pa(r), _p(partial), _p(w1d.detach().contiguous()), k, _p(prelu), _p(gate), _pa(out),
                                                  B, H, W, _stream()), "eca_finish")
        return out
    u = torch.empty_like(o) if save else None
    _lib.check(lib().paif_eca_finish_fwd(_p(o), _p(r), _p(partial), _p(w1d.detach().contiguous()), k, _p(prelu), _p(gate), _p(out),
                                         _p(u), B, H, W, _stream()), "eca_finish")
    return (out, u, gate) if save else out


ECA_ROWS_TAG = "eca_conv2_rows<0> + eca_scale_kernel + eca_conv2_rows<1>"     # the three launches of paif_eca_conv2_gated_fwd_f16


def eca_block_tail(r, wpk, k, w1d, prelu):
    """ECABasicBlock behind its conv1 (inference): PReLU(o * gate + r), o = conv_k(PReLU(r)), gate = sigmoid(conv1d(mean o)).
    fp16 maps with plain fp16 weights at the sizes paif_eca_conv2_gated_fits names (PAIF_ECA_ROWS): conv2 runs twice as a row-streaming
    kernel and o is never stored (csrc/conv_eca_rows.hip); everything else: conv2d(pool=True) + eca_finish.  Bit-identical either way."""
    B, H, W, C = r.shape
    L = lib()
    if r.dtype == torch.float16 and C == 32 and k == 3 and wpk.precision == "f16" and L.paif_eca_conv2_gated_fits(B, H, W):
        out = torch.empty_like(r)
        partial = torch.empty((L.paif_conv2d_blocks(B, H, W), 32), device=r.device, dtype=torch.float32)
        gate = torch.empty((B, 32), device=r.device, dtype=torch.float32)
        e0 = TIMER.start(ECA_ROWS_TAG) if TIMER is not None else None
        _lib.check(L.paif_eca_conv2_gated_fwd_f16(_pa(r), _p(wpk.data), _p(prelu), _p(partial), _p(w1d.detach().contiguous()), k, _p(prelu),
                                                  _p(gate), _pa(out), B, H, W, _stream()), "eca_conv2_gated")
        if e0 is not None:      # conv2 twice; r read twice, out written once (the partials and the gate are noise)
            px = B * H * W
            TIMER.stop(ECA_ROWS_TAG, e0, 2 * 2 * px * 9 * 32 * 32, px * 2 * 32 * 3)
        return out
    o, partial = conv2d([r], wpk, k, 1, in_act=ACT_PRELU, in_prelu=prelu, pool=True)
    return eca_finish(o, r, partial, w1d, k, prelu)


def eca_layer_fwd(x, w1d, k):
    """Stand-alone eca_layer.forward (operations_m.py:353-367) on an NHWC fp32 map: x * sigmoid(conv1d_k(avgpool(x))) -- the pooling
    kernel + the fused block's own finish kernel (zero residual, PReLU slope 1 = identity)."""
    B, H, W, C = x.shape
    assert C == 32 and x.dtype == torch.float32
    L = lib()
    chunks = L.paif_conv2d_blocks(1, H, W)
    partial = torch.empty((B, chunks, 32), device=x.device, dtype=torch.float32)
    _lib.check(L.paif_channel_sum_chunks_fwd(_p(x), _p(partial), chunks, B, H, W, _stream()), "channel_sum_chunks")
    one = torch.ones(1, device=x.device, dtype=torch.float32)
    return eca_finish(x, torch.zeros_like(x), partial, w1d, k, one)


def eca_bwd(dout, u, o, gate, w1d, k, prelu, want_partial=False):
    B, H, W, _ = o.shape
    L = lib()
    partial = torch.empty((B, L.paif_eca_bwd_blocks(H, W), 32), device=o.device, dtype=torch.float32)
    coef = torch.empty((B, 32), device=o.device, dtype=torch.float32)
    d_o, d_r = torch.empty_like(o), torch.empty_like(o)
    _lib.check(L.paif_eca_bwd_input(_p(dout), _p(u), _p(o), _p(gate), _p(w1d.detach().contiguous()), k, _p(prelu), _p(partial), _p(coef),
                                    _p(d_o), _p(d_r), B, H, W, _stream()), "eca_bwd")
    return (d_o, d_r, partial) if want_partial else (d_o, d_r)


def spa_blend_bwd(dagg, w, ir, vis, s, add_ir=None, add_vis=None, want_dpre=False):
    B, H, W, _ = ir.shape
    dpre = torch.empty((B, H, W), device=ir.device, dtype=torch.float32)
    d_ir, d_vis = torch.empty_like(ir), torch.empty_like(vis)
    _lib.check(lib().paif_spa_blend_bwd_input(_p(dagg), _p(w.detach().contiguous()), _p(ir), _p(vis), _p(s), _p(add_ir), _p(add_vis),
                                              _p(dpre), _p(d_ir), _p(d_vis), B, H, W, _stream()), "spa_blend_bwd")
    return (d_ir, d_vis, dpre) if want_dpre else (d_ir, d_vis)


def dwconv_bwd(dt, w, k, dil, aux=None, add=None):
    B, H, W, _ = dt.shape
    out = torch.empty_like(dt)
    _lib.check(lib().paif_dwconv_bwd_input(_p(dt), _p(w.detach().contiguous()), _p(aux), _p(add), _p(out), k, dil, B, H, W, _stream()),
               "dwconv_bwd")
    return out


def guided_filter_bwd(guide, y, ab, dlf, eps=(0.001, 0.0001), add=None):
    B, H, W, _ = y.shape
    dev = y.device
    if isinstance(ab, GfTape):
        t_my, t_mgy, dy = torch.empty_like(y), torch.empty_like(y), torch.empty_like(y)
        t_g = torch.empty((B, H, W, 4), device=dev, dtype=torch.float32)
        _lib.check(lib().paif_guided_filter_bwd_input_mc(_p(guide), _p(y), _p(ab.mc), _p(ab.stats), _p(dlf), _p(add), _p(t_my), _p(t_mgy),
                                                         _p(t_g), _p(dy), B, H, W, _stream()), "guided_filter_bwd_mc")
        return dy
    # per-pixel guide statistics: the fused forward's workspace (planes mean_g, 1/(var+eps_e), 1/n + the flag line); the round-1
    # kernels (PAIF_GF_BWD=v1, sizes beyond the streaming form's 32-bit offsets) use its first 2 floats per pixel
    gstat = torch.empty(lib().paif_guided_filter_fused_workspace_floats(B, H, W), device=dev, dtype=torch.float32)
    t_my, t_mgy = torch.empty_like(y), torch.empty_like(y)
    t_g = torch.empty((B, H, W, 4), device=dev, dtype=torch.float32)
    dy = torch.empty_like(y)
    _lib.check(lib().paif_guided_filter_bwd_input(_p(guide), _p(y), _p(ab), _p(dlf), eps[0], eps[1], _p(add), _p(gstat), _p(t_my),
                                                  _p(t_mgy), _p(t_g), _p(dy), B, H, W, _stream()), "guided_filter_bwd")
    return dy


def stem_bwd(dfeat, feat, w, prelu):
    B, H, W, _ = feat.shape
    dimg = torch.empty((B, 1, H, W), device=feat.device, dtype=torch.float32)
    _lib.check(lib().paif_stem_bwd_input(_p(dfeat), _p(feat), _p(w.detach().contiguous()), _p(prelu), _p(dimg), B, H, W, _stream()), "stem_bwd")
    return dimg


def tail_bwd(dfused, fused, z, w, prelu):
    B, _, H, W = fused.shape
    dt16 = torch.empty((B, H, W, 16), device=fused.device, dtype=torch.float32)
    _lib.check(lib().paif_tail_bwd_input(_p(dfused.contiguous()), _p(fused), _p(z), _p(w.detach().contiguous()), _p(prelu), _p(dt16), B, H, W,
                                         _stream()), "tail_bwd")
    return dt16


def stem_out_pack(w1, w2):
    """Weight operand of stem_out_fused: w1 [16,32,3,3], w2 [1,16,3,3] -> the composed 5x5 32->1 kernel as three-piece bf16 MFMA operands."""
    assert tuple(w1.shape) == (16, 32, 3, 3) and tuple(w2.shape) == (1, 16, 3, 3)
    L = lib()
    wpk = torch.empty(L.paif_stem_out_pack_floats(), device=w1.device, dtype=torch.float32)
    _lib.check(L.paif_stem_out_pack(_p(w1.detach().contiguous()), _p(w2.detach().contiguous()), _p(wpk), _stream()), "stem_out_pack")
    return wpk


def stem_out_fused(x, wpk, prelu):
    """bf16 NHWC-32 map -> fused [B,1,H,W] fp32: conv3x3 32->16, conv3x3 16->1, PReLU, tanh (core/model_fusion_auto.py:616-620, :640) in one
    launch pair; the 16-channel map never goes to HBM."""
    B, H, W, C = x.shape
    assert C == 32 and x.dtype in (torch.bfloat16, torch.float32)
    fused = torch.empty((B, 1, H, W), device=x.device, dtype=torch.float32)
    if _ACT_BF16[0] is torch.float16:     # fp16 storage: the range guard rides on this kernel (f16_guard_flag)
        flag = f16_guard_flag(x.device)
        _lib.check(lib().paif_stem_out_fwd_guard(_pa(x), int(x.dtype == torch.float32), _p(wpk), _p(prelu), _p(fused),
                                                 ctypes.c_void_p(flag.data_ptr()), B, H, W, _stream()), "stem_out_fused")
        return fused
    fn = lib().paif_stem_out_fwd_bf16 if x.dtype == torch.bfloat16 else lib().paif_stem_out_fwd_f32
    _lib.check(fn(_pa(x), _p(wpk), _p(prelu), _p(fused), B, H, W, _stream()), "stem_out_fused")
    return fused


def tail(x16, w, prelu, save=False):
    B, H, W, C = x16.shape
    assert C == 16
    fused = torch.empty((B, 1, H, W), device=x16.device, dtype=torch.float32)
    if x16.dtype in H16:
        assert not save
        fn = lib().paif_tail_fwd_f16 if x16.dtype == torch.float16 else lib().paif_tail_fwd_bf16
        _lib.check(fn(_pa(x16), _p(w.detach().contiguous()), _p(prelu), _p(fused), B, H, W, _stream()), "tail")
        return fused
    z = torch.empty((B, 1, H, W), device=x16.device, dtype=torch.float32) if save else None
    _lib.check(lib().paif_tail_fwd(_p(x16), _p(w.detach().contiguous()), _p(prelu), _p(fused), _p(z), B, H, W, _stream()), "tail")
    return (fused, z) if save else fused


def add(a, b):
    assert a.shape == b.shape
    if a.dtype in H16 or b.dtype in H16:
        dt = a.dtype if a.dtype in H16 else b.dtype
        a, b = cast_storage(a, dt), cast_storage(b, dt)
        out = torch.empty_like(a)
        fn = lib().paif_add_fwd_f16 if dt == torch.float16 else lib().paif_add_fwd_bf16
        _lib.check(fn(_pa(a), _pa(b), _pa(out), a.numel(), _stream()), "add")
        return out
    out = torch.empty_like(a)
    _lib.check(lib().paif_add_fwd(_p(a), _p(b), _p(out), a.numel(), _stream()), "add")
    return out


# ---------------------------------------------------------------------------------------------
# segmentation network (token tensors [B,N,C] = NHWC)
# ---------------------------------------------------------------------------------------------
_GEMM2_PACKS = {}   # id(weight tensor) -> (weakref, validity key, {precision: packed image})


def _gemm2_pack(w, prec):
    """The pre-split image of a Linear weight for csrc/gemm_split2.hip, built once per (tensor object, data_ptr, version, weights
    generation) and precision.  Keyed on the tensor OBJECT (weak reference): a temporary's address can be reused by another tensor
    with the same version counter, an object cannot while it is alive.  Callers on a hot path pass the same object every call
    (module parameters, the cached transposes of the backward)."""
    key = (w.data_ptr(), w._version, tuple(w.shape), str(w.device), CONFIG.get("weights_generation", 0))
    ent = _GEMM2_PACKS.get(id(w))
    if ent is None or ent[0]() is not w or ent[1] != key:
        ent = (weakref.ref(w, lambda _, i=id(w): _GEMM2_PACKS.pop(i, None)), key, {})
        _GEMM2_PACKS[id(w)] = ent
    pk = ent[2].get(prec)
    if pk is None:
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("the pre-split image of a %s GEMM weight (%s) is missing while a hipGraph is being captured: run one eager "
                               "step in this arithmetic first" % (tuple(w.shape), prec))
        N, K = w.shape
        L = lib()
        pk = torch.empty(L.paif_gemm2_packed_bytes(N, K, _PREC_CODE[prec]), device=w.device, dtype=torch.uint8)
        _lib.check(L.paif_gemm2_pack_weight(_p(w.detach()), ctypes.c_void_p(pk.data_ptr()), N, K, _PREC_CODE[prec], _stream()), "gemm2_pack")
        ent[2][prec] = pk
    return pk


def gemm(a, w, scale=None, shift=None, act=ACT_NONE, res=None, out=None, out_cols=None, col_offset=0,
         a_cols=None, a_mask=None, a_scale=None):
    """a [..., K] x w [N, K]^T -> [..., N].  scale/shift per output column (bias = shift).
    `out` (+col_offset) writes into a channel slice of a wider row-major buffer;
    `a_cols=(c0, K)` reads a column slice of a wider dense `a` (row stride a.shape[-1]);
    `a_mask`/`a_scale`: dgrad prologue A' = A * (mask > 0) * a_scale[k]."""
    N = w.shape[0]
    lda = a.shape[-1]
    if a_cols is None:
        K, aptr = lda, _p(a)
    else:
        _p(a)
        c0, K = a_cols
        assert c0 % 4 == 0 and c0 + K <= lda
        aptr = ctypes.c_void_p(a.data_ptr() + 4 * c0)
    assert w.shape[1] == K, (tuple(w.shape), K)
    M = a.numel() // lda
    if out is None:
        out = torch.empty(a.shape[:-1] + (N,), device=a.device, dtype=torch.float32)
        ldc, cptr = N, _p(out)
    else:
        ldc = out.shape[-1]
        assert out.is_contiguous() and col_offset + N <= ldc
        cptr = ctypes.c_void_p(out.data_ptr() + 4 * col_offset)
    if res is not None:
        assert res.shape[-1] == N and res.numel() == M * N
    if a_mask is not None:
        assert a_cols is None and a_mask.shape == a.shape
    L = lib()
    prec = CONFIG["gemm_precision"]
    splits = 1
    if a_mask is None and a_scale is None:
        splits = L.paif_gemm_splitk_plan(M, N, K)   # small grid + long k loop (small batch): spread k over the idle CUs
    if prec == "auto":   # with or without split-K (its partial products take the same arithmetic, the reduction is fp32)
        prec = "bf16x3" if (K >= 256 and M >= CONFIG["gemm_split_min_m"]) else "f32"
    elif prec == "auto6":  # the attack loops: three-piece splits (fp32-level parity) where the exact GEMM is matrix-pipe bound
        prec = "bf16x6" if (K >= 256 and M >= CONFIG["gemm_split_min_m"]) else "f32"
    elif prec == "auto6h":  # the attack loops since round 5: fp16 pairs (22 bits per operand, three MFMAs) -- for every k extent: at a
        # fifth of the exact MFMA's matrix-pipe time the short-k GEMMs are faster on them too (CONFIG["f16x3_min_k"])
        prec = "f16x3" if (K >= CONFIG["f16x3_min_k"] and M >= CONFIG["gemm_split_min_m"]) else "f32"
    tag = "gemm_mfma_%s" % prec
    e0 = TIMER.start(tag) if TIMER is not None else None
    nt = 0
    if CONFIG["gemm2"] and splits == 1 and a_mask is None and a_scale is None and prec in ("bf16x3", "bf16x6") and ldc % 4 == 0:
        nt = L.paif_gemm2_plan(M, N, K, _PREC_CODE[prec])
        if CONFIG["gemm2"] is not True and nt:      # A/B: a forced tile width (tools/gemm_shapes_b16.py)
            nt = int(CONFIG["gemm2"]) if N % (64 * int(CONFIG["gemm2"])) == 0 else nt
    if nt:
        _lib.check(L.paif_gemm2_fwd(aptr, lda, ctypes.c_void_p(_gemm2_pack(w, prec).data_ptr()), _p(scale), _p(shift), act, _p(res), N, cptr, ldc, M, N, K,
                                    _PREC_CODE[prec], nt, _stream()), "gemm2")
    elif splits > 1:
        ws = torch.empty(splits * M * N, device=a.device, dtype=torch.float32)
        _lib.check(L.paif_gemm_splitk_fwd_p(aptr, lda, _p(w), _p(scale), _p(shift), act, _p(res), N, cptr, ldc, M, N, K, splits,
                                            _p(ws), _PREC_CODE[prec], _stream()), "gemm_splitk")
    else:
        _lib.check(L.paif_gemm_masked_fwd(aptr, lda, _p(a_mask), _p(a_scale), _p(w), _p(scale), _p(shift), act, _p(res), N, cptr,
                                          ldc, M, N, K, _PREC_CODE[prec], _stream()), "gemm")
    if e0 is not None:
        TIMER.stop(tag, e0, 2 * M * N * K, 4 * (M * K + N * K + M * N * (2 if res is not None else 1)))
    return out


def transpose_pad(w2d, npad=None):
    """w [N,K] -> [K,Npad] (zero padded to a multiple of 32): the dgrad GEMM's weight operand."""
    N, K = w2d.shape
    npad = npad or (N + 31) // 32 * 32
    wt = torch.empty((K, npad), device=w2d.device, dtype=torch.float32)
    _lib.check(lib().paif_transpose_pad_fwd(_p(w2d.detach().contiguous()), _p(wt), N, K, npad, _stream()), "transpose_pad")
    return wt


def layernorm_bwd(x, weight, dy, eps, add=None):
    C = x.shape[-1]
    dx = torch.empty_like(x)
    _lib.check(lib().paif_layernorm_bwd_input(_p(x), _p(weight), _p(dy), _p(add), _p(dx), x.numel() // C, C, eps, _stream()),
               "layernorm_bwd")
    return dx


def dwconv3_bias_gelu_bwd(x, w, bias, dy, want_dpre=False):
    """-> dx (and, with want_dpre, the gradient at the depthwise conv's OUTPUT, dy * gelu'(conv(x)+b): the operand of its
    weight / bias gradient)."""
    B, H, W, C = x.shape
    tmp = torch.empty_like(x)
    dx = torch.empty_like(x)
    _lib.check(lib().paif_dwconv3_bias_gelu_bwd_input(_p(x), _p(w.detach().contiguous()), _p(bias), _p(dy), _p(tmp), _p(dx), B, H, W, C,
                                                      _stream()), "dwconv3_bias_gelu_bwd")
    return (dx, tmp) if want_dpre else dx


def col2im(dcol, B, H, W, Cin, k, stride, pad):
    kpad = dcol.shape[-1]
    dx = torch.empty((B, H, W, Cin), device=dcol.device, dtype=torch.float32)
    _lib.check(lib().paif_col2im_fwd(_p(dcol), _p(dx), B, H, W, Cin, k, stride, pad, kpad, _stream()), "col2im")
    return dx


def gemm_col2im(dy, wt, B, H, W, C, sr):
    """Input gradient of a non-overlapping sr x sr / stride-sr conv (Attention.sr): dy [B*(H/sr)*(W/sr), K] . wt [sr*sr*C, K]^T scattered
    to dx [B,H,W,C] by the GEMM's epilogue (paif_gemm_col2im_fwd) -- bit-identical to gemm + col2im, which it falls back to on maps
    whose size is not a multiple of sr (pixels without a patch must be zeroed) or with CONFIG["gemm_gather"] off."""
    K = dy.shape[-1]
    N = wt.shape[0]
    assert N == sr * sr * C and wt.shape[1] == K
    M = dy.numel() // K
    if not CONFIG["gemm_gather"] or H % sr or W % sr or C % 4:
        return col2im(gemm(dy, wt), B, H, W, C, sr, sr, 0)
    assert M == B * (H // sr) * (W // sr)
    prec = CONFIG["gemm_precision"]
    big = M >= CONFIG["gemm_split_min_m"]
    if prec == "auto":
        prec = "bf16x3" if (K >= 256 and big) else "f32"
    elif prec == "auto6":
        prec = "bf16x6" if (K >= 256 and big) else "f32"
    elif prec == "auto6h":
        prec = "f16x3" if (K >= CONFIG["f16x3_min_k"] and big) else "f32"
    dx = torch.empty((B, H, W, C), device=dy.device, dtype=torch.float32)
    tag = "gemm_mfma_%s" % prec
    e0 = TIMER.start(tag) if TIMER is not None else None
    _lib.check(lib().paif_gemm_col2im_fwd(_p(dy), K, _p(wt), _p(dx), B, H, W, C, sr, K, _PREC_CODE[prec], _stream()), "gemm_col2im")
    if e0 is not None:
        TIMER.stop(tag, e0, 2 * M * N * K, 4 * (M * K + N * K + M * N))
    return dx


def resize_bilinear_adjoint(dout, coff, C, IH, IW):
    """dout [B,OH,OW,ldo] -> dx [B,IH,IW,C] (adjoint of resize_bilinear_into on channels [coff,coff+C))."""
    B, OH, OW, ldo = dout.shape
    dx = torch.empty((B, IH, IW, C), device=dout.device, dtype=torch.float32)
    _lib.check(lib().paif_resize_bilinear_adjoint_fwd(_p(dout), _p(dx), B, IH, IW, C, OH, OW, ldo, coff, _stream()),
               "resize_bilinear_adjoint")
    return dx


def _attn_precision():
    """Arithmetic of the attention products, following the GEMMs: 0 = exact fp32 MFMA under set_gemm_precision("f32") (all gradient-
    parity tests), 6 = fp16 pairs (three fp16 MFMAs, ~2^-21.5) where the attack loops run their GEMMs on them ("auto6h"), 3 = three-piece
    bf16 splits (fp32-level, six MFMAs per product) under "bf16x6" / "auto6" (CONFIG["attn_x6"] = False keeps the exact kernels there:
    round 4's form), 1 = split-bf16 (three MFMAs) otherwise."""
    g = CONFIG["gemm_precision"]
    if g == "f32":
        return 0
    if g in ("f16x3", "auto6h") and CONFIG["attn_f16x3"]:
        return 6
    if g in ("bf16x6", "auto6", "f16x3", "auto6h"):
        return 3 if CONFIG["attn_x6"] else 0
    return 1


def sr_attention_bwd(q, kv, o, dout, lse, heads):
    B, N, C = q.shape
    Nk = kv.shape[1]
    L = lib()
    nchunk = L.paif_sr_attention_bwd_chunks(B, N, heads)
    delta = torch.empty((B, heads, N), device=q.device, dtype=torch.float32)
    dq = torch.empty_like(q)
    dkv = torch.empty_like(kv)
    partial = torch.empty((nchunk, B, Nk, 2 * C), device=q.device, dtype=torch.float32)
    split = _attn_precision()     # arithmetic follows the GEMMs (sr_attention)
    _lib.check(L.paif_sr_attention_bwd_input_p(_p(q), _p(kv), _p(o), _p(dout.contiguous()), _p(lse), _p(delta), _p(dq), _p(dkv), _p(partial),
                                               B, N, Nk, C, heads, split, _stream()), "sr_attention_bwd")
    return dq, dkv


def nchw_to_nhwc_pad(x, cp):
    x = x.contiguous()
    B, C, H, W = x.shape
    y = torch.empty((B, H, W, cp), device=x.device, dtype=torch.float32)
    _lib.check(lib().paif_nchw_to_nhwc_pad_fwd(_p(x), _p(y), B, H * W, C, cp, _stream()), "nchw_to_nhwc_pad")
    return y


def upsample_ce_fwd(logits, label, ignore_index=255):
    """logits NHWC [B,IH,IW,C], label int64 [B,OH,OW] -> tensor [2] = (mean NLL over valid px, #valid)."""
    B, IH, IW, C = logits.shape
    _, OH, OW = label.shape
    assert label.dtype == torch.int64 and label.is_cuda and label.is_contiguous()
    L = lib()
    nblk = L.paif_upsample_ce_blocks(B, OH, OW)
    partial = torch.empty(2 * nblk, device=logits.device, dtype=torch.float32)
    out = torch.empty(2, device=logits.device, dtype=torch.float32)
    _lib.check(L.paif_upsample_ce_fwd(_p(logits), ctypes.c_void_p(label.data_ptr()), _p(partial), _p(out), B, IH, IW, C, OH, OW,
                                      ignore_index, _stream()), "upsample_ce_fwd")
    return out


def upsample_ce_bwd(logits, label, gscale, cp=32, ignore_index=255):
    """-> dlogits NHWC [B,IH,IW,cp] (channels >= C zero); gscale: 1-element device tensor = dloss / count."""
    B, IH, IW, C = logits.shape
    _, OH, OW = label.shape
    dfull = torch.empty((B, OH, OW, cp), device=logits.device, dtype=torch.float32)
    _lib.check(lib().paif_upsample_ce_bwd(_p(logits), ctypes.c_void_p(label.data_ptr()), _p(gscale), _p(dfull), B, IH, IW, C, OH, OW,
                                          ignore_index, cp, _stream()), "upsample_ce_bwd")
    return resize_bilinear_adjoint(dfull, 0, cp, IH, IW)


def grad_of(p):
    """The tensor parameter gradients ACCUMULATE into: p.grad (a view into the flat gradient arena when an optimizer of
    paif_amd.utils.optimizer owns the parameter; allocated as zeros otherwise).  None when p does not require grad."""
    if p is None or not p.requires_grad:
        return None
    if p.grad is None:
        view = getattr(p, "_paif_grad_view", None)     # the parameter's slot in the optimizer's gradient arena (zeroed by zero_grad)
        p.grad = view if view is not None else torch.zeros_like(p, memory_format=torch.contiguous_format)
    if not p.grad.is_contiguous():
        raise RuntimeError("parameter gradients must be dense")
    return p.grad


def conv2d_wgrad(srcs, dout, kh, dil=1, z=None, scale=None, act=ACT_NONE, prelu=None, alpha=1.0, out=None, cout=32):
    """Weight gradient of the dense conv over the virtual concat of `srcs` (NHWC [B,H,W,32] each):
    dW [cout, 32*len(srcs), kh, kh]; ACCUMULATED into `out` when given, else returned fresh.
    dout NHWC [B,H,W,32] (zero padded when cout < 32); z = saved pre-activation when act != none."""
    B, H, W, C = srcs[0].shape
    assert C == 32 and tuple(dout.shape) == (B, H, W, 32) and 1 <= len(srcs) <= 3
    L = lib()
    ptrs = (ctypes.c_void_p * len(srcs))(*[s.data_ptr() for s in srcs])
    for s_ in srcs:
        _p(s_)
    ws = torch.empty(L.paif_conv2d_wgrad_workspace_floats(len(srcs), kh, B, H), device=dout.device, dtype=torch.float32)
    acc = out is not None
    dw = out if acc else torch.empty((cout, 32 * len(srcs), kh, kh), device=dout.device, dtype=torch.float32)
    assert dw.numel() == cout * 32 * len(srcs) * kh * kh
    _lib.check(L.paif_conv2d_wgrad(ptrs, len(srcs), _p(dout), _p(z), _p(scale), _p(prelu), act, alpha, kh, dil, _p(ws), _p(dw), cout,
                                   int(acc), B, H, W, _stream()), "conv2d_wgrad")
    return dw


def gemm_wgrad(dy, x, want_bias=True, out_w=None, out_b=None, n=None, k=None, dy_col0=0):
    """Linear-layer gradients: dy [..., ldy], x [..., ldx] (same leading shape) -> (dW [N, K], db [N] or None).
    n / k: use only n columns of dy (starting at dy_col0) / the first k columns of x.  out_w / out_b: ACCUMULATE into these."""
    lddy, ldx = dy.shape[-1], x.shape[-1]
    N, K = n or (lddy - dy_col0), k or ldx
    assert dy_col0 % 4 == 0 and dy_col0 + N <= lddy
    M = dy.numel() // lddy
    assert x.numel() // ldx == M
    L = lib()
    splits = L.paif_gemm_wgrad_splits(M, N, K)
    ws = torch.empty(splits * (N * K + N), device=dy.device, dtype=torch.float32)
    acc = out_w is not None
    dw = out_w if acc else torch.empty((N, K), device=dy.device, dtype=torch.float32)
    assert dw.numel() == N * K
    if acc:
        db = out_b
        assert db is None or db.numel() == N
    else:
        db = torch.empty(N, device=dy.device, dtype=torch.float32) if want_bias else None
    _p(dy)
    dyp = ctypes.c_void_p(dy.data_ptr() + 4 * dy_col0)
    gs = CONFIG["_wgrad_scale"] if CONFIG["wgrad_f16x3"] else None
    if gs:      # the training step's reverse pass (wgrad_scale context): fp16 pairs, dY scaled into fp16's exponent range
        _lib.check(L.paif_gemm_wgrad_p(dyp, lddy, _p(x), ldx, _p(dw), _p(db), M, N, K, splits, _p(ws), int(acc), _PREC_CODE["f16x3"], gs,
                                       _stream()), "gemm_wgrad")
    else:
        _lib.check(L.paif_gemm_wgrad(dyp, lddy, _p(x), ldx, _p(dw), _p(db), M, N, K, splits, _p(ws), int(acc), _stream()), "gemm_wgrad")
    return dw, db


class wgrad_scale:
    """Around the reverse pass of a training step over `pixels` image pixels: the Linear-layer weight-gradient kernels run on fp16 pairs
    (CONFIG["wgrad_f16x3"]) with dY multiplied by 2^(floor(log2 pixels) - 6) inside the kernel (and the result divided by it): losses
    averaged over the pixels put |dY| around 1 / pixels, far below fp16's exponent range.  Outside this context (stand-alone calls, the
    gradient-parity tests of the kernels) the exact fp32-MFMA kernels run."""

    def __init__(self, pixels):
        self.k = max(0, int(pixels).bit_length() - 1 - 6)

    def __enter__(self):
        self.old = CONFIG["_wgrad_scale"]
        CONFIG["_wgrad_scale"] = float(2 ** self.k)

    def __exit__(self, *a):
        CONFIG["_wgrad_scale"] = self.old


def layernorm_wgrad(x, dy, eps, out_g=None, out_b=None):
    """LayerNorm affine gradients: x, dy [..., C] -> (dgamma [C], dbeta [C]); accumulated into out_g / out_b when given."""
    C = x.shape[-1]
    M = x.numel() // C
    assert dy.shape == x.shape
    L = lib()
    ws = torch.empty(L.paif_layernorm_wgrad_blocks(M) * 2 * C, device=x.device, dtype=torch.float32)
    acc = out_g is not None
    assert acc == (out_b is not None)
    dg = out_g if acc else torch.empty(C, device=x.device, dtype=torch.float32)
    db = out_b if acc else torch.empty(C, device=x.device, dtype=torch.float32)
    _lib.check(L.paif_layernorm_wgrad(_p(x), _p(dy), _p(dg), _p(db), _p(ws), M, C, eps, int(acc), _stream()), "layernorm_wgrad")
    return dg, db


# ---------------------------------------------------------------------------------------------
# training step (csrc/train_kernels.hip): every *_wgrad ACCUMULATES into its `out` tensors
# ---------------------------------------------------------------------------------------------
def _rr_ws(M, C, nacc, device, mult=1):
    n = lib().paif_row_reduce_workspace_floats(M, C, nacc)
    if n == 0:
        raise NotImplementedError("row reduction over %d channels is not built (C must be a multiple of 4)" % C)
    return torch.empty(mult * n, device=device, dtype=torch.float32)


def nhwc_slice_to_nchw(x, C):
    """x NHWC [B,H,W,ld] -> NCHW [B,C,H,W] of channels [0,C)."""
    B, H, W, ld = x.shape
    y = torch.empty((B, C, H, W), device=x.device, dtype=torch.float32)
    _lib.check(lib().paif_nhwc_slice_to_nchw_fwd(_p(x), _p(y), B, H * W, C, ld, _stream()), "nhwc_slice_to_nchw")
    return y


def decomp_cat(x, lf):
    """x [B,H,W,32], lf [2,B,H,W,32] -> (cat(LF0, LF1), cat(x-LF0, x-LF1)) as NHWC [B,H,W,64] each."""
    B, H, W, _ = x.shape
    lfc = torch.empty((B, H, W, 64), device=x.device, dtype=torch.float32)
    hfc = torch.empty_like(lfc)
    _lib.check(lib().paif_decomp_cat_fwd(_p(x), _p(lf), _p(lfc), _p(hfc), B * H * W, _stream()), "decomp_cat")
    return lfc, hfc


def pad_channels(x, cd):
    cs = x.shape[-1]
    y = torch.empty(x.shape[:-1] + (cd,), device=x.device, dtype=torch.float32)
    _lib.check(lib().paif_pad_channels_fwd(_p(x), _p(y), x.numel() // cs, cs, cd, _stream()), "pad_channels")
    return y


def bn_stats(x, gamma, beta, eps, momentum, running_mean, running_var):
    """Train-mode BatchNorm statistics of x [..., C] -> (mean, invstd, scale, shift); running stats updated in place."""
    C = x.shape[-1]
    M = x.numel() // C
    st = torch.empty((4, C), device=x.device, dtype=torch.float32)
    ws = _rr_ws(M, C, 2, x.device, mult=2)
    _lib.check(lib().paif_bn_stats_fwd(_p(x), M, C, _p(gamma), _p(beta), eps, momentum, _p(running_mean), _p(running_var), _p(st[0]),
                                       _p(st[1]), _p(st[2]), _p(st[3]), _p(ws), _stream()), "bn_stats")
    return st[0], st[1], st[2], st[3]


def affine_act_res(x, scale, shift, act=ACT_NONE, prelu=None, res=(), want_z=False):
    """act(x*scale[c] + shift[c]) + res[0] + res[1] (+ further residuals as plain adds); optionally also the pre-activation."""
    C = x.shape[-1]
    res = [r for r in res if r is not None]
    out = torch.empty_like(x)
    z = torch.empty_like(x) if want_z else None
    _lib.check(lib().paif_affine_act_res_fwd(_p(x), _p(scale), _p(shift), act, _p(prelu), _p(res[0]) if res else None,
                                             _p(res[1]) if len(res) > 1 else None, _p(out), _p(z), x.numel() // C, C, _stream()),
               "affine_act_res")
    for r in res[2:]:
        out = add(out, r)
    return (out, z) if want_z else out


def bn_eval_stats(gamma, beta, running_mean, running_var, eps):
    """Eval-mode BatchNorm as (mean, invstd, scale, shift) -- same tuple as bn_stats, from the running statistics."""
    C = running_mean.numel()
    st = torch.empty((4, C), device=running_mean.device, dtype=torch.float32)
    _lib.check(lib().paif_bn_eval_stats(_p(gamma), _p(beta), _p(running_mean), _p(running_var), eps, C, _p(st[0]), _p(st[1]), _p(st[2]),
                                        _p(st[3]), _stream()), "bn_eval_stats")
    return st[0], st[1], st[2], st[3]


def bn_act_bwd(g, x, stats, act=ACT_NONE, prelu=None, d_gamma=None, d_beta=None, d_slope=None, training=True):
    """Backward of act(BN(x)) (stats = (mean, invstd, scale, shift) of bn_stats / bn_eval_stats): returns dx; accumulates the
    affine / slope gradients into d_gamma, d_beta, d_slope (any may be None).  training=False: running statistics."""
    C = x.shape[-1]
    M = x.numel() // C
    mean, invstd, scale, shift = stats
    dx = torch.empty_like(x)
    sums = torch.empty(2 * C, device=x.device, dtype=torch.float32)
    ws = _rr_ws(M, C, 3, x.device)
    _lib.check(lib().paif_bn_act_bwd(_p(g), _p(x), _p(scale), _p(shift), _p(mean), _p(invstd), act, _p(prelu), _p(dx), _p(d_gamma),
                                     _p(d_beta), _p(d_slope), _p(sums), _p(ws), int(training), M, C, _stream()), "bn_act_bwd")
    return dx


def prelu_bwd(t, r, prelu, d_slope, add=None, want_dx=False, factor=1.0):
    """d_slope[0] += factor * sum t*r over r<0; with want_dx also returns t*P'(r) (+ add)."""
    assert t.shape == r.shape and t.numel() % 4 == 0
    dx = torch.empty_like(t) if want_dx else None
    ws = torch.empty(2048, device=t.device, dtype=torch.float32)
    if d_slope is None:   # slope frozen: only the input gradient is wanted
        d_slope = torch.zeros(1, device=t.device, dtype=torch.float32)
    _lib.check(lib().paif_prelu_bwd(_p(t), _p(r), _p(add), _p(prelu), factor, _p(dx), _p(d_slope), _p(ws), t.numel(), _stream()), "prelu_bwd")
    return dx


def tail_dz(dfused, fused, z, prelu, d_slope):
    dz = torch.empty_like(fused)
    ws = torch.empty(2048, device=fused.device, dtype=torch.float32)
    if d_slope is None:
        d_slope = torch.zeros(1, device=fused.device, dtype=torch.float32)
    _lib.check(lib().paif_tail_dz(_p(dfused.contiguous()), _p(fused), _p(z), _p(prelu), _p(dz), _p(d_slope), _p(ws), fused.numel(), _stream()),
               "tail_dz")
    return dz


def colsum(x, out, ncols=None):
    """out[c] += column sums of x [..., ld] (first ncols columns)."""
    ld = x.shape[-1]
    C = ncols or ld
    M = x.numel() // ld
    ws = _rr_ws(M, C, 1, x.device)
    _lib.check(lib().paif_colsum(_p(x), ld, _p(out), _p(ws), M, C, _stream()), "colsum")
    return out


def dwconv_wgrad(x, dy, k, dil, in_relu, out_w, out_b=None):
    """Depthwise-conv gradients accumulated into out_w [C,1,k,k] (and out_b [C])."""
    B, H, W, C = x.shape
    assert dy.shape == x.shape and out_w.numel() == C * k * k
    ws = _rr_ws(B * H * W, C, k * k + 1, x.device)
    _lib.check(lib().paif_dwconv_wgrad(_p(x), _p(dy), _p(out_w), _p(out_b), _p(ws), k, dil, int(in_relu), B, H, W, C, _stream()), "dwconv_wgrad")


def stem_wgrad(img, dfeat, w, prelu, out_w, out_slope):
    """stem conv (1->32, 3x3) + PReLU gradients accumulated into out_w [32,1,3,3], out_slope [1]."""
    B, _, H, W = img.shape
    if img.stride(3) != 1 or img.stride(2) != W:
        img = img.contiguous()
    bstride = img.stride(0) if B > 1 else H * W
    ws = _rr_ws(B * H * W, 32, 10, dfeat.device)
    dev = dfeat.device
    ow = out_w if out_w is not None else torch.zeros(32 * 9, device=dev)
    osl = out_slope if out_slope is not None else torch.zeros(1, device=dev)
    _lib.check(lib().paif_stem_wgrad(ctypes.c_void_p(img.data_ptr()), bstride, _p(dfeat), _p(w.detach()), _p(prelu), _p(ow), _p(osl), _p(ws),
                                     B, H, W, _stream()), "stem_wgrad")


def corr1_wgrad(s, m, k, out_w):
    """out_w [1,Cm,k,k] += sum_px s[px] * m[px+tap][c]   (s [B,H,W] or [B,1,H,W], m NHWC [B,H,W,Cm])."""
    B, H, W, Cm = m.shape
    assert s.numel() == B * H * W and out_w.numel() == Cm * k * k
    ws = _rr_ws(B * H * W, Cm, k * k, m.device)
    _lib.check(lib().paif_corr1_wgrad(_p(s), _p(m), _p(out_w), _p(ws), Cm, k, B, H, W, _stream()), "corr1_wgrad")


def eca_wgrad(pool_partial, dgate_partial, gate, k, out_w, B, H, W):
    ws = torch.empty(9 * B, device=gate.device, dtype=torch.float32)
    _lib.check(lib().paif_eca_wgrad(_p(pool_partial), _p(dgate_partial), dgate_partial.shape[1], _p(gate), k, _p(out_w), _p(ws), B, H, W,
                                    _stream()), "eca_wgrad")


def unfold_decomp1x1_wgrad(G, out_w):
    assert G.numel() == 32 * 96 and out_w.numel() == 32 * 128
    _lib.check(lib().paif_unfold_decomp1x1_wgrad(_p(G), _p(out_w), _stream()), "unfold_decomp1x1_wgrad")


def unpack_conv_gemm_wgrad(dwp, out_w):
    Cout, Cin, k, _ = out_w.shape
    _lib.check(lib().paif_unpack_conv_gemm_wgrad(_p(dwp), _p(out_w), Cout, Cin, k, dwp.shape[1], _stream()), "unpack_conv_gemm_wgrad")


class DropRNG:
    """Counter-based random stream of the stochastic layers (DropPath, Dropout2d): mask i of a call is the uniform
    u(seed, offset + i) of paif_keep_mask (= paif_amd.synthetic.hash_uniform), offset advancing by the mask size per call
    -- reproducible from (seed, rank, step) alone."""

    def __init__(self, seed=0):
        self.reseed(seed)

    def reseed(self, seed, rank=0, step=0):
        self.seed = (int(seed) * 1000003 + int(rank) * 7919 + int(step) * 104729) & 0xFFFFFFFF
        self.offset = 0

    def keep_mask(self, n, p, device):
        out = torch.empty(n, device=device, dtype=torch.float32)
        _lib.check(lib().paif_keep_mask(_p(out), n, self.seed, self.offset, float(p), _stream()), "keep_mask")
        self.offset += n
        return out


DROP_RNG = DropRNG(0)


def rowscale_add(x, s, res=None, per_channel=False):
    """x [B, ..., C] * s[b] (or s[b, c]) + res."""
    B, C = x.shape[0], x.shape[-1]
    out = torch.empty_like(x)
    _lib.check(lib().paif_rowscale_add_fwd(_p(x), _p(s), _p(res), _p(out), B, x.numel() // (B * C), C, int(per_channel), _stream()),
               "rowscale_add")
    return out


class UpsampleCE(torch.autograd.Function):
    """CrossEntropyLoss(ignore_index)(F.interpolate(seg_map, label.shape[1:], bilinear, align_corners=False), label) as the
    fused HIP kernels paif_upsample_ce_fwd / _bwd (attack/attack.py:103-114,446-448; core/model_fusion_auto.py:1096-1098)."""

    @staticmethod
    def forward(ctx, seg_map, label, ignore_index):
        logits = to_nhwc(seg_map.detach())
        lc = upsample_ce_fwd(logits, label, ignore_index)
        ctx.save_for_backward(logits, label, lc)
        ctx.ignore_index = ignore_index
        return lc[0].clone()

    @staticmethod
    def backward(ctx, g):
        logits, label, lc = ctx.saved_tensors
        gscale = (g.reshape(1).to(torch.float32) / lc[1:2]).contiguous()      # dloss / #valid (1-element tensor)
        d32 = upsample_ce_bwd(logits, label, gscale, ignore_index=ctx.ignore_index)
        return nhwc_slice_to_nchw(d32, logits.shape[-1]), None, None


ATTACK_WAYS = {"PGD": 0, "newPGD": 0, "segPGD": 1, "cosPGD": 2}


def attack_loss_weights(attack_way, i, attack_iters):
    """(way code, w_true, w_false) of attack/attack.py:447-499.  segPGD: lambda = (i-1)/(2*iters) (:450);
    newPGD: cos_t / cos_f with pred_t == pred_f (:486-492) is exactly 1 and its gradient identically 0 -> the PGD loss."""
    if attack_way not in ATTACK_WAYS:
        raise NameError("loss")   # the reference leaves `loss` unbound for an unknown attack_way
    lamb = (i - 1) / (attack_iters * 2)
    return (ATTACK_WAYS[attack_way], 1.0 - lamb, lamb) if attack_way == "segPGD" else (ATTACK_WAYS[attack_way], 1.0, 1.0)


def attack_loss_fwd(logits, label, way, w_true=1.0, w_false=1.0, ignore_index=255):
    """logits NHWC [B,IH,IW,C], label int64 [B,OH,OW] -> coef tensor [8]: (loss, #valid, CE, cos, ..., [7] = number of labels outside
    [0, C) that are not ignore_index: dropped like ignored pixels, never used as an index) -- paif_attack_loss_fwd."""
    B, IH, IW, C = logits.shape
    _, OH, OW = label.shape
    assert label.dtype == torch.int64 and label.is_cuda and label.is_contiguous()
    L = lib()
    nblk = L.paif_attack_loss_blocks(B, OH, OW)
    partial = torch.empty(6 * nblk, device=logits.device, dtype=torch.float32)
    coef = torch.empty(8, device=logits.device, dtype=torch.float32)
    _lib.check(L.paif_attack_loss_fwd(_p(logits), ctypes.c_void_p(label.data_ptr()), _p(partial), _p(coef), way, w_true, w_false,
                                      B, IH, IW, C, OH, OW, ignore_index, _stream()), "attack_loss_fwd")
    return coef


def attack_loss_bwd(logits, label, coef, way, w_true=1.0, w_false=1.0, upstream=1.0, cp=32, ignore_index=255):
    """-> d loss / d logits NHWC [B,IH,IW,cp] (channels >= C zero)."""
    B, IH, IW, C = logits.shape
    _, OH, OW = label.shape
    dfull = torch.empty((B, OH, OW, cp), device=logits.device, dtype=torch.float32)
    _lib.check(lib().paif_attack_loss_bwd(_p(logits), ctypes.c_void_p(label.data_ptr()), _p(coef), _p(dfull), way, w_true, w_false,
                                          float(upstream), B, IH, IW, C, OH, OW, ignore_index, cp, _stream()), "attack_loss_bwd")
    return resize_bilinear_adjoint(dfull, 0, cp, IH, IW)


class AttackLoss(torch.autograd.Function):
    """The segPGD / cosPGD losses on F.interpolate(seg_map, label.shape[1:], bilinear) as the fused HIP kernels
    paif_attack_loss_fwd / _bwd (autograd node for the fresh-gradient attacks seg_pgd / cos_pgd, attack/attack.py:307-411)."""

    @staticmethod
    def forward(ctx, seg_map, label, way, w_true, w_false):
        logits = to_nhwc(seg_map.detach())
        coef = attack_loss_fwd(logits, label, way, w_true, w_false)
        ctx.save_for_backward(logits, label, coef)
        ctx.args = (way, w_true, w_false)
        return coef[0].clone()

    @staticmethod
    def backward(ctx, g):
        logits, label, coef = ctx.saved_tensors
        way, w_true, w_false = ctx.args
        d32 = attack_loss_bwd(logits, label, coef, way, w_true, w_false, upstream=float(g))
        return nhwc_slice_to_nchw(d32, logits.shape[-1]), None, None, None, None


def attack_loss(seg_map, label, attack_way, i, attack_iters):
    """seg_map [B,C,h,w] (low resolution), label int64 [B,H,W] -> the attack variant's loss (differentiable w.r.t. seg_map)."""
    way, wt, wf = attack_loss_weights(attack_way, i, attack_iters)
    label = label.contiguous().type(torch.long)
    if torch.is_grad_enabled() and seg_map.requires_grad:
        return AttackLoss.apply(seg_map, label, way, wt, wf)
    return attack_loss_fwd(to_nhwc(seg_map.detach()), label, way, wt, wf)[0]


# ---- image-space attack losses (attack/attack.py:75-100, 132-133, 216-218): all-HIP autograd nodes ----
_SEG_MEAN = (123.675, 116.28, 103.53)
_SEG_STD = (58.395, 57.12, 57.375)
_TF_CONST = {}


def _tf_consts(device):
    k = str(device)
    if k not in _TF_CONST:
        sd = torch.tensor([v / 255.0 for v in _SEG_STD], device=device, dtype=torch.float32)
        mean = torch.tensor([v / 255.0 for v in _SEG_MEAN], device=device, dtype=torch.float32)
        _TF_CONST[k] = (sd, mean)
    return _TF_CONST[k]


def channel_affine_nchw(x, scale, shift=None):
    x = x.contiguous()
    B, C, H, W = x.shape
    out = torch.empty_like(x)
    _lib.check(lib().paif_channel_affine_nchw_fwd(_p(x), _p(scale), _p(shift), _p(out), B, C, H, W, _stream()), "channel_affine_nchw")
    return out


class TransFormat(torch.autograd.Function):
    """attack/attack.py:75-100 `trans_format(image_fusion, images_vis)`: RGB from the fused Y and the visible image's Cr / Cb, clamp to
    [0, 1], batch-global min-max -- the composite model's own fusion->seg glue without its mean / std step, so it is that glue
    (paif_recompose_clamp_fwd + paif_minmax_normalize_fwd; backward paif_glue_bwd_input) and one per-channel affine each way."""

    @staticmethod
    def forward(ctx, fused, ycc):
        fused = fused.detach().contiguous()
        seg_in, mm = seg_input_from_fused(fused, ycc, return_minmax=True)
        sd, mean = _tf_consts(fused.device)
        ctx.save_for_backward(fused, ycc, mm)
        return channel_affine_nchw(seg_in, sd, mean)          # (s * sd + mean) / 255 = (rgb - min) / (max - min)

    @staticmethod
    def backward(ctx, g):
        fused, ycc, mm = ctx.saved_tensors
        sd, _ = _tf_consts(fused.device)
        dfused, _ = glue_bwd(channel_affine_nchw(g, sd), fused, ycc, mm)
        return dfused, None


def trans_format(fused, vis):
    """fused [B,1,H,W] (may require grad), vis RGB [B,3,H,W] -> [B,3,H,W] in [0, 1]."""
    with torch.no_grad():
        ycc = rgb2ycrcb(vis.contiguous())
    if torch.is_grad_enabled() and fused.requires_grad:
        return TransFormat.apply(fused, ycc)
    seg_in = seg_input_from_fused(fused.detach().contiguous(), ycc)
    sd, mean = _tf_consts(fused.device)
    return channel_affine_nchw(seg_in, sd, mean)


class ImageLoss(torch.autograd.Function):
    """sign * nn.MSELoss()(a, target) (kind 0) / nn.L1Loss() (kind 1), mean reduction, target [B,C,H,W] or [B,1,H,W] (broadcast)."""

    @staticmethod
    def forward(ctx, a, target, kind, sign):
        a = a.detach().contiguous()
        target = target.detach().contiguous()
        B, C, H, W = a.shape
        Ct = target.shape[1]
        assert target.shape[0] == B and tuple(target.shape[2:]) == (H, W) and Ct in (1, C), (tuple(a.shape), tuple(target.shape))
        L = lib()
        partial = torch.empty(L.paif_image_loss_blocks(), device=a.device, dtype=torch.float32)
        loss = torch.empty(1, device=a.device, dtype=torch.float32)
        _lib.check(L.paif_image_loss_fwd(_p(a), _p(target), kind, B, C, Ct, H, W, _p(partial), _p(loss), _stream()), "image_loss")
        ctx.save_for_backward(a, target)
        ctx.args = (kind, sign)
        return loss[0] * sign if sign != 1.0 else loss[0].clone()

    @staticmethod
    def backward(ctx, g):
        a, target = ctx.saved_tensors
        kind, sign = ctx.args
        B, C, H, W = a.shape
        da = torch.empty_like(a)
        _lib.check(lib().paif_image_loss_bwd(_p(a), _p(target), kind, B, C, target.shape[1], H, W, float(g) * sign, _p(da), _stream()),
                   "image_loss_bwd")
        return da, None, None, None


def image_loss(a, target, kind, sign=1.0):
    """kind: "l_2" (MSE) or "l_1" (L1), as the reference's criteria; differentiable w.r.t. a."""
    return ImageLoss.apply(a, target, {"l_2": 0, "l_1": 1}[kind], float(sign))


def upsample_ce(seg_map, label, ignore_index=255):
    """seg_map [B,C,h,w] (any strides), label int64 [B,H,W] -> mean NLL over the valid pixels (differentiable w.r.t. seg_map)."""
    label = label.contiguous()
    if torch.is_grad_enabled() and seg_map.requires_grad:
        return UpsampleCE.apply(seg_map, label, ignore_index)
    return upsample_ce_fwd(to_nhwc(seg_map.detach()), label, ignore_index)[0]


# ---- segmentation criteria (core/loss.py:342-383) on csrc/seg_criteria.hip ----
SEG_NORMAL, SEG_FOCAL, SEG_OHEM = 0, 1, 2
SEG_KINDS = {"normal": SEG_NORMAL, "focal": SEG_FOCAL, "ohem": SEG_OHEM}
SEG_MAXC = 32        # the kernels' channel limit (the CE_MAXC of upsample_ce)


def _seg_criterion_args(logits, label, kind, gamma, T, n_min):
    """Shape and parameter checks of seg_criterion_fwd, on the host and before any launch -> (kind code, param, n_min)."""
    if kind not in SEG_KINDS:
        raise ValueError("seg_criterion: kind %r (one of %s)" % (kind, sorted(SEG_KINDS)))
    if logits.dim() != 4 or label.dim() != 3 or label.shape[0] != logits.shape[0] or logits.numel() == 0 or label.numel() == 0:
        raise ValueError("seg_criterion: expected logits [B,IH,IW,C] and labels [B,OH,OW], got %s and %s"
                         % (tuple(logits.shape), tuple(label.shape)))
    if logits.shape[-1] > SEG_MAXC:
        raise NotImplementedError("seg_criterion: built for C <= %d classes, got %d" % (SEG_MAXC, logits.shape[-1]))
    if logits.dtype != torch.float32 or label.dtype != torch.int64:
        raise TypeError("seg_criterion: expected float32 logits and int64 labels, got %s and %s" % (logits.dtype, label.dtype))
    code, param, k = SEG_KINDS[kind], 0.0, 0
    if code == SEG_FOCAL:
        if not gamma >= 0:
            raise ValueError("seg_criterion: focal gamma must be >= 0, got %r" % (gamma,))
        param = float(gamma)
    elif code == SEG_OHEM:
        n = label.numel()
        if int(n_min) != n_min or not 1 <= n_min <= n:
            raise ValueError("seg_criterion: OHEM n_min = %r outside [1, %d] (the number of pixels)" % (n_min, n))
        if not T >= 0:
            raise ValueError("seg_criterion: OHEM T = -log(thresh) must be >= 0, got %r" % (T,))
        param, k = float(T), int(n_min)
    if not (logits.is_cuda and label.is_cuda):      # last, so that every refusal above is the same with and without a GPU
        raise RuntimeError("paif_amd ops need CUDA(HIP) tensors; got %s (logits) and %s (labels) -- there is no CPU path"
                           % (logits.device, label.device))
    return code, param, k


def seg_criterion_fwd(logits, label, kind, gamma=0.0, T=0.0, n_min=0, ignore_index=255):
    """logits NHWC [B,IH,IW,C], label int64 [B,OH,OW] -> (coef [8], l plane, lse plane): paif_seg_criterion_fwd.  coef = (value, mode,
    threshold, weight above it, weight at it, #valid, #labels outside [0, C) that are not ignore_index, #above); no host read."""
    code, param, n_min = _seg_criterion_args(logits, label, kind, gamma, T, n_min)
    B, IH, IW, C = logits.shape
    _, OH, OW = label.shape
    assert label.is_contiguous()
    L = lib()
    ws = torch.empty(L.paif_seg_criterion_workspace_words(B, OH, OW), device=logits.device, dtype=torch.int32)
    planes = torch.empty((2, B, OH, OW), device=logits.device, dtype=torch.float32)
    coef = torch.empty(8, device=logits.device, dtype=torch.float32)
    _lib.check(L.paif_seg_criterion_fwd(_p(logits), ctypes.c_void_p(label.data_ptr()), _p(planes[0]), _p(planes[1]),
                                        ctypes.c_void_p(ws.data_ptr()), _p(coef), code, param, n_min, B, IH, IW, C, OH, OW,
                                        int(ignore_index), _stream()), "seg_criterion_fwd")
    return coef, planes[0], planes[1]


def seg_criterion_bwd(logits, label, lplane, lse, coef, upstream, kind, gamma=0.0, ignore_index=255):
    """-> (d value / d logits NHWC [B,IH,IW,cp], the full-resolution buffer [B,OH,OW,cp]); cp = C rounded up to 4, the narrowest pad the
    adjoint kernel takes; pad channels zero.  upstream: 0-d / 1-element float32 device tensor.  Identity scale: both are one tensor."""
    B, IH, IW, C = logits.shape
    _, OH, OW = label.shape
    cp = (C + 3) // 4 * 4
    dfull = torch.empty((B, OH, OW, cp), device=logits.device, dtype=torch.float32)
    _lib.check(lib().paif_seg_criterion_bwd(_p(logits), ctypes.c_void_p(label.data_ptr()), _p(lplane), _p(lse), _p(coef),
                                            _p(upstream), _p(dfull), SEG_KINDS[kind], float(gamma), B, IH, IW, C, OH, OW,
                                            int(ignore_index), cp, _stream()), "seg_criterion_bwd")
    if (IH, IW) == (OH, OW):
        return dfull, dfull          # the interpolation is the identity, and so is its adjoint
    return resize_bilinear_adjoint(dfull, 0, cp, IH, IW), dfull


class SegCriterion(torch.autograd.Function):
    """NormalLoss / SoftmaxFocalLoss / OhemCELoss on F.interpolate(seg_map, label.shape[1:], bilinear, align_corners=False) as the fused
    HIP kernels paif_seg_criterion_fwd / _bwd; differentiable w.r.t. seg_map only."""

    @staticmethod
    def forward(ctx, seg_map, label, kind, gamma, T, n_min, ignore_index):
        logits = to_nhwc(seg_map.detach())
        coef, lplane, lse = seg_criterion_fwd(logits, label, kind, gamma, T, n_min, ignore_index)
        ctx.save_for_backward(logits, label, coef, lplane, lse)
        ctx.args = (kind, gamma, ignore_index)
        return coef[0].clone()

    @staticmethod
    def backward(ctx, g):
        logits, label, coef, lplane, lse = ctx.saved_tensors
        kind, gamma, ignore_index = ctx.args
        up = g.reshape(1).to(torch.float32).contiguous()
        d, _ = seg_criterion_bwd(logits, label, lplane, lse, coef, up, kind, gamma, ignore_index)
        return nhwc_slice_to_nchw(d, logits.shape[-1]), None, None, None, None, None, None


def seg_criterion(seg_map, label, kind, gamma=0.0, T=0.0, n_min=0, ignore_index=255):
    """seg_map [B,C,h,w] (any strides), label int64 [B,H,W], kind "normal" | "focal" | "ohem" -> the criterion's value as a 0-d device
    tensor (differentiable w.r.t. seg_map).  T = -log(thresh) as a float32 value; C > 32 raises NotImplementedError."""
    label = label.contiguous()
    if torch.is_grad_enabled() and seg_map.requires_grad:
        return SegCriterion.apply(seg_map, label, kind, gamma, T, n_min, ignore_index)
    return seg_criterion_fwd(to_nhwc(seg_map.detach()), label, kind, gamma, T, n_min, ignore_index)[0][0]


_SSIM_WINDOW = {}


def _ssim_window(device):
    import math
    g = _SSIM_WINDOW.get(device)
    if g is None:
        g1 = torch.Tensor([math.exp(-(i - 11 // 2) ** 2 / float(2 * 1.5 ** 2)) for i in range(11)])
        g = _SSIM_WINDOW[device] = (g1 / g1.sum()).to(device)
    return g


def ssim_l1_bwd(x, y, k_l1, k_ss):
    """d/dx of k_l1 * sum|y - x| + k_ss * sum(1 - SSIM map): x, y [B,1,H,W]; k_* 0-d device tensors -> dx [B,1,H,W]."""
    x, y = x.contiguous(), y.contiguous()
    B, _, H, W = x.shape
    k = torch.stack([k_l1.reshape(()), k_ss.reshape(())]).to(torch.float32).contiguous()
    abc = torch.empty((3, B, H, W), device=x.device, dtype=torch.float32)
    dx = torch.empty_like(x)
    _lib.check(lib().paif_ssim_l1_bwd_input(_p(x), _p(y), _p(_ssim_window(x.device)), _p(k), _p(abc), _p(dx), B, H, W, _stream()),
               "ssim_l1_bwd")
    return dx


def ssim_l1(x, y):
    """x, y: [B,1,H,W] -> (mean SSIM_11x11(x, y), mean |y - x|) as 0-d device tensors (forward values only).
    pytorch_ssim/__init__.py:8-43: Gaussian window sigma 1.5 (built in fp32 like the reference), zero padding, mean."""
    assert x.shape == y.shape and x.shape[1] == 1
    x, y = x.contiguous(), y.contiguous()
    B, _, H, W = x.shape
    g = _ssim_window(x.device)
    L = lib()
    partial = torch.empty((L.paif_ssim_l1_blocks(B, H, W), 2), device=x.device, dtype=torch.float32)
    s = torch.empty(2, device=x.device, dtype=torch.float32)
    _lib.check(L.paif_ssim_l1_fwd(_p(x), _p(y), _p(g), _p(partial), _p(s), B, H, W, _stream()), "ssim_l1")
    return s[0], s[1]


# ---- Sobel fusion criteria (csrc/sobel_loss.hip; core/loss.py:423-474, 516-571, 595-603, 634-650) ----
SOBEL_NONE, SOBEL_MAX, SOBEL_MASK, SOBEL_LIN = 0, 1, 2, 3


def _check_plane0(t, shape, name):
    """dtype and shape of a plane argument (before any device check, so that a wrong argument is named as such on any device)."""
    if t is None:
        return
    if t.dtype != torch.float32:
        raise TypeError("%s: expected float32, got %s" % (name, t.dtype))
    B, _, H, W = shape
    if t.dim() != 4 or t.shape[1] < 1 or (t.shape[0], t.shape[2], t.shape[3]) != (B, H, W):
        raise ValueError("%s: expected [%d, C >= 1, %d, %d] like the generated image, got %s" % (name, B, H, W, tuple(t.shape)))


def _plane0(t, shape, name):
    """Channel 0 of a [B,C,H,W] fp32 device tensor as (keep-alive tensor, pointer, batch stride in floats), read in place when the
    channel's rows are dense; `shape` = the generated image's [B,1,H,W]."""
    if t is None:
        return None, None, 0
    _check_plane0(t, shape, name)
    if not t.is_cuda:
        raise RuntimeError("paif_amd ops need CUDA(HIP) tensors; got a %s tensor for %s -- there is no CPU path" % (t.device, name))
    B, _, H, W = shape
    t = t.detach()
    if not ((W == 1 or t.stride(3) == 1) and (H == 1 or t.stride(2) == W) and (B == 1 or t.stride(0) >= H * W)):
        t = t[:, :1].contiguous()
    return t, ctypes.c_void_p(t.data_ptr()), (t.stride(0) if B > 1 else H * W)


def _sobel_desc(gen, ir, y, mask, intensity, gradient):
    """intensity: up to two (kind, weight, alpha, beta); gradient: one such tuple or None -> (paif_sobel_desc, tensors kept alive)."""
    if gen.dtype != torch.float32:
        raise TypeError("generated image: expected float32, got %s" % gen.dtype)
    if gen.dim() != 4 or gen.shape[1] != 1:
        raise ValueError("generated image: expected [B,1,H,W], got %s" % (tuple(gen.shape),))
    for t, name in ((ir, "image_ir"), (y, "image_vis"), (mask, "mask")):
        _check_plane0(t, gen.shape, name)
    if not gen.is_cuda:
        raise RuntimeError("paif_amd ops need CUDA(HIP) tensors; got a %s tensor for the generated image -- there is no CPU path" % gen.device)
    if len(intensity) > 2:
        raise ValueError("sobel_loss: at most two intensity terms, got %d" % len(intensity))
    gen = gen.detach().contiguous()
    d = _lib.SobelDesc()
    keep = [gen]
    d.f, d.f_bs = ctypes.c_void_p(gen.data_ptr()), gen.shape[2] * gen.shape[3]
    for fld, t, name in (("a", ir, "image_ir"), ("b", y, "image_vis"), ("m", mask, "mask")):
        tt, ptr, bs = _plane0(t, gen.shape, name)
        keep.append(tt)
        setattr(d, fld, ptr)
        setattr(d, fld + "_bs", bs)
    for i, (kind, w, al, be) in enumerate(intensity):
        d.t_kind[i], d.t_weight[i], d.t_alpha[i], d.t_beta[i] = kind, w, al, be
    if gradient is not None:
        d.q_kind, d.q_weight, d.q_alpha, d.q_beta = gradient
    return d, keep


def sobel_loss(gen, ir, y, mask, intensity, gradient):
    """sum_i w_i mean|T_i - gen| + w_q mean|Q - S(gen)|  (include/paif_hip.h: paif_sobel_desc) on channel 0 of ir / y / mask (None where
    no term reads it) -> device tensor [4]: the means of the two intensity terms and of the gradient term, and the weighted sum.
    Forward value only; no host synchronisation."""
    d, keep = _sobel_desc(gen, ir, y, mask, intensity, gradient)
    B, _, H, W = gen.shape
    L = lib()
    nblk = L.paif_sobel_loss_blocks(B, H, W)
    if nblk <= 0:
        raise ValueError("sobel_loss: a batch of %d x %d x %d planes is empty or has more tiles than a 32-bit block index" % (B, H, W))
    partial = torch.empty((nblk, 3), device=gen.device, dtype=torch.float32)
    out = torch.empty(4, device=gen.device, dtype=torch.float32)
    _lib.check(L.paif_sobel_loss_fwd(ctypes.byref(d), _p(partial), _p(out), B, H, W, _stream()), "sobel_loss")
    return out


def sobel_loss_bwd(gen, ir, y, mask, intensity, gradient, g):
    """g (0-d or 1-element fp32 device tensor: the upstream gradient) -> g * d sobel_loss[3] / d gen, [B,1,H,W]; sign(0) = 0."""
    d, keep = _sobel_desc(gen, ir, y, mask, intensity, gradient)
    B, _, H, W = gen.shape
    df = torch.empty((B, 1, H, W), device=gen.device, dtype=torch.float32)
    g = g.detach().reshape(1).to(torch.float32).contiguous()
    _lib.check(lib().paif_sobel_loss_bwd(ctypes.byref(d), _p(g), _p(df), B, H, W, _stream()), "sobel_loss_bwd")
    return df


class SobelLoss(torch.autograd.Function):
    """The weighted sum of sobel_loss as a 0-d tensor, differentiable w.r.t. the generated image only."""

    @staticmethod
    def forward(ctx, gen, ir, y, mask, intensity, gradient):
        out = sobel_loss(gen, ir, y, mask, intensity, gradient)
        ctx.save_for_backward(*[t.detach() for t in (gen, ir, y, mask) if t is not None])
        ctx.have = [t is not None for t in (gen, ir, y, mask)]
        ctx.terms = (intensity, gradient)
        return out[3].clone()

    @staticmethod
    def backward(ctx, g):
        it = iter(ctx.saved_tensors)
        gen, ir, y, mask = [next(it) if h else None for h in ctx.have]
        return sobel_loss_bwd(gen, ir, y, mask, ctx.terms[0], ctx.terms[1], g), None, None, None, None, None


def sobel_criterion(gen, ir, y, mask, intensity, gradient):
    """sobel_loss's weighted sum with autograd: the gradient w.r.t. `gen` is built, the one w.r.t. ir / y / mask is refused."""
    if torch.is_grad_enabled():
        for t, name in ((ir, "image_ir"), (y, "image_vis"), (mask, "mask")):
            if t is not None and t.requires_grad:
                raise NotImplementedError("Sobel fusion criteria: the gradient w.r.t. %s is not built (only the generated image's is)" % name)
        if gen.requires_grad:
            return SobelLoss.apply(gen, ir, y, mask, tuple(intensity), gradient)
    with torch.no_grad():
        return sobel_loss(gen, ir, y, mask, intensity, gradient)[3].clone()


def sobelxy_bwd(x, g):
    """(x, cotangent map g), both [B,1,H,W] -> dx = Gx^T(g sign(Gx x)) + Gy^T(g sign(Gy x))."""
    if x.dim() != 4 or x.shape[1] != 1 or g.shape != x.shape:
        raise ValueError("sobelxy_bwd: expected two [B,1,H,W] maps, got %s and %s" % (tuple(x.shape), tuple(g.shape)))
    tx, px, bs = _plane0(x, x.shape, "Sobelxy input")
    B, _, H, W = x.shape
    g = g.detach().contiguous()
    dx = torch.empty((B, 1, H, W), device=x.device, dtype=torch.float32)
    _lib.check(lib().paif_sobelxy_bwd(px, bs, _p(g), _p(dx), B, H, W, _stream()), "sobelxy_bwd")
    return dx


class Sobelxy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x.detach())
        return sobelxy_fwd(x)

    @staticmethod
    def backward(ctx, g):
        return sobelxy_bwd(ctx.saved_tensors[0], g)


def sobelxy_fwd(x):
    if x.dim() != 4 or x.shape[1] != 1:
        raise ValueError("Sobelxy: expected a 1-channel map [B,1,H,W], got %s" % (tuple(x.shape),))
    tx, px, bs = _plane0(x, x.shape, "Sobelxy input")
    B, _, H, W = x.shape
    out = torch.empty((B, 1, H, W), device=x.device, dtype=torch.float32)
    _lib.check(lib().paif_sobelxy_fwd(px, bs, _p(out), B, H, W, _stream()), "sobelxy")
    return out


def sobelxy(x):
    """S(x) = |Gx * x| + |Gy * x| of a 1-channel map (core/loss.py:647-650), differentiable w.r.t. x."""
    if torch.is_grad_enabled() and x.requires_grad:
        return Sobelxy.apply(x)
    return sobelxy_fwd(x)


def layernorm(x, weight, bias, eps):
    C = x.shape[-1]
    y = torch.empty_like(x)
    _lib.check(lib().paif_layernorm_fwd(_p(x), _p(weight), _p(bias), _p(y), x.numel() // C, C, eps, _stream()), "layernorm")
    return y


def conv_out_size(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def im2col(x, k, stride, pad, kpad):
    """x NHWC [B,H,W,Cin] -> [B, OH, OW, kpad]."""
    B, H, W, Cin = x.shape
    OH, OW = conv_out_size(H, k, stride, pad), conv_out_size(W, k, stride, pad)
    col = torch.empty((B, OH, OW, kpad), device=x.device, dtype=torch.float32)
    _lib.check(lib().paif_im2col_fwd(_p(x), _p(col), B, H, W, Cin, k, stride, pad, kpad, _stream()), "im2col")
    return col


def conv_gemm(x, wp, k, stride, pad, shift=None, scale=None, act=ACT_NONE):
    """Strided k x k conv of an NHWC map as ONE GEMM: x [B,H,W,Cin], wp [N, Kpad] (pack_conv_gemm_weight) -> tokens [B, OH*OW, N], OH, OW.
    The A operand is gathered from the map inside the GEMM's loader (paif_gemm_conv_fwd: no im2col matrix in HBM; bit-identical to
    the pair) in two forms: 128-byte segments for Cin % 32 == 0 under a split-bf16 GEMM arithmetic (the SR convs, patch embeds 2-4), and
    element-wise through a column table for the exact fp32 MFMA at Kpad <= 160 (the 3-channel 7x7 patch embed 1).  Anything else:
    im2col + gemm."""
    B, H, W, Cin = x.shape
    N, kpad = wp.shape
    OH, OW = conv_out_size(H, k, stride, pad), conv_out_size(W, k, stride, pad)
    M, K = B * OH * OW, k * k * Cin
    prec = CONFIG["gemm_precision"]
    if prec == "auto":
        prec = "bf16x3" if (K >= 256 and M >= CONFIG["gemm_split_min_m"]) else "f32"
    elif prec == "auto6":
        prec = "bf16x6" if (K >= 256 and M >= CONFIG["gemm_split_min_m"]) else "f32"
    elif prec == "auto6h":
        prec = "f16x3" if (K >= CONFIG["f16x3_min_k"] and M >= CONFIG["gemm_split_min_m"]) else "f32"
    if Cin % 32 != 0 and kpad <= 160 and prec == "f16x3" and CONFIG["gemm_precision"] == "auto6h":
        prec = "f32"      # the 3-channel patch embed inside an attack loop: the exact gathered form beats im2col + a split GEMM
    split_form = prec in ("bf16x3", "bf16x6", "f16x3") and Cin % 32 == 0 and kpad == K
    exact_form = prec == "f32" and kpad <= 160 and kpad == (K + 31) // 32 * 32      # element-wise gather, any Cin (the 3-channel patch embed)
    if not CONFIG["gemm_gather"] or not (split_form or exact_form):
        col = im2col(x, k, stride, pad, kpad)
        return gemm(col.view(B, OH * OW, kpad), wp, scale=scale, shift=shift, act=act), OH, OW
    L = lib()
    splits = L.paif_gemm_splitk_plan(M, N, K) if split_form else 1
    out = torch.empty((B, OH * OW, N), device=x.device, dtype=torch.float32)
    ws = torch.empty(splits * M * N, device=x.device, dtype=torch.float32) if splits > 1 else None
    tag = "gemm_mfma_%s" % prec
    e0 = TIMER.start(tag) if TIMER is not None else None
    _lib.check(L.paif_gemm_conv_fwd(_p(x), B, H, W, Cin, k, stride, pad, _p(wp), _p(scale), _p(shift), act, None, 0, _p(out), N, N,
                                    _PREC_CODE[prec], splits, _p(ws), _stream()), "gemm_conv")
    if e0 is not None:
        TIMER.stop(tag, e0, 2 * M * N * kpad, 4 * (M * kpad + N * kpad + M * N))
    return out, OH, OW


def pack_conv_gemm_weight(w):
    """[Cout,Cin,k,k] -> [Cout,Kpad] (Kpad = k*k*Cin rounded up to a multiple of 32)."""
    Cout, Cin, k, k2 = w.shape
    assert k == k2
    kpad = (k * k * Cin + 31) // 32 * 32
    out = torch.empty((Cout, kpad), device=w.device, dtype=torch.float32)
    _lib.check(lib().paif_pack_conv_gemm_weight(_p(w.detach().contiguous()), _p(out), Cout, Cin, k, kpad, _stream()), "pack_conv_gemm_weight")
    return out


def dwconv3_bias_gelu(x, w, bias):
    B, H, W, C = x.shape
    y = torch.empty_like(x)
    _lib.check(lib().paif_dwconv3_bias_gelu_fwd(_p(x), _p(w.detach().contiguous()), _p(bias), _p(y), B, H, W, C, _stream()), "dwconv3_bias_gelu")
    return y


def sr_attention(q, kv, heads, want_lse=False):
    """q [B,N,C], kv [B,Nk,2C] -> [B,N,C] (and the per-query log-sum-exp [B,heads,N] for the backward)."""
    B, N, C = q.shape
    Nk = kv.shape[1]
    assert kv.shape[2] == 2 * C
    out = torch.empty_like(q)
    lse = torch.empty((B, heads, N), device=q.device, dtype=torch.float32) if want_lse else None
    split = _attn_precision()
    tag = {0: "sr_attention", 1: "sr_attention_bf16x3", 3: "sr_attention_bf16x6", 6: "sr_attention_f16x3"}[split]
    e0 = TIMER.start(tag) if TIMER is not None else None
    if split:
        _lib.check(lib().paif_sr_attention_split_fwd(_p(q), _p(kv), _p(out), _p(lse), B, N, Nk, C, heads, split, _stream()), "sr_attention")
    else:
        _lib.check(lib().paif_sr_attention_fwd(_p(q), _p(kv), _p(out), _p(lse), B, N, Nk, C, heads, _stream()), "sr_attention")
    if e0 is not None:
        TIMER.stop(tag, e0, 4 * B * N * Nk * C, 4 * (2 * B * N * C + 2 * B * Nk * C))
    return (out, lse) if want_lse else out


def _self_attention_check(qkv, heads):
    _p(qkv)
    if qkv.dim() != 3 or heads < 1 or qkv.shape[-1] != 192 * heads:
        raise ValueError("self_attention: qkv must be [B, N, 192 * heads] (head dim 64), got %s for heads=%d" % (tuple(qkv.shape), heads))
    return qkv.shape[0], qkv.shape[1]


def self_attention(qkv, heads, want_lse=False):
    """SelfPath's attention core (operations_m.py:31-61) on the to_qkv GEMM's output as it stands: qkv [B,N,192*heads] (q | k | v column
    blocks, head hd at 64*hd in each) -> out [B,N,64*heads] (and lse [B,heads,N] for the reverse pass).  Flash form: no N x N tensor."""
    B, N = _self_attention_check(qkv, heads)
    L = lib()
    nws = L.paif_self_attention_workspace_bytes(B, N, heads)
    if nws == 0:
        raise NotImplementedError("self_attention: B=%d N=%d heads=%d is not built" % (B, N, heads))
    ws = torch.empty(nws, device=qkv.device, dtype=torch.uint8)
    out = torch.empty((B, N, 64 * heads), device=qkv.device, dtype=torch.float32)
    lse = torch.empty((B, heads, N), device=qkv.device, dtype=torch.float32) if want_lse else None
    tag = "self_attention_f16x3"
    e0 = TIMER.start(tag) if TIMER is not None else None
    _lib.check(L.paif_self_attention_fwd(_p(qkv), _p(out), _p(lse), ctypes.c_void_p(ws.data_ptr()), B, N, heads, _stream()), "self_attention")
    if e0 is not None:
        TIMER.stop(tag, e0, 4 * B * heads * N * N * 64, 4 * B * N * 256 * heads)
    return (out, lse) if want_lse else out


def self_attention_bwd(qkv, out, dout, lse, heads):
    """d(qkv) [B,N,192*heads] of self_attention from d(out) and the saved lse.  `out` may be None: the kernels do not read it (they form
    delta from the recomputed P), so a caller need not keep it.  Deterministic (no atomics)."""
    B, N = _self_attention_check(qkv, heads)
    L = lib()
    nws = L.paif_self_attention_bwd_workspace_bytes(B, N, heads)
    if nws == 0:
        raise NotImplementedError("self_attention_bwd: B=%d N=%d heads=%d is not built" % (B, N, heads))
    assert tuple(dout.shape) == (B, N, 64 * heads) and tuple(lse.shape) == (B, heads, N) and (out is None or tuple(out.shape) == tuple(dout.shape))
    ws = torch.empty(nws, device=qkv.device, dtype=torch.uint8)
    dqkv = torch.empty_like(qkv)
    tag = "self_attention_bwd_f32"
    e0 = TIMER.start(tag) if TIMER is not None else None
    _lib.check(L.paif_self_attention_bwd_input(_p(qkv), _p(out), _p(dout.contiguous()), _p(lse), _p(dqkv), ctypes.c_void_p(ws.data_ptr()),
                                               B, N, heads, _stream()), "self_attention_bwd")
    if e0 is not None:
        TIMER.stop(tag, e0, 16 * B * heads * N * N * 64, 4 * B * N * (192 + 192 + 64) * heads)      # eight N x N x 64 products
    return dqkv


def resize_bilinear_into(x, out, coff):
    """x NHWC [B,IH,IW,C] -> bilinear (align_corners=False) into out[B,OH,OW,coff:coff+C]."""
    B, IH, IW, C = x.shape
    _, OH, OW, ldo = out.shape
    _lib.check(lib().paif_resize_bilinear_into_fwd(_p(x), _p(out), B, IH, IW, C, OH, OW, ldo, coff, _stream()), "resize_bilinear_into")
    return out


def head_sum(zs, scale, shift):
    """relu((z1 + up z2 + up z3 + up z4) * scale + shift): zs = 4 NHWC maps, the first at the output resolution."""
    B, H1, W1, C = zs[0].shape
    hw = (ctypes.c_int * 8)(*[d for z in zs for d in z.shape[1:3]])
    out = torch.empty_like(zs[0])
    _lib.check(lib().paif_head_sum_fwd(_p(zs[0]), _p(zs[1]), _p(zs[2]), _p(zs[3]), hw, _p(scale), _p(shift), _p(out), B, C, _stream()), "head_sum")
    return out


def relu_mask_scale(dx, x, scale):
    C = x.shape[-1]
    out = torch.empty_like(x)
    _lib.check(lib().paif_relu_mask_scale_fwd(_p(dx), _p(x), _p(scale), _p(out), x.numel() // C, C, _stream()), "relu_mask_scale")
    return out


def nhwc_to_nchw(x):
    B, H, W, C = x.shape
    y = torch.empty((B, C, H, W), device=x.device, dtype=torch.float32)
    _lib.check(lib().paif_nhwc_to_nchw_fwd(_p(x), _p(y), B, H * W, C, _stream()), "nhwc_to_nchw")
    return y


def nchw_to_nhwc(x):
    x = x.contiguous()
    B, C, H, W = x.shape
    y = torch.empty((B, H, W, C), device=x.device, dtype=torch.float32)
    _lib.check(lib().paif_nchw_to_nhwc_fwd(_p(x), _p(y), B, H * W, C, _stream()), "nchw_to_nhwc")
    return y


# ---------------------------------------------------------------------------------------------
# glue backward, PGD update
# ---------------------------------------------------------------------------------------------
def glue_bwd(dseg, fused, ycc, minmax, dfused_direct=None):
    """d/d(seg_in) NCHW [B,3,H,W] -> (d/d(fused) [B,1,H,W], d/d(Cr,Cb) [B,2,H,W])."""
    B, _, H, W = ycc.shape
    L = lib()
    partial = torch.empty(4 * L.paif_glue_bwd_blocks(B, H, W), device=ycc.device, dtype=torch.float32)
    dfused = torch.empty((B, 1, H, W), device=ycc.device, dtype=torch.float32)
    dcrcb = torch.empty((B, 2, H, W), device=ycc.device, dtype=torch.float32)
    _lib.check(L.paif_glue_bwd_input(_p(dseg.contiguous()), _p(fused), _p(ycc), _p(minmax), _p(dfused_direct), _p(partial), _p(dfused),
                                     _p(dcrcb), B, H, W, _stream()), "glue_bwd")
    return dfused, dcrcb


def plane_clamp_minmax(x):
    """forward_object's extra step (core/model_fusion_auto.py:743-751): clamp to [0,1], batch-global min-max.
    x [B,1,H,W] -> (normalised plane, the 2 floats (min, max) the backward needs)."""
    x = x.contiguous()
    L = lib()
    n = x.numel()
    partial = torch.empty(2 * L.paif_plane_minmax_blocks(n), device=x.device, dtype=torch.float32)
    out = torch.empty_like(x)
    mm = torch.empty(2, device=x.device, dtype=torch.float32)
    _lib.check(L.paif_plane_clamp_minmax_fwd(_p(x), _p(out), _p(partial), _p(mm), n, _stream()), "plane_clamp_minmax")
    return out, mm


def plane_clamp_minmax_bwd(dout, x, mm):
    x = x.contiguous()
    L = lib()
    n = x.numel()
    partial = torch.empty(4 * L.paif_plane_minmax_blocks(n), device=x.device, dtype=torch.float32)
    dx = torch.empty_like(x)
    _lib.check(L.paif_plane_clamp_minmax_bwd_input(_p(dout.contiguous()), _p(x), _p(mm), _p(partial), _p(dx), n, _stream()),
               "plane_clamp_minmax_bwd")
    return dx


def rgb2ycrcb_bwd(dY, dcrcb):
    B, _, H, W = dcrcb.shape
    dvis = torch.empty((B, 3, H, W), device=dcrcb.device, dtype=torch.float32)
    _lib.check(lib().paif_rgb2ycrcb_bwd_input(_p(dY.contiguous()), _p(dcrcb), _p(dvis), B, H, W, _stream()), "rgb2ycrcb_bwd")
    return dvis


def pgd_step_(delta, grad_sum, X, alpha, eps):
    _lib.check(lib().paif_pgd_step(_p(delta), _p(grad_sum), _p(X), alpha, eps, delta.numel(), _stream()), "pgd_step")
    return delta


def axpy_(y, x, a=1.0):
    _lib.check(lib().paif_axpy(_p(y), _p(x), a, y.numel(), _stream()), "axpy")
    return y


# ---------------------------------------------------------------------------------------------
# evaluation harness
# ---------------------------------------------------------------------------------------------
def upsample_argmax(logits_nhwc, OH, OW):
    B, IH, IW, C = logits_nhwc.shape
    pred = torch.empty((B, OH, OW), device=logits_nhwc.device, dtype=torch.int64)
    _lib.check(lib().paif_upsample_argmax_fwd(_p(logits_nhwc), ctypes.c_void_p(pred.data_ptr()), B, IH, IW, C, OH, OW, _stream()),
               "upsample_argmax")
    return pred


def confusion_matrix_accum_(conf, label, pred, ncls):
    """conf: int64 [ncls, ncls] device tensor (rows = label, cols = prediction), accumulated in place."""
    assert conf.dtype == torch.int64 and conf.is_contiguous() and label.dtype == torch.int64 and pred.dtype == torch.int64
    label, pred = label.contiguous(), pred.contiguous()
    _lib.check(lib().paif_confusion_matrix_accum(ctypes.c_void_p(label.data_ptr()), ctypes.c_void_p(pred.data_ptr()),
                                                 ctypes.c_void_p(conf.data_ptr()), label.numel(), ncls, _stream()), "confusion_matrix")
    return conf


# ---------------------------------------------------------------------------------------------
# SPAattention
# ---------------------------------------------------------------------------------------------
def spa1(o, r, w, k, prelu, save=False, want_comp=False):
    B, H, W, _ = o.shape
    comp = torch.empty((B, H, W, 2), device=o.device, dtype=torch.float32)
    out = torch.empty_like(o)
    s = torch.empty((B, H, W), device=o.device, dtype=torch.float32) if save else None
    u = torch.empty_like(o) if save else None
    _lib.check(lib().paif_spa1_fwd(_p(o), _p(r), _p(w.detach().contiguous()), k, _p(prelu), _p(comp), _p(s), _p(u), _p(out), B, H, W, _stream()),
               "spa1")
    if want_comp:
        return out, u, s, comp
    return (out, u, s) if save else out


def spa1_bwd(dout, u, o, s, w, k, prelu, want_dpre=False):
    B, H, W, _ = o.shape
    dpre = torch.empty((B, H, W), device=o.device, dtype=torch.float32)
    d_o, d_r = torch.empty_like(o), torch.empty_like(o)
    _lib.check(lib().paif_spa1_bwd_input(_p(dout), _p(u), _p(o), _p(s), _p(w.detach().contiguous()), k, _p(prelu), _p(dpre), _p(d_o), _p(d_r),
                                         B, H, W, _stream()), "spa1_bwd")
    return (d_o, d_r, dpre) if want_dpre else (d_o, d_r)


# ---------------------------------------------------------------------------------------------
# ReCoNet baseline (csrc/reconet.hip; fusion_model/reconet.py is the module)
# ---------------------------------------------------------------------------------------------
def _plane(t):
    """([B,1,H,W] fp32 device view whose planes are dense) -> (pointer, batch stride in floats): a channel slice of a dense
    [B,C,H,W] tensor is passed as it is, anything else is made dense first."""
    if not t.is_cuda:
        raise RuntimeError("paif_amd ops need CUDA(HIP) tensors; got a %s tensor -- there is no CPU path" % t.device)
    if t.dtype != torch.float32:
        raise TypeError("expected float32, got %s" % t.dtype)
    B, C, H, W = t.shape
    assert C == 1, "a 1-channel plane is expected, got %d channels" % C
    if not ((W == 1 or t.stride(3) == 1) and (H == 1 or t.stride(2) == W) and (B == 1 or t.stride(0) >= H * W)):
        t = t.contiguous()
    return t, ctypes.c_void_p(t.data_ptr()), (t.stride(0) if B > 1 else H * W)


def reconet_pack(att_a_w, att_b_w, groups, w_s, b_s, dim):
    """groups: three (conv weight [dim,3,3,3], conv bias, bn) with bn = None or (gamma, beta, running_mean, running_var, eps)
    -> the kernels' weight layout (eval-mode BatchNorm folded into weight and bias)."""
    dev = w_s.device
    pack = torch.empty(lib().paif_reconet_pack_floats(dim), device=dev, dtype=torch.float32)
    c = lambda t: t.detach().contiguous()
    ws = c(w_s)
    _lib.check(lib().paif_reconet_pack_head(_p(c(att_a_w)), _p(c(att_b_w)), _p(c(b_s)), _p(pack), _stream()), "reconet_pack_head")
    for g, (w, b, bn) in enumerate(groups):
        ga, be, mu, var, eps = (c(bn[0]), c(bn[1]), c(bn[2]), c(bn[3]), bn[4]) if bn is not None else (None, None, None, None, 0.0)
        _lib.check(lib().paif_reconet_pack_group(_p(c(w)), _p(c(b)), _p(ga), _p(be), _p(mu), _p(var), eps, _p(ws), dim, g, _p(pack), _stream()),
                   "reconet_pack_group")
    return pack


def reconet_init(i1, i2, use_max):
    B, _, H, W = i1.shape
    i1, p1, s1 = _plane(i1)
    i2, p2, s2 = _plane(i2)
    out = torch.empty((B, 1, H, W), device=i1.device, dtype=torch.float32)
    _lib.check(lib().paif_reconet_init(p1, s1, p2, s2, int(use_max), _p(out), B, H, W, _stream()), "reconet_init")
    return out


def reconet_init_bwd_(d_i1, d_i2, i1, i2, use_max, d_f0):
    """d_i1, d_i2 += the initialisation's share of d_f0 (in place)."""
    B, _, H, W = i1.shape
    i1, p1, s1 = _plane(i1)
    i2, p2, s2 = _plane(i2)
    _lib.check(lib().paif_reconet_init_bwd(p1, s1, p2, s2, int(use_max), _p(d_f0), _p(d_i1), _p(d_i2), B, H, W, _stream()), "reconet_init_bwd")


def reconet_step(i1, i2, f_prev, pack, dim, want_att=False):
    """One recurrence: -> f_next, or (f_next, att_a, att_b)."""
    B, _, H, W = i1.shape
    i1, p1, s1 = _plane(i1)
    i2, p2, s2 = _plane(i2)
    f_next = torch.empty((B, 1, H, W), device=i1.device, dtype=torch.float32)
    att_a = torch.empty_like(f_next) if want_att else None
    att_b = torch.empty_like(f_next) if want_att else None
    _lib.check(lib().paif_reconet_step_fwd(p1, s1, p2, s2, _p(f_prev), _p(pack), dim, _p(f_next), _p(att_a), _p(att_b), B, H, W, _stream()),
               "reconet_step_fwd")
    return (f_next, att_a, att_b) if want_att else f_next


def reconet_step_bwd(i1, i2, f_prev, att_a, att_b, f_next, d_f_next, pack, dim, d_i1, d_i2, workspace, accumulate):
    """Reverse of one recurrence: d_i1, d_i2 written (accumulate False) or added to, -> d_f_prev."""
    B, _, H, W = i1.shape
    i1, p1, s1 = _plane(i1)
    i2, p2, s2 = _plane(i2)
    d_f_prev = torch.empty((B, 1, H, W), device=i1.device, dtype=torch.float32)
    _lib.check(lib().paif_reconet_step_bwd(p1, s1, p2, s2, _p(f_prev), _p(att_a), _p(att_b), _p(f_next), _p(d_f_next), _p(pack), dim, _p(d_i1), _p(d_i2),
                                           _p(d_f_prev), _p(workspace), int(accumulate), B, H, W, _stream()), "reconet_step_bwd")
    return d_f_prev


# ---------------------------------------------------------------------------------------------
# SDNet baseline (csrc/sdnet.hip; fusion_model/sdnet.py is the module)
# ---------------------------------------------------------------------------------------------
def sdnet_pack(convs):
    """convs: nine (layer, encoder, weight, bias) -- layer 0 the 5x5 stems, 1..3 the dense 3x3 convs, 4 the fuse 1x1 -> the kernels'
    weight layout (the dense convs in MFMA operand order, forward and reverse)."""
    dev = convs[0][2].device
    pack = torch.zeros(lib().paif_sdnet_pack_floats(), device=dev, dtype=torch.float32)
    for layer, enc, w, b in convs:
        _lib.check(lib().paif_sdnet_pack_conv(_p(w.detach().contiguous()), _p(b.detach().contiguous()), layer, enc, _p(pack), _stream()),
                   "sdnet_pack_conv")
    return pack


def sdnet_forward(x1, x2, pack):
    """Two [B,1,H,W] planes -> (feat [2,4,B,H,W,16]: the eight LeakyReLU maps, NHWC; fused [B,1,H,W]).  Five launches."""
    B, _, H, W = x1.shape
    x1, p1, s1 = _plane(x1)
    x2, p2, s2 = _plane(x2)
    L = lib()
    feat = torch.empty((2, 4, B, H, W, 16), device=x1.device, dtype=torch.float32)
    out = torch.empty((B, 1, H, W), device=x1.device, dtype=torch.float32)
    _lib.check(L.paif_sdnet_stem_fwd(p1, s1, p2, s2, _p(pack), _p(feat), B, H, W, _stream()), "sdnet_stem_fwd")
    for level in (1, 2, 3):
        _lib.check(L.paif_sdnet_dense_fwd(_p(pack), _p(feat), level, B, H, W, _stream()), "sdnet_dense_fwd")
    _lib.check(L.paif_sdnet_fuse_fwd(_p(pack), _p(feat), _p(out), B, H, W, _stream()), "sdnet_fuse_fwd")
    return feat, out


def sdnet_backward(feat, out, d_out, pack):
    """Reverse of sdnet_forward (input gradients) from the taped maps and fused plane -> (d_x1, d_x2) [B,1,H,W].  Five launches."""
    B, _, H, W = out.shape
    L = lib()
    d_out = d_out.contiguous()
    dfeat = torch.empty_like(feat)
    d1, d2 = torch.empty_like(out), torch.empty_like(out)
    _lib.check(L.paif_sdnet_fuse_bwd(_p(pack), _p(out), _p(d_out), _p(dfeat), B, H, W, _stream()), "sdnet_fuse_bwd")
    for level in (3, 2, 1):
        _lib.check(L.paif_sdnet_dense_bwd(_p(pack), _p(feat), _p(dfeat), level, B, H, W, _stream()), "sdnet_dense_bwd")
    _lib.check(L.paif_sdnet_stem_bwd(_p(pack), _p(feat), _p(dfeat), _p(d1), _p(d2), B, H, W, _stream()), "sdnet_stem_bwd")
    return d1, d2


# ---------------------------------------------------------------------------------------------
# U2Fusion baseline (csrc/u2fusion.hip; fusion_model/u2fusion.py is the module)
# ---------------------------------------------------------------------------------------------
def u2fusion_pack(convs):
    """convs: the ten (weight, bias) in layer order -- conv_1, dense_layers.0..4, sub.0..3 -> the kernels' weight layout (layers 1..8 in
    MFMA operand order, forward and transposed)."""
    dev = convs[0][0].device
    pack = torch.zeros(lib().paif_u2fusion_pack_floats(), device=dev, dtype=torch.float32)
    for layer, (w, b) in enumerate(convs):
        _lib.check(lib().paif_u2fusion_pack_conv(_p(w.detach().contiguous()), _p(b.detach().contiguous()), layer, _p(pack), _stream()),
                   "u2fusion_pack_conv")
    return pack


def u2fusion_forward(x_over, x_under, pack):
    """Two [B,1,H,W] planes -> ((cat [B,H,W,264], s1 [B,H,W,128], s2 [B,H,W,64], s3 [B,H,W,32]): the nine LeakyReLU maps, NHWC;
    fused [B,1,H,W]).  Ten launches."""
    B, _, H, W = x_over.shape
    x_over, p1, s1_ = _plane(x_over)
    x_under, p2, s2_ = _plane(x_under)
    L = lib()
    dev = x_over.device
    cat, s1, s2, s3 = (torch.empty((B, H, W, c), device=dev, dtype=torch.float32) for c in (264, 128, 64, 32))
    fused = torch.empty((B, 1, H, W), device=dev, dtype=torch.float32)
    _lib.check(L.paif_u2fusion_stem_fwd(p1, s1_, p2, s2_, _p(pack), _p(cat), B, H, W, _stream()), "u2fusion_stem_fwd")
    for layer, src, dst in ((1, cat, cat), (2, cat, cat), (3, cat, cat), (4, cat, cat), (5, cat, cat), (6, cat, s1), (7, s1, s2), (8, s2, s3)):
        _lib.check(L.paif_u2fusion_conv_fwd(_p(pack), layer, _p(src), _p(dst), B, H, W, _stream()), "u2fusion_conv_fwd")
    _lib.check(L.paif_u2fusion_head_fwd(_p(pack), _p(s3), _p(fused), B, H, W, _stream()), "u2fusion_head_fwd")
    return (cat, s1, s2, s3), fused


def u2fusion_backward(cat, s1, s2, s3, fused, d_fused, pack):
    """Reverse of u2fusion_forward (input gradients) from the taped maps and fused plane -> (d_x_over, d_x_under) [B,1,H,W].  Ten launches;
    nothing is recomputed and nothing needs a memset."""
    B, _, H, W = fused.shape
    L = lib()
    d_fused = d_fused.contiguous()
    d_cat, d_s1, d_s2, d_s3 = (torch.empty_like(m) for m in (cat, s1, s2, s3))
    d1, d2 = torch.empty_like(fused), torch.empty_like(fused)
    _lib.check(L.paif_u2fusion_head_bwd(_p(pack), _p(fused), _p(d_fused), _p(d_s3), B, H, W, _stream()), "u2fusion_head_bwd")
    for layer, taped, d_out, d_in in ((8, s3, d_s3, d_s2), (7, s2, d_s2, d_s1), (6, s1, d_s1, d_cat), (5, cat, d_cat, d_cat), (4, cat, d_cat, d_cat),
                                      (3, cat, d_cat, d_cat), (2, cat, d_cat, d_cat), (1, cat, d_cat, d_cat)):
        _lib.check(L.paif_u2fusion_conv_bwd(_p(pack), layer, _p(taped), _p(d_out), _p(d_in), B, H, W, _stream()), "u2fusion_conv_bwd")
    _lib.check(L.paif_u2fusion_stem_bwd(_p(pack), _p(cat), _p(d_cat), _p(d1), _p(d2), B, H, W, _stream()), "u2fusion_stem_bwd")
    return d1, d2


# ---------------------------------------------------------------------------------------------
# SeAFusion baseline (csrc/seafusion.hip, csrc/conv_slab.h; fusion_model/seafusion.py is the module)
# ---------------------------------------------------------------------------------------------
def _pb(t):
    """Device pointer of a dense uint8 CUDA tensor (the sign tapes)."""
    if not t.is_cuda or t.dtype != torch.uint8 or not t.is_contiguous():
        raise RuntimeError("expected a dense uint8 CUDA tensor")
    return ctypes.c_void_p(t.data_ptr())


def seafusion_pack(convs):
    """convs: the thirty (weight, bias or None) in paif_amd.synthetic.SEAFUSION_CONVS order -> the kernels' weight layout (the 3x3 and
    1x1 convs in MFMA operand order, forward and transposed; the two 1x1 of an RGBD side by side in one pack)."""
    dev = convs[0][0].device
    pack = torch.zeros(lib().paif_seafusion_pack_floats(), device=dev, dtype=torch.float32)
    for conv, (w, b) in enumerate(convs):
        _lib.check(lib().paif_seafusion_pack_conv(_p(w.detach().contiguous()), None if b is None else _p(b.detach().contiguous()), conv,
                                                  _p(pack), _stream()), "seafusion_pack_conv")
    return pack


def seafusion_forward(x_vis, x_inf, pack):
    """Two [B,1,H,W] planes (the reference's image_vis[:, :1] and image_ir) -> (maps, fused [B,1,H,W]).  maps: slab1 [B,H,W,64] and slab2
    [B,H,W,128] per stream (vis first), enc [B,H,W,96], dec4 / dec3 / dec2 [B,H,W,64 / 32 / 16], all fp32 NHWC, and sgn: the four sign
    tapes [B,H,W,C] uint8 of the depthwise pairs.  22 launches."""
    B, _, H, W = x_vis.shape
    L = lib()
    dev = x_vis.device
    planes = [_plane(x_vis), _plane(x_inf)]

    def new(c, dtype=torch.float32):
        return torch.empty((B, H, W, c), device=dev, dtype=dtype)

    slab1, slab2 = [new(64), new(64)], [new(128), new(128)]
    enc, dec4, dec3, dec2 = new(96), new(64), new(32), new(16)
    sgn = [new(16 << (k & 1), torch.uint8) for k in range(4)]
    fused = torch.empty((B, 1, H, W), device=dev, dtype=torch.float32)
    for s in range(2):
        _, p, sb = planes[s]
        _lib.check(L.paif_seafusion_stem_fwd(p, sb, _p(pack), s, _p(slab1[s]), B, H, W, _stream()), "seafusion_stem_fwd")
        for r, slab, out in ((0, slab1[s], slab2[s]), (1, slab2[s], enc)):
            k = 2 * s + r
            for layer in (2 * k, 2 * k + 1):
                _lib.check(L.paif_seafusion_conv_fwd(_p(pack), layer, _p(slab), _p(slab), B, H, W, _stream()), "seafusion_conv_fwd")
            _lib.check(L.paif_seafusion_sobel_fwd(_p(pack), k, _p(slab), _pb(sgn[k]), B, H, W, _stream()), "seafusion_sobel_fwd")
            _lib.check(L.paif_seafusion_tail_fwd(_p(pack), k, _p(slab), _p(out), B, H, W, _stream()), "seafusion_tail_fwd")
    for layer, src, dst in ((8, enc, dec4), (9, dec4, dec3), (10, dec3, dec2)):
        _lib.check(L.paif_seafusion_conv_fwd(_p(pack), layer, _p(src), _p(dst), B, H, W, _stream()), "seafusion_conv_fwd")
    _lib.check(L.paif_seafusion_head_fwd(_p(pack), _p(dec2), _p(fused), B, H, W, _stream()), "seafusion_head_fwd")
    return dict(slab1=slab1, slab2=slab2, enc=enc, dec4=dec4, dec3=dec3, dec2=dec2, sgn=sgn), fused


def seafusion_backward(maps, fused, d_fused, pack):
    """Reverse of seafusion_forward (input gradients) from the taped maps and fused plane -> (d_x_vis, d_x_inf) [B,1,H,W].  22 launches;
    nothing is recomputed and nothing needs a memset."""
    B, _, H, W = fused.shape
    L = lib()
    d_fused = d_fused.contiguous()
    enc, dec4, dec3, dec2 = maps["enc"], maps["dec4"], maps["dec3"], maps["dec2"]
    d_enc, d_dec4, d_dec3, d_dec2 = (torch.empty_like(m) for m in (enc, dec4, dec3, dec2))
    _lib.check(L.paif_seafusion_head_bwd(_p(pack), _p(fused), _p(d_fused), _p(d_dec2), B, H, W, _stream()), "seafusion_head_bwd")
    for layer, taped, d_out, d_in in ((10, dec2, d_dec2, d_dec3), (9, dec3, d_dec3, d_dec4), (8, dec4, d_dec4, d_enc)):
        _lib.check(L.paif_seafusion_conv_bwd(_p(pack), layer, _p(taped), _p(d_out), _p(d_in), B, H, W, _stream()), "seafusion_conv_bwd")
    grads = []
    for s in range(2):
        slab1, slab2 = maps["slab1"][s], maps["slab2"][s]
        d_slab1, d_slab2 = torch.empty_like(slab1), torch.empty_like(slab2)
        for r, slab, d_slab, out, d_out in ((1, slab2, d_slab2, enc, d_enc), (0, slab1, d_slab1, slab2, d_slab2)):
            k = 2 * s + r
            _lib.check(L.paif_seafusion_tail_bwd(_p(pack), k, _p(out), _p(d_out), _p(d_slab), B, H, W, _stream()), "seafusion_tail_bwd")
            _lib.check(L.paif_seafusion_sobel_bwd(_p(pack), k, _pb(maps["sgn"][k]), _p(d_slab), B, H, W, _stream()), "seafusion_sobel_bwd")
            for layer in (2 * k + 1, 2 * k):
                _lib.check(L.paif_seafusion_conv_bwd(_p(pack), layer, _p(slab), _p(d_slab), _p(d_slab), B, H, W, _stream()), "seafusion_conv_bwd")
        d_x = torch.empty_like(fused)
        _lib.check(L.paif_seafusion_stem_bwd(_p(pack), s, _p(slab1), _p(d_slab1), _p(d_x), B, H, W, _stream()), "seafusion_stem_bwd")
        grads.append(d_x)
    return grads[0], grads[1]


# ---------------------------------------------------------------------------------------------
# DIDFuse baseline (csrc/didfuse.hip, csrc/conv_slab.h; fusion_model/didfuse.py is the module)
# ---------------------------------------------------------------------------------------------
class DidfusePack:
    """The packed weights of DIDFuse (BatchNorm folded in) and the six PReLU slopes as Python floats, in module order: per encoder cov1,
    cov2; then cov5, cov6."""

    __slots__ = ("weights", "slopes")

    def __init__(self, weights, slopes):
        self.weights, self.slopes = weights, tuple(float(s) for s in slopes)


def didfuse_pack(convs, slopes):
    """convs: the eleven (Conv2d weight, bias, BatchNorm2d weight, bias, running_mean, running_var, eps) in paif_amd.synthetic.DIDFUSE_CONVS
    order; slopes: the six PReLU slopes (one-element tensors or floats), read to the host HERE, once per pack -> DidfusePack.  The fold
    gamma * rsqrt(var + eps) runs on the device in fp32.  A negative slope is refused: the reverse pass reads the PReLU branch off the taped
    output."""
    if len(convs) != 11 or len(slopes) != 6:
        raise ValueError("didfuse_pack: eleven convs and six PReLU slopes are expected, got %d and %d" % (len(convs), len(slopes)))
    host = [float(s.detach().reshape(-1)[0]) if torch.is_tensor(s) else float(s) for s in slopes]
    for k, s in enumerate(host):
        if not s >= 0.0:
            raise ValueError("DIDFuse: PReLU slope %d is %g; the reverse pass reads the branch off the taped output, which is right for "
                             "slopes >= 0 only" % (k, s))
    dev = convs[0][0].device
    pack = torch.zeros(lib().paif_didfuse_pack_floats(), device=dev, dtype=torch.float32)
    for conv, (w, b, g, be, mu, var, eps) in enumerate(convs):
        ptrs = [_p(x.detach().contiguous()) for x in (w, b, g, be, mu, var)]
        _lib.check(lib().paif_didfuse_pack_conv(*ptrs, float(eps), conv, _p(pack), _stream()), "didfuse_pack_conv")
    return DidfusePack(pack, host)


def didfuse_forward(x_over, x_under, pack):
    """Two [B,1,H,W] planes -> (maps, fused [B,1,H,W]).  maps: enc [B,H,W,256] per stream (f1 | f2 | fB | fD; x_over first), bd = F_b | F_d,
    d1 = Out1 | F_2, d2 = Out2 | F_1 [B,H,W,128], all fp32 NHWC.  Ten launches; the means are written by the second stream's launches."""
    B, _, H, W = x_over.shape
    L = lib()
    dev = x_over.device
    planes = [_plane(x_over), _plane(x_under)]
    wp, sl = _p(pack.weights), pack.slopes

    def new(c):
        return torch.empty((B, H, W, c), device=dev, dtype=torch.float32)

    enc, bd, d1, d2 = [new(256), new(256)], new(128), new(128), new(128)
    fused = torch.empty((B, 1, H, W), device=dev, dtype=torch.float32)
    for s in range(2):
        _, p, sb = planes[s]
        e, pair = _p(enc[s]), (_p(enc[0]) if s else None)
        _lib.check(L.paif_didfuse_stem_fwd(p, sb, wp, s, sl[2 * s], e, pair, _p(d2) if s else None, B, H, W, _stream()), "didfuse_stem_fwd")
        _lib.check(L.paif_didfuse_conv_fwd(wp, 2 * s, sl[2 * s + 1], e, e, pair, _p(d1) if s else None, B, H, W, _stream()), "didfuse_conv_fwd")
        _lib.check(L.paif_didfuse_conv_fwd(wp, 2 * s + 1, 0.0, e, e, pair, _p(bd) if s else None, B, H, W, _stream()), "didfuse_conv_fwd")
    _lib.check(L.paif_didfuse_conv_fwd(wp, 4, sl[4], _p(bd), _p(d1), None, None, B, H, W, _stream()), "didfuse_conv_fwd")
    _lib.check(L.paif_didfuse_conv_fwd(wp, 5, sl[5], _p(d1), _p(d2), None, None, B, H, W, _stream()), "didfuse_conv_fwd")
    _lib.check(L.paif_didfuse_head_fwd(wp, _p(d2), _p(fused), B, H, W, _stream()), "didfuse_head_fwd")
    return dict(enc=enc, bd=bd, d1=d1, d2=d2), fused


def didfuse_backward(maps, fused, d_fused, pack):
    """Reverse of didfuse_forward (input gradients) from the taped maps and fused plane -> (d_x_over, d_x_under) [B,1,H,W].  Nine
    launches; nothing is recomputed and nothing needs a memset."""
    B, _, H, W = fused.shape
    L = lib()
    d_fused = d_fused.contiguous()
    wp, sl = _p(pack.weights), pack.slopes
    d_d2, d_d1, d_bd, dg = (torch.empty_like(maps["bd"]) for _ in range(4))
    _lib.check(L.paif_didfuse_head_bwd(wp, _p(fused), _p(d_fused), _p(d_d2), B, H, W, _stream()), "didfuse_head_bwd")
    _lib.check(L.paif_didfuse_conv_bwd(wp, 5, sl[5], _p(maps["d2"]), _p(d_d2), _p(d_d1), None, B, H, W, _stream()), "didfuse_conv_bwd")
    _lib.check(L.paif_didfuse_conv_bwd(wp, 4, sl[4], _p(maps["d1"]), _p(d_d1), _p(d_bd), None, B, H, W, _stream()), "didfuse_conv_bwd")
    grads = []
    for s in range(2):      # dg is reused: the second stream's launches follow the first's on the same HIP stream
        e = _p(maps["enc"][s])
        _lib.check(L.paif_didfuse_conv_bwd(wp, 2 * s + 1, 0.0, e, _p(d_bd), _p(dg), None, B, H, W, _stream()), "didfuse_conv_bwd")
        _lib.check(L.paif_didfuse_conv_bwd(wp, 2 * s, sl[2 * s + 1], e, _p(dg), _p(dg), _p(d_d1), B, H, W, _stream()), "didfuse_conv_bwd")
        d_x = torch.empty_like(fused)
        _lib.check(L.paif_didfuse_stem_bwd(wp, s, sl[2 * s], e, _p(dg), _p(d_d2), _p(d_x), B, H, W, _stream()), "didfuse_stem_bwd")
        grads.append(d_x)
    return grads[0], grads[1]


# ---------------------------------------------------------------------------------------------
# BFFusion baseline (csrc/bffusion.hip, csrc/conv_slab.h; fusion_model/bffusion.py is the module)
# ---------------------------------------------------------------------------------------------
BFF_NB = (16, 32, 64, 96)        # channels of a level's encoder output, attention and fused map
BFF_CIN = (16, 16, 32, 64)       # channels a level's DenseBlock starts from: its slab holds x | conv1 | conv2 = 3 cin
BFF_HEADS = (4, 8, 8, 16)
BFF_DCH = (96, 160, 224, 96)     # decoder slabs: up | f1 | x1_1 | x1_2 | x1_3;  up | f2 | x2_1 | x2_2;  up | f3 | x3_1;  f4
BFF_FOFF = (32, 64, 96, 0)       # where the fused map sits in its level's slab
# The six decoder convs in forward order (DB1_1, DB2_1, DB1_2, DB3_1, DB2_2, DB1_3): (level, level and offset of the map that is upsampled,
# its channels, channels the conv reads = slab[0:K), offset of its output, output channels).  The upsampled map always lands in slab[0:C):
# a conv's input is never needed again (only outputs are taped), so the three convs of level 1 share that slot one after the other.
BFF_DEC = ((0, 1, 64, 32, 48, 48, 16), (1, 2, 96, 64, 96, 96, 32), (0, 1, 96, 32, 64, 64, 16),
           (2, 3, 0, 96, 160, 160, 64), (1, 2, 160, 64, 128, 128, 32), (0, 1, 128, 32, 80, 80, 16))
BFF_DEC_STORE = (32, 64, 32, 160, 128, 80)   # reverse: channels the fold WRITES (the rest it adds to); the first reverse consumer writes all
BFF_DEC_UPADD = (1, 1, 1, 0, 0, 0)           # reverse: the upsample's transpose adds to (1) or writes (0) the source's gradient
_EPI_ACT, _EPI_STORE, _EPI_ADD = 0, 1, 2


def _po(t, off=0):
    """Device pointer of channel `off` of a dense fp32 NHWC map."""
    assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and 0 <= off < t.shape[-1]
    return ctypes.c_void_p(t.data_ptr() + 4 * off)


class _BffConv:
    """One conv's operand packs (forward and transposed), bias, shape and form."""

    __slots__ = ("fwd", "tr", "bias", "M", "K", "taps", "slope", "refl")

    def __init__(self, parts, co, K, taps, bias, slope, refl):
        L = lib()
        dev = parts[0][0].device
        self.M, self.K, self.taps, self.slope, self.refl = co, K, taps, float(slope), refl
        self.fwd = torch.zeros(L.paif_bffusion_ops_floats(co, K, taps), device=dev, dtype=torch.float32)
        self.tr = torch.zeros(L.paif_bffusion_ops_floats(K, co, taps), device=dev, dtype=torch.float32)
        for w, off in parts:
            w = w.detach().to(torch.float32).contiguous()
            assert w.shape[0] == co and w[0, 0].numel() == taps
            _lib.check(L.paif_bffusion_pack_ops(_p(w), co, w.shape[1], off, co, K, taps, 0, _p(self.fwd), _stream()), "bffusion_pack_ops")
            _lib.check(L.paif_bffusion_pack_ops(_p(w), co, w.shape[1], off, K, co, taps, 1, _p(self.tr), _stream()), "bffusion_pack_ops")
        self.bias = None if bias is None else bias.detach().to(torch.float32).contiguous().clone()


class BffusionPack:
    """The packed weights of BFFR: stems and head as they are, every other conv as a _BffConv (BatchNorm folded in), LayerNorm affine."""

    __slots__ = ("stem", "dense", "attn", "dec", "head")


def _bff_fold(w, b, g, be, mu, var, eps):
    """Eval-mode BatchNorm into weight and bias, fp32 on the device."""
    scale = g.detach() * torch.rsqrt(var.detach() + eps)
    return w.detach() * scale[:, None, None, None], be.detach() + (b.detach() - mu.detach()) * scale


def bffusion_pack(spec):
    """spec (BFFR._pack_spec): stem [2][(w, b)], dense [2][4][(w1, b1, w2, b2, wd, bd)], attn [4][2] dicts (convs: four (w, b, gamma, beta,
    mean, var, eps) = conv_pre then ffn; wq, wk, wv, wp, bp, ln_w, ln_b, ln_eps), dec [6][(w, b)] in BFF_DEC order, head (w, b); stream 0
    is the `_vi` modules with attn2, stream 1 the `_ir` modules with attn1 -> BffusionPack."""
    pk = BffusionPack()
    c = lambda t: t.detach().to(torch.float32).contiguous().clone()
    pk.stem = [(c(w).reshape(16), c(b)) for w, b in spec["stem"]]
    pk.head = (c(spec["head"][0]).reshape(16), c(spec["head"][1]))
    pk.dense = []
    for s in range(2):
        row = []
        for l in range(4):
            cin, w1, b1, w2, b2, wd, bd = (BFF_CIN[l],) + tuple(spec["dense"][s][l])
            row.append((_BffConv([(w1, 0)], cin, cin, 9, b1, 0.2, 0), _BffConv([(w2, 0)], cin, 2 * cin, 9, b2, 0.2, 0),
                        _BffConv([(wd, 0)], BFF_NB[l], 3 * cin, 1, bd, 0.1, 0)))
        pk.dense.append(row)
    pk.attn = []
    for l in range(4):
        dim, row = BFF_NB[l], []
        for s in range(2):
            a = spec["attn"][l][s]
            convs = []
            for w, b, g, be, mu, var, eps in a["convs"]:
                wf, bf = _bff_fold(w, b, g, be, mu, var, float(eps))
                convs.append(_BffConv([(wf, 0)], dim, dim, 9, bf, 0.0, 1))
            qkv = torch.cat([a["wq"].detach(), a["wk"].detach(), a["wv"].detach()], 0).reshape(3 * dim, dim, 1, 1)
            row.append(dict(convs=convs, qkv=_BffConv([(qkv, 0)], 3 * dim, dim, 1, None, 1.0, 0),
                            proj=_BffConv([(a["wp"].detach().reshape(dim, dim, 1, 1), 0)], dim, dim, 1, a["bp"], 1.0, 0),
                            ln_w=c(a["ln_w"]), ln_b=c(a["ln_b"]), ln_eps=float(a["ln_eps"]), d=dim // BFF_HEADS[l]))
        pk.attn.append(row)
    pk.dec = []
    for (lvl, _, _, cup, K, _, M), (w, b) in zip(BFF_DEC, spec["dec"]):
        # the reference's concat is (fused, earlier outputs ..., upsampled); the slab holds the upsampled map first
        rest = K - cup
        pk.dec.append(_BffConv([(w.detach()[:, :rest], cup), (w.detach()[:, rest:], 0)], M, K, 9, b, 0.01, 1))
    return pk


def _bff_conv(cv, src, src_off, dst, dst_off, B, H, W):
    """Forward launch of a _BffConv: channels [src_off, + K) of src -> [dst_off, + M) of dst."""
    epi = _EPI_STORE if cv.bias is None else _EPI_ACT
    assert src_off + cv.K <= src.shape[-1] and dst_off + cv.M <= dst.shape[-1] and src.shape[:3] == dst.shape[:3] == (B, H, W)
    _lib.check(lib().paif_bffusion_conv(_p(cv.fwd), _p(cv.bias), cv.slope, epi, cv.taps, cv.refl, _po(src, src_off), None, src.shape[-1], cv.K,
                                        _po(dst, dst_off), dst.shape[-1], cv.M, B, H, W, _stream()), "bffusion_conv")


def _bff_conv_t(cv, taped, d_out, out_off, d_in, in_off, ring, add, n_store, B, H, W):
    """Transposed launch: the cotangent d_out[out_off, + M), masked by the taped output (null: no activation), -> d_in[in_off, + K).
    A reflected conv goes through the ring map and the fold (n_store channels written, the rest added to); a zero-pad one writes or adds."""
    L = lib()
    assert out_off + cv.M <= d_out.shape[-1] and in_off + cv.K <= d_in.shape[-1] and d_out.shape[:3] == d_in.shape[:3] == (B, H, W)
    mask = None if taped is None else _po(taped, out_off)
    assert taped is None or taped.shape == d_out.shape
    if cv.refl:
        assert ring.numel() >= B * (H + 2) * (W + 2) * cv.K
        _lib.check(L.paif_bffusion_conv(_p(cv.tr), None, cv.slope, _EPI_STORE, 9, 2, _po(d_out, out_off), mask, d_out.shape[-1], cv.M, _p(ring), cv.K,
                                        cv.K, B, H, W, _stream()), "bffusion_conv")
        _lib.check(L.paif_bffusion_fold(_p(ring), cv.K, n_store, _po(d_in, in_off), d_in.shape[-1], B, H, W, _stream()), "bffusion_fold")
    else:
        _lib.check(L.paif_bffusion_conv(_p(cv.tr), None, cv.slope, _EPI_ADD if add else _EPI_STORE, cv.taps, 0, _po(d_out, out_off), mask,
                                        d_out.shape[-1], cv.M, _po(d_in, in_off), d_in.shape[-1], cv.K, B, H, W, _stream()), "bffusion_conv")


def bffusion_forward(x0, x1, pack):
    """Two [B,1,H,W] planes (x0 -> the `_vi` modules, x1 -> the `_ir` modules; H, W >= 16) -> (maps, fused [B,1,H,W]).  maps (fp32 NHWC):
    E[s][l] the DenseBlock slabs x | conv1 | conv2; EN[s][l] the encoder outputs; A[l][s] per attention block p1, p2 (conv_pre), qkv, ctx
    [B,dim,d], y (end_proj1), z (LayerNorm), f1, f2 (ffn); D[l] the decoder slabs (BFF_DCH; slot [0:C) holds the LAST upsampled map)."""
    B, _, H, W = x0.shape
    L, dev = lib(), x0.device
    st = _stream
    sizes = [(H >> l, W >> l) for l in range(4)]

    def new(l, c, dtype=torch.float32):
        return torch.empty((B, sizes[l][0], sizes[l][1], c), device=dev, dtype=dtype)

    E = [[new(l, 3 * BFF_CIN[l]) for l in range(4)] for _ in range(2)]
    EN = [[new(l, BFF_NB[l]) for l in range(4)] for _ in range(2)]
    D = [new(l, BFF_DCH[l]) for l in range(4)]
    for s, x in enumerate((x0, x1)):
        keep, p, sb = _plane(x)
        w, b = pack.stem[s]
        _lib.check(L.paif_bffusion_stem_fwd(p, sb, _p(w), _p(b), _p(E[s][0]), 48, B, H, W, st()), "bffusion_stem_fwd")
        for l in range(4):
            h, wd = sizes[l]
            cin, (c1, c2, cd) = BFF_CIN[l], pack.dense[s][l]
            _bff_conv(c1, E[s][l], 0, E[s][l], cin, B, h, wd)
            _bff_conv(c2, E[s][l], 0, E[s][l], 2 * cin, B, h, wd)
            _bff_conv(cd, E[s][l], 0, EN[s][l], 0, B, h, wd)
            if l < 3:
                _lib.check(L.paif_bffusion_pool_fwd(_p(EN[s][l]), BFF_NB[l], BFF_NB[l], _p(E[s][l + 1]), 3 * BFF_CIN[l + 1], B, h, wd, st()),
                           "bffusion_pool_fwd")
    A = []
    for l in range(4):
        h, wd = sizes[l]
        dim, row = BFF_NB[l], []
        chunks = L.paif_bffusion_ctx_chunks(h, wd)
        for s in range(2):
            a = pack.attn[l][s]
            d = a["d"]
            m = dict(p1=new(l, dim), p2=new(l, dim), qkv=new(l, 3 * dim), y=new(l, dim), z=new(l, dim), f1=new(l, dim), f2=new(l, dim),
                     ctx=torch.empty((B, dim, d), device=dev, dtype=torch.float32))
            xa = new(l, dim)
            partial = torch.empty((B, chunks, dim * d), device=dev, dtype=torch.float64)
            _bff_conv(a["convs"][0], EN[s][l], 0, m["p1"], 0, B, h, wd)
            _bff_conv(a["convs"][1], m["p1"], 0, m["p2"], 0, B, h, wd)
            _bff_conv(a["qkv"], m["p2"], 0, m["qkv"], 0, B, h, wd)
            _lib.check(L.paif_bffusion_ctx_partial(_po(m["qkv"], 0), 3 * dim, _po(m["qkv"], dim), 3 * dim, dim, d, _pd(partial), B, h, wd, st()),
                       "bffusion_ctx_partial")
            _lib.check(L.paif_bffusion_ctx_softmax(_pd(partial), dim, d, float(d) ** -0.5, _p(m["ctx"]), B, h, wd, st()), "bffusion_ctx_softmax")
            _lib.check(L.paif_bffusion_attn_apply_fwd(_p(m["qkv"]), _p(m["ctx"]), dim, d, _p(xa), B, h, wd, st()), "bffusion_attn_apply_fwd")
            _bff_conv(a["proj"], xa, 0, m["y"], 0, B, h, wd)
            _lib.check(L.paif_bffusion_ln_fwd(_p(m["y"]), _p(a["ln_w"]), _p(a["ln_b"]), a["ln_eps"], dim, _p(m["z"]), B, h, wd, st()), "bffusion_ln_fwd")
            _bff_conv(a["convs"][2], m["z"], 0, m["f1"], 0, B, h, wd)
            _bff_conv(a["convs"][3], m["f1"], 0, m["f2"], 0, B, h, wd)
            row.append(m)
        # FusionBlock_res: (attn1(en_ir) + attn2(en_vi)) / 2 -- stream 1 is the `_ir` stream
        _lib.check(L.paif_bffusion_gate_fwd(_p(EN[1][l]), dim, _p(row[1]["f2"]), _p(EN[0][l]), dim, _p(row[0]["f2"]), dim, _po(D[l], BFF_FOFF[l]),
                                            BFF_DCH[l], B, h, wd, st()), "bffusion_gate_fwd")
        A.append(row)
    for cv, (lvl, sl, soff, cup, K, ooff, M) in zip(pack.dec, BFF_DEC):
        h, wd = sizes[lvl]
        assert sizes[sl] == (h // 2, wd // 2)
        _lib.check(L.paif_bffusion_up_fwd(_po(D[sl], soff), BFF_DCH[sl], cup, _p(D[lvl]), BFF_DCH[lvl], B, h, wd, st()), "bffusion_up_fwd")
        _bff_conv(cv, D[lvl], 0, D[lvl], ooff, B, h, wd)
    fused = torch.empty((B, 1, H, W), device=dev, dtype=torch.float32)
    _lib.check(L.paif_bffusion_head_fwd(_p(pack.head[0]), _p(pack.head[1]), _po(D[0], 80), 96, _p(fused), B, H, W, st()), "bffusion_head_fwd")
    return dict(E=E, EN=EN, A=A, D=D), fused


def _pd(t):
    """Device pointer of a dense float64 CUDA tensor (the context reduction's partial sums)."""
    if not t.is_cuda or t.dtype != torch.float64 or not t.is_contiguous():
        raise RuntimeError("expected a dense float64 CUDA tensor")
    return ctypes.c_void_p(t.data_ptr())


def bffusion_backward(maps, fused, d_fused, pack):
    """Reverse of bffusion_forward (input gradients) from the taped maps and fused plane -> (d_x0, d_x1) [B,1,H,W].  Nothing is recomputed
    but the LayerNorm statistics; no memset."""
    B, _, H, W = fused.shape
    L, dev = lib(), fused.device
    st = _stream
    d_fused = d_fused.contiguous()
    E, EN, A, D = maps["E"], maps["EN"], maps["A"], maps["D"]
    sizes = [(H >> l, W >> l) for l in range(4)]
    # the ring map of the largest reflected transpose
    ring_n = max([B * (sizes[l][0] + 2) * (sizes[l][1] + 2) * K for (l, _, _, _, K, _, _) in BFF_DEC] +
                 [B * (sizes[l][0] + 2) * (sizes[l][1] + 2) * BFF_NB[l] for l in range(4)])
    ring = torch.empty(ring_n, device=dev, dtype=torch.float32)
    dD = [torch.empty_like(t) for t in D]
    _lib.check(L.paif_bffusion_head_bwd(_p(pack.head[0]), _p(fused), _p(d_fused), _po(dD[0], 80), 96, B, H, W, st()), "bffusion_head_bwd")
    for k in range(5, -1, -1):
        lvl, sl, soff, cup, K, ooff, M = BFF_DEC[k]
        h, wd = sizes[lvl]
        _bff_conv_t(pack.dec[k], D[lvl], dD[lvl], ooff, dD[lvl], 0, ring, False, BFF_DEC_STORE[k], B, h, wd)
        _lib.check(L.paif_bffusion_up_bwd(_p(dD[lvl]), BFF_DCH[lvl], cup, _po(dD[sl], soff), BFF_DCH[sl], BFF_DEC_UPADD[k], B, h, wd, st()),
                   "bffusion_up_bwd")
    grads = []
    for s in range(2):
        dE = [torch.empty_like(t) for t in E[s]]
        for l in range(3, -1, -1):
            h, wd = sizes[l]
            dim, cin, a, m = BFF_NB[l], BFF_CIN[l], pack.attn[l][s], A[l][s]
            d = a["d"]
            dEN = torch.empty_like(EN[s][l])
            da, db, dqkv = torch.empty_like(dEN), torch.empty_like(dEN), torch.empty_like(m["qkv"])
            dS = torch.empty_like(m["ctx"])
            partial = torch.empty((B, L.paif_bffusion_ctx_chunks(h, wd), dim * d), device=dev, dtype=torch.float64)
            # the gate and the mean: d_f2 -> da, d_skip -> dEN (written)
            _lib.check(L.paif_bffusion_gate_bwd(_po(dD[l], BFF_FOFF[l]), BFF_DCH[l], _p(EN[s][l]), dim, _p(m["f2"]), dim, _p(da), _p(dEN), B, h, wd,
                                                st()), "bffusion_gate_bwd")
            _bff_conv_t(a["convs"][3], m["f2"], da, 0, db, 0, ring, False, dim, B, h, wd)      # -> d_f1
            _bff_conv_t(a["convs"][2], m["f1"], db, 0, da, 0, ring, False, dim, B, h, wd)      # -> d_z
            _lib.check(L.paif_bffusion_ln_bwd(_p(m["y"]), _p(a["ln_w"]), a["ln_eps"], dim, _p(da), _p(db), B, h, wd, st()), "bffusion_ln_bwd")
            _bff_conv_t(a["proj"], None, db, 0, da, 0, ring, False, dim, B, h, wd)             # d_y -> d_x (the attention's output)
            _lib.check(L.paif_bffusion_ctx_partial(_po(m["qkv"], 2 * dim), 3 * dim, _p(da), dim, dim, d, _pd(partial), B, h, wd, st()),
                       "bffusion_ctx_partial")
            _lib.check(L.paif_bffusion_ctx_softmax_bwd(_pd(partial), dim, d, float(d) ** -0.5, _p(m["ctx"]), _p(dS), B, h, wd, st()),
                       "bffusion_ctx_softmax_bwd")
            _lib.check(L.paif_bffusion_attn_apply_bwd(_p(m["qkv"]), _p(da), _p(m["ctx"]), _p(dS), dim, d, _p(dqkv), B, h, wd, st()),
                       "bffusion_attn_apply_bwd")
            _bff_conv_t(a["qkv"], None, dqkv, 0, db, 0, ring, False, dim, B, h, wd)            # -> d_p2
            _bff_conv_t(a["convs"][1], m["p2"], db, 0, da, 0, ring, False, dim, B, h, wd)      # -> d_p1
            _bff_conv_t(a["convs"][0], m["p1"], da, 0, dEN, 0, ring, False, 0, B, h, wd)       # adds to d_skip
            if l < 3:
                _lib.check(L.paif_bffusion_pool_bwd(_p(EN[s][l]), dim, dim, _p(dE[l + 1]), 3 * BFF_CIN[l + 1], _p(dEN), dim, B, h, wd, st()),
                           "bffusion_pool_bwd")
            c1, c2, cd = pack.dense[s][l]
            _bff_conv_t(cd, EN[s][l], dEN, 0, dE[l], 0, ring, False, 0, B, h, wd)              # writes all 3 cin
            _bff_conv_t(c2, E[s][l], dE[l], 2 * cin, dE[l], 0, ring, True, 0, B, h, wd)
            _bff_conv_t(c1, E[s][l], dE[l], cin, dE[l], 0, ring, True, 0, B, h, wd)
        d_x = torch.empty_like(fused)
        _lib.check(L.paif_bffusion_stem_bwd(_p(pack.stem[s][0]), _p(dE[0]), 48, _p(d_x), B, H, W, st()), "bffusion_stem_bwd")
        grads.append(d_x)
    return grads[0], grads[1]


# ---------------------------------------------------------------------------------------------
# The hand-designed fusion network: Fusion_Network over two DRDB (csrc/drdb.hip, csrc/conv_slab.h; fusion_model/drdb.py is the module)
# ---------------------------------------------------------------------------------------------
class DrdbPack:
    """The packed weights of Fusion_Network and its one PReLU slope as a Python float."""

    __slots__ = ("weights", "slope")

    def __init__(self, weights, slope):
        self.weights, self.slope = weights, float(slope)


def drdb_pack(convs, slope=0.0):
    """convs: (weight, bias) per conv, by position in paif_amd.synthetic.DRDB_CONVS order (conv1, DRDB1.Dcov1..5, DRDB1.conv, DRDB2.*, conv2,
    conv21); an entry may be None (a DRDB alone packs its own six at positions 1..6 and leaves the rest as zeros).  slope: the PReLU slope
    (a one-element tensor or a float), read to the host HERE, once per pack -> DrdbPack.  A negative slope is refused: the reverse pass
    reads the PReLU branch off the taped output."""
    if len(convs) != 15:
        raise ValueError("drdb_pack: fifteen convs are expected, got %d" % len(convs))
    host = float(slope.detach().reshape(-1)[0]) if torch.is_tensor(slope) else float(slope)
    if not host >= 0.0:
        raise ValueError("Fusion_Network: the PReLU slope is %g; the reverse pass reads the branch off the taped output, which is right for "
                         "slopes >= 0 only" % host)
    dev = next(c for c in convs if c is not None)[0].device
    pack = torch.zeros(lib().paif_drdb_pack_floats(), device=dev, dtype=torch.float32)
    for conv, c in enumerate(convs):
        if c is not None:
            _lib.check(lib().paif_drdb_pack_conv(_p(c[0].detach().contiguous()), _p(c[1].detach().contiguous()), conv, _p(pack), _stream()),
                       "drdb_pack_conv")
    return DrdbPack(pack, host)


def _drdb_block_fwd(wp, block, slab, out, r6, B, H, W):
    L = lib()
    for k in range(1, 6):
        _lib.check(L.paif_drdb_dcov_fwd(wp, block, k, _p(slab), B, H, W, _stream()), "drdb_dcov_fwd")
    _lib.check(L.paif_drdb_tail_fwd(wp, block, _p(slab), _p(out), out.shape[-1], _p(r6), B, H, W, _stream()), "drdb_tail_fwd")


def _drdb_block_bwd(wp, block, slab, r6, d_out, d_slab, B, H, W):
    """d_out: the first 64 channels of a dense [B,H,W,224 | 64] map; d_slab: written whole, [..., 0:64] ends as the gradient of x."""
    L = lib()
    _lib.check(L.paif_drdb_tail_bwd(wp, block, _p(r6), _p(d_out), d_out.shape[-1], _p(d_slab), B, H, W, _stream()), "drdb_tail_bwd")
    for k in range(5, 0, -1):
        _lib.check(L.paif_drdb_dcov_bwd(wp, block, k, _p(slab), _p(d_slab), B, H, W, _stream()), "drdb_dcov_bwd")


def drdb_forward(ir, vis, pack):
    """Two [B,1,H,W] planes (channel 0 of the reference's ir and vis) -> (maps, fused [B,1,H,W]).  maps: slab [B,H,W,224] and r6 [B,H,W,64]
    per DRDB, f2 [B,H,W,64] (DRDB2's output), c2 [B,H,W,32], f [B,1,H,W] (conv21's PReLU output BEFORE the clamp), all fp32, and minmax:
    the 2 floats (min, max of the clamped f over the whole batch).  17 launches."""
    B, _, H, W = ir.shape
    L = lib()
    dev = ir.device
    (_, p_ir, sb_ir), (_, p_vis, sb_vis) = keep = (_plane(ir), _plane(vis))

    def new(c):
        return torch.empty((B, H, W, c), device=dev, dtype=torch.float32)

    wp, sl = _p(pack.weights), pack.slope
    slab, r6, f2, c2 = [new(224), new(224)], [new(64), new(64)], new(64), new(32)
    f = torch.empty((B, 1, H, W), device=dev, dtype=torch.float32)
    _lib.check(L.paif_drdb_stem_fwd(p_ir, sb_ir, p_vis, sb_vis, wp, sl, _p(slab[0]), B, H, W, _stream()), "drdb_stem_fwd")
    _drdb_block_fwd(wp, 0, slab[0], slab[1], r6[0], B, H, W)
    _drdb_block_fwd(wp, 1, slab[1], f2, r6[1], B, H, W)
    _lib.check(L.paif_drdb_conv2_fwd(wp, sl, _p(f2), _p(c2), B, H, W, _stream()), "drdb_conv2_fwd")
    _lib.check(L.paif_drdb_head_fwd(wp, sl, _p(c2), _p(f), B, H, W, _stream()), "drdb_head_fwd")
    fused, mm = plane_clamp_minmax(f)
    del keep
    return dict(slab=slab, r6=r6, f2=f2, c2=c2, f=f, minmax=mm), fused


def drdb_backward(maps, d_fused, pack):
    """Reverse of drdb_forward (input gradients) from the taped maps -> (d_ir, d_vis) [B,1,H,W].  19 launches; nothing is recomputed and
    nothing needs a memset.  The extremum terms of the normalisation follow torch (paif_plane_clamp_minmax_bwd_input): they reach an
    extremal pixel only where the clamp passes."""
    B, _, H, W = maps["f"].shape
    L = lib()
    wp, sl = _p(pack.weights), pack.slope
    d_f = plane_clamp_minmax_bwd(d_fused, maps["f"], maps["minmax"])
    d_c2, d_f2 = torch.empty_like(maps["c2"]), torch.empty_like(maps["f2"])
    d_slab = [torch.empty_like(maps["slab"][0]), torch.empty_like(maps["slab"][1])]
    _lib.check(L.paif_drdb_head_bwd(wp, sl, _p(maps["f"]), _p(d_f), _p(d_c2), B, H, W, _stream()), "drdb_head_bwd")
    _lib.check(L.paif_drdb_conv2_bwd(wp, sl, _p(maps["c2"]), _p(d_c2), _p(d_f2), B, H, W, _stream()), "drdb_conv2_bwd")
    _drdb_block_bwd(wp, 1, maps["slab"][1], maps["r6"][1], d_f2, d_slab[1], B, H, W)
    _drdb_block_bwd(wp, 0, maps["slab"][0], maps["r6"][0], d_slab[1], d_slab[0], B, H, W)
    d_ir, d_vis = torch.empty_like(maps["f"]), torch.empty_like(maps["f"])
    _lib.check(L.paif_drdb_stem_bwd(wp, sl, _p(maps["slab"][0]), _p(d_slab[0]), _p(d_ir), _p(d_vis), B, H, W, _stream()), "drdb_stem_bwd")
    return d_ir, d_vis


def drdb_block_forward(x, pack):
    """One DRDB alone: x [B,64,H,W] fp32 NCHW -> (maps, out [B,64,H,W]).  The block's weights sit at DRDB1's place in the pack.  maps: slab
    [B,H,W,224] and r6 [B,H,W,64].  Six launches between two layout copies."""
    B, C, H, W = x.shape
    if C != 64:
        raise ValueError("DRDB: a [B,64,H,W] map is expected (in_ch = 64, growth_rate = 32 is the built form), got %s" % (tuple(x.shape),))
    slab = torch.empty((B, H, W, 224), device=x.device, dtype=torch.float32)
    slab[..., 0:64].copy_(x.permute(0, 2, 3, 1))
    out, r6 = (torch.empty((B, H, W, 64), device=x.device, dtype=torch.float32) for _ in range(2))
    _drdb_block_fwd(_p(pack.weights), 0, slab, out, r6, B, H, W)
    return dict(slab=slab, r6=r6), out.permute(0, 3, 1, 2).contiguous()


def drdb_block_backward(maps, d_out, pack):
    """Reverse of drdb_block_forward: d_out [B,64,H,W] -> d_x [B,64,H,W]."""
    B, H, W, _ = maps["slab"].shape
    g = d_out.permute(0, 2, 3, 1).contiguous()
    d_slab = torch.empty_like(maps["slab"])
    _drdb_block_bwd(_p(pack.weights), 0, maps["slab"], maps["r6"], g, d_slab, B, H, W)
    return d_slab[..., 0:64].permute(0, 3, 1, 2).contiguous()


# ---------------------------------------------------------------------------------------------
# SKFF and Fusion_Network2 (csrc/skff.hip; operations_m.SKFF and fusion_model/skff.py are the modules)
# ---------------------------------------------------------------------------------------------
class SkffPack:
    """The gate's parameters of one SKFF in the kernels' order, its shape and its PReLU slope as a Python float."""

    __slots__ = ("weights", "height", "d", "slope")

    def __init__(self, weights, height, d, slope):
        self.weights, self.height, self.d, self.slope = weights, int(height), int(d), float(slope)


def skff_pack(du_weight, du_bias, slope, fcs):
    """du_weight [d,64,1,1], du_bias [d] or None: conv_du.0; slope: conv_du.1's PReLU weight (a one-element tensor or a float), read to the
    host HERE, once per pack (any sign: the reverse pass reads the branch off the taped z); fcs: (weight [64,d,1,1], bias [64] or None) per
    input -> SkffPack."""
    n, d = len(fcs), du_weight.shape[0]
    if n not in (2, 3) or du_weight.shape[1] != 64 or not 1 <= d <= 64:
        raise ValueError("skff_pack: 64 channels, 2 or 3 inputs and d <= 64 are built, got %d channels, %d inputs, d = %d" % (du_weight.shape[1], n, d))
    host = float(slope.detach().reshape(-1)[0]) if torch.is_tensor(slope) else float(slope)
    dev = du_weight.device

    def flat(t, count):
        return torch.zeros(count, device=dev, dtype=torch.float32) if t is None else t.detach().to(torch.float32).reshape(-1)

    parts = [flat(du_weight, d * 64), flat(du_bias, d)] + [flat(w, 64 * d) for w, _ in fcs] + [flat(b, 64) for _, b in fcs]
    pack = torch.cat(parts).contiguous()
    assert pack.numel() == lib().paif_skff_pack_floats(n, d)
    return SkffPack(pack, n, d, host)


def _skff_inputs(xs):
    """Channel-last views [B,H,W,>=64] whose first 64 channels are the inputs -> the six (pointer, pixel stride) arguments."""
    args = []
    for x in xs:
        args += [_p(x), x.shape[-1]]
    return args + [None, 0] * (3 - len(xs))


def skff_forward_nhwc(xs, pack, out=None):
    """xs: the inputs as dense channel-last maps (the first 64 channels of each are used); out: the dense map whose channels [0, 64) receive
    V (default: a new [B,H,W,64]) -> (tape, out).  tape: a [B,n,64], z [B,d].  Three launches."""
    B, H, W, _ = xs[0].shape
    dev = xs[0].device
    L = lib()
    if out is None:
        out = torch.empty((B, H, W, 64), device=dev, dtype=torch.float32)
    partial = torch.empty(B * L.paif_skff_blocks(H, W) * 64, device=dev, dtype=torch.float32)
    a = torch.empty((B, pack.height, 64), device=dev, dtype=torch.float32)
    z = torch.empty((B, pack.d), device=dev, dtype=torch.float32)
    _lib.check(L.paif_skff_fwd(*_skff_inputs(xs), pack.height, pack.d, _p(pack.weights), pack.slope, _p(partial), _p(a), _p(z), _p(out),
                               out.shape[-1], 0, B, H, W, _stream()), "skff_fwd")
    return dict(a=a, z=z), out


def skff_backward_nhwc(xs, tape, d_v, pack, want=None):
    """Reverse of skff_forward_nhwc.  d_v: a dense channel-last map whose first 64 channels are dV; want: per input whether its gradient
    is built (default: all) -> the list of d_x_h [B,H,W,64] (None where not wanted).  Three launches."""
    B, H, W, _ = xs[0].shape
    dev = xs[0].device
    L = lib()
    want = [True] * len(xs) if want is None else list(want)
    partial = torch.empty(B * L.paif_skff_blocks(H, W) * 64 * pack.height, device=dev, dtype=torch.float32)
    d_s = torch.empty((B, 64), device=dev, dtype=torch.float32)
    d_xs = [torch.empty((B, H, W, 64), device=dev, dtype=torch.float32) if w else None for w in want]
    _lib.check(L.paif_skff_bwd(*_skff_inputs(xs), pack.height, pack.d, _p(pack.weights), pack.slope, _p(tape["a"]), _p(tape["z"]), _p(d_v),
                               d_v.shape[-1], _p(partial), _p(d_s), *[_p(g) for g in d_xs + [None] * (3 - len(xs))], B, H, W, _stream()),
               "skff_bwd")
    return d_xs


def skff_forward(xs, pack):
    """SKFF alone: n [B,64,H,W] fp32 NCHW maps -> (tape, V [B,64,H,W]).  Three launches between the layout copies."""
    maps = [x.permute(0, 2, 3, 1).contiguous() for x in xs]
    tape, out = skff_forward_nhwc(maps, pack)
    tape["x"] = maps
    return tape, out.permute(0, 3, 1, 2).contiguous()


def skff_backward(tape, d_out, pack, want=None):
    """Reverse of skff_forward: dV [B,64,H,W] -> the list of d_x_h [B,64,H,W] (None where not wanted).  Three launches between the layout
    copies."""
    d_xs = skff_backward_nhwc(tape["x"], tape, d_out.permute(0, 2, 3, 1).contiguous(), pack, want)
    return [None if g is None else g.permute(0, 3, 1, 2).contiguous() for g in d_xs]


def plane_minmax(x):
    """x [B,1,H,W] -> ((x - min x) / (max x - min x) over the whole tensor, NO clamp; the 2 floats (min, max) the reverse pass needs).
    Two launches."""
    x = x.contiguous()
    L = lib()
    n = x.numel()
    partial = torch.empty(2 * L.paif_plane_minmax_nc_blocks(n), device=x.device, dtype=torch.float32)
    out, mm = torch.empty_like(x), torch.empty(2, device=x.device, dtype=torch.float32)
    _lib.check(L.paif_plane_minmax_nc_fwd(_p(x), _p(out), _p(partial), _p(mm), n, _stream()), "plane_minmax")
    return out, mm


def plane_minmax_bwd(dout, x, mm):
    """Reverse of plane_minmax; the gradient of an extremum is spread evenly over the elements that attain it.  Two launches."""
    x = x.contiguous()
    L = lib()
    n = x.numel()
    partial = torch.empty(4 * L.paif_plane_minmax_nc_blocks(n), device=x.device, dtype=torch.float32)
    dx = torch.empty_like(x)
    _lib.check(L.paif_plane_minmax_nc_bwd_input(_p(dout.contiguous()), _p(x), _p(mm), _p(partial), _p(dx), n, _stream()), "plane_minmax_bwd")
    return dx


class Fn2Pack:
    """The packed weights of Fusion_Network2: the DrdbPack of conv1, DRDB1 and DRDB2 (with the one PReLU slope), the pack of conv3, conv4
    and conv2, and the two gates' SkffPack."""

    __slots__ = ("drdb", "weights", "skff", "skff2")

    def __init__(self, drdb, weights, skff, skff2):
        self.drdb, self.weights, self.skff, self.skff2 = drdb, weights, skff, skff2


def fn2_pack(convs, slope, skff, skff2):
    """convs: (weight, bias) of the sixteen Conv2d outside the gates in paif_amd.synthetic.FN2_CONVS order (conv1, DRDB1.*, DRDB2.*, conv2,
    conv3, conv4); slope: relu.weight, read to the host HERE, once per pack, refused when negative (the reverse pass reads the branch off
    the taped output); skff, skff2: the gates' SkffPack -> Fn2Pack."""
    if len(convs) != 16:
        raise ValueError("fn2_pack: sixteen convs are expected, got %d" % len(convs))
    host = float(slope.detach().reshape(-1)[0]) if torch.is_tensor(slope) else float(slope)
    if not host >= 0.0:
        raise ValueError("Fusion_Network2: the PReLU slope is %g; the reverse pass reads the branch off the taped output, which is right for "
                         "slopes >= 0 only" % host)
    drdb = drdb_pack(list(convs[:13]) + [None, None], host)
    pack = torch.zeros(lib().paif_fn2_pack_floats(), device=convs[0][0].device, dtype=torch.float32)
    for conv, k in ((2, 13), (0, 14), (1, 15)):
        w, b = convs[k]
        _lib.check(lib().paif_fn2_pack_conv(_p(w.detach().contiguous()), _p(b.detach().contiguous()), conv, _p(pack), _stream()), "fn2_pack_conv")
    return Fn2Pack(drdb, pack, skff, skff2)


def fn2_forward(ir, vis, out1, out2, pack):
    """Two [B,1,H,W] planes (channel 0 of the reference's ir and vis), out1 [B,64,H,W], out2 [B,128,H,W] -> (maps, fused [B,1,H,W]).  maps:
    slab [B,H,W,224] and r6 [B,H,W,64] per DRDB, f1, c3, f2, c4, v2 [B,H,W,64], the gates' tapes g1, g2 (a, z), f [B,1,H,W] (conv2's PReLU
    output before the normalisation) and minmax, all fp32.  24 launches between the guidance maps' layout copies: conv1 1, DRDB1 6, conv3
    1, skff 3, DRDB2 6, conv4 1, skff2 3, conv2 1, the normalisation 2."""
    B, _, H, W = ir.shape
    L = lib()
    dev = ir.device
    (_, p_ir, sb_ir), (_, p_vis, sb_vis) = keep = (_plane(ir), _plane(vis))
    g1n, g2n = out1.permute(0, 2, 3, 1).contiguous(), out2.permute(0, 2, 3, 1).contiguous()

    def new(c):
        return torch.empty((B, H, W, c), device=dev, dtype=torch.float32)

    wp, sl, fp = _p(pack.drdb.weights), pack.drdb.slope, _p(pack.weights)
    slab, r6 = [new(224), new(224)], [new(64), new(64)]
    f1, c3, f2, c4 = new(64), new(64), new(64), new(64)
    f = torch.empty((B, 1, H, W), device=dev, dtype=torch.float32)
    _lib.check(L.paif_drdb_stem_fwd(p_ir, sb_ir, p_vis, sb_vis, wp, sl, _p(slab[0]), B, H, W, _stream()), "drdb_stem_fwd")
    _drdb_block_fwd(wp, 0, slab[0], f1, r6[0], B, H, W)
    _lib.check(L.paif_fn2_guide_fwd(fp, 0, _p(g1n), _p(c3), B, H, W, _stream()), "fn2_guide_fwd")
    g1, _ = skff_forward_nhwc([f1, c3], pack.skff, out=slab[1])
    _drdb_block_fwd(wp, 1, slab[1], f2, r6[1], B, H, W)
    _lib.check(L.paif_fn2_guide_fwd(fp, 1, _p(g2n), _p(c4), B, H, W, _stream()), "fn2_guide_fwd")
    g2, v2 = skff_forward_nhwc([f2, c4], pack.skff2)
    _lib.check(L.paif_fn2_head_fwd(fp, sl, _p(v2), _p(f), B, H, W, _stream()), "fn2_head_fwd")
    fused, mm = plane_minmax(f)
    del keep
    return dict(slab=slab, r6=r6, f1=f1, c3=c3, f2=f2, c4=c4, v2=v2, g1=g1, g2=g2, f=f, minmax=mm), fused


def fn2_backward(maps, d_fused, pack, want_guides=True):
    """Reverse of fn2_forward (input gradients) from the taped maps -> (d_ir, d_vis [B,1,H,W], d_out1 [B,64,H,W], d_out2 [B,128,H,W]).
    want_guides False: d_out1 and d_out2 are None, the gates skip the gradients of c3 and c4 and the two transposed 1x1 launches are not
    made.  24 launches without the guidance gradients (the normalisation 2, conv2 1, skff2 3, DRDB2 7, skff 3, DRDB1 7, conv1 1), 26 with
    them plus the two layout copies; nothing is recomputed and nothing needs a memset."""
    B, _, H, W = maps["f"].shape
    L = lib()
    wp, sl, fp = _p(pack.drdb.weights), pack.drdb.slope, _p(pack.weights)
    want = [True, bool(want_guides)]
    d_f = plane_minmax_bwd(d_fused, maps["f"], maps["minmax"])
    d_v2 = torch.empty_like(maps["v2"])
    d_slab = [torch.empty_like(maps["slab"][0]), torch.empty_like(maps["slab"][1])]
    _lib.check(L.paif_fn2_head_bwd(fp, sl, _p(maps["f"]), _p(d_f), _p(d_v2), B, H, W, _stream()), "fn2_head_bwd")
    d_f2, d_c4 = skff_backward_nhwc([maps["f2"], maps["c4"]], maps["g2"], d_v2, pack.skff2, want)
    _drdb_block_bwd(wp, 1, maps["slab"][1], maps["r6"][1], d_f2, d_slab[1], B, H, W)
    d_f1, d_c3 = skff_backward_nhwc([maps["f1"], maps["c3"]], maps["g1"], d_slab[1], pack.skff, want)
    _drdb_block_bwd(wp, 0, maps["slab"][0], maps["r6"][0], d_f1, d_slab[0], B, H, W)
    d_ir, d_vis = torch.empty_like(maps["f"]), torch.empty_like(maps["f"])
    _lib.check(L.paif_drdb_stem_bwd(wp, sl, _p(maps["slab"][0]), _p(d_slab[0]), _p(d_ir), _p(d_vis), B, H, W, _stream()), "drdb_stem_bwd")
    d_out1 = d_out2 = None
    if want_guides:
        d1 = torch.empty((B, H, W, 64), device=d_ir.device, dtype=torch.float32)
        d2 = torch.empty((B, H, W, 128), device=d_ir.device, dtype=torch.float32)
        _lib.check(L.paif_fn2_guide_bwd(fp, 0, _p(d_c3), _p(d1), B, H, W, _stream()), "fn2_guide_bwd")
        _lib.check(L.paif_fn2_guide_bwd(fp, 1, _p(d_c4), _p(d2), B, H, W, _stream()), "fn2_guide_bwd")
        d_out1, d_out2 = d1.permute(0, 3, 1, 2).contiguous(), d2.permute(0, 3, 1, 2).contiguous()
    return d_ir, d_vis, d_out1, d_out2
