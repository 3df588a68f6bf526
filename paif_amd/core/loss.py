"""Fusion loss of the training API -- counterpart of the reference's core/loss.py:490-502 and pytorch_ssim/__init__.py:
`Fusionloss_grad2` = L1(mask, fused) + 1.1 * (1 - SSIM_11x11(fused, mask)).  Both entry scripts import and instantiate it
(test_original.py:10, robust_test.py:261) but never call it.

Built: the forward value and the gradient w.r.t. the generated image (HIP kernels paif_ssim_l1_fwd / _bwd_input), so the loss
can sit on top of the models' input-gradient autograd nodes.  Not built: parameter gradients -- the training step (BASELINE
config 5: wgrad kernels, AdamW kernels, RCCL gradient all-reduce) is outside round 1.  A `mask` that requires grad raises.

The Sobel criteria of core/loss.py:423-474, 516-571, 595-603 -- `Fusionloss` (max intensity + max Sobel gradient), `Fusionloss2/3/4/6`,
`Fusionloss_add`, `Total_fusion_loss3` -- and the `Sobelxy` operator (:634-650) run on csrc/sobel_loss.hip: one launch (plus a one-block
finish) reads each plane once and gives the value as a 0-d device tensor, one launch gives d/d(generated image); channel 0 of `ir`, `vis`
and `mask` is read in place.  `Fusionloss_grad3` (:504-515) is MSE + 1.1 * (1 - SSIM) on the existing kernels.  Every criterion is
differentiable w.r.t. the generated image only: `ir`, `vis` or `mask` requiring grad under recording autograd raises NotImplementedError.
A class that reads its image arguments says so with `reads_images = True`; the composite models then refuse `ir` / `vis` that require
grad in their `_loss*` methods instead of dropping the criterion's direct image term.  Not built: `new_loss_sobel`,
`Total_fusion_loss`, `Total_fusion_loss2`, `IQALoss` / `Entropy`, `Fusionloss_grad`, and the FCOS criteria.

The segmentation criteria of core/loss.py:342-383 -- `OhemCELoss`, `SoftmaxFocalLoss`, `NormalLoss` -- run on csrc/seg_criteria.hip
(ops.seg_criterion): `forward(logits, labels)` is the reference's call on full-resolution logits, `from_seg_map(seg_map, labels)` takes
the head's low-resolution map and folds F.interpolate(bilinear, align_corners=False) into the same kernels, which is the route the
composite models take (`takes_seg_map = True`).  Value and gradient stay on the device: OHEM's n_min-th largest loss comes from an exact
radix select, not from a sort.  Limits: C <= 32 classes (above that `forward` and the composite models compute the criterion with torch
ops, `from_seg_map` and ops.seg_criterion raise NotImplementedError); gradients w.r.t. the logits only; no class weights or label
smoothing.  A label outside [0, C) that is not `ignore_lb` is dropped like an ignored pixel (torch raises).
Differences from torch, both in the gradient only: OHEM pixels that tie at the n_min-th largest loss share the remaining weight equally
(torch's sort hands it to an unspecified subset of them; the value is the same, and ties at 0 -- ignored pixels -- carry no gradient
either way); the focal gradient is 0 where 1 - p is exactly 0 (torch gives NaN there for 0 < gamma < 1).  `OhemCELoss` refuses `n_min`
outside [1, number of pixels] with a ValueError at the call (the reference raises IndexError above and is silently wrong at 0)."""
import torch
import torch.nn as nn

from .. import ops


class _SsimL1Fn(torch.autograd.Function):
    """w_l1 * mean|y - x| + w_ss * (1 - mean SSIM(x, y)), differentiable w.r.t. x only."""

    @staticmethod
    def forward(ctx, x, y, w_l1, w_ss):
        xd, yd = x.detach(), y.detach()
        s, l1 = ops.ssim_l1(xd, yd)
        ctx.save_for_backward(xd, yd)
        ctx.w = (w_l1, w_ss)
        return w_l1 * l1 + w_ss * (1 - s)

    @staticmethod
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        n = float(x.numel())
        dx = ops.ssim_l1_bwd(x, y, g * (ctx.w[0] / n), g * (ctx.w[1] / n))
        return dx, None, None, None


def _ssim_l1(x, y, w_l1, w_ss):
    if torch.is_grad_enabled() and y.requires_grad:
        raise NotImplementedError("ssim / Fusionloss_grad2: the gradient w.r.t. the second image (mask) is not built")
    if torch.is_grad_enabled() and x.requires_grad:
        return _SsimL1Fn.apply(x, y, w_l1, w_ss)
    with torch.no_grad():
        s, l1 = ops.ssim_l1(x, y)
        return w_l1 * l1 + w_ss * (1 - s)


def ssim(img1, img2, window_size=11, size_average=True):
    """pytorch_ssim.ssim for single-channel images (the only use on the path), mean over the batch."""
    if window_size != 11 or not size_average or img1.shape[1] != 1:
        raise NotImplementedError("ssim: built for window_size=11, size_average=True, 1 channel (core/loss.py:501)")
    return 1 - _ssim_l1(img1, img2, 0.0, 1.0)


class Fusionloss_grad2(nn.Module):
    def __init__(self):
        super().__init__()

    def forward(self, image_ir, image_vis, generate_img, mask):
        return _ssim_l1(generate_img, mask[:, :1, :, :], 1.0, 1.1)


class Fusionloss_grad3(nn.Module):
    """core/loss.py:504-515: MSE(mask, gen) + 1.1 * (1 - ssim(gen, mask)) on the MSE (ops.image_loss) and SSIM kernels.  The reference's
    constructor also builds a LapLoss2 it never calls; that third-party module is absent here and nothing is constructed."""

    def __init__(self):
        super().__init__()

    def forward(self, image_ir, image_vis, generate_img, mask):
        mask = mask[:, :1, :, :]
        if torch.is_grad_enabled() and mask.requires_grad:
            raise NotImplementedError("Fusionloss_grad3: the gradient w.r.t. the mask is not built")
        _check_gen(generate_img, mask, "mask")
        return ops.image_loss(generate_img, mask, "l_2") + _ssim_l1(generate_img, mask, 0.0, 1.1)


def _check_gen(gen, other, name):
    if gen.dtype != torch.float32 or other.dtype != torch.float32:
        raise TypeError("expected float32, got %s (generated image) and %s (%s)" % (gen.dtype, other.dtype, name))
    if gen.dim() != 4 or gen.shape[1] != 1 or tuple(other.shape) != tuple(gen.shape):
        raise ValueError("expected the generated image and %s as one shape [B,1,H,W], got %s and %s" % (name, tuple(gen.shape), tuple(other.shape)))
    if not (gen.is_cuda and other.is_cuda):
        raise RuntimeError("paif_amd ops need CUDA(HIP) tensors; got %s (generated image) and %s (%s) -- there is no CPU path"
                           % (gen.device, other.device, name))


class Sobelxy(nn.Module):
    """core/loss.py:634-650: |Gx * x| + |Gy * x| of a 1-channel map, zero padding 1 (ops.sobelxy: value and input gradient).  weightx /
    weighty keep the reference's surface and are not read by the kernels; they are plain tensors, so state_dict() is empty -- as in
    the reference on a GPU, where `.cuda()` on the Parameter leaves a tensor that the module does not register."""

    def __init__(self):
        super().__init__()
        self.weightx = torch.tensor([[-1., 0., 1.], [-2., 0., 2.], [-1., 0., 1.]]).unsqueeze(0).unsqueeze(0)
        self.weighty = torch.tensor([[1., 2., 1.], [0., 0., 0.], [-1., -2., -1.]]).unsqueeze(0).unsqueeze(0)

    def forward(self, x):
        return ops.sobelxy(x)


class _SobelCriterion(nn.Module):
    """One launch for the value, one for d/d(generated image): the term table of ops.sobel_loss.  `self.sobelconv` as in the reference."""

    def __init__(self):
        super().__init__()
        self.sobelconv = Sobelxy()


_MAX, _MASK, _LIN = ops.SOBEL_MAX, ops.SOBEL_MASK, ops.SOBEL_LIN


class Fusionloss(_SobelCriterion):
    """core/loss.py:423-440 (SeAFusion's loss): L1(max(y, ir), gen) + 8 * L1(max(S y, S ir), S gen)."""

    reads_images = True   # the composite models must not detach ir / vis in front of this criterion: see _CompositeBase._refuse_image_grads
    criterion_args = ("ir", "vis", "gen")   # no mask: the composite models call the criterion by this order (_CompositeBase._call_criterion)

    def forward(self, image_ir, image_vis, generate_img):
        return ops.sobel_criterion(generate_img, image_ir, image_vis, None, [(_MAX, 1.0, 0.0, 0.0)], (_MAX, 8.0, 0.0, 0.0))


class Fusionloss2(_SobelCriterion):
    """core/loss.py:441-457: L1(mask, gen)."""

    def forward(self, image_ir, image_vis, generate_img, mask):
        return ops.sobel_criterion(generate_img, None, None, mask, [(_MASK, 1.0, 0.0, 0.0)], None)


class Fusionloss3(_SobelCriterion):
    """core/loss.py:459-474: L1(mask, gen) + L1(S mask, S gen)."""

    def forward(self, image_ir, image_vis, generate_img, mask):
        return ops.sobel_criterion(generate_img, None, None, mask, [(_MASK, 1.0, 0.0, 0.0)], (_MASK, 1.0, 0.0, 0.0))


class Fusionloss6(_SobelCriterion):
    """core/loss.py:516-535: 0.5 * L1(mask, gen) + 0.5 * L1(y + ir, gen) + 6 * L1(max(S y, S ir), S gen)."""

    reads_images = True

    def forward(self, image_ir, image_vis, generate_img, mask):
        return ops.sobel_criterion(generate_img, image_ir, image_vis, mask, [(_MASK, 0.5, 0.0, 0.0), (_LIN, 0.5, 1.0, 1.0)],
                                   (_MAX, 6.0, 0.0, 0.0))


class Fusionloss4(_SobelCriterion):
    """core/loss.py:537-552: syn = (y + ir) / 2; L1(syn, gen) + 4 * L1(S syn, S gen).  The mask is not read."""

    reads_images = True

    def forward(self, image_ir, image_vis, generate_img, mask):
        return ops.sobel_criterion(generate_img, image_ir, image_vis, None, [(_LIN, 1.0, 0.5, 0.5)], (_LIN, 4.0, 0.5, 0.5))


class Fusionloss_add(_SobelCriterion):
    """core/loss.py:554-571: 1.5 * L1(0.4 * y + 0.6 * ir, gen) + 5 * L1(max(S y, S ir), S gen)."""

    reads_images = True
    criterion_args = ("ir", "vis", "gen")

    def forward(self, image_ir, image_vis, generate_img):
        return ops.sobel_criterion(generate_img, image_ir, image_vis, None, [(_LIN, 1.5, 0.6, 0.4)], (_MAX, 5.0, 0.0, 0.0))


class Total_fusion_loss3(nn.Module):
    """core/loss.py:595-603: 3 * Fusionloss(ir, vis, gen).  Note the argument order: the mask comes third and is not read."""

    reads_images = True
    criterion_args = ("ir", "vis", "mask", "gen")

    def __init__(self):
        super().__init__()
        self.fl = Fusionloss()

    def forward(self, image_ir, image_vis, mask, generate_img):
        return ops.sobel_criterion(generate_img, image_ir, image_vis, None, [(_MAX, 3.0, 0.0, 0.0)], (_MAX, 24.0, 0.0, 0.0))


class _SegCriterion(nn.Module):
    """One fused route for the three segmentation criteria: `from_seg_map` upsamples inside the kernels, `forward` is the identity-scale
    case of the same kernels.  `takes_seg_map` is what `_CompositeBase._seg_term` recognises.  No parameters, no buffers."""

    takes_seg_map = True
    seg_kind = None

    def _seg_params(self):
        return {}

    def from_seg_map(self, seg_map, labels):
        """criterion(F.interpolate(seg_map, size=labels.shape[1:], mode='bilinear', align_corners=False), labels), seg_map [B,C,h,w]."""
        return ops.seg_criterion(seg_map, labels.type(torch.long), self.seg_kind, ignore_index=self.ignore_lb, **self._seg_params())

    def forward(self, logits, labels):
        if logits.dim() != 4 or labels.dim() != 3 or tuple(logits.shape[2:]) != tuple(labels.shape[1:]):
            raise ValueError("expected logits [B,C,H,W] and labels [B,H,W] of one size, got %s and %s (from_seg_map takes a low-resolution "
                             "map)" % (tuple(logits.shape), tuple(labels.shape)))
        if logits.shape[1] > ops.SEG_MAXC:
            # more classes than the kernels take: the torch route, where the composite models send such a criterion (`_seg_term`)
            return self._torch_forward(logits, labels.type(torch.long))
        return self.from_seg_map(logits, labels)

    def _pixel_ce(self, logits, labels):
        return nn.functional.cross_entropy(logits, labels, ignore_index=self.ignore_lb, reduction="none")


class OhemCELoss(_SegCriterion):
    """core/loss.py:342-358: with l the per-pixel cross entropy sorted in descending order, the mean of {l > T} if l[n_min - 1] > T, else
    the mean of the n_min largest; T = -log(thresh) in float32.  `thresh` holds T as a plain float (the reference keeps a 0-d tensor)."""

    seg_kind = "ohem"

    def __init__(self, thresh, n_min, ignore_lb=255, *args, **kwargs):
        super().__init__()
        if not 0.0 < thresh <= 1.0:
            raise ValueError("OhemCELoss: thresh must lie in (0, 1], got %r" % (thresh,))
        self.thresh = float(-torch.log(torch.tensor(thresh, dtype=torch.float)))
        self.n_min = n_min
        self.ignore_lb = ignore_lb

    @property
    def T(self):
        return self.thresh

    def _seg_params(self):
        return dict(T=self.thresh, n_min=self.n_min)

    def _torch_forward(self, logits, labels):
        l = self._pixel_ce(logits, labels).flatten()
        if not 1 <= self.n_min <= l.numel():
            raise ValueError("OhemCELoss: n_min = %r outside [1, %d] (the number of pixels)" % (self.n_min, l.numel()))
        above = l > self.thresh
        return l[above].mean() if int(above.sum()) >= self.n_min else torch.topk(l, self.n_min).values.mean()


class SoftmaxFocalLoss(_SegCriterion):
    """core/loss.py:361-373: NLLLoss(ignore_index)((1 - softmax)^gamma * log_softmax, labels), the mean over the valid pixels."""

    seg_kind = "focal"

    def __init__(self, gamma, ignore_lb=255, *args, **kwargs):
        super().__init__()
        if not gamma >= 0:
            raise ValueError("SoftmaxFocalLoss: built for gamma >= 0, got %r" % (gamma,))
        self.gamma = gamma
        self.ignore_lb = ignore_lb

    def _seg_params(self):
        return dict(gamma=float(self.gamma))

    def _torch_forward(self, logits, labels):
        logp = torch.log_softmax(logits, dim=1)
        return nn.functional.nll_loss(torch.pow(1.0 - torch.exp(logp), self.gamma) * logp, labels, ignore_index=self.ignore_lb)


class NormalLoss(_SegCriterion):
    """core/loss.py:375-383: the mean of CrossEntropyLoss(ignore_index, reduction='none') over ALL pixels, the ignored ones included."""

    seg_kind = "normal"

    def __init__(self, ignore_lb=255, *args, **kwargs):
        super().__init__()
        self.ignore_lb = ignore_lb

    def _torch_forward(self, logits, labels):
        return self._pixel_ce(logits, labels).mean()
