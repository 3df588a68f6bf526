"""What the native two-plane fusion networks share: the checks of their planes, the `forward` gate, the protocol of the fusion network
inside the composite models, and one autograd node.

THE PROTOCOL (core/model_fusion_auto.py: _CompositeBase).  `forward_impl(ir, vis, inter=None, tape=None)` takes channel 0 of `ir` and of
`vis` and returns the fused plane [B,1,H,W]; with a `tape` (a dict) it keeps what `backward_impl(d_fused, tape, wgrad=False)` needs, which
returns the two input gradients as [B,1,H,W] each.  So `Network_MM_CompModel(<network>, ...)` runs through `attack_both` and the
robustness harness like the searched network.

NOT BUILT (raises, never a fall-back): parameter gradients (training the network) -- in `forward` when a parameter requires grad outside
ops.no_param_grads() / torch.no_grad(), in `forward_impl` under a weight-gradient tape, in `backward_impl(wgrad=True)`; the searched
network's `inter`; a CPU path.

SETTINGS THAT DO NOT APPLY.  The maps stay fp32 under ops.set_storage("bf16" | "f16"), and the conv_precision / gemm_precision settings
and ops.CONFIG["two_stream"] change nothing: there is one arithmetic (exact fp32).

A network derives from NativeFusion, sets NAME and keeps its module tree, `_pack`, `_run(a, b, tape)`, `_reverse(d_fused, tape)` and
`_map_list`; its `forward` carries the reference's argument names and calls `_gate`.  The base registers no parameter, buffer or
submodule: every state_dict is the network's own."""
import torch
import torch.nn as nn

from .. import ops
from ..operations_m import grad_anchor


def need_device(t):
    if not t.is_cuda:
        raise RuntimeError("paif_amd ops need CUDA(HIP) tensors; got a %s tensor -- there is no CPU path" % t.device)


class NativeFusion(nn.Module):
    """Base of ReCoNet, SDNet, U2Fusion, SeaFusion, DID, BFFR and Fusion_Network."""

    NAME = None                             # the network's name in every message
    TRAINING = "training the baseline"      # what parameter gradients would be for
    SHAPE_NOTE = ""                         # appended to "... planes of one shape are expected"
    TAPED = ("maps",)                       # the tape entries _map_list takes, in its argument order

    # ---- checks ----------------------------------------------------------------------------------------------------------
    @classmethod
    def _check_planes(cls, a, b):
        """Device, then dtype, then [B,1,H,W] of one shape.  A network with a minimum size checks it after this."""
        for t in (a, b):
            need_device(t)
            if t.dtype != torch.float32:
                raise TypeError("%s: fp32 planes are expected, got %s" % (cls.NAME, t.dtype))
        if a.dim() != 4 or a.shape[1] != 1 or a.shape != b.shape:
            raise ValueError("%s: two [B,1,H,W] planes of one shape are expected%s, got %s and %s"
                             % (cls.NAME, cls.SHAPE_NOTE, tuple(a.shape), tuple(b.shape)))

    def _check_mode(self):
        """Nothing by default; a network whose BatchNorm is folded from the running statistics refuses .train() here."""

    @classmethod
    def _no_wgrad(cls):
        return "%s: parameter gradients (%s) are not built" % (cls.NAME, cls.TRAINING)

    @classmethod
    def _no_wgrad_true(cls):
        return cls._no_wgrad() + " (wgrad=True)"

    # ---- the gate of `forward` -------------------------------------------------------------------------------------------
    def _wants_node(self, a, b):
        """The checks of `forward` in their order; -> whether an autograd node is to record the call."""
        self._check_mode()
        if ops.want_param_grads(self):
            raise NotImplementedError(self._no_wgrad() + " -- freeze the parameters (requires_grad_(False)), or run under "
                                      "ops.no_param_grads() / torch.no_grad() for input gradients")
        self._check_planes(a, b)
        return torch.is_grad_enabled() and (a.requires_grad or b.requires_grad)

    def _gate(self, a, b, *extra):
        """-> the fused plane, with the autograd node where an input asks for a gradient.  `extra` goes to _run before the tape."""
        if self._wants_node(a, b):
            return _NativeFn.apply(a, b, self, *extra, grad_anchor(a.device))
        with torch.no_grad():
            return self._run(a, b, *extra, None)

    def _features(self, a, b):
        """The taped maps (_map_list) as NCHW tensors -- for the tests."""
        self._check_mode()
        self._check_planes(a, b)
        tape = {}
        with torch.no_grad():
            self._run(a, b, tape)
        return [m.permute(0, 3, 1, 2).contiguous() for m in self._map_list(*(tape[k] for k in self.TAPED))]

    # ---- the composite models' protocol ----------------------------------------------------------------------------------
    def _impl_planes(self, ir, vis, inter, tape):
        """The refusals of forward_impl, then channel 0 of each, checked."""
        if inter is not None:
            raise NotImplementedError("%s: `inter` (the searched network's decomposition intermediates) does not apply" % self.NAME)
        if tape is not None and ops.taping_wgrad():
            raise NotImplementedError(self._no_wgrad())
        self._check_mode()
        a, b = ir[:, 0:1, :, :], vis[:, 0:1, :, :]
        self._check_planes(a, b)
        return a, b

    def forward_impl(self, ir, vis, inter=None, tape=None):
        """ir, vis: [B,>=1,H,W], channel 0 is used -> fused [B,1,H,W]; tape (dict): filled for backward_impl."""
        a, b = self._impl_planes(ir, vis, inter, tape)
        return self._run(a, b, tape)

    def backward_impl(self, d_fused, tape, wgrad=False):
        """d/d(fused) [B,1,H,W] -> the gradients of forward_impl's two planes as [B,1,H,W] each."""
        if wgrad:
            raise NotImplementedError(self._no_wgrad_true())
        return self._reverse(d_fused, tape)


class _NativeFn(torch.autograd.Function):
    """Autograd node of a NativeFusion network: hand-written reverse pass, input gradients only."""

    @staticmethod
    def forward(ctx, a, b, module, *rest):
        """rest: what _run takes between the planes and the tape, then the gradient anchor."""
        tape = {}
        out = module._run(a.detach(), b.detach(), *rest[:-1], tape)
        ctx.tape, ctx.module, ctx.nones = tape, module, (None,) * (1 + len(rest))
        return out

    @staticmethod
    def backward(ctx, d_out):
        d_a, d_b = ctx.module.backward_impl(d_out.contiguous(), ctx.tape)
        ctx.tape = None
        return (d_a, d_b) + ctx.nones
