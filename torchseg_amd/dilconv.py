"""Dilated 3x3 convolutions on our kernels (csrc/dilconv.hip).

`workloads/pspnet.py::_nostride_dilate` turns every 3x3 layer of the ResNet-v1c layer3 / layer4 behind PSPNet and PSANet into
`nn.Conv2d(C_in, C_out, 3, stride=1, padding=d, dilation=d, bias=False)` with d = 2 / 4.  convwrw._route does not take a
dilated layer (every plain 3x3 kernel is padding 1 / dilation 1), so these ran on the vendor library: no BatchNorm
statistics in the forward epilogue, a weight gradient that is not reproducible, no side stream.  `DilatedConv2d` runs
  - the forward on tsg_conv3x3_dil_fwd (in training mode with the statistics partial of the output attached for the
    SyncBatchNorm behind the layer),
  - the data gradient on the same kernel with the rotated / transposed (mode 1) filter,
  - the weight gradient on tsg_conv3x3_dil_wrw (fp32, fixed-order fp64 fold: bit-identical from run to run) through
    convwrw.wrw_on_side_stream, i.e. under the side-stream, capture and deferred-launch rules of the other 3x3 layers.
The fragment-order filters of a channels_last parameter come from the shadow bank (one refresh per optimizer step);
any other weight is cast per call.

The DDP wrapper and prepare_inference re-class matching modules in place (same parameter, same state-dict key) under
TSG_CONV_DIL=1 (default 0: see DESIGN.md 4.4 for the measurements and for what keeps it opt-in).  Any other call — a CPU input, an
input that is not channels_last, fp32 outside autocast (the parity mode, where exactconv takes the layer), a shape the
kernels do not take — runs the stock `nn.Conv2d.forward`.
"""
import torch
import torch.nn as nn

from . import kernels as K
from .convwrw import _bf16_nhwc, _with_partial, wrw_on_side_stream
from .stemconv import _wants_bf16


class _DilConvFn(torch.autograd.Function):
    """Second output: the statistics partial of y (or an empty tensor)."""

    @staticmethod
    def forward(ctx, x, weight, dilation, with_stats):
        kp = K.provider()
        out = kp.conv3x3_dil_fwd(x, kp.conv3x3_dil_prep_filter(weight, 0, x), weight.shape[0], dilation, with_stats=with_stats)
        y, partial = out if with_stats else (out, x.new_empty(0, dtype=torch.float32))
        ctx.dilation = dilation
        ctx.save_for_backward(x, weight)
        ctx.mark_non_differentiable(partial)
        ctx.set_materialize_grads(False)
        return y, partial

    @staticmethod
    def backward(ctx, dy, _dpartial):
        x, weight = ctx.saved_tensors
        if dy is None:
            return None, None, None, None
        kp = K.provider()
        d = ctx.dilation
        dy = _bf16_nhwc(dy)
        dx = kp.conv3x3_dil_dgrad(dy, weight, d) if ctx.needs_input_grad[0] else None
        dw = None
        if ctx.needs_input_grad[1]:
            dw = wrw_on_side_stream(lambda out=None: K.provider().conv3x3_dil_wrw(x, dy, d, out=out), weight, x, dy,
                                    defer_out=(dy.shape[1], x.shape[1])).to(weight.dtype)
        return dx, dw, None, None


class DilatedConv2d(nn.Conv2d):
    """nn.Conv2d(C_in, C_out, 3, 1, d, d, bias=False) whose bf16 channels_last HIP calls run on tsg_conv3x3_dil_*."""

    def takes(self, x):
        """x as the kernels read it (bf16; x itself when it already is) when this call is ours, else None"""
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 4 and _wants_bf16(x)
                and self.weight.dtype == torch.float32 and self.bias is None and self.padding_mode == "zeros"
                and self.stride[0] == self.stride[1] and self.padding[0] == self.padding[1]
                and self.dilation[0] == self.dilation[1] and x.shape[1] == self.in_channels
                and x.is_contiguous(memory_format=torch.channels_last)):
            return None
        xb = _bf16_nhwc(x)
        if not K.provider().conv3x3_dil_supported(xb, self.weight, self.stride[0], self.padding[0], self.dilation[0], self.groups):
            return None
        return xb

    def forward(self, x):
        xb = self.takes(x)
        if xb is None:
            return super().forward(x)
        with torch.autocast("cuda", enabled=False):
            y, partial = _DilConvFn.apply(xb, self.weight, self.dilation[0], bool(self.training and torch.is_grad_enabled()))
        return _with_partial(y, partial)


def _eligible(m):
    return (type(m) is nn.Conv2d and m.kernel_size == (3, 3) and m.stride == (1, 1) and m.dilation in ((2, 2), (4, 4))
            and m.padding == m.dilation and m.groups == 1 and m.bias is None and m.padding_mode == "zeros"
            and m.in_channels % 16 == 0 and m.out_channels % 64 == 0
            and not m._forward_hooks and not m._forward_pre_hooks and not m._backward_hooks)


def install_dilated_conv(module):
    """Re-class, in place, the dilated 3x3 convolutions of `module` to DilatedConv2d; returns how many."""
    n = 0
    for m in module.modules():
        if _eligible(m):
            m.__class__ = DilatedConv2d
            n += 1
    return n
