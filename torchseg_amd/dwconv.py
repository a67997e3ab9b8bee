"""Depthwise 3x3 convolutions on our kernels (csrc/dwconv.hip).

Xception39 (furnace/base_model/xception.py, the context path of BiSeNet-X39) is built from 51
`nn.Conv2d(C, C, 3, stride, 1, groups=C, bias=False)` layers.  None of the other kernels of this package takes a grouped
layer, and the vendor library would give these a weight gradient that is not reproducible and, in the fp32 parity mode, a
forward 5-6e-5 from float64.  `DepthwiseConv2d` runs forward, data gradient and weight gradient on `tsg_dwconv3x3_*`:
  - bf16 under autocast: bf16 activations, the fp32 filter read as is, fp32 accumulation, one rounding;
  - fp32 outside autocast (the parity mode): exact products, fp64 accumulation, one rounding;
  - the weight gradient is fp32, folded from per-block partials in a fixed order: bit-identical from run to run.
No atomics, no side streams, no deferred launches, no host synchronisation (the workspace comes from the caching
allocator), so the layer can be captured in a graph.

The DDP wrapper re-classes matching modules in place (same parameter, same state-dict key).  Any other call — an NCHW or
CPU input, fp32 under autocast, a shape the kernels do not take — runs the stock `nn.Conv2d.forward`.  TSG_DW_CONV=1|0
(default 1) switches the swap.
"""
import os

import torch
import torch.nn as nn

from . import kernels as K

ENABLED = os.environ.get("TSG_DW_CONV", "1") != "0"


class _DwConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, stride):
        ctx.stride = stride
        ctx.save_for_backward(x, weight)
        return K.provider().dwconv3x3_fwd(x, weight, stride)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        kp = K.provider()
        if dy.dtype != x.dtype:
            dy = dy.to(x.dtype)
        dy = dy.contiguous(memory_format=torch.channels_last)
        dx = kp.dwconv3x3_dgrad(dy, weight, x, ctx.stride) if ctx.needs_input_grad[0] else None
        dw = kp.dwconv3x3_wgrad(x, dy, weight, ctx.stride) if ctx.needs_input_grad[1] else None
        return dx, dw, None


def _mode_ok(x):
    """bf16 under bf16 autocast, or fp32 outside autocast"""
    if torch.is_autocast_enabled():
        return x.dtype == torch.bfloat16 and torch.get_autocast_dtype("cuda") == torch.bfloat16
    return x.dtype == torch.float32


class DepthwiseConv2d(nn.Conv2d):
    """nn.Conv2d(C, C, 3, stride, 1, groups=C, bias=False) whose channels_last HIP calls run on tsg_dwconv3x3_*."""

    def takes(self, x):
        return (isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 4 and _mode_ok(x)
                and self.weight.dtype == torch.float32 and self.bias is None and self.padding_mode == "zeros"
                and x.is_contiguous(memory_format=torch.channels_last)
                and K.provider().dwconv3x3_supported(x, self.weight, self.stride[0], self.padding[0], self.dilation[0],
                                                     self.groups))

    def forward(self, x):
        if self.takes(x):
            return _DwConvFn.apply(x, self.weight, self.stride[0])
        return super().forward(x)


def _eligible(m):
    if type(m) is not nn.Conv2d:
        return False
    c = m.in_channels
    return (m.groups == c and m.out_channels == c and m.kernel_size == (3, 3)
            and m.padding == (1, 1) and m.dilation == (1, 1) and m.stride in ((1, 1), (2, 2)) and m.bias is None
            and m.padding_mode == "zeros" and not m._forward_hooks and not m._forward_pre_hooks
            and not m._backward_hooks)


def install_depthwise_conv(module):
    """Re-class, in place, the depthwise 3x3 convolutions of `module` to DepthwiseConv2d; returns how many."""
    n = 0
    for m in module.modules():
        if _eligible(m):
            m.__class__ = DepthwiseConv2d
            n += 1
    return n
