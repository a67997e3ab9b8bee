"""Xception's separable unit as one launch at inference (csrc/sepconv.hip).

`SeparableConvBnRelu` of furnace/base_model/xception.py is a depthwise 3x3 convolution straight into a point-wise
ConvBnRelu, with no BatchNorm in between.  In eval mode the BatchNorm is an affine map of the running statistics, so the
unit is `relu?(a * (W_p . dw3x3(x, W_d)) + b (+ shortcut))`, and `tsg_sepconv_fwd` computes it without the depthwise
result ever reaching memory: one launch instead of tsg_dwconv3x3_fwd + the vendor 1x1 convolution + tsg_bn_apply_fwd.

`install_fused_separable(module)` re-classes, in place, every module that has the unit's STRUCTURE (not its class: the
reference's own network.py built on our furnace is covered as well):
  - `conv1`: a depthwise 3x3 convolution that torchseg_amd.dwconv takes (or already a DepthwiseConv2d);
  - `point_wise_cbr`: `.conv` a 1x1, stride-1, bias-free convolution, `.bn` a BatchNorm, optionally `.relu`.
Parameters, buffers and state-dict keys stay what they were.  The re-classed unit takes the fused kernel only when all of
this holds: the unit and its BatchNorm are in eval mode, gradients are disabled, the input is a channels_last HIP tensor
in the mode torchseg_amd.dwconv accepts (bf16 under bf16 autocast, fp32 outside autocast), `tsg_sepconv_supported` takes
the shape, and a residual has the output's shape, dtype and layout.  Every other call — training, gradients enabled, a
CPU or NCHW input — runs the stock method it replaced, bit for bit.

The constants (both filters and the BatchNorm's a, b in the order the kernel reads them) are packed on the device once
per unit, device and dtype, and again when the `_version` (or storage) of conv1.weight, point_wise_cbr.conv.weight, the
BatchNorm's weight, bias, running_mean or running_var has changed: `load_state_dict` and in-place writes show in the
next call.  A pack is never built during a graph capture (a stale unit runs its stock path there); the warm-up call of
InferenceModule.forward builds it.

TSG_SEPCONV_FUSED=0|1 (default 0) is read by torchseg_amd.infer.prepare_inference(fuse_separable=None); the DDP wrapper
and ddp.install_kernels never install this.
"""
import torch
import torch.nn as nn
from torch.nn.modules.batchnorm import _BatchNorm

from . import kernels as K
from . import dwconv


def _no_hooks(*mods):
    return not any(m._forward_hooks or m._forward_pre_hooks or m._backward_hooks for m in mods)


def _is_unit(m):
    conv1, pw = getattr(m, "conv1", None), getattr(m, "point_wise_cbr", None)
    if not isinstance(conv1, nn.Conv2d) or not isinstance(pw, nn.Module):
        return False
    if not (isinstance(conv1, dwconv.DepthwiseConv2d) or dwconv._eligible(conv1)):
        return False
    conv, bn = getattr(pw, "conv", None), getattr(pw, "bn", None)
    if not isinstance(conv, nn.Conv2d) or not isinstance(bn, _BatchNorm) or not getattr(pw, "has_bn", True):
        return False
    return (conv.kernel_size == (1, 1) and conv.stride == (1, 1) and conv.padding == (0, 0) and conv.dilation == (1, 1)
            and conv.groups == 1 and conv.bias is None and conv.in_channels == conv1.out_channels
            and bn.num_features == conv.out_channels and _no_hooks(pw, conv1, conv, bn))


class _FusedSeparable:
    """Mixed in front of the unit's own class by install_fused_separable."""

    tsg_fused_calls = 0                 # calls of this unit that took tsg_sepconv_fwd

    def _sep_pack(self, x):
        """the unit's constants for x's device and dtype, or None when they are stale and a capture is running"""
        conv1, pw = self.conv1, self.point_wise_cbr
        bn = pw.bn
        srcs = (conv1.weight, pw.conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var)
        stamp = tuple((t._version, t.data_ptr()) if t is not None else None for t in srcs) + (bn.eps,)
        cache = self.__dict__.setdefault("_tsg_sep_packs", {})
        key = (x.device, x.dtype)
        hit = cache.get(key)
        if hit is not None and hit[0] == stamp:
            return hit[1]
        if torch.cuda.is_current_stream_capturing():
            return None
        kp = K.provider()
        with torch.autocast("cuda", enabled=False):
            mean = bn.running_mean.float()
            invstd = torch.rsqrt(bn.running_var.float() + bn.eps)
            gamma = bn.weight.float() if bn.weight is not None else None
            beta = bn.bias.float() if bn.bias is not None else None
            fp = kp.bn_affine(mean, invstd, gamma, beta)
            wd = conv1.weight if K._dw_filter_dense(conv1.weight) else conv1.weight.contiguous()
            wp = pw.conv.weight
            if wp.stride(0) != wp.shape[1] or wp.stride(1) != 1:
                wp = wp.contiguous()
            pack = kp.sepconv_pack(wd, wp, fp, x.dtype)
        cache[key] = (stamp, pack)
        return pack

    def _sep_fused(self, x, residual, relu):
        """the fused result, or None when this call has to take the stock method"""
        pw = self.point_wise_cbr
        conv1, conv, bn = self.conv1, pw.conv, pw.bn
        if (self.training or bn.training or pw.training or torch.is_grad_enabled() or not isinstance(x, torch.Tensor)
                or not x.is_cuda or x.dim() != 4 or not dwconv._mode_ok(x)
                or not x.is_contiguous(memory_format=torch.channels_last)
                or conv1.weight.dtype != torch.float32 or conv.weight.dtype != torch.float32
                or bn.running_mean is None or bn.running_var is None or not bn.track_running_stats
                or x.shape[1] != conv1.in_channels or not _no_hooks(pw, conv1, conv, bn)):
            return None
        kp = K.provider()
        Cout, stride = conv.out_channels, conv1.stride[0]
        if not kp.sepconv_supported(x, Cout, stride):
            return None
        if residual is not None:
            oh, ow = (x.shape[2] - 1) // stride + 1, (x.shape[3] - 1) // stride + 1
            if (not isinstance(residual, torch.Tensor) or tuple(residual.shape) != (x.shape[0], Cout, oh, ow)
                    or residual.dtype != x.dtype or residual.device != x.device or residual.data_ptr() % 16
                    or not residual.is_contiguous(memory_format=torch.channels_last)):
                return None
        pack = self._sep_pack(x)
        if pack is None:
            return None
        y = kp.sepconv_fwd(x, pack, Cout, stride, residual, relu)
        self.tsg_fused_calls += 1
        return y

    def forward(self, x):
        y = self._sep_fused(x, None, bool(getattr(self.point_wise_cbr, "has_relu", False)))
        return y if y is not None else super().forward(x)

    def forward_residual(self, x, residual, relu):
        y = self._sep_fused(x, residual, relu is not None)
        if y is not None:
            return y
        stock = getattr(super(), "forward_residual", None)
        if stock is not None:
            return stock(x, residual, relu)
        from seg_opr.seg_oprs import norm_act         # a unit class without the method: the same composition
        pw = self.point_wise_cbr
        return norm_act(pw.bn, relu, pw.conv(self.conv1(x)), residual=residual)


_CLASSES = {}


def _fused_class(cls):
    sub = _CLASSES.get(cls)
    if sub is None:
        sub = _CLASSES[cls] = type("Fused" + cls.__name__, (_FusedSeparable, cls), {"__module__": __name__})
    return sub


def install_fused_separable(module):
    """Re-class, in place, every separable unit of `module` (see the module docstring); returns how many."""
    n = 0
    for m in module.modules():
        if not isinstance(m, _FusedSeparable) and _is_unit(m):
            m.__class__ = _fused_class(type(m))
            n += 1
    return n


def fused_calls(module):
    """how many calls of the units below `module` took the fused kernel so far"""
    return sum(m.tsg_fused_calls for m in module.modules() if isinstance(m, _FusedSeparable))
