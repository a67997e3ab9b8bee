"""1x1 convolution + BatchNorm (+ shortcut) (+ ReLU) as one launch at inference (csrc/pwbn.hip).

In eval mode a BatchNorm is an affine map of its running statistics, so `conv1x1 -> bn -> (+ residual) -> relu` is
`relu?(fma(a, conv1x1(x, W), b) + residual)`, and `tsg_conv1x1_bnact_fwd` computes it from the fp32 accumulators of the
convolution with one rounding, at the store: one launch instead of the 1x1 convolution + tsg_bn_apply_fwd.  The unfused
chain rounds the convolution to bf16 first, so the fused result is not bit-equal to it.  This is the point-wise twin of
convbn.py (the 3x3 layers), with the same gates, the same pack cache and the same decline-to-the-replaced-method rule.

`install_fused_pointwise(module)` re-classes, in place, every module that has one of three STRUCTURES (not classes).
"A 1x1" below is an nn.Conv2d with kernel 1x1, stride (1, 1) or (2, 2), padding 0, groups 1 and C_in, C_out multiples of 64
in [64, 2048]; dilation is irrelevant:
  1. `ConvBnRelu`-shaped: `.conv` a 1x1, `has_bn` with `.bn` a BatchNorm, optionally `.relu` (`has_relu`):
     FeatureFusion.conv_1x1, the PSP / PSA reductions, a `has_bias=True` layer;
  2. blocks with `_identity`, `downsample[0]` a 1x1 and `downsample[1]` a BatchNorm: `_identity(x)` runs the shortcut as one
     launch (no ReLU, no residual) wherever the running forward forms the residual through it;
  3. `Bottleneck`-shaped (`conv1 / bn1 / conv2 / bn2 / conv3 / bn3`, conv1 and conv3 a 1x1): `conv1 + bn1 + relu` and
     `conv3 + bn3 + residual + relu` are fused; the convolution in the middle runs exactly what the class behind the mixin
     would run: convbn's fused 3x3 where the module is convbn's too and its gate holds, else the stock
     `norm_act(bn2, relu, conv2(out))`.  The mixin goes IN FRONT of the module's current class in either install order
     (convbn.install_fused_convbn slides its own mixin in behind ours).
Parameters, buffers and state-dict keys stay what they were.  The installer returns the number of LAYERS (convolutions)
it can fuse: a Bottleneck counts 2, or 3 with a 1x1 shortcut.

A re-classed module takes the fused kernel only when all of this holds: the module and its BatchNorms are in eval mode,
gradients are disabled, the input is a channels_last bf16 HIP tensor under bf16 autocast, the BatchNorms track running
statistics and have their buffers, the convolution weights are fp32, no module involved has a forward, forward-pre or
backward hook, the map is not 1x1 (pooled maps stay with vecconv.pooled_layer), no ConvBnRelu chain fusion is active
(fusion.CHAIN_ACTIVE), `tsg_conv1x1_bnact_supported` takes the shape, and a residual has the output's shape, dtype and
layout and is 16-byte aligned.  Every other call runs the method it replaced, bit for bit.  The kernel writes a new
tensor; the input and the residual are never written.

The constants are packed once per layer, device and dtype, and again when the `_version` (or storage) of the
convolution's weight or bias or of the BatchNorm's weight, bias, running_mean or running_var, or `eps`, has changed; any
call that finds the module or one of its BatchNorms in train mode drops the packs.  A pack is never built during a graph
capture (a stale layer runs its stock path there); the warm-up call of InferenceModule.forward builds it.

TSG_PWBN_FUSED=0|1 (default 0) is read by torchseg_amd.infer.prepare_inference(fuse_pointwise=None); the DDP wrapper and
ddp.install_kernels never install this.
"""
import torch
import torch.nn as nn
from torch.nn.modules.batchnorm import _BatchNorm

from . import _lib as L
from . import fusion as _fusion
from . import kernels as K
from .convbn import _FusedConvBn, _as_input, _has, _input_ok, _no_hooks, _out_shape, _residual_ok


def _is_1x1(conv):
    return (isinstance(conv, nn.Conv2d) and conv.kernel_size == (1, 1) and conv.stride in ((1, 1), (2, 2))
            and conv.padding == (0, 0) and conv.groups == 1
            and conv.in_channels % 64 == 0 and 64 <= conv.in_channels <= 2048
            and conv.out_channels % 64 == 0 and 64 <= conv.out_channels <= 2048)


def _pair(conv, bn):
    return _is_1x1(conv) and isinstance(bn, _BatchNorm) and bn.num_features == conv.out_channels


def _cbr_layers(m):
    """the fusable layers of a ConvBnRelu-shaped module: [(conv, bn)] or []"""
    if not isinstance(m, nn.Module) or not getattr(m, "has_bn", False):
        return []
    conv, bn = getattr(m, "conv", None), getattr(m, "bn", None)
    relu = getattr(m, "relu", None) if getattr(m, "has_relu", False) else None
    if getattr(m, "has_relu", False) and not isinstance(relu, nn.ReLU):
        return []
    return [(conv, bn)] if _pair(conv, bn) and _no_hooks(m, conv, bn, relu) else []


def _shortcut_layers(m):
    """the 1x1 shortcut of a block that forms its residual through `_identity`: [(conv, bn)] or []"""
    if not isinstance(m, nn.Module) or not _has(m, "_identity", "downsample"):
        return []
    ds = m.downsample
    if not isinstance(ds, (nn.Sequential, nn.ModuleList)) or len(ds) < 2:
        return []
    return [(ds[0], ds[1])] if _pair(ds[0], ds[1]) and _no_hooks(m, ds, ds[0], ds[1]) else []


def _bottleneck_layers(m):
    if not _has(m, "conv1", "bn1", "relu", "conv2", "bn2", "conv3", "bn3", "downsample", "_identity"):
        return []
    if not isinstance(m.conv2, nn.Conv2d) or isinstance(m.conv2.padding, str) or not isinstance(m.bn2, _BatchNorm):
        return []
    if not isinstance(m.relu, nn.ReLU) or not _pair(m.conv1, m.bn1) or not _pair(m.conv3, m.bn3):
        return []
    if m.conv2.in_channels != m.conv1.out_channels or m.conv3.in_channels != m.conv2.out_channels:
        return []
    if not _no_hooks(m, m.conv1, m.bn1, m.relu, m.conv2, m.bn2, m.conv3, m.bn3, getattr(m, "relu_inplace", None)):
        return []
    return [(m.conv1, m.bn1), (m.conv3, m.bn3)] + _shortcut_layers(m)


class _FusedPointwise:
    """What the three mixins share: the per-layer pack cache and the gate of a single fused call."""

    tsg_pw_fused_calls = 0              # calls of tsg_conv1x1_bnact_fwd made for this module

    def _pwb_pack(self, slot, conv, bn, x):
        """the constants of layer `slot` for x's device and dtype, or None when they are stale and a capture is running"""
        srcs = (conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var)
        stamp = tuple((t._version, t.data_ptr()) if t is not None else None for t in srcs) + (bn.eps,)
        cache = self.__dict__.setdefault("_tsg_pwb_packs", {})
        key = (slot, x.device, x.dtype)
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
            pack = kp.conv1x1_bnact_pack(conv.weight, conv.bias, fp)
        cache[key] = (stamp, pack)
        return pack

    def _pwb_ready(self, slot, conv, bn, shape, x, mods):
        """the pack of layer `slot` when a call on an input of `shape` (x's device, dtype and layout) can be fused"""
        if bn.training:
            self._pwb_drop()
            return None
        if (not _pair(conv, bn) or not bn.track_running_stats or bn.running_mean is None or bn.running_var is None
                or conv.weight.dtype != torch.float32 or shape[1] != conv.in_channels or (shape[2] == 1 and shape[3] == 1)
                or not _no_hooks(conv, bn, *mods)):
            return None
        if not K.provider().lib.tsg_conv1x1_bnact_supported(L.BF16, shape[0], shape[2], shape[3], conv.in_channels,
                                                            conv.out_channels, conv.stride[0]):
            return None
        return self._pwb_pack(slot, conv, bn, x)

    def _pwb_drop(self):
        """whenever the module or one of its BatchNorms is found in train mode the packs go (convbn._FusedConvBn._cbn_drop)"""
        self.__dict__.pop("_tsg_pwb_packs", None)

    def _pwb_gate(self, x):
        if self.training:
            self._pwb_drop()
            return False
        return (not torch.is_grad_enabled() and not _fusion.CHAIN_ACTIVE and _input_ok(x)
                and x.data_ptr() % 16 == 0)

    def _pwb_run(self, x, pack, conv, residual, relu):
        y = K.provider().conv1x1_bnact_fwd(x, pack, conv.out_channels, conv.stride[0], residual, relu)
        self.tsg_pw_fused_calls += 1
        return y


class _FusedPwCbr(_FusedPointwise):
    """Mixed in front of a ConvBnRelu-shaped module's own class."""

    @_fusion.outside_mode(keeps_chain=True)
    def forward(self, x):
        if self._pwb_gate(x) and getattr(self, "has_bn", False):
            relu = self.relu if getattr(self, "has_relu", False) else None
            pack = self._pwb_ready("conv", self.conv, self.bn, x.shape, x, (self, relu))
            if pack is not None:
                return self._pwb_run(x, pack, self.conv, None, relu is not None)
        return super().forward(x)


class _FusedPwShortcut(_FusedPointwise):
    """Mixed in front of a block that forms its residual through `_identity`: the whole BasicBlock support."""

    def _identity(self, x):
        ds = self.downsample
        if (isinstance(ds, (nn.Sequential, nn.ModuleList)) and len(ds) >= 2 and not self.__dict__.get("_tsg_pwb_declined")
                and self._pwb_gate(x)):
            pack = self._pwb_ready("downsample", ds[0], ds[1], x.shape, x, (self, ds))
            if pack is not None:
                return self._pwb_run(x, pack, ds[0], None, False)
        return super()._identity(x)


class _FusedPwBottleneck(_FusedPwShortcut):
    """Mixed in front of a Bottleneck-shaped module's current class (which may be convbn's FusedBottleneck)."""

    def _pwb_decline(self, x):
        """the replaced forward and nothing of ours: its `_identity` call runs the replaced shortcut too"""
        self.__dict__["_tsg_pwb_declined"] = True
        try:
            return super().forward(x)
        finally:
            self.__dict__.pop("_tsg_pwb_declined", None)

    def forward(self, x):
        if not self._pwb_gate(x):
            return self._pwb_decline(x)
        if self.bn1.training or self.bn2.training or self.bn3.training:
            self._pwb_drop()
            return self._pwb_decline(x)
        from seg_opr.seg_oprs import norm_act
        conv1, conv2, conv3 = self.conv1, self.conv2, self.conv3
        tail = getattr(self, "relu_inplace", self.relu)
        mods = (self, self.relu, tail)
        if not isinstance(conv2, nn.Conv2d) or isinstance(conv2.padding, str) or not _no_hooks(conv2, self.bn2):
            return self._pwb_decline(x)
        # everything is decided before the first launch of the three layers: a decline below runs the replaced method and
        # nothing else of ours (the residual is formed first, as in convbn's BasicBlock; our shortcut's output always passes)
        mid1 = _out_shape(conv1, x.shape)
        mid2 = _out_shape(conv2, mid1)
        out_shape = _out_shape(conv3, mid2)
        if min(mid1[2:]) < 1 or min(mid2[2:]) < 1:
            return self._pwb_decline(x)
        pack1 = self._pwb_ready("conv1", conv1, self.bn1, x.shape, x, mods)
        pack3 = self._pwb_ready("conv3", conv3, self.bn3, mid2, x, mods) if pack1 is not None else None
        if pack3 is None:
            return self._pwb_decline(x)
        pack2 = None                                       # the 3x3 in the middle: what the class behind this one would run
        if isinstance(self, _FusedConvBn) and self._cbn_gate(x):
            pack2 = self._cbn_ready("conv2", conv2, self.bn2, mid1, x,
                                    (self, conv1, self.bn1, self.relu, conv3, self.bn3, getattr(self, "relu_inplace", None)))
        residual = self._identity(x)                       # eval mode: no state moves, the stock method may form it again
        if not _residual_ok(residual, out_shape, x):
            return self._pwb_decline(x)
        out = self._pwb_run(x, pack1, conv1, None, True)
        if pack2 is not None:
            out = self._cbn_run(out, pack2, conv2.out_channels, None, True)
        else:
            out = _as_input(norm_act(self.bn2, self.relu, conv2(out)))
        return self._pwb_run(out, pack3, conv3, residual, True)


_CLASSES = {}


def _fused_class(cls, mixin):
    sub = _CLASSES.get((cls, mixin))
    if sub is None:
        # tsg_pw_front: (our mixin, the class behind it) -- convbn.install_fused_convbn re-bases on it, so that its mixin
        # lands BEHIND ours whichever installer runs first
        sub = _CLASSES[(cls, mixin)] = type("FusedPw" + cls.__name__, (mixin, cls),
                                            {"__module__": __name__, "tsg_pw_front": (mixin, cls)})
    return sub


def rebased(cls, wrap):
    """`cls` with the class behind our mixin replaced by wrap(that class); `cls` itself when it is not one of ours"""
    front = cls.__dict__.get("tsg_pw_front")
    if front is None:
        return wrap(cls)
    return _fused_class(wrap(front[1]), front[0])


def eligible_layers(m):
    """(mixin, [(conv, bn), ...]) of a module that has one of the three structures, else (None, [])"""
    for mixin, find in ((_FusedPwBottleneck, _bottleneck_layers), (_FusedPwShortcut, _shortcut_layers),
                        (_FusedPwCbr, _cbr_layers)):
        layers = find(m)
        if layers:
            return mixin, layers
    return None, []


def install_fused_pointwise(module):
    """Re-class, in place, every module of `module` with one of the three structures (see the module docstring); returns
    how many layers (convolutions) the re-classed modules can fuse."""
    n = 0
    for m in module.modules():
        if isinstance(m, _FusedPointwise):
            continue
        mixin, layers = eligible_layers(m)
        if mixin is not None:
            m.__class__ = _fused_class(type(m), mixin)
            n += len(layers)
    return n


def fused_calls(module):
    """how many launches of the fused 1x1 kernel the modules below `module` made so far"""
    return sum(m.tsg_pw_fused_calls for m in module.modules() if isinstance(m, _FusedPointwise))
