"""3x3 convolution + BatchNorm (+ shortcut) (+ ReLU) as one launch at inference (csrc/convbn.hip).

In eval mode a BatchNorm is an affine map of its running statistics, so `conv3x3 -> bn -> (+ residual) -> relu` is
`relu?(fma(a, conv3x3(x, W), b) + residual)`, and `tsg_conv3x3_bnact_fwd` computes it from the fp32 accumulators of the
convolution with one rounding, at the store: one launch instead of tsg_conv3x3_gen_fwd (or tsg_conv3x3_c64_fwd) +
tsg_bn_apply_fwd, one read of x and of the residual and one write of y.  The unfused chain rounds the convolution to
bf16 first, so the fused result is not bit-equal to it (and is the closer of the two to the fp32 network).

`install_fused_convbn(module)` re-classes, in place, every module that has one of three STRUCTURES (not classes: the
reference's own network.py built on our furnace is covered as well).  "A 3x3" below is an nn.Conv2d with kernel 3x3,
stride 1, padding 1, dilation 1, groups 1, zero padding, C_in % 16 == 0 and C_out % 64 == 0:
  1. `ConvBnRelu`-shaped: `.conv` a 3x3, `has_bn` with `.bn` a BatchNorm, optionally `.relu` (`has_relu`): BiSeNet's
     attention-refinement 3x3, refines and head 3x3;
  2. `BasicBlock`-shaped (`conv1 / bn1 / relu / conv2 / bn2 / downsample`, `conv2` a 3x3): `conv2 + bn2 + residual + relu`
     is fused, and `conv1 + bn1 + relu` where conv1 is a 3x3 too (a stride-2 conv1 runs the stock conv1 and norm_act);
     the residual is `x` or the block's own `_identity(x)`;
  3. `Bottleneck`-shaped (`conv1 / bn1 / conv2 / bn2 / conv3 / bn3`): `conv2 + bn2 + relu` where conv2 is a 3x3.
Parameters, buffers and state-dict keys stay what they were.  The installer returns the number of LAYERS (convolutions)
it can fuse: a BasicBlock counts 2 or 1.

A re-classed module takes the fused kernel only when all of this holds: the module and its BatchNorms are in eval mode,
gradients are disabled, the input is a channels_last bf16 HIP tensor under bf16 autocast, the BatchNorms track running
statistics and have their buffers, the convolution weights are fp32, no module involved has a forward, forward-pre or
backward hook, the map is not 1x1 (pooled maps stay with vecconv.pooled_layer), `tsg_conv3x3_bnact_supported` takes the
shape, and a residual has the output's shape, dtype and layout and is 16-byte aligned.  Every other call — training,
gradients enabled, fp32 (the parity mode stays on the exact kernels), CPU or NCHW input — runs the method it replaced,
bit for bit.  The kernel writes a new tensor; the input and the residual are never written.

The constants (the filter in the kernel's fragment order and the BatchNorm's a, b with a convolution bias folded in) are
packed once per layer, device and dtype, and again when the `_version` (or storage) of the convolution's weight or bias
or of the BatchNorm's weight, bias, running_mean or running_var, or `eps`, has changed: `load_state_dict` and in-place
writes show in the next call, and any call that finds the module or one of its BatchNorms in train mode drops the packs
(our SyncBatchNorm moves the running statistics inside a kernel, where no tensor version counts it).  A pack is never built during a graph capture (a stale layer runs its stock path there);
the warm-up call of InferenceModule.forward builds it.

Dilated layers (csrc/dilbn.hip).  `install_fused_convbn(module, dilated=True)` also takes "a 3x3" with
padding == dilation == 2 or 4 at stride 1: the middle convolution of every Bottleneck of layer3 / layer4 in the PSPNet /
PSANet backbones (workloads/pspnet.py::_nostride_dilate; 8 layers in R50, 25 in R101).  Such a layer runs
`tsg_conv3x3_dil_bnact_fwd` instead of the vendor convolution (or `tsg_conv3x3_dil_fwd` under TSG_CONV_DIL=1) +
`tsg_bn_apply_fwd`; structures, gates, decline rules and the pack cache are the ones above, the filter of the pack does not
depend on the dilation, and the pack carries the dilation so that `_cbn_run` (and pwbn.py's Bottleneck through it) picks
the entry point.  `plain=False` re-classes only modules that hold a dilated layer.  Without `dilated=True` nothing about the
selection changes, and a dilated layer is never fused behind a module installed without it.  `fused_calls` counts the
launches of all kernels, `dil_fused_calls` those of the dilated one.

Stride-2 layers (csrc/s2bn.hip).  `install_fused_convbn(module, strided=True)` also takes "a 3x3" with stride (2, 2),
padding (1, 1) and dilation (1, 1) (never stride 2 together with a dilation above 1): BasicBlock.conv1 of the first block
of layer2 / 3 / 4 and the detail branch's conv_3x3_1 / conv_3x3_2 in BiSeNet-R18 (5 layers), Bottleneck.conv2 of the first
block of layer2 / 3 / 4 in ResNet-50 / 101 (3 layers; 1 in the dilated PSPNet / PSANet backbones).  Such a layer runs
`tsg_conv3x3_s2_bnact_fwd` instead of the vendor convolution + `tsg_bn_apply_fwd`, so a whole stride-2 BasicBlock is three
launches of ours with pwbn's shortcut (conv1 / 2, conv2 + residual, shortcut) and a Bottleneck four (conv1, conv2 / 2,
conv3, shortcut), in either install order and without a change to pwbn.py: the pack carries the stride (it is part of its
stamp) and `_cbn_run` picks the entry point.  Structures, gates, decline rules, the pack cache and hook handling are the
ones above; `_cbn_ready` asks `tsg_conv3x3_s2_bnact_supported` with the INPUT's H and W.  The flag is an attribute of the
module INSTANCE (`tsg_cbn_strided`; no parameter, buffer or state-dict key): a plain install re-classes BasicBlocks with
a stride-2 conv1 (their conv2 is eligible), and a later `strided=True` install switches the strided behaviour on for such
a module, behind pwbn's mixin too, counting its stride-2 layers only.  `plain=False` re-classes or upgrades only modules
that hold a stride-2 layer (or a dilated one with `dilated=True`).  Without `strided=True` nothing about the selection
changes, and a stride-2 layer is never fused behind a module installed without it.  `s2_fused_calls` counts the launches
of the stride-2 kernel.  seg_oprs.cbr_chain (our SpatialPath) runs its modules one after the other when gradients are
disabled and a link is an eval-mode module with the strided behaviour on, so that the re-classed forward is what runs.
The deep stem's three 3x3 layers and the 7x7 image stem of a ConvBnRelu are not taken here: torchseg_amd/stembn.py
(`install_fused_stem`, TSG_STEMBN_FUSED) fuses them, the two inner deep-stem layers on this file's kernel, gates and pack cache.

TSG_CONVBN_FUSED=0|1 (default 0) is read by torchseg_amd.infer.prepare_inference(fuse_convbn=None), TSG_DILBN_FUSED=0|1
(default 0) by prepare_inference(fuse_dilated=None), TSG_S2BN_FUSED=0|1 (default 0) by prepare_inference(fuse_strided=None);
the DDP wrapper and ddp.install_kernels never install any of them.
"""
import torch
import torch.nn as nn
from torch.nn.modules.batchnorm import _BatchNorm

from . import _lib as L
from . import fusion as _fusion
from . import kernels as K


def _no_hooks(*mods):
    return not any(m._forward_hooks or m._forward_pre_hooks or m._backward_hooks for m in mods if m is not None)


_DILATIONS = ((2, 2), (4, 4))           # what csrc/dilbn.hip takes; dilation 1 is csrc/convbn.hip's


def _is_3x3(conv, dilated=False, strided=False):
    if not (isinstance(conv, nn.Conv2d) and conv.kernel_size == (3, 3) and conv.padding == conv.dilation
            and conv.groups == 1 and conv.padding_mode == "zeros"
            and conv.in_channels % 16 == 0 and conv.out_channels % 64 == 0):
        return False
    if conv.stride == (2, 2):                           # csrc/s2bn.hip: never together with a dilation above 1
        return strided and conv.dilation == (1, 1)
    return conv.stride == (1, 1) and (conv.dilation == (1, 1) or (dilated and conv.dilation in _DILATIONS))


def _is_dilated(conv):
    return _is_3x3(conv, True) and conv.dilation != (1, 1)


def _is_strided(conv):
    return _is_3x3(conv, False, True) and conv.stride == (2, 2)


def _pair(conv, bn, dilated=False, strided=False):
    return _is_3x3(conv, dilated, strided) and isinstance(bn, _BatchNorm) and bn.num_features == conv.out_channels


def _cbr_layers(m, dilated=False, strided=False):
    """the fusable layers of a ConvBnRelu-shaped module: [(conv, bn)] or []"""
    if not isinstance(m, nn.Module) or not getattr(m, "has_bn", False):
        return []
    conv, bn = getattr(m, "conv", None), getattr(m, "bn", None)
    relu = getattr(m, "relu", None) if getattr(m, "has_relu", False) else None
    if getattr(m, "has_relu", False) and not isinstance(relu, nn.ReLU):
        return []
    return [(conv, bn)] if _pair(conv, bn, dilated, strided) and _no_hooks(m, conv, bn, relu) else []


def _has(m, *names):
    return all(hasattr(m, n) for n in names)


def _basic_layers(m, dilated=False, strided=False):
    if not _has(m, "conv1", "bn1", "relu", "conv2", "bn2", "downsample", "_identity") or hasattr(m, "conv3"):
        return []
    if not isinstance(m.conv1, nn.Conv2d) or not isinstance(m.bn1, _BatchNorm) or not isinstance(m.relu, nn.ReLU):
        return []
    if not _pair(m.conv2, m.bn2, dilated, strided) or m.conv2.in_channels != m.conv1.out_channels:
        return []
    if not _no_hooks(m, m.conv1, m.bn1, m.relu, m.conv2, m.bn2, getattr(m, "relu_inplace", None)):
        return []
    return ([(m.conv1, m.bn1)] if _pair(m.conv1, m.bn1, dilated, strided) else []) + [(m.conv2, m.bn2)]


def _bottleneck_layers(m, dilated=False, strided=False):
    if not _has(m, "conv1", "bn1", "relu", "conv2", "bn2", "conv3", "bn3", "downsample", "_identity"):
        return []
    if not all(isinstance(c, nn.Conv2d) for c in (m.conv1, m.conv3)) or not isinstance(m.relu, nn.ReLU):
        return []
    if not all(isinstance(b, _BatchNorm) for b in (m.bn1, m.bn3)) or not _pair(m.conv2, m.bn2, dilated, strided):
        return []
    if not _no_hooks(m, m.conv1, m.bn1, m.relu, m.conv2, m.bn2, m.conv3, m.bn3, getattr(m, "relu_inplace", None)):
        return []
    return [(m.conv2, m.bn2)]


def _out_shape(conv, shape):
    """shape of conv's output for an input of `shape`"""
    hw = [(n + 2 * p - d * (k - 1) - 1) // s + 1
          for n, p, d, k, s in zip(shape[2:], conv.padding, conv.dilation, conv.kernel_size, conv.stride)]
    return (shape[0], conv.out_channels, hw[0], hw[1])


def _input_ok(x):
    return (isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 4 and x.dtype == torch.bfloat16
            and not (x.shape[2] == 1 and x.shape[3] == 1) and torch.is_autocast_enabled()
            and torch.get_autocast_dtype("cuda") == torch.bfloat16
            and x.is_contiguous(memory_format=torch.channels_last))


class _Pack(tuple):
    """(wf, ab) of kernels.conv3x3_bnact_pack with the layer's `dilation` and `stride` as attributes"""


class _FusedConvBn:
    """What the three mixins share: the per-layer pack cache and the gate of a single fused call."""

    tsg_fused_calls = 0                 # calls of tsg_conv3x3_bnact_fwd, _dil_bnact_fwd and _s2_bnact_fwd made for this module
    tsg_dil_fused_calls = 0             # those of tsg_conv3x3_dil_bnact_fwd among them
    tsg_s2_fused_calls = 0              # those of tsg_conv3x3_s2_bnact_fwd among them
    tsg_cbn_dilated = False             # install_fused_convbn(dilated=True) re-classed this module (_dilated_mixin)
    tsg_cbn_strided = False             # install_fused_convbn(strided=True) took this module: set on the INSTANCE, so that a
                                        # module re-classed earlier (by a plain install, behind pwbn's mixin or not) is upgraded
                                        # without a second re-classing; no parameter, buffer or state-dict key

    def _cbn_pack(self, slot, conv, bn, x, build=None):
        """the constants of layer `slot` for x's device and dtype, or None when they are stale and a capture is running;
        `build(kp, conv, fp)` makes a pack other than conv3x3_bnact_pack's (stembn.py: the image convolutions)"""
        srcs = (conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var)
        stamp = tuple((t._version, t.data_ptr()) if t is not None else None for t in srcs) + (bn.eps, conv.dilation[0], conv.stride[0])
        cache = self.__dict__.setdefault("_tsg_cbn_packs", {})
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
            if build is not None:
                pack = build(kp, conv, fp)
            else:
                pack = _Pack(kp.conv3x3_bnact_pack(conv.weight, conv.bias, fp))    # the filter depends on neither
                pack.dilation, pack.stride = conv.dilation[0], conv.stride[0]
        cache[key] = (stamp, pack)
        return pack

    def _cbn_ready(self, slot, conv, bn, shape, x, mods):
        """the pack of layer `slot` when a call on an INPUT of `shape` (x's device, dtype and layout) can be fused"""
        if bn.training:
            self._cbn_drop()
            return None
        if (not bn.track_running_stats or bn.running_mean is None or bn.running_var is None
                or conv.weight.dtype != torch.float32 or shape[1] != conv.in_channels or (shape[2] == 1 and shape[3] == 1)
                or not _no_hooks(conv, bn, *mods)):
            return None
        lib = K.provider().lib
        if conv.stride != (1, 1):               # csrc/s2bn.hip: only behind an install that asked for it; H, W of the input
            ok = (self.tsg_cbn_strided and _is_strided(conv)
                  and lib.tsg_conv3x3_s2_bnact_supported(L.BF16, shape[0], shape[2], shape[3], conv.in_channels,
                                                         conv.out_channels))
        elif conv.dilation == (1, 1):
            ok = lib.tsg_conv3x3_bnact_supported(L.BF16, shape[0], shape[2], shape[3], conv.in_channels, conv.out_channels)
        else:                                   # csrc/dilbn.hip: only behind an install that asked for it
            ok = (self.tsg_cbn_dilated and _is_dilated(conv)
                  and lib.tsg_conv3x3_dil_bnact_supported(L.BF16, shape[0], shape[2], shape[3], conv.in_channels,
                                                          conv.out_channels, conv.dilation[0]))
        if not ok:
            return None
        return self._cbn_pack(slot, conv, bn, x)

    def _cbn_drop(self):
        """A training forward of our SyncBatchNorm moves the running statistics inside its kernel, where no tensor version
        counts it: whenever the module or one of its BatchNorms is found in train mode the packs go, and are rebuilt by
        the next fused call."""
        self.__dict__.pop("_tsg_cbn_packs", None)

    def _cbn_gate(self, x):
        if self.training:
            self._cbn_drop()
            return False
        return (not torch.is_grad_enabled() and not _fusion.CHAIN_ACTIVE and _input_ok(x)
                and x.data_ptr() % 16 == 0)

    def _cbn_run(self, x, pack, Cout, residual, relu):
        d = getattr(pack, "dilation", 1)                   # the pack carries it: callers (pwbn.py too) pass what _cbn_ready gave
        if getattr(pack, "stride", 1) == 2:
            y = K.provider().conv3x3_s2_bnact_fwd(x, pack, Cout, residual, relu)
            self.tsg_s2_fused_calls += 1
        elif d == 1:
            y = K.provider().conv3x3_bnact_fwd(x, pack, Cout, residual, relu)
        else:
            y = K.provider().conv3x3_dil_bnact_fwd(x, pack, Cout, d, residual, relu)
            self.tsg_dil_fused_calls += 1
        self.tsg_fused_calls += 1
        return y


def _residual_ok(r, shape, like):
    """r can be the kernel's residual for an output of `shape` on `like`'s device and of its dtype"""
    return (isinstance(r, torch.Tensor) and tuple(r.shape) == tuple(shape) and r.dtype == like.dtype
            and r.device == like.device and r.data_ptr() % 16 == 0 and r.is_contiguous(memory_format=torch.channels_last))


def _as_input(t):
    """the stock layer's output as the kernel reads it: channels_last and 16-byte aligned (a copy only if it is not)"""
    if t.is_contiguous(memory_format=torch.channels_last) and t.data_ptr() % 16 == 0:
        return t
    return t.clone(memory_format=torch.channels_last)


class _FusedCbr(_FusedConvBn):
    """Mixed in front of a ConvBnRelu-shaped module's own class."""

    @_fusion.outside_mode(keeps_chain=True)
    def forward(self, x):
        if self._cbn_gate(x) and getattr(self, "has_bn", False):
            relu = self.relu if getattr(self, "has_relu", False) else None
            pack = self._cbn_ready("conv", self.conv, self.bn, x.shape, x, (self, relu))
            if pack is not None:
                return self._cbn_run(x, pack, self.conv.out_channels, None, relu is not None)
        return super().forward(x)


class _FusedBasicBlock(_FusedConvBn):
    """Mixed in front of a BasicBlock-shaped module's own class."""

    def forward(self, x):
        if not self._cbn_gate(x):
            return super().forward(x)
        from seg_opr.seg_oprs import norm_act
        conv1, conv2 = self.conv1, self.conv2
        tail = getattr(self, "relu_inplace", self.relu)
        mods = (self, self.relu, tail)
        if self.bn1.training:
            self._cbn_drop()
            return super().forward(x)
        if isinstance(conv1.padding, str) or not _no_hooks(conv1, self.bn1):
            return super().forward(x)
        # everything is decided before the first launch: a decline below runs the replaced method and nothing else
        mid = _out_shape(conv1, x.shape)
        pack2 = self._cbn_ready("conv2", conv2, self.bn2, mid, x, mods)
        if pack2 is None:
            return super().forward(x)
        pack1 = None
        if _pair(conv1, self.bn1, self.tsg_cbn_dilated, self.tsg_cbn_strided):
            pack1 = self._cbn_ready("conv1", conv1, self.bn1, x.shape, x, mods)
            if pack1 is None:
                return super().forward(x)
        residual = self._identity(x)                       # eval mode: no state moves, the stock method may form it again
        if not _residual_ok(residual, _out_shape(conv2, mid), x):
            return super().forward(x)
        if pack1 is not None:
            out = self._cbn_run(x, pack1, conv1.out_channels, None, True)
        else:                                              # a stride-2 conv1 without `strided`: the stock layer, bf16 here
            out = _as_input(norm_act(self.bn1, self.relu, conv1(x)))
        return self._cbn_run(out, pack2, conv2.out_channels, residual, True)


class _FusedBottleneck(_FusedConvBn):
    """Mixed in front of a Bottleneck-shaped module's own class."""

    def forward(self, x):
        if not self._cbn_gate(x) or self.bn1.training or self.bn3.training:
            return super().forward(x)
        from seg_opr.seg_oprs import norm_act
        mods = (self, self.conv1, self.bn1, self.relu, self.conv3, self.bn3, getattr(self, "relu_inplace", None))
        if isinstance(self.conv1.padding, str):
            return super().forward(x)
        mid = _out_shape(self.conv1, x.shape)
        pack = self._cbn_ready("conv2", self.conv2, self.bn2, mid, x, mods)
        if pack is None:
            return super().forward(x)
        out = _as_input(norm_act(self.bn1, self.relu, self.conv1(x)))      # bf16 under this autocast, of shape `mid`
        out = self._cbn_run(out, pack, self.conv2.out_channels, None, True)
        return norm_act(self.bn3, getattr(self, "relu_inplace", self.relu), self.conv3(out), residual=self._identity(x))


_CLASSES = {}


def _fused_class(cls, mixin):
    sub = _CLASSES.get((cls, mixin))
    if sub is None:
        sub = _CLASSES[(cls, mixin)] = type("Fused" + cls.__name__, (mixin, cls), {"__module__": __name__})
    return sub


_DILATED = {}


def _dilated_mixin(mixin):
    """`mixin` as install_fused_convbn(dilated=True) installs it: the same methods, and the dilated layers are taken"""
    sub = _DILATED.get(mixin)
    if sub is None:
        sub = _DILATED[mixin] = type(mixin.__name__ + "Dilated", (mixin,), {"__module__": __name__, "tsg_cbn_dilated": True})
    return sub


def eligible_layers(m, dilated=False, strided=False):
    """(mixin, [(conv, bn), ...]) of a module that has one of the three structures, else (None, []); `dilated`: a 3x3 of
    dilation 2 or 4 (padding alike) counts as well; `strided`: one of stride 2 (padding 1, dilation 1) too"""
    for mixin, find in ((_FusedBottleneck, _bottleneck_layers), (_FusedBasicBlock, _basic_layers), (_FusedCbr, _cbr_layers)):
        layers = find(m, dilated, strided)
        if layers:
            return (_dilated_mixin(mixin) if dilated else mixin), layers
    return None, []


def eligible_dilated_layers(m):
    """the dilated (2 or 4) layers among eligible_layers(m, dilated=True)[1]: what csrc/dilbn.hip would run"""
    return [(conv, bn) for conv, bn in eligible_layers(m, True)[1] if _is_dilated(conv)]


def eligible_strided_layers(m):
    """the stride-2 layers among eligible_layers(m, strided=True)[1]: what csrc/s2bn.hip would run"""
    return [(conv, bn) for conv, bn in eligible_layers(m, False, True)[1] if _is_strided(conv)]


def install_fused_convbn(module, dilated=False, plain=True, strided=False):
    """Re-class, in place, every module of `module` with one of the three structures (see the module docstring); returns
    how many layers (convolutions) become fusable by this call.  `dilated`: layers of dilation 2 and 4 are taken too.
    `strided`: layers of stride 2 are taken too, and a module re-classed by an earlier call without it is upgraded (its
    stride-2 layers are what is counted then).  `plain=False` (with `dilated` / `strided`): only modules that hold a dilated
    / stride-2 layer are re-classed or upgraded."""
    from .pwbn import rebased                                # a module pwbn.py re-classed keeps that mixin in front of ours
    n = 0
    for m in module.modules():
        if isinstance(m, _FusedConvBn):
            if strided and not m.tsg_cbn_strided:            # the upgrade: the class stays, the stride-2 layers are switched on
                layers = [cb for cb in eligible_layers(m, m.tsg_cbn_dilated, True)[1] if _is_strided(cb[0])]
                if layers:
                    m.__dict__["tsg_cbn_strided"] = True
                    n += len(layers)
            continue
        mixin, layers = eligible_layers(m, dilated, strided)
        if mixin is not None and (plain or (dilated and eligible_dilated_layers(m))
                                  or (strided and eligible_strided_layers(m))):
            m.__class__ = rebased(type(m), lambda cls: _fused_class(cls, mixin))
            if strided:
                m.__dict__["tsg_cbn_strided"] = True
            n += len(layers)
    return n


def fused_calls(module):
    """how many launches of the fused kernels (csrc/convbn.hip, csrc/dilbn.hip and csrc/s2bn.hip) the modules below `module`
    made so far"""
    return sum(m.tsg_fused_calls for m in module.modules() if isinstance(m, _FusedConvBn))


def dil_fused_calls(module):
    """how many launches of the dilated kernel (csrc/dilbn.hip) alone"""
    return sum(m.tsg_dil_fused_calls for m in module.modules() if isinstance(m, _FusedConvBn))


def s2_fused_calls(module):
    """how many launches of the stride-2 kernel (csrc/s2bn.hip) alone"""
    return sum(m.tsg_s2_fused_calls for m in module.modules() if isinstance(m, _FusedConvBn))
