"""The image stems and the v1c deep stem with their BatchNorm (+ ReLU) as one launch per layer at inference.

What torchseg_amd/convbn.py and pwbn.py leave out is everything in front of layer1: the two convolutions that read the
image (C_in = 3) and the deep stem's two inner 3x3 layers, which sit in a bare nn.Sequential with their last BatchNorm
outside it.  They are the largest maps of every network.  `install_fused_stem(module)` re-classes, in place and by
STRUCTURE, two kinds of module:

  1. `ConvBnRelu`-shaped with a 7x7 image stem: `.conv` an nn.Conv2d(3, 64, 7, stride 2, padding 3, bias=False) (the
     hyper-parameters of stemconv._is_stem; the class may already be StemConv2d), `has_bn` with `.bn` a BatchNorm of 64
     features, optionally `.relu`: BiSeNet's SpatialPath.conv_7x7.  Its forward runs `tsg_stem_conv_bnact_fwd`
     (csrc/stemconv.hip stem_bnact_fwd_k) on the bf16 image: one launch instead of stem_pack_w + tsg_stem_conv_fwd +
     tsg_bn_apply_fwd.  One layer.
  2. `ResNet`-shaped with a v1c deep stem of width 64: `conv1` an nn.Sequential of exactly
     [Conv 3->64 3x3/2/1 no bias, BN(64), ReLU, Conv 64->64 3x3/1/1, BN(64), ReLU, Conv 64->128 3x3/1/1], and `bn1`
     (128 features), `relu`, `maxpool`, `_stem`: FCN, PSPNet, PSANet, DFN, BiSeNet-R101.  `_stem` then runs
     `tsg_stem3_conv_bnact_fwd` (c0 + c1 + c2; csrc/deepstem.hip ds_bnact_fwd_k), `tsg_conv3x3_bnact_fwd` (c3 + c4 + c5),
     `tsg_conv3x3_bnact_fwd` (c6 + bn1 + relu) and `self.maxpool`.  Three layers.  A stem of another width, or whose first
     convolution has a bias, groups or another kernel, is left alone (the image kernel is 3 -> 64).
Parameters, buffers and state-dict keys stay what they were; the installer returns the number of LAYERS taken, 0 for a
module it re-classed before.

Each layer is fused on its own terms at every call: the image layer needs `tsg_stem*_conv_bnact_supported` (the 7x7: an
even W), the inner two `tsg_conv3x3_bnact_supported`; a layer that declines runs its stock modules and the others still
fuse.  The gates are convbn.py's: the module and the BatchNorms in eval mode, gradients disabled, bf16 autocast, the
BatchNorms tracking running statistics and holding their buffers, fp32 weights, no hook on any module involved, an image
that does not require a gradient; the constants are packed once per layer, device and dtype under convbn's stamp (again
after load_state_dict or an in-place write), never during a graph capture (a stale layer runs its stock modules there), and
dropped whenever the module or one of its BatchNorms is found in train mode.  In fp32 (the parity mode) nothing is fused.
A call where nothing can be fused runs the method that was replaced, bit for bit.  The image kernels round once, at the
store, so their result is not bit-equal to the two-launch chain (and is the closer of the two to the fp32 network).

seg_oprs.cbr_chain (our SpatialPath) runs its modules one after the other when gradients are disabled and a link is an
eval-mode module of kind 1, as it does behind convbn's strided install.

`fused_calls(module)`: the launches made through this installer; `image_fused_calls(module)`: those of the two image
kernels.  TSG_STEMBN_FUSED=0|1 (default 0) is read by torchseg_amd.infer.prepare_inference(fuse_stem=None), which installs
this after the other four installers; the DDP wrapper and ddp.install_kernels never install it.
"""
import torch
import torch.nn as nn
from torch.nn.modules.batchnorm import _BatchNorm

from . import _lib as L
from . import fusion as _fusion
from . import kernels as K
from .convbn import _FusedConvBn, _as_input, _input_ok, _no_hooks, _pair
from .stemconv import _as_bf16_image


def _image_conv(conv, k):
    """nn.Conv2d(3, 64, k, stride 2, padding k // 2, bias=False), whatever class the kernel install gave it"""
    return (isinstance(conv, nn.Conv2d) and conv.in_channels == 3 and conv.out_channels == 64
            and conv.kernel_size == (k, k) and conv.stride == (2, 2) and conv.padding == (k // 2, k // 2)
            and conv.dilation == (1, 1) and conv.groups == 1 and conv.bias is None and conv.padding_mode == "zeros")


def _image_pair(conv, bn, k):
    return _image_conv(conv, k) and isinstance(bn, _BatchNorm) and bn.num_features == 64


def _cbr_stem(m):
    """a ConvBnRelu-shaped module around a 7x7 image stem"""
    if not isinstance(m, nn.Module) or not getattr(m, "has_bn", False):
        return False
    conv, bn = getattr(m, "conv", None), getattr(m, "bn", None)
    relu = getattr(m, "relu", None) if getattr(m, "has_relu", False) else None
    if getattr(m, "has_relu", False) and not isinstance(relu, nn.ReLU):
        return False
    return _image_pair(conv, bn, 7) and _no_hooks(m, conv, bn, relu)


def _deep_stem(m):
    """the seven entries of a ResNet-shaped module's v1c deep stem of width 64, or None"""
    if not all(hasattr(m, n) for n in ("conv1", "bn1", "relu", "maxpool", "_stem")):
        return None
    c = m.conv1
    if not isinstance(c, nn.Sequential) or len(c) != 7 or not isinstance(m.relu, nn.ReLU):
        return None
    if not isinstance(c[2], nn.ReLU) or not isinstance(c[5], nn.ReLU) or not isinstance(m.maxpool, nn.Module):
        return None
    if not (_image_pair(c[0], c[1], 3) and _pair(c[3], c[4]) and _pair(c[6], m.bn1)):
        return None
    if (c[3].in_channels, c[3].out_channels, c[6].in_channels, c[6].out_channels) != (64, 64, 64, 128):
        return None
    return tuple(c)


def _image_pack(kp, conv, fp):
    return kp.image_bnact_pack(conv.weight, fp)


class _FusedStem:
    """What the two mixins share: convbn's pack cache (its methods, not copies of them), the gate on the image and the
    two counters."""

    tsg_stem_fused = True               # seg_oprs.cbr_chain asks for it
    tsg_stem_fused_calls = 0            # launches of the four entry points made for this module
    tsg_stem_image_calls = 0            # those of tsg_stem_conv_bnact_fwd / tsg_stem3_conv_bnact_fwd among them
    tsg_cbn_dilated = False             # _cbn_ready reads them: the inner layers are plain stride-1 3x3s
    tsg_cbn_strided = False

    _cbn_pack = _FusedConvBn._cbn_pack
    _cbn_ready = _FusedConvBn._cbn_ready
    _cbn_drop = _FusedConvBn._cbn_drop

    def _stb_gate(self, x):
        if self.training:
            self._cbn_drop()
            return False
        return (not torch.is_grad_enabled() and not _fusion.CHAIN_ACTIVE and isinstance(x, torch.Tensor) and x.is_cuda
                and x.dim() == 4 and x.shape[1] == 3 and x.dtype in (torch.float32, torch.bfloat16)
                and not x.requires_grad and torch.is_autocast_enabled()
                and torch.get_autocast_dtype("cuda") == torch.bfloat16)

    def _stb_image_ready(self, slot, conv, bn, k, x, mods):
        """(pack, bf16 image) when the image layer `slot` (a k x k convolution) can be fused on x, else None; nothing is
        launched before the shape is known to be taken"""
        if bn.training:
            self._cbn_drop()
            return None
        if (not _image_pair(conv, bn, k) or not bn.track_running_stats or bn.running_mean is None
                or bn.running_var is None or conv.weight.dtype != torch.float32 or not _no_hooks(conv, bn, *mods)):
            return None
        supported = getattr(K.provider().lib, "tsg_stem_conv_bnact_supported" if k == 7 else "tsg_stem3_conv_bnact_supported")
        if not supported(L.BF16, x.shape[0], x.shape[2], x.shape[3]):
            return None
        xb = _as_bf16_image(x)
        if not K.provider().image_bnact_supported(xb, k):
            return None
        pack = self._cbn_pack(slot, conv, bn, xb, build=_image_pack)
        return None if pack is None else (pack, xb)

    def _stb_image_run(self, ready, k, relu):
        y = K.provider().image_bnact_fwd(ready[1], ready[0], k, relu)
        self.tsg_stem_image_calls += 1
        self.tsg_stem_fused_calls += 1
        return y

    def _stb_inner_run(self, x, pack, Cout):
        y = K.provider().conv3x3_bnact_fwd(x, pack, Cout, None, True)
        self.tsg_stem_fused_calls += 1
        return y


class _FusedStemCbr(_FusedStem):
    """Mixed in front of a ConvBnRelu-shaped module's own class."""

    @_fusion.outside_mode(keeps_chain=True)
    def forward(self, x):
        if self._stb_gate(x) and getattr(self, "has_bn", False):
            relu = self.relu if getattr(self, "has_relu", False) else None
            ready = self._stb_image_ready("conv", self.conv, self.bn, 7, x, (self, relu))
            if ready is not None:
                return self._stb_image_run(ready, 7, relu is not None)
        return super().forward(x)


class _FusedDeepStem(_FusedStem):
    """Mixed in front of a ResNet-shaped module's own class: `_stem` is what changes."""

    def _stem(self, x):
        c = _deep_stem(self) if self._stb_gate(x) else None
        if c is None:
            return super()._stem(x)
        from seg_opr.seg_oprs import norm_act
        mods = (self, self.conv1, c[2], c[5], self.relu, self.maxpool)
        # the three decisions, before the first launch: a call where nothing fuses is the replaced method and nothing else
        ready0 = self._stb_image_ready("c0", c[0], c[1], 3, x, mods)
        mid = (x.shape[0], 64, (x.shape[2] - 1) // 2 + 1, (x.shape[3] - 1) // 2 + 1)
        like = ready0[1] if ready0 is not None else torch.empty(0, dtype=torch.bfloat16, device=x.device)
        pack1 = self._cbn_ready("c3", c[3], c[4], mid, like, mods)
        pack2 = self._cbn_ready("c6", c[6], self.bn1, mid, like, mods)
        if ready0 is None and pack1 is None and pack2 is None:
            return super()._stem(x)
        y = self._stb_image_run(ready0, 3, True) if ready0 is not None else norm_act(c[1], c[2], c[0](x))
        for pack, conv, bn, relu in ((pack1, c[3], c[4], c[5]), (pack2, c[6], self.bn1, self.relu)):
            yin = _as_input(y) if pack is not None and isinstance(y, torch.Tensor) and y.dim() == 4 else None
            if yin is not None and _input_ok(yin) and tuple(yin.shape) == mid:
                y = self._stb_inner_run(yin, pack, conv.out_channels)
            elif conv is c[3]:
                y = norm_act(bn, relu, conv(y))
            else:                                              # the stock tail of ResNet._stem
                y = conv(y)
                if y.is_cuda:
                    from .syncbn import bn_relu_maxpool
                    out = bn_relu_maxpool(bn, y, self.maxpool)
                    if out is not None:
                        return out
                return self.maxpool(norm_act(bn, relu, y))
        return self.maxpool(y)


_CLASSES = {}


def _fused_class(cls, mixin):
    sub = _CLASSES.get((cls, mixin))
    if sub is None:
        sub = _CLASSES[(cls, mixin)] = type("FusedStem" + cls.__name__, (mixin, cls), {"__module__": __name__})
    return sub


def eligible(m):
    """(mixin, number of layers) of a module with one of the two structures, else (None, 0)"""
    if _cbr_stem(m):
        return _FusedStemCbr, 1
    c = _deep_stem(m)
    if c is not None and _no_hooks(m, m.conv1, *c, m.bn1, m.relu, m.maxpool):
        return _FusedDeepStem, 3
    return None, 0


def install_fused_stem(module):
    """Re-class, in place, every module of `module` with one of the two structures (see the module docstring); returns how
    many layers (convolutions) become fusable by this call."""
    n = 0
    for m in module.modules():
        if isinstance(m, _FusedStem):
            continue
        mixin, layers = eligible(m)
        if mixin is not None:
            m.__class__ = _fused_class(type(m), mixin)
            n += layers
    return n


def fused_calls(module):
    """how many launches the modules below `module` made through this installer so far (image and inner layers)"""
    return sum(m.tsg_stem_fused_calls for m in module.modules() if isinstance(m, _FusedStem))


def image_fused_calls(module):
    """how many launches of the two image kernels (stem_bnact_fwd_k, ds_bnact_fwd_k) alone"""
    return sum(m.tsg_stem_image_calls for m in module.modules() if isinstance(m, _FusedStem))
