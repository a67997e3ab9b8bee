"""PSPNet's pyramid pooling head without the concatenation at inference (csrc/ppmbn.hip).

The stock head (workloads/pspnet.py::PyramidPooling.forward, the reference's network.py alike) pools x on n grids, runs a
1x1 ConvBnRelu on each pooled map, up-samples the n results bilinearly (align_corners=True) back to the full map,
concatenates them with x and runs `conv6`: a 3x3 ConvBnRelu over C + n Cb channels, a dropout and the classifier.  Half of
that convolution's K dimension is the interpolation of at most 50 pooled pixels.  Interpolation and convolution are both
linear, so `install_fused_pyramid` contracts that half on the pooled maps (csrc/ppm_geom.h states the arithmetic):

    p_s = ppm[s](x)                                           as the modules run today
    T   = tsg_ppm_taps_fwd(p_0 .. p_{n-1}, W6[:, C:])         fp32 tap tables [B, cells, 9, Cout]
    E   = tsg_ppm_addend_fwd(T)                               fp32 NHWC: the pooled channels' share of the convolution
    y   = tsg_conv3x3_bnact_add_fwd(x, W6[:, :C], E, a, b)    bf16(relu(fma(a, conv3x3(x) + E, b))), ONE rounding
    out = conv6[1:](y)

Neither the up-sampled maps nor the concatenated tensor is formed, and the full-map convolution reads x alone.  The stock
chain rounds the up-sampled maps to bf16 before the convolution reads them; here the interpolated values stay fp32, so the
result is not bit-equal to the chain's (and is the closer of the two to the fp32 network).

`install_fused_pyramid(module)` re-classes, in place, every module that has this STRUCTURE (not class: the reference's own
PyramidPooling built on our furnace is covered):
  - `ppm`: an nn.ModuleList of 1 to 4 `nn.Sequential(nn.AdaptiveAvgPool2d, ConvBnRelu-shaped 1x1)`, all of the same input
    width C and output width Cb (a multiple of 16);
  - `conv6`: an nn.Sequential whose first entry is a ConvBnRelu-shaped 3x3 / stride 1 / padding 1 layer (BatchNorm, C_out a
    multiple of 64) with `in_channels == C + n Cb`;
  - no forward, forward-pre or backward hook on the module, on `conv6`, on its first entry or on any module of `ppm`.
Parameters, buffers and state-dict keys stay what they were.  The installer returns the number of heads it re-classed:
1 for PSPNet, 0 for BiSeNet, PSANet and FCN.

Gates, decline rules, hook handling, the pack cache and its stamp are convbn.py's (its methods, not copies): the module and
conv6's BatchNorm in eval mode, gradients disabled, x a channels_last bf16 HIP tensor under bf16 autocast and 16-byte
aligned, running statistics present, an fp32 weight, no hooks, `tsg_ppm_supported` takes the shape (pooled maps of at most
64 cells each and 32 columns together), and every p_s comes out bf16 with the shape its pool announces.  Every other call
runs the method it replaced, bit for bit -- with a `conv6[0]` that install_fused_convbn re-classed, that layer's own fused
forward included.  The pack (the filter of W6[:, :C] in conv3x3_bnact_pack's order, a and b with a bias folded in, and the
branch slices [n, 9, Cout, Cb] rounded to bf16) is built once per layer, device and dtype, rebuilt when a source tensor's
version or storage changed, and never built during a graph capture.  The workspace of T and E (tsg_ppm_ws_bytes) is one
torch allocation per call: the three launches are capturable and bit-identical from call to call.

TSG_PPMBN_FUSED=0|1 (default 0) is read by torchseg_amd.infer.prepare_inference(fuse_pyramid=None); the DDP wrapper never
installs this.  Not covered: the pools and the branch convolutions, the classifier, PSANet's cat([x, psa]), training.
"""
import torch
import torch.nn as nn

from . import kernels as K
from .convbn import _FusedConvBn, _cbr_layers, _no_hooks

MAX_BRANCHES = 4


def _branch(seq):
    """(pool, cbr) of a `Sequential(AdaptiveAvgPool2d, 1x1 ConvBnRelu)`, else None"""
    if not isinstance(seq, nn.Sequential) or len(seq) != 2 or not isinstance(seq[0], nn.AdaptiveAvgPool2d):
        return None
    cbr = seq[1]
    conv = getattr(cbr, "conv", None)
    if not (isinstance(cbr, nn.Module) and isinstance(conv, nn.Conv2d) and conv.kernel_size == (1, 1)
            and conv.stride == (1, 1) and conv.padding == (0, 0) and conv.groups == 1 and hasattr(cbr, "has_bn")):
        return None
    return seq[0], cbr


def _pyramid(m):
    """(branches [(pool, cbr)], conv6[0], C, Cb) of a module with the head's structure, else None"""
    ppm, conv6 = getattr(m, "ppm", None), getattr(m, "conv6", None)
    if not isinstance(m, nn.Module) or not isinstance(ppm, nn.ModuleList) or not isinstance(conv6, nn.Sequential):
        return None
    if not 1 <= len(ppm) <= MAX_BRANCHES or len(conv6) < 1:
        return None
    branches = [_branch(seq) for seq in ppm]
    if any(b is None for b in branches):
        return None
    C, Cb = branches[0][1].conv.in_channels, branches[0][1].conv.out_channels
    if Cb % 16 or any(cbr.conv.in_channels != C or cbr.conv.out_channels != Cb for _, cbr in branches):
        return None
    head = conv6[0]
    if not _cbr_layers(head) or head.conv.in_channels != C + len(branches) * Cb or C % 16:    # a plain 3x3 + BatchNorm, unhooked
        return None
    if not _no_hooks(m, conv6, *[k for seq in ppm for k in seq.modules()]):
        return None
    return branches, head, C, Cb


def _pool_shape(pool, H, W):
    """the map an nn.AdaptiveAvgPool2d gives on an H x W input"""
    size = pool.output_size
    sh, sw = (size, size) if not isinstance(size, (tuple, list)) else size
    return (H if sh is None else int(sh)), (W if sw is None else int(sw))


class _PpmPack(tuple):
    """(wf, ab) of kernels.conv3x3_bnact_pack for W6[:, :C], with the branch slices `wb` [n, 9, Cout, Cb] as an attribute"""


class _FusedPyramid:
    """Mixed in front of a pyramid-pooling-shaped module's own class."""

    tsg_ppm_fused_calls = 0             # forwards that took the three launches of csrc/ppmbn.hip

    _cbn_pack = _FusedConvBn._cbn_pack
    _cbn_drop = _FusedConvBn._cbn_drop
    _cbn_gate = _FusedConvBn._cbn_gate

    def _ppm_ready(self, x):
        """(branches, head, maps, pack) when this call can take the fused chain; everything that can be known before the
        branches run is decided here"""
        found = _pyramid(self)
        if found is None:
            return None
        branches, head, C, Cb = found
        conv, bn = head.conv, head.bn
        if bn.training or head.training:
            self._cbn_drop()
            return None
        if (not bn.track_running_stats or bn.running_mean is None or bn.running_var is None
                or conv.weight.dtype != torch.float32 or x.shape[1] != C):
            return None
        B, _, H, W = x.shape
        maps = [_pool_shape(pool, H, W) for pool, _ in branches]
        kp = K.provider()
        if not kp.ppm_supported(x, maps, Cb, conv.out_channels):
            return None
        n = len(branches)

        def build(kp, conv, fp):
            pack = _PpmPack(kp.conv3x3_bnact_pack(conv.weight[:, :C], conv.bias, fp))
            pack.wb = kp.ppm_pack_branches(conv.weight, C, n)
            return pack

        pack = self._cbn_pack("conv6", conv, bn, x, build=build)
        return None if pack is None else (branches, head, maps, pack)

    def forward(self, x):
        if not self._cbn_gate(x):
            return super().forward(x)
        ready = self._ppm_ready(x)
        if ready is None:
            return super().forward(x)
        branches, head, maps, pack = ready
        B, Cb = x.shape[0], branches[0][1].conv.out_channels
        pooled = []
        for seq, (sh, sw) in zip(self.ppm, maps):                 # the branches, as their modules run today
            p = seq(x)
            if not (isinstance(p, torch.Tensor) and p.dtype == torch.bfloat16 and tuple(p.shape) == (B, Cb, sh, sw)
                    and p.device == x.device):
                return super().forward(x)                         # eval mode: no state moved, the stock method forms them again
            p = p.contiguous(memory_format=torch.channels_last)
            pooled.append(p if p.data_ptr() % 16 == 0 else p.clone(memory_format=torch.channels_last))
        kp = K.provider()
        Cout = head.conv.out_channels
        with torch._C.DisableTorchFunction():
            T, E = kp.ppm_workspace(x, maps, Cb, Cout)
            kp.ppm_taps_fwd(pooled, pack.wb, T)
            kp.ppm_addend_fwd(T, maps, E)
            y = kp.conv3x3_bnact_add_fwd(x, pack, Cout, E, getattr(head, "has_relu", False))
        self.tsg_ppm_fused_calls += 1
        for m in list(self.conv6)[1:]:
            y = m(y)
        return y


_CLASSES = {}


def _fused_class(cls):
    sub = _CLASSES.get(cls)
    if sub is None:
        sub = _CLASSES[cls] = type("FusedPyramid" + cls.__name__, (_FusedPyramid, cls), {"__module__": __name__})
    return sub


def eligible(m):
    """whether `m` has the head's structure (see the module docstring)"""
    return _pyramid(m) is not None


def install_fused_pyramid(module):
    """Re-class, in place, every pyramid-pooling-shaped module of `module`; returns how many heads this call re-classed."""
    n = 0
    for m in module.modules():
        if not isinstance(m, _FusedPyramid) and eligible(m):
            m.__class__ = _fused_class(type(m))
            n += 1
    return n


def pyramid_fused_calls(module):
    """how many forwards of the heads below `module` took the fused chain so far"""
    return sum(m.tsg_ppm_fused_calls for m in module.modules() if isinstance(m, _FusedPyramid))
