"""Inference wrapper: a trained network on our kernels for evaluation and timing.

`prepare_inference(network)` returns a module with the network's call signature, in eval mode and without gradients:
  - nn.BatchNorm2d layers become our SyncBatchNorm (eval mode: the running-statistics apply path);
  - the layers are re-classed onto our kernels exactly as the DDP wrapper does it (ddp.install_kernels);
  - forward runs under bf16 autocast (TSG_DTYPE=fp32: the fp32 parity mode, exact convolutions) and FuseMode with
    `infer=True`: under no_grad the head's `F.interpolate(logits, bilinear, align_corners=True)` and the
    `F.log_softmax(., dim=1)` after it stay pending (fusion.DeferredLogSoftmax(tail=True)).  The Evaluator consumes that
    value without materialising it (tsg_seg_tail_accum); any other use materialises it through tsg_seg_tail_logprob, so
    the value is what the network returns;
  - graph=True: the forward is captured once per input shape and dtype (one hipGraph on the capturing stream, no side
    streams: TSG_FORK_MODULES is not applied here) and replayed from a static input buffer.  The returned tensor is that
    graph's static output: it is overwritten by the next call with the same shape;
  - fuse_separable=True (default: TSG_SEPCONV_FUSED, 0): Xception's separable units run as one launch each
    (torchseg_amd.sepconv.install_fused_separable, after the kernel install; csrc/sepconv.hip).  Opt-in;
  - fuse_convbn=True (default: TSG_CONVBN_FUSED, 0): the stride-1 3x3 convolutions of the ResNet blocks and ConvBnRelu layers
    run with their BatchNorm, shortcut and ReLU as one launch each (torchseg_amd.convbn.install_fused_convbn, after the
    kernel install; csrc/convbn.hip).  Opt-in;
  - fuse_dilated=True (default: TSG_DILBN_FUSED, 0): the dilated (2, 4) 3x3 convolutions of the PSPNet / PSANet backbones'
    layer3 / layer4 Bottlenecks run with their BatchNorm and ReLU as one launch each
    (torchseg_amd.convbn.install_fused_convbn(dilated=True, plain=False), after fuse_convbn's install and before
    fuse_pointwise's, on the modules not yet re-classed; csrc/dilbn.hip; the count is `fused_dilated`).  Works with
    fuse_convbn off: only blocks with a dilated 3x3 are re-classed then.  Opt-in: profiles/dilbn_infer_bench.txt;
  - fuse_strided=True (default: TSG_S2BN_FUSED, 0): the stride-2 3x3 convolutions (BasicBlock.conv1 / Bottleneck.conv2 of
    the first block of layer2 / 3 / 4, the detail branch's conv_3x3_1 / conv_3x3_2) run with their BatchNorm and ReLU as one
    launch each (torchseg_amd.convbn.install_fused_convbn(strided=True, plain=False), after fuse_dilated's install and
    before fuse_pointwise's: modules not yet re-classed that hold such a layer are re-classed, modules fuse_convbn
    re-classed are upgraded; csrc/s2bn.hip; `fused_strided` is the number of stride-2 LAYERS taken: 5 for BiSeNet-R18 with
    or without fuse_convbn, 3 for ResNet-50, 1 for PSPNet-R50).  With it our SpatialPath runs its ConvBnRelu modules one
    after the other (seg_oprs.cbr_chain), so its conv_1x1 goes through its module and is fused by fuse_pointwise.
    Opt-in: profiles/s2bn_infer_bench.txt;
  - fuse_pointwise=True (default: TSG_PWBN_FUSED, 0): the 1x1 convolutions of the Bottlenecks, the 1x1 shortcuts and the 1x1
    ConvBnRelu layers run with their BatchNorm, shortcut and ReLU as one launch each
    (torchseg_amd.pwbn.install_fused_pointwise, after convbn's install; csrc/pwbn.hip).  Opt-in;
  - fuse_stem=True (default: TSG_STEMBN_FUSED, 0): the 7x7 image stem of a ConvBnRelu (SpatialPath.conv_7x7) and the three
    3x3 layers of a v1c deep stem of width 64 (ResNet._stem of FCN / PSPNet / PSANet / DFN / BiSeNet-R101) run with their
    BatchNorm and ReLU as one launch each (torchseg_amd.stembn.install_fused_stem, after the four installs above;
    stem_bnact_fwd_k in csrc/stemconv.hip, ds_bnact_fwd_k in csrc/deepstem.hip, and csrc/convbn.hip's kernel for the two
    inner layers; `fused_stem` is the number of LAYERS taken: 1 for BiSeNet-R18, 3 for PSPNet / PSANet / FCN, 0 for a plain
    ResNet-50).  The filters of the image layers are packed once, not per call.  With every switch on, a deep-stem
    backbone runs no convolution outside our kernels.  Opt-in: profiles/stembn_infer_bench.txt;
  - fuse_pyramid=True (default: TSG_PPMBN_FUSED, 0): PSPNet's pyramid pooling head runs without its four up-samplings and
    its concatenation (torchseg_amd.ppmbn.install_fused_pyramid, after the five installs above; csrc/ppmbn.hip): the pooled
    channels' share of `conv6[0]` is contracted on the pooled maps (tsg_ppm_taps_fwd, tsg_ppm_addend_fwd) and the full-map
    3x3 convolution reads x alone, with that share added in its epilogue (tsg_conv3x3_bnact_add_fwd).  `fused_pyramid` is
    the number of HEADS taken: 1 for PSPNet, 0 for BiSeNet, PSANet and FCN.  The pools, the branch convolutions and the
    classifier run as before.  Opt-in: profiles/ppmbn_infer_bench.txt.
The `+=` / interpolate pre-sum and the ConvBnRelu chain fusions stay gated on autograd as in training (not enabled here).
"""
import contextlib
import os

import torch
import torch.nn as nn


def _compute_dtype(dtype):
    if dtype is not None:
        return dtype
    name = os.environ.get("TSG_DTYPE", "bf16").lower()
    return {"bf16": torch.bfloat16, "bfloat16": torch.bfloat16, "fp32": torch.float32, "float32": torch.float32}[name]


class InferenceModule(nn.Module):
    def __init__(self, network, dtype=None, channels_last=None, graph=False, fuse_separable=None, fuse_convbn=None,
                 fuse_pointwise=None, fuse_dilated=None, fuse_strided=None, fuse_stem=None, fuse_pyramid=None):
        super().__init__()
        from . import ddp
        from .syncbn import convert_syncbn_model
        first = next(network.parameters(), None)
        if first is None or not first.is_cuda:
            raise RuntimeError("prepare_inference: move the network to the GPU first (there is no CPU path)")
        network = convert_syncbn_model(network)
        network.eval()
        for p in network.parameters():
            p.requires_grad_(False)
        self.module = network
        self.compute_dtype = _compute_dtype(dtype)
        if channels_last is None:
            channels_last = ddp._env_flag("TSG_CHANNELS_LAST", True)
        self.channels_last = bool(channels_last)
        if self.channels_last:
            ddp.apply_channels_last(self.module)
            from . import syncbn
            syncbn.PREFER_CHANNELS_LAST_OUTPUT = True
        from .upsample import install_aten_overrides
        install_aten_overrides()
        ddp.install_kernels(self.module, self.compute_dtype)
        if fuse_separable is None:
            fuse_separable = ddp._env_flag("TSG_SEPCONV_FUSED", False)
        self.fused_separable = 0
        if fuse_separable:
            from .sepconv import install_fused_separable
            self.fused_separable = install_fused_separable(self.module)
        if fuse_convbn is None:
            fuse_convbn = ddp._env_flag("TSG_CONVBN_FUSED", False)
        self.fused_convbn = 0
        if fuse_convbn:
            from .convbn import install_fused_convbn
            self.fused_convbn = install_fused_convbn(self.module)
        if fuse_dilated is None:
            fuse_dilated = ddp._env_flag("TSG_DILBN_FUSED", False)
        self.fused_dilated = 0
        if fuse_dilated:                         # only the modules with a dilated 3x3 that are not re-classed yet
            from .convbn import install_fused_convbn
            self.fused_dilated = install_fused_convbn(self.module, dilated=True, plain=False)
        if fuse_strided is None:
            fuse_strided = ddp._env_flag("TSG_S2BN_FUSED", False)
        self.fused_strided = 0
        if fuse_strided:                         # the stride-2 LAYERS: of modules re-classed above (upgraded) and of new ones
            from .convbn import eligible_strided_layers, install_fused_convbn
            install_fused_convbn(self.module, strided=True, plain=False)
            self.fused_strided = sum(len(eligible_strided_layers(m)) for m in self.module.modules()
                                     if getattr(m, "tsg_cbn_strided", False))
        if fuse_pointwise is None:
            fuse_pointwise = ddp._env_flag("TSG_PWBN_FUSED", False)
        self.fused_pointwise = 0
        if fuse_pointwise:
            from .pwbn import install_fused_pointwise
            self.fused_pointwise = install_fused_pointwise(self.module)
        if fuse_stem is None:
            fuse_stem = ddp._env_flag("TSG_STEMBN_FUSED", False)
        self.fused_stem = 0
        if fuse_stem:                            # the image stems and the deep stem: modules none of the above re-classes
            from .stembn import install_fused_stem
            self.fused_stem = install_fused_stem(self.module)
        if fuse_pyramid is None:
            fuse_pyramid = ddp._env_flag("TSG_PPMBN_FUSED", False)
        self.fused_pyramid = 0
        if fuse_pyramid:                         # the pyramid pooling head: a module none of the above re-classes
            from .ppmbn import install_fused_pyramid
            self.fused_pyramid = install_fused_pyramid(self.module)
        self.graph = bool(graph)
        self._graphs = {}

    def train(self, mode=True):
        return super().train(False)              # an inference module stays in eval mode

    def _eager(self, *inputs, **kwargs):
        from .fusion import FuseMode
        with contextlib.ExitStack() as stack:
            stack.enter_context(torch.no_grad())
            if self.compute_dtype != torch.float32:
                stack.enter_context(torch.autocast("cuda", dtype=self.compute_dtype))
            stack.enter_context(FuseMode(loss=False, add_up=False, head=False, chain=False, infer=True))
            return self.module(*inputs, **kwargs)

    def forward(self, *inputs, **kwargs):
        if not self.graph or kwargs or len(inputs) != 1 or not isinstance(inputs[0], torch.Tensor):
            return self._eager(*inputs, **kwargs)
        from .fusion import materialize
        x = inputs[0]
        key = (tuple(x.shape), x.dtype, x.device)
        entry = self._graphs.get(key)
        if entry is None:
            static_in = x.clone()
            with torch.no_grad():
                materialize(self._eager(static_in))          # warm-up: allocations, lazy installs, kernel selection
            torch.cuda.current_stream().synchronize()
            # the image's bf16 cast belongs to the capture: the stems' cast cache (stemconv._as_bf16_image) still holds the
            # warm-up's copy of static_in at this version, and a hit would leave the cast out of the graph — every replay
            # would then read the image of the first call, from memory the graph does not own
            from . import stemconv
            stemconv._cast_cache[0] = None
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                static_out = materialize(self._eager(static_in))
            entry = self._graphs[key] = (g, static_in, static_out)
        g, static_in, static_out = entry
        static_in.copy_(x)
        g.replay()
        return static_out


def prepare_inference(network, dtype=None, channels_last=None, graph=False, fuse_separable=None, fuse_convbn=None,
                      fuse_pointwise=None, fuse_dilated=None, fuse_strided=None, fuse_stem=None, fuse_pyramid=None):
    """See the module docstring.  `dtype`: torch.bfloat16 or torch.float32 (default: TSG_DTYPE, bf16)."""
    if isinstance(network, InferenceModule):
        return network
    return InferenceModule(network, dtype=dtype, channels_last=channels_last, graph=graph, fuse_separable=fuse_separable,
                           fuse_convbn=fuse_convbn, fuse_pointwise=fuse_pointwise, fuse_dilated=fuse_dilated,
                           fuse_strided=fuse_strided, fuse_stem=fuse_stem, fuse_pyramid=fuse_pyramid)


def pending_tail(out):
    """(z, (H, W)) when `out` is the pending log_softmax of an up-sampled head, else None."""
    from .fusion import DeferredLogSoftmax
    if isinstance(out, DeferredLogSoftmax) and out.tail and out._value is None:
        return out.x.z.contiguous(), out.x.out_hw
    return None
