"""Host side of the 3x3 convolutions (padding 1, stride 1 / 2, C_in and C_out multiples of 64) of the ResNets and heads.

  * `install_conv_wrw` re-classes the eligible `nn.Conv2d` to `WrwConv2d`; `_route` decides, per call, which kernel family
    serves a layer: conv64 (csrc/conv64.hip), the general kernel (csrc/conv3g.hip), the vendor library's forward with the
    stride-2 parity data gradient, or the vendor library for both.  The weight gradient is `tsg_conv3x3_wrw` in every case.
  * The autograd nodes: `_ConvWrwFn`, `_ConvGenFn`, and the fused BatchNorm -> ReLU -> convolution nodes `_BnReluConvFn`
    (`bn_relu_conv`) and `_StemBnReluConvFn` (`stem_bn_relu_conv`); `conv_with_skip` routes a residual block's skip
    connection through the convolution's node so that its gradient is an epilogue addend of the data-gradient kernel.
  * `wrw_on_side_stream`: the weight gradients run on a side HIP stream, joined at the end of the backward pass, or — while
    `_DEFER` is a list — are only listed, for a caller that replays them as a graph of its own.

On by default under the DDP wrapper (bf16, channels_last); TSG_CONV_WRW=0 leaves every layer to the vendor library.  Every
switch below is consulted per call (tests and bench.py flip them at run time).  The measurements behind the defaults:
DESIGN.md section 4.3 and appendix A."""
import collections
import os as _os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import kernels as K
from . import syncbn as S
from .stemconv import StemConv2d, _as_bf16_image, _wants_bf16, attach_bn_partial, take_bn_partial

# ---- which kernel family serves a layer (read by _route only) ----
# TSG_CONV_C64=1|0 (default 1): forward and data gradient of the 64 -> 64 layers, stride 1 and 2, on tsg_conv3x3_c64_*
# (104 us against 172 us for the library's kernel at [16, 64, 256, 256], tools/bench_conv64.py)
_OWN_C64 = _os.environ.get("TSG_CONV_C64", "1") != "0"
# TSG_CONV_C64_S1=1|0 (default 1): 0 sends the STRIDE-1 64 -> 64 layers (ResNet layer1) to the general kernel (3.8
# non-MFMA instructions per MFMA against conv64's 8.9) and keeps conv64 for the stride-2 layers of the spatial path
# (profiles/r04_ab_conv64_vs_conv3g.txt)
_OWN_C64_S1 = _os.environ.get("TSG_CONV_C64_S1", "1") != "0"
# TSG_CONV_C64_STATS=1|0 (default 1): the BatchNorm statistics of a conv64 output in that kernel's epilogue: the
# SyncBatchNorm behind each of the six 64 -> 64 layers (layer1 x 4 at 16 x 64 x 256^2, SpatialPath x 2) skips its own pass
# over 134 / 34 MB (profiles/r04_conv64_stats_epilogue.txt)
_C64_STATS = _os.environ.get("TSG_CONV_C64_STATS", "1") != "0"
# TSG_CONV_GEN=1|0 (default 1): forward and data gradient of every other stride-1 layer on tsg_conv3x3_gen_fwd instead of
# the vendor library; TSG_CONV_GEN_STATS=1|0 (default 1): the BatchNorm statistics of the output in its epilogue (every
# one of these convolutions feeds a SyncBatchNorm)
_OWN_GEN = _os.environ.get("TSG_CONV_GEN", "1") != "0"
_GEN_STATS = _os.environ.get("TSG_CONV_GEN_STATS", "1") != "0"
# TSG_CONV_S2_DGRAD=1|0 (default 1): data gradient of the stride-2 layers other than 64 -> 64 (ResNet layer2-4's first
# convolution) by output parity on tsg_conv3x3_s2_dgrad, with the shortcut branch's gradient as its epilogue addend
# (profiles/r04_s2_dgrad.txt)
_OWN_S2_DGRAD = _os.environ.get("TSG_CONV_S2_DGRAD", "1") != "0"
# TSG_CONV_DGRAD_FWD=0|1|2 (default 2): where the vendor library computes a stride-1 data gradient, it does so as a
# FORWARD convolution with the rotated / transposed filter: for the C_in == C_out layers (1) or for every layer (2; the
# forward shapes this creates are in the shipped MIOpen find-db).  Same box: 0 -> 807, 1 -> 827 img/s; on the re-tuned db
# 1 -> 839, 2 -> 845
_DGRAD_MODE = _os.environ.get("TSG_CONV_DGRAD_FWD", "2").strip().lower()
_DGRAD_FWD = _DGRAD_MODE not in ("0", "false", "no", "off", "")
_DGRAD_ANY = _DGRAD_MODE == "2"

# ---- fusions around the convolution ----
# TSG_BN_ON_LOAD=1|0 (default 1): BatchNorm + ReLU in front of a 64 -> 64 convolution applied while that convolution (and
# its weight gradient) load their input, instead of as a pass of its own (bn_relu_conv)
_BN_ON_LOAD = _os.environ.get("TSG_BN_ON_LOAD", "1") != "0"
# TSG_CONV_GEN_BN_ON_LOAD=0|1 (default 0): the same in front of a general-kernel layer.  Bit-equal to the separate pass
# (tests/test_bnconv_gpu.py) and it never writes the normalised activation, but slower in the step (1103 against 1116
# img/s; 12.38 against 12.17 ms under the segmented replay): the 6 BatchNorm passes it removes (layer2-4's
# bn1: ~0.1 ms) cost less than the transform adds to the staging code of 12 convolution / weight-gradient launches
_GEN_BN_ON_LOAD = _os.environ.get("TSG_CONV_GEN_BN_ON_LOAD", "0") == "1"
# TSG_STEM_BN_WRW=1|0 (default 1): stem -> BN -> ReLU -> 64 -> 64 convolution as one autograd node (_StemBnReluConvFn)
_STEM_BN_WRW = _os.environ.get("TSG_STEM_BN_WRW", "1") != "0"
# TSG_BN_BSUM=1|0 (default 0): the backward sums of a BatchNorm -> ReLU in the epilogue of the data gradient of the 64 -> 64
# convolution behind it (tsg_conv3x3_c64_*dgrad_bnsums) instead of a pass of their own over the gradient and the
# BatchNorm's input (tsg_bn_bwd_reduce).  Same values up to the order of the fp32 sums, but slower in every geometry (144
# against 78 + 42 us, profiles/r06_bn_bsum_in_dgrad_epilogue.txt), hence opt-in
_BN_BSUM = _os.environ.get("TSG_BN_BSUM", "0") == "1"
# TSG_FUSE_SKIP_GRAD=1|0 (default 1): in a residual block whose skip connection is the block input itself (resnet.py:
# 48-52), the gradient of the skip path is added in the epilogue of conv1's data-gradient kernel (conv_with_skip)
_FUSE_SKIP = _os.environ.get("TSG_FUSE_SKIP_GRAD", "1") != "0"
# TSG_SKIP_SUBSAMPLE=1|0 (default 1): a stride-2 block hands its shortcut convolution x[:, :, ::2, ::2] as a compact tensor
# (conv_with_skip(subsample=True)) instead of x (profiles/r06_shortcut_on_subsampled_map.txt)
_SKIP_SUB = _os.environ.get("TSG_SKIP_SUBSAMPLE", "1") != "0"
# TSG_WEIGHT_SHADOW=1|0 (default 1): bf16 / rotated / fragment-order filters from torchseg_amd.shadow, refreshed by one
# launch per optimizer step instead of ~57 cast / rotate / preparation launches.  Neutral for the GPU when it was measured
# for the ~45 casts alone (1032.5 against 1035.5 img/s, DESIGN.md A.2: such launches sit back to back in the queue); it is
# the host and the replayed graph that have fewer launches to issue
_SHADOW = _os.environ.get("TSG_WEIGHT_SHADOW", "1") != "0"

# ---- where the weight gradients run ----
# TSG_WRW_STREAM=1|0: the 3x3 weight gradients on a side HIP stream.  A layer's weight gradient is needed by nobody until
# the optimizer step, while everything else in the backward pass waits for the DATA gradient; issued on the compute stream
# it sits in the dependent chain all the same.  On a side stream its matrix-core work (25 launches, 2.7 ms of the step,
# MFMA pipe busy 0.41) runs beside the HBM-bound SyncBatchNorm backward passes of the layers in front of it (2.3 ms that
# leave the matrix pipes idle).  The operands are kept alive for the side stream (record_stream), the result belongs to
# the compute stream, and the end of the backward pass (an autograd engine callback) makes the compute stream wait for
# the side stream, so the optimizer, the DDP buckets' gather and anything after .backward() see finished gradients.
#
# Default: on in a process WITHOUT gradient collectives, off once a DDP reducer exists (N > 1, or TSG_FORCE_COLLECTIVES=1);
# TSG_WRW_STREAM=1 forces it on there too.  The HIP runtime multiplexes a process's streams onto 4 hardware queues, least
# used first; with RCCL's and the process group's streams in the process the side stream lands on the compute stream's OWN
# hardware queue (rocprofv3 kernel trace: Queue_Id 1 for both), where two streams run strictly in order and every
# cross-stream event is a bubble: zero overlap and 1 091 img/s on the N > 1 code path of one rank, against 1 175 without
# the side stream and 1 173 with GPU_MAX_HW_QUEUES=8 — i.e. no gain left to defend there
# (profiles/r05_side_stream_hw_queue.txt).
_WRW_ENV = _os.environ.get("TSG_WRW_STREAM")
_WRW_STREAM = _WRW_ENV != "0"
# TSG_WRW_IN_GRAPH=1|0 (default 0): under hipGraph capture the side stream can be kept — its fork (side waits for the
# capturing stream) and its join (the end-of-backward callback) become EDGES of the captured graph.  Interleaved on one box
# (profiles/r06_graph_ab.txt): a single-stream graph of the step 1 198 / 1 203 img/s (host 0.15-0.2 ms per step), the same
# graph with the 27 weight-gradient forks inside it 1 168 / 1 166 (host 7.2 ms: hipGraphLaunch walks a branching graph node
# by node), eager with the side stream 1 196 / 1 202 (host 12.2-13.2 ms).  A linear graph replays as fast as the eager step
# overlaps, without the host; so the captured step stays on one stream.
_WRW_IN_GRAPH = _os.environ.get("TSG_WRW_IN_GRAPH", "0") == "1"
# A list while a caller wants the 3x3 weight gradients LAUNCHED LATER (bench.SegmentedStep: captured into a graph of their
# own that replays on another stream beside the rest of the backward pass): wrw_on_side_stream then hands autograd the
# (still unwritten) result tensor and appends (launch, operands, buffer) to the list — for a parameter whose gradient
# nothing reads before the list runs (may_defer below); any other weight gradient is computed in place and is not listed.
# The caller runs the list and keeps it alive as long as the operands are read.
_DEFER = None


def side_stream_off_for_collectives():
    """ddp.DistributedDataParallel calls this when it builds a reducer (see TSG_WRW_STREAM above); an explicit
    TSG_WRW_STREAM wins."""
    global _WRW_STREAM
    if _WRW_ENV is None:
        _WRW_STREAM = False


_wrw_side = {}
_wrw_join_queued = [False]
_wrw_pending = set()                   # id(param) of every parameter whose gradient of THIS backward pass is on the side stream
_OWN_GRAD_HOOKS = set()                # post-accumulate-grad hooks that join the side stream themselves (ddp.Reducer._on_grad)


def allow_grad_hook(fn):
    """Register a post-accumulate-grad hook (by its function object) as one that calls join_wrw_stream() before it reads
    p.grad: the DDP reducer's.  Any OTHER such hook on a parameter (an optimizer-in-backward step) keeps that parameter's
    weight gradient on the compute stream."""
    _OWN_GRAD_HOOKS.add(getattr(fn, "__func__", fn))


def _foreign_grad_hooks(param):
    hooks = getattr(param, "_post_accumulate_grad_hooks", None)
    if not hooks:
        return False
    return any(getattr(h, "__func__", h) not in _OWN_GRAD_HOOKS for h in hooks.values())


def join_wrw_stream():
    """Make the current stream wait for weight gradients still running on the side stream (the engine callback does this
    at the end of every backward pass; the DDP reducer calls it before it gathers a bucket early, FusedSGD before it
    reads the gradients, the DDP wrapper at the start of the next forward — which also re-arms the callback should a
    backward pass have died between queueing and running it)."""
    for dev, side in _wrw_side.items():
        torch.cuda.current_stream(dev).wait_stream(side)


def _wrw_join():
    _wrw_join_queued[0] = False
    _wrw_pending.clear()
    join_wrw_stream()


def _kept_as_gradient(out, param):
    """autograd's layout contract for a first gradient (torch/csrc/autograd/functions/accumulate_grad.h): the strides of
    the parameter on every dimension longer than 1."""
    if out.shape != param.shape or out.dtype != param.dtype:
        return False
    return all(a == b for a, b, n in zip(out.stride(), param.stride(), out.shape) if n != 1)


_deferred = {}                         # id(param) -> its entry in _DEFER (None once launched) for THIS backward pass
_deferred_clear_queued = [False]


def _deferred_clear():
    _deferred_clear_queued[0] = False
    _deferred.clear()


def may_defer(param, buf):
    """May the weight gradient of `param` be handed to autograd UNWRITTEN (`buf`), its launch only listed in _DEFER?  Only
    where nothing reads the tensor before the caller runs the list: AccumulateGrad must keep it as it is (a leaf without a
    gradient, of the buffer's dtype and layout; with a gradient there it would add the unwritten buffer at once), no cast
    and no hook may touch it, and the parameter must not have another result in this backward pass (the engine would sum
    the two) — the conditions of the side stream above."""
    return (param is not None and param.is_leaf and param.grad is None and param.dtype == torch.float32
            and id(param) not in _wrw_pending and id(param) not in _deferred and not param._backward_hooks
            and not _foreign_grad_hooks(param) and _kept_as_gradient(buf, param))


def note_deferred(param, entry):
    """List `entry` = (launch, operands, buffer) in _DEFER as the pending weight gradient of `param`."""
    _DEFER.append(entry)
    _deferred[id(param)] = entry
    if not _deferred_clear_queued[0]:
        _deferred_clear_queued[0] = True
        from torch.autograd import Variable
        try:
            Variable._execution_engine.queue_callback(_deferred_clear)
        except RuntimeError:                           # not inside a backward pass
            _deferred_clear()


def launch_deferred_of(param):
    """A second use of a parameter whose first weight gradient of this backward pass was deferred: the engine is about to
    sum the two, so the listed launch runs now (and leaves the list).  True when `param` had one: the caller then computes
    in place as well."""
    if param is None or id(param) not in _deferred:
        return False
    entry, _deferred[id(param)] = _deferred[id(param)], None
    if entry is not None:
        if _DEFER is not None:
            _DEFER[:] = [e for e in _DEFER if e is not entry]
        entry[0]()
    return True


def wrw_on_side_stream(fn, param, *operands, defer_out=None):
    """`fn()` (launches a weight-gradient kernel, returns its result tensor) on the side stream of the operands' device.
    `param`: the parameter the result is the gradient of.  Only a parameter WITHOUT a gradient takes the side stream:
    autograd's AccumulateGrad then just keeps the tensor; with a gradient already there (accumulation over several backward
    passes, zero_grad(set_to_none=False)) it runs `grad += result` on the compute stream right after this node returns,
    which would read the result under the running kernel.  The same holds for a parameter used TWICE in one backward pass
    (shared weights; `loss = net(x1) + net(x2)`): both uses see `grad is None` at node time, and the engine sums the two
    results on the compute stream — so a parameter that already has a side-stream result in this pass (`_wrw_pending`,
    cleared by the end-of-backward join) makes the compute stream wait for the side stream and computes the second one
    there.  A post-accumulate-grad hook that is not the DDP reducer's would read p.grad before the join."""
    if _DEFER is not None and defer_out is not None:
        Cout, Cin = defer_out
        buf = torch.empty((Cout, Cin, 3, 3), dtype=torch.float32, device=operands[0].device, memory_format=torch.channels_last)
        if may_defer(param, buf):
            note_deferred(param, (lambda: fn(out=buf), operands, buf))
            # an ALIAS of its own: AccumulateGrad keeps an incoming gradient only when nobody else holds that tensor object,
            # and clones it otherwise — the copy would be taken here, before the deferred launch has written anything
            return buf.detach()
        if launch_deferred_of(param):                  # (anything else reads the result at once: it is computed in place)
            return fn()
    if not _WRW_STREAM or not operands[0].is_cuda or param is None or not param.is_leaf or param.grad is not None \
            or param.dtype != torch.float32 or param._backward_hooks or _foreign_grad_hooks(param) \
            or (torch.cuda.is_current_stream_capturing() and not _WRW_IN_GRAPH):
        if _wrw_side and operands[0].is_cuda:
            # anything computed here may be summed with (or share scratch state with) a result still on the side stream
            dev = operands[0].device
            side = _wrw_side.get(dev)
            if side is not None and (param is None or id(param) in _wrw_pending):
                torch.cuda.current_stream(dev).wait_stream(side)
        return fn()                                    # (a non-leaf, a cast or a tensor hook would touch the result at once)
    dev = operands[0].device
    cur = torch.cuda.current_stream(dev)
    if id(param) in _wrw_pending:                      # second use of the parameter in this backward pass: see above
        side = _wrw_side.get(dev)
        if side is not None:
            cur.wait_stream(side)
        return fn()
    side = _wrw_side.get(dev)
    if side is None:
        side = _wrw_side[dev] = torch.cuda.Stream(device=dev)
    side.wait_stream(cur)                              # the operands (dy above all) are complete
    with torch.cuda.stream(side):
        out = fn()
    for t in operands:
        if t is not None:
            t.record_stream(side)                      # their memory must not be handed out again under the running kernel
    out.record_stream(cur)
    _wrw_pending.add(id(param))
    if not _kept_as_gradient(out, param):
        # AccumulateGrad keeps a first gradient as it is only when it has the parameter's layout; otherwise it copies it
        # into that layout on the compute stream, at once: the copy must see the finished kernel
        cur.wait_stream(side)
    if not _wrw_join_queued[0]:
        _wrw_join_queued[0] = True
        from torch.autograd import Variable
        try:
            Variable._execution_engine.queue_callback(_wrw_join)
        except RuntimeError:                           # not inside a backward pass (a test calling the function directly)
            _wrw_join()
    return out


def _conv_wrw(x, dy, stride, param, in_ab=None):
    """The weight gradient of a 3x3 layer from its input and output gradient (`in_ab`: x is the input of the BatchNorm +
    ReLU in front of the layer, applied on load), wherever wrw_on_side_stream — looked up per call: tests replace it —
    runs it."""
    operands = (x, dy) if in_ab is None else (x, dy, in_ab)
    return wrw_on_side_stream(lambda out=None: K.provider().conv3x3_wrw(x, dy, stride=stride, in_ab=in_ab, out=out), param,
                              *operands, defer_out=(dy.shape[1], x.shape[1]))


def _bf16_nhwc(t):
    """t as the kernels here take an activation: bf16, channels_last (t itself when it already is)."""
    if t.dtype != torch.bfloat16:
        t = t.to(torch.bfloat16)
    return t.contiguous(memory_format=torch.channels_last)


def _filters(weight):
    """(bf16 filter, its rotated / transposed image or None) of an fp32 master weight: kept fresh once per step by the
    shadow bank, or cast here (the rotation then happens where a data gradient asks for it, _rotated)."""
    if _SHADOW and weight.is_contiguous(memory_format=torch.channels_last):
        from .shadow import bank
        return bank.get(weight, want_rot=True)
    return weight.detach().to(torch.bfloat16), None


def _rotated(wrt, wb):
    return wrt if wrt is not None else K.provider().conv3x3_weight_rot180_t(wb)


def _with_partial(y, partial):
    """y, with the statistics its producer collected left on it: the SyncBatchNorm behind it skips its statistics pass."""
    if partial.numel():
        attach_bn_partial(y, partial)
    return y


def _skip_addend(dskip, like_shape):
    """The gradient of a skip connection as an epilogue addend of the data-gradient kernel (bf16, channels_last,
    the shape of dx), or None when it cannot be one."""
    if dskip is None or tuple(dskip.shape) != tuple(like_shape):
        return None
    return _bf16_nhwc(dskip)


# What _route decides for one layer and one call:
#   family      "c64": forward and data gradient on conv64 | "gen": both on the general kernel | "s2": the library's forward,
#               data gradient by output parity on tsg_conv3x3_s2_dgrad | "lib": the library for both
#   stats       the BatchNorm statistics of the output come from the forward kernel's epilogue
#   skip        conv_with_skip routes the block input through the node (the family's data gradient takes the skip
#               gradient as an epilogue addend)
#   compact     ... and may hand out the sub-sampled alias x[:, :, ::2, ::2] instead, when the caller asks for it
#   bn_on_load  bn_relu_conv may apply the BatchNorm + ReLU in front of the layer while the layer loads its input
#   dgrad_fwd   family "lib": the data gradient is spelt as a forward convolution (TSG_CONV_DGRAD_FWD)
Route = collections.namedtuple("Route", "family stats skip compact bn_on_load dgrad_fwd")


def _route(conv, xb, general=True):
    """The Route of `conv` (a WrwConv2d) for the bf16 channels_last input `xb`, or None when the layer is not ours (then
    nn.Conv2d.forward runs it).  Only the dtype, layout and channel count of xb are looked at.  general=False: the caller
    has no general-kernel form (the stem node)."""
    kp = K.provider()
    stride, geom = conv.stride[0], (conv.padding[0], conv.dilation[0], conv.groups)
    if not kp.conv3x3_wrw_supported(xb, conv.weight, stride, *geom):
        return None
    nhwc = conv.weight.is_contiguous(memory_format=torch.channels_last)
    c64 = _OWN_C64 and kp.conv3x3_c64_supported(xb, conv.weight, stride, *geom)           # 64 -> 64
    if (general and _OWN_GEN and stride == 1 and not (c64 and _OWN_C64_S1) and nhwc
            and kp.conv3x3_gen_supported(xb, conv.weight, 1, *geom)):
        family, stats, skip = "gen", _GEN_STATS, True
    else:
        if c64 and nhwc:
            family = "c64"
        elif _OWN_S2_DGRAD and stride == 2 and nhwc and kp.conv3x3_s2_dgrad_supported(conv.in_channels, conv.out_channels):
            family = "s2"
        else:
            family = "lib"
        stats = _C64_STATS and family == "c64"
        # conv64's stride-2 data gradient has no addend.  (A stride-1 64 -> 64 layer whose filter is not channels_last
        # runs on the library and still takes the skip through its node, which then adds the gradient itself.)
        skip = family == "s2" or (c64 and _OWN_C64_S1 and stride == 1)
    return Route(family, bool(stats and conv.training), bool(skip), family == "s2",
                 (family == "c64" and (_OWN_C64_S1 or stride == 2))
                 or (family == "gen" and _GEN_BN_ON_LOAD and conv.in_channels <= 512),
                 family == "lib" and _DGRAD_FWD and stride == 1 and (_DGRAD_ANY or conv.in_channels == conv.out_channels))


class _ConvWrwFn(torch.autograd.Function):
    """conv3x3 / padding 1 of the families "c64", "s2" and "lib" (see Route).  Second output: the statistics partial of y
    (or an empty tensor)."""

    @staticmethod
    def forward(ctx, x, weight, wb, wrt, stride, route, skip=False):
        # x bf16 channels_last, wb = weight rounded to bf16 (what autocast feeds the convolution)
        kp = K.provider()
        partial = x.new_empty(0, dtype=torch.float32)
        if route.stats:
            y, partial = kp.conv3x3_c64_fwd(x, wb, with_stats=True, stride=stride)
        elif route.family == "c64":
            y = kp.conv3x3_c64_fwd(x, wb, stride=stride)
        else:
            y = F.conv2d(x, wb, None, stride, 1)
        ctx.route, ctx.stride = route, stride
        ctx.wrt = wrt                                  # not a graph tensor: a shadow owned by torchseg_amd.shadow
        # the fp32 master (a parameter) for the parity data gradient: its fragment-order image comes from the shadow bank
        ctx.master = weight if (route.family == "s2" and _SHADOW and weight.dtype == torch.float32) else None
        ctx.save_for_backward(x, wb)
        ctx.wparam = weight                            # (not a graph tensor here: only its .grad is looked at in backward)
        ctx.need_dx = x.requires_grad
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(partial)
        # skip: x is returned as a further output for the block's skip connection, so that the gradient of that path
        # arrives HERE (dskip) and is added in the epilogue of the data-gradient kernel instead of by autograd's own pass.
        # skip == 2 (stride 2): the further output is x[:, :, ::2, ::2] — what the block's 1x1 / stride-2 shortcut
        # convolution reads — as a compact tensor; the shortcut then runs as a stride-1 convolution of it and its gradient
        # comes back compact (tsg_conv3x3_s2_dgrad_subadd adds it at the even pixels of dx)
        ctx.skip_sub = skip == 2
        if not skip:
            return y, partial
        return y, partial, (x[:, :, ::2, ::2].contiguous(memory_format=torch.channels_last) if ctx.skip_sub else x)

    @staticmethod
    def backward(ctx, dy, _dpartial, dskip=None):
        kp = K.provider()
        x, wb = ctx.saved_tensors
        family, stride = ctx.route.family, ctx.stride
        sub = None
        if dskip is not None and ctx.skip_sub:
            sub, dskip = _bf16_nhwc(dskip), None           # compact: on the grid of x[:, :, ::2, ::2]
        if dy is None:                                     # only the skip path was used
            if sub is not None:
                dskip = torch.zeros_like(x)
                dskip[:, :, ::2, ::2] = sub
            return dskip, None, None, None, None, None, None
        dy = _bf16_nhwc(dy)
        dx = None
        if ctx.need_dx:
            in_hw = (x.shape[2], x.shape[3])
            add = _skip_addend(dskip, x.shape) if (family == "s2" or (family == "c64" and stride == 1)) else None
            if add is not None:                            # the kernel below adds it
                dskip = None
            if family == "s2":
                dx = kp.conv3x3_s2_dgrad(dy, wb if ctx.master is None else ctx.master, in_hw, addend=add, addend_sub=sub)
                sub = None
            elif family == "c64" and stride == 2:
                dx = kp.conv3x3_c64_s2_dgrad(dy, _rotated(ctx.wrt, wb), in_hw)
            elif family == "c64":
                dx = kp.conv3x3_c64_fwd(dy, _rotated(ctx.wrt, wb), addend=add)
            elif ctx.route.dgrad_fwd:
                # dx = conv(dy, rot180(w)^T): the library's forward kernels beat its backward-data kernels on the
                # symmetric layers (tools/probe_conv2.py); same bf16 operands, fp32 accumulation
                dx = F.conv2d(dy, _rotated(ctx.wrt, wb), None, 1, 1)
            else:
                dx = torch.ops.aten.convolution_backward(dy, x, wb, None, [stride, stride], [1, 1], [1, 1], False, [0, 0], 1,
                                                         [True, False, False])[0]
            if dskip is not None:
                dx = dx + dskip.to(dx.dtype)
            if sub is not None:                            # a data-gradient path without the compact addend
                dx[:, :, ::2, ::2] += sub.to(dx.dtype)
        dw = _conv_wrw(x, dy, stride, ctx.wparam)
        return dx, dw.to(ctx.wparam.dtype), None, None, None, None, None


class _ConvGenFn(torch.autograd.Function):
    """conv3x3 / stride 1 / padding 1 on the general MFMA kernel: forward from the fp32 master weight (the bf16 cast
    happens inside the filter preparation), data gradient as the forward convolution of dy with the rotated / transposed
    filter, weight gradient on tsg_conv3x3_wrw_gen.  Second output: the statistics partial of y (or an empty tensor)."""

    @staticmethod
    def forward(ctx, x, weight, with_stats, skip=False):
        kp = K.provider()
        wf = kp.conv3x3_gen_prep_filter(weight, 0, x)
        out = kp.conv3x3_gen_fwd(x, wf, weight.shape[0], with_stats=with_stats)
        y, partial = out if with_stats else (out, x.new_empty(0, dtype=torch.float32))
        ctx.save_for_backward(x, weight)
        ctx.need_dx = x.requires_grad
        ctx.mark_non_differentiable(partial)
        ctx.set_materialize_grads(False)
        return (y, partial, x) if skip else (y, partial)      # skip: see _ConvWrwFn.forward

    @staticmethod
    def backward(ctx, dy, _dpartial, dskip=None):
        kp = K.provider()
        x, weight = ctx.saved_tensors
        if dy is None:                                     # only the skip path was used
            return dskip, None, None, None
        dy = _bf16_nhwc(dy)
        dx = None
        if ctx.need_dx:
            O, I = weight.shape[0], weight.shape[1]
            if O % 16 == 0 and I % 64 == 0:
                add = _skip_addend(dskip, x.shape)
                dx = kp.conv3x3_gen_fwd(dy, kp.conv3x3_gen_prep_filter(weight, 1, dy), I, addend=add)
                if add is not None:
                    dskip = None
            else:
                dx = F.conv2d(dy, kp.conv3x3_weight_rot180_t(weight.detach().to(torch.bfloat16)), None, 1, 1)
            if dskip is not None:
                dx = dx + dskip.to(dx.dtype)
        dw = _conv_wrw(x, dy, 1, weight)
        return dx, dw.to(weight.dtype), None, None


class WrwConv2d(nn.Conv2d):
    def forward(self, x):
        return self._forward(x, False)

    def _forward(self, x, want_skip):
        """want_skip (True, or 2: the compact sub-sampled alias will do): returns (y, x_skip): x_skip is x — or the alias
        — as a further output of the convolution's autograd node when the fused path is taken, else None.
        want_skip=False: returns y."""
        route = None
        if (x.is_cuda and self.bias is None and self.weight.dtype == torch.float32 and x.dim() == 4
                and self.padding_mode == "zeros" and torch.is_grad_enabled() and self.weight.requires_grad and _wants_bf16(x)):
            xb = _bf16_nhwc(x)
            route = _route(self, xb)
        if route is None:
            y = super().forward(x)
            return (y, None) if want_skip else y
        skip = bool(want_skip and route.skip and xb is x and x.requires_grad)      # the alias must BE the block input
        with torch.autocast("cuda", enabled=False):
            if route.family == "gen":
                out = _ConvGenFn.apply(xb, self.weight, route.stats, skip)
            else:
                wb, wrt = _filters(self.weight)
                out = _ConvWrwFn.apply(xb, self.weight, wb, wrt, self.stride[0], route,
                                       2 if (skip and want_skip == 2 and route.compact) else skip)
        y = _with_partial(out[0], out[1])
        return (y, out[2] if skip else None) if want_skip else y


def conv_with_skip(conv, x, subsample=False):
    """`conv(x)` for the first convolution of a residual block whose skip connection is x itself (stride 1) or starts from x
    (stride 2: the 1x1 shortcut convolution, resnet.py:139-146).  Returns (y, x_skip):
    x_skip is x routed through the convolution's autograd node when our kernels compute its data gradient (then the
    block must use x_skip for `out += residual`: the skip path's gradient is added in that kernel's epilogue), else None
    (use x).  subsample=True (stride 2 only): x_skip may come back as the COMPACT x[:, :, ::2, ::2] — recognisable by its
    size — on which the 1x1 / stride-2 shortcut convolution is a stride-1 convolution; its gradient then returns compact
    too and is added at the even pixels of dx (no zero-filled full-size gradient)."""
    if _FUSE_SKIP and isinstance(conv, WrwConv2d) and conv.stride in ((1, 1), (2, 2)) and isinstance(x, torch.Tensor) \
            and x.is_cuda and torch.is_grad_enabled():
        return conv._forward(x, 2 if (subsample and _SKIP_SUB and conv.stride == (2, 2)) else True)
    return conv(x), None


def _c64_dgrad_and_bn_sums(kp, dy, rot, x, fp, stride, layout, N, C, HW):
    """(da, partial, S): the data gradient of a 64 -> 64 convolution whose input was relu(bn(x)) and the backward sums of
    that BatchNorm — from the kernel's epilogue where it has one, else by the separate pass."""
    if _BN_BSUM and kp.conv3x3_c64_bnsums_supported(x.shape[0], x.shape[2], x.shape[3], stride):
        if stride == 2:
            da, partial = kp.conv3x3_c64_s2_dgrad(dy, rot, (x.shape[2], x.shape[3]), bsum=(x, fp))
        else:
            da, partial = kp.conv3x3_c64_fwd(dy, rot, bsum=(x, fp))
        return da, partial, partial.shape[0]
    da = kp.conv3x3_c64_s2_dgrad(dy, rot, (x.shape[2], x.shape[3])) if stride == 2 else kp.conv3x3_c64_fwd(dy, rot)
    partial, Sn = kp.bn_bwd_reduce(da, x, None, layout, N, C, HW, fp, True)
    return da, partial, Sn


def _c64_fwd_on_load(kp, x, wb, stride, fp, out_stats):
    """(y, statistics partial of y or an empty tensor) of conv64 over relu(bn(x)), the BatchNorm applied on load."""
    if out_stats:
        return kp.conv3x3_c64_fwd(x, wb, with_stats=True, stride=stride, in_ab=fp)
    return kp.conv3x3_c64_fwd(x, wb, stride=stride, in_ab=fp), x.new_empty(0, dtype=torch.float32)


class _BnReluConvFn(torch.autograd.Function):
    """conv(relu(bn(x))) for the 3x3 layers our kernels cover, with the normalised activation never stored: the
    convolution (tsg_conv3x3_c64_*_fwd for 64 -> 64, tsg_conv3x3_gen_fwd for every other stride-1 layer) and its weight
    gradient (tsg_conv3x3_wrw_*_norm) apply a x + b, ReLU while they stage x; the data gradient of the convolution feeds
    the ordinary SyncBN backward, which needs dy and x only.  Second output: the statistics partial of y or an empty
    tensor."""

    @staticmethod
    def forward(ctx, x, gamma, beta, bn, use_batch_stats, group, hint, weight, wb, stride, wrt, gen=False, out_stats=False):
        kp = K.provider()
        layout, N, C, HW = K.bn_layout(x)
        invstd, fp, count_dev, world = S._forward_pack(kp, x, layout, N, C, HW, bn, gamma, beta, use_batch_stats, group, hint)
        if gen:
            out = kp.conv3x3_gen_fwd(x, kp.conv3x3_gen_prep_filter(weight, 0, x), weight.shape[0], with_stats=out_stats,
                                     in_ab=fp)
            y, partial = out if out_stats else (out, x.new_empty(0, dtype=torch.float32))
        else:
            y, partial = _c64_fwd_on_load(kp, x, wb, stride, fp, out_stats)
        ctx.save_for_backward(x, weight if gen else wb, gamma, beta, invstd, fp, count_dev)
        ctx.wparam = weight
        ctx.cfg = (layout, N, C, HW, use_batch_stats, group, world, stride, gen)
        ctx.wrt = wrt
        ctx.mark_non_differentiable(partial)
        return y, partial

    @staticmethod
    def backward(ctx, dy, _dpartial):
        kp = K.provider()
        x, wb, gamma, beta, invstd, fp, count_dev = ctx.saved_tensors
        layout, N, C, HW, use_batch_stats, group, world, stride, gen = ctx.cfg
        dy = _bf16_nhwc(dy)
        dw = _conv_wrw(x, dy, stride, ctx.wparam, in_ab=fp)
        if gen:                                                  # wb is the fp32 master weight here
            da = kp.conv3x3_gen_fwd(dy, kp.conv3x3_gen_prep_filter(wb, 1, dy), wb.shape[1])
            partial, Sn = kp.bn_bwd_reduce(da, x, None, layout, N, C, HW, fp, True)
        else:
            da, partial, Sn = _c64_dgrad_and_bn_sums(kp, dy, _rotated(ctx.wrt, wb), x, fp, stride, layout, N, C, HW)
        dgamma, dbeta, bp = S._backward_pack(kp, partial, Sn, C, N * HW, invstd, fp, count_dev, use_batch_stats, group,
                                             world, x.device)
        dx, _ = kp.bn_bwd_apply(da, x, None, layout, N, C, HW, bp, True, False)
        dgamma, dbeta = S._affine_grads(dgamma, dbeta, gamma, beta)
        return dx, dgamma, dbeta, None, None, None, None, dw.to(ctx.wparam.dtype), None, None, None, None, None


class _StemBnReluConvFn(torch.autograd.Function):
    """conv_3x3(relu(bn(stem(image)))) — SpatialPath's first two ConvBnRelu (bisenet network.py:116-117) — as ONE node:
    forward as StemConv2d + _BnReluConvFn; backward additionally folds the BatchNorm backward APPLY into the staging of the
    stem's weight gradient (tsg_stem_conv_wrw_bn), its only consumer, so neither relu(bn(xc)) nor d(xc) is ever stored."""

    @staticmethod
    def forward(ctx, img, w_stem, gamma, beta, bn, use_batch_stats, group, weight, wb, stride, wrt, out_stats=False):
        kp = K.provider()
        if use_batch_stats:
            xc, hint = kp.stem_conv_fwd_stats(img, w_stem)
        else:
            xc, hint = kp.stem_conv_fwd(img, w_stem), None
        layout, N, C, HW = K.bn_layout(xc)
        invstd, fp, count_dev, world = S._forward_pack(kp, xc, layout, N, C, HW, bn, gamma, beta, use_batch_stats, group, hint)
        y, partial = _c64_fwd_on_load(kp, xc, wb, stride, fp, out_stats)
        ctx.save_for_backward(img, xc, wb, gamma, beta, invstd, fp, count_dev)
        ctx.wparam, ctx.wstem = weight, w_stem
        ctx.cfg = (layout, N, C, HW, use_batch_stats, group, world, stride)
        ctx.wrt = wrt
        ctx.mark_non_differentiable(partial)
        return y, partial

    @staticmethod
    def backward(ctx, dy, _dpartial=None):
        kp = K.provider()
        img, xc, wb, gamma, beta, invstd, fp, count_dev = ctx.saved_tensors
        layout, N, C, HW, use_batch_stats, group, world, stride = ctx.cfg
        dy = _bf16_nhwc(dy)
        dw = _conv_wrw(xc, dy, stride, ctx.wparam, in_ab=fp)
        da, partial, Sn = _c64_dgrad_and_bn_sums(kp, dy, _rotated(ctx.wrt, wb), xc, fp, stride, layout, N, C, HW)
        dgamma, dbeta, bp = S._backward_pack(kp, partial, Sn, C, N * HW, invstd, fp, count_dev, use_batch_stats, group,
                                             world, xc.device)
        # the BatchNorm backward apply happens in the staging of the stem's weight gradient
        dw_stem = wrw_on_side_stream(lambda: kp.stem_conv_wrw_bn(img, da, xc, bp), ctx.wstem, img, da, xc, bp)
        dgamma, dbeta = S._affine_grads(dgamma, dbeta, gamma, beta)
        return None, dw_stem.to(ctx.wstem.dtype), dgamma, dbeta, None, None, None, dw.to(ctx.wparam.dtype), None, None, None, None


def stem_bn_relu_conv(stem, bn, relu, img, conv):
    """`conv(relu(bn(stem(img))))`: the fused node when everything is on the HIP path, None otherwise."""
    if not (_STEM_BN_WRW and _BN_ON_LOAD and relu is not None and isinstance(stem, StemConv2d)
            and isinstance(bn, S.SyncBatchNorm) and isinstance(conv, WrwConv2d) and isinstance(img, torch.Tensor)
            and img.is_cuda and img.dim() == 4 and not img.requires_grad and stem.bias is None and conv.bias is None
            and stem.weight.dtype == torch.float32 and conv.weight.dtype == torch.float32 and stem.weight.requires_grad
            and conv.weight.requires_grad and torch.is_grad_enabled() and stem.padding_mode == "zeros"
            and _wants_bf16(img) and bn.momentum is not None and bn.num_features == 64):
        return None
    # the stem's output does not exist yet: the route is asked with a stand-in of its dtype, layout and channel count
    route = _route(conv, torch.empty((1, conv.in_channels, 1, 1), dtype=torch.bfloat16, device="meta"), general=False)
    if route is None or route.family != "c64":
        return None
    xb = _as_bf16_image(img)
    w_stem = stem.weight if stem.weight.is_contiguous() else stem.weight.contiguous()
    if not K.provider().stem_conv_supported(xb, w_stem, stem.stride[0], stem.padding[0], stem.dilation[0], stem.groups):
        return None
    use_batch_stats = bn.training or not bn.track_running_stats
    with torch.autocast("cuda", enabled=False):
        wb, wrt = _filters(conv.weight)
        return _with_partial(*_StemBnReluConvFn.apply(xb, w_stem, bn.weight, bn.bias, bn, use_batch_stats, bn.process_group,
                                                      conv.weight, wb, conv.stride[0], wrt, route.stats))


def bn_relu_conv(bn, relu, x, conv):
    """`conv(relu(bn(x)))` — seg_oprs.py:39-46 followed by the next ConvBnRelu's convolution (bisenet network.py:117-118),
    BasicBlock's bn1 -> relu -> conv2 (resnet.py:36-46).  One fused autograd node on HIP tensors when `bn` is our
    SyncBatchNorm and `conv` one of the 3x3 layers our convolution kernels cover (64 -> 64 stride 1 / 2: conv64; with
    TSG_CONV_GEN_BN_ON_LOAD any other stride-1 layer with C_in <= 512: the general kernel); the three modules otherwise."""
    from .furnace_glue import norm_act
    route = None
    if (_BN_ON_LOAD and relu is not None and isinstance(bn, S.SyncBatchNorm) and isinstance(conv, WrwConv2d)
            and isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 4 and x.dtype == torch.bfloat16
            and x.shape[1] == conv.in_channels and conv.bias is None
            and conv.weight.dtype == torch.float32 and conv.weight.requires_grad and torch.is_grad_enabled()
            and bn.momentum is not None and not x.is_contiguous() and x.is_contiguous(memory_format=torch.channels_last)):
        route = _route(conv, x)
    if route is None or not route.bn_on_load:
        return conv(norm_act(bn, relu, x))
    bn._check_input_dim(x)
    use_batch_stats = bn.training or not bn.track_running_stats
    hint = take_bn_partial(x) if use_batch_stats and hasattr(x, "_tsg_bn_partial") else None
    gen = route.family == "gen"
    with torch.autocast("cuda", enabled=False):
        wb, wrt = (None, None) if gen else _filters(conv.weight)     # the general kernel reads the fp32 master
        return _with_partial(*_BnReluConvFn.apply(x, bn.weight, bn.bias, bn, use_batch_stats, bn.process_group, hint,
                                                  conv.weight, wb, conv.stride[0], wrt, gen, route.stats))


def _eligible(m):
    return (type(m) is nn.Conv2d and m.in_channels % 64 == 0 and m.out_channels % 64 == 0 and m.kernel_size == (3, 3)
            and m.stride in ((1, 1), (2, 2)) and m.padding == (1, 1) and m.dilation == (1, 1) and m.groups == 1 and m.bias is None)


def install_conv_wrw(module):
    """Re-class the eligible convolutions in place (both channel counts up to TSG_CONV_WRW_MAXC, default 512); returns how
    many were found."""
    maxc = int(_os.environ.get("TSG_CONV_WRW_MAXC", "512"))
    n = 0
    for m in module.modules():
        if _eligible(m) and max(m.in_channels, m.out_channels) <= maxc:
            m.__class__ = WrwConv2d
            n += 1
    return n
