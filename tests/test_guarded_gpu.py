"""Every HIP kernel family inside poisoned, guard-banded buffers (tests/_guard.py).

While a case runs, each provider method of GUARDED is interposed: one call becomes three calls of the same method on
the same operands — inside arenas filled with 0xFF (operands copied through `guarded`, outputs and workspaces from
`Guarded`, the workspaces at exactly the size the library reports), the same with 0xA5, and plain.  The interposer
asserts that no guard byte moved, that every output (statistics partials, argmax and mask bytes included) and every
operand afterwards is bit-identical in the three calls, and hands the guarded 0xFF result back to the caller.  The
callers are the families' own test functions and `_check` helpers, imported from their files and run at small ragged
shapes: their oracle assertions, with the project's bounds, therefore judge the guarded 0xFF result.  No tolerance is
stated in this file; every comparison it adds itself is exact.

In-place launches: a call with out= (or dst, the accumulator of seg_tail_accum) hands the caller their own tensor back,
bit-identical to the guarded results; sgd_step / sgd_step_dev return nothing, and the comparison of the operands
afterwards is their check.  Launches that take raw addresses in tables (HAND_BUILT) cannot be interposed: each has a
hand-built test at the end of this file.

CASES is the driver table: (family, case id, callable, argument, switches, the launch forms the case must reach under
guard).  tests/test_guard_cpu.py diffs it against the list of entry points and switches that must stay covered."""
import inspect
import os

import numpy as np
import pytest
import torch

import _guard

# provider methods that run under guard (everything the required families launch through)
GUARDED = """
conv3x3_gen_fwd conv3x3_gen_prep_filter conv3x3_s2_dgrad
conv3x3_c64_fwd conv3x3_c64_s2_dgrad conv3x3_weight_rot180_t conv3x3_wrw
conv3x3_dil_fwd conv3x3_dil_dgrad conv3x3_dil_wrw conv3x3_dil_prep_filter
stem_conv_fwd stem_conv_fwd_stats stem_conv_wrw stem_conv_wrw_bn stem3_conv_fwd stem3_conv_wrw
stem_conv_stats stem_conv_bn_relu_pool_fwd stem_conv_bn_relu_pool_bwd_reduce stem_conv_wrw_bn_pool
dwconv3x3_fwd dwconv3x3_dgrad dwconv3x3_wgrad
cls_head_fwd cls_head_bwd conv1x1_vec_fwd conv1x1_vec_bwd conv1x1_vec_bnact_fwd conv1x1_vec_bnact_bwd
bn_stats bn_apply_fwd bn_bwd_reduce bn_bwd_apply bn_apply_fwd_bits bn_bwd_reduce_bits bn_bwd_apply_bits
bn_apply_fwd_mixed bn_bwd_reduce_mixed bn_bwd_apply_mixed
bn_relu_pool_fwd bn_relu_pool_bwd_reduce bn_relu_pool_bwd_apply
maxpool_fwd maxpool_bwd gap_fwd gap_bwd adaptive_avgpool_fwd adaptive_avgpool_bwd
chanscale_fwd chanscale_bwd chanscale_bwd_ds chanscale_bwd_dx cat_channels
upsample_fwd upsample_fwd_nhwc upsample_presum_fwd upsample_bwd upsample_bwd_nhwc resize_bilinear_hp upsample_nearest
conv2d_f32_exact_fwd conv2d_f32_exact_dgrad conv2d_f32_exact_wgrad
ohem_fwd ohem_bwd ohem_up_fwd ohem_up_bwd ohem_target_prob kth_value focal_fwd focal_bwd
psa_fwd psa_bwd confusion_map confusion_logits seg_tail_logprob seg_tail_accum
sgd_step sgd_step_dev augment_crop edge_labels
""".split()

# launches that take raw addresses in host or device tables: the interposer cannot wrap their operands, so each has a
# hand-built test below that places every segment in an arena of its own (tests/test_guard_cpu.py checks the names)
HAND_BUILT = {"sgd_multi_step_dev": "test_sgd_multi_step_under_guard", "multi_copy": "test_multi_copy_under_guard",
              "tsg_weight_shadow_refresh": "test_weight_shadow_refresh_under_guard"}

# -> (partial [S_max, 2, C], S): the launch decides how many partial rows it needs and returns that count; the rows
# behind it are not part of the result (every consumer folds partial[:S]), so the comparison stops at S
_ROWS_RETURNED = ("bn_stats", "bn_bwd_reduce", "bn_bwd_reduce_bits", "bn_bwd_reduce_mixed")

# arguments that make a launch form of their own: "+name" joins the method's name when the argument is given / true
_FORM_ARGS = ("with_stats", "in_ab", "addend", "addend_sub", "bsum", "zflip", "out", "xc", "residual", "add", "accumulate")
# an argument named `out` that is an operand, not a destination
_OUT_IS_AN_OPERAND = ("psa_bwd",)
# the argument a launch updates in place and hands back (out=; dst of seg_tail_accum): the caller gets their own tensor
_IN_PLACE = ("out", "dst")


def _form(name, args):
    f = name
    if name.startswith("ohem_") and args.get("weight") is not None:    # the optional class-weight table of the criteria
        f += "+weight"
    for k in _FORM_ARGS:
        v = args.get(k)
        if v is not None and v is not False and not (k == "out" and name in _OUT_IS_AN_OPERAND):
            f += "+" + k
    if name == "augment_crop":
        if args.get("gts") is not None:
            f += "+gts"
        if args["pad_pixel"] >= 0:
            f += "+pad_pixel"
        if args.get("inv_scale") is not None:
            f += "+inv_scale"
    labels = [args.get(k) for k in ("labels", "target", "gt")]
    if any(isinstance(v, torch.Tensor) and v.dtype == torch.uint8 for v in labels) or args.get("label_dtype") is torch.uint8:
        f += "+labels_u8"
    if args.get("stride") == 2:
        f += "+stride2"
    if name == "conv3x3_wrw" and args.get("variant"):
        f += "+" + args["variant"]
    if name in ("conv3x3_gen_prep_filter", "conv3x3_dil_prep_filter"):
        f += "+mode%d" % int(args["mode"])
    return f


def _wrap(o, fill):
    if isinstance(o, torch.Tensor):
        return _guard.guarded(o.detach(), fill)
    if isinstance(o, (tuple, list)):
        return type(o)(_wrap(v, fill) for v in o)
    return o


def _comparable(o):
    """host arrays among the operands (geometry tables, mean / std) as tensors, for assert_bit_identical"""
    if isinstance(o, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(o))
    if isinstance(o, (tuple, list)):
        return type(o)(_comparable(v) for v in o)
    return o


def _detached(o):
    """the guarded result as tensors of their own (an autograd node may not return a view of the arena)"""
    if isinstance(o, torch.Tensor):
        return o.clone()
    if isinstance(o, (tuple, list)):
        return type(o)(_detached(v) for v in o)
    return o


class UnderGuard:
    """Interposes the GUARDED methods of the provider's class for the duration of one case (instance-level spies of the
    existing tests, which delete themselves, sit on top and leave it in place)."""

    def __init__(self, monkeypatch, inject=None):
        from torchseg_amd import kernels as K
        self.K, self.hits, self.busy, self.inject = K, set(), False, inject or {}
        prov = K.provider()
        for name in GUARDED:
            monkeypatch.setattr(K.HipKernels, name, self._interposed(name, getattr(K.HipKernels, name)))
            if name in vars(prov):            # a bound method an earlier test's monkeypatch put back ON THE INSTANCE would
                monkeypatch.delattr(prov, name)                # shadow the class: aside for this case

    def _interposed(self, name, fn):
        sig = inspect.signature(fn)
        ctx = self

        def method(prov, *a, **kw):
            if ctx.busy:                                  # a provider method calling another one: already under guard
                return fn(prov, *a, **kw)
            b = sig.bind(prov, *a, **kw)
            b.apply_defaults()
            args = dict(b.arguments)
            args.pop("self", None)
            if name in ctx.inject:
                args.update(ctx.inject[name](args))
            form = _form(name, args)
            dt = next((v.dtype for v in args.values() if isinstance(v, torch.Tensor)), None)
            ctx.busy = True
            try:
                results, after, names = [], [], []
                for fill in _guard.FILLS:
                    with _guard.Guarded(fill, prov=prov, module=ctx.K) as g:
                        ga = {k: _wrap(v, fill) for k, v in args.items()}
                        results.append(fn(prov, **ga))
                    g.check()
                    after.append(ga)
                    names.append("guarded 0x%02X" % fill)
                results.append(fn(prov, **args))
                after.append(args)
                names.append("plain")
            finally:
                ctx.busy = False
            defined = [(r[0][:r[1]], r[1]) for r in results] if name in _ROWS_RETURNED else results
            _guard.assert_bit_identical(defined, names)
            # the operands afterwards: nothing but a documented in-place result (out=, running statistics) may have
            # changed, and that equally in the three calls
            keys = sorted(args)
            _guard.assert_bit_identical([tuple(_comparable(x[k]) for k in keys) for x in after], names)
            ctx.hits.add(form)
            ctx.hits.add(name)
            if dt is not None:
                ctx.hits.add("%s:%s" % (name, str(dt).replace("torch.", "")))
            if name not in _OUT_IS_AN_OPERAND and any(args.get(k) is not None for k in _IN_PLACE):
                return results[2]                         # the caller's own tensor, bit-identical to the guarded results
            return _detached(results[0])

        return method


# ---------------------------------------------------------------------------------------------------------------------
# the families' own checks, at the shapes of the issue
def _mods():
    import test_bn_gpu, test_bnconv_gpu, test_clshead_gpu, test_conv3g_gpu, test_conv64_gpu, test_convwrw_gpu
    import test_deepstem_gpu, test_dilconv_gpu, test_dwconv_gpu, test_exactconv_gpu, test_pool_gpu, test_stemconv_gpu
    import test_stemfuse_gpu, test_stempool_gpu, test_upsample_gpu, test_vecconv_gpu
    import test_augment_gpu, test_focal_gpu, test_fused_head_gpu, test_metric_gpu, test_ohem_gpu, test_psa_gpu, test_segtail_gpu
    import test_evalkernels_gpu
    return locals()


def _cl(t, cuda):
    return t.to(cuda).bfloat16().contiguous(memory_format=torch.channels_last)


def _kp():
    from torchseg_amd import kernels as K
    return K.provider()


def gen_all_forms(cuda, shape, mp):
    """conv3x3_gen_fwd: plain (+ both masters of the filter), statistics, normalise-on-load, the mode-1 filter, addend"""
    m = _mods()["test_conv3g_gpu"]
    B, Cin, Cout, H, W = shape
    kp = _kp()
    m.test_forward_vs_oracle(cuda, shape, None)
    m.test_statistics_epilogue_and_determinism(cuda, shape, None)
    if os.environ.get("TSG_CONV3G_V2") == "0":
        # a launch with in_ab always takes the eight-row kernel; the check compares it bit for bit with a launch
        # without in_ab, which holds where that one takes the eight-row kernel too
        m.test_normalise_on_load_equals_bn_apply_then_conv(cuda, shape, None)
    if Cin % 64 == 0:
        m.test_mode1_filter_is_the_data_gradient(cuda, shape, None)
    x, w, xb, wd = m._operands(cuda, *shape, seed=sum(shape) + 2)
    wf = kp.conv3x3_gen_prep_filter(wd, 0, xb)
    y = kp.conv3x3_gen_fwd(xb, wf, Cout)
    m._check(y, m.conv_ref.conv2d_ref(m.conv_ref.bf16_round(x), m.conv_ref.bf16_round(w), stride=1, pad=1))
    skip = _cl(torch.randn(B, Cout, H, W, generator=torch.Generator().manual_seed(3)), cuda)
    assert torch.equal(kp.conv3x3_gen_fwd(xb, wf, Cout, addend=skip), y + skip)     # bf16(bf16(conv) + addend)


def gen_reaches_the_sixteen_row_kernel(cuda, shape, mp):
    B, Cin, Cout, H, W = shape
    assert _kp().conv3x3_gen_variant(B, H, W, Cin, Cout) == 1
    gen_all_forms(cuda, shape, mp)


def gen_prep_filter(cuda, oi, mp):
    """tile widths 32 / 64 / 128, both modes, fp32 and bf16 master: the two masters give one image, and the image is a
    permutation of the bf16-rounded weights (what the consuming kernels' oracle checks then rely on)"""
    O, I = oi
    kp = _kp()
    w = torch.randn(O, I, 3, 3, generator=torch.Generator().manual_seed(O + I))
    wd = w.to(cuda).contiguous(memory_format=torch.channels_last)
    wb = wd.bfloat16().contiguous(memory_format=torch.channels_last)
    for mode in (0, 1):
        like = torch.empty(1, O if mode else I, 3, 5, device=cuda, dtype=torch.bfloat16)
        for bn in (32, 64, 128):
            if (I if mode else O) % bn:
                continue
            a, _ = kp.conv3x3_gen_prep_filter(wd, mode, like, bn=bn)
            b, _ = kp.conv3x3_gen_prep_filter(wb, mode, like, bn=bn)
            assert torch.equal(a, b)
            assert torch.equal(a.float().sort().values, wb.float().flatten().sort().values)


def s2_dgrad(cuda, shape, mp):
    m = _mods()["test_conv3g_gpu"]
    m.test_stride2_data_gradient_vs_oracle(cuda, shape)
    m.test_stride2_data_gradient_with_compact_addend(cuda, shape)


def c64_fwd(cuda, shape, mp):
    m = _mods()["test_conv64_gpu"]
    kp = _kp()
    B, H, W = shape
    m._run(cuda, B, H, W, seed=sum(shape))
    x, w, xb, wb, y, partial = m._run(cuda, B, H, W, seed=sum(shape), with_stats=True)
    skip = _cl(torch.randn(B, 64, H, W, generator=torch.Generator().manual_seed(3)), cuda)
    assert torch.equal(kp.conv3x3_c64_fwd(xb, wb, addend=skip), y + skip)           # bf16(bf16(conv) + addend)
    m.test_conv64_stride2_forward_and_data_gradient_vs_fp64(cuda, shape)


def c64_in_ab(cuda, shape, mp):
    m = _mods()["test_bnconv_gpu"]
    for stride in (1, 2):
        m.test_kernels_with_affine_on_load_equal_the_materialised_path(cuda, shape, stride)


def c64_bsum(cuda, shapes, mp):
    m = _mods()["test_conv64_gpu"]
    kp = _kp()
    for stride in (1, 2):
        ok = [s for s in shapes if kp.conv3x3_c64_bnsums_supported(*s, stride)]
        assert ok, "no shape of the list takes the fused sums at stride %d" % stride
        for s in ok:
            m.test_conv64_data_gradient_with_bn_backward_sums(cuda, s, stride)


def rot180(cuda, oi, mp):
    m = _mods()["test_convwrw_gpu"]
    for dtype in (torch.float32, torch.bfloat16):
        m.test_weight_rot180_transpose_is_exact(cuda, oi[0], oi[1], dtype)


def wrw_64(cuda, arg, mp):
    shape, variant = arg
    _mods()["test_convwrw_gpu"]._check(cuda, *shape, variant=variant)


def wrw_gen(cuda, arg, mp):
    shape, stride = arg
    _mods()["test_convwrw_gpu"]._check_gen(cuda, *shape, stride=stride)


def _nan_out(args):
    """out= for a weight-gradient call that did not pass one: an fp32 channels_last tensor full of NaN"""
    if args.get("out") is not None:
        return {}
    x, dy = args["x"], args["dy"]
    out = torch.full((dy.shape[1], x.shape[1], 3, 3), float("nan"), device=x.device)
    return {"out": out.contiguous(memory_format=torch.channels_last)}


def dil_fwd_dgrad(cuda, shape, mp):
    m = _mods()["test_dilconv_gpu"]
    m.test_forward_and_data_gradient_vs_float64(cuda, shape)
    m.test_statistics_epilogue_and_determinism(cuda, shape)


def dil_wrw(cuda, shape, mp):
    _mods()["test_dilconv_gpu"].test_weight_gradient_vs_float64_and_the_plain_kernel(cuda, shape)


def stem(cuda, shape, mp):
    ms = _mods()
    ms["test_stemconv_gpu"]._check(cuda, *shape)
    ms["test_stemfuse_gpu"].test_stem_conv_stats_epilogue(cuda, shape)
    ms["test_bnconv_gpu"].test_stem_weight_gradient_with_bn_backward_on_load(cuda, shape)


def stem_recompute(cuda, shape, mp):
    m = _mods()["test_stempool_gpu"]
    m.test_statistics_without_the_activation(cuda, shape)
    m.test_forward_equals_conv_then_bn_relu_pool(cuda, shape)
    m.test_backward_sums_and_weight_gradient(cuda, shape)


def stem3(cuda, shape, mp):
    _mods()["test_deepstem_gpu"]._check(cuda, *shape)


def dwconv(cuda, case, mp):
    m = _mods()["test_dwconv_gpu"]
    for dtype in (torch.bfloat16, torch.float32):
        m.test_kernels_against_float64(cuda, *case, dtype)


def clshead(cuda, case, mp):
    _mods()["test_clshead_gpu"].test_cls_head_kernels_vs_oracle(cuda, case)


def vecconv(cuda, shape, mp):
    _mods()["test_vecconv_gpu"].test_forward_and_both_gradients_vs_fp64(cuda, shape)


def vecconv_bnact(cuda, cfg, mp):
    _mods()["test_vecconv_gpu"].test_pooled_layer_in_one_launch_equals_the_module_sequence(cuda, cfg, True)


def bn(cuda, arg, mp):
    m = _mods()["test_bn_gpu"]
    from torchseg_amd import syncbn
    mp.setattr(syncbn, "PREFER_CHANNELS_LAST_OUTPUT", False)   # the module default (a DDP wrapper earlier in the process sets it)
    shape, layout = arg
    for relu, res in ((False, False), (True, False), (True, True), (False, True)):
        m.test_bn_fp32(cuda, shape, layout, relu, res)
    for relu, res in ((True, False), (True, True)):
        m.test_bn_bf16(cuda, shape, layout, relu, res)


def bn_mixed(cuda, shape, mp):
    m = _mods()["test_bn_gpu"]
    for dtype in (torch.float32, torch.bfloat16):
        for relu in (True, False):
            m.test_bn_mixed_layout_stem(cuda, shape, dtype, relu)


def bn_bits(cuda, shape, mp):
    m = _mods()["test_bn_gpu"]
    for dtype in (torch.bfloat16, torch.float32):
        m.test_block_tail_with_bit_mask_equals_the_stored_output_mask(cuda, shape, dtype, mp)


def bn_relu_pool(cuda, case, mp):
    m = _mods()["test_stemfuse_gpu"]
    for dtype in (torch.bfloat16, torch.float32):
        m.test_bn_relu_pool_forward_equals_the_unfused_kernels(cuda, case, dtype)
        m.test_bn_relu_pool_backward_equals_the_unfused_kernels(cuda, case, dtype)


def gap_chanscale(cuda, shape, mp):
    m = _mods()["test_pool_gpu"]
    from torchseg_amd import pool
    mp.setattr(pool, "_GAP_BWD_EXPAND", False)                 # the dense gradient (tsg_gap_bwd), not the broadcast view
    for layout in ("nchw", "nhwc"):
        for dtype in (torch.float32, torch.bfloat16):
            m.test_global_avg_pool(cuda, shape, layout, dtype)
            for ident in (False, True):
                m.test_channel_scale(cuda, shape, layout, dtype, ident)


def gated_scale(cuda, shape, mp):
    m = _mods()["test_pool_gpu"]
    for dtype in (torch.bfloat16, torch.float32):
        m.test_gated_scale_equals_pool_branch_and_channel_scale(cuda, shape, dtype, True, mp)


def maxpool(cuda, arg, mp):
    m = _mods()["test_pool_gpu"]
    for dtype in (torch.float32, torch.bfloat16):
        m.test_maxpool_channels_last(cuda, *arg, dtype)


def adaptive(cuda, case, mp):
    m = _mods()["test_pool_gpu"]
    for dtype in (torch.float32, torch.bfloat16):
        m.test_adaptive_avg_pool_channels_last(cuda, case, dtype)


def cat(cuda, shape, mp):
    _mods()["test_pool_gpu"].test_channel_concatenation_equals_torch_cat_forward_and_backward(cuda, shape)


def upsample_nchw(cuda, size, mp):
    m = _mods()["test_upsample_gpu"]
    for dtype in (torch.float32, torch.bfloat16):
        m.test_bilinear_fwd_bwd(cuda, *size, dtype)


def upsample_add_nearest(cuda, _, mp):
    m = _mods()["test_upsample_gpu"]
    m.test_bilinear_fused_add(cuda)
    m.test_nearest(cuda)


def upsample_nhwc(cuda, case, mp):
    m = _mods()["test_upsample_gpu"]
    for dtype in (torch.float32, torch.bfloat16):
        m.test_bilinear_channels_last(cuda, *case, dtype)


def upsample_presum(cuda, shape, mp):
    m = _mods()["test_upsample_gpu"]
    for dtype in (torch.float32, torch.bfloat16):
        for cl in (False, True):
            m.test_presum_upsample_matches_add_then_interpolate(cuda, dtype, cl, shape)


def resize_hp(cuda, case, mp):
    """tsg_resize_bilinear_hp under guard: the oracle check of tests/test_evalkernels_gpu.py (resize_scores and torch's
    float64 interpolate, at that file's bound) at this case's shape, and the exact relations between its launch forms —
    out= writes what the plain call returns, and accumulate=True adds the same resize to what `out` held (0 + y)"""
    N, C, IH, IW, OH, OW = case
    kp = _kp()
    for dtype in (torch.float32, torch.bfloat16):
        _mods()["test_evalkernels_gpu"].test_resize_hp_matches_both_oracles(cuda, dtype, (N * C, IH, IW, OH, OW))
    g = torch.Generator().manual_seed(IH + OW)
    for dtype in (torch.float32, torch.bfloat16):
        x = torch.randn(N, C, IH, IW, generator=g).to(dtype).to(cuda)
        y = kp.resize_bilinear_hp(x, OH, OW)
        assert y.dtype == torch.float32 and tuple(y.shape) == (N, C, OH, OW)
        out = torch.zeros_like(y)
        assert kp.resize_bilinear_hp(x, OH, OW, out=out, accumulate=True) is out and torch.equal(out, y)     # 0 + y
        assert torch.equal(kp.resize_bilinear_hp(x, OH, OW, out=out), y)


def exactconv(cuda, case, mp):
    _mods()["test_exactconv_gpu"].test_forward_dgrad_wgrad_are_correctly_rounded(cuda, case)


# (B, Cin, Cout, H, W): partial pixel tiles both ways, a 1x1 map, B >= 2, the smallest (16 / 64) and non-power-of-two
# (96, 192) channel counts, several oc tiles, many chunks
GEN_SHAPES = [(1, 16, 64, 5, 37), (2, 64, 128, 19, 70), (1, 32, 192, 1, 1), (2, 96, 64, 33, 31), (3, 256, 64, 9, 33)]
S2_SHAPES = [(1, 32, 32, 7, 9), (1, 64, 96, 33, 31), (3, 32, 64, 1, 1), (2, 96, 32, 20, 130)]
C64_SHAPES = [(1, 5, 37), (2, 8, 32), (1, 33, 70), (1, 1, 1), (1, 2, 2)]
BSUM_SHAPES = [(2, 8, 32), (1, 5, 37), (2, 9, 64), (1, 33, 70), (1, 1, 1), (1, 2, 2)]
# (B, Cin, Cout, H, W, d): H = 3 is smaller than the halo of d = 4 and H = 9 just larger; Cin 16 / 32 are no multiple of 64
DIL_SHAPES = [(1, 16, 64, 5, 37, 2), (1, 32, 192, 1, 1, 2), (1, 64, 128, 3, 7, 4), (2, 32, 64, 9, 11, 4), (3, 128, 64, 19, 70, 2)]
STEM_SHAPES = [(1, 70, 96), (3, 22, 130), (2, 129, 66), (1, 35, 130)]          # W is even by the kernel's contract
STEM3_SHAPES = [(1, 65, 97), (3, 22, 130), (1, 1, 1), (2, 7, 300)]
DW_CASES = [(2, 16, 33, 47, 2), (2, 24, 13, 29, 1), (3, 8, 7, 5, 2), (1, 40, 1, 9, 2), (2, 8, 1, 1, 1)]
CLS_CASES = [(3, 64, 20, 12, 21, True), (2, 128, 8, 14, 19, True), (1, 32, 4, 4, 7, False)]
VEC_SHAPES = [(5, 48, 80), (1, 16, 16), (2, 128, 128)]
BN_SHAPES = [(2, 64, 33, 47), (3, 24, 8, 8), (2, 19, 7, 5), (16, 128, 1, 1)]
EXACT_CASES = [(2, 24, 17, 15, 20, 3, 2, 2, 2, False), (1, 80, 17, 15, 72, 3, 1, 2, 2, True), (3, 5, 8, 8, 7, 5, 3, 1, 1, False)]

_GEN_FORMS = ["conv3x3_gen_fwd", "conv3x3_gen_fwd+with_stats", "conv3x3_gen_fwd+in_ab", "conv3x3_gen_fwd+addend",
              "conv3x3_gen_prep_filter+mode0", "conv3x3_gen_prep_filter:float32", "conv3x3_gen_prep_filter:bfloat16", "bn_stats"]

CASES = []


def _add(family, fn, args, forms, env=None, inject=None, ident=None):
    for a in args:
        CASES.append(dict(family=family, fn=fn, arg=a, forms=list(forms), env=dict(env or {}), inject=inject,
                          id="%s-%s-%s%s" % (family, ident or fn.__name__, str(a).replace(" ", ""),
                                             "".join("-%s=%s" % kv for kv in sorted((env or {}).items())))))


for _v2 in ("0", "2"):
    for _bn in ("64", "128"):
        _env = {"TSG_CONV3G_V2": _v2, "TSG_CONV3G_BN": _bn}
        _f = [f for f in _GEN_FORMS if _v2 == "0" or "in_ab" not in f]
        _add("conv3g", gen_all_forms, [s for s in GEN_SHAPES if s[1] % 64], _f, _env)
        _add("conv3g", gen_all_forms, [s for s in GEN_SHAPES if s[1] % 64 == 0], _f + ["conv3x3_gen_prep_filter+mode1"], _env)
_add("conv3g", gen_reaches_the_sixteen_row_kernel, [(2, 128, 128, 8, 32), (1, 32, 64, 37, 45)], _f,
     {"TSG_CONV3G_V2": "2", "TSG_CONV3G_BN": "64"})
_add("conv3g", gen_prep_filter, [(64, 32), (128, 256), (192, 96)],
     ["conv3x3_gen_prep_filter+mode0", "conv3x3_gen_prep_filter+mode1", "conv3x3_gen_prep_filter:float32",
      "conv3x3_gen_prep_filter:bfloat16"])
_add("conv3g", s2_dgrad, S2_SHAPES, ["conv3x3_s2_dgrad", "conv3x3_s2_dgrad+addend", "conv3x3_s2_dgrad+addend_sub"])
_add("conv64", c64_fwd, C64_SHAPES,
     ["conv3x3_c64_fwd", "conv3x3_c64_fwd+with_stats", "conv3x3_c64_fwd+addend", "conv3x3_c64_fwd+stride2",
      "conv3x3_c64_fwd+with_stats+stride2", "conv3x3_c64_s2_dgrad", "conv3x3_weight_rot180_t"])
_add("conv64", c64_in_ab, [(2, 24, 40), (1, 33, 70)],
     ["conv3x3_c64_fwd+in_ab", "conv3x3_c64_fwd+in_ab+stride2", "conv3x3_c64_fwd+with_stats+in_ab",
      "conv3x3_wrw+in_ab", "conv3x3_wrw+in_ab+stride2", "conv3x3_wrw+in_ab+gen", "bn_apply_fwd"])
_add("conv64", c64_bsum, [tuple(BSUM_SHAPES)], ["conv3x3_c64_fwd+bsum", "conv3x3_c64_s2_dgrad+bsum", "bn_bwd_reduce"])
_add("conv64", rot180, [(64, 64), (128, 64), (96, 160)], ["conv3x3_weight_rot180_t:float32", "conv3x3_weight_rot180_t:bfloat16"])
for _v in ("tr", "v1", "gen"):
    _add("conv3wrw", wrw_64, [(s, _v) for s in [(1, 3, 5), (3, 17, 70), (2, 6, 40)]], ["conv3x3_wrw+" + _v])
    _add("conv3wrw", wrw_64, [((3, 17, 70), _v)], ["conv3x3_wrw+out+" + _v], inject={"conv3x3_wrw": _nan_out}, ident="out")
_add("conv3wrw", wrw_gen, [((2, 6, 40, 64, 128), 1), ((1, 9, 33, 128, 64), 1), ((1, 5, 7, 128, 192), 1), ((3, 9, 33, 64, 64), 1)],
     ["conv3x3_wrw+gen"])
_add("conv3wrw", wrw_gen, [((2, 13, 70, 64, 128), 2), ((1, 9, 33, 128, 64), 2), ((1, 2, 2, 64, 64), 2), ((1, 31, 129, 64, 64), 2)],
     ["conv3x3_wrw+stride2+gen"])
_add("conv3wrw", wrw_gen, [((2, 6, 40, 64, 128), 1), ((3, 9, 33, 64, 64), 1)], ["conv3x3_wrw+out+gen"],
     inject={"conv3x3_wrw": _nan_out}, ident="out")
_add("conv3wrw", wrw_gen, [((2, 13, 70, 64, 128), 2)], ["conv3x3_wrw+out+stride2+gen"], inject={"conv3x3_wrw": _nan_out}, ident="out")
_add("dilconv", dil_fwd_dgrad, DIL_SHAPES,
     ["conv3x3_dil_fwd", "conv3x3_dil_fwd+with_stats", "conv3x3_dil_dgrad", "conv3x3_dil_dgrad+addend",
      "conv3x3_dil_prep_filter+mode0"])
_add("dilconv", dil_wrw, DIL_SHAPES, ["conv3x3_dil_wrw", "conv3x3_dil_wrw+out"])
_add("stem", stem, STEM_SHAPES, ["stem_conv_fwd", "stem_conv_fwd_stats", "stem_conv_wrw", "stem_conv_wrw_bn", "bn_bwd_apply"])
_add("stem", stem_recompute, [(1, 70, 96), (2, 22, 130), (1, 35, 130)],
     ["stem_conv_stats", "stem_conv_bn_relu_pool_fwd", "stem_conv_bn_relu_pool_bwd_reduce", "stem_conv_wrw_bn_pool",
      "stem_conv_wrw_bn_pool+xc", "bn_relu_pool_fwd", "bn_relu_pool_bwd_reduce", "bn_relu_pool_bwd_apply"])
_add("stem", stem3, STEM3_SHAPES, ["stem3_conv_fwd", "stem3_conv_wrw"])
_add("dwconv", dwconv, DW_CASES,
     ["dwconv3x3_fwd:bfloat16", "dwconv3x3_fwd:float32", "dwconv3x3_dgrad:bfloat16", "dwconv3x3_dgrad:float32",
      "dwconv3x3_wgrad:bfloat16", "dwconv3x3_wgrad:float32"])
_add("clshead", clshead, CLS_CASES, ["cls_head_fwd", "cls_head_bwd"])
_add("vecconv", vecconv, VEC_SHAPES, ["conv1x1_vec_fwd", "conv1x1_vec_bwd"])
_add("vecconv", vecconv_bnact, [(128, 128, True, False, True), (64, 48, True, False, False), (256, 256, False, True, False)],
     ["conv1x1_vec_bnact_fwd", "conv1x1_vec_bnact_bwd"])
_add("bn", bn, [(s, l) for s in BN_SHAPES for l in ("nchw", "nhwc")],
     ["bn_stats:float32", "bn_stats:bfloat16", "bn_apply_fwd", "bn_apply_fwd+residual", "bn_bwd_reduce", "bn_bwd_apply"])
_add("bn", bn_mixed, [(2, 8, 8, 12), (3, 64, 40, 24)], ["bn_apply_fwd_mixed", "bn_bwd_reduce_mixed", "bn_bwd_apply_mixed"])
_add("bn", bn_bits, [(2, 64, 33, 47), (3, 24, 8, 8), (16, 128, 1, 1)],
     ["bn_apply_fwd_bits:bfloat16", "bn_apply_fwd_bits:float32", "bn_bwd_reduce_bits", "bn_bwd_apply_bits"])
_add("bnpool", bn_relu_pool, [(2, 16, 9, 11), (2, 8, 7, 30), (1, 128, 33, 18)],
     ["bn_relu_pool_fwd:bfloat16", "bn_relu_pool_fwd:float32", "bn_relu_pool_bwd_reduce", "bn_relu_pool_bwd_apply",
      "maxpool_fwd", "maxpool_bwd"])
_add("pool", gap_chanscale, [(2, 64, 7, 5), (3, 19, 9, 9)],
     ["gap_fwd:float32", "gap_fwd:bfloat16", "gap_bwd", "chanscale_fwd", "chanscale_bwd"])
_add("pool", gated_scale, [(1, 8, 5, 7), (2, 64, 33, 47)], ["chanscale_bwd_ds", "chanscale_bwd_dx"])
_add("pool", maxpool, [((2, 64, 33, 47), 3, 2, 1), ((4, 8, 16, 16), 2, 2, 0), ((1, 128, 20, 12), 3, 1, 1)],
     ["maxpool_fwd:float32", "maxpool_fwd:bfloat16", "maxpool_bwd"])
_add("pool", adaptive, [(3, 24, 7, 10, 3), (1, 64, 33, 47, (5, 4)), (2, 128, 8, 8, 8)],
     ["adaptive_avgpool_fwd:float32", "adaptive_avgpool_fwd:bfloat16", "adaptive_avgpool_bwd"])
_add("pool", cat, [(2, 64, 256, 7, 9), (1, 8, 24, 5, 3)], ["cat_channels"])
_add("upsample", upsample_nchw, [(7, 5, 13, 9), (8, 8, 64, 64)], ["upsample_fwd:float32", "upsample_fwd:bfloat16", "upsample_bwd"])
_add("upsample", upsample_nchw, [(1, 1, 32, 32)], ["upsample_fwd:float32", "upsample_fwd:bfloat16"])      # 1x1: a broadcast
_add("upsample", upsample_add_nearest, [None], ["upsample_fwd+add", "upsample_nearest"])
_add("upsample", upsample_nhwc, [(8, 7, 5, 13, 9), (16, 9, 9, 4, 3), (24, 2, 3, 40, 17), (128, 32, 32, 64, 64)],
     ["upsample_fwd_nhwc", "upsample_bwd_nhwc"])
_add("upsample", upsample_presum, [(1, 16, 5, 7, 13, 9)], ["upsample_presum_fwd:float32", "upsample_presum_fwd:bfloat16"])
_add("upsample", resize_hp, [(2, 3, 7, 5, 13, 9), (1, 19, 9, 11, 5, 31)],
     ["resize_bilinear_hp:float32", "resize_bilinear_hp:bfloat16", "resize_bilinear_hp+out", "resize_bilinear_hp+out+accumulate"])
_add("convf32", exactconv, EXACT_CASES, ["conv2d_f32_exact_fwd", "conv2d_f32_exact_dgrad", "conv2d_f32_exact_wgrad"])


# ---------------------------------------------------------------------------------------------------------------------
# criteria, attention, metric, evaluation tail, optimizer, pre-processing
def _same_run(a, b):
    """two results of test_ohem_gpu._run -> equal bit for bit (loss, gradient, selection)"""
    assert a[0] == b[0] or (a[0] != a[0] and b[0] != b[0]), (a[0], b[0])
    _guard.assert_bit_identical([a[1], b[1]], ["int64 labels", "uint8 labels"])
    assert a[2] == b[2], (a[2], b[2])


def ohem(cuda, case, mp):
    """fp32 and bf16 logits against the oracle; uint8 labels give what int64 labels give, bit for bit"""
    m = _mods()["test_ohem_gpu"]
    B, C, H, W, regime, frac, thresh = case
    m.test_ohem_vs_oracle_fp32(cuda, case)
    m.test_ohem_bf16(cuda, case)
    pred, t = m._make(B, C, H, W, regime, seed=B * 1000 + H)
    k = int(B * H * W * frac)
    for dtype in (torch.float32, torch.bfloat16):
        _same_run(m._run(cuda, pred, t, thresh, k, dtype=dtype), m._run(cuda, pred, t, thresh, k, dtype=dtype, ltype=torch.uint8))


def ohem_more_than_valid(cuda, case, mp):
    """min_kept > num_valid: no mining (branch 2), every valid pixel kept"""
    m = _mods()["test_ohem_gpu"]
    B, C, H, W, regime, frac, thresh = case
    _, t = m._make(B, C, H, W, regime, seed=B * 1000 + H)
    assert int(B * H * W * frac) > int((t != 255).sum()) > 0
    dev = m._check_vs_oracle(cuda, case)
    assert dev["branch"] == 2 and dev["n_kept"] == dev["num_valid"] == int((t != 255).sum())


def ohem_all_ignored(cuda, shape, mp):
    """every label ignored: loss NaN (a mean over no pixel), nll == 0 everywhere, n_kept == 0, gradient all zero"""
    kp = _kp()
    B, C, H, W = shape
    g = torch.Generator().manual_seed(sum(shape))
    pred = torch.randn(B, C, H, W, generator=g)
    for dtype in (torch.float32, torch.bfloat16):
        for ltype in (torch.int64, torch.uint8):
            p = pred.to(dtype).to(cuda)
            t = torch.full((B, H, W), 255, dtype=ltype, device=cuda)
            loss, nll, lse, sel = kp.ohem_fwd(p, t, 255, 0.7, B * H * W // 4, None)
            s = sel.cpu()
            assert bool(torch.isnan(loss).all()) and not bool(nll.any())
            assert int(s[1]) == 0 and int(s[2]) == 0 and int(s[3]) == 2 and int(s[5]) == 0 and int(s[6]) == 0 and int(s[7]) == 0
            d = kp.ohem_bwd(p, t, 255, None, nll, lse, sel, torch.ones(1, device=cuda))
            assert d.dtype == dtype and d.shape == p.shape and not bool(d.float().any()), "gradient of an all-ignored batch"


def ohem_weights(cuda, arg, mp):
    _mods()["test_ohem_gpu"].test_ohem_class_weights_vs_oracle_fp32(cuda, *arg)


def ohem_target_prob(cuda, shape, mp):
    _mods()["test_ohem_gpu"].test_ohem_selection_bit_exact_given_device_probs(cuda, shapes=(shape,))


def kth(cuda, nk, mp):
    _mods()["test_ohem_gpu"].test_kth_value_bit_exact(cuda, *nk)


def ohem_up(cuda, case, mp):
    kp = _kp()
    B, C, IH, IW, OH, OW, regime, frac, thresh = case
    assert kp.ohem_up_supported(torch.empty(B, C, IH, IW, device="meta"), OH, OW, thresh), "the narrow fused head must take this shape"
    _mods()["test_fused_head_gpu"].test_fused_head_vs_oracle_fp32(cuda, case)


def focal(cuda, case, mp):
    _mods()["test_focal_gpu"].test_focal_vs_oracle(cuda, *case)


def psa(cuda, shape, mp):
    m = _mods()["test_psa_gpu"]
    m.test_psa_fp32(cuda, shape)
    m.test_psa_bf16(cuda, shape)


def psa_outside_range(cuda, regime, mp):
    """the flag and the three-launch redo of the bf16 forward over a poisoned workspace"""
    _mods()["test_psa_gpu"].test_psa_bf16_logits_outside_the_optimistic_range_take_the_guarded_path(
        cuda, regime, shape=(1, 64, 264, 200))


def confusion(cuda, shape, mp):
    m = _mods()["test_metric_gpu"]
    for dtype in (torch.float32, torch.bfloat16):
        m.test_hist_info_from_logits_vs_oracle(cuda, dtype, shape)


def confusion_out_twice(cuda, shape, mp):
    """out= accumulates: a second call into the same tensor adds the same counts"""
    kp = _kp()
    B, C, H, W = shape
    g = torch.Generator().manual_seed(sum(shape))
    z = torch.randn(B, C, H, W, generator=g).to(cuda)
    gt = torch.randint(0, C, (B, H, W), generator=g)
    gt[torch.rand(B, H, W, generator=g) < 0.2] = 255
    pred = z.argmax(1)
    for labels in (gt.to(cuda), gt.to(torch.uint8).to(cuda)):
        for first, call in ((kp.confusion_map(pred, labels, C), lambda o: kp.confusion_map(pred, labels, C, out=o)),
                            (kp.confusion_logits(z, labels, C), lambda o: kp.confusion_logits(z, labels, C, out=o))):
            once = first.clone()
            assert int(once[:C * C].sum()) == int((gt != 255).sum()) > 0
            assert call(first) is first and torch.equal(first, 2 * once)
            assert call(first) is first and torch.equal(first, 3 * once)


def segtail_logprob(cuda, case, mp):
    m = _mods()["test_segtail_gpu"]
    for dtype in (torch.float32, torch.bfloat16):
        m.test_logprob_matches_float64(cuda, *case, dtype)


def segtail_accum(cuda, arg, mp):
    m = _mods()["test_segtail_gpu"]
    name, dtype = arg
    for flip in (False, True):
        for accumulate in (False, True):
            m.test_accum_matches_reference_loop(cuda, name, flip, accumulate, dtype)


def _sgd_ref(p, g, b, lr, mom, wd, gs, first=False):
    """float64: d = g * gs + wd * p; b = d (first step) or mom * b + d; p -= lr * b (torch.optim.SGD, dampening 0)"""
    d = g * gs + wd * p
    b = d if first else mom * b + d
    return p - lr * b, b


def _close(got, want):
    torch.testing.assert_close(got.double().cpu(), want, rtol=1e-5, atol=1e-6)     # the bound of tests/test_optim_gpu.py


def sgd_single(cuda, n, mp):
    """tsg_sgd_step (host lr, `first` ignores the buffer's content) and tsg_sgd_step_dev (device lr, zeroed buffer), two
    steps each, against the float64 update; both return nothing and update their operands"""
    kp = _kp()
    gen = torch.Generator().manual_seed(n)
    p0, g1, g2 = (torch.randn(n, generator=gen) for _ in range(3))
    lr, mom, wd, gs = 0.05, 0.9, 5e-4, 0.5
    rp, rb = _sgd_ref(p0.double(), g1.double(), None, lr, mom, wd, gs, first=True)
    rp2, rb2 = _sgd_ref(rp, g2.double(), rb, lr, mom, wd, gs)
    p, b = p0.to(cuda), torch.full((n,), float("nan"), device=cuda)
    assert kp.sgd_step(p, g1.to(cuda), b, lr, mom, wd, gs, 1) is None
    _close(p, rp), _close(b, rb)
    kp.sgd_step(p, g2.to(cuda), b, lr, mom, wd, gs, 0)
    _close(p, rp2), _close(b, rb2)
    lr_dev = torch.tensor([0.1], device=cuda)                       # lr = lr_dev[0] * lr_mult
    rp, rb = _sgd_ref(p0.double(), g1.double(), torch.zeros(n, dtype=torch.float64), lr, mom, wd, gs)
    rp2, rb2 = _sgd_ref(rp, g2.double(), rb, lr, mom, wd, gs)
    p, b = p0.to(cuda), torch.zeros(n, device=cuda)
    assert kp.sgd_step_dev(p, g1.to(cuda), b, lr_dev, 0.5, mom, wd, gs) is None
    _close(p, rp), _close(b, rb)
    kp.sgd_step_dev(p, g2.to(cuda), b, lr_dev, 0.5, mom, wd, gs)
    _close(p, rp2), _close(b, rb2)
    assert bool(torch.equal(lr_dev.cpu(), torch.tensor([0.1])))


def augment(cuda, case, mp):
    m = _mods()["test_augment_gpu"]
    for label_dtype in (torch.int64, torch.uint8):
        m.test_augment_matches_oracle(cuda, case, label_dtype)


def augment_image_only(cuda, case, mp):
    """gts=None gives the image of the call with labels, bit for bit; pad_pixel >= 0 changes the padded pixels alone, to
    (pad_pixel / 255 - mean) / std formed in fp32 as the library's host code forms it"""
    m = _mods()["test_augment_gpu"]
    kp = _kp()
    (H, W), crop, p = case
    img, gt = m._sample(H, W, H + W)
    gt[gt == 255] = 0                                              # 255 in the label output then marks the padding alone
    imgs, gts = [torch.from_numpy(img).to(cuda)], [torch.from_numpy(gt).to(cuda)]
    geom = np.array([[H, W, int(H * p["scale"]), int(W * p["scale"]), int(p["flip"]), p["crop_y"], p["crop_x"]]], dtype=np.int32)
    mean, std = m.MEAN.astype(np.float32), m.STD.astype(np.float32)
    with_gt, lab = kp.augment_crop(imgs, gts, geom, crop, mean, std)
    alone, none = kp.augment_crop(imgs, None, geom, crop, mean, std)
    assert none is None and torch.equal(alone, with_gt)
    raw, _ = kp.augment_crop(imgs, None, geom, crop, mean, std, pad_pixel=7.0)
    pad = (lab == 255)[:, None].expand_as(raw)
    assert torch.equal(raw[~pad], with_gt[~pad])
    if bool(pad.any()):
        assert not bool(with_gt[pad].any())                        # pad_pixel < 0: the normalised image is padded with 0
        for c in range(3):
            want = (np.float32(7.0) / np.float32(255.0) - mean[c]) * (np.float32(1.0) / std[c])
            got = raw[:, c][lab == 255]
            assert bool((got == float(want)).all()), (c, float(want), got.unique().tolist())


def augment_eval_windows(cuda, case, mp):
    """the form Evaluator.scale_scores launches: inv_scale given, no labels, the raw image padded with 0, every window of
    the scale in one call, against the oracle's own windows"""
    _mods()["test_evalkernels_gpu"].test_augment_crop_as_the_evaluator_calls_it(cuda, case)


def edge(cuda, case, mp):
    m = _mods()["test_augment_gpu"]
    for label_dtype in (torch.int64, torch.uint8):
        m.test_dfn_edge_labels_match_oracle(cuda, case, label_dtype)


from test_augment_gpu import CASES as AUG_CASES                                       # module level: the tables below
from test_focal_gpu import FOCAL_CASES
from test_fused_head_gpu import CASES as HEAD_CASES
from test_ohem_gpu import WEIGHTED as OHEM_WEIGHTED
from test_segtail_gpu import GEOMS as SEGTAIL_GEOMS

OHEM_CASES = [(2, 19, 33, 47, "confident", 1 / 3, 0.7), (3, 7, 31, 5, "random", 1 / 2, 0.05), (1, 150, 9, 11, "confident", 1 / 4, 0.6),
              (2, 2, 16, 16, "confident", 1.0, 0.999)]
_OHEM_FORMS = ["ohem_fwd:float32", "ohem_fwd:bfloat16", "ohem_fwd+labels_u8", "ohem_bwd:float32", "ohem_bwd:bfloat16",
               "ohem_bwd+labels_u8"]
# the two smallest narrow (C <= 32) entries of test_fused_head_gpu.CASES, and a ragged one: IH, IW odd, OH no multiple of
# the 32-row band, OW = 301 one full 256-column tile and a partial one
OHEM_UP_CASES = sorted((c for c in HEAD_CASES if c[1] <= 32), key=lambda c: c[0] * c[1] * c[4] * c[5])[:2] + \
    [(1, 7, 5, 37, 21, 301, "confident", 1 / 3, 0.7)]
PSA_SHAPES = [(1, 24, 8, 8), (2, 64, 72, 72), (1, 40, 136, 200)]
CONFUSION_SHAPES = [(3, 5, 1, 7), (1, 150, 17, 13), (1, 1, 4, 4), (1, 192, 3, 5)]      # the last: n_cl = 192, the kernels' limit
SEGTAIL_CASES = [(1, 19, 5, 7, 20, 28), (2, 1, 3, 5, 9, 13), (1, 256, 4, 4, 13, 10)]   # C = 1; C = 256 on a 4x4 map
SGD_SIZES = [1, 3, 4095, 4096, 4097, 12289]                                             # the chunk is 4096 elements
EDGE_CASES = AUG_CASES[:7] + [((256, 512), (192, 192), dict(flip=True, scale=1.75, crop_y=100, crop_x=300))]

_add("ohem", ohem, OHEM_CASES, _OHEM_FORMS)
_add("ohem", ohem_more_than_valid, [(1, 5, 16, 16, "random", 0.97, 0.5)], ["ohem_fwd", "ohem_bwd"])
_add("ohem", ohem_all_ignored, [(2, 5, 7, 9)], _OHEM_FORMS)
_add("ohem", ohem_weights, OHEM_WEIGHTED, ["ohem_fwd+weight", "ohem_bwd+weight"])
_add("ohem", ohem_target_prob, [(3, 7, 31, 5, "random", 0.9)], ["ohem_target_prob", "ohem_fwd", "ohem_bwd"])
_add("ohem", kth, [(1, 1), (5, 3), (1000, 1000), (65539, 4096)], ["kth_value"])
_add("ohemup", ohem_up, OHEM_UP_CASES, ["ohem_up_fwd", "ohem_up_bwd"])
for _c in FOCAL_CASES:
    _dt = str(_c[1]).replace("torch.", "")
    _add("focal", focal, [_c], ["focal_fwd:" + _dt, "focal_bwd:" + _dt] +
         (["focal_fwd+labels_u8", "focal_bwd+labels_u8"] if _c[2] is torch.uint8 else ["focal_fwd", "focal_bwd"]))
_add("psa", psa, PSA_SHAPES, ["psa_fwd:float32", "psa_fwd:bfloat16", "psa_bwd:float32", "psa_bwd:bfloat16"])
_add("psa", psa_outside_range, ["all_large", "all_very_negative"], ["psa_fwd:bfloat16", "psa_bwd:bfloat16"])
_add("metric", confusion, [s for s in CONFUSION_SHAPES if s[1] > 2],
     ["confusion_logits:float32", "confusion_logits:bfloat16", "confusion_logits+out", "confusion_map", "confusion_map+out+labels_u8"])
_add("metric", confusion, [s for s in CONFUSION_SHAPES if s[1] <= 2],
     ["confusion_logits:float32", "confusion_logits:bfloat16", "confusion_logits+out", "confusion_map+out+labels_u8"])
_add("metric", confusion_out_twice, [(3, 5, 1, 7), (1, 150, 17, 13)],
     ["confusion_map", "confusion_map+out", "confusion_map+labels_u8", "confusion_map+out+labels_u8", "confusion_logits",
      "confusion_logits+out", "confusion_logits+labels_u8", "confusion_logits+out+labels_u8"])
_add("segtail", segtail_logprob, SEGTAIL_CASES, ["seg_tail_logprob:float32", "seg_tail_logprob:bfloat16"])
for _dt in (torch.float32, torch.bfloat16):
    _add("segtail", segtail_accum, [(n, _dt) for n in sorted(SEGTAIL_GEOMS)],
         ["seg_tail_accum", "seg_tail_accum+zflip", "seg_tail_accum+accumulate", "seg_tail_accum+zflip+accumulate",
          "seg_tail_accum:" + str(_dt).replace("torch.", "")])
_add("sgd", sgd_single, SGD_SIZES, ["sgd_step", "sgd_step_dev"])
_add("augment", augment, AUG_CASES, ["augment_crop+gts", "augment_crop+gts+labels_u8"])
_add("augment", augment_image_only, AUG_CASES[:7], ["augment_crop", "augment_crop+pad_pixel", "augment_crop+gts"])
_add("augment", augment_eval_windows, [((33, 47), 32, 1.25)], ["augment_crop+pad_pixel+inv_scale"])
_add("augment", edge, EDGE_CASES, ["edge_labels", "edge_labels+labels_u8", "augment_crop+gts", "augment_crop+gts+labels_u8"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_under_guard(cuda, case, monkeypatch):
    kp = _kp()
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    kp._npart.clear()                                          # cached geometry answers depend on the overrides
    ug = UnderGuard(monkeypatch, case["inject"])
    try:
        case["fn"](cuda, case["arg"], monkeypatch)
    finally:
        kp._npart.clear()
    missing = [f for f in case["forms"] if f not in ug.hits]
    assert not missing, ("launch forms this case must reach under guard but did not", missing, sorted(ug.hits))


# ---------------------------------------------------------------------------------------------------------------------
# the launches that take addresses (HAND_BUILT): every segment in an arena of its own, the tables built from those
# data_ptr()s, under both fills and plain; the guards, bit-identity of every segment, and the plain reference of the operation
MULTI_SIZES = SGD_SIZES + [9 * 64 * 64]
_UNALIGNED = 2                  # this segment's gradient / source starts 4 bytes off a 16-byte boundary: the scalar path


def _three_ways(run):
    """run(place, empty) under both fills and plain -> the three results, guards checked, bit-identical"""
    results, names = [], []
    for fill in _guard.FILLS:
        with _guard.Guarded(fill) as g:
            out = run(g.guarded, g.module.__dict__["torch"].empty)
        g.check()
        results.append(out)
        names.append("guarded 0x%02X" % fill)
    results.append(run(lambda t: t.clone(), torch.empty))
    names.append("plain")
    _guard.assert_bit_identical(results, names)
    return results[0]


@pytest.mark.gpu
def test_sgd_multi_step_under_guard(cuda):
    """tsg_sgd_multi_step_dev: segments of 1, 3, 4095, 4096, 4097, 12289 and 9*64*64 elements in two parameter groups,
    two steps from zeroed momentum buffers, against the float64 update at the bound of tests/test_optim_gpu.py"""
    kp = _kp()
    gen = torch.Generator().manual_seed(11)
    p0 = [torch.randn(n, generator=gen) for n in MULTI_SIZES]
    grads = [[torch.randn(n, generator=gen) for n in MULTI_SIZES] for _ in range(2)]
    group = np.array([i % 2 for i in range(len(MULTI_SIZES))], dtype=np.int32)
    numel = np.array(MULTI_SIZES, dtype=np.int64)
    lr, mom, wd, gs = [0.05, 0.5], np.array([0.9, 0.5], dtype=np.float32), np.array([5e-4, 0.0], dtype=np.float32), 0.25

    def run(place, empty):
        ps = [place(t.to(cuda)) for t in p0]
        bs = [place(torch.zeros(n, device=cuda)) for n in MULTI_SIZES]
        lr_dev = place(torch.tensor(lr, device=cuda))
        bmap = place(kp.sgd_multi_blockmap(numel, cuda))
        for step in range(2):
            gr = []
            for i, t in enumerate(grads[step]):
                if i == _UNALIGNED:
                    gr.append(place(torch.cat([torch.zeros(1), t]).to(cuda))[1:])
                    assert gr[-1].data_ptr() % 16 == 4
                else:
                    gr.append(place(t.to(cuda)))
            ptrs = np.array([[t.data_ptr() for t in ps], [t.data_ptr() for t in gr], [t.data_ptr() for t in bs]], dtype=np.uint64)
            kp.sgd_multi_step_dev(ptrs, numel, group, lr_dev, mom, wd, bmap, grad_scale=gs)
            torch.cuda.synchronize()
        return tuple(ps) + tuple(bs) + tuple(gr) + (lr_dev, bmap)

    out = _three_ways(run)
    for i, n in enumerate(MULTI_SIZES):
        gi = int(group[i])
        rp, rb = p0[i].double(), torch.zeros(n, dtype=torch.float64)
        for step in range(2):
            rp, rb = _sgd_ref(rp, grads[step][i].double(), rb, lr[gi], float(mom[gi]), float(wd[gi]), gs)
        _close(out[i], rp), _close(out[len(MULTI_SIZES) + i], rb)
        assert torch.equal(out[2 * len(MULTI_SIZES) + i].cpu(), grads[1][i])           # the gradients are read only


@pytest.mark.gpu
@pytest.mark.parametrize("with_map", [False, True])
def test_multi_copy_under_guard(cuda, with_map):
    """tsg_multi_copy_f32: dst[i] = scale * src[i], exact (one fp32 multiplication per element), into destinations that
    hold the fill; one source and one destination start off a 16-byte boundary"""
    kp = _kp()
    gen = torch.Generator().manual_seed(12)
    src = [torch.randn(n, generator=gen) for n in MULTI_SIZES]
    scale = 0.3

    def run(place, empty):
        ss = [place(torch.cat([torch.zeros(1), t]).to(cuda))[1:] if i == _UNALIGNED else place(t.to(cuda)) for i, t in enumerate(src)]
        ds = [empty(n + 1, dtype=torch.float32, device=cuda)[1:] if i == _UNALIGNED + 1 else empty(n, dtype=torch.float32, device=cuda)
              for i, n in enumerate(MULTI_SIZES)]
        bmap = place(kp.sgd_multi_blockmap(np.array(MULTI_SIZES, dtype=np.int64), cuda)) if with_map else None
        back = kp.multi_copy(ss, ds, blockmap=bmap, scale=scale)
        torch.cuda.synchronize()
        assert bmap is None or back is bmap
        return tuple(ds) + tuple(ss)

    out = _three_ways(run)
    for i, t in enumerate(src):
        assert torch.equal(out[i].cpu(), t * torch.tensor(scale, dtype=torch.float32)), MULTI_SIZES[i]
        assert torch.equal(out[len(src) + i].cpu(), t)


@pytest.mark.gpu
@pytest.mark.parametrize("own_pass", [True, False])
def test_weight_shadow_refresh_under_guard(cuda, own_pass, monkeypatch):
    """tsg_weight_shadow_refresh through torchseg_amd.shadow._Bank: the masters copied into arenas, every shadow (bf16
    cast, rot180-transpose, both fragment-order images) allocated by the bank inside arenas that hold the fill.  Exact:
    wb = bf16(w), wrt = the rot180-transpose of tests/test_convwrw_gpu.py, the fragment images what
    tsg_conv3x3_gen_prep_filter writes.  own_pass False: every image written by the blocks that walk the source."""
    from torchseg_amd import shadow
    kp = _kp()
    monkeypatch.setattr(shadow, "_WF1_PASS", own_pass)
    gen = torch.Generator().manual_seed(13)
    filters = [torch.randn(*s, generator=gen).to(cuda).contiguous(memory_format=torch.channels_last)
               for s in [(64, 32, 3, 3), (32, 64, 3, 3), (96, 32, 3, 3)]]
    plain = [torch.randn(n, generator=gen).to(cuda) for n in (5, 4097)]          # 1-D parameters: the cast alone

    def run(place):
        bank = shadow._Bank()
        ws, vs = [place(w) for w in filters], [place(v) for v in plain]
        out = []
        for w in ws:
            wb, wrt = bank.get(w, want_rot=True)
            out += [wb, wrt, bank.get_gen(w, 0, 32), bank.get_gen(w, 1, 32)]
        for v in vs:
            out.append(bank.get(v)[0])
        with torch.no_grad():
            ws[1].mul_(1.5)                              # a change torch sees: one launch rewrites every shadow
        out.append(bank.get(ws[1], want_rot=True)[0])
        torch.cuda.synchronize()
        return tuple(out) + tuple(ws) + tuple(vs)

    results, names = [], []
    for fill in _guard.FILLS:
        with _guard.Guarded(fill, prov=None, module=shadow) as g:
            out = run(g.guarded)
        g.check()
        results.append(out)
        names.append("guarded 0x%02X" % fill)
    results.append(run(lambda t: t.clone()))
    names.append("plain")
    _guard.assert_bit_identical(results, names)
    out = results[0]
    for i, w0 in enumerate(filters):
        w = w0 * 1.5 if i == 1 else w0
        wb, wrt, wf0, wf1 = out[4 * i:4 * i + 4]
        assert wb.stride() == w.stride() and torch.equal(wb, w.to(torch.bfloat16))
        assert wrt.is_contiguous(memory_format=torch.channels_last) and torch.equal(wrt, w.flip(2, 3).transpose(0, 1).to(torch.bfloat16))
        O, I = w.shape[0], w.shape[1]
        for mode, got in ((0, wf0), (1, wf1)):
            like = torch.empty(1, O if mode else I, 8, 8, device=cuda)
            assert torch.equal(got, kp.conv3x3_gen_prep_filter(w, mode, like, bn=32)[0]), (tuple(w.shape), mode)
    n = 4 * len(filters)
    for j, v in enumerate(plain):
        assert torch.equal(out[n + j], v.to(torch.bfloat16))
    assert torch.equal(out[n + len(plain)], (filters[1] * 1.5).to(torch.bfloat16))
