"""Every HIP kernel family inside poisoned, guard-banded buffers (tests/_guard.py).

While a case runs, each provider method of GUARDED is interposed: one call becomes three calls of the same method on
the same operands — inside arenas filled with 0xFF (operands copied through `guarded`, outputs and workspaces from
`Guarded`, the workspaces at exactly the size the library reports), the same with 0xA5, and plain.  The interposer
asserts that no guard byte moved, that every output (statistics partials, argmax and mask bytes included) and every
operand afterwards is bit-identical in the three calls, and hands the guarded 0xFF result back to the caller.  The
callers are the families' own test functions and `_check` helpers, imported from their files and run at small ragged
shapes: their oracle assertions, with the project's bounds, therefore judge the guarded 0xFF result.  No tolerance is
stated in this file; every comparison it adds itself is exact.

CASES is the driver table: (family, case id, callable, argument, switches, the launch forms the case must reach under
guard).  tests/test_guard_cpu.py diffs it against the list of entry points and switches that must stay covered."""
import inspect
import os

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
""".split()

# -> (partial [S_max, 2, C], S): the launch decides how many partial rows it needs and returns that count; the rows
# behind it are not part of the result (every consumer folds partial[:S]), so the comparison stops at S
_ROWS_RETURNED = ("bn_stats", "bn_bwd_reduce", "bn_bwd_reduce_bits", "bn_bwd_reduce_mixed")

# arguments that make a launch form of their own: "+name" joins the method's name when the argument is given / true
_FORM_ARGS = ("with_stats", "in_ab", "addend", "addend_sub", "bsum", "out", "xc", "residual", "add", "accumulate")


def _form(name, args):
    f = name
    for k in _FORM_ARGS:
        v = args.get(k)
        if v is not None and v is not False:
            f += "+" + k
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
            _guard.assert_bit_identical([tuple(x[k] for k in keys) for x in after], names)
            ctx.hits.add(form)
            ctx.hits.add(name)
            if dt is not None:
                ctx.hits.add("%s:%s" % (name, str(dt).replace("torch.", "")))
            if args.get("out") is not None:
                return results[2]                         # the caller's own tensor, bit-identical to the guarded results
            return _detached(results[0])

        return method


# ---------------------------------------------------------------------------------------------------------------------
# the families' own checks, at the shapes of the issue
def _mods():
    import test_bn_gpu, test_bnconv_gpu, test_clshead_gpu, test_conv3g_gpu, test_conv64_gpu, test_convwrw_gpu
    import test_deepstem_gpu, test_dilconv_gpu, test_dwconv_gpu, test_exactconv_gpu, test_pool_gpu, test_stemconv_gpu
    import test_stemfuse_gpu, test_stempool_gpu, test_upsample_gpu, test_vecconv_gpu
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
    """tsg_resize_bilinear_hp has no kernel-level oracle check in the suite to import (the evaluator tests hold it to the
    oracle end to end): under guard, with the exact relations between its launch forms — out= writes what the plain call
    returns, and accumulate=True adds the same resize to what `out` held (0 + y)"""
    N, C, IH, IW, OH, OW = case
    kp = _kp()
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
