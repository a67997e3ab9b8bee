"""The guarded-buffer checker (tests/_guard.py) checked on the host: small torch functions stand in for kernels, written
the way the provider's wrappers are (outputs from torch.empty of this module's `torch`, which Guarded swaps).  Each of
the four ways a kernel can be wrong without an ordinary test noticing must fail the checker, a correct one must pass,
and the views must keep dtype, shape and strides."""
import sys

import pytest
import torch

import _guard
from _guard import Guarded, guarded, three_calls

ME = sys.modules[__name__]


def _scale(x):
    """a correct 'kernel': every output element written, nothing outside the operands touched"""
    y = torch.empty_like(x)
    y.copy_(x * 2)
    return y, torch.zeros(3, dtype=torch.int32)


def _store_before(x):
    y = torch.empty_like(x)
    y.copy_(x * 2)
    flat = y.as_strided((1,), (1,), y.storage_offset() - 1)
    flat.fill_(7.0)
    return y


def _store_after(x):
    y = torch.empty(x.numel(), dtype=x.dtype)
    y.copy_(x.reshape(-1) * 2)
    y.as_strided((1,), (1,), y.storage_offset() + y.numel()).fill_(7.0)
    return y


def _skips_one(x):
    y = torch.empty(x.numel(), dtype=x.dtype)
    y[:-1] = x.reshape(-1)[:-1] * 2
    return y


def _reads_behind(x):
    """sums one element more than the operand has (the 'halo' behind its end)"""
    y = torch.empty(1, dtype=x.dtype)
    y[0] = x.as_strided((x.numel() + 1,), (1,), x.storage_offset()).sum()
    return y


def _x(n=37, dtype=torch.float32):
    return (torch.arange(n, dtype=torch.float32) * 0.25 - 3).to(dtype)


def test_arena_layout_and_fill():
    t = _x(37, torch.bfloat16)
    with Guarded(0xA5, module=ME) as g:
        v = g.guarded(t)
        y = torch.empty(5, 3, dtype=torch.float32)
        z = torch.zeros(4, dtype=torch.int64)
    assert len(g.arenas) == 3
    for a, view, nbytes in zip(g.arenas, (v, y, z), (74, 60, 32)):
        assert a.nbytes == nbytes and a.off >= _guard.GUARD_BYTES and a.raw.numel() - a.off - nbytes >= _guard.GUARD_BYTES
        assert view.data_ptr() % 256 == 0 and view.data_ptr() == a.raw.data_ptr() + a.off
        assert bool((a.raw[:a.off] == 0xA5).all()) and bool((a.raw[a.off + nbytes:] == 0xA5).all())
    assert torch.equal(v, t)
    assert bool((y.view(torch.uint8) == 0xA5).all())                   # an 'empty' output holds the fill ...
    assert bool((z == 0).all())                                        # ... zeros is zero in its payload alone
    g.check()
    assert ME.torch is torch                                           # the module's torch is back
    nan = torch.full((2,), 0xFF, dtype=torch.uint8)
    assert bool(nan.view(torch.bfloat16).isnan().all()) and bool(torch.full((4,), 0xFF, dtype=torch.uint8).view(torch.float32).isnan().all())
    small = torch.full((4,), 0xA5, dtype=torch.uint8)
    assert -1e-10 < small.view(torch.float32).item() < 0 and -1e-10 < small[:2].view(torch.bfloat16).item() < 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.uint8])
def test_views_keep_dtype_shape_and_strides(dtype):
    base = (torch.arange(2 * 6 * 5 * 7) % 251).reshape(2, 6, 5, 7).to(dtype)
    for t in (base, base.contiguous(memory_format=torch.channels_last), base[:1].contiguous(memory_format=torch.channels_last),
              base[:, :, :1, :1].contiguous(), base.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)):
        v = guarded(t, 0xFF)
        assert v.dtype == t.dtype and v.shape == t.shape and v.stride() == t.stride() and torch.equal(v, t)
        assert v.is_contiguous() == t.is_contiguous()
        assert v.is_contiguous(memory_format=torch.channels_last) == t.is_contiguous(memory_format=torch.channels_last)
        assert v._guard_arena.nbytes == t.numel() * t.element_size()
    with Guarded(0xFF, module=ME) as g:
        e = torch.empty((2, 6, 5, 7), dtype=dtype, memory_format=torch.channels_last)
        l = torch.empty_like(base.contiguous(memory_format=torch.channels_last))
        m = torch.empty_like(base, memory_format=torch.channels_last)
    for v in (e, l, m):
        assert v.dtype == dtype and v.stride() == (210, 1, 42, 6) and v.is_contiguous(memory_format=torch.channels_last)
    g.check()


def test_a_correct_function_passes():
    plain, ff, a5 = three_calls(_scale, [_x()], module=ME)
    assert torch.equal(ff[0], _x() * 2) and torch.equal(a5[1], torch.zeros(3, dtype=torch.int32))


def test_store_one_element_before_the_payload_is_caught():
    with Guarded(0xFF, module=ME) as g:
        _store_before(g.guarded(_x()))
    with pytest.raises(AssertionError, match=r"allocation #1 empty_like \(37,\) torch.float32 .* damaged at payload offset -4"):
        g.check()


def test_store_one_element_after_the_payload_is_caught():
    x = _x(37, torch.bfloat16)
    with Guarded(0xA5, module=ME) as g:
        _store_after(g.guarded(x))
    with pytest.raises(AssertionError, match=r"allocation #1 empty \(37,\) torch.bfloat16 \(payload 74 bytes, fill 0xA5\) damaged at payload offset 74"):
        g.check()


def test_a_store_into_an_operands_guard_is_caught():
    x = guarded(_x(), 0xFF)                                            # made before the context: adopted by it
    with Guarded(0xFF, module=ME) as g:
        g.adopt(x)
        x.as_strided((1,), (1,), x.storage_offset() + x.numel()).fill_(0.0)
    with pytest.raises(AssertionError, match=r"allocation #0 operand \(37,\) torch.float32 .* damaged at payload offset 148"):
        g.check()


def test_an_unwritten_output_element_is_caught():
    with pytest.raises(AssertionError, match=r"output 0 \(37,\) torch.float32: .* differ in 4 bytes, first at byte 144"):
        three_calls(_skips_one, [_x()], module=ME)


def test_a_result_that_depends_on_an_element_behind_an_operand_is_caught():
    big = _x(38)
    x = big[:37]                                # the plain call may read element 37: it is the view's own storage
    with pytest.raises(AssertionError, match=r"output 0 \(1,\) torch.float32: .* differ in"):
        three_calls(_reads_behind, [x], module=ME)
    # ... while under one fill alone nothing is visibly wrong: the guards are intact and the value is finite
    with Guarded(0xA5, module=ME) as g:
        y = _reads_behind(g.guarded(x))
    g.check()
    assert bool(torch.isfinite(y).all())


def test_scratch_buffers_are_set_aside_and_retired():
    class Prov:
        def scratch(self, n):
            pool = self.__dict__.setdefault("_scratch_bufs", {})
            if "k" not in pool or pool["k"].numel() < n:
                pool["k"] = torch.empty(n, dtype=torch.uint8)
            return pool["k"]

    p = Prov()
    old = p.scratch(1000)
    with Guarded(0xFF, prov=p, module=ME) as g:
        ws = p.scratch(24)
        assert ws.numel() == 24 and bool((ws == 0xFF).all()) and ws is not old      # exactly the size asked for, poisoned
    assert p._scratch_bufs["k"] is old and any(r is ws for r in p._scratch_retired)
    g.check()


# ---- the driver table of tests/test_guarded_gpu.py against the entry points and switches that must stay under guard ----
# "method[+form]" as the interposer names a launch (UnderGuard / _form), "method:dtype" for the operand type
REQUIRED = """
conv3x3_gen_fwd conv3x3_gen_fwd+with_stats conv3x3_gen_fwd+in_ab conv3x3_gen_fwd+addend
conv3x3_gen_prep_filter+mode0 conv3x3_gen_prep_filter+mode1 conv3x3_gen_prep_filter:float32 conv3x3_gen_prep_filter:bfloat16
conv3x3_s2_dgrad conv3x3_s2_dgrad+addend conv3x3_s2_dgrad+addend_sub
conv3x3_c64_fwd conv3x3_c64_fwd+with_stats conv3x3_c64_fwd+in_ab conv3x3_c64_fwd+addend conv3x3_c64_fwd+bsum
conv3x3_c64_fwd+stride2 conv3x3_c64_fwd+with_stats+stride2 conv3x3_c64_fwd+in_ab+stride2
conv3x3_c64_s2_dgrad conv3x3_c64_s2_dgrad+bsum conv3x3_weight_rot180_t
conv3x3_wrw+gen conv3x3_wrw+tr conv3x3_wrw+v1 conv3x3_wrw+stride2+gen conv3x3_wrw+in_ab conv3x3_wrw+in_ab+stride2
conv3x3_wrw+out+gen conv3x3_wrw+out+tr conv3x3_wrw+out+v1 conv3x3_wrw+out+stride2+gen
conv3x3_dil_fwd conv3x3_dil_fwd+with_stats conv3x3_dil_dgrad conv3x3_dil_dgrad+addend conv3x3_dil_wrw conv3x3_dil_wrw+out
stem_conv_fwd stem_conv_fwd_stats stem_conv_wrw stem_conv_wrw_bn stem3_conv_fwd stem3_conv_wrw
stem_conv_stats stem_conv_bn_relu_pool_fwd stem_conv_bn_relu_pool_bwd_reduce stem_conv_wrw_bn_pool stem_conv_wrw_bn_pool+xc
dwconv3x3_fwd:bfloat16 dwconv3x3_fwd:float32 dwconv3x3_dgrad:bfloat16 dwconv3x3_dgrad:float32
dwconv3x3_wgrad:bfloat16 dwconv3x3_wgrad:float32
cls_head_fwd cls_head_bwd conv1x1_vec_fwd conv1x1_vec_bwd conv1x1_vec_bnact_fwd conv1x1_vec_bnact_bwd
bn_stats:float32 bn_stats:bfloat16 bn_apply_fwd bn_apply_fwd+residual bn_bwd_reduce bn_bwd_apply
bn_apply_fwd_bits:bfloat16 bn_apply_fwd_bits:float32 bn_bwd_reduce_bits bn_bwd_apply_bits
bn_apply_fwd_mixed bn_bwd_reduce_mixed bn_bwd_apply_mixed
bn_relu_pool_fwd:bfloat16 bn_relu_pool_fwd:float32 bn_relu_pool_bwd_reduce bn_relu_pool_bwd_apply
maxpool_fwd:float32 maxpool_fwd:bfloat16 maxpool_bwd gap_fwd:float32 gap_fwd:bfloat16 gap_bwd
adaptive_avgpool_fwd:float32 adaptive_avgpool_fwd:bfloat16 adaptive_avgpool_bwd
chanscale_fwd chanscale_bwd chanscale_bwd_ds chanscale_bwd_dx cat_channels
upsample_fwd:float32 upsample_fwd:bfloat16 upsample_fwd+add upsample_fwd_nhwc upsample_presum_fwd:float32
upsample_presum_fwd:bfloat16 upsample_bwd upsample_bwd_nhwc resize_bilinear_hp:float32 resize_bilinear_hp:bfloat16
upsample_nearest conv2d_f32_exact_fwd conv2d_f32_exact_dgrad conv2d_f32_exact_wgrad
ohem_fwd:float32 ohem_fwd:bfloat16 ohem_fwd+weight ohem_fwd+labels_u8
ohem_bwd:float32 ohem_bwd:bfloat16 ohem_bwd+weight ohem_bwd+labels_u8
ohem_up_fwd ohem_up_bwd ohem_target_prob kth_value
focal_fwd:float32 focal_fwd:bfloat16 focal_fwd+labels_u8 focal_bwd:float32 focal_bwd:bfloat16 focal_bwd+labels_u8
psa_fwd:float32 psa_fwd:bfloat16 psa_bwd:float32 psa_bwd:bfloat16
confusion_map confusion_map+out confusion_map+labels_u8 confusion_map+out+labels_u8
confusion_logits:float32 confusion_logits:bfloat16 confusion_logits+out confusion_logits+labels_u8 confusion_logits+out+labels_u8
seg_tail_logprob:float32 seg_tail_logprob:bfloat16 seg_tail_accum:float32 seg_tail_accum:bfloat16
seg_tail_accum seg_tail_accum+zflip seg_tail_accum+accumulate seg_tail_accum+zflip+accumulate
sgd_step sgd_step_dev
augment_crop augment_crop+gts augment_crop+gts+labels_u8 augment_crop+pad_pixel augment_crop+pad_pixel+inv_scale edge_labels edge_labels+labels_u8
""".split()

# launches that take raw addresses in tables: a hand-built guarded test each (test_guarded_gpu.HAND_BUILT)
REQUIRED_BY_HAND = ("sgd_multi_step_dev", "multi_copy", "tsg_weight_shadow_refresh")


def test_every_required_entry_point_and_switch_has_a_guarded_case():
    import test_guarded_gpu as T
    from torchseg_amd import kernels as K
    declared = set()
    for c in T.CASES:
        declared.update(c["forms"])
    missing = sorted(set(REQUIRED) - declared)
    assert not missing, "launch forms without a guarded case in tests/test_guarded_gpu.py: %s" % missing
    for f in sorted(declared):                                   # every declared form names an interposed provider method
        name = f.split("+")[0].split(":")[0]
        assert name in T.GUARDED and callable(getattr(K.HipKernels, name, None)), f
    # both kernels and both tile widths of the general convolution, every form of it under each
    for v2 in ("0", "2"):
        for bn in ("64", "128"):
            forms = set()
            for c in T.CASES:
                if c["env"] == {"TSG_CONV3G_V2": v2, "TSG_CONV3G_BN": bn}:
                    forms.update(c["forms"])
            want = {"conv3x3_gen_fwd", "conv3x3_gen_fwd+with_stats", "conv3x3_gen_fwd+addend", "conv3x3_gen_prep_filter+mode1"}
            if v2 == "0":
                want.add("conv3x3_gen_fwd+in_ab")                # normalise-on-load always takes the eight-row kernel
            assert want <= forms, (v2, bn, sorted(want - forms))
    ids = [c["id"] for c in T.CASES]
    assert len(set(ids)) == len(ids)
    for name in REQUIRED_BY_HAND:
        fn = getattr(T, T.HAND_BUILT[name], None)
        assert callable(fn) and any(m.name == "gpu" for m in getattr(fn, "pytestmark", [])), name
    # the shapes the criteria, attention, metric, tail and optimizer kernels must keep running at
    by_family = {}
    for c in T.CASES:
        if c["family"] in ("ohem", "ohemup", "focal", "psa", "metric", "segtail", "sgd"):
            by_family.setdefault(c["family"], set()).add(c["arg"])
    assert {(2, 19, 33, 47, "confident", 1 / 3, 0.7), (3, 7, 31, 5, "random", 1 / 2, 0.05), (1, 150, 9, 11, "confident", 1 / 4, 0.6),
            (2, 2, 16, 16, "confident", 1.0, 0.999), (1, 1), (5, 3), (1000, 1000), (65539, 4096)} <= by_family["ohem"]
    assert len(by_family["ohemup"]) >= 3 and all(a[1] <= 32 for a in by_family["ohemup"])
    assert {(1, 24, 8, 8), (2, 64, 72, 72), (1, 40, 136, 200), "all_large", "all_very_negative"} <= by_family["psa"]
    assert {(3, 5, 1, 7), (1, 150, 17, 13), (1, 1, 4, 4)} <= by_family["metric"] and any(a[1] == 192 for a in by_family["metric"])
    assert (1, 19, 5, 7, 20, 28) in by_family["segtail"]
    assert {a[1] for a in by_family["segtail"] if len(a) == 6} >= {1, 256}
    import test_segtail_gpu
    assert {(n, d) for n in test_segtail_gpu.GEOMS for d in (torch.float32, torch.bfloat16)} <= by_family["segtail"]
    assert {1, 3, 4095, 4096, 4097, 12289} <= by_family["sgd"] and set(T.MULTI_SIZES) == {1, 3, 4095, 4096, 4097, 12289, 9 * 64 * 64}
    focal = {a for a in by_family["focal"]}
    assert {(P, d, l, False) for P in (1, 255, 257, 4099) for d in (torch.float32, torch.bfloat16)
            for l in (torch.int64, torch.uint8)} <= focal and any(a[3] for a in focal)
    # the issue's shapes of the general and the stride-2 data-gradient kernels are all there
    args = {c["arg"] for c in T.CASES if c["family"] == "conv3g" and isinstance(c["arg"], tuple)}
    assert {(1, 16, 64, 5, 37), (2, 64, 128, 19, 70), (1, 32, 192, 1, 1), (2, 96, 64, 33, 31), (3, 256, 64, 9, 33),
            (1, 32, 32, 7, 9), (1, 64, 96, 33, 31), (3, 32, 64, 1, 1), (2, 96, 32, 20, 130)} <= args


def test_the_cpu_stand_in_returns_the_documented_selection_words():
    """sel[8] = {thr, n_kept, num_valid, branch, denominator, n_bad, 0, 0} (include/tsg_hip.h): the stand-in provider of the
    host-logic tests hands out the same eight words as the kernels, the two spare ones zero"""
    from _cpu_provider import OracleProvider
    g = torch.Generator().manual_seed(0)
    z = torch.randn(2, 5, 3, 4, generator=g)
    t = torch.randint(0, 5, (2, 3, 4), generator=g)
    t[0, 0] = 255
    t[1, 1, 1] = 7                                                   # neither a class nor the ignore value: n_bad
    loss, nll, lse, sel = OracleProvider().ohem_fwd(z, t, 255, 1.0, 0, None)
    valid = int(((t != 255) & (t < 5)).sum())
    assert sel.dtype == torch.int32 and tuple(sel.shape) == (8,)
    assert sel[1:4].tolist() == [valid, valid, 2] and int(sel[5]) == 1 and sel[6:].tolist() == [0, 0]
    assert sel[4:5].view(torch.float32).item() == float(valid) and sel[0:1].view(torch.float32).item() == float("inf")
