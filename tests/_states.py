"""Shared by tests/test_module_states_{cpu,gpu}.py: the module states the parity tests of each kernel family do not visit
(eval-mode BatchNorm in a backward pass, frozen parameters, inputs without a gradient, accumulation into an existing
.grad, a second backward pass over a retained graph), the float64 references on the CPU and the bounds, each quoted from
the sibling test of its family."""
import contextlib

import numpy as np
import torch
import torch.nn as nn

# ---- bounds of tests/test_bn_gpu.py ----------------------------------------------------------------------------------
BN_FP32 = 1e-4            # test_bn_gpu.py:62-67 (y, dx; dgamma / dbeta with atol 1e-4 sqrt(n))
BN_BF16 = 8e-3            # test_bn_gpu.py:80,82 (y; dx with at most ...
BN_BF16_OUTLIERS = 1e-3   # ... this share of elements outside, test_bn_gpu.py:83)
BN_BF16_PARAM = 2e-2      # test_bn_gpu.py:84-85 (dgamma / dbeta, atol 2e-2 sqrt(n))

BN_STATES = ("eval", "frozen_affine", "eval_frozen_affine", "no_affine", "no_track", "no_dx", "accumulate", "retain")


@contextlib.contextmanager
def counted(kp, into):
    """`into` (a dict) receives the call count of every public provider method that ran inside the block."""
    from torchseg_amd import kernels as K
    cnt = K.CallCounter(kp)
    try:
        yield
    finally:
        into.update(cnt.stop())


def grads_of(leaves):
    return [None if t.grad is None else t.grad.detach().clone() for t in leaves]


def clear(leaves):
    for t in leaves:
        t.grad = None


def assert_same_bits(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert (a is None) == (b is None), (what, i)
        if a is not None:
            assert a.dtype == b.dtype and torch.equal(a, b), (what, i, (a.float() - b.float()).abs().max().item())


def assert_close_lists(got, want, rel, what):
    """vendor kernels in the path: max |a - b| <= rel * max |b| per tensor"""
    for i, (a, b) in enumerate(zip(got, want)):
        assert (a is None) == (b is None), (what, i)
        if a is not None:
            err, scale = (a.double() - b.double()).abs().max().item(), b.double().abs().max().item()
            assert err <= rel * max(scale, 1e-30), (what, i, err, scale)


def check_accumulate(step, leaves, dy1, dy2, g1, rel=None):
    """`step(dy)`: one forward + backward.  g1: the gradients of a single pass with dy1 onto empty .grad.  Two passes without
    zero_grad in between must leave g1 + g2 (the bits of the two single passes, added once in the gradient's dtype), and
    again after zero_grad(set_to_none=False).  rel: the sibling's tolerance where a vendor kernel is not run-to-run equal."""
    same = assert_same_bits if rel is None else (lambda a, b, w: assert_close_lists(a, b, rel, w))
    clear(leaves)
    step(dy2)
    g2 = grads_of(leaves)
    want = [None if a is None else a + b for a, b in zip(g1, g2)]
    clear(leaves)
    step(dy1)
    same(grads_of(leaves), g1, "first pass again")
    step(dy2)
    same(grads_of(leaves), want, "g1 + g2 onto a first gradient")
    for t in leaves:                                       # zero_grad(set_to_none=False)
        if t.grad is not None:
            t.grad.zero_()
    step(dy1)
    step(dy2)
    same(grads_of(leaves), want, "g1 + g2 onto zeroed gradients")


def check_retain(y, dy, leaves, g1, rel=None):
    """y: the output of a graph that has gone through backward(dy, retain_graph=True) once (g1).  The second pass over the
    same graph gives the same bits."""
    same = assert_same_bits if rel is None else (lambda a, b, w: assert_close_lists(a, b, rel, w))
    clear(leaves)
    y.backward(dy)
    same(grads_of(leaves), g1, "second pass over the retained graph")


def outlier_share(got, want, tol):
    got, want = got.double().cpu(), want.double().cpu()
    return ((got - want).abs() > tol + tol * want.abs()).double().mean().item()


def conv_check(y, y_ref, what=""):
    """_check of tests/test_conv3g_gpu.py:29-32: one bf16 ulp of the fp64 value plus 1e-3 of the output's scale."""
    y_ref = y_ref.double().cpu()
    err = (y.double().cpu() - y_ref).abs()
    bound = y_ref.abs() * 2.0 ** -8 + 1e-3 * y_ref.abs().max()
    assert bool((err <= bound).all()), (what, err.max().item(), y_ref.abs().max().item())


def wgrad_check(dw, dw_ref, what=""):
    """tests/test_conv3g_gpu.py:147 (test_autograd_node_installed_by_the_wrapper): 2e-3 of the weight gradient's scale."""
    dw_ref = dw_ref.double().cpu()
    err = (dw.double().cpu() - dw_ref).abs().max().item()
    assert err <= 2e-3 * dw_ref.abs().max().item(), (what, err, dw_ref.abs().max().item())


def bf16r(t):
    return t.to(torch.bfloat16).to(torch.float32)


# ---- SyncBatchNorm ---------------------------------------------------------------------------------------------------
class BnCase:
    """One SyncBatchNorm(+ residual)(+ ReLU) in `state` on `device`, and nn.BatchNorm2d in float64 on the CPU with the same
    (dtype-rounded) operands.  Inputs keep away from ReLU ties as tests/test_bn_gpu.py:20 does (scale 1.5, offset 0.4)."""

    def __init__(self, device, shape, layout, dtype, relu, res, state, seed=0):
        from torchseg_amd.syncbn import SyncBatchNorm
        assert state in BN_STATES or state == "train"
        N, C, H, W = shape
        self.shape, self.dtype, self.relu, self.res, self.state = shape, dtype, relu, res, state
        self.n = N * H * W
        self.training = state not in ("eval", "eval_frozen_affine")
        self.affine = state != "no_affine"
        self.track = state != "no_track"
        self.frozen = state in ("frozen_affine", "eval_frozen_affine")
        g = torch.Generator().manual_seed(seed + sum(shape))
        x = (torch.randn(shape, generator=g) * 1.5 + 0.4).to(dtype)
        r = torch.randn(shape, generator=g).to(dtype) if res else None
        self.dys = [torch.randn(shape, generator=g).to(dtype) for _ in range(2)]
        gamma = torch.randn(C, generator=g) * 0.5 + 1.0
        beta = torch.randn(C, generator=g) * 0.5
        rm0 = torch.randn(C, generator=g) * 0.3
        rv0 = torch.rand(C, generator=g) + 0.5
        self.fmt = torch.channels_last if layout == "nhwc" else torch.contiguous_format
        self.dy_fmt = torch.channels_last if layout in ("nhwc", "mixed") else torch.contiguous_format

        def make(cls, freeze=True):
            bn = cls(C, eps=1e-5, momentum=0.1, affine=self.affine, track_running_stats=self.track)
            with torch.no_grad():
                if self.affine:
                    bn.weight.copy_(gamma)
                    bn.bias.copy_(beta)
                if self.track:
                    bn.running_mean.copy_(rm0)
                    bn.running_var.copy_(rv0)
            bn.train(self.training)
            if self.frozen and freeze:
                bn.weight.requires_grad_(False)
                bn.bias.requires_grad_(False)
            return bn

        self.bn = make(SyncBatchNorm).to(device)
        self.x = x.to(device).contiguous(memory_format=self.fmt).requires_grad_(state != "no_dx")
        self.r = r.to(device).contiguous(memory_format=self.fmt).requires_grad_(True) if res else None
        self.dev_dys = [d.to(device).contiguous(memory_format=self.dy_fmt) for d in self.dys]
        self.leaves = [self.x] + ([self.r] if res else []) + list(self.bn.parameters())
        self.stats0 = self.stats()

        # the reference: the stock modules in float64
        ref = make(nn.BatchNorm2d, freeze=False).double()
        xr = x.double().requires_grad_(True)
        rr = r.double().requires_grad_(True) if res else None
        yr = ref(xr)
        if res:
            yr = yr + rr
        if relu:
            yr = torch.relu(yr)
        wanted = [xr] + ([rr] if res else []) + ([ref.weight, ref.bias] if self.affine else [])
        got = torch.autograd.grad(yr, wanted, self.dys[0].double(), allow_unused=True)
        self.ref = dict(y=yr.detach(), dx=got[0], dres=got[1] if res else None,
                        dgamma=got[-2] if self.affine else None, dbeta=got[-1] if self.affine else None,
                        rm=ref.running_mean, rv=ref.running_var,
                        nbt=int(ref.num_batches_tracked) if self.track else None)
        if not self.training and not relu:
            # eval: dx = dy gamma invstd of the running estimates (no batch terms)
            want = self.dys[0].double() * (gamma.double() * (rv0.double() + 1e-5).rsqrt()).view(1, -1, 1, 1)
            assert torch.allclose(self.ref["dx"], want, rtol=1e-12, atol=1e-12)

    def stats(self):
        if not self.track:
            return None
        return (self.bn.running_mean.clone(), self.bn.running_var.clone(), self.bn.num_batches_tracked.clone())

    def forward(self):
        return self.bn(self.x, residual=self.r, relu=self.relu)

    def step(self, dy, retain=False):
        y = self.forward()
        y.backward(dy, retain_graph=retain)
        return y

    def check(self, y, fp32_tol, exact_dres):
        """parity of the first pass (dys[0]) with the float64 modules, at the bounds of tests/test_bn_gpu.py"""
        ref, n, bn = self.ref, self.n, self.bn
        f = lambda t: t.detach().float().cpu().numpy()
        if self.dtype == torch.float32:
            tol, ptol = fp32_tol, fp32_tol
            np.testing.assert_allclose(f(y), ref["y"].numpy(), rtol=tol, atol=tol)
            if self.state != "no_dx":
                np.testing.assert_allclose(f(self.x.grad), ref["dx"].numpy(), rtol=tol, atol=tol)
            if self.res:
                np.testing.assert_allclose(f(self.r.grad), ref["dres"].numpy(), rtol=0 if exact_dres else tol,
                                           atol=0 if exact_dres else tol)               # test_bn_gpu.py:65
        else:
            tol, ptol = BN_BF16, BN_BF16_PARAM
            np.testing.assert_allclose(f(y), ref["y"].numpy(), rtol=tol, atol=tol)
            if self.state != "no_dx":
                share = outlier_share(self.x.grad, ref["dx"], tol)
                assert share < BN_BF16_OUTLIERS, share
            if self.res:
                share = outlier_share(self.r.grad, ref["dres"], tol)
                assert share < BN_BF16_OUTLIERS, share
        if self.state == "no_dx":
            assert self.x.grad is None
        if self.affine and not self.frozen:
            np.testing.assert_allclose(f(bn.weight.grad), ref["dgamma"].numpy(), rtol=ptol, atol=ptol * np.sqrt(n))
            np.testing.assert_allclose(f(bn.bias.grad), ref["dbeta"].numpy(), rtol=ptol, atol=ptol * np.sqrt(n))
        elif self.affine:
            assert bn.weight.grad is None and bn.bias.grad is None
        else:
            assert bn.weight is None and bn.bias is None
        if not self.track:
            assert bn.running_mean is None and bn.running_var is None and bn.num_batches_tracked is None
        elif not self.training:
            for a, b in zip(self.stats(), self.stats0):                                # bit-unchanged
                assert torch.equal(a, b)
        else:
            fp32 = self.dtype == torch.float32
            np.testing.assert_allclose(f(bn.running_mean), ref["rm"].numpy(), rtol=1e-5 if fp32 else 1e-4,
                                       atol=1e-6 if fp32 else 1e-5)                    # test_bn_gpu.py:68,86
            if fp32:
                np.testing.assert_allclose(f(bn.running_var), ref["rv"].numpy(), rtol=1e-4, atol=1e-6)   # test_bn_gpu.py:69
            assert int(bn.num_batches_tracked) == ref["nbt"]

    def check_calls(self, counts, fwd="bn_apply_fwd", bwd=("bn_bwd_reduce", "bn_bwd_apply")):
        """which provider methods the first forward + backward ran"""
        every = {"bn_apply_fwd", "bn_apply_fwd_bits", "bn_apply_fwd_mixed", "bn_bwd_reduce", "bn_bwd_reduce_bits",
                 "bn_bwd_reduce_mixed", "bn_bwd_apply", "bn_bwd_apply_bits", "bn_bwd_apply_mixed"}
        for name in (fwd,) + tuple(bwd) + ("bn_bwd_coeffs",):
            assert counts.get(name) == 1, (name, counts)
        for name in every - {fwd} - set(bwd):
            assert name not in counts, (name, counts)
        if self.training or not self.track:
            assert counts.get("bn_stats") == 1 and counts.get("bn_finalize") == 1 and "bn_affine" not in counts, counts
        else:
            assert counts.get("bn_affine") == 1 and "bn_stats" not in counts and "bn_finalize" not in counts, counts
        assert "bn_collapse" not in counts, counts

    def run(self, kp, fp32_tol=BN_FP32, exact_dres=True, fwd="bn_apply_fwd", bwd=("bn_bwd_reduce", "bn_bwd_apply")):
        counts = {}
        with counted(kp, counts):
            y = self.step(self.dev_dys[0], retain=self.state == "retain")
        self.check_calls(counts, fwd, bwd)
        self.check(y, fp32_tol, exact_dres)
        g1 = grads_of(self.leaves)
        if self.state == "retain":
            check_retain(y, self.dev_dys[0], self.leaves, g1)
        if self.state == "accumulate":
            check_accumulate(lambda dy: self.step(dy), self.leaves, self.dev_dys[0], self.dev_dys[1], g1)
        return counts


# ---- depthwise 3x3: the bound of tests/test_dwconv_gpu.py:31-43 ------------------------------------------------------------
def _ulp(v, mant):
    """one unit in the last place of the float64 value v in a format with `mant` explicit mantissa bits"""
    e = torch.floor(torch.log2(v.abs().clamp_min(1e-38)))
    return torch.pow(2.0, e - mant)


def ulp_check(got, want, scale, mant, acc_eps, what):
    """|got - want| <= 1 ulp of want in the output format + the accumulation's own rounding (acc_eps x sum of |terms|)"""
    err = (got.double().cpu() - want).abs()
    tol = _ulp(want, mant) + acc_eps * scale
    bad = err > tol
    assert not bool(bad.any()), (what, int(bad.sum()), float(err.max()), float((err - tol).max()))


def spy_kwargs(kp, name, log):
    """Record the keyword arguments of every call of provider method `name` (set BEFORE a `counted` block, whose end removes
    every instance attribute it finds on the provider, this one included)."""
    orig = getattr(kp, name)
    setattr(kp, name, lambda *a, **k: (log.append(dict(k)), orig(*a, **k))[1])
