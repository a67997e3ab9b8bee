"""GPU parity of the OHEM cross-entropy kernels (through the C-ABI).

Bars (BASELINE.json north_star): selection is integer-exact; fp32 loss within
1e-4 of the reference CPU path.
 * k-th value select: bit-exact vs torch.sort on the same fp32 values.
 * golden cases (reference-generated): loss/grad within 1e-4; kept mask equal.
 * random large cases vs the oracle: kept mask equal away from the threshold
   (a 1-ulp softmax difference may flip membership AT the threshold).
"""
import os

import numpy as np
import pytest
import torch

from oracle import ohem_ref

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("n,k", [(1, 1), (5, 3), (1000, 1), (1000, 1000), (65536, 4096), (1 << 20, 65536),
                                 (3_000_001, 1_234_567)])
def test_kth_value_bit_exact(cuda, n, k):
    from torchseg_amd import kernels as K
    g = torch.Generator().manual_seed(n + k)
    v = torch.rand(n, generator=g)
    v[::7] = v[3] if n > 3 else v[0]          # ties
    if n > 10:
        v[5] = 0.0; v[6] = 1.0; v[7] = 1e-42  # zero, one, a subnormal
    ref = torch.sort(v)[0][k - 1]
    out = K.provider().kth_value(v.to(cuda), k).cpu()[0]
    assert out.view(torch.int32).item() == ref.view(torch.int32).item()


def _run(cuda, pred, target, thresh, min_kept, weight=None, dtype=torch.float32, ltype=torch.int64):
    from torchseg_amd.losses import ohem_cross_entropy
    p = pred.to(cuda).to(dtype).requires_grad_(True)
    t = target.to(cuda).to(ltype)
    w = weight.to(cuda) if weight is not None else None
    loss, sel = ohem_cross_entropy(p, t, 255, thresh, min_kept, w, return_selection=True)
    if torch.isfinite(loss):
        (loss * 1.5).backward()
        grad = p.grad.float().cpu() / 1.5
    else:
        grad = torch.zeros_like(pred)
    sel = sel.cpu()
    return loss.item(), grad, dict(thr=sel[0:1].view(torch.float32).item(), n_kept=int(sel[1]),
                                   num_valid=int(sel[2]), branch=int(sel[3]))


def test_ohem_golden_fp32(cuda):
    z = np.load(os.path.join(GOLD, "ohem_golden.npz"))
    names = sorted({k.split("/")[0] for k in z.files})
    for name in names:
        pred = torch.from_numpy(z[name + "/pred"])
        target = torch.from_numpy(z[name + "/target"].astype(np.int64))
        thresh, min_kept, use_w = z[name + "/cfg"]
        w = torch.tensor(ohem_ref.CITYSCAPES_WEIGHT) if use_w else None
        for ltype in (torch.int64, torch.uint8):
            loss, grad, info = _run(cuda, pred, target, float(thresh), int(min_kept), w, ltype=ltype)
            ref_loss = float(z[name + "/loss"])
            if np.isnan(ref_loss):
                assert np.isnan(loss), name
                continue
            assert abs(loss - ref_loss) <= 1e-4 * max(1.0, abs(ref_loss)), (name, loss, ref_loss)
            kept = (grad.abs().sum(1) > 0).numpy()
            kept_ref = np.abs(z[name + "/grad"]).sum(1) > 0
            np.testing.assert_array_equal(kept, kept_ref, err_msg=name)
            np.testing.assert_allclose(grad.numpy(), z[name + "/grad"], rtol=1e-4, atol=1e-7, err_msg=name)
            assert info["n_kept"] == int(kept_ref.sum()), name


CASES = [  # B, C, H, W, regime, min_kept fraction, thresh
    (2, 19, 64, 64, "random", 1 / 16, 0.7),
    (2, 19, 64, 64, "confident", 1 / 2, 0.7),
    (4, 19, 128, 96, "confident", 1 / 16, 0.7),
    (1, 150, 60, 60, "confident", 1 / 4, 0.6),
    (2, 19, 33, 47, "confident", 1 / 3, 0.7),     # HW not a multiple of the vector width
    (3, 7, 31, 5, "random", 1 / 2, 0.05),
    (2, 19, 256, 256, "confident", 1 / 16, 0.7),
    (2, 2, 16, 16, "confident", 1.0, 0.999),
]


def _make(B, C, H, W, regime, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, C, (B, H, W), generator=g)
    t[:, : max(1, H // 16)] = 255
    if regime == "random":
        pred = torch.randn(B, C, H, W, generator=g)
    else:
        t2 = t.clone(); t2[t2 == 255] = 0
        flip = torch.rand(t.shape, generator=g) < 0.1
        t2[flip] = torch.randint(0, C, (int(flip.sum()),), generator=g)
        pred = 8.0 * torch.nn.functional.one_hot(t2, C).permute(0, 3, 1, 2).float() + torch.randn(B, C, H, W, generator=g)
    return pred, t


def _check_vs_oracle(cuda, case, weight=None):
    B, C, H, W, regime, frac, thresh = case
    pred, t = _make(B, C, H, W, regime, seed=B * 1000 + H)
    min_kept = int(B * H * W * frac)
    p = pred.clone().requires_grad_(True)
    ref_loss, info = ohem_ref.ohem_cross_entropy(p, t, 255, thresh, min_kept, weight, return_info=True)
    ref_loss.backward()
    loss, grad, dev = _run(cuda, pred, t, thresh, min_kept, weight)
    assert dev["num_valid"] == info["num_valid"]
    assert dev["branch"] == info["branch"], (dev, info["branch"])
    assert abs(loss - ref_loss.item()) <= 1e-4 * max(1.0, abs(ref_loss.item()))
    kept = (grad.abs().sum(1) > 0).numpy()
    if info["mask_prob"] is None:      # min_kept > num_valid: no selection happened (loss_opr.py:78-79)
        near = np.zeros((B, H, W), dtype=bool)
    else:
        mp = info["mask_prob"].view(B, H, W).numpy()
        near = np.abs(mp - info["threshold"]) <= 4e-7 * max(info["threshold"], 1e-30)  # within ~2 ulp of the threshold
    np.testing.assert_array_equal(kept[~near], info["kept"].numpy()[~near])
    assert abs(dev["n_kept"] - info["n_kept"]) <= int(near.sum())
    if dev["branch"] == 1:   # threshold is the k-th value: equal up to softmax rounding
        assert abs(dev["thr"] - info["threshold"]) <= 4e-7 * info["threshold"]
    ok = ~near[:, None].repeat(C, 1)
    np.testing.assert_allclose(grad.numpy()[ok], p.grad.numpy()[ok], rtol=2e-4, atol=1e-7)
    return dev


@pytest.mark.parametrize("case", CASES)
def test_ohem_vs_oracle_fp32(cuda, case):
    _check_vs_oracle(cuda, case)


# class weights (loss_opr.py:57-63): nn.CrossEntropyLoss(weight=...) over the kept pixels = sum(w_t nll) / sum(w_t), at
# the bounds of the unweighted test; one case per threshold branch (0: thr == thresh, 1: the k-th value)
WEIGHTED = [((2, 19, 33, 47, "confident", 1 / 16, 0.7), 0), ((3, 7, 31, 5, "random", 1 / 2, 0.05), 1)]


@pytest.mark.parametrize("case,branch", WEIGHTED)
def test_ohem_class_weights_vs_oracle_fp32(cuda, case, branch):
    C = case[1]
    w = torch.tensor(ohem_ref.CITYSCAPES_WEIGHT) if C == 19 else \
        torch.rand(C, generator=torch.Generator().manual_seed(C)) * 3.0 + 0.25
    dev = _check_vs_oracle(cuda, case, w)
    assert dev["branch"] == branch


_SELECTION_SHAPES = ((2, 19, 128, 128, "confident", 0.5), (1, 19, 512, 512, "confident", 1 / 4), (3, 7, 31, 5, "random", 0.9))


def test_ohem_selection_bit_exact_given_device_probs(cuda, shapes=_SELECTION_SHAPES):
    """The selection contract, bit for bit (north_star: "bit-exact for OHEM top-k indices"): with p_t as the device
    computes it (tsg_ohem_target_prob: the kernels' own exp(-nll)), the threshold equals torch.sort(p_t)[k-1]
    (loss_opr.py:86-89) exactly and the kept set is exactly {valid & p_t <= thr} (loss_opr.py:90-92), so the kept
    INDICES equal the reference's given the same probabilities.  End to end against the CPU softmax the only
    possible difference is a pixel whose p_t differs by an ulp across devices AND sits at the threshold
    (SURVEY.md section 7), which test_ohem_vs_oracle_fp32 bounds."""
    from torchseg_amd import kernels as K
    kp = K.provider()
    for (B, C, H, W, regime, frac) in shapes:
        pred, t = _make(B, C, H, W, regime, seed=5)
        k = int(B * H * W * frac)
        td = t.to(cuda)
        loss, nll, lse, sel = kp.ohem_fwd(pred.to(cuda).contiguous(), td, 255, 0.05 if regime == "random" else 0.7, k, None)
        sel = sel.cpu()
        thr_bits = int(sel[0])
        assert int(sel[3]) == 1                                   # the k-th-value branch
        p = kp.ohem_target_prob(nll, td, C, 255).cpu()
        valid = t.view(-1) != 255
        ref_thr = torch.sort(p)[0][k - 1]                         # loss_opr.py:86-87 on the same fp32 values
        assert thr_bits == ref_thr.view(torch.int32).item()
        kept_ref = valid & (p <= ref_thr)                         # loss_opr.py:90-92
        assert int(sel[1]) == int(kept_ref.sum())
        g = kp.ohem_bwd(pred.to(cuda).contiguous(), td, 255, None, nll, lse, sel.to(cuda), torch.ones(1, device=cuda))
        kept_dev = (g.abs().sum(1) > 0).view(-1).cpu()
        assert torch.equal(kept_dev, kept_ref)                    # the kept indices, exactly
        mean = (nll.cpu().double() * kept_ref).sum() / kept_ref.sum()
        assert abs(mean.item() - loss.item()) <= 1e-5 * max(1.0, abs(mean.item()))


@pytest.mark.parametrize("case", CASES[:5])
def test_ohem_bf16(cuda, case):
    B, C, H, W, regime, frac, thresh = case
    pred, t = _make(B, C, H, W, regime, seed=77)
    pred = pred.bfloat16().float()     # oracle sees the same rounded logits
    min_kept = int(B * H * W * frac)
    p = pred.clone().requires_grad_(True)
    ref_loss, info = ohem_ref.ohem_cross_entropy(p, t, 255, thresh, min_kept, None, return_info=True)
    ref_loss.backward()
    loss, grad, dev = _run(cuda, pred, t, thresh, min_kept, dtype=torch.bfloat16)
    assert abs(loss - ref_loss.item()) <= 1e-4 * max(1.0, abs(ref_loss.item()))
    assert dev["branch"] == info["branch"]
    np.testing.assert_allclose(grad.numpy(), p.grad.numpy(), rtol=1.6e-2, atol=1e-6 + 4e-3 * np.abs(p.grad.numpy()).max())


def test_ohem_full_size_properties(cuda):
    """BASELINE config-2 size (16 x 19 x 1024 x 1024): size-independent properties.
    n_kept >= min_kept; kept == (p <= thr) recount; loss == mean nll over kept;
    gradient sums to zero over classes for every pixel and is zero on dropped pixels."""
    from torchseg_amd import kernels as K
    B, C, H, W = 16, 19, 1024, 1024
    g = torch.Generator(device=cuda).manual_seed(1)
    t = torch.randint(0, C, (B, H, W), generator=g, device=cuda)
    t[:, :8] = 255
    flip = torch.rand(t.shape, generator=g, device=cuda) < 0.1
    t2 = torch.where(flip, torch.randint(0, C, t.shape, generator=g, device=cuda), t).clamp(max=C - 1)
    pred = torch.randn(B, C, H, W, generator=g, device=cuda)
    pred.scatter_add_(1, t2.unsqueeze(1), torch.full((B, 1, H, W), 8.0, device=cuda))
    pred = pred.bfloat16()
    min_kept = B * H * W // 16
    kp = K.provider()
    loss, nll, lse, sel = kp.ohem_fwd(pred, t, 255, 0.7, min_kept, None)
    s = sel.cpu()
    thr = s[0:1].view(torch.float32).item()
    n_kept, num_valid, branch = int(s[1]), int(s[2]), int(s[3])
    valid = t.view(-1) != 255
    assert num_valid == int(valid.sum())
    assert n_kept >= min(min_kept, num_valid) - int((~valid).sum()) * 0
    p = torch.exp(-nll)
    kept = valid & (p <= thr)
    assert abs(int(kept.sum()) - n_kept) <= 64          # torch expf vs ocml expf at the threshold
    mean_nll = (nll.double() * kept).sum() / kept.sum()
    assert abs(mean_nll.item() - loss.item()) <= 1e-4 * max(1.0, abs(loss.item()))
    gs = torch.ones(1, device=cuda)
    d = kp.ohem_bwd(pred, t, 255, None, nll, lse, sel, gs).float()
    assert d.sum(1).abs().max().item() <= 1e-6          # softmax - onehot sums to 0 (bf16-rounded)
    dropped = ~kept.view(B, H, W)
    far = dropped & ((p.view(B, H, W) - thr).abs() > 1e-5)
    assert d.abs().sum(1)[far].max().item() == 0.0
