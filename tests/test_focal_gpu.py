"""GPU parity: sigmoid focal loss vs reference-generated golden vectors and the oracle."""
import os

import numpy as np
import pytest
import torch

from oracle import focal_ref

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_focal_golden(cuda):
    from torchseg_amd.losses import SigmoidFocalLoss
    z = np.load(os.path.join(GOLD, "focal_golden.npz"))
    for name in sorted({k.split("/")[0] for k in z.files}):
        gamma, alpha = z[name + "/cfg"]
        crit = SigmoidFocalLoss(255, gamma=float(gamma), alpha=float(alpha))
        for ltype in (torch.int64, torch.uint8):
            pred = torch.from_numpy(z[name + "/pred"]).to(cuda).requires_grad_(True)
            tgt = torch.from_numpy(z[name + "/target"].astype(np.int64)).to(cuda).to(ltype)
            loss = crit(pred, tgt)
            loss.backward()
            assert abs(loss.item() - float(z[name + "/loss"])) <= 1e-6
            np.testing.assert_allclose(pred.grad.cpu().numpy(), z[name + "/grad"], rtol=1e-4, atol=1e-8)


def test_focal_dfn_size_bf16(cuda):
    from torchseg_amd.losses import SigmoidFocalLoss
    g = torch.Generator().manual_seed(3)
    pred = (torch.randn(2, 1, 1024, 1024, generator=g) * 3).bfloat16()
    tgt = torch.randint(0, 2, (2, 1024, 1024), generator=g)
    tgt[torch.rand(tgt.shape, generator=g) < 0.1] = 255
    pr = pred.float().requires_grad_(True)
    ref = focal_ref.sigmoid_focal_loss(pr, tgt, 255, 2.0, 0.1)
    ref.backward()
    pd = pred.to(cuda).requires_grad_(True)
    loss = SigmoidFocalLoss(255, 2.0, 0.1)(pd, tgt.to(cuda))
    loss.backward()
    assert abs(loss.item() - ref.item()) <= 1e-5
    np.testing.assert_allclose(pd.grad.float().cpu().numpy(), pr.grad.numpy(), rtol=1e-2, atol=1e-9)


# P = 1, 255, 257, 4099 elements as [1, 1, 1, P]: one element, one short of / one past a block of 256 threads, several
# blocks with a ragged end.  The logits are randn and asserted to stay inside |x| < 5: the oracle forms 1 - sigmoid(x) in
# fp32 as the reference does and the gradient is proportional to it; one bit of sigmoid(x) (6e-8) is 1e-4 of
# 1 - sigmoid(7.4), so out there the oracle's own rounding reaches the fp32 gradient bound of this file (1e-5 of it at 5).
FOCAL_CASES = [(P, dtype, ltype, False) for P in (1, 255, 257, 4099) for dtype in (torch.float32, torch.bfloat16)
               for ltype in (torch.int64, torch.uint8)] + [(257, torch.float32, torch.int64, True)]


@pytest.mark.parametrize("P,dtype,ltype,all_ignored", FOCAL_CASES)
def test_focal_vs_oracle(cuda, P, dtype, ltype, all_ignored):
    """loss within 1e-5 absolute, gradient rtol 1e-4 (fp32) / 1e-2 (bf16): the bounds of the two tests above.  Every label
    ignored: the loss and the whole gradient are exactly 0 (the mean runs over all P elements, loss_opr.py:40-43)."""
    from torchseg_amd.losses import SigmoidFocalLoss
    g = torch.Generator().manual_seed(P)
    pred = torch.randn(1, 1, 1, P, generator=g).to(dtype)
    assert float(pred.float().abs().max()) < 5.0
    tgt = torch.randint(0, 2, (1, 1, P), generator=g)
    tgt[torch.rand(tgt.shape, generator=g) < 0.1] = 255
    if all_ignored:
        tgt[:] = 255
    pr = pred.float().clone().requires_grad_(True)             # a copy: .float() of an fp32 tensor is the tensor itself
    ref = focal_ref.sigmoid_focal_loss(pr, tgt, 255, 2.0, 0.25)
    ref.backward()
    pd = pred.to(cuda).requires_grad_(True)
    loss = SigmoidFocalLoss(255, 2.0, 0.25)(pd, tgt.to(ltype).to(cuda))
    loss.backward()
    assert pd.grad.dtype == dtype and pd.grad.shape == pred.shape
    got = pd.grad.float().cpu().numpy()
    print("P %d %s: loss %.8f (oracle %.8f), max |dgrad| %.3e" % (P, dtype, loss.item(), ref.item(),
                                                                 float(np.abs(got - pr.grad.numpy()).max())))
    assert abs(loss.item() - ref.item()) <= 1e-5
    if all_ignored:
        assert loss.item() == 0.0 and not got.any()
    elif dtype == torch.float32:
        np.testing.assert_allclose(got, pr.grad.numpy(), rtol=1e-4, atol=1e-8)
    else:
        np.testing.assert_allclose(got, pr.grad.numpy(), rtol=1e-2, atol=1e-9)
