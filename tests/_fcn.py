"""Shared by tests/test_fcn_cpu.py and tests/golden/make_fcn_golden.py: the script that builds FCN-32s (the unchanged
reference network.py of voc.fcn32s.R101_v1c in the working directory, or our workload builder) on the CPU with
nn.BatchNorm2d under the experiment's seed and train.py's init_weight of the heads, and prints what the checks compare:
state-dict keys and shapes, parameter count, seeded-init fingerprint, the loss of one batch with Dropout2d at p = 0 and
a fixed sample of its gradients, and the loss with Dropout2d at its own p under a seeded mask."""

EXP = "voc.fcn32s.R101_v1c"
B, S = 2, 128

SCRIPT = r'''
import json, numpy as np, torch, torch.nn as nn
MODE, SEED, NCLS = "%(mode)s", %(seed)s, %(ncls)s
if MODE == "ref":
    from config import config           # the experiment's config.py: puts <TorchSeg>/furnace on sys.path
    import network
    SEED, NCLS, FCN = config.seed, config.num_classes, network.FCN
else:
    from torchseg_amd.workloads.fcn import FCN
from utils.init_func import init_weight
B, S = %(B)d, %(S)d
torch.manual_seed(SEED)
criterion = nn.CrossEntropyLoss(reduction='mean', ignore_index=255)        # train.py:45-46
model = FCN(NCLS, criterion=criterion, pretrained_model=None, norm_layer=nn.BatchNorm2d)
init_weight(model.business_layer, nn.init.kaiming_normal_, nn.BatchNorm2d, 1e-5, 0.1,
            mode='fan_out', nonlinearity='relu')                            # train.py:55-57
sd = model.state_dict()
fp = [[k, float(v.double().sum()), float(v.double().square().sum())] for k, v in sd.items()]
g = torch.Generator().manual_seed(0)
x = torch.randn(B, 3, S, S, generator=g)
y = torch.randint(0, NCLS, (B, S, S), generator=g)
y[:, :S // 16] = 255
model.train()
drops = [m for m in model.modules() if isinstance(m, nn.Dropout2d)]
ps = [m.p for m in drops]
for m in drops:
    m.p = 0.0
loss = model(x, y)
loss.backward()
allg = torch.cat([p.grad.reshape(-1) for p in model.parameters()])
idx = torch.from_numpy(np.random.default_rng(0).integers(0, allg.numel(), 65536))
stem = dict(model.named_parameters())["backbone.conv1.0.weight"].grad
for m, p in zip(drops, ps):
    m.p = p
torch.manual_seed(7)
with torch.no_grad():
    loss_drop = model(x, y)
print(json.dumps(dict(keys=[[k, list(v.shape)] for k, v in sd.items()], nparam=sum(p.numel() for p in model.parameters()),
                      fp=fp, loss=loss.item(), loss_drop=loss_drop.item(), dropout_p=ps, grad_sample=allg[idx].tolist(),
                      stem_grad=stem.reshape(-1).tolist(), gmax=allg.abs().max().item(), seed=SEED, ncls=NCLS)))
'''


def script(mode, seed=None, ncls=None):
    return SCRIPT % dict(mode=mode, seed=seed, ncls=ncls, B=B, S=S)


def ce_upsample_ref64(z, target, size, ignore_index=255):
    """float64 oracle of the FCN head: nn.CrossEntropyLoss(ignore_index)(F.interpolate(z, size, bilinear,
    align_corners=True), target) on the CPU -> (loss, dL/dz)."""
    import torch
    import torch.nn.functional as F
    zr = z.detach().double().cpu().requires_grad_(True)
    logits = F.interpolate(zr, size=size, mode="bilinear", align_corners=True)
    loss = F.cross_entropy(logits, target.cpu(), ignore_index=ignore_index, reduction="mean")
    loss.backward()
    return loss.detach(), zr.grad
