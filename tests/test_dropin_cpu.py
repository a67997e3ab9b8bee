"""CPU plumbing (BASELINE config 1): the reference's UNCHANGED network.py files
import against our furnace/ + shims and run one forward/backward; our BiSeNet
workload builder is the same network (same init under a seed, same loss).
Where the reference checkout is absent, every test checks our side against what
the reference's own files computed in the same script, stored under
tests/golden/ (dropin_golden.*, written by tests/golden/make_dropin_golden.py)."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

from _dropin import GOLDEN, REF, ROOT, golden, have_reference, run_in, stage

# What every script below prints about a network: the state-dict keys, a per-tensor fingerprint of the seeded init
# (float64 sum and sum of squares) and a fixed sample of the flattened gradients.
_FINGERPRINT = r'''
import numpy as np
def fingerprint(sd):
    return [[k, float(v.double().sum()), float(v.double().square().sum())] for k, v in sd.items()]
def grad_sample(params, n=65536):
    g = torch.cat([p.grad.reshape(-1) for p in params])
    idx = torch.from_numpy(np.random.default_rng(0).integers(0, g.numel(), n))
    return g[idx].tolist()
'''

# REF: the staged reference experiment (its config.py + network.py); otherwise our workload builder alone, with the
# reference config values the golden file holds (CFG).
_SOURCES = r'''
import types
REF = %(ref)s
if REF:
    from config import config            # unchanged reference config.py (adds furnace/ to sys.path)
    import network                       # unchanged reference network.py
else:
    config = types.SimpleNamespace(**%(cfg)s)
'''


def _fingerprints_equal(ours, ref):
    assert [k for k, _, _ in ours] == [k for k, _, _ in ref], "state-dict keys differ"
    for (k, s, q), (_, rs, rq) in zip(ours, ref):
        assert abs(s - rs) <= 1e-6 * max(1.0, abs(rs)) and abs(q - rq) <= 1e-6 * max(1.0, abs(rq)), (k, s, rs, q, rq)


_BISENET = _SOURCES + _FINGERPRINT + r'''
import json, sys, torch, torch.nn as nn
from oracle.ohem_ref import ProbOhemCrossEntropy2d
from torchseg_amd.workloads.bisenet import BiSeNet as Ours
def build(cls):
    torch.manual_seed(config.seed)
    crit = ProbOhemCrossEntropy2d(ignore_label=255, thresh=0.7, min_kept=2*96*96//16, use_weight=False)
    return cls(config.num_classes, is_training=True, criterion=crit, pretrained_model=None, norm_layer=nn.BatchNorm2d)
ours = build(Ours)
ref = build(network.BiSeNet) if REF else None
sd_o = ours.state_dict()
if REF:
    sd_r = ref.state_dict()
    assert list(sd_r.keys()) == list(sd_o.keys())
    assert all(torch.equal(sd_r[k], sd_o[k]) for k in sd_r), "seeded init differs"
fp = fingerprint(sd_o)
g = torch.Generator().manual_seed(0)
x = torch.randn(2, 3, 96, 96, generator=g); y = torch.randint(0, 19, (2, 96, 96), generator=g); y[:, :8] = 255
lo = ours(x, y)
lo.backward()
go = torch.cat([p.grad.reshape(-1) for p in ours.parameters()])
out = dict(loss_ours=lo.item(), fp=fp, sample_ours=grad_sample(list(ours.parameters())),
           nparam_ours=sum(p.numel() for p in ours.parameters()))
if REF:
    lr = ref(x, y)
    lr.backward()
    gr = torch.cat([p.grad.reshape(-1) for p in ref.parameters()])
    out.update(loss_ref=lr.item(), gdiff=(gr-go).abs().max().item(), gmax=gr.abs().max().item(),
               nparam=sum(p.numel() for p in ref.parameters()), sample_ref=grad_sample(list(ref.parameters())),
               cfg=dict(seed=config.seed, num_classes=config.num_classes))
print(json.dumps(out))
'''


def test_bisenet_reference_network_runs_and_matches_workload(tmp_path):
    if have_reference():
        d = stage(tmp_path, "bisenet", "cityscapes.bisenet.R18")
        out = json.loads(run_in(d, _BISENET % dict(ref=True, cfg=None)).strip().splitlines()[-1])
    else:
        gold = golden()
        g = gold["bisenet"]
        out = json.loads(run_in(str(tmp_path), _BISENET % dict(ref=False, cfg=repr(g["cfg"])),
                                furnace=True).strip().splitlines()[-1])
        _fingerprints_equal(out["fp"], g["fp"])
        sample_ref = gold["arrays"]["bisenet_grad_sample"]
        out.update(loss_ref=g["loss_ref"], nparam=g["nparam"], gmax=g["gmax"],
                   gdiff=float(np.abs(np.asarray(out["sample_ours"]) - sample_ref).max()))
    assert out["nparam"] == out["nparam_ours"] == 13494777
    assert abs(out["loss_ref"] - out["loss_ours"]) <= 1e-5 * abs(out["loss_ref"])
    assert out["gdiff"] <= 1e-4 * out["gmax"]


_FAMILY = _SOURCES + r'''
import json, torch, torch.nn as nn
torch.manual_seed(1)
crit = nn.CrossEntropyLoss(reduction='mean', ignore_index=-1)
kind = "%(kind)s"
if not REF:
    from torchseg_amd.workloads.dfn import DFN
    from torchseg_amd.workloads.pspnet import PSPNet, PSANet
    network = types.SimpleNamespace(DFN=DFN, PSPNet={"pspnet": PSPNet, "psanet": PSANet}.get(kind))
    if kind != "dfn":
        network.PSPNet = (lambda cls: lambda n, **kw: cls(n, kw["criterion"], kw["pretrained_model"], kw["norm_layer"],
                                                          depth=50))(network.PSPNet)
if kind == "dfn":
    from oracle.focal_ref import SigmoidFocalLoss
    model = network.DFN(config.num_classes, criterion=nn.CrossEntropyLoss(ignore_index=255),
                        aux_criterion=SigmoidFocalLoss(ignore_label=255, gamma=2.0, alpha=0.25),
                        alpha=config.aux_loss_alpha, pretrained_model=None, norm_layer=nn.BatchNorm2d)
    S = 64
    x = torch.randn(2, 3, S, S); y = torch.randint(0, config.num_classes, (2, S, S)); e = torch.randint(0, 2, (2, S, S))
    loss = model(x, y, e)
else:
    model = network.PSPNet(config.num_classes, criterion=crit, pretrained_model=None, norm_layer=nn.BatchNorm2d)
    S = 480 if kind == "psanet" else 96
    B = 1 if kind == "psanet" else 2
    x = torch.randn(B, 3, S, S); y = torch.randint(0, config.num_classes, (B, S, S))
    if kind == "psanet":
        model.eval()      # BN over a batch of 1 at 1x1 pooling is undefined in train mode; plumbing only
        for p in model.parameters(): p.requires_grad_(True)
    loss = model(x, y)
loss.backward()
nograd = [n for n, p in model.named_parameters() if p.grad is None]
cfg = dict(num_classes=config.num_classes, aux_loss_alpha=getattr(config, "aux_loss_alpha", None))
print(json.dumps(dict(loss=loss.item(), nparam=sum(p.numel() for p in model.parameters()), nograd=len(nograd), cfg=cfg)))
'''


@pytest.mark.parametrize("family,exp,kind,nparam", [
    ("pspnet", "ade.pspnet.R50_v1c", "pspnet", None),
    ("dfn", "cityscapes.dfn.R101_v1c", "dfn", None),
    ("psanet", "ade.psanet.R50_v1c", "psanet", None),
])
def test_other_families_import_and_step(tmp_path, family, exp, kind, nparam):
    if have_reference():
        d = stage(tmp_path, family, exp)
        out = json.loads(run_in(d, _FAMILY % dict(ref=True, cfg=None, kind=kind), timeout=900).strip().splitlines()[-1])
    else:
        # our builder of the family through the same script: the reference's parameter count, unused parameters and
        # loss (same seed, same draws)
        g = golden()["family_step"][kind]
        out = json.loads(run_in(str(tmp_path), _FAMILY % dict(ref=False, cfg=repr(g["cfg"]), kind=kind), timeout=900,
                                furnace=True).strip().splitlines()[-1])
        assert out["nparam"] == g["nparam"] and out["nograd"] == g["nograd"], (out, g)
        assert abs(out["loss"] - g["loss"]) <= 1e-5 * max(1.0, abs(g["loss"])), (out["loss"], g["loss"])
    assert np.isfinite(out["loss"])
    if kind == "dfn":
        assert out["nograd"] == 5      # statically unused params: DDP must tolerate them


_WORKLOAD_EQ = _SOURCES + _FINGERPRINT + r'''
import json, torch, torch.nn as nn
kind = "%(kind)s"
def build(ref):
    torch.manual_seed(3)
    crit = nn.CrossEntropyLoss(reduction='mean', ignore_index=-1)
    if kind == "dfn":
        from oracle.focal_ref import SigmoidFocalLoss
        args = dict(criterion=nn.CrossEntropyLoss(ignore_index=255), aux_criterion=SigmoidFocalLoss(255, 2.0, 0.25),
                    alpha=config.aux_loss_alpha, pretrained_model=None, norm_layer=nn.BatchNorm2d)
        if ref:
            return network.DFN(config.num_classes, **args)
        from torchseg_amd.workloads.dfn import DFN
        return DFN(config.num_classes, **args)
    if ref:
        return network.PSPNet(config.num_classes, criterion=crit, pretrained_model=None, norm_layer=nn.BatchNorm2d)
    from torchseg_amd.workloads.pspnet import PSPNet, PSANet
    cls = PSPNet if kind == "pspnet" else PSANet
    return cls(config.num_classes, crit, None, nn.BatchNorm2d, depth=50)
ours = build(False)
so = ours.state_dict()
fp = fingerprint(so)
ours.eval()                        # dropout off, running stats: deterministic comparison
if REF:
    ref = build(True)
    sr = ref.state_dict()
    assert list(sr.keys()) == list(so.keys()), [k for k in sr if k not in so][:5]
    assert all(torch.equal(sr[k], so[k]) for k in sr), "seeded init differs"
    ref.eval()
g = torch.Generator().manual_seed(1)
if kind == "dfn":
    x = torch.randn(1, 3, 64, 64, generator=g); y = torch.randint(0, config.num_classes, (1, 64, 64), generator=g)
    e = torch.randint(0, 2, (1, 64, 64), generator=g)
    lo = ours(x, y, e)
    lr = ref(x, y, e) if REF else None
else:
    S = 480 if kind == "psanet" else 96
    x = torch.randn(1, 3, S, S, generator=g); y = torch.randint(0, config.num_classes, (1, S, S), generator=g)
    lo = ours(x, y)
    lr = ref(x, y) if REF else None
print(json.dumps(dict(loss_ref=None if lr is None else lr.item(), loss_ours=lo.item(), nkeys=len(so), fp=fp)))
'''


@pytest.mark.parametrize("family,exp,kind", [
    ("pspnet", "ade.pspnet.R50_v1c", "pspnet"),
    ("dfn", "cityscapes.dfn.R101_v1c", "dfn"),
    ("psanet", "ade.psanet.R50_v1c", "psanet"),
])
def test_workload_builders_equal_reference_networks(tmp_path, family, exp, kind):
    """torchseg_amd/workloads/{pspnet,dfn}.py are the reference networks: same state-dict keys,
    identical seeded init, identical loss."""
    if have_reference():
        d = stage(tmp_path, family, exp)
        out = json.loads(run_in(d, _WORKLOAD_EQ % dict(ref=True, cfg=None, kind=kind),
                                timeout=900).strip().splitlines()[-1])
    else:
        g = golden()["workload_eq"][kind]
        cfg = golden()["family_step"][kind]["cfg"]
        out = json.loads(run_in(str(tmp_path), _WORKLOAD_EQ % dict(ref=False, cfg=repr(cfg), kind=kind), timeout=900,
                                furnace=True).strip().splitlines()[-1])
        _fingerprints_equal(out["fp"], g["fp"])
        out["loss_ref"] = g["loss_ref"]
    assert abs(out["loss_ref"] - out["loss_ours"]) <= 1e-5 * max(1.0, abs(out["loss_ref"])), out


_CKPT_COMMON = r'''
import sys, types, json, torch, torch.nn as nn
def make():
    torch.manual_seed(5)
    m = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.BatchNorm2d(8), nn.ReLU(), nn.Conv2d(8, 4, 1))
    return m
def groups(m):
    return [dict(params=[p for p in m.parameters() if p.dim() > 1], lr=0.05),
            dict(params=[p for p in m.parameters() if p.dim() <= 1], lr=0.5, weight_decay=0.0)]
def digest(m, opt):
    sd = opt.state_dict()
    return dict(params=[float(p.double().sum()) for p in m.parameters()],
                bufs=[float(b.double().sum()) for b in m.buffers()],
                mom=[float(sd['state'][k]['momentum_buffer'].double().sum()) for k in sorted(sd['state'])],
                mom_shapes=[list(sd['state'][k]['momentum_buffer'].shape) for k in sorted(sd['state'])],
                lrs=[g['lr'] for g in sd['param_groups']])
class Wrapped(nn.Module):            # what apex / our DDP wrapper looks like to the state dict: 'module.' prefix
    def __init__(self, m):
        super().__init__(); self.module = m
'''

_CKPT_REF_WRITE = _CKPT_COMMON + r'''
sys.path.insert(0, "%(ref)s/furnace")
import utils.pyt_utils
from engine.engine import Engine, State
m = make(); opt = torch.optim.SGD(groups(m), lr=0.05, momentum=0.9, weight_decay=5e-4)
for _ in range(2):
    opt.zero_grad(); m(torch.randn(2, 3, 8, 8)).square().mean().backward(); opt.step()
st = State(); st.register(model=Wrapped(m), optimizer=opt); st.epoch = 3; st.iteration = 77
Engine.save_checkpoint(types.SimpleNamespace(state=st), sys.argv[1])
print(json.dumps(digest(m, opt)))
'''

_CKPT_OURS = _CKPT_COMMON + r'''
from engine.engine import Engine, State          # torchseg_amd/furnace (cwd-staged path)
from torchseg_amd.optim import FusedSGD
m = make()
for p in m.parameters():
    p.data.add_(1.0)                             # make sure the restore really overwrites
m[3].weight.data = m[3].weight.data.contiguous(memory_format=torch.channels_last)
opt = FusedSGD(groups(m), lr=0.01, momentum=0.9, weight_decay=5e-4)
st = State(); st.register(model=Wrapped(m), optimizer=opt)
eng = types.SimpleNamespace(state=st, continue_state_object=sys.argv[1], distributed=True)
Engine.restore_checkpoint(eng)
assert st.epoch == 4 and st.iteration == 77, (st.epoch, st.iteration)
Engine.save_checkpoint(eng, sys.argv[2])
print(json.dumps(digest(st.model.module, opt)))
'''

_CKPT_REF_READ = _CKPT_COMMON + r'''
sys.path.insert(0, "%(ref)s/furnace")
import utils.pyt_utils
from engine.engine import Engine, State
m = make(); opt = torch.optim.SGD(groups(m), lr=0.01, momentum=0.9, weight_decay=5e-4)
st = State(); st.register(model=Wrapped(m), optimizer=opt)
eng = types.SimpleNamespace(state=st, continue_state_object=sys.argv[1], distributed=True)
Engine.restore_checkpoint(eng)
assert st.epoch == 5 and st.iteration == 77
opt.zero_grad(); m(torch.ones(1, 3, 8, 8)).square().mean().backward(); opt.step()    # the restored state is usable
print(json.dumps(digest(m, opt)))
'''

# Without the reference Engine: its restore (engine.py: torch.load, 'module.'-prefix-aware load of 'model', the
# optimizer's load_state_dict, epoch + 1) done with plain torch on a checkpoint whose layout (keys, types, tensor shapes)
# must equal the one the reference Engine wrote.
_CKPT_PLAIN_READ = _CKPT_COMMON + r'''
def layout(o):
    if isinstance(o, dict):
        return {str(k): layout(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [layout(v) for v in o]
    if torch.is_tensor(o):
        return ["tensor", str(o.dtype), list(o.shape)]
    return type(o).__name__
blob = torch.load(sys.argv[1], map_location="cpu")
ref_blob = torch.load(sys.argv[2], map_location="cpu")
assert layout(blob) == layout(ref_blob), (layout(blob), layout(ref_blob))
m = make(); opt = torch.optim.SGD(groups(m), lr=0.01, momentum=0.9, weight_decay=5e-4)
m.load_state_dict(blob["model"])
opt.load_state_dict(blob["optimizer"])
assert blob["epoch"] + 1 == 5 and blob["iteration"] == 77
opt.zero_grad(); m(torch.ones(1, 3, 8, 8)).square().mean().backward(); opt.step()    # the restored state is usable
print(json.dumps(digest(m, opt)))
'''


def test_checkpoints_interchange_with_reference_engine(tmp_path):
    """a checkpoint written by the reference Engine (torch SGD, 'module.'-stripped keys) restores
    into our Engine + FusedSGD, and the checkpoint our Engine writes restores into the reference's.  Without the
    reference: the checkpoint its Engine wrote (tests/golden/dropin_ckpt_ref.pth) and the digest of that run."""
    import subprocess
    import sys as _sys
    ref_ckpt, our_ckpt = str(tmp_path / "ref.pth"), str(tmp_path / "ours.pth")
    d = stage(tmp_path, "bisenet", "cityscapes.bisenet.R18") if have_reference() else str(tmp_path)

    def run(script, *args, ours):
        env = dict(os.environ)
        env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "torchseg_amd", "shims")]
                                            + ([os.path.join(ROOT, "torchseg_amd", "furnace")] if ours else []))
        r = subprocess.run([_sys.executable, "-c", script, *args], cwd=d, env=env, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + "\n" + r.stderr[-3000:]
        return json.loads(r.stdout.strip().splitlines()[-1])

    if have_reference():
        a = run(_CKPT_REF_WRITE % dict(ref=REF), ref_ckpt, ours=False)
    else:
        shutil.copy(os.path.join(GOLDEN, "dropin_ckpt_ref.pth"), ref_ckpt)
        a = golden()["checkpoint"]
    b = run(_CKPT_OURS, ref_ckpt, our_ckpt, ours=True)
    for k in ("params", "bufs", "mom", "mom_shapes", "lrs"):
        assert a[k] == b[k], (k, a[k], b[k])
    if have_reference():
        c = run(_CKPT_REF_READ % dict(ref=REF), our_ckpt, ours=False)
    else:
        c = run(_CKPT_PLAIN_READ, our_ckpt, ref_ckpt, ours=False)
    assert c["mom_shapes"] == a["mom_shapes"] and c["lrs"] == a["lrs"]


_IMPORTS = r'''
import ast, importlib, json, os, sys
REF = %(ref)s
if REF:
    from config import config                     # puts <TorchSeg>/furnace on sys.path, as the scripts do first
    statements = []
    for script in ("train.py", "eval.py", "dataloader.py"):
        if not os.path.exists(script):
            continue
        tree = ast.parse(open(script).read())
        for node in ast.walk(tree):
            if isinstance(node, ast.ImportFrom) and node.level == 0:
                if node.module.split(".")[0] in ("tools",):  # tools/benchmark of the .speed variants: out of scope
                    continue
                statements.append([script, node.module, [a.name for a in node.names]])
            elif isinstance(node, ast.Import):
                statements.extend([script, a.name, None] for a in node.names)
else:
    statements = json.load(open("statements.json"))    # the same statements, recorded from the reference's files
missing, local = [], []
for script, module, names in statements:
    try:
        mod = importlib.import_module(module)
    except ImportError as e:
        if module.startswith("apex"):
            raise
        missing.append("%%s: import %%s (%%s)" %% (script, module, e)); continue
    if REF and os.path.dirname(os.path.abspath(getattr(mod, "__file__", None) or "/")) == os.getcwd():
        local.append(module)                      # the experiment's own config / network / dataloader
    for name in names or ():
        if name != "*" and not hasattr(mod, name):
            try:
                importlib.import_module(module + "." + name)
            except ImportError:
                missing.append("%%s: from %%s import %%s" %% (script, module, name))
print(json.dumps(dict(missing=missing, statements=[s for s in statements if s[1] not in local])))
'''


@pytest.mark.parametrize("family,exp", [("bisenet", "cityscapes.bisenet.R18"), ("dfn", "cityscapes.dfn.R101_v1c"),
                                        ("pspnet", "ade.pspnet.R50_v1c"), ("psanet", "ade.psanet.R50_v1c")])
def test_every_import_of_the_unchanged_scripts_resolves(tmp_path, family, exp):
    """INTEGRATION.md's drop-in step must not end in an ImportError: every `import` / `from ... import name` of the
    UNCHANGED train.py, eval.py and dataloader.py of each family resolves against our furnace/ (+ the apex / easydict
    shims, + the cv2 stand-in only because this image has no OpenCV).  Without the reference: the same statements,
    recorded from those files (the experiment's own modules left out), against our furnace/ on the path."""
    if have_reference():
        files = [f for f in ("config.py", "network.py", "train.py", "eval.py", "dataloader.py")
                 if os.path.exists(os.path.join(REF, "model", family, exp, f))]
        d = stage(tmp_path, family, exp, files=files)
        out = json.loads(run_in(d, _IMPORTS % dict(ref=True)).strip().splitlines()[-1])
    else:
        with open(str(tmp_path / "statements.json"), "w") as fh:
            json.dump(golden()["imports"][family], fh)
        out = json.loads(run_in(str(tmp_path), _IMPORTS % dict(ref=False), furnace=True).strip().splitlines()[-1])
    assert out["statements"]
    assert not out["missing"], out["missing"]


_TRAINPRE = r'''
import json, random, numpy as np
from config import config
from dataloader import TrainPre                   # the UNCHANGED reference class, running on OUR utils.img_utils
sys_path_ok = True
rng = np.random.RandomState(0)
img = rng.randint(0, 256, size=(96, 160, 3)).astype(np.uint8)
gt = rng.randint(0, 19, size=(96, 160)).astype(np.uint8)
config.image_height, config.image_width = 64, 80
config.train_scale_array = [0.75, 1.0, 1.5]
pre = TrainPre(config.image_mean, config.image_std)
random.seed(3)
p_img, p_gt, extra = pre(img, gt)
from oracle import augment_ref as R
random.seed(3)
par = R.draw_params(img.shape[:2], config.train_scale_array, (64, 80))
w_img, w_gt = R.train_pre(img, gt, par, config.image_mean, config.image_std, (64, 80))
print(json.dumps(dict(shape=list(p_img.shape), gt_equal=bool(np.array_equal(p_gt, w_gt)),
                      frac_off=float((np.abs(p_img - w_img) > 1e-5).mean()), max_off=float(np.abs(p_img - w_img).max()),
                      mean=np.asarray(config.image_mean).tolist(), std=np.asarray(config.image_std).tolist(),
                      p_img=np.asarray(p_img, np.float32).reshape(-1).tolist(), p_gt=np.asarray(p_gt).reshape(-1).tolist())))
'''


def test_unchanged_trainpre_runs_on_our_img_utils_and_equals_the_oracle(tmp_path):
    """The reference's own TrainPre (bisenet dataloader.py:11-35), unchanged, on our utils.img_utils: same sample as the
    step-by-step oracle the GPU pipeline is tested against (labels equal; image equal up to uint8 .5 ties).  Without the
    reference: the oracle against the sample that TrainPre produced (tests/golden)."""
    if have_reference():
        d = stage(tmp_path, "bisenet", "cityscapes.bisenet.R18", files=("config.py", "network.py", "dataloader.py"))
        out = json.loads(run_in(d, _TRAINPRE).strip().splitlines()[-1])
    else:
        import random
        from oracle import augment_ref as R
        g, arrays = golden()["trainpre"], golden()["arrays"]
        rng = np.random.RandomState(0)
        img = rng.randint(0, 256, size=(96, 160, 3)).astype(np.uint8)
        gt = rng.randint(0, 19, size=(96, 160)).astype(np.uint8)
        random.seed(3)
        par = R.draw_params(img.shape[:2], [0.75, 1.0, 1.5], (64, 80))
        w_img, w_gt = R.train_pre(img, gt, par, np.asarray(g["mean"]), np.asarray(g["std"]), (64, 80))
        p_img, p_gt = arrays["trainpre_img"], arrays["trainpre_gt"]
        out = dict(shape=list(p_img.shape), gt_equal=bool(np.array_equal(p_gt, w_gt)),
                   frac_off=float((np.abs(p_img - w_img) > 1e-5).mean()), max_off=float(np.abs(p_img - w_img).max()))
    assert out["shape"] == [3, 64, 80] and out["gt_equal"]
    assert out["frac_off"] <= 1e-3 and out["max_off"] <= (1 / 255) / 0.224 + 1e-5


_TABLES = r"""
import json
REF = %(ref)s
if REF:
    from config import config
from datasets import Cityscapes, VOC
def ref(path, name):
    src = open(path).read().replace("from datasets.BaseDataset import BaseDataset", "BaseDataset = object")
    ns = {}
    exec(compile(src.split("if __name__")[0], path, "exec"), ns)
    return ns[name]
if REF:
    RC = ref("%(ref_dir)s/furnace/datasets/cityscapes/cityscapes.py", "Cityscapes")
    RV = ref("%(ref_dir)s/furnace/datasets/voc/voc.py", "VOC")
    tables = dict(city_colors=RC.get_class_colors(), city_names=RC.get_class_names(), city_trans=RC.trans_labels,
                  voc_colors=RV.get_class_colors(), voc_names=RV.get_class_names())
    assert (Cityscapes.get_class_colors() == RC.get_class_colors() and Cityscapes.get_class_names() == RC.get_class_names()
            and Cityscapes.trans_labels == RC.trans_labels and VOC.get_class_colors() == RV.get_class_colors()
            and VOC.get_class_names() == RV.get_class_names())
else:
    tables = json.load(open("tables.json"))
tables = json.loads(json.dumps(tables))                 # the JSON form either way (tuples -> lists)
ours = json.loads(json.dumps(dict(city_colors=Cityscapes.get_class_colors(), city_names=Cityscapes.get_class_names(),
                                  city_trans=Cityscapes.trans_labels, voc_colors=VOC.get_class_colors(),
                                  voc_names=VOC.get_class_names())))
print(json.dumps(dict(city=all(ours[k] == tables[k] for k in ("city_colors", "city_names", "city_trans")),
                      voc=all(ours[k] == tables[k] for k in ("voc_colors", "voc_names")), tables=tables)))
"""


def test_dataset_tables_match_the_reference(tmp_path):
    if have_reference():
        d = stage(tmp_path, "bisenet", "cityscapes.bisenet.R18")
        out = json.loads(run_in(d, _TABLES % dict(ref=True, ref_dir=REF)).strip().splitlines()[-1])
    else:
        with open(str(tmp_path / "tables.json"), "w") as fh:
            json.dump(golden()["tables"], fh)
        out = json.loads(run_in(str(tmp_path), _TABLES % dict(ref=False, ref_dir=None),
                                furnace=True).strip().splitlines()[-1])
    assert (out["city"], out["voc"]) == (True, True)
