"""CPU: the inference additions -- furnace/tools/benchmark (the import the `.speed` eval.py scripts make, `stat`'s
counting conventions, `compute_speed`'s protocol and log lines) and the window geometry the Evaluator hands to
tsg_seg_tail_accum."""
import json
import logging
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FURNACE = os.path.join(ROOT, "torchseg_amd", "furnace")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _dropin import REF, have_reference, run_in, stage  # noqa: E402

EXPS = {"R18": "cityscapes.bisenet.R18.speed", "X39": "cityscapes.bisenet.X39.speed"}


def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "infer_golden.json")) as fh:
        return json.load(fh)


def _furnace_on_path():
    if FURNACE not in sys.path:
        sys.path.insert(0, FURNACE)


_IMPORTS = r'''
import ast, importlib, json, os, sys
if os.path.exists("eval.py"):
    from config import config                     # puts <TorchSeg>/furnace on sys.path, as the script does first
    statements = []
    for node in ast.walk(ast.parse(open("eval.py").read())):
        if isinstance(node, ast.ImportFrom) and node.level == 0:
            statements.append(["eval.py", node.module, [a.name for a in node.names]])
        elif isinstance(node, ast.Import):
            statements.extend(["eval.py", a.name, None] for a in node.names)
else:
    statements = json.load(open("statements.json"))
missing = []
for script, module, names in statements:
    if module in ("config", "network"):
        continue                                  # the experiment's own files
    try:
        mod = importlib.import_module(module)
    except ImportError as e:
        missing.append("import %s (%s)" % (module, e)); continue
    for name in names or ():
        if name != "*" and not hasattr(mod, name):
            try:
                importlib.import_module(module + "." + name)
            except ImportError:
                missing.append("from %s import %s" % (module, name))
print(json.dumps(dict(missing=missing, statements=statements)))
'''


@pytest.mark.parametrize("key", sorted(EXPS))
def test_every_import_of_the_speed_eval_scripts_resolves(tmp_path, key):
    """`from tools.benchmark import compute_speed, stat` (eval.py:17 of both .speed experiments) and every other import
    of the unchanged eval.py resolve against our furnace/."""
    if have_reference():
        d = stage(tmp_path, "bisenet", EXPS[key], files=("config.py", "network.py", "eval.py"))
        out = json.loads(run_in(d, _IMPORTS).strip().splitlines()[-1])
    else:
        with open(str(tmp_path / "statements.json"), "w") as fh:
            json.dump(_golden()["imports"][key], fh)
        out = json.loads(run_in(str(tmp_path), _IMPORTS, furnace=True).strip().splitlines()[-1])
    assert ["eval.py", "tools.benchmark", ["compute_speed", "stat"]] in out["statements"]
    assert not out["missing"], out["missing"]


def _rows_by_name(rows):
    return {r["module name"]: r for r in rows}


@pytest.mark.parametrize("key", sorted(EXPS))
def test_stat_counters_reproduce_the_reference_numbers(key):
    """Every leaf module the reference's counters measured on the .speed network (1x3x64x128): our counters give the
    same FLOPs, MAdd, memory read / written and parameter count, module by module, rebuilt from the recorded layer."""
    _furnace_on_path()
    from tools.benchmark import compute_flops, compute_madd, compute_memory
    gold = _golden()["stat"][key]
    assert len(gold) > 100
    for g in gold:
        m = eval("nn." + g["repr"], {"nn": nn})
        m.eval()
        inp = torch.zeros(g["input_shape"])
        with torch.no_grad():
            out = m(inp)
        assert list(out.shape) == g["output_shape"], g
        flops, _ = compute_flops(m, inp, out)
        rd, wr = compute_memory(m, inp, out)
        got = dict(Flops=int(flops), MAdd=int(compute_madd(m, inp, out)), MemRead=int(rd) * 4, MemWrite=int(wr) * 4,
                   params=int(sum(p.numel() for p in m._parameters.values() if p is not None)))
        want = {k: g[k] for k in got}
        assert got == want, (g["name"], g["repr"], got, want)


@pytest.mark.parametrize("key", sorted(EXPS))
def test_stat_on_the_speed_network(tmp_path, key):
    """`stat` itself on the unchanged .speed network.py (reference checkout or its staged archive) on our furnace:
    the same leaf modules, shapes and numbers as the golden table."""
    from _dropin import have_staged_reference
    if not have_staged_reference():
        pytest.skip("needs the reference's network.py (checkout or the archive build() stages)")
    d = stage(tmp_path, "bisenet", EXPS[key])
    script = r'''
import json, torch, torch.nn as nn
from config import config
import network
from tools.benchmark import collect
torch.manual_seed(config.seed)
model = network.BiSeNet(config.num_classes, is_training=False, criterion=None, ohem_criterion=None,
                        pretrained_model=None, norm_layer=nn.BatchNorm2d)
print(json.dumps(collect(model, (1, 3, 64, 128))))
'''
    rows = json.loads(run_in(d, script, furnace=True).strip().splitlines()[-1])
    gold = _golden()["stat"][key]
    assert [r["module name"] for r in rows] == [g["name"] for g in gold]
    for r, g in zip(rows, gold):
        assert r["input shape"] == g["input_shape"][1:] and r["output shape"] == g["output_shape"][1:], g["name"]
        assert (r["Flops"], r["MAdd"], r["MemRead(B)"], r["MemWrite(B)"], r["params"]) == \
            (g["Flops"], g["MAdd"], g["MemRead"], g["MemWrite"], g["params"]), g["name"]


def test_stat_report_lists_uncounted_types(capsys):
    _furnace_on_path()
    from tools.benchmark import stat
    net = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1, bias=False), nn.BatchNorm2d(8), nn.ReLU(), nn.Dropout(0.1),
                        nn.AdaptiveAvgPool2d(1), nn.Sigmoid())
    rows = stat(net, (2, 3, 8, 8))
    text = capsys.readouterr().out
    assert [r["type"] for r in rows] == ["Conv2d", "BatchNorm2d", "ReLU", "Dropout", "AdaptiveAvgPool2d", "Sigmoid"]
    assert rows[0]["Flops"] == 3 * 3 * 3 * 8 * 2 * 64 and rows[0]["MAdd"] == (27 + 26) * 8 * 64
    assert rows[3]["Flops"] == rows[3]["MAdd"] == rows[3]["MemRead(B)"] == 0
    assert "Total Flops" in text and "counted as 0: Dropout" in text


def _evaluator_windows(H, W, s, crop, stride_rate):
    _furnace_on_path()
    from engine.evaluator import Evaluator, tail_geometry
    ev = Evaluator(None, 19, [0.5] * 3, [0.2] * 3, None, [s], False, [0])
    img = torch.zeros(H, W, 3, dtype=torch.uint8)
    sh, sw, pad_rows, pad_cols, margin, wins, _ = ev._windows(img, s, crop, stride_rate)
    return sh, sw, pad_rows, pad_cols, margin, wins, tail_geometry


@pytest.mark.parametrize("H,W,s,crop,rate", [(1024, 2048, 1.0, 1024, 2 / 3), (1024, 2048, 0.75, 1024, 2 / 3),
                                             (300, 500, 1.0, 512, 2 / 3), (700, 500, 1.0, 512, 2 / 3),
                                             (97, 211, 1.5, 64, 0.5), (64, 64, 1.0, 64, 2 / 3)])
def test_tail_geometry_selects_what_the_padded_loop_selects(H, W, s, crop, rate):
    """For every window: the dst pixels its (oy, ox, t, l, rows, cols) writes, and the window pixels it reads, equal
    what adding the whole window into the padded map and slicing the margins off afterwards selects -- one window,
    padded one window, and the sliding grid."""
    sh, sw, pad_rows, pad_cols, margin, wins, tail_geometry = _evaluator_windows(H, W, s, crop, rate)
    geom = tail_geometry(wins, margin, sh, sw, crop)
    win_ids = np.arange(crop * crop).reshape(crop, crop)
    for (sy, sx), (oy, ox, t, l, rows, cols) in zip(wins, geom):
        padded = np.full((pad_rows, pad_cols), -1, np.int64)
        padded[sy:sy + crop, sx:sx + crop] = win_ids
        want = padded[margin[0]:pad_rows - margin[1], margin[2]:pad_cols - margin[3]]
        got = np.full((sh, sw), -1, np.int64)
        got[oy:oy + rows, ox:ox + cols] = win_ids[t:t + rows, l:l + cols]
        assert np.array_equal(got, want), ((sy, sx), (oy, ox, t, l, rows, cols))


class _FakeCuda:
    def __init__(self):
        self.syncs = 0
        self.device = None

    def set_device(self, d):
        self.device = d

    def synchronize(self):
        self.syncs += 1


def test_compute_speed_protocol_and_log_lines(monkeypatch, caplog):
    """50 warm-up calls, then `iteration` timed calls under no_grad, and the reference's log lines; the device calls
    are mocked (the model runs on the CPU here)."""
    _furnace_on_path()
    from tools.benchmark import speed
    fake = _FakeCuda()
    monkeypatch.setattr(speed.torch, "cuda", fake)
    monkeypatch.delenv("TSG_INFER", raising=False)
    monkeypatch.delenv("TSG_INFER_GRAPH", raising=False)
    calls = []

    class Tiny(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = nn.Conv2d(3, 4, 1)

        def cuda(self):
            return self

        def forward(self, x):
            calls.append((tuple(x.shape), torch.is_grad_enabled(), self.training))
            return self.conv(x)

    real_randn = torch.randn
    monkeypatch.setattr(speed.torch, "randn", lambda *s, device=None: real_randn(*s))
    caplog.set_level(logging.INFO)
    per_iter = speed.compute_speed(Tiny(), (1, 3, 8, 16), 0, 7)
    assert fake.device == 0
    assert len(calls) == speed.WARMUP + 7
    assert all(c == ((1, 3, 8, 16), False, False) for c in calls)
    assert fake.syncs >= speed.WARMUP + 2 * 7
    text = caplog.text
    assert "=========Speed Testing=========" in text
    assert "Elapsed time: [" in text and "s / 7 iter]" in text
    import re
    m = re.search(r"Speed Time: ([0-9.]+) ms / iter    FPS: ([0-9.]+)", text)
    assert m, text
    assert per_iter > 0 and "torchprof is not installed" in text
