"""Record, from the reference checkout, what tests/test_infer_cpu.py checks where the reference is absent.  Only data is
written (run where the reference is present, on the CPU):

    tests/golden/infer_golden.json
        imports    per .speed experiment: the import statements of its unchanged eval.py ([script, module, names]),
                   `from tools.benchmark import compute_speed, stat` included
        stat       per .speed experiment: the per-leaf-module numbers of the reference's counters (compute_flops.py,
                   compute_madd.py, compute_memory.py, loaded as files: the package __init__ imports cv2 / torchprof)
                   for the eval-mode network (nn.BatchNorm2d) on the reference's own furnace at 1x3x64x128 -- name,
                   repr, input / output shape, parameters, MAdd, FLOPs, memory read / written in bytes

    python tests/golden/make_infer_golden.py
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
sys.path.insert(0, HERE)

from _dropin import REF, have_reference, run_in  # noqa: E402
from make_x39_golden import stage_on_reference_furnace  # noqa: E402

EXPS = {"R18": "cityscapes.bisenet.R18.speed", "X39": "cityscapes.bisenet.X39.speed"}
INPUT = (1, 3, 64, 128)

SCRIPT = r'''
import ast, importlib.util, json, os, sys
import numpy as np, torch, torch.nn as nn
from config import config                         # puts <TorchSeg>/furnace on sys.path
import network
bench = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(network.__file__))), "..", "..", "furnace",
                     "tools", "benchmark")
def load(name):
    spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(bench, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m
cf, cm, cme = load("compute_flops"), load("compute_madd"), load("compute_memory")
statements = []
for node in ast.walk(ast.parse(open("eval.py").read())):
    if isinstance(node, ast.ImportFrom) and node.level == 0:
        statements.append(["eval.py", node.module, [a.name for a in node.names]])
    elif isinstance(node, ast.Import):
        statements.extend(["eval.py", a.name, None] for a in node.names)
torch.manual_seed(config.seed)
model = network.BiSeNet(config.num_classes, is_training=False, criterion=None, ohem_criterion=None,
                        pretrained_model=None, norm_layer=nn.BatchNorm2d)
model.eval()
rows = {}
leaves = [(n, m) for n, m in model.named_modules() if n and not list(m.children())]
def hook(name):
    def fn(module, args, out):
        inp = args[0]
        item = inp.detach().numpy().itemsize
        flops, _ = cf.compute_flops(module, inp, out)
        mem = np.array(cme.compute_memory(module, inp, out), dtype=np.int32) * item
        rows[name] = dict(name=name, repr=repr(module), type=type(module).__name__,
                          input_shape=list(inp.shape), output_shape=list(out.shape),
                          params=int(sum(p.numel() for p in module._parameters.values() if p is not None)),
                          MAdd=int(cm.compute_madd(module, inp, out)), Flops=int(flops),
                          MemRead=int(mem[0]), MemWrite=int(mem[1]))
    return fn
for n, m in leaves:
    m.register_forward_hook(hook(n))
with torch.no_grad():
    model(torch.rand(*%(input)r))
print(json.dumps(dict(imports=statements, stat=[rows[n] for n, _ in leaves if n in rows])))
'''


def main():
    assert have_reference(), "needs the reference checkout at %s" % REF
    gold = {"input_size": list(INPUT), "imports": {}, "stat": {}}
    with tempfile.TemporaryDirectory(prefix="tsg_infer_golden_") as tmp:
        for key, exp in EXPS.items():
            d = stage_on_reference_furnace(tmp, exp, files=("config.py", "network.py", "eval.py"))
            out = json.loads(run_in(d, SCRIPT % dict(input=INPUT)).strip().splitlines()[-1])
            gold["imports"][key] = out["imports"]
            gold["stat"][key] = out["stat"]
            print(exp, "%d leaf modules, %d statements" % (len(out["stat"]), len(out["imports"])))
    with open(os.path.join(HERE, "infer_golden.json"), "w") as fh:
        json.dump(gold, fh, indent=0)


if __name__ == "__main__":
    main()
