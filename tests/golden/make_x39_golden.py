"""Record what the reference's own BiSeNet-X39 computes — its unchanged network.py of cityscapes.bisenet.X39 and
X39.speed on ITS OWN furnace (base_model/xception.py, seg_opr/seg_oprs.py), so that the backbone is pinned to the
reference's code and not to ours — for the checks tests/test_bisenet_x39_cpu.py makes where the reference checkout is
absent.  Only numbers and names are written (run where the reference is present):

    tests/golden/x39_golden.json   per experiment: state-dict keys and shapes, parameter count, seeded-init fingerprint,
                                   loss, the depthwise layers' names, config seed / classes; the ImportFrom statements of
                                   X39's train.py / eval.py / dataloader.py
    tests/golden/x39_golden.npz    per experiment: every depthwise weight gradient and a fixed sample of all gradients

    python tests/golden/make_x39_golden.py
"""
import json
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)

import _x39  # noqa: E402
import test_dropin_cpu as T  # noqa: E402
from _dropin import REF, have_reference, run_in, stage  # noqa: E402


def stage_on_reference_furnace(tmp, exp, files=("config.py", "network.py")):
    base = os.path.join(tmp, exp, "TorchSeg")
    d = os.path.join(base, "model", "bisenet", exp)
    os.makedirs(d)
    for f in files:
        shutil.copy(os.path.join(REF, "model", "bisenet", exp, f), d)
    os.symlink(os.path.join(REF, "furnace"), os.path.join(base, "furnace"))
    return d


def main():
    assert have_reference(), "needs the reference checkout at %s" % REF
    gold, arrays = {}, {}
    with tempfile.TemporaryDirectory(prefix="tsg_x39_golden_") as tmp:
        for exp in _x39.EXPS:
            out = json.loads(run_in(stage_on_reference_furnace(tmp, exp), _x39.script("ref", exp)).strip().splitlines()[-1])
            key = exp.rsplit(".", 1)[-1] if exp.endswith(".speed") else "X39"
            arrays[key + "_dw_grad"] = np.asarray(out.pop("dw_grad"), np.float32)
            arrays[key + "_grad_sample"] = np.asarray(out.pop("grad_sample"), np.float32)
            gold[key] = out
            print(exp, "loss %.6f, %d parameters, %d depthwise layers" % (out["loss"], out["nparam"], len(out["dw_names"])))
        exp = _x39.EXPS[0]
        d = stage(os.path.join(tmp, "imports"), "bisenet", exp,
                  files=("config.py", "network.py", "train.py", "eval.py", "dataloader.py"))
        gold["imports"] = json.loads(run_in(d, T._IMPORTS % dict(ref=True)).strip().splitlines()[-1])["statements"]
    with open(os.path.join(HERE, "x39_golden.json"), "w") as fh:
        json.dump(gold, fh)
    np.savez_compressed(os.path.join(HERE, "x39_golden.npz"), **arrays)


if __name__ == "__main__":
    main()
