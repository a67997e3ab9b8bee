"""Record what the reference's own FCN-32s computes — its unchanged network.py of voc.fcn32s.R101_v1c on ITS OWN
furnace (base_model/resnet.py, seg_opr/seg_oprs.py), on the CPU with seeded init — for the checks
tests/test_fcn_cpu.py makes where the reference checkout is absent.  Only numbers and names are written (run where the
reference is present):

    tests/golden/fcn_golden.json   state-dict keys and shapes, parameter count, seeded-init fingerprint, the loss at
                                   2 x 3 x 128^2 with Dropout2d at p = 0 and the loss under a seeded Dropout2d mask,
                                   config seed / classes; the ImportFrom statements of train.py / eval.py / dataloader.py
    tests/golden/fcn_golden.npz    a fixed sample of all gradients and the deep stem's first weight gradient

    python tests/golden/make_fcn_golden.py
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

import _fcn  # noqa: E402
import test_dropin_cpu as T  # noqa: E402
from _dropin import REF, have_reference, run_in, stage  # noqa: E402


def stage_on_reference_furnace(tmp, files=("config.py", "network.py")):
    base = os.path.join(tmp, "ref", "TorchSeg")
    d = os.path.join(base, "model", "fcn", _fcn.EXP)
    os.makedirs(d)
    for f in files:
        shutil.copy(os.path.join(REF, "model", "fcn", _fcn.EXP, f), d)
    os.symlink(os.path.join(REF, "furnace"), os.path.join(base, "furnace"))
    return d


def main():
    assert have_reference(), "needs the reference checkout at %s" % REF
    with tempfile.TemporaryDirectory(prefix="tsg_fcn_golden_") as tmp:
        gold = json.loads(run_in(stage_on_reference_furnace(tmp), _fcn.script("ref")).strip().splitlines()[-1])
        arrays = {"grad_sample": np.asarray(gold.pop("grad_sample"), np.float32),
                  "stem_grad": np.asarray(gold.pop("stem_grad"), np.float32)}
        print("loss %.6f (dropout mask: %.6f), %d parameters" % (gold["loss"], gold["loss_drop"], gold["nparam"]))
        d = stage(os.path.join(tmp, "imports"), "fcn", _fcn.EXP,
                  files=("config.py", "network.py", "train.py", "eval.py", "dataloader.py"))
        gold["imports"] = json.loads(run_in(d, T._IMPORTS % dict(ref=True)).strip().splitlines()[-1])["statements"]
    with open(os.path.join(HERE, "fcn_golden.json"), "w") as fh:
        json.dump(gold, fh)
    np.savez_compressed(os.path.join(HERE, "fcn_golden.npz"), **arrays)


if __name__ == "__main__":
    main()
