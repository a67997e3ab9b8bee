"""Record what the reference's own experiment files compute in the scripts of tests/test_dropin_cpu.py and
tests/test_cpu_reference.py, for the checks those tests make where the reference checkout is absent (run where it is
present; nothing of the reference is copied, only the numbers, names and tables its code produced).  Output (committed):

    tests/golden/dropin_golden.json   losses, parameter counts, state-dict fingerprints, config values, import
                                      statements, dataset tables, the checkpoint digest, the CPU reference leg's loss
    tests/golden/dropin_golden.npz    the BiSeNet gradient sample, the TrainPre sample
    tests/golden/dropin_ckpt_ref.pth  the checkpoint the reference Engine writes

    python tests/golden/make_dropin_golden.py
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)

import test_dropin_cpu as T  # noqa: E402
from _dropin import REF, ROOT, have_reference, run_in, stage  # noqa: E402

FAMILIES = {"pspnet": ("pspnet", "ade.pspnet.R50_v1c"), "dfn": ("dfn", "cityscapes.dfn.R101_v1c"),
            "psanet": ("psanet", "ade.psanet.R50_v1c")}
IMPORTS = (("bisenet", "cityscapes.bisenet.R18"), ("dfn", "cityscapes.dfn.R101_v1c"), ("pspnet", "ade.pspnet.R50_v1c"),
           ("psanet", "ade.psanet.R50_v1c"))


def last_json(text):
    return json.loads(text.strip().splitlines()[-1])


def main():
    assert have_reference(), "needs the reference checkout at %s" % REF
    gold, arrays = {}, {}
    with tempfile.TemporaryDirectory(prefix="tsg_golden_") as tmp:
        def fresh(name):
            p = os.path.join(tmp, name)
            os.makedirs(p)
            return p

        out = last_json(run_in(stage(fresh("bisenet"), "bisenet", "cityscapes.bisenet.R18"),
                               T._BISENET % dict(ref=True, cfg=None)))
        gold["bisenet"] = dict(loss_ref=out["loss_ref"], nparam=out["nparam"], gmax=out["gmax"], fp=out["fp"],
                               cfg=out["cfg"])
        arrays["bisenet_grad_sample"] = np.asarray(out["sample_ref"], np.float32)

        gold["family_step"], gold["workload_eq"] = {}, {}
        for kind, (family, exp) in FAMILIES.items():
            out = last_json(run_in(stage(fresh("f_" + kind), family, exp), T._FAMILY % dict(ref=True, cfg=None, kind=kind),
                                   timeout=900))
            gold["family_step"][kind] = out
            out = last_json(run_in(stage(fresh("w_" + kind), family, exp),
                                   T._WORKLOAD_EQ % dict(ref=True, cfg=None, kind=kind), timeout=900))
            gold["workload_eq"][kind] = dict(loss_ref=out["loss_ref"], fp=out["fp"])

        d = stage(fresh("ckpt"), "bisenet", "cityscapes.bisenet.R18")
        env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "torchseg_amd", "shims")]))
        ckpt = os.path.join(HERE, "dropin_ckpt_ref.pth")
        r = subprocess.run([sys.executable, "-c", T._CKPT_REF_WRITE % dict(ref=REF), ckpt], cwd=d, env=env,
                           capture_output=True, text=True, timeout=600, check=True)
        gold["checkpoint"] = last_json(r.stdout)
        import torch
        torch.load(ckpt, map_location="cpu", weights_only=True)      # plain data: tensors, dicts, numbers

        gold["imports"] = {}
        for family, exp in IMPORTS:
            files = [f for f in ("config.py", "network.py", "train.py", "eval.py", "dataloader.py")
                     if os.path.exists(os.path.join(REF, "model", family, exp, f))]
            out = last_json(run_in(stage(fresh("i_" + family), family, exp, files=files), T._IMPORTS % dict(ref=True)))
            assert not out["missing"], out["missing"]
            gold["imports"][family] = out["statements"]

        out = last_json(run_in(stage(fresh("trainpre"), "bisenet", "cityscapes.bisenet.R18",
                                     files=("config.py", "network.py", "dataloader.py")), T._TRAINPRE))
        gold["trainpre"] = dict(mean=out["mean"], std=out["std"])
        arrays["trainpre_img"] = np.asarray(out["p_img"], np.float32).reshape(out["shape"])
        arrays["trainpre_gt"] = np.asarray(out["p_gt"]).astype(np.uint8).reshape(out["shape"][1:])

        out = last_json(run_in(stage(fresh("tables"), "bisenet", "cityscapes.bisenet.R18"),
                               T._TABLES % dict(ref=True, ref_dir=REF)))
        gold["tables"] = out["tables"]

    # tests/test_cpu_reference.py: the reference's own furnace + network.py on the host (tools/cpu_reference.py)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "cpu_reference.py"), "--size", "128", "--batch", "2",
                        "--budget", "0.5", "--max-steps", "1", "--threads", "4", "--check"], capture_output=True,
                       text=True, timeout=300, check=True)
    rec = json.loads([line for line in r.stdout.splitlines() if line.startswith("{")][-1])
    gold["cpu_reference"] = dict(params=rec["params"], first_loss=rec["first_loss"])

    with open(os.path.join(HERE, "dropin_golden.json"), "w") as fh:
        json.dump(gold, fh, indent=0, sort_keys=True)
        fh.write("\n")
    np.savez_compressed(os.path.join(HERE, "dropin_golden.npz"), **arrays)


if __name__ == "__main__":
    main()
