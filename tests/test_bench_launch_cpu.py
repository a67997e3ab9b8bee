"""bench.py's launcher contract, on CPU: `python bench.py --gpus N` with no launcher around it must start N ranks
itself (the driver's single-process command shape), `--gpus N` under a launcher of a different size must refuse,
and the JSON line must be the last line of stdout with n_gpus = the size of the process group that actually ran."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None, timeout=240):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                          env=env, timeout=timeout, cwd=ROOT)


def test_plain_python_gpus2_self_launches_two_ranks():
    r = _run(["--gpus", "2", "--launch-check"])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    last = [l for l in r.stdout.splitlines() if l.strip()][-1]
    out = json.loads(last)
    assert out == {"launch_check": True, "n_gpus": 2, "backend": "gloo", "scaling": "weak", "per_rank_batch": 16,
                   "global_batch": 32, "min_kept": 16 * 1024 * 1024 // 16}


def test_strong_scaling_splits_the_global_batch_like_the_reference():
    """--scaling strong: the reference's setting (bisenet dataloader.py:51-53 batch_size // world_size; train.py:48-49
    min_kept from the per-rank batch): global 16 -> 8 per rank at 2 ranks, min_kept 8 * 1024^2 / 16; a split that leaves a
    rank fewer than 2 images is refused."""
    r = _run(["--gpus", "2", "--launch-check", "--scaling", "strong"])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.strip()][-1])
    assert out["scaling"] == "strong" and out["per_rank_batch"] == 8 and out["global_batch"] == 16
    assert out["min_kept"] == 8 * 1024 * 1024 // 16
    r = _run(["--gpus", "1", "--launch-check", "--scaling", "strong", "--batch", "1"])
    assert r.returncode != 0 and "strong" in r.stderr


def test_world_size_mismatch_is_refused():
    r = _run(["--gpus", "4", "--launch-check"], {"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0
    assert "WORLD_SIZE=1" in r.stderr


def test_defaults_follow_survey_8d():
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert '"--steps", type=int, default=50' in src and '"--warmup", type=int, default=20' in src


def test_full_is_off_by_default():
    """A plain run times the headline only; the side records (CPU baselines, probes, other precisions and networks) need
    --full, and their own options keep their defaults for it."""
    sys.path.insert(0, ROOT)
    import bench
    plain = bench.build_parser().parse_args(["--gpus", "1", "--steps", "5", "--warmup", "2"])
    assert plain.full is False and (plain.steps, plain.warmup) == (5, 2)
    full = bench.build_parser().parse_args(["--full"])
    assert full.full is True
    assert (full.i64_steps, full.ref_steps, full.fp32_steps, full.forced_steps) == (10, 20, 3, 20)
    assert not (full.no_cpu_baseline or full.no_ohem_probe or full.no_psa_probe)


def test_dump_outputs_writes_the_step_results(tmp_path):
    """--dump-outputs: loss, a fixed sample of the parameters and their gradients at the same positions, the floating-point
    buffers; float32 / float64 only, the same sample positions on every call, under 64 MB."""
    import numpy as np
    import torch
    import torch.nn as nn
    sys.path.insert(0, ROOT)
    import bench
    torch.manual_seed(0)
    net = nn.Sequential(nn.Conv2d(3, 8, 3), nn.BatchNorm2d(8), nn.Conv2d(8, 4, 1), nn.Conv2d(4, 4, 1))
    loss = net[:3](torch.randn(2, 3, 8, 8)).square().mean()
    loss.backward()                                  # net[3] gets no gradient: dumped as zeros
    names = bench.dump_outputs(str(tmp_path / "a"), net, loss)
    assert names == ["buffers", "gradients", "loss", "parameters"]
    a = {n: np.load(str(tmp_path / "a" / (n + ".npy"))) for n in names}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    flat = torch.cat([p.detach().reshape(-1) for p in net.parameters()]).numpy()
    assert a["loss"].dtype == np.float64 and a["loss"][0] == float(loss)
    assert a["parameters"].dtype == np.float32 and np.array_equal(a["parameters"], flat)
    assert a["gradients"].dtype == np.float32 and a["gradients"].shape == a["parameters"].shape
    assert np.array_equal(a["gradients"][-(16 + 4):], np.zeros(20, np.float32))
    assert a["buffers"].dtype == np.float64 and a["buffers"].size == 16
    big = nn.Linear(1500, 1500)                      # 2.25 M entries > DUMP_SAMPLE: a seeded sample
    loss = big(torch.randn(2, 1500)).sum()
    loss.backward()
    bench.dump_outputs(str(tmp_path / "b"), big, loss)
    bench.dump_outputs(str(tmp_path / "c"), big, loss)
    idx = bench.dump_sample_index(1500 * 1501)
    assert np.array_equal(idx, bench.dump_sample_index(1500 * 1501)) and 0 < idx.size <= bench.DUMP_SAMPLE
    flat = torch.cat([p.detach().reshape(-1) for p in big.parameters()]).numpy()
    for d in ("b", "c"):
        assert np.array_equal(np.load(str(tmp_path / d / "parameters.npy")), flat[idx])
    assert sum(os.path.getsize(str(tmp_path / "b" / f)) for f in os.listdir(str(tmp_path / "b"))) < 64 << 20
