"""compute_speed: the inference-FPS protocol of the `.speed` experiments (eval.py:113): 50 warm-up calls, then
`iteration` calls under no_grad, each bracketed by device synchronisations and timed on the host; the log lines
`Elapsed time: [...]` and `Speed Time: ... FPS: ...`.

By default the model runs as given.  TSG_INFER=1 runs it through torchseg_amd.infer.prepare_inference (our kernels,
bf16 autocast unless TSG_DTYPE=fp32); TSG_INFER_GRAPH=1 additionally replays it as one captured graph per input shape.
The per-module profiler table the reference prints after the timing needs `torchprof`, which is not a dependency here:
one log line says so instead."""
import os
import time

import numpy as np
import torch

from engine.logger import get_logger

logger = get_logger()

WARMUP = 50


def _env_flag(name):
    return os.environ.get(name, "0").strip().lower() not in ("", "0", "false", "no")


def compute_speed(model, input_size, device, iteration):
    torch.cuda.set_device(device)
    torch.backends.cudnn.benchmark = True
    model.eval()
    model = model.cuda()
    if _env_flag("TSG_INFER") or _env_flag("TSG_INFER_GRAPH"):
        from torchseg_amd.infer import prepare_inference
        model = prepare_inference(model, graph=_env_flag("TSG_INFER_GRAPH"))
        logger.info("compute_speed: prepared for inference (graph=%s)" % _env_flag("TSG_INFER_GRAPH"))
    x = torch.randn(*input_size, device=device)

    torch.cuda.synchronize()
    with torch.no_grad():
        for _ in range(WARMUP):
            model(x)
            torch.cuda.synchronize()

    logger.info('=========Speed Testing=========')
    spent = []
    for _ in range(iteration):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            model(x)
        torch.cuda.synchronize()
        spent.append(time.perf_counter() - t0)
    torch.cuda.synchronize()
    elapsed = float(np.sum(spent))
    logger.info("per-module profile: not available (torchprof is not installed)")
    logger.info('Elapsed time: [%.2f s / %d iter]' % (elapsed, iteration))
    logger.info('Speed Time: %.2f ms / iter    FPS: %.2f' % (elapsed / iteration * 1000, iteration / elapsed))
    return elapsed / iteration
