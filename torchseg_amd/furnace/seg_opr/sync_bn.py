"""The names FCN's train.py imports from `seg_opr.sync_bn` (model/fcn/voc.fcn32s.R101_v1c/train.py:20):
`DataParallelModel`, `Reduce` and `BatchNorm2d`.

The reference's module is a threaded single-process DataParallel with a cross-GPU BatchNorm.  Here the multi-device
path is the distributed launch (one process per GPU, torchseg_amd.ddp.DistributedDataParallel + SyncBatchNorm), so
these are thin compatibility names:

- `BatchNorm2d` is our SyncBatchNorm (plain BatchNorm in a single process).
- `DataParallelModel` wraps a module on ONE device and returns its output as a one-element list, which is what
  `Reduce.apply(*loss)` consumes.  More than one device is refused with a pointer to the distributed launch.
- `Reduce.apply(*xs)` sums its inputs.
"""
import torch
import torch.nn as nn

from torchseg_amd.syncbn import SyncBatchNorm as BatchNorm2d

__all__ = ['BatchNorm2d', 'DataParallelModel', 'Reduce']


class DataParallelModel(nn.Module):
    def __init__(self, module, device_ids=None, output_device=None, dim=0):
        super(DataParallelModel, self).__init__()
        if device_ids is not None and len(device_ids) > 1:
            raise RuntimeError(
                "seg_opr.sync_bn.DataParallelModel covers a single device only (got device_ids=%r); run one process "
                "per GPU with `python -m torch.distributed.launch --nproc_per_node=N train.py` (engine.Engine "
                "then wraps the model in DistributedDataParallel with SyncBatchNorm)" % (list(device_ids),))
        self.module = module
        self.device_ids = list(device_ids) if device_ids is not None else None
        self.dim = dim

    def forward(self, *inputs, **kwargs):
        return [self.module(*inputs, **kwargs)]


class Reduce(torch.autograd.Function):
    """Sum of the per-device outputs (the reference's Reduce adds them on one device)."""

    @staticmethod
    def forward(ctx, *inputs):
        ctx.n = len(inputs)
        out = inputs[0]
        for x in inputs[1:]:
            out = out + x
        return out.clone() if ctx.n == 1 else out

    @staticmethod
    def backward(ctx, grad):
        return (grad,) * ctx.n
