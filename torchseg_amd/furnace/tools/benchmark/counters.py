"""Per-leaf-module cost counters, with the counting conventions the reference's `stat` table uses, for the module types
of the BiSeNet R18 / X39 networks.  Each takes (module, input, output) of one call; every other type counts 0.

  FLOPs   Conv2d: k_h * k_w * C_in * (C_out / groups) per output position of the batch, + C_out per position for a bias;
          BatchNorm2d: one per input element of the batch, two with an affine transform; ReLU / Sigmoid (and the other
          pointwise activations): one per input element; Max / Avg / Adaptive pooling: one per input element;
          Linear: batch * in * out.
  MAdd    Conv2d: per output element of ONE sample, k_h * k_w * C_in / groups multiplies and one add fewer (+1 with a
          bias); BatchNorm2d: 4 per input element of one sample; ReLU: 1 per element of one sample; MaxPool2d:
          k_h * k_w - 1 per output element; Linear: (2 * in - 1) per output feature.  Sigmoid, adaptive pooling and
          Dropout count 0.
  memory  (elements read, elements written) of the batch: the input (+ the trainable parameters per sample for Conv2d
          and Linear, + 2 per channel for BatchNorm2d) and the output; ReLU reads and writes its input; pooling reads
          its input and writes its output.  Sigmoid and Dropout count (0, 0).  `stat` multiplies by the element size.
"""
import math

import torch.nn as nn

_ACT = (nn.ReLU, nn.ReLU6, nn.PReLU, nn.ELU, nn.LeakyReLU, nn.Sigmoid)
_POOL = (nn.AvgPool2d, nn.MaxPool2d, nn.AdaptiveAvgPool2d, nn.AdaptiveMaxPool2d)


def _numel(shape):
    return int(math.prod(shape))


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def _trainable(module):
    return sum(p.numel() for p in module.parameters() if p.requires_grad)


def compute_flops(module, inp, out):
    """-> (flops, kind); kind is -1 for a module type that is not counted."""
    if isinstance(module, nn.Conv2d):
        kh, kw = module.kernel_size
        positions = out.shape[0] * out.shape[2] * out.shape[3]
        per = kh * kw * inp.shape[1] * (out.shape[1] // module.groups)
        return per * positions + (out.shape[1] * positions if module.bias is not None else 0), "Conv2d"
    if isinstance(module, nn.BatchNorm2d):
        return _numel(inp.shape) * (2 if module.affine else 1), "BatchNorm2d"
    if isinstance(module, _POOL):
        return _numel(inp.shape), "Pool2d"
    if isinstance(module, _ACT):
        return _numel(inp.shape), "Activation"
    if isinstance(module, nn.Linear):
        return inp.shape[0] * inp.shape[1] * out.shape[1], "Linear"
    return 0, -1


def compute_madd(module, inp, out):
    if isinstance(module, nn.Conv2d):
        kh, kw = module.kernel_size
        muls = kh * kw * (inp.shape[1] // module.groups)
        adds = muls - 1 + (1 if module.bias is not None else 0)
        return (muls + adds) * _numel(out.shape[1:])
    if isinstance(module, nn.BatchNorm2d):
        return 4 * _numel(inp.shape[1:])
    if isinstance(module, nn.MaxPool2d):
        kh, kw = _pair(module.kernel_size)
        return (kh * kw - 1) * _numel(out.shape[1:])
    if isinstance(module, nn.AvgPool2d):
        kh, kw = _pair(module.kernel_size)
        return kh * kw * _numel(out.shape[1:])
    if isinstance(module, (nn.ReLU, nn.ReLU6)):
        return _numel(inp.shape[1:])
    if isinstance(module, nn.Linear):
        return out.shape[1] * (2 * inp.shape[1] - 1)
    return 0


def compute_memory(module, inp, out):
    """-> (elements read, elements written)"""
    b = inp.shape[0]
    if isinstance(module, (nn.ReLU, nn.ReLU6, nn.ELU, nn.LeakyReLU)):
        return b * _numel(inp.shape[1:]), b * _numel(inp.shape[1:])
    if isinstance(module, nn.PReLU):
        return b * (_numel(inp.shape[1:]) + _trainable(module)), b * _numel(inp.shape[1:])
    if isinstance(module, nn.Conv2d):
        return b * (_numel(inp.shape[1:]) + _trainable(module)), b * _numel(out.shape[1:])
    if isinstance(module, nn.BatchNorm2d):
        return b * (_numel(inp.shape[1:]) + 2 * inp.shape[1]), _numel(inp.shape)
    if isinstance(module, nn.Linear):
        return b * (_numel(inp.shape[1:]) + _trainable(module)), _numel(out.shape)
    if isinstance(module, _POOL):
        return b * _numel(inp.shape[1:]), b * _numel(out.shape[1:])
    return 0, 0
