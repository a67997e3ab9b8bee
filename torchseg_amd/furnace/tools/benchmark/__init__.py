"""Inference timing and per-module cost tables for the `.speed` experiments (model/bisenet/*.speed/eval.py:17, :113,
:116): `compute_speed(model, input_size, device, iteration)` and `stat(model, input_size)`, with the per-module counters
`compute_flops`, `compute_madd` and `compute_memory` they are built on."""
from .counters import compute_flops, compute_madd, compute_memory
from .speed import compute_speed
from .statistics import stat, collect

__all__ = ["compute_speed", "stat", "collect", "compute_flops", "compute_madd", "compute_memory"]
