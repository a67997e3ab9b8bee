"""stat(model, input_size): one forward of a random CPU input through the model in eval mode, and a table of every
leaf module it called: input / output shape (without the batch), parameters, output memory (MB, fp32), MAdd, FLOPs and
memory read / written (bytes), with totals.  A module called more than once reports its last call."""
import numpy as np
import torch
import torch.nn as nn

from .counters import compute_flops, compute_madd, compute_memory

COLUMNS = ("module name", "input shape", "output shape", "params", "memory(MB)", "MAdd", "Flops", "MemRead(B)",
           "MemWrite(B)")


def collect(model, input_size):
    """-> list of dicts, one per leaf module the forward called, in module-registration order."""
    assert isinstance(model, nn.Module) and isinstance(input_size, (list, tuple))
    rows, handles = {}, []
    names = [(n, m) for n, m in model.named_modules() if n and not list(m.children())]

    def hook(name):
        def fn(module, args, out):
            inp = args[0]
            if not isinstance(out, torch.Tensor) or not isinstance(inp, torch.Tensor):
                return
            itemsize = inp.element_size()
            flops, _ = compute_flops(module, inp, out)
            mread, mwrite = compute_memory(module, inp, out)
            rows[name] = {
                "module name": name,
                "type": type(module).__name__,
                "input shape": list(inp.shape[1:]),
                "output shape": list(out.shape[1:]),
                "params": int(sum(p.numel() for p in module._parameters.values() if p is not None)),
                "memory(MB)": float(np.prod(out.shape[1:])) * 4 / 1024 ** 2,
                "MAdd": int(compute_madd(module, inp, out)),
                "Flops": int(flops),
                "MemRead(B)": int(mread) * itemsize,
                "MemWrite(B)": int(mwrite) * itemsize,
            }
        return fn

    for n, m in names:
        handles.append(m.register_forward_hook(hook(n)))
    try:
        model.eval()
        with torch.no_grad():
            model(torch.rand(*input_size))
    finally:
        for h in handles:
            h.remove()
    return [rows[n] for n, _ in names if n in rows]


def _human(v, binary=False):
    base = 1024.0 if binary else 1000.0
    for unit in ("", "K", "M", "G", "T"):
        if abs(v) < base or unit == "T":
            return ("%d" % v if unit == "" else "%.2f%s" % (v, unit + ("B" if binary else "")))
        v /= base


def report(rows):
    table = [[str(r[c]) if c != "memory(MB)" else "%.2f" % r[c] for c in COLUMNS] for r in rows]
    widths = [max(len(c), *(len(t[i]) for t in table)) if table else len(c) for i, c in enumerate(COLUMNS)]
    lines = ["  ".join(c.rjust(w) for c, w in zip(COLUMNS, widths))]
    lines += ["  ".join(v.rjust(w) for v, w in zip(t, widths)) for t in table]
    zero = sorted({r["type"] for r in rows if r["MAdd"] == 0 and r["Flops"] == 0 and r["MemRead(B)"] == 0})
    tot = {c: sum(r[c] for r in rows) for c in ("params", "memory(MB)", "MAdd", "Flops", "MemRead(B)", "MemWrite(B)")}
    lines.append("=" * 40)
    lines.append("Total params: %s" % _human(tot["params"]))
    lines.append("Total memory: %.2fMB" % tot["memory(MB)"])
    lines.append("Total MAdd: %sMAdd" % _human(tot["MAdd"]))
    lines.append("Total Flops: %sFlops" % _human(tot["Flops"]))
    lines.append("Total MemR+W: %s" % _human(tot["MemRead(B)"] + tot["MemWrite(B)"], binary=True))
    if zero:
        lines.append("counted as 0: %s" % ", ".join(zero))
    return "\n".join(lines)


def stat(model, input_size, query_granularity=1):
    rows = collect(model, input_size)
    print(report(rows))
    return rows
