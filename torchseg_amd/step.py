"""ReplayedStep: the training step captured once into a hipGraph and replayed.

    step = ReplayedStep(model, optimizer, warmup=3, max_graphs=4, loss_ring=0, strict=False)
    for it, (imgs, gts) in ...:
        for i, g in enumerate(optimizer.param_groups):      # the reference's train.py:133-139, unchanged
            g["lr"] = lr if i < 2 else lr * 10
        loss = step(imgs, gts)                              # device tensor, valid until the next call

One call is `optimizer.zero_grad() -> loss = model(*batch) -> loss.backward() -> optimizer.step()`.  The eager step of the
R50 / R101 families is bound by the host that enqueues it (PSPNet: 16.2 of 19.1 ms); a replayed step costs the host a few
copies and one graph launch.  The protocol:

  * Capture key = (shape, dtype, device) of every input, model.training, which parameters require a gradient, the number
    of parameter groups.  The first `warmup` calls under a new key are ordinary eager steps (nothing is thrown away), the
    next call captures the step and replays it once (capture executes nothing), every later call copies the batch into
    the key's static inputs and replays.  At most `max_graphs` keys are held, the least recently used one goes first,
    together with its graph and its memory pool; it is captured again when it comes back.
  * ONE stream, owned by the object, carries warm-up, capture, replays and an eager optimizer: state the convolution
    library keeps from an eager step is bound to the stream it ran on, and a replay on another stream returns non-finite
    values by its second launch.  On entry that stream waits for the caller's current stream (the batch was
    produced there), on exit the caller's stream waits for it, so `loss.item()` in the caller needs no further care.
  * The graph is linear: the weight-gradient side stream and the forks of the workload builders switch themselves off
    while a stream is capturing (convwrw.py, workloads/bisenet.py, fusion.py); a branched graph replays slower here.
  * An optimizer with `refresh_lr` (optim.FusedSGD: learning rates in a device vector) is captured with the step, and
    `refresh_lr()` runs before every replay; any other optimizer runs eagerly behind each replay on the same stream.
  * `loss_ring=R`: every step also writes its loss into an fp32 [R] device ring through a device-side position, inside
    the graph; `losses()` returns the last min(R, steps) of them with one synchronisation (the replacement for a
    `loss.item()` per iteration, which would tie host and device together again).

The step runs eagerly (`mode == "eager"`, `reason` says why) when the first parameter is not on a GPU, with
TSG_STEP_REPLAY=0, with a process group or a gradient reducer (replay of the N > 1 path is not covered), when
model.training is false, and for a key whose capture raised (strict=False; the step that was being captured runs eagerly,
the exception text is kept in `reason`).  Captures are dropped after optimizer.load_state_dict (its state tensors are
replaced), and when the model's mode, the set of trainable parameters or the number of parameter groups changes
(add_param_group).  model.load_state_dict copies in place and needs no new capture.
"""
import collections
import gc
import os
import sys
import traceback

import torch
import torch.distributed as dist


class _Entry(object):
    __slots__ = ("graph", "inputs", "loss", "grads")

    def __init__(self, graph, inputs, loss, grads):
        self.graph, self.inputs, self.loss, self.grads = graph, inputs, loss, grads


def _error_text(e):
    """The exception and what it replaced: torch's graph context raises the error of the capture's end over the one that
    invalidated the capture."""
    parts, seen = [], set()
    while e is not None and id(e) not in seen:
        seen.add(id(e))
        line = (str(e).strip().splitlines() or [""])[0]
        parts.append("%s: %s" % (type(e).__name__, line[:200]))
        e = e.__cause__ or e.__context__
    return " <- ".join(parts)


def _clear_frames(e):
    """Drop the locals of every finished frame the exception chain holds (they keep the abandoned graph alive)."""
    seen = set()
    while e is not None and id(e) not in seen:
        seen.add(id(e))
        traceback.clear_frames(e.__traceback__)
        e = e.__cause__ or e.__context__


class ReplayedStep(object):
    def __init__(self, model, optimizer, warmup=3, max_graphs=4, loss_ring=0, strict=False):
        if warmup < 1:
            # optimizer state that first appears inside a capture (a momentum buffer's zeros) would be reset by every replay
            raise ValueError("ReplayedStep: warmup must be at least 1 (optimizer state is created by an eager step)")
        if max_graphs < 1:
            raise ValueError("ReplayedStep: max_graphs must be at least 1")
        self.model = model
        self.optimizer = optimizer
        self.warmup = int(warmup)
        self.max_graphs = int(max_graphs)
        self.strict = bool(strict)
        self.captures = 0                      # graphs captured so far (re-captures included)
        self.replays = 0
        self.steps = 0                         # steps executed, eager or replayed
        self._params = list(model.parameters())
        self._opt_inside = hasattr(optimizer, "refresh_lr")
        self._graphs = collections.OrderedDict()
        self._warm = {}                        # key -> eager steps taken under it
        self._uncapturable = {}                # key -> reason
        self._sig = None
        self._stream = None
        self._grad_owner = None                # the entry whose static gradients the parameters' .grad point at
        self._ring_len = int(loss_ring)
        self._ring = self._ring_pos = None
        self._hook = optimizer.register_load_state_dict_post_hook(self._on_optimizer_load)
        self.mode, self.reason = "replay", "warming up"
        why = self._static_reason()
        if why:
            self.mode, self.reason = "eager", why

    # ---- what decides the path ------------------------------------------------------------------------------------
    def _static_reason(self):
        why = []
        first = self._params[0] if self._params else None
        if os.environ.get("TSG_STEP_REPLAY", "1") == "0":
            why.append("TSG_STEP_REPLAY=0 switches replay off")
        if dist.is_initialized() or getattr(self.model, "reducer", None) is not None:
            why.append("a process group is initialised or the wrapper has a gradient reducer (replay of the N > 1 path "
                       "is not covered)")
        if first is None or not first.is_cuda:
            why.append("the model's first parameter is on device '%s', not on a GPU"
                       % ("none" if first is None else first.device))
        return "; ".join(why)

    def _signature(self):
        return (bool(self.model.training), tuple(p.requires_grad for p in self._params), len(self.optimizer.param_groups))

    def _on_optimizer_load(self, optimizer):
        self._drop()

    def _drop(self):
        """Forget every capture (and what was learnt about keys): the next call of a key warms up again."""
        if self._graphs:
            torch.cuda.synchronize()           # no graph goes while one of its replays is still queued
        self._graphs.clear()
        self._warm.clear()
        self._uncapturable.clear()
        self._grad_owner = None

    @property
    def stream(self):
        """The stream every step runs on (None where the step is the eager loop on the caller's stream).  The hand-over
        between the caller's stream and this one costs 0.3 - 0.45 ms per step on an MI355X (two cross-queue waits between
        consecutive graph launches); a loop that runs under `with torch.cuda.stream(step.stream)` does not pay it."""
        first = self._params[0] if self._params else None
        if first is None or not first.is_cuda:
            return None
        if self._stream is None or self._stream.device != first.device:
            self._stream = torch.cuda.Stream(device=first.device)
        return self._stream

    # ---- the step -------------------------------------------------------------------------------------------------
    def __call__(self, *batch):
        why = self._static_reason()
        if not why and not all(isinstance(t, torch.Tensor) for t in batch):
            why = "an input is not a tensor"
        if why:
            self.mode, self.reason = "eager", why
            return self._eager(batch)
        dev = self._params[0].device
        caller = torch.cuda.current_stream(dev)
        own = self.stream                                      # created on first use
        own.wait_stream(caller)
        with torch.cuda.stream(own):
            loss = self._on_stream(batch, dev)
        caller.wait_stream(own)
        return loss

    def _on_stream(self, batch, dev):
        sig = self._signature()
        if sig != self._sig:
            if self._sig is not None:
                self._drop()
            self._sig = sig
        if not sig[0]:
            self.mode, self.reason = "eager", "model.training is false"
            return self._eager(batch)
        key = (tuple((tuple(t.shape), t.dtype, t.device) for t in batch),) + sig
        why = self._uncapturable.get(key)
        if why is not None:
            self.mode, self.reason = "eager", why
            return self._eager(batch)
        entry = self._graphs.get(key)
        if entry is None:
            done = self._warm.get(key, 0)
            if done < self.warmup:
                self._warm[key] = done + 1
                self.mode, self.reason = "replay", "warming up (%d of %d eager steps)" % (done + 1, self.warmup)
                return self._eager(batch)
            entry = self._capture(key, batch, dev)
            if entry is None:                                  # capture raised: the step is not lost
                return self._eager(batch)
        else:
            self._graphs.move_to_end(key)
        self.mode, self.reason = "replay", "replaying a captured step"
        for s, t in zip(entry.inputs, batch):
            s.copy_(t, non_blocking=True)
        if self._opt_inside:
            self.optimizer.refresh_lr()
        self._refresh_stale_shadows(dev)
        entry.graph.replay()
        if self._grad_owner is not entry:
            # an eager step or another key's graph left other tensors in .grad: the eager optimizer below (and anybody who
            # looks) must see the ones this graph writes
            for p, g in zip(self._params, entry.grads):
                p.grad = g
            self._grad_owner = entry
        if not self._opt_inside:
            self.optimizer.step()
        self.replays += 1
        self.steps += 1
        return entry.loss

    def _body(self, batch, with_optimizer):
        self.optimizer.zero_grad(set_to_none=True)
        loss = self.model(*batch)
        loss.backward()
        if with_optimizer:
            self.optimizer.step()
        self._ring_write(loss)
        return loss

    def _eager(self, batch):
        self._grad_owner = None
        loss = self._body(batch, True)
        self.steps += 1
        return loss

    def _capture(self, key, batch, dev):
        from . import kernels as K
        while len(self._graphs) >= self.max_graphs:
            torch.cuda.synchronize()
            self._graphs.popitem(last=False)                   # least recently used: graph, static tensors and pool go
            self._grad_owner = None
        opt = self.optimizer
        self._ring_alloc(dev)
        inputs = [torch.empty_like(t).copy_(t) for t in batch]
        graph = torch.cuda.CUDAGraph()
        # A graph object's destructor synchronises the device, which the runtime refuses while any stream is capturing, and
        # an exception in a destructor ends the process.  So nothing is finalised inside the capture: the cyclic collector
        # (which may find a graph somebody dropped earlier) rests until the capture has ended.
        gc_was_on = gc.isenabled()
        try:
            if hasattr(opt, "prepare"):
                opt.prepare()                                  # static tables: host -> device copies, refused under capture
            K.provider().presize_scratch((self._stream,), dev)  # no scratch buffer may grow (= move) inside the capture
            self._refresh_stale_shadows(dev, always=True)      # its table is rebuilt (host -> device) when a model has died
            torch.cuda.synchronize()
            opt.zero_grad(set_to_none=True)                    # the captured backward allocates them in the graph's pool
            gc.disable()
            with torch.cuda.graph(graph, stream=self._stream):
                loss = self._body(inputs, self._opt_inside)
        except Exception as e:                                 # noqa: BLE001 - the eager step is always there
            self._end_failed_capture(graph, dev)
            # the abandoned graph goes HERE, outside any capture, not whenever the collector finds the traceback's frames
            _clear_frames(e)
            graph = inputs = None
            if self.strict:
                raise
            self.mode = "eager"
            self.reason = self._uncapturable[key] = "capture failed, this key runs eagerly: " + _error_text(e)
            return None
        finally:
            if gc_was_on:
                gc.enable()
        self.captures += 1
        entry = self._graphs[key] = _Entry(graph, inputs, loss, [p.grad for p in self._params])
        return entry

    def _end_failed_capture(self, graph, dev):
        """Leave the stream, the allocator and the parameters as an eager step expects them."""
        try:
            if torch.cuda.is_current_stream_capturing():
                graph.capture_end()
        except Exception:                                      # noqa: BLE001 - an invalidated capture ends with an error
            pass
        try:                                                   # the allocator stops routing this stream to the graph's pool
            torch._C._cuda_endAllocateToPool(dev.index if dev.index is not None else torch.cuda.current_device(), graph.pool())
        except Exception:                                      # noqa: BLE001 - already ended by capture_end
            pass
        torch.cuda.synchronize()
        self.optimizer.zero_grad(set_to_none=True)             # gradients of the abandoned capture live in its pool
        self._grad_owner = None

    @staticmethod
    def _refresh_stale_shadows(dev, always=False):
        """The bf16 filter shadows (shadow.py) are refreshed by host code that a replay does not run: a parameter written
        through torch since the capture (model.load_state_dict, an eager optimizer) is re-cast here, before the replay.
        `always`: before a capture, so that the launch table the captured refresh uses exists and is current."""
        shadow = sys.modules.get(__package__ + ".shadow")
        if shadow is None:
            return
        if always:
            shadow.bank.refresh_all(dev)
            return
        for e in shadow.bank.entries.values():
            p = e.ref()
            if p is not None and e.version != p._version and e.wb.device == dev:
                shadow.bank.refresh_all(dev)
                return

    # ---- loss ring ------------------------------------------------------------------------------------------------
    def _ring_alloc(self, dev):
        if self._ring_len > 0 and (self._ring is None or self._ring.device != dev):
            self._ring = torch.zeros(self._ring_len, dtype=torch.float32, device=dev)
            self._ring_pos = torch.zeros(1, dtype=torch.int64, device=dev)

    def _ring_write(self, loss):
        if self._ring_len <= 0:
            return
        self._ring_alloc(loss.device)
        self._ring.index_copy_(0, self._ring_pos, loss.detach().float().reshape(1))
        self._ring_pos.add_(1).remainder_(self._ring_len)

    def losses(self):
        """The last min(loss_ring, steps) losses, oldest first, as an fp32 CPU tensor (one synchronisation)."""
        if self._ring_len <= 0:
            raise RuntimeError("ReplayedStep was built with loss_ring=0")
        n = min(self._ring_len, self.steps)
        if n == 0:
            return torch.empty(0, dtype=torch.float32)
        ring = self._ring.cpu()                # the caller's stream has waited for the step's stream at the end of the call
        order = [(self.steps - n + i) % self._ring_len for i in range(n)]
        return ring[order]
