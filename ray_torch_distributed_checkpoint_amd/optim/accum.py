"""GradAccumulator: k backward passes per optimizer step, added in place in the flat buffer.

    acc = optim.GradAccumulator(opt, steps=k, ddp=net_or_None, average=True)
    for i in range(k):
        with acc.micro_step(i):
            loss_fn(net, *batch_i).backward()
    opt.step(); opt.zero_grad(set_to_none=True)

Between two micro-batches `FlatParamSpace.next_micro_step()` detaches every `p.grad` again, so
each backward runs in the single-backward protocol (the ops return the flat view, AccumulateGrad
adopts it, the DDP hooks fire) while `ops.gradbuf.grad_slot` tells the kernels to ADD into the
slices that already hold this step's earlier micro-batches: the grouped weight-gradient GEMMs,
the column-sum reductions and the embedding backward accumulate in their own epilogues - no
parameter-sized temporary, no add kernel, no memset.  Whatever still arrives outside the buffer
(ResNet's convolution / BatchNorm gradients, the norm parameters, every CPU path) is added by
the fold-back, which the accumulator runs at the end of each micro-batch.

Only the last micro-batch reduces: the others run under `ddp.no_sync()`, so the bucket
collectives (ZeRO-1 reduce-scatter, bf16 communication, the deferred tail) run once per step
over the accumulated buffer.

average=True makes the step use the MEAN over the micro-batches at no cost: it sets the space's
`grad_scale` to 1/k, which the AdamW / SGD kernels and the clipping norm already multiply in,
so clipping sees the norm of the averaged gradient.  As with clipping, `p.grad` itself holds
the unscaled SUM.  The scale stays set while the accumulator is in use; `close()` restores it.

steps=1 calls nothing of this: `micro_step` is an empty context.
"""
from __future__ import annotations

import contextlib

import torch

from .flat import space_of


class GradAccumulator:
    def __init__(self, opt, steps: int, ddp=None, average: bool = True):
        steps = int(steps)
        if steps < 1:
            raise ValueError(f"GradAccumulator: steps must be >= 1, got {steps}")
        self.opt, self.steps, self.ddp, self.average = opt, steps, ddp, bool(average)
        self.space = None
        self._old_scale = None
        if steps == 1:
            return
        if getattr(opt, "_overlap", None) is not None:
            raise RuntimeError("GradAccumulator with BackwardOverlap: the overlapped updates run during the first "
                               "backward pass and cannot take a second gradient; use the plain optimizer step")
        params = [p for g in opt.param_groups for p in g["params"]]
        sp = getattr(opt, "_space", None) or space_of(params)
        if sp is None:
            ensure = getattr(opt, "_ensure_space", None)
            if ensure is None:
                raise RuntimeError("GradAccumulator needs parameters in a FlatParamSpace (FusedAdamW / FusedSGD, "
                                   "or a DistributedDataParallel wrap)")
            sp = ensure()
        if sp.grad is None:
            raise RuntimeError("GradAccumulator needs a flat gradient buffer (FlatParamSpace(grads=True))")
        self.space = sp
        if self.average:
            self._old_scale = sp.grad_scale
            sp.grad_scale = sp.grad_scale / steps

    def close(self) -> None:
        """Restore the space's grad_scale (average=True changed it)."""
        if self._old_scale is not None:
            self.space.grad_scale = self._old_scale
            self._old_scale = None

    @contextlib.contextmanager
    def micro_step(self, i: int):
        """Context of micro-batch i (0 <= i < steps) of the current optimizer step."""
        if self.steps == 1:
            yield
            return
        if not 0 <= i < self.steps:
            raise IndexError(f"micro_step({i}) of {self.steps}")
        if getattr(self.opt, "_overlap", None) is not None:
            raise RuntimeError("GradAccumulator with BackwardOverlap: use the plain optimizer step")
        sp = self.space
        if sp.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("gradient accumulation inside a graph capture (utils.graphs.CapturedStep) is not "
                               "supported: capture single-backward steps, or accumulate eagerly")
        if i > 0:
            sp.next_micro_step()
        elif sp.accumulating:
            raise RuntimeError("micro_step(0) while the previous accumulated step is still open: call "
                               "opt.zero_grad() after opt.step()")
        sync = contextlib.nullcontext() if (self.ddp is None or i == self.steps - 1) else self.ddp.no_sync()
        with sync:
            yield
        # gradients that arrived outside the flat buffer: into their slices now (added to the
        # earlier micro-batches' sum), so the next micro-batch - and a reader of p.grad - finds
        # every gradient at its slice.  (The last micro-batch of a DDP step folds in its hooks,
        # before each bucket's collective.)
        from ..ops.gemm import flush_wgrads

        flush_wgrads()
        if self.ddp is None or i < self.steps - 1:
            sp.fold_grads()
