"""Where a native backward writes a parameter gradient.

With a FlatParamSpace in "fresh" mode (after `zero_grad(set_to_none=True)`) a parameter's
first gradient contribution of the step is written by the producing kernel straight into
the parameter's slice of the flat gradient buffer; torch's AccumulateGrad sees `p.grad is
None` and adopts that tensor as `p.grad` without a copy (the stealing path of
torch/csrc/autograd/functions/accumulate_grad.h), so there is neither an add kernel nor a
memset of the buffer per step, and the DDP buckets / fused optimizer find the gradient in
place.  A second contribution in the same step (tied weights) gets a fresh tensor and is
added by autograd as usual; anything that ends up outside the buffer is folded back by the
DDP hook / `FlatParamSpace.ensure_grad_views`.

A first contribution may be a DEFERRED weight gradient (ops/gemm.py `_WgradGroup`): its slice
is written only at the next flush, and the write overwrites.  Whenever a second contribution
of the same step is about to read or add to that slice (a weight shared by two linears, whose
second gradient autograd adds out of place; a linear head tied to an embedding, whose
backward adds in place through `claimed_target`), the pending products are flushed first.

Gradient accumulation over micro-batches (optim/accum.py) keeps this protocol: between two
backward passes `FlatParamSpace.next_micro_step()` detaches every `p.grad` again, and
`grad_slot` tells an op whether its kernel writes the slice or adds to what the earlier
micro-batches left there.
"""
from __future__ import annotations

import torch


def grad_slot(p: torch.Tensor | None) -> tuple[torch.Tensor | None, bool]:
    """(view, accumulate): the flat-buffer view p's gradient goes into, and whether the kernel
    must ADD to it.  accumulate is true in a later micro-batch of a gradient-accumulation step
    (`FlatParamSpace.next_micro_step`) for a parameter whose slice already holds this step's
    earlier micro-batches; a parameter touched for the first time in a later micro-batch is
    written (its slice still holds last step's values).  Either way the op returns the view
    as the gradient: p.grad is None in every micro-batch, so AccumulateGrad adopts it without
    a copy and the post-accumulate hooks (DDP, BackwardOverlap) fire as in a single backward."""
    if p is None:
        return None, False
    sp = getattr(p, "_rtdc_space", None)
    if sp is None or sp.grad is None or not sp.fresh or p.grad is not None:
        return None, False
    view = sp.grad_view(p)
    if getattr(p, "_rtdc_claim", -1) == sp.step_id:
        # already handed out this step (second use of a tied weight): autograd will add this
        # contribution to the slice - which must hold the first one by then.  (Not marked as a
        # twice-used weight: a bias slot is also claimed twice, by the LayerNorm backward that
        # reduces it on the way out and by its projection's colsum(), which returns that same
        # gradient - one contribution.)
        _flush_if_pending(view)
        if sp.accumulating:
            buf = sp._claim_bufs.get(id(p))
            if buf is not None:
                _flush_if_pending(buf)
            elif sp.touched(p):
                # the first use added in place, and autograd now sums (slice + this one) out of
                # place: that sum already holds the earlier micro-batches - the fold-back copies
                sp._sum_has_slice.add(sp.segment_of(p).index)
        return None, False
    acc = sp.accumulating and sp.touched(p)
    if acc and getattr(p, "_rtdc_tied", False):
        # a weight with two uses per backward (tied table): this micro-batch's two contributions
        # are summed in a temporary exactly as a single backward sums them, and the fold-back
        # adds that sum to the slice - one add per micro-batch, G = fl(g1 + g2).  Adding both
        # straight into the slice would round (g1 + first) where the two contributions cancel,
        # an error the size of the partial instead of the gradient.
        buf = torch.empty_like(view)
        sp._claim_bufs[id(p)] = buf.view(buf.shape)  # (an alias: AccumulateGrad adopts `buf` only unshared)
        p._rtdc_claim = sp.step_id
        return buf, False
    if acc:
        # (a product deferred in an earlier micro-batch is launched by next_micro_step; this
        # covers a flat view someone handed out by other means)
        _flush_if_pending(view)
    p._rtdc_claim = sp.step_id
    return view, acc


def grad_target(p: torch.Tensor | None) -> torch.Tensor | None:
    """The flat-buffer view to WRITE p's gradient into, or None (allocate normally): for call
    sites whose kernel cannot add.  In a later micro-batch of an accumulation step a parameter
    that already has a gradient gets None - the op allocates, and the fold-back
    (`FlatParamSpace.fold_grads`, DDP's hook) adds the temporary to the slice."""
    if p is None:
        return None
    sp = getattr(p, "_rtdc_space", None)
    if sp is not None and sp.grad is not None and sp.accumulating and sp.touched(p):
        if getattr(p, "_rtdc_claim", -1) == sp.step_id:
            _flush_if_pending(sp.grad_view(p))  # (autograd adds to what grad_slot handed out)
        return None
    return grad_slot(p)[0]


def _flush_if_pending(view: torch.Tensor) -> None:
    from .gemm import _WG, flush_wgrads

    # only a deferred PRODUCT overwrites its slice at the flush; a pending column-sum job into a
    # bias slot claimed twice is the LayerNorm offer protocol (ops/gemm.py colsum), which
    # retargets the job instead of reading the slot
    if _WG.pending_product(view):
        flush_wgrads()


def claimed_target(p: torch.Tensor | None) -> torch.Tensor | None:
    """For the second use of a tied weight in one step: the flat-buffer view that the first
    use's backward already wrote (handed out by grad_target, not yet adopted by AccumulateGrad),
    so a native backward can ADD its contribution in place and return no gradient - instead
    of a fresh zero-filled tensor that autograd adds out of place and the optimizer copies
    back into the buffer (3 full passes over a 154 MB GPT-2 table)."""
    if p is None:
        return None
    sp = getattr(p, "_rtdc_space", None)
    if sp is None or sp.grad is None or not sp.fresh or p.grad is not None:
        return None
    if getattr(p, "_rtdc_claim", -1) != sp.step_id:
        return None
    p._rtdc_tied = True
    view = sp._claim_bufs.get(id(p)) if sp.accumulating else None  # (grad_slot's temporary of this micro-batch)
    if view is None:
        view = sp.grad_view(p)
    _flush_if_pending(view)  # the in-place add must land on the first use's written gradient
    return view
