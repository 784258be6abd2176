"""`step()` is shared by both fused optimizers; the one rule in it that only FusedSGD reaches:
a constant-lr FusedSGD that is NOT capturable still captures into a hipGraph (its launches take
host scalars that never change), and such a captured step is counted like an eager one - once,
when it is captured - because nothing on the device counts its replays."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SIZES = (1027, 64, 5)  # a vector body with a scalar tail, exactly one aligned segment, a sub-64 one


def test_captured_step_of_plain_sgd_counts_once_and_replays_update():
    from ray_torch_distributed_checkpoint_amd import ops
    from ray_torch_distributed_checkpoint_amd.optim import FusedSGD
    from ray_torch_distributed_checkpoint_amd.utils.graphs import CapturedStep

    torch.cuda.synchronize()
    ops.default_stream().exit_graph_mode()  # (a capture an earlier test never closed)
    gen = torch.Generator().manual_seed(4)
    init = [torch.randn(n, generator=gen) for n in SIZES]
    grads = [[torch.randn(n, generator=gen).to(DEV) for n in SIZES] for _ in range(4)]

    def make():
        ps = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
        return ps, FusedSGD(ps, lr=0.05, momentum=0.9, capturable=False)

    ps, opt = make()
    for p, g in zip(ps, grads[0]):
        p.grad = g.clone()
    opt.step()  # eager: the momentum buffers exist, the gradients are views of the flat buffer
    assert opt.step_count == 1
    cs = CapturedStep(opt.step, warmup=0)
    for k in (1, 2):
        for p, g in zip(ps, grads[k]):
            p.grad.copy_(g)
        cs.replay()
    cs.close()
    torch.cuda.synchronize()
    buf = opt._bufs["momentum_buffer"].clone()
    print("step_count after 1 eager step, 1 capture, 2 replays:", opt.step_count, "captured:", opt._captured)

    twin_ps, twin = make()
    eager = []
    for k in range(4):
        for p, g in zip(twin_ps, grads[k]):
            p.grad = g.clone()
        twin.step()
        torch.cuda.synchronize()
        eager.append((twin._bufs["momentum_buffer"].clone(), twin.flat_space.data.clone()))
    print("momentum buffer equals the twin's after eager steps:",
          [k + 1 for k in range(4) if torch.equal(buf, eager[k][0])])

    # the capture itself ran nothing: the eager step and the two replays are three updates ...
    assert torch.equal(buf, eager[2][0]) and torch.equal(opt.flat_space.data, eager[2][1])
    assert not torch.equal(buf, eager[3][0])
    # ... and the host counted the eager step and the capture; nothing is read back from the device
    assert opt.step_count == 2
    assert opt._captured is None and opt._dev is None
