"""Attention dropout through the whole model on the GPU: GPT-2 and Llama with `attn_dropout`."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

B, T, P = 2, 128, 0.1


def _model(name):
    from ray_torch_distributed_checkpoint_amd.models import GPT2, GPT2Config, Llama, LlamaConfig

    torch.manual_seed(0)
    if name.startswith("llama"):
        cfg = LlamaConfig.named(name)
        return cfg, Llama(cfg, attn_dropout=P)
    cfg = GPT2Config.named(name)
    return cfg, GPT2(cfg, attn_dropout=P)


def _batch(cfg, device):
    torch.manual_seed(2)
    tok = torch.randint(0, cfg.vocab_size, (B, T + 1))
    return tok[:, :-1].contiguous().to(device), tok[:, 1:].contiguous().to(device)


def _step(net, x, y, seed=11):
    """loss and gradients of one forward + backward from a given state of the mask stream"""
    from ray_torch_distributed_checkpoint_amd import ops

    ops.manual_seed(seed)
    for p in net.parameters():
        p.grad = None
    loss = net(x, y)
    loss.backward()
    if x.is_cuda:
        torch.cuda.synchronize()
    return loss.detach().float().cpu(), {n: p.grad.detach().float().cpu() for n, p in net.named_parameters()}


@pytest.mark.parametrize("name", ["llama3-tiny", "gpt2-tiny"])
def test_train_eval_and_reproducibility(name):
    from ray_torch_distributed_checkpoint_amd import ops

    cfg, net = _model(name)
    net = net.cuda()
    x, y = _batch(cfg, "cuda")
    loss, grads = _step(net, x, y)
    assert torch.isfinite(loss) and all(torch.isfinite(g).all() for g in grads.values())
    assert ops.default_stream().offset > 0  # the masks came from the default stream
    # the same stream state twice: the same loss and gradients, bit for bit
    loss2, grads2 = _step(net, x, y)
    assert torch.equal(loss, loss2) and all(torch.equal(grads[n], grads2[n]) for n in grads)
    # another state, another mask
    assert not torch.equal(loss, _step(net, x, y, seed=12)[0])
    # eval mode draws nothing and is the model without the attribute
    net.eval()
    off = ops.default_stream().offset
    with torch.no_grad():
        ev = net(x, y).float().cpu()
    assert ops.default_stream().offset == off
    assert not torch.equal(ev, loss)
    net.train()
    net.attn_dropout = 0.0
    with torch.no_grad():
        assert torch.equal(net(x, y).float().cpu(), ev)
    assert ops.default_stream().offset == off


@pytest.mark.parametrize("name", ["llama3-tiny", "gpt2-tiny"])
def test_gpu_and_cpu_draw_the_same_mask(name):
    """GPU against the model's fp32 CPU path from the same stream state.  The bound is the one of
    tests/test_models_window_gpu.py's CPU/GPU comparison: the GPU-vs-CPU error of the same model
    and input without the feature; with dropout it may be at most 1.5 x that - room for another
    rounding pattern, not for another mask (a mask that differs in one block moves the logits far
    more, which the test measures as `moved`).  Judged on the train-mode logits, on the loss
    (whose error the largest logit error bounds) and on the gradients (the largest error over all
    parameters)."""
    from ray_torch_distributed_checkpoint_amd import ops

    cfg, ref = _model(name)
    gpu = copy.deepcopy(ref).cuda()
    x, y = _batch(cfg, "cpu")

    def logits(net, xx):
        ops.manual_seed(11)
        with torch.no_grad():
            return net(xx).float().cpu()

    def errs():
        lg, lc = logits(gpu, x.cuda()), logits(ref, x)
        (gl, gg), (cl, cg) = _step(gpu, x.cuda(), y.cuda()), _step(ref, x, y)
        return (lg - lc).abs().max().item(), (gl - cl).abs().item(), max((gg[n] - cg[n]).abs().max().item() for n in cg), lc

    d_logit, d_loss, d_grad, with_drop = errs()
    gpu.attn_dropout = ref.attn_dropout = 0.0
    p_logit, p_loss, p_grad, without = errs()
    ops.manual_seed(12)
    ref.attn_dropout = P
    with torch.no_grad():
        moved = (ref(x).float() - with_drop).abs().max().item()  # what another mask does to the logits
    print(f"{name}: GPU-vs-CPU max error  logits plain {p_logit:.4e} dropout {d_logit:.4e} | loss plain {p_loss:.4e} "
          f"dropout {d_loss:.4e} | grads plain {p_grad:.4e} dropout {d_grad:.4e} | another mask moves the logits "
          f"{moved:.3e}")
    assert (with_drop - without).abs().max().item() > 10 * p_logit  # dropout does change the logits
    assert moved > 10 * p_logit
    assert d_logit <= 1.5 * p_logit, (d_logit, p_logit)
    assert d_loss <= 1.5 * p_logit, (d_loss, p_logit)
    assert d_grad <= 1.5 * p_grad, (d_grad, p_grad)
