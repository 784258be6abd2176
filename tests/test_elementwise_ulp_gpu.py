"""The embedding, dropout and ReLU-dropout kernels of elementwise.hip judged per element (GPU only).

The yardstick is the last section of tests/ulp.py.  Embedding forward: a bf16 output against the fp64 sum
of the two rows, 0.5 ulp + 16 x the fp32 twin, every element in its own last place (the sum of two bf16
numbers is exact in fp32 unless it is absorbed); without a position table the gathered rows bit for bit.
Embedding backward: fp32 sums against the fp64 `index_add`, max(16 x the twin, (R + 16) 2^-24) of the sum
of |terms|, R the terms a lane adds serially (the longest run of one id; the batch).  Dropout: the zero
pattern against the keep mask computed in NumPy from ops/random.py's Philox twin, bit for bit; what is kept
against fp64 x / (1 - p).  Outputs are pre-filled with NaN and followed by 64 guard elements.  Each judged
output prints one ULP line, each test its WORST lines; those of one run are kept in
profiles/elementwise_ulp_worst.txt.

Arm -> the test that reaches it:

  embed_fwd_kernel: D = 8 (one lane busy), 128, 520 (the column loop twice, 8 lanes the second
  time), 1024 (twice, all lanes); ntok 1, 15, 74 (the last block partial, `t % T` wraps);
  with and without wpe; ids 0 and V - 1                                                     test_embedding_forward
  embed_bwd_wte_kernel: runs of one id that cross the 4-token blocks, every id distinct,
  accumulate 0 / 1, rows no token uses; embed_bwd_wpe_kernel: accumulate 0 / 1, D < 256
  and the second block of columns (D = 520, 1024); two launches agree bit for bit           test_embedding_backward
  dropout_kernel<float / bf16>: n < 4, the partial last quad, the second sweep of the capped
  grid, p = 0.25 / 0.5, a non-zero offset, `off_dev` null / set                            test_dropout
  ops.dropout: the backward regenerates the forward's mask                                  test_dropout_backward_regenerates_the_mask
  relu_dropout_kernel<float / bf16>: backward 0 / 1 / 2, p = 0 (no Philox call) / 0.25,
  the exact h > 0 boundary (planted +-0 and negatives); mode 2 on mode 0's output == mode 1  test_relu_dropout

Not run: fill_f32_kernel is in tests/test_optim_ulp_gpu.py with the casts; data_ops.hip and p2p_allreduce.hip
have exact tests of their own.
"""
import pytest
import torch

from tests import ulp as U

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F64, F32, BF16 = U.F64, U.F32, U.BF16
NAN = float("nan")
PAD = 64
SEED = 0x0123_4567_89AB_CDEF


def _ext():
    from ray_torch_distributed_checkpoint_amd.ops._ext import gpu_ext

    return gpu_ext()


def _bits(t):
    return t.contiguous().view({F32: torch.int32, BF16: torch.int16}[t.dtype])


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _guarded(shape, dtype, fill=NAN):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + PAD,), fill, dtype=dtype, device=DEV)
    return buf, buf[:n].view(shape)


def _guard_ok(buf, fill=NAN):
    g = buf[-PAD:]
    return bool(g.isnan().all()) if fill != fill else bool((g == fill).all())


# ------------------------------------------------------------------------------- embedding
@pytest.mark.parametrize("D", U.EMBED_WIDTHS)
def test_embedding_forward(D):
    J = U.Judge()
    for B, T in U.EMBED_BT:
        c = U.embed_inputs(B, T, D, dev=DEV)
        for wpe in (c["wpe"], None):
            buf, out = _guarded((B * T, D), BF16)
            _ext().embed_fwd(c["idx"], c["wte"], wpe, out, T)
            a = (c["idx"], c["wte"], wpe, T)
            r, t = U.embed_ref(F64, *a), U.embed_ref(F32, *a)
            J.ulp("embed_fwd", (B, T, D, wpe is not None), "out", out, r, t, 0.0)
            if wpe is None:
                assert _same(out, c["wte"][c["idx"].view(-1)])
            assert _guard_ok(buf)
    J.check()


@pytest.mark.parametrize("D", U.EMBED_WIDTHS)
def test_embedding_backward(D):
    from ray_torch_distributed_checkpoint_amd.ops.embedding import sort_ids

    J = U.Judge()
    for distinct in (False, True):
        c = U.embed_bwd_inputs(D, distinct, dev=DEV)
        B, T = c["idx"].shape
        V = c["V"]
        sidx, perm = sort_ids(c["idx"].reshape(-1), V)
        for acc_wte, acc_wpe in ((False, False), (True, False), (False, True), (True, True)):
            a = (c["idx"], c["dout"], c["dwte0"], c["dwpe0"], acc_wte, acc_wpe)
            r, t = U.embed_bwd_ref(F64, *a), U.embed_bwd_ref(F32, *a)
            got = []
            for _ in range(2):
                (bw, dwte), (bp, dwpe) = _guarded((V, D), F32), _guarded((T, D), F32)
                dwte.copy_(c["dwte0"])   # the prior gradient where it accumulates; elsewhere a sentinel
                dwpe.copy_(c["dwpe0"])
                _ext().embed_bwd(sidx, perm, c["dout"], dwte, dwpe, B, T, acc_wpe, acc_wte)
                assert _guard_ok(bw) and _guard_ok(bp)
                got.append((dwte, dwpe))
            assert _same(got[0][0], got[1][0]) and _same(got[0][1], got[1][1])
            dwte, dwpe = got[0]
            u = r["used"]
            shape = (D, "distinct" if distinct else "runs", acc_wte, acc_wpe)
            # R: a lane adds the run of one id serially, then the prior content (embed_bwd_wte_kernel's j loop)
            J.rel("embed_bwd", shape, "dwte", dwte[u], r["dwte"][u], t["dwte"][u], r["S_dwte"][u].clamp_min(U.TINY),
                  r["run"] + acc_wte)
            # R: the batch, serially, then the prior content (embed_bwd_wpe_kernel's b loop)
            J.rel("embed_bwd", shape, "dwpe", dwpe, r["dwpe"], t["dwpe"], r["S_dwpe"].clamp_min(U.TINY), B + acc_wpe)
            assert _same(dwte[~u], c["dwte0"][~u]) and int((~u).sum()) > 0   # rows no token uses
    J.check()


# ------------------------------------------------------------------------------- dropout
COUNTER = 782   # the Philox counter of the launch's first quad: offset, or offset + the device base


def _streams():
    """(stream without a device base, stream with one): both reserve the same counters"""
    from ray_torch_distributed_checkpoint_amd.ops.random import PhiloxStream

    host = PhiloxStream(SEED, offset=COUNTER)
    graph = PhiloxStream(SEED, offset=COUNTER - 5)
    graph.enter_graph_mode(DEV)   # the base moves to the device, the host offset restarts at 0
    graph.reserve(20)             # five quads: the offset of the launch is not zero
    assert host.device_base() is None and int(graph.device_base().item()) == COUNTER - 5
    return host, graph


def _dropout_x(n, dtype, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(n, device=DEV, generator=gen).to(dtype)
    x[x == 0] = 1.0
    return x


def _judge_kept(J, op, shape, out, r, t, keep, dtype):
    if dtype == F32:   # R: 1.f / (1.f - p) and the product
        J.rel(op, shape, "kept", out[keep], r[keep], t[keep], r[keep].abs().clamp_min(U.TINY), 3)
    else:
        J.ulp(op, shape, "kept", out[keep], r[keep], t[keep], 0.0)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", U.DROPOUT_SIZES)
def test_dropout(n, dtype):
    J = U.Judge()
    x = _dropout_x(n, dtype, n)
    for p in (0.25, 0.5):
        keep = U.dropout_keep(SEED, COUNTER, n, p).to(DEV)
        r, t = U.dropout_ref(F64, x, keep, p), U.dropout_ref(F32, x, keep, p)
        for st in _streams():
            seed, off = st.reserve(n)
            base = st.device_base()
            assert off != 0 and off + (0 if base is None else int(base.item())) == COUNTER
            buf, y = _guarded((n,), dtype)
            _ext().dropout(x, y, p, seed, off, base)
            assert torch.equal(y == 0, ~keep), int(((y == 0) != ~keep).sum())
            assert not y.isnan().any() and _guard_ok(buf)
            _judge_kept(J, "dropout", (n, p, base is not None), y, r, t, keep, dtype)
    J.check()


def test_dropout_backward_regenerates_the_mask():
    from ray_torch_distributed_checkpoint_amd.ops.dropout import dropout

    n, p = 1027, 0.25
    for st in _streams():
        x = _dropout_x(n, F32, 1).requires_grad_(True)
        dy = _dropout_x(n, F32, 2)
        y = dropout(x, p, True, st)
        y.backward(dy)
        keep = U.dropout_keep(SEED, COUNTER, n, p).to(DEV)
        assert torch.equal(y == 0, ~keep) and torch.equal(x.grad == 0, ~keep)
        assert _same(x.grad, torch.where(keep, dy * (1.0 / (1.0 - p)), torch.zeros_like(dy)))   # 1 / 0.75 in fp32, as the kernel


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("p", [0.0, 0.25])
def test_relu_dropout(p, dtype):
    J = U.Judge()
    n = 1027
    h = _dropout_x(n, dtype, 3)
    h[::7] = 0.0
    h[3::14] = -0.0
    dy = _dropout_x(n, dtype, 4)
    assert (h < 0).any() and (h == 0).sum() > 100
    keep = U.dropout_keep(SEED, COUNTER, n, p).to(DEV) if p > 0 else torch.ones(n, dtype=torch.bool, device=DEV)
    live = keep & (h > 0)
    outs = {}
    for mode in (0, 1, 2):
        buf, o = _guarded((n,), dtype)
        src = outs[0] if mode == 2 else h   # mode 2 reads the mask off the saved output
        if mode == 0:
            _ext().relu_dropout(src, o, None, None, p, SEED, COUNTER, 0)
        else:
            _ext().relu_dropout(src, None, dy, o, p, SEED, COUNTER, mode)
        assert _guard_ok(buf) and not o.isnan().any()
        assert torch.equal(o == 0, ~live), (mode, int(((o == 0) != ~live).sum()))
        a = (h, keep, p, None if mode == 0 else dy)
        r, t = U.relu_dropout_ref(F64, *a), U.relu_dropout_ref(F32, *a)
        _judge_kept(J, "relu_dropout", (n, p, mode), o, r, t, live, dtype)
        outs[mode] = o
    assert _same(outs[2], outs[1])
    if p == 0:   # no scaling: the forward is relu(h) up to the sign of a zero
        assert torch.equal(outs[0], torch.relu(h))
    J.check()
