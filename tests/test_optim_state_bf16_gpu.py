"""FusedAdamW(state_dtype=torch.bfloat16) on the GPU: `adamw_bf16state_kernel` against the NumPy
twin of its rounding rule bit for bit, against fp64, its rounding frequency, the unchanged fp32
path, chunk-cut / clipping / BackwardOverlap invariance, the CPU reference path, and an exact
resume of a packed workload."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
BF16 = torch.bfloat16
PAD = 64  # untouched guard elements behind every buffer's used part


def _ext():
    from ray_torch_distributed_checkpoint_amd.ops._ext import gpu_ext

    return gpu_ext()


def _table(rows):
    """rows: [(start, len, sstart)] or [(start, len, sstart, decay)] -> (int64 [n, 3] GPU tensor, n)."""
    t = [(r[0], r[1] | ((r[3] if len(r) > 3 else 0) << 32), r[2]) for r in rows]
    return torch.tensor(t, dtype=torch.int64, device=DEV), len(t)


def _bits16(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _decay_case(rows_by_step, n_p, n_s, seed):
    """g = 0, wd = 0, b1 = b2 = 0.75 over random bf16 state: 0.75 x is exact in fp32 for a bf16 x
    and the gradient term is 0, so the pre-rounding value does not depend on FMA contraction and
    the stored bits must equal sr_bf16(0.75 x, twin bits) exactly.  rows_by_step: {step: rows},
    one launch per step over disjoint chunks.  Elements outside every chunk stay untouched."""
    from ray_torch_distributed_checkpoint_amd.ops.random import sr_bf16_bits, sr_words

    for rows in rows_by_step.values():
        for r in rows:
            assert 0 <= r[0] and r[0] + r[1] <= n_p and 0 <= r[2] and r[2] + r[1] <= n_s, r  # in bounds
    gen = torch.Generator().manual_seed(5)
    p = torch.randn(n_p + PAD, generator=gen).to(DEV)
    g = torch.zeros(n_p + PAD, device=DEV)
    m0 = (torch.randn(n_s + PAD, generator=gen) * torch.exp(4 * torch.randn(n_s + PAD, generator=gen))).bfloat16()
    v0 = (torch.randn(n_s + PAD, generator=gen) * torch.exp(4 * torch.randn(n_s + PAD, generator=gen))).abs().bfloat16()
    m, v = m0.to(DEV), v0.to(DEV)
    for step, rows in rows_by_step.items():
        chunks, n = _table(rows)
        _ext().adamw(chunks, n, p, g, m, v, None, 1e-3, 0.75, 0.75, 1e-8, 0.0, 1 - 0.75 ** step,
                     math.sqrt(1 - 0.75 ** step), 1.0, 0, 0, seed, step)
    torch.cuda.synchronize()
    em, ev = _bits16(m0).copy(), _bits16(v0).copy()
    for step, rows in rows_by_step.items():
        for r in rows:
            start, ln, so = r[0], r[1], r[2]
            w = sr_words(seed, step, start, ln)
            em[so:so + ln] = sr_bf16_bits(m0[so:so + ln].float().numpy() * np.float32(0.75), w & 0xFFFF)
            ev[so:so + ln] = sr_bf16_bits(v0[so:so + ln].float().numpy() * np.float32(0.75), w >> 16)
    gm, gv = _bits16(m), _bits16(v)
    assert np.array_equal(gm, em), np.flatnonzero(gm != em)[:10]
    assert np.array_equal(gv, ev), np.flatnonzero(gv != ev)[:10]
    assert (gv < 0x8000).all()  # a non-negative v stays non-negative
    assert not np.array_equal(gm[:n_s], _bits16(m0)[:n_s])  # (the launch did something)


LENS = [1, 3, 4, 5, 7, 63, 64, 65, 1027]


def test_kernel_matches_twin_every_length_and_alignment():
    """Starts at multiples of 64 (every segment), and every other alignment `chunk_table_splits`
    can emit: a split may fall anywhere, so a piece can start at any offset mod 4 and have any
    length, with `sstart` moved by the same amount."""
    rows, at = [], 0
    for ln in LENS:
        rows.append((at, ln, at))
        at += (ln + 63) // 64 * 64
    for off in (1, 2, 3, 5, 6, 7):  # a chunk cut at an odd offset: the first piece ends there, the second starts
        for ln in (1, 3, 4, 5, 64, 1027 - off):
            rows.append((at + off, ln, at + off))
            at += 1152
    rows.append((at, 16384, at))  # a full chunk: 16 iterations per lane
    at += 16384
    rows.append((at, 16384 - 3, at))
    at += 16384
    _decay_case({1: rows}, at, at, seed=0x1234_5678_9ABC_DEF0)


def test_kernel_matches_twin_zero1_compact_layout():
    """`sstart != start`: the state buffers hold this rank's shards back to back (ZeRO-1), the
    rounding bits stay keyed by the flat offset `start`.  Includes a state offset whose
    alignment differs from the parameter offset's (the vector path needs both)."""
    rows = [(4096, 1027, 0), (8192 + 64, 65, 1088), (12288, 7, 1216), (16384, 640, 1280),
            (20000, 256, 1922), (24002, 256, 2180)]
    _decay_case({3: rows}, 24002 + 256, 2180 + 256, seed=7)


def test_kernel_matches_twin_more_chunks_than_blocks_and_two_steps():
    """5000 chunks (the grid is capped at 4096 blocks: some blocks walk two chunks), and two
    launches with different step numbers over disjoint chunks of the same buffers."""
    lens = [8, 5, 64, 3]
    rows = [(64 * i, lens[i % 4], 64 * i) for i in range(5000)]
    n = 64 * 5000
    _decay_case({2: rows[:5000:2] + rows[1:5000:2]}, n, n, seed=1)
    _decay_case({1: rows[:2500], 4: rows[2500:]}, n, n, seed=(1 << 64) - 1)


def test_general_step_against_fp64():
    """wd != 0, clip coefficient on, decay flag per chunk.  p within tests/test_optim.py's
    tolerance of the fp64 update (which reads the UNROUNDED moments); each stored moment is one
    of the two bf16 neighbours of the fp64 value (or the value), with one fp32 ulp of slack at
    the bracket ends.

    Why one ulp suffices for these inputs: b1 = 0.5, b2 = 0.75, clip coefficient 0.5 and
    bf16-representable gradients make every product of the moment updates exact in fp32
    (0.5 x, 0.75 x and 0.25 x of an 8-bit significand; g^2 has 16 bits), so the kernel's
    pre-rounding value is the fp64 value rounded to fp32 once, contracted or not."""
    n = 64 * 40
    rows = [(0, 1027, 0, 1), (1088, 65, 1088, 0), (1216, 7, 1216, 1), (1283, 250, 1283, 1), (1536, 1024, 1536, 0)]
    gen = torch.Generator().manual_seed(9)
    p0 = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen).bfloat16().float()
    m0 = (0.1 * torch.randn(n, generator=gen)).bfloat16()
    v0 = (0.1 * torch.randn(n, generator=gen)).square().bfloat16()
    lr, b1, b2, eps, wd, step, seed, coef = 1e-2, 0.5, 0.75, 1e-8, 0.1, 3, 21, 0.5
    bc1, bc2s = 1 - b1 ** step, math.sqrt(1 - b2 ** step)
    p, m, v = p0.to(DEV), m0.to(DEV), v0.to(DEV)
    clip = torch.tensor([2.0, coef], device=DEV)
    chunks, nc = _table(rows)
    _ext().adamw(chunks, nc, p, g.to(DEV), m, v, None, lr, b1, b2, eps, wd, bc1, bc2s, 1.0, 0, clip.data_ptr(), seed,
                 step)
    torch.cuda.synchronize()
    f32 = lambda x: float(np.float32(x))  # noqa: E731  (the kernel's scalar arguments are fp32)
    touched = np.zeros(n, dtype=bool)
    decay = np.ones(n)
    for s, ln, _, d in rows:
        touched[s:s + ln] = True
        if d:
            decay[s:s + ln] = f32(1 - f32(lr) * f32(wd))
    g64 = g.double().numpy() * coef
    m64 = b1 * m0.double().numpy() + (1 - b1) * g64
    v64 = b2 * v0.double().numpy() + (1 - b2) * g64 * g64
    p64 = p0.double().numpy() * decay - f32(f32(lr) / f32(bc1)) * m64 / (np.sqrt(v64) / f32(bc2s) + f32(eps))
    pg = p.cpu().double().numpy()
    assert np.array_equal(pg[~touched], p0.double().numpy()[~touched])
    assert np.allclose(pg[touched], p64[touched], rtol=1e-5, atol=1e-6)
    for name, got, x64, old in (("exp_avg", m, m64, m0), ("exp_avg_sq", v, v64, v0)):
        gb = _bits16(got)
        assert np.array_equal(gb[~touched], _bits16(old)[~touched]), name
        mag = np.abs(x64).astype(np.float32).view(np.uint32).astype(np.int64)  # fp32 bits of |x|
        lo = np.maximum(mag - 1, 0) >> 16          # bf16 at or below |x| - 1 ulp
        hi = (mag + 1 + 0xFFFF) >> 16              # bf16 at or above |x| + 1 ulp
        sm = (gb & 0x7FFF).astype(np.int64)
        ok = (lo <= sm) & (sm <= hi) & (((gb >> 15) == (x64 < 0)) | (sm == 0))
        assert ok[touched].all(), (name, np.flatnonzero(~ok & touched)[:10])
        assert (sm[touched] != (mag >> 16)[touched]).any(), name  # some were rounded away from zero


def test_rounding_frequency():
    """2^20 elements with one pre-rounding value 0.9f * 1.0 = 0x3F666666: fractional position
    f = 0x6666 / 65536 = 0.4 between its bf16 neighbours.  The share rounded away from zero is
    within 6 sigma of f (the stream is fixed: deterministic)."""
    n = 1 << 20
    pre = int(np.float32(0.9).view(np.uint32))
    f = (pre & 0xFFFF) / 65536
    p = torch.zeros(n, device=DEV)
    g = torch.zeros(n, device=DEV)
    m = torch.ones(n, dtype=BF16, device=DEV)
    v = torch.zeros(n, dtype=BF16, device=DEV)
    rows = [(s, min(16384, n - s), s) for s in range(0, n, 16384)]
    chunks, nc = _table(rows)
    _ext().adamw(chunks, nc, p, g, m, v, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.1, 0.03, 1.0, 0, 0, 99, 1)
    torch.cuda.synchronize()
    mb = _bits16(m)
    assert set(np.unique(mb).tolist()) == {pre >> 16, (pre >> 16) + 1}
    share = float((mb == (pre >> 16) + 1).mean())
    print(f"f {f:.6f} share rounded away {share:.6f} 6 sigma {6 * (f * (1 - f) / n) ** 0.5:.6f}")
    assert abs(share - f) <= 6 * (f * (1 - f) / n) ** 0.5
    assert (_bits16(v) == 0).all()  # an exact value (0) is never changed


def test_fp32_state_through_the_changed_binding_and_type_checks():
    """fp32 m / v through `ext.adamw` (no seed / step arguments) is bitwise the step FusedAdamW
    takes with `state_dtype` left at its default; m and v of differing dtype are refused."""
    from ray_torch_distributed_checkpoint_amd.optim import FusedAdamW

    torch.manual_seed(2)
    ps = [torch.nn.Parameter(torch.randn(s, device=DEV)) for s in ((33, 17), (1027,), (64, 8), (5,))]
    opt = FusedAdamW(ps, lr=0.01, weight_decay=0.1)
    assert opt.state_dtype == torch.float32
    sp = opt._ensure_space()
    grads = [torch.randn_like(p) for p in ps]
    p1, m1, v1 = sp.data.clone(), torch.zeros_like(sp.data), torch.zeros_like(sp.data)
    g1 = torch.zeros_like(sp.data)
    for p, gr in zip(ps, grads):
        s = sp.segment_of(p)
        g1[s.offset:s.offset + s.numel] = gr.reshape(-1)
    for k in (1, 2):
        for p, gr in zip(ps, grads):
            p.grad = gr.clone()
        opt.step()
        chunks, n = sp.chunk_table(ps, [True] * len(ps))
        _ext().adamw(chunks, n, p1, g1, m1, v1, None, 0.01, 0.9, 0.999, 1e-8, 0.1, 1 - 0.9 ** k,
                     math.sqrt(1 - 0.999 ** k), 1.0)
    torch.cuda.synchronize()
    assert opt._bufs["exp_avg"].dtype == torch.float32
    assert torch.equal(sp.data, p1) and torch.equal(opt._bufs["exp_avg"], m1)
    assert torch.equal(opt._bufs["exp_avg_sq"], v1)
    chunks, n = sp.chunk_table(ps, [True] * len(ps))
    with pytest.raises(RuntimeError, match="exp_avg is"):
        _ext().adamw(chunks, n, p1, g1, m1.bfloat16(), v1, None, 0.01, 0.9, 0.999, 1e-8, 0.1, 0.1, 0.03, 1.0, 0, 0,
                     0, 1)
    with pytest.raises(RuntimeError, match="step number"):
        _ext().adamw(chunks, n, p1, g1, m1.bfloat16(), v1.bfloat16(), None, 0.01, 0.9, 0.999, 1e-8, 0.1, 0.1, 0.03, 1.0)


# ------------------------------------------------------------------ the optimizer on the GPU
def _gpt2_run(mode: str, steps: int = 3):
    """gpt2-tiny with bf16 optimizer state; mode: plain | cuts_a | cuts_b | clip | overlap."""
    from ray_torch_distributed_checkpoint_amd.models import GPT2, GPT2Config
    from ray_torch_distributed_checkpoint_amd.optim import BackwardOverlap, FusedAdamW

    torch.manual_seed(0)
    model = GPT2(GPT2Config.named("gpt2-tiny")).to(DEV)
    opt = FusedAdamW(model.parameters(), lr=1e-3, weight_decay=0.1, state_dtype=BF16, rounding_seed=17,
                     max_grad_norm=1e9 if mode == "clip" else None)  # (far above the norm: coefficient exactly 1)
    sp = opt._ensure_space()
    calls = []
    if mode == "overlap":
        ov = BackwardOverlap(opt, bucket_mb=0.05)
        assert len(ov.groups) > 2
    if mode.startswith("cuts"):
        inner = sp.chunk_table_splits
        sp.chunk_table_splits = lambda *a: calls.append(a[2]) or inner(*a)
    third = sp.numel // 3
    cuts = {"cuts_a": [third + 1, 2 * third + 2], "cuts_b": [77, third - 3, third + 16384 + 5, sp.numel - 70]}.get(mode)
    g = torch.Generator(device=DEV).manual_seed(1)
    losses = []
    for _ in range(steps):
        data = torch.randint(0, 1000, (4, 65), device=DEV, generator=g)
        loss = model(data[:, :-1], data[:, 1:])
        loss.backward()
        if cuts:  # the deferred-tail path: pieces of a collective "in flight", cut at any offset
            sp.pending_tail = [(c, lambda: None) for c in cuts]
        opt.step()
        opt.zero_grad()
        losses.append(loss.item())
    torch.cuda.synchronize()
    if cuts:
        assert len(calls) == steps and all(list(c) == cuts for c in calls)
    if mode == "clip":
        assert float(opt._clip_ws["out"][1]) == 1.0
    assert all(b.dtype == BF16 for b in opt._bufs.values())
    return losses, sp.data.clone(), {k: b.clone() for k, b in opt._bufs.items()}


def test_cut_clip_and_overlap_invariance_on_gpu():
    base = _gpt2_run("plain")
    assert base[2]["exp_avg_sq"].float().abs().sum() > 0
    for mode in ("cuts_a", "cuts_b", "clip", "overlap"):
        losses, data, st = _gpt2_run(mode)
        assert losses == base[0], mode
        assert torch.equal(data, base[1]), mode
        for k in st:
            assert torch.equal(st[k], base[2][k]), (mode, k)


def _ulp16_dist(a, b):
    """Distance of bf16 tensors in bf16 ulps (on the sign-magnitude number line)."""
    def key(t):
        x = _bits16(t).astype(np.int64)
        return np.where(x & 0x8000, -(x & 0x7FFF), x)

    return np.abs(key(a) - key(b))


@functools.lru_cache(maxsize=None)
def _gpu_and_cpu_runs():
    """The same gradients (computed on the GPU, copied to a CPU twin of the model) through the
    kernel and through the CPU reference path, 3 steps of gpt2-tiny, with bf16 and with fp32 state.
    Returns ({dtype: [(gpu param, cpu param)]}, {dtype: [(gpu moment, cpu moment)]}); computed once."""
    from ray_torch_distributed_checkpoint_amd.models import GPT2, GPT2Config
    from ray_torch_distributed_checkpoint_amd.optim import FusedAdamW

    state, params = {}, {}
    for dt in (BF16, torch.float32):
        torch.manual_seed(0)
        gm = GPT2(GPT2Config.named("gpt2-tiny")).to(DEV)
        torch.manual_seed(0)
        cm = GPT2(GPT2Config.named("gpt2-tiny"))
        for a, b in zip(gm.parameters(), cm.parameters()):
            assert torch.equal(a.detach().cpu(), b.detach())
        go = FusedAdamW(gm.parameters(), lr=1e-3, weight_decay=0.1, state_dtype=dt, rounding_seed=5)
        co = FusedAdamW(cm.parameters(), lr=1e-3, weight_decay=0.1, state_dtype=dt, rounding_seed=5)
        g = torch.Generator(device=DEV).manual_seed(1)
        for _ in range(3):
            data = torch.randint(0, 1000, (4, 65), device=DEV, generator=g)
            gm(data[:, :-1], data[:, 1:]).backward()
            for a, b in zip(gm.parameters(), cm.parameters()):
                b.grad = a.grad.detach().cpu().clone()
            go.step()
            co.step()
            go.zero_grad()
            co.zero_grad()
        torch.cuda.synchronize()
        params[dt] = [(a.detach().cpu(), b.detach().clone()) for a, b in zip(gm.parameters(), cm.parameters())]
        state[dt] = [(go.state[a][k].detach().cpu().reshape(-1), co.state[b][k].detach().reshape(-1))
                     for a, b in zip(gm.parameters(), cm.parameters()) for k in ("exp_avg", "exp_avg_sq")]
    for dt, pairs in params.items():
        bad = sum(int((~torch.isclose(a, b, rtol=1e-5, atol=1e-6)).sum()) for a, b in pairs)
        worst = max(float((a - b).abs().max()) for a, b in pairs)
        print(f"{dt}: parameters outside rtol 1e-5 / atol 1e-6: {bad} of {sum(a.numel() for a, _ in pairs)}, "
              f"greatest absolute difference {worst:.3e}")
    return params, state


def test_gpu_state_against_cpu_path_three_steps():
    """Both paths draw the same Philox bits, and the CPU path computes the moments it stores in
    the kernel's own operation order (fp32 products, one fused multiply-add each, the constants
    (float)b and 1.f - (float)b), emulating the fused operation in fp64.  The stored state can
    therefore differ only where that emulation rounds twice (about 2^-29 of the operations) and
    the one-fp32-ulp result then falls on the other side of a rounding threshold (2^-16 of
    those): none is expected among 1.1 M elements.  The bounds are those of a CPU path a few
    fp32 ulps away from the kernel: 4 ulps of the 65536 between two bf16 values, per step and
    element, over 3 steps, with a margin of 5: 1e-3 of the elements; a difference, once there,
    stays one bf16 ulp (the next pre-rounding values are less than one bf16 ulp apart): beyond one
    ulp at most 1e-5.  (When the CPU path stored the moments of its torch-op update instead -
    whose 1 - beta2 is the rounded double, 1.3e-5 from the kernel's 1.f - 0.999f - 1.2e-3 of
    the elements differed and this test failed.)  For comparison, with fp32 state the two
    paths' moments differ in some bit on most elements (93.7 % measured)."""
    _, state = _gpu_and_cpu_runs()
    f32_diff = np.concatenate([(a != b).numpy() for a, b in state[torch.float32]])
    d = np.concatenate([_ulp16_dist(a, b) for a, b in state[BF16]])
    print(f"elements {d.size}: bf16 state differs on {float((d > 0).mean()):.3e}, beyond one bf16 ulp on "
          f"{float((d > 1).mean()):.3e}; fp32 state differs (any bit) on {float(f32_diff.mean()):.3e}")
    assert float((d > 0).mean()) < 1e-3
    assert float((d > 1).mean()) < 1e-5


def test_gpu_params_against_cpu_path_three_steps():
    """Parameters of the same runs within tests/test_optim.py's tolerance (rtol 1e-5, atol 1e-6),
    with fp32 and with bf16 state.  This holds only because the two paths keep the same stored
    state: an element whose stored moment is one bf16 ulp apart gets a next update that differs
    by up to lr * 2^-7 |m / sqrt(v)| ~ 8e-6, above atol."""
    params, _ = _gpu_and_cpu_runs()
    for dt in (torch.float32, BF16):
        for a, b in params[dt]:
            torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)


def test_packed_workload_resumes_exactly_on_gpu_with_bf16_state(tmp_path, monkeypatch):
    """Packed llama3-tiny with opt_state_dtype="bf16", trained and exactly resumed on the GPU: losses
    and the final checkpoint bit-identical; the checkpoint's exp_avg entries are bf16 in `.metadata`."""
    from ray_torch_distributed_checkpoint_amd.checkpoint import dcp
    from tests.test_optim_state_bf16_cpu import _dcp_dir, run_resume_case

    for k in ("RTDC_FAIL_AT_STEP", "RTDC_HANG_AT_STEP", "RTDC_FORCE_CPU", "RTDC_FAIL_AT_REPORT"):
        monkeypatch.delenv(k, raising=False)
    first = run_resume_case(tmp_path, use_gpu=True, model="llama3-tiny", steps=4, doc_len=16)
    md = dcp.read_metadata(_dcp_dir(first))
    moments = {k: m.properties.dtype for k, m in md.state_dict_metadata.items()
               if k.endswith(("exp_avg", "exp_avg_sq"))}
    assert moments and set(moments.values()) == {BF16}, moments
