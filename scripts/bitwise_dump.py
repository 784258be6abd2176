"""Dump a kernel family's outputs (fixed seeds) to a .pt file, so two builds of the extension
(RTDC_EXT_SO=<path>) can be compared bitwise - the check behind every "bitwise equal" A/B record
in profiles/.

    python scripts/bitwise_dump.py attn|norm|colsum|xent|resnet|gemm OUT.pt
    python scripts/bitwise_dump.py compare A.pt B.pt

`norm`, `colsum` and `xent` call the native entry points at small shapes that reach every
instantiation and launcher branch (profiles/norm_bwd_merge.md); `norm` and `colsum` are run once more
with RTDC_NORM_BWD_VW4=0 RTDC_COLSUM_WIDE=0.  `norm` also runs ops/norm.py, so against a build whose
norm bindings differ it is run from that build's own checkout, with this file dropped in.

`attn` runs every instantiation of the flash kernels at small shapes (all three rows-per-wave knobs
at 1 and at 2, head splits, plain and document-masked, every output), then three large default
cases (profiles/attn_merge_bitwise.md).

The `optim` family compares two COMMITS, not two builds: it covers the Python side of the fused
optimizers' step as well, so drop this file into a checkout of the other commit, build the
extension there and run it in both (profiles/optim_step_refactor_bitwise.md).

    python scripts/bitwise_dump.py optim OUT.pt cpu|cuda
    python scripts/bitwise_dump.py compare A.pt B.pt
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _attn_variants(out):
    """Every instantiation of the flash kernels, and dkdv_reduce_kernel, at small shapes: the native
    entry points called as ops/attention.py's backward calls them (column-sum workspace requested,
    head split from RTDC_FA_QS as _dkdv_head_split takes it), with every output kept - y, lse, dqkv,
    delta and the colsum workspace.  T = 192 falls back to one 16-row group per wave at any knob,
    T = 384 is an odd number of 128-row blocks; (2, 2, 2) at Dh = 128 is the dK/dV opt-in.  Plain, and
    one ragged document layout: boundaries inside a tile (37, T - 5, 100) and, from T = 192 on, a
    document that spans several tiles."""
    from ray_torch_distributed_checkpoint_amd.ops import DocLayout
    from ray_torch_distributed_checkpoint_amd.ops._ext import gpu_ext

    ext, B = gpu_ext(), 2
    saved = {k: os.environ.get(k) for k in ("RTDC_FA_FWD", "RTDC_FA_DQ", "RTDC_FA_DKDV")}
    for T in (64, 192, 256, 384):
        docs = DocLayout.from_lengths([[37, T - 42, 5], [100, T - 100] if T > 100 else [T]], T, "cuda")
        for H, Hkv, Dh in ((4, 4, 64), (8, 2, 64), (8, 2, 128)):
            W, scale = (H + 2 * Hkv) * Dh, Dh ** -0.5
            torch.manual_seed(T + H + Dh)
            qkv = (torch.randn(B, T, W, device="cuda") * 0.5).bfloat16()
            dy = torch.randn(B, T, H * Dh, device="cuda").bfloat16()
            for knob in (1, 2):
                for k in saved:
                    os.environ[k] = str(knob)
                for qs in (1, 2, 4):
                    if (H // Hkv) % qs:
                        continue
                    for d in (None, docs):
                        y = torch.zeros((B, T, H * Dh), dtype=torch.bfloat16, device="cuda")
                        lse = torch.zeros((B * H, T), dtype=torch.float32, device="cuda")
                        delta, dqkv = torch.zeros_like(lse), torch.zeros_like(qkv)
                        cs = torch.zeros((B * T // 16, W), dtype=torch.float32, device="cuda")
                        part = torch.zeros(qs * B * T * Hkv * 2 * Dh, dtype=torch.float32, device="cuda") if qs > 1 else None
                        if d is None:
                            ext.flash_fwd(qkv, y, lse, B, T, H, Hkv, Dh, scale)
                            ext.flash_bwd(qkv, y, dy, lse, delta, dqkv, B, T, H, Hkv, Dh, scale, cs, part, qs)
                        else:
                            ext.flash_fwd_doc(qkv, y, lse, d.start, d.end, B, T, H, Hkv, Dh, scale)
                            ext.flash_bwd_doc(qkv, y, dy, lse, delta, dqkv, d.start, d.end, B, T, H, Hkv, Dh, scale,
                                              cs, part, qs)
                        torch.cuda.synchronize()
                        name = f"T{T}.H{H}kv{Hkv}d{Dh}.knobs{knob}.qs{qs}.{'plain' if d is None else 'doc'}"
                        out[name] = {"y": y.cpu(), "lse": lse.cpu(), "dqkv": dqkv.cpu(), "delta": delta.cpu(),
                                     "colsum": cs.cpu()}
    for k, v in saved.items():  # the large cases below run at the caller's knobs
        if v is None:
            del os.environ[k]
        else:
            os.environ[k] = v


def attn():
    from ray_torch_distributed_checkpoint_amd.ops.attention import causal_attention

    out = {}
    _attn_variants(out)
    for name, B, T, H, Hkv, Dh in [("gpt2", 4, 1024, 12, 12, 64), ("gqa64", 2, 512, 8, 2, 64),
                                   ("llama", 1, 1024, 32, 8, 128)]:
        torch.manual_seed(7)
        qkv = (torch.randn(B, T, (H + 2 * Hkv) * Dh, device="cuda") * 0.5).bfloat16().requires_grad_(True)
        y = causal_attention(qkv, H, Hkv)
        y.backward(torch.randn_like(y))
        torch.cuda.synchronize()
        out[name] = (y.detach().cpu(), qkv.grad.detach().cpu())
    return out


def _nargs(fn):
    """positional arguments of a binding, from its pybind11 signature line"""
    return fn.__doc__.splitlines()[0].count(": ")


def _norm_variants(out):
    """Every norm_bwd_kernel instantiation through layernorm_bwd / rmsnorm_bwd: D over every width
    branch (8-B form: 256, 768), M = 1, 5, 67 on 16 waves (a wave owns up to 5 rows) and 9001 x 768 on
    the default waves (grid capped at the resident slots); with and without dres and, for LayerNorm,
    the dx column sums; reduced at once, and deferred (the partial rows, then colsum_multi).  Keeps
    every output and the raw partial-row workspace [nz][nblk][D].  An older build's bindings still
    take `accumulate` (False) and, for RMSNorm, `dxsum` (None): passed only where the binding has them."""
    from ray_torch_distributed_checkpoint_amd.ops._ext import gpu_ext

    ext = gpu_ext()
    old_ln, old_rms = _nargs(ext.layernorm_bwd) == 14, _nargs(ext.rmsnorm_bwd) == 11
    cases = [(M, D, 16) for D in (8, 200, 256, 512, 520, 768, 1024, 2048, 4096) for M in (1, 5, 67)] + [(9001, 768, 4096)]
    for M, D, nw in cases:
        g = torch.Generator().manual_seed(1000 * D + M)
        x, dy, dres = ((torch.randn(M, D, generator=g) * 2).bfloat16().cuda() for _ in range(3))
        gam = (1 + 0.1 * torch.randn(D, generator=g)).bfloat16().cuda()
        bet = (0.1 * torch.randn(D, generator=g)).bfloat16().cuda()
        nblk_max = nw // 4
        for rms in (False, True):
            y, mean, rstd = torch.zeros_like(x), torch.zeros(M, device="cuda"), torch.zeros(M, device="cuda")
            if rms:
                ext.rmsnorm_fwd(x, gam, y, rstd, 1e-5)
            else:
                ext.layernorm_fwd(x, gam, bet, y, mean, rstd, 1e-5)
            for dr in (None, dres):
                for cs in ((False,) if rms else (False, True)):
                    for defer in ((False,) if rms else (False, True)):
                        nz = (1 if rms else 2) + cs
                        ws = torch.zeros(nz * (nblk_max + 64) * D, device="cuda")
                        dx = torch.zeros_like(x)
                        dg, db, dxs = (torch.zeros(D, device="cuda") for _ in range(3))
                        if rms:
                            ext.rmsnorm_bwd(dy, x, gam, rstd, dr, dx, ws, dg, *((None, nw, False) if old_rms else (nw,)))
                            nblk = 0
                        else:
                            nblk = ext.layernorm_bwd(dy, x, gam, mean, rstd, dr, dx, ws, dg, db, dxs if cs else None, nw,
                                                     *((False, defer) if old_ln else (defer,)))
                        res = {"dx": dx, "ws": ws.clone()}
                        if defer:
                            assert 1 <= nblk <= nblk_max
                            outs = [dg, db] + ([dxs] if cs else [])
                            rows = ws[: nz * nblk * D].view(nz, nblk * D)
                            ext.colsum_multi([rows[z] for z in range(nz)], outs, [nblk] * nz, [D] * nz, [0] * nz)
                            res["nblk"] = nblk
                        res.update(dgamma=dg, dbeta=db, dxsum=dxs, y=y, mean=mean, rstd=rstd)
                        torch.cuda.synchronize()
                        name = f"{'rms' if rms else 'ln'}.M{M}.D{D}.{'dres' if dr is not None else 'plain'}" \
                               f"{'.colsum' if cs else ''}{'.defer' if defer else ''}"
                        out[name] = {k: v.cpu() if torch.is_tensor(v) else v for k, v in res.items()}


def norm():
    from ray_torch_distributed_checkpoint_amd.ops.norm import layer_norm, rms_norm

    out = {}
    _norm_variants(out)
    for kind, M, D in [("rms", 2048, 4096), ("ln", 512, 4096), ("rms", 1024, 1024), ("ln", 4096, 768),
                       ("ln", 256, 2048)]:
        torch.manual_seed(M + D)
        x = torch.randn(M, D, device="cuda").bfloat16().requires_grad_(True)
        w = torch.nn.Parameter(1 + 0.1 * torch.randn(D, device="cuda"))
        b = torch.nn.Parameter(0.1 * torch.randn(D, device="cuda"))
        y = rms_norm(x, w) if kind == "rms" else layer_norm(x, w, b)
        y.backward(torch.randn_like(y))
        torch.cuda.synchronize()
        out[f"{kind}_{M}x{D}"] = (y.detach().cpu(), x.grad.cpu(), w.grad.cpu(),
                                  b.grad.cpu() if b.grad is not None else torch.zeros(1))
    return out


def colsum():
    """G.colsum (stage 1 + the reduction: vector loads at N % 8 == 0, scalar ones at N = 200 on a
    padded row), written and accumulated, bf16 and fp32; colsum_partial; and one colsum_multi launch of
    5 jobs of mixed (W, D), W = 1 and W = 4096 among them, two of them accumulating."""
    from ray_torch_distributed_checkpoint_amd.ops import gemm as G
    from ray_torch_distributed_checkpoint_amd.ops._ext import gpu_ext

    ext, out = gpu_ext(), {}
    for dt in (torch.bfloat16, torch.float32):
        for N in (8, 200, 768, 2304):
            for M in (64, 4096, 16384):
                g = torch.Generator().manual_seed(N + M)
                X = torch.randn(M, N, generator=g).to(dt).cuda()
                o = torch.zeros(N, device="cuda")
                G.colsum(X, out=o)
                acc = o.clone()
                G.colsum(X, out=acc, accumulate=True)
                nblk = min(256, max(1, M // 64))
                ws = torch.zeros(nblk * N, device="cuda")
                ext.colsum_partial(X, M, N, N, ws, nblk)
                case = {"sum": o, "acc": acc, "partial": ws}
                if N == 200:  # rows padded to 203 elements: never the vector form
                    Xp = torch.randn(M, 203, generator=g).to(dt).cuda()
                    op = torch.zeros(N, device="cuda")
                    G.colsum(Xp[:, :N], out=op)
                    case["strided"] = op
                torch.cuda.synchronize()
                out[f"{str(dt)[6:]}.M{M}.N{N}"] = {k: v.cpu() for k, v in case.items()}
    g = torch.Generator().manual_seed(5)
    jobs = [(1, 768), (4096, 200), (67, 8), (192, 2304), (1000, 50)]
    wss = [torch.randn(W * D, generator=g).cuda() for W, D in jobs]
    outs = [torch.randn(D, generator=g).cuda() for _, D in jobs]
    ext.colsum_multi(wss, outs, [W for W, _ in jobs], [D for _, D in jobs], [0, 1, 0, 1, 0])
    torch.cuda.synchronize()
    out["multi"] = {f"job{j}": o.cpu() for j, o in enumerate(outs)}
    return out


def xent():
    """xent (plain, and label smoothing 0.1 with z-loss 1e-4; with and without argmax / lse) at one
    (V, ld) per launcher branch (tests/ulp.py XENT_ARMS), both xent_finalize entries (with and without
    the ce rows, counted and fixed divisor) and both xent_bwd entries on the dense [M, V] logits."""
    from ray_torch_distributed_checkpoint_amd.ops._ext import gpu_ext
    from tests import ulp as U

    ext, out = gpu_ext(), {}
    for dtype, V, ld, arm in U.XENT_ARMS:
        for planted in (False, True):
            c = U.xent_inputs(dtype, V, ld, planted, dev="cuda")
            M = c["logits"].shape[0]
            for eps, z in ((0.0, 0.0), (0.1, 1e-4)):
                case = {}
                for with_arg in (False, True):
                    dl = torch.zeros_like(c["logits"])
                    loss, ce = torch.zeros(M, device="cuda"), torch.zeros(M, device="cuda")
                    lse = torch.zeros(M, device="cuda") if with_arg else None
                    am = torch.zeros(M, dtype=torch.int64, device="cuda") if with_arg else None
                    ext.xent(c["logits"], dl, c["target"], loss, lse, am, M, V, ld, 1.0 / 7, U.IGNORE_INDEX, eps, z, ce)
                    fin = torch.zeros(2, 2, 3, device="cuda")
                    for i, (tg, n) in enumerate(((c["target"], 0.0), (None, 4.0))):
                        ext.xent_finalize(loss, tg, n, fin[i][0])
                        ext.xent_finalize(loss, tg, n, fin[i][1], ce)
                    case["arg" if with_arg else "noarg"] = {"grad": dl, "loss": loss, "ce": ce, "lse": lse, "argmax": am,
                                                            "finalize": fin}
                dense = c["logits"][:, :V].contiguous()
                lse = torch.logsumexp(dense.float(), 1)
                dlb = torch.zeros_like(dense)
                ext.xent_bwd(dense, dlb, c["target"], lse, torch.full((1,), 3.0, device="cuda"),
                             torch.full((1,), 7.0, device="cuda"), U.IGNORE_INDEX, eps, z)
                case["bwd"] = dlb
                torch.cuda.synchronize()
                name = f"{str(dtype)[6:]}.V{V}.ld{ld}.{'planted' if planted else 'randn'}.{'aux' if eps else 'plain'}"
                out[name] = {k: ({a: (b.cpu() if b is not None else 0) for a, b in v.items()} if isinstance(v, dict)
                                 else v.cpu()) for k, v in case.items()}
    return out


def resnet():
    from ray_torch_distributed_checkpoint_amd import ops
    from ray_torch_distributed_checkpoint_amd.models import ResNet18

    torch.manual_seed(3)
    model = ResNet18(num_classes=10).cuda()
    x = torch.randn(32, 3, 128, 128, device="cuda")
    y = torch.randint(0, 10, (32,), device="cuda")
    loss = ops.cross_entropy(model(x), y)
    loss.backward()
    torch.cuda.synchronize()
    out = {"loss": loss.detach().cpu()}
    for n, p in model.named_parameters():
        out["grad." + n] = p.grad.detach().cpu()
    for n, b in model.named_buffers():
        out["buf." + n] = b.detach().cpu()
    return out


def gemm():
    from ray_torch_distributed_checkpoint_amd.ops import gemm as G

    out = {}
    for name, M, K, N in [("qkv", 16384, 768, 2304), ("lm", 4096, 768, 50304), ("l_o", 2048, 4096, 4096),
                          ("l_qkv", 2048, 4096, 6144)]:
        torch.manual_seed(M + N)
        x = torch.randn(M, K, device="cuda").bfloat16()
        w = torch.randn(N, K, device="cuda").bfloat16()
        dy = torch.randn(M, N, device="cuda").bfloat16()
        out[name] = (G.linear_fwd(x, w).cpu(), G.linear_dgrad(dy, w).cpu())
    return out


def optim(device="cpu"):
    """The fused optimizers, every step path: {case: {step: {name: tensor | scalar | list}}}.  Uses the
    public API and the private attributes the tests read, so it runs in older trees too."""
    from ray_torch_distributed_checkpoint_amd.optim import BackwardOverlap, FusedAdamW, FusedSGD, LRSchedule
    from ray_torch_distributed_checkpoint_amd.optim.flat import FlatParamSpace

    dev = torch.device(device)
    cuda = dev.type == "cuda"
    # more than one 16384-element chunk, a sub-64 segment, tails that are no multiples of 4; the last
    # parameter has no gradient in steps 1-2 (its Adam step number trails the optimizer's)
    shapes = [(1027,), (64,), (5,), (40000,), (63,), (33, 7), (129,)]
    late, steps = len(shapes) - 1, 6
    gen = torch.Generator().manual_seed(11)
    init = [torch.randn(s, generator=gen) for s in shapes]
    grads = [[torch.randn(s, generator=gen).to(dev) for s in shapes] for _ in range(steps)]
    kinds = {
        "adamw": lambda g, kw: FusedAdamW(g, lr=1e-2, betas=(0.9, 0.95), **kw),
        "adamw_bf16": lambda g, kw: FusedAdamW(g, lr=1e-2, betas=(0.9, 0.95), state_dtype=torch.bfloat16,
                                               rounding_seed=5, **kw),
        "sgd_nesterov": lambda g, kw: FusedSGD(g, lr=0.05, momentum=0.9, nesterov=True, **kw),
        "sgd_plain": lambda g, kw: FusedSGD(g, lr=0.05, **kw),
    }
    variants = {
        "base": {}, "clip": {"max_grad_norm": 0.5}, "gscale": {"grad_scale": 0.25},
        "sched": {"lr_schedule": LRSchedule.warmup_cosine(2, 6)}, "tail": {"tail": True},
        "tail_clip": {"tail": True, "max_grad_norm": 0.5},
    }

    def make(kind, kw, zero=False):
        ps = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
        if zero:  # ZeRO-1 with one rank that owns everything: the chunk walk with torch ops, compact state
            sp = FlatParamSpace(ps)
            sp.set_zero(ZeroLayout([(0, sp.numel)], 0, 1))
        groups = [{"params": ps[0::2], "weight_decay": 0.0}, {"params": ps[1::2], "weight_decay": 0.1}]
        opt = kinds[kind](groups, kw)
        return ps, opt, opt._ensure_space()

    def snap(opt, sp, full=True):
        if cuda:
            torch.cuda.synchronize()
        d = {}
        if full:  # (reads the device counter of a captured optimizer back: only where that is meant)
            for i, st in opt.state_dict()["state"].items():
                for k, v in st.items():
                    if not opt._bufs or k == "step":  # (the other values are views of the flat buffers below)
                        d[f"state.{i}.{k}"] = v.clone() if torch.is_tensor(v) else v
        d.update(data=sp.data.clone(), step_count=opt.step_count, lr=opt.get_last_lr())
        if sp.shadow is not None:
            d["shadow"] = sp.shadow.clone()
        for k, b in opt._bufs.items():
            d["buf." + k] = b.clone()
        if opt._clip_ws is not None:
            d["clip_out"], d["grad_norm"] = opt._clip_ws["out"].clone(), opt.grad_norm.clone()
        return {k: v.cpu() if torch.is_tensor(v) else v for k, v in d.items()}

    def set_grads(ps, sp, n, in_place):
        for i, (p, g) in enumerate(zip(ps, grads[n])):
            if i == late and n < 2:
                p.grad = None
            elif not in_place:
                p.grad = g.clone()
            else:  # into the flat slice: a gradient outside it would make the step wait for the tail first
                if p.grad is None:
                    p.grad = FlatParamSpace.view(sp.grad, sp.segment_of(p))
                p.grad.copy_(g)

    if not cuda:
        import tempfile

        import torch.distributed as dist
        from ray_torch_distributed_checkpoint_amd.optim.flat import ZeroLayout

        dist.init_process_group("gloo", init_method="file://" + tempfile.mktemp(), rank=0, world_size=1)
    out = {}
    for kind in kinds:
        for vname, v in variants.items():
            for mode in ("", ".capturable") if cuda else ("", ".zero1"):
                kw = {k: x for k, x in v.items() if k in ("max_grad_norm", "lr_schedule")}
                ps, opt, sp = make(kind, dict(kw, capturable=mode == ".capturable"), zero=mode == ".zero1")
                sp.grad_scale = v.get("grad_scale", 1.0)
                case = out[f"{kind}.{vname}{mode}"] = {}
                for n in range(steps):
                    set_grads(ps, sp, n, "tail" in v)
                    if "tail" in v:  # a deferred last-bucket all-reduce in four pieces, odd offsets included
                        sp.pending_tail = [(off, lambda: None) for off in (7, 1090, 1091, 20001)]
                    opt.step()
                    case[n + 1] = snap(opt, sp)
    if not cuda:
        dist.destroy_process_group()
        return out

    from ray_torch_distributed_checkpoint_amd.models import GPT2, GPT2Config
    from ray_torch_distributed_checkpoint_amd.utils.graphs import CapturedStep

    # captured steps: one eager warm-up step, three replays, then state_dict() (the read-back)
    for kind, kw in (("adamw", {"capturable": True}), ("adamw_bf16", {"capturable": True}),
                     ("sgd_nesterov", {"max_grad_norm": 0.5})):
        ps, opt, sp = make(kind, kw)
        for p, g in zip(ps, grads[0]):
            p.grad = g.clone()
        cs = CapturedStep(opt.step, warmup=1)
        case = out[f"{kind}.graph"] = {0: snap(opt, sp, full=False)}
        for n in (1, 2, 3):
            for p, g in zip(ps, grads[n]):
                p.grad.copy_(g)
            cs.replay()
            case[n] = snap(opt, sp, full=False)
        cs.close()
        case["end"] = snap(opt, sp)

    for overlap in (False, True):
        torch.manual_seed(0)
        model = GPT2(GPT2Config.named("gpt2-tiny")).to(dev)
        opt = FusedAdamW(model.parameters(), lr=1e-3, weight_decay=0.1)
        if overlap:
            BackwardOverlap(opt, bucket_mb=0.05)
        g = torch.Generator(device=dev).manual_seed(1)
        case = out["gpt2_tiny" + (".overlap" if overlap else "")] = {}
        for n in range(3):
            data = torch.randint(0, 1000, (4, 65), device=dev, generator=g)
            loss = model(data[:, :-1], data[:, 1:])
            loss.backward()
            opt.step()
            opt.zero_grad()
            case[n + 1] = dict(snap(opt, opt.flat_space), loss=loss.item())
    return out


def compare(a, b, path=""):
    """(values compared, paths that differ) of two dumps: tensors by torch.equal, the rest by ==."""
    if isinstance(a, dict) and isinstance(b, dict) and a.keys() == b.keys():
        n, bad = 0, []
        for k in a:
            dn, db = compare(a[k], b[k], f"{path}/{k}")
            n, bad = n + dn, bad + db
        return n, bad
    if isinstance(a, (tuple, list)) and isinstance(b, (tuple, list)) and len(a) == len(b) and any(map(torch.is_tensor, a)):
        return compare(dict(enumerate(a)), dict(enumerate(b)), path)
    if torch.is_tensor(a) and torch.is_tensor(b):
        same = a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    else:
        same = type(a) is type(b) and a == b
    return 1, [] if same else [path]


if __name__ == "__main__":
    if sys.argv[1] == "compare":  # compare A.pt B.pt: the paths that differ, the totals; exit 1 on a mismatch
        a, b = torch.load(sys.argv[2]), torch.load(sys.argv[3])
        n, bad = compare(a, b)
        for k in bad:
            print("MISMATCH", k)
        print(f"{len(a)} cases, {n} values compared, {len(bad)} mismatches")
        sys.exit(1 if bad else 0)
    family = {"attn": attn, "norm": norm, "colsum": colsum, "xent": xent, "resnet": resnet, "gemm": gemm,
              "optim": optim}[sys.argv[1]]
    torch.save(family(*sys.argv[3:]), sys.argv[2])
