"""Every bf16 GEMM kernel and epilogue judged per element against fp64 (GPU only).

The yardstick is the GEMM section of tests/ulp.py: `gemm_ref` in float64 is the reference, in
float32 the twin (computed on the device with torch, once per case, shared by every variant); a
bf16 output is held to 0.5 ulp + 16 x the twin's error with a floor of FLOOR_GEMM x the sum of
|terms|, an fp32 output to max(16 x the twin, (K + 16) 2^-24) of that sum.  Every output is
pre-filled with NaN.  Each judged output prints one ULP line, each test its WORST lines; those of
one run are kept in profiles/gemm_ulp_worst.txt.

Arm -> the test that reaches it:

  tile_cfg 0..13 x layouts x fp32 / bf16 C, partial tiles, K = 1, 2, 3, 5 K-tiles   test_tile_configs
  documented fall-backs (13 -> 6 off the forward layout, 11 -> 6 for an fp32 C or
  an MN-major A, 6 -> 0 for a misaligned operand or ldc % 8 != 0)                   test_tile_configs, test_ldc_wider_than_n
  nothing written outside [M, N] with ldc > N                                       test_ldc_wider_than_n
  split-K (slabs counted) and K = 31 K-tiles (no slab)                              test_splitk
  persistent kernels over several tiles per block                                   test_persistent_multi_tile
  tail split, pick_cfg_few_rows, long-K forward -> cfg 12, the gemm4b setter         test_automatic_routes, test_gemm4b_setter
  epilogue4 / tile_epilogue_bf16 / cfg 12, 13 epilogues, both column-sum arms       test_epilogues
  batch strides and the causal modes (cfg 0)                                        test_batched_and_causal
  gemm8g_kernel / gemm8gp_kernel (grouped weight gradients)                         test_grouped_weight_gradients
  gemm_f32                                                                          test_gemm_f32

Not run: cfg 8 / 9 at one K-tile, which the launcher refuses (the persistent form needs two).
"""
import pytest
import torch

from tests import ulp as U

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64, F32, BF16 = U.F64, U.F32, U.BF16
NAN = float("nan")
_refs: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_refs():
    yield
    _refs.clear()


def _G():
    from ray_torch_distributed_checkpoint_amd.ops import gemm as G

    return G


def _ext():
    from ray_torch_distributed_checkpoint_amd.ops._ext import gpu_ext

    return gpu_ext()


def _case(gen, M, N, K, epi="plain", out_fp32=False, keep=True, aux_in=None):
    """case, fp64 reference and twin: computed once, shared, never modified"""
    key = (gen, M, N, K, epi, out_fp32 and U.GEMM_EPILOGUES[epi].get("cin") is not None)
    if aux_in is None and key in _refs:
        c, r, t = _refs[key]
        return dict(c, out_fp32=out_fp32), r, t
    c = U.gemm_case(gen, M, N, K, epi, out_fp32, DEV, aux_in=aux_in)
    got = (c, U.gemm_ref_of(F64, c), U.gemm_ref_of(F32, c))
    if keep and aux_in is None:
        _refs[key] = got
    return got


def _bits(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


def _same(x, y):
    return all(torch.equal(_bits(x[n].contiguous()), _bits(y[n].contiguous())) for n in x)


def _lay(a_k, b_k):
    return ("K" if a_k else "M") + ("K" if b_k else "M")


def _run(c, a_k, b_k, cfg=-1, ldc_pad=0, bias=None):
    """one gemm_bf16 call on a case; C is [M, N] of a NaN-filled [M + 1, N + ldc_pad] buffer whose
    other elements must keep their bits"""
    G = _G()
    M, N, K = c["M"], c["N"], c["K"]
    A, B = U.gemm_store(c["a"], c["b"], a_k, b_k)
    odt = F32 if c["out_fp32"] else BF16
    ldc = N + ldc_pad
    assert ldc_pad == 0 or (c["cin"] != "sep" and c["act"] == 0)   # every [M, N] operand shares ldc
    buf = torch.full((M + 1, ldc), NAN, dtype=odt, device=DEV)
    C = buf[:M]
    Cin = None
    if c["cin"] == "alias":
        buf[:M, :N] = c["Cin"]
        Cin = C
    elif c["cin"] == "sep":
        Cin = c["Cin"]
    before = buf.clone()
    aux_out = torch.full((M, N), NAN, dtype=BF16, device=DEV) if c["act"] in (2, 5) else None
    cs = torch.full((N,), NAN, dtype=F32, device=DEV) if c["colsum"] else None
    G.gemm_bf16(A, B, C, M, N, K, A.shape[-1], B.shape[-1], ldc, a_k, b_k, Cin=Cin,
                bias=c["bias"] if bias is None else bias, aux_in=c["aux_in"], aux_out=aux_out, alpha=c["alpha"],
                beta=c["beta"], act=c["act"], tile_cfg=cfg, alpha_dev=c["alpha_dev"], colsum_out=cs)
    torch.cuda.synchronize()
    assert torch.equal(_bits(buf[M]), _bits(before[M])), "a store below the last row"
    assert torch.equal(_bits(buf[:M, N:]), _bits(before[:M, N:])), "a store into [N, ldc)"
    outs = {"C": buf[:M, :N]}
    if aux_out is not None:
        outs["aux_out"] = aux_out
    if cs is not None:
        outs["colsum"] = cs
    return outs


# ------------------------------------------------------------------------------- forced configurations
@pytest.mark.parametrize("cfg", sorted(U.GEMM_TILES))
def test_tile_configs(cfg):
    """(BM + 8, 2 BN - 8) and (2 BM - 8, BN + 8) x K = 64, 128, 192, 320 x every layout x fp32 and
    bf16 C x both generators; a forced configuration that the launcher runs as another one equals
    that one bit for bit"""
    J = U.Judge()
    for M, N in U.gemm_tile_shapes(cfg):
        for K in U.GEMM_KS:
            for gen in U.GEMM_GENS:
                for f32 in (False, True):
                    c, r, t = _case(gen, M, N, K, "plain", f32)
                    for a_k, b_k in U.GEMM_LAYOUTS:
                        runs_as = U.gemm_cfg_runs_as(cfg, a_k, b_k, f32, K)
                        if runs_as is None:
                            continue
                        outs = _run(c, a_k, b_k, cfg)
                        if runs_as != cfg:
                            assert _same(outs, _run(c, a_k, b_k, runs_as)), (cfg, runs_as, a_k, b_k, f32)
                        shape = "%dx%dx%d %s %s %s" % (M, N, K, gen, _lay(a_k, b_k), "f32" if f32 else "bf16")
                        U.judge_gemm(J, "cfg%d" % cfg, shape, c, r, t, outs)
    J.check()


@pytest.mark.parametrize("cfg", [0, 6, 8, 12, 13])
def test_ldc_wider_than_n(cfg):
    """C is [M, N] of a [M + 1, N + 24] NaN buffer: the columns [N, ldc) and the guard row keep
    their bits (_run asserts it) - the general kernel, an 8-wave one, the persistent form, cfg 12
    and 13, plain and with a bias, fp32 and bf16.  With cfg 6: a bias that is only 8-byte aligned,
    and ldc % 8 != 0, fall back to cfg 0 (the binding itself refuses a C off 16 bytes, so the
    misaligned operand is the bias); equal to the forced cfg 0 and judged as well."""
    J = U.Judge()
    M, N = U.gemm_tile_shapes(cfg)[0]
    K = 128
    for f32 in (False, True):
        for epi in ("plain", "bias_bf16"):
            c, r, t = _case("randn", M, N, K, epi, f32)
            outs = _run(c, True, True, cfg, ldc_pad=24)
            U.judge_gemm(J, "cfg%d" % cfg, "%dx%dx%d ldc+24 %s %s" % (M, N, K, epi, "f32" if f32 else "bf16"), c, r, t, outs)
    if cfg == 6:
        c, r, t = _case("randn", M, N, K, "bias_bf16", False)
        wide = torch.zeros(N + 8, dtype=BF16, device=DEV)
        wide[4:4 + N] = c["bias"]
        off8 = wide[4:4 + N]
        assert off8.data_ptr() % 16 == 8
        for name, kw in (("bias+8B", {"bias": off8}), ("ldc+4", {"ldc_pad": 4})):
            outs = _run(c, True, True, 6, **kw)
            assert _same(outs, _run(c, True, True, 0, **kw)), name
            U.judge_gemm(J, "cfg6->0", "%dx%dx%d %s" % (M, N, K, name), c, r, t, outs)
    J.check()


# ------------------------------------------------------------------------------- split-K
@pytest.mark.parametrize("cfg", U.GEMM_SPLITK_CFGS)
def test_splitk(cfg):
    """K = 2048 (32 K-tiles) through ops.gemm.gemm_bf16, which supplies the slab workspace: the
    workspace is NaN before the call and more than one slab comes back finite; K = 1984 (31
    K-tiles): no slab is written.  fp32 and bf16 C, with and without Cin = C, beta = 1; every output
    is rounded once (the slabs are fp32), so k = 1 as everywhere."""
    G = _G()
    J = U.Judge()
    dev = torch.empty(0, device=DEV).device   # the key the wrapper looks its workspace up by
    for M, N in U.GEMM_SPLITK_SHAPES:
        ws = G.workspace(dev, min(16 * M * N, G.SPLITK_WS_ELEMS), "splitk")
        for K in U.GEMM_SPLITK_KS:
            for f32 in (False, True):
                for epi, gen in (("plain", "randn"), ("plain", "range"), ("accumulate", "randn")):
                    c, r, t = _case(gen, M, N, K, epi, f32)
                    for a_k, b_k in ((True, True), (False, False)):
                        if cfg >= 0 and U.gemm_cfg_runs_as(cfg, a_k, b_k, f32, K) != cfg:
                            continue
                        ws.fill_(NAN)
                        outs = _run(c, a_k, b_k, cfg)
                        assert G.workspace(dev, 1, "splitk") is ws
                        slabs = sum(bool(torch.isfinite(ws[s * M * N:(s + 1) * M * N]).all()) for s in range(16))
                        if K == 2048:
                            assert slabs > 1, (cfg, M, N, K, slabs)
                        else:
                            assert bool(torch.isnan(ws).all()), (cfg, M, N, K)
                        shape = "%dx%dx%d %s %s %s %s slabs %d" % (M, N, K, gen, epi, _lay(a_k, b_k),
                                                                   "f32" if f32 else "bf16", slabs)
                        U.judge_gemm(J, "splitk%d" % cfg, shape, c, r, t, outs)
    J.check()


# ------------------------------------------------------------------------------- persistent
@pytest.mark.parametrize("K", U.GEMM_PERSIST_KS)
@pytest.mark.parametrize("gen", U.GEMM_GENS)
def test_persistent_multi_tile(gen, K):
    """4392 x 4160: blocks walk several tiles, the last row and column are partial.  cfg 8 / 9
    forced in every layout, and the automatic persistent form of cfg 6 / 7 (forward layout), which
    equals the forced one bit for bit"""
    M, N = U.GEMM_PERSIST_MN
    J = U.Judge()
    for f32 in (False, True):
        c, r, t = _case(gen, M, N, K, "plain", f32, keep=False)
        fwd = {}
        for cfg in (8, 9, 6, 7):
            for a_k, b_k in (U.GEMM_LAYOUTS if cfg in (8, 9) else U.GEMM_LAYOUTS[:1]):
                outs = _run(c, a_k, b_k, cfg)
                if a_k and b_k:
                    fwd[cfg] = outs
                U.judge_gemm(J, "cfg%d" % cfg, "%dx%dx%d %s %s %s" % (M, N, K, gen, _lay(a_k, b_k), "f32" if f32 else "bf16"),
                             c, r, t, outs)
        assert _same(fwd[6], fwd[8]) and _same(fwd[7], fwd[9])
        del c, r, t, fwd
    J.check()


# ------------------------------------------------------------------------------- automatic routes
@pytest.mark.parametrize("route", U.GEMM_ROUTES, ids=lambda r: r[0])
def test_automatic_routes(monkeypatch, route):
    """the launcher's own choice under the default knobs equals the forced configuration bit for
    bit (the tail split also with RTDC_GEMM_TAIL=0, which is read per call) and is judged per
    element.  The knobs cached in function-local statics are not touched."""
    name, M, N, K, (a_k, b_k), epi, f32, forced = route
    monkeypatch.delenv("RTDC_GEMM_TAIL", raising=False)
    J = U.Judge()
    for gen in U.GEMM_GENS:
        c, r, t = _case(gen, M, N, K, epi, f32, keep=False)
        auto = _run(c, a_k, b_k, -1)
        assert _same(auto, _run(c, a_k, b_k, forced)), (name, forced)
        if name.startswith("tail_split"):
            monkeypatch.setenv("RTDC_GEMM_TAIL", "0")
            assert _same(auto, _run(c, a_k, b_k, -1))
            monkeypatch.delenv("RTDC_GEMM_TAIL")
        U.judge_gemm(J, name, "%dx%dx%d %s %s" % (M, N, K, gen, _lay(a_k, b_k)), c, r, t, auto)
        del c, r, t, auto
    J.check()


def test_gemm4b_setter():
    """gemm4b(1) sends the automatic 256x256 choice (here cfg 6: a weight-gradient layout with 30
    tiles) to cfg 12; gemm4b(0) restores it"""
    M, N, K = 1528, 1032, 192
    c, r, t = _case("randn", M, N, K, "plain", True, keep=False)
    old = _ext().gemm4b(1)
    try:
        on = _run(c, False, False, -1)
    finally:
        _ext().gemm4b(old)
    off = _run(c, False, False, -1)
    assert _same(on, _run(c, False, False, 12)) and _same(off, _run(c, False, False, 6))
    J = U.Judge()
    U.judge_gemm(J, "gemm4b=1", "%dx%dx%d MM f32" % (M, N, K), c, r, t, on)
    U.judge_gemm(J, "gemm4b=0", "%dx%dx%d MM f32" % (M, N, K), c, r, t, off)
    J.check()


# ------------------------------------------------------------------------------- epilogues
@pytest.mark.parametrize("cfg", U.GEMM_EPI_CFGS)
def test_epilogues(cfg):
    """every variant of U.GEMM_EPILOGUES at (520, 392, 192): the forward ones in the forward layout,
    the input-gradient activations in the dgrad layout (cfg 13: forward only).  act 6 reads the
    gelu' that this kernel's act-5 call stored, and each half is judged against fp64.  Column
    sums: the fused arm (cfg 6..13, bf16 C) against the unrounded product, the other against the
    kernel's own C.  An input-gradient activation with a residual runs as cfg 0."""
    M, N, K = U.GEMM_EPI_SHAPE
    J = U.Judge()
    for f32 in ((False, True) if cfg == 0 else (False,)):
        for gen in U.GEMM_GENS:
            saved = None
            for epi in U.GEMM_EPILOGUES:
                bwd = U.GEMM_EPILOGUES[epi].get("act", 0) in U.GEMM_BWD_ACTS
                a_k, b_k = (True, True) if (not bwd or cfg == 13) else (True, False)
                c, r, t = _case(gen, M, N, K, epi, f32, aux_in=saved if epi == "mul" else None)
                outs = _run(c, a_k, b_k, cfg)
                if epi == "gelu_save_grad":
                    saved = outs["aux_out"].clone()
                if epi == "gelu_bwd_res" and cfg != 0:
                    assert _same(outs, _run(c, a_k, b_k, 0))
                fused = c["colsum"] and cfg in U.GEMM_CS_ROWS and not f32
                shape = "%dx%dx%d %s %s %s %s" % (M, N, K, gen, epi, _lay(a_k, b_k), "f32" if f32 else "bf16")
                U.judge_gemm(J, "epi-cfg%d" % cfg, shape, c, r, t, outs, cs_rows=U.GEMM_CS_ROWS[cfg] if fused else None)
    J.check()


# ------------------------------------------------------------------------------- batched, causal
def _sub(d, rows, cols):
    return {"aux_out": None, **{k: d[k][..., rows, cols] for k in ("C", "S", "S_rel")}}


def test_batched_and_causal():
    """what ops/attention.py launches, on cfg 0: batch = 3 x 2 with two-level strides (the inner
    batch interleaved in the operand rows, as heads are), and the three causal modes with the
    triangular operands they are fed.  Mode 1 promises only the tiles that touch the lower
    triangle: those are judged, the skipped one keeps its NaN."""
    G = _G()
    Zo, Zi, M, N, K = U.GEMM_BATCH
    J = U.Judge()
    heads = lambda x: x.permute(0, 2, 1, 3).contiguous()   # [Zo, Zi, R, K] -> [Zo, R, Zi, K]
    for gen in U.GEMM_GENS:
        a, b = U.gemm_inputs(gen, M, N, K, batch=(Zo, Zi), dev=DEV)
        A, B = heads(a), heads(b.transpose(-1, -2))
        kw = {"alpha": 0.125}
        r, t = U.gemm_ref(F64, a, b, True, False, **kw), U.gemm_ref(F32, a, b, True, False, **kw)
        for f32 in (False, True):
            for causal in (0, 1):
                C = torch.full((Zo, Zi, M, N), NAN, dtype=F32 if f32 else BF16, device=DEV)
                G.gemm_bf16(A, B, C, M, N, K, Zi * K, Zi * K, N, True, True, causal=causal, batch=Zo * Zi, batch_inner=Zi,
                            strides=(M * Zi * K, K, N * Zi * K, K, Zi * M * N, M * N), **kw)
                torch.cuda.synchronize()
                c = {"K": K, "M": M, "out_fp32": f32, "colsum": False}
                shape = "%dx%dx%dx%d %s %s" % (Zo * Zi, M, N, K, gen, "f32" if f32 else "bf16")
                if causal == 0:
                    U.judge_gemm(J, "batched", shape, c, r, t, {"C": C})
                    continue
                assert bool(torch.isnan(C[..., :128, 128:]).all()), "mode 1 wrote a tile above the diagonal"
                for rows, cols in ((slice(0, 128), slice(0, 128)), (slice(128, M), slice(0, N))):
                    U.judge_gemm(J, "causal1", shape + " rows %d:" % rows.start, c, _sub(r, rows, cols), _sub(t, rows, cols),
                                 {"C": C[..., rows, cols]})
        # modes 2 (k <= the row tile's last row: P.V, dS.K) and 3 (k >= the row tile's first row:
        # dS^T.Q, P^T.dO): T = 192 rows and keys, 64 columns
        T, Dh = 192, 64
        a, b = U.gemm_inputs(gen, T, Dh, T, batch=(Zo, Zi), dev=DEV)
        for causal, a_k, tri in ((2, True, torch.tril), (3, False, torch.triu)):
            at = tri(a)
            A, B = U.gemm_store(at, b, a_k, False)
            r, t = U.gemm_ref(F64, at, b, True, False), U.gemm_ref(F32, at, b, True, False)
            for f32 in (False, True):
                C = torch.full((Zo, Zi, T, Dh), NAN, dtype=F32 if f32 else BF16, device=DEV)
                G.gemm_bf16(A, B, C, T, Dh, T, T, Dh, Dh, a_k, False, causal=causal, batch=Zo * Zi, batch_inner=Zi,
                            strides=(Zi * T * T, T * T, Zi * T * Dh, T * Dh, Zi * T * Dh, T * Dh))
                torch.cuda.synchronize()
                c = {"K": T, "M": T, "out_fp32": f32, "colsum": False}
                U.judge_gemm(J, "causal%d" % causal, "%dx%dx%dx%d %s %s" % (Zo * Zi, T, Dh, T, gen, "f32" if f32 else "bf16"),
                             c, r, t, {"C": C})
    J.check()


# ------------------------------------------------------------------------------- grouped weight gradients
def _grouped(J, op, gen, products, tokens, acc):
    As, Bs, outs, dims, refs = [], [], [], [], []
    g = torch.Generator().manual_seed(len(products) + sum(tokens))
    for (N, K), T, flag in zip(products, tokens, acc):
        a, b = U.gemm_inputs(gen, N, K, T, dev=DEV)            # dW[N, K] = dY[T, N]^T X[T, K]
        dy, x = U.gemm_store(a, b, False, False)
        pre = torch.randn(N, K, generator=g).to(DEV) if flag else None
        kw = {"Cin": pre, "beta": 1.0} if flag else {}
        refs.append((U.gemm_ref(F64, a, b, True, False, **kw), U.gemm_ref(F32, a, b, True, False, **kw)))
        As.append(dy)
        Bs.append(x)
        outs.append(pre.clone() if flag else torch.full((N, K), NAN, dtype=F32, device=DEV))
        dims += [N, K, T, N, K, K]
    _ext().gemm_bf16_grouped(As, Bs, outs, dims, False, False, list(acc) if any(acc) else None)
    torch.cuda.synchronize()
    for (N, K), T, flag, out, (r, t) in zip(products, tokens, acc, outs, refs):
        c = {"K": T, "M": N, "out_fp32": True, "colsum": False}
        U.judge_gemm(J, op, "%dx%dx%d %s%s" % (N, K, T, gen, " +=" if flag else ""), c, r, t, {"C": out})


@pytest.mark.parametrize("tokens", U.GEMM_GROUP_TOKENS)
def test_grouped_weight_gradients(tokens):
    """gemm_bf16_grouped, every product by Judge.rel: three products under one round of the chip
    (56 tiles, ragged N = 1000 and K-in = 2736), 332 tiles (the persistent grouped kernel walks
    several tiles per block), and - token counts mixed in one launch - the one-block-per-tile
    kernel; accumulate flags mixed, with a gradient already in the flagged outputs"""
    J = U.Judge()
    for gen in U.GEMM_GENS:
        _grouped(J, "group-small", gen, U.GEMM_GROUP_SMALL, (tokens,) * 3, (0, 1, 0))
        _grouped(J, "group-mixed", gen, U.GEMM_GROUP_SMALL, (tokens, 320, tokens), (1, 0, 0))
    _grouped(J, "group-big", "randn", U.GEMM_GROUP_BIG, (tokens,) * 3, (0, 1, 1))
    _grouped(J, "group-big", "range", U.GEMM_GROUP_BIG, (tokens,) * 3, (0, 0, 0))
    J.check()


# ------------------------------------------------------------------------------- gemm_f32
def test_gemm_f32():
    """the exact-fp32 MFMA kernel on the shapes of the fp32 model and of its tests: plain,
    bias + relu with the pre-activation as aux_out, relu-backward, beta accumulate; the weight
    K-major ([N, K], as nn.Linear holds it) and MN-major.  (The fused dropout keeps its bitwise test.)"""
    G = _G()
    J = U.Judge()
    for M, N, K in U.GEMM_F32_SHAPES:
        for epi in U.GEMM_F32_EPIS:
            for gen in U.GEMM_GENS:
                c = U.gemm_case(gen, M, N, K, epi, True, DEV, dtype=F32)
                r, t = U.gemm_ref_of(F64, c), U.gemm_ref_of(F32, c)
                for b_k in (True, False):
                    Bm = c["b"].t().contiguous() if b_k else c["b"]
                    sbk, sbn = (1, K) if b_k else (N, 1)
                    C = c["Cin"].clone() if c["cin"] else torch.full((M, N), NAN, device=DEV)
                    aux = torch.full((M, N), NAN, device=DEV) if c["act"] == 1 else None
                    G.gemm_f32(c["a"], Bm, C, M, N, K, K, 1, sbk, sbn, N, Cin=C if c["cin"] else None, bias=c["bias"],
                               aux_in=c["aux_in"], aux_out=aux, alpha=c["alpha"], beta=c["beta"], act=c["act"])
                    torch.cuda.synchronize()
                    outs = {"C": C} if aux is None else {"C": C, "aux_out": aux}
                    U.judge_gemm(J, "gemm_f32", "%dx%dx%d %s %s B%s" % (M, N, K, gen, epi, "K" if b_k else "M"), c, r, t,
                                 outs, aux_fp32=True)
    J.check()
