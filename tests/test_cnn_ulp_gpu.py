"""The convolution, BatchNorm and pooling kernels (ResNet path) judged per element against fp64 (GPU only).

The yardstick is the CNN section of tests/ulp.py: `conv_ref`, `bn_ref` and the pool references in
float64 are the reference, in float32 the twin, both computed on the device with tap loops and
matmuls (no convolution library), once per case and shared.  A bf16 output is held to 0.5 ulp +
16 x the twin's error with a floor of FLOOR_* x the sum of |terms|, an fp32 output to
max(16 x the twin, (R + 16) 2^-24) of that sum; dx through linear_dgrad + col2im to the allowance
counted from its bf16 column values; everything that only moves data, and the max-pool forward,
to its index formula bit for bit.  Outputs of the launches made here are pre-filled with NaN (the
autograd ops of ops/cnn.py allocate their own).  Every shape has H != W.  Each judged output prints
one ULP line, each test its WORST lines; those of one run are kept in profiles/cnn_ulp_worst.txt.

The six cached native knobs are switched in this process through `conv_knobs_reload()`, which
returns what the launchers then see (one bit per knob): the arm taken is read, not assumed.

Arm -> the test that reaches it:

  conv_knobs_reload, all six knobs                                                  test_knobs_reload_reads_the_environment
  mode 1 forward + stride-1 dgrad, Cout = 64 (256x64 tiles, RTDC_CONV64_W8 0 / 1),
  Cout = 128 / 192 (128x128, RTDC_CONV128_W8 0 / 1, partial column tile), C = 128,
  3x3/2/1, 1x1/2/0, 5x5/1/2, with and without a GradStash addend                    test_conv_implicit
  dgrad through linear_dgrad + col2im (stride 2, odd sizes, addend)                 test_conv_implicit
  mode 2: > 4 tiles, non-3x3, strided; Cout = 64 on 64x256 (RTDC_CONV64WG_W8 0 / 1),
  Cout = 128 (RTDC_CONV128_W8 0 / 1); contiguous weights, and channels-last ones
  whose NaN-filled flat gradient slice the kernel writes in place                   test_conv_implicit
  the same slice written by conv3x3_wgrad_kernel, by the column path's row copy
  and by stem_dw_from_s2d                                                           test_wgrad3, test_im2col_kernels_and_column_path,
                                                                                    test_stem_space_to_depth
  mode 2 for a 3x3/1/1 (RTDC_CONV3_WGRAD=0), and long enough for pick_splitk        test_wgrad3_switched_off, test_wgrad_splitk
  conv3x3_wgrad_kernel<64>: one partial chunk, 17x19, W = 33, W = 64, uneven split  test_wgrad3
  conv3x3_wgrad_kernel<128> (RTDC_CONV3_KP=128)                                     test_wgrad3_kp128
  space-to-depth stem, nchw_to_s2d, stem_w_to_s2d, stem_dw_from_s2d, to_nhwc_bf16   test_stem_space_to_depth
  im2col_small (C = 3), im2col_stem<224, 192>, im2col vector (C = 24) and scalar
  (C = 4), col2im, conv_w_flip_t                                                    test_im2col_kernels_and_column_path
  conv_tile_stats (GM 3): 256- and 128-row tiles, partial last tile, `offset`,
  as partials, through batch_norm and through batch_norm_relu_max_pool              test_fused_statistics
  split merge (S = 4, partial last split) and RTDC_BN_SPLIT_FINALIZE=0              test_fused_statistics
  bn_reduce / bn_finalize / bn_apply / bn_bwd_apply: C = 64, 192, 512, 2056
  (generic apply loops, idle lanes, second gbase), _BN_LOADS = 1 (many row-blocks,
  empty ones, > 256 partials) and the default (nblk >= 2), relu x residual,
  residual_grad_to, backward modes 0 / 1 / 2                                        test_batchnorm, test_batchnorm_many_blocks
  FLOOR_BN_DX: the device twin's half of its rule                                   test_floor_bn_dx_on_the_device
  eval mode, num_batches_tracked                                                    test_batchnorm_eval_and_batches_tracked
  the ReLU boundary: mode 2 == mode 1 bit for bit on planted elements               test_relu_boundary_mode2_is_mode1
  conv_gemm_bnb / bnb_tile_stats (RTDC_BNB_FUSED) at C = 64 and 128, both masks     test_bnb_fused_partials
  maxpool_fwd, maxpool3s2_bwd<64>, generic maxpool_bwd, 3x3/2/1 and 2x2/2/0,
  planted ties, all-negative borders, +-0                                           test_max_pool
  bn_relu_maxpool == the unfused pair bit for bit (y and argmax)                    test_bn_relu_maxpool_is_the_unfused_pair
  pool_bn_bwd at the default _POOL_BN_BLOCKS and at 3                               test_pool_bn_bwd
  avgpool forward / backward at HW = 35, classifier at N = 10 and N = 1000          test_avg_pool_and_classifier

Not run: the `direct` branch of _Conv2d.forward (1x1 / 1 / 0 with K % 64 == 0) - such a shape has
C % 64 == 0 and _implicit_ok takes it first for every M < 2^24, so the branch is unreachable.
"""
import importlib

import pytest
import torch

from tests import ulp as U

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64, F32, BF16 = U.F64, U.F32, U.BF16
NAN = float("nan")
EPS, MOM = 1e-5, 0.1
_refs: dict = {}
KNOB_BITS = {"RTDC_CONV64_W8": 1, "RTDC_CONV128_W8": 2, "RTDC_CONV64WG_W8": 4, "RTDC_CONV3_WGRAD": 8,
             "RTDC_CONV3_KP": 16, "RTDC_BN_SPLIT_FINALIZE": 32}
KNOB_DEFAULT = 1 | 2 | 8 | 32


@pytest.fixture(scope="module", autouse=True)
def _drop_refs():
    yield
    _refs.clear()


def _cnn():
    return importlib.import_module("ray_torch_distributed_checkpoint_amd.ops.cnn")


def _ext():
    from ray_torch_distributed_checkpoint_amd.ops._ext import gpu_ext

    return gpu_ext()


@pytest.fixture
def knobs(monkeypatch):
    """set(**env) -> the knob mask the native launchers now hold; the defaults are restored (and
    re-read) afterwards"""
    for k in KNOB_BITS:
        monkeypatch.delenv(k, raising=False)
    assert _ext().conv_knobs_reload() == KNOB_DEFAULT

    def set_(**env):
        for k, v in env.items():
            monkeypatch.setenv(k, str(v))
        return _ext().conv_knobs_reload()

    yield set_
    monkeypatch.undo()
    _ext().conv_knobs_reload()


def _bits(t):
    return t.contiguous().view({F32: torch.int32, BF16: torch.int16, torch.uint8: torch.uint8}[t.dtype])


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _pix(r):
    return r["y"].numel() // r["y"].shape[-1]


# ------------------------------------------------------------------------------- convolutions
def _conv_refs(case, gen):
    """inputs and (reference, twin) with and without the addend, and for the column path"""
    key = (case, gen)
    if key not in _refs:
        _, B, H, W, C, Co, k, s, p = case
        c = U.conv_inputs(gen, B, H, W, C, Co, k, k, s, p, dev=DEV, addend=True)
        implicit = s == 1 and Co % 64 == 0
        out = {}
        for add in (False, True):
            a = (c["x"], c["w"], s, p, c["dy"], c["addend"] if add else None)
            if implicit:
                out[add] = (U.conv_ref(F64, *a), U.conv_ref(F32, *a))
            else:
                out[add] = (U.conv_ref(F64, *a, path="cols"), U.conv_ref(F32, *a, path="cols", twin=True))
        _refs[key] = (c, implicit, out)
    return _refs[key]


def _flat_slot(w):
    """w as a channels-last parameter of a FlatParamSpace in its per-step state (p.grad None), the
    whole flat gradient buffer NaN: the weight-gradient kernel writes the [Cout, K] slice itself"""
    from ray_torch_distributed_checkpoint_amd.optim import FlatParamSpace

    p = torch.nn.Parameter(w.clone().to(memory_format=torch.channels_last))
    sp = FlatParamSpace([p])
    sp.zero_grad(set_to_none=True)
    sp.grad.fill_(NAN)
    return p, sp


def _slot_holds(p, sp):
    """autograd adopted the slice as p.grad, and nothing was stored past it"""
    s = sp.segment_of(p)
    lo = sp.grad.data_ptr() + 4 * s.offset
    assert p.grad is not None and p.grad.data_ptr() == lo, "the gradient is not the flat slice"
    assert torch.isnan(sp.grad[s.offset + s.numel:]).all() and torch.isnan(sp.grad[:s.offset]).all()
    assert not torch.isnan(sp.grad[s.offset:s.offset + s.numel]).any()


def _conv_run(c, s, p, addend=False, channels_last=False, dx=True, flat=False):
    cnn = _cnn()
    x = c["x"].clone().requires_grad_(dx)
    w = c["w"].clone()
    if flat:
        w, sp = _flat_slot(w)
    elif channels_last:
        w = w.to(memory_format=torch.channels_last)
    w.requires_grad_(True)
    st = None
    if addend:   # the other consumer's gradient is already in the stash: this dgrad adds it
        st = cnn.GradStash(1)
        st.t = c["addend"].clone()
    y = cnn.conv2d(x, w, s, p, grad_accum=st)
    y.backward(c["dy"])
    torch.cuda.synchronize()
    if flat:
        _slot_holds(w, sp)
    return {"y": y.detach(), "dx": x.grad, "dw": w.grad}


def _judge_conv_case(J, op, case, gen, outs, addend, implicit, refs, names=("y", "dx", "dw")):
    r, t = refs[addend]
    shape = "%s %s%s" % (case[0], gen, " +addend" if addend else "")
    U.judge_conv(J, op, shape, r, t, outs, names=tuple(n for n in names if n != "dx" or implicit), pixels=_pix(r))
    if "dx" in names and not implicit:
        J.within("col2im", shape, "dx", outs["dx"], r["dx"], t["dx"], r["allow_dx"])


@pytest.mark.parametrize("arm", ["w8", "w4"])
@pytest.mark.parametrize("case", U.CNN_CONV_IMPLICIT, ids=U.conv_case_id)
def test_conv_implicit(case, arm, knobs):
    """forward, dgrad (implicit GEMM at stride 1, else linear_dgrad + col2im) and the weight gradient
    of every case x generator, with and without an addend.  w8: the defaults (8-wave 256x64 and
    128x128 tiles, 4-wave 64x256 weight-gradient tiles), contiguous weights (the gradient is allocated
    and copied); w4: the other value of RTDC_CONV64_W8, RTDC_CONV128_W8 and RTDC_CONV64WG_W8, and
    channels-last weights in a FlatParamSpace: mode 2 (or conv3x3_wgrad_kernel, at c64 and c128)
    writes the NaN-filled [Cout, K] gradient slice in place."""
    if arm == "w4":
        assert knobs(RTDC_CONV64_W8=0, RTDC_CONV128_W8=0, RTDC_CONV64WG_W8=1) == 4 | 8 | 32
    _, B, H, W, C, Co, k, s, p = case
    J = U.Judge()
    for gen in U.CNN_GENS:
        c, implicit, refs = _conv_refs(case, gen)
        for addend in (False, True):
            outs = _conv_run(c, s, p, addend, flat=arm == "w4")
            _judge_conv_case(J, "conv-" + arm, case, gen, outs, addend, implicit, refs,
                             names=("y", "dx", "dw") if not addend else ("dx",))
    J.check()


def _wgrad3_case(row):
    name, H, W, C, Co = row
    return (name, 3, H, W, C, Co, 3, 1, 1)


@pytest.mark.parametrize("row", U.CNN_WGRAD3, ids=lambda r: r[0])
def test_wgrad3(row, knobs):
    """conv3x3_wgrad_kernel<64> (B = 3): the halo arithmetic at W != H, partial chunks, splits"""
    case = _wgrad3_case(row)
    assert U.conv3_wgrad_plan(3, *row[1:]) is not None and U.conv3_wgrad_plan(3, *row[1:])[0] == 64
    J = U.Judge()
    c, implicit, refs = _conv_refs(case, "randn")
    for flat in (False, True):   # allocated, and written in place into the flat gradient slice
        outs = _conv_run(c, 1, 1, flat=flat)
        _judge_conv_case(J, "wgrad3<64>", case, "randn" + (" slot" if flat else ""), outs, False, implicit, refs)
    J.check()


@pytest.mark.parametrize("row", U.CNN_WGRAD3_KP128 + [U.CNN_WGRAD3[1]], ids=lambda r: r[0])
def test_wgrad3_kp128(row, knobs):
    """the same kernel on 128-pixel chunks where its 3/4-fill rule admits the shape"""
    case = _wgrad3_case(row)
    assert U.conv3_wgrad_plan(3, *row[1:], kp_env=128)[0] == 128
    c, implicit, refs = _conv_refs(case, "randn")
    base = _conv_run(c, 1, 1)["dw"]
    assert knobs(RTDC_CONV3_KP=128) == KNOB_DEFAULT | 16
    J = U.Judge()
    outs = _conv_run(c, 1, 1)
    # (99 to 128 pixels a chunk instead of 33 to 57, and other splits: another summation order)
    assert not _same(outs["dw"], base), "the 128-pixel chunks gave the bits of the 64-pixel ones"
    _judge_conv_case(J, "wgrad3<128>", case, "randn", outs, False, implicit, refs, names=("dw",))
    J.check()


@pytest.mark.parametrize("wg8", [0, 1])
def test_wgrad3_switched_off(wg8, knobs):
    """RTDC_CONV3_WGRAD=0: a 3x3 / 1 / 1 weight gradient on mode 2 of the implicit GEMM (64x256 tiles of
    4 and of 8 waves at Cout = 64, 128x128 at Cout = 128); it sums 64 padded pixels a k-tile where the
    input-reuse kernel sums whole image rows a chunk, so the bits differ from the default's"""
    rows = (U.CNN_WGRAD3[1], U.CNN_WGRAD3[2])
    base = [_conv_run(_conv_refs(_wgrad3_case(row), "randn")[0], 1, 1)["dw"] for row in rows]
    assert knobs(RTDC_CONV3_WGRAD=0, RTDC_CONV64WG_W8=wg8) == (1 | 2 | 32 | (4 if wg8 else 0))
    J = U.Judge()
    for row, b0 in zip(rows, base):
        case = _wgrad3_case(row)
        c, implicit, refs = _conv_refs(case, "randn")
        outs = _conv_run(c, 1, 1)
        assert not _same(outs["dw"], b0), "mode 2 gave the bits of conv3x3_wgrad_kernel"
        _judge_conv_case(J, "conv-mode2", case, "randn", outs, False, implicit, refs, names=("dw",))
    J.check()


def test_wgrad_splitk(knobs):
    """37 k-tiles of pixels: pick_splitk splits the mode-2 product (5x5, Cout = 64) four ways (the
    mirror of its time model, held against the launcher's workspace size here)"""
    from ray_torch_distributed_checkpoint_amd.ops import gemm as G

    case = U.CNN_WGRAD_SPLITK
    _, B, H, W, C, Co, k, s, p = case
    Kp = -(-B * H * W // 64) * 64
    assert U.pick_splitk(Co, k * k * C, Kp, -(-k * k * C // 256), G.SPLITK_WS_ELEMS) == 4
    J = U.Judge()
    c, implicit, refs = _conv_refs(case, "randn")
    outs = _conv_run(c, case[7], case[8])
    _judge_conv_case(J, "conv-splitk", case, "randn", outs, False, implicit, refs)
    J.check()


# ------------------------------------------------------------------------------- stem, layout kernels
@pytest.mark.parametrize("B,H,W", U.CNN_STEM_S2D)
def test_stem_space_to_depth(B, H, W):
    cnn, ext = _cnn(), _ext()
    g = torch.Generator().manual_seed(H * W)
    x = torch.randn(B, 3, H, W, generator=g).to(DEV)
    w = (torch.randn(64, 3, 7, 7, generator=g) * 0.1).to(DEV)
    dy = torch.randn(B, H // 2, W // 2, 64, generator=g).to(BF16).to(DEV)
    # the data movers, bit for bit
    xs = torch.full((B, H // 2, W // 2, 16), NAN, dtype=BF16, device=DEV)
    ext.stem_s2d(x, xs)
    assert _same(xs, U.s2d_ref(x))
    nhwc = cnn.to_nhwc_bf16(x)
    assert _same(nhwc, U.nhwc_bf16_ref(x))
    wm = w.to(BF16).permute(0, 2, 3, 1).reshape(64, 147).contiguous()
    wp = torch.full((64, 256), NAN, dtype=BF16, device=DEV)
    ext.stem_w_s2d(wm, wp)
    assert _same(wp, U.stem_w_s2d_ref(wm))
    dwp = torch.randn(64, 256, device=DEV)
    dwf = torch.full((64, 147), NAN, device=DEV)
    ext.stem_dw_s2d(dwp, dwf)
    assert _same(dwf, U.stem_dw_ref(dwp))
    # the convolution against the 7x7 / 2 / 3 reference
    J = U.Judge()
    r, t = (U.conv_ref(dt, nhwc, w, 2, 3, dy) for dt in (F64, F32))
    for flat in (True, False):   # flat: stem_dw_from_s2d gathers into the channels-last gradient slice
        wi, sp = _flat_slot(w) if flat else (w.clone().requires_grad_(True), None)
        y = cnn.stem_conv(x, wi, bn_stats=True)
        y.backward(dy)
        torch.cuda.synchronize()
        if flat:
            _slot_holds(wi, sp)
        outs = {"y": y.detach(), "dw": wi.grad}
        U.judge_conv(J, "stem-s2d", (B, H, W, "slot" if flat else "contig"), r, t, outs, names=("y", "dw"), pixels=_pix(r))
        _judge_tile_stats(J, "stem-s2d", (B, H, W), y)
    J.check()


def _judge_tile_stats(J, op, shape, y):
    """the epilogue's per-tile (mean, M2) against the kernel's own stored y"""
    mean_t, m2_t, bm = y._rtdc_bn_stats
    y2 = y.detach().reshape(-1, y.shape[-1])
    sr, st = U.tile_stats_ref(F64, y2, bm), U.tile_stats_ref(F32, y2, bm)
    assert mean_t.shape == sr["mean"].shape, (mean_t.shape, bm)
    J.rel(op, shape, "t-mean", mean_t, sr["mean"], st["mean"], sr["mean_scale"].clamp_min(U.TINY), U.CNN_STATS_ROWS)
    J.rel(op, shape, "t-m2", m2_t, sr["m2"], st["m2"], sr["m2_scale"].clamp_min(U.TINY), U.CNN_STATS_ROWS)
    return bm


def test_im2col_kernels_and_column_path():
    """the three im2col kernels and conv_w_flip_t against their index formulas (padding taps, k >= K
    and the rows M..Mp zero), then conv2d through the column path: C = 24 (vector gather, K = 216 ->
    Kp = 256; forward, dw, dx through col2im) and C = 4 (scalar gather; forward and dw)"""
    cnn, ext = _cnn(), _ext()
    g = torch.Generator().manual_seed(11)
    for name, B, H, W in U.CNN_STEM_COLS:
        x = torch.randn(B, H, W, 3, generator=g).to(BF16).to(DEV)
        Ho, Wo = U.out_hw(H, W, 7, 7, 2, 3)
        cols = torch.full((B * Ho * Wo, 192), NAN, dtype=BF16, device=DEV)
        ext.im2col(x, cols, Ho, Wo, 7, 7, 2, 3)
        assert _same(cols, U.im2col_ref(x, 7, 7, 2, 3, 192, B * Ho * Wo)), name
    for C, k, s, p, Kp in ((24, 3, 1, 1, 256), (24, 3, 2, 1, 256), (4, 3, 1, 1, 64), (4, 5, 2, 2, 128)):
        x = torch.randn(2, 7, 10, C, generator=g).to(BF16).to(DEV)
        Ho, Wo = U.out_hw(7, 10, k, k, s, p)
        cols = torch.full((2 * Ho * Wo, Kp), NAN, dtype=BF16, device=DEV)
        ext.im2col(x, cols, Ho, Wo, k, k, s, p)
        assert _same(cols, U.im2col_ref(x, k, k, s, p, Kp, 2 * Ho * Wo)), (C, k, s)
    for Co, k, C in ((64, 3, 64), (192, 3, 128), (64, 5, 64), (128, 1, 64)):
        wm = torch.randn(Co, k * k * C, generator=g).to(BF16).to(DEV)
        out = torch.full((C, k * k * Co), NAN, dtype=BF16, device=DEV)
        ext.conv_w_flip_t(wm, out, k, k)
        assert _same(out, U.w_flip_t_ref(wm, Co, k, k, C)), (Co, k, C)
    J = U.Judge()
    for C, dx in ((24, True), (4, False)):
        for s in (1, 2):
            case = ("cols-c%d-s%d" % (C, s), 2, 9, 11, C, 64, 3, s, 1)
            c = U.conv_inputs("randn", *case[1:6], 3, 3, s, 1, dev=DEV)
            a = (c["x"], c["w"], s, 1, c["dy"], None)
            r, t = U.conv_ref(F64, *a, path="cols"), U.conv_ref(F32, *a, path="cols", twin=True)
            for flat in (False, True):   # flat: the [Cout, Kp] product copied into the [Cout, K] slice
                outs = _conv_run(c, s, 1, dx=dx, flat=flat)
                shape = case[0] + (" slot" if flat else "")
                U.judge_conv(J, "conv-cols", shape, r, t, outs, names=("y", "dw"), pixels=_pix(r))
                if dx:
                    J.within("col2im", shape, "dx", outs["dx"], r["dx"], t["dx"], r["allow_dx"])
    J.check()


# ------------------------------------------------------------------------------- BatchNorm
def _bn_run(c, relu, res, loads=None, monkeypatch=None, stash=False, training=True, nbt=None, x=None):
    """cnn.batch_norm forward + backward on [N, C] rows (as a [1, 1, N, C] NHWC tensor)"""
    cnn = _cnn()
    if loads is not None:
        monkeypatch.setattr(cnn, "_BN_LOADS", loads)
    xi = (c["x"] if x is None else x).detach().clone().requires_grad_(True)
    if x is not None and hasattr(x, "_rtdc_bn_stats"):
        xi._rtdc_bn_stats = x._rtdc_bn_stats
    g, b = c["gamma"].clone().requires_grad_(True), c["beta"].clone().requires_grad_(True)
    rm, rv = c["rm"].clone(), c["rv"].clone()
    ri = c["res"].view(xi.shape).clone().requires_grad_(True) if res else None
    st = None
    extra = None
    if stash:   # the shortcut's gradient joins another consumer's, left in the stash before
        st = cnn.GradStash(1)
        extra = torch.randn(xi.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3)).to(BF16)
        st.t = extra.clone()
    y = cnn.batch_norm(xi, g, b, rm, rv, training, MOM, EPS, residual=ri, relu=relu, num_batches_tracked=nbt,
                       residual_grad_to=st)
    outs = {"y": y.detach(), "running_mean": rm, "running_var": rv}
    if training:
        y.backward(c["dy"].view(y.shape))
        outs.update(dx=xi.grad, dgamma=g.grad, dbeta=b.grad)
        if res:
            outs["dres"] = ri.grad
            outs["extra"] = extra
    torch.cuda.synchronize()
    return outs


def _judge_bn_case(J, op, shape, c, relu, res, outs, R, x=None):
    """reference and twin with the mask of the kernel's own forward (stored y > 0)"""
    C = c["gamma"].numel()
    x2 = (c["x"] if x is None else x).detach().reshape(-1, C)
    a = (x2, c["gamma"], c["beta"], EPS, MOM, c["rm"], c["rv"], c["res"] if res else None, relu)
    mask = (outs["y"].reshape(-1, C) > 0) if relu else None
    r, t = (U.bn_ref(dt, *a, mask=mask, dy=c["dy"]) for dt in (F64, F32))
    flat = {n: (v.reshape(-1, C) if v.dim() > 1 else v) for n, v in outs.items() if v is not None}
    U.judge_bn(J, op, shape, r, t, flat, R, bwd=("dx", "dgamma", "dbeta"))
    if res and "dres" in flat:   # dres = the masked gradient, a copy (+ what the stash held, one rounding)
        want = r["dres"].to(BF16)
        if flat.get("extra") is not None:
            want = (want.float() + flat["extra"].float()).to(BF16)
        assert _same(flat["dres"], want), (op, shape, "dres")
    return r


CNN_BN_WAYS = ((False, False), (True, False), (True, True), (False, True))   # (relu, residual)


@pytest.mark.parametrize("N,C", U.CNN_BN + [U.CNN_BN_BIG])
def test_batchnorm(N, C, monkeypatch):
    """relu x residual (backward modes 0, 1, 2 and mode 1 by RTDC_BN_MASK_FROM_X=0) on every generator,
    at the default _BN_LOADS and at 1 (many row-blocks, empty trailing ones)"""
    cnn = _cnn()
    J = U.Judge()
    for gen in U.CNN_GENS + ("planted",):
        c = U.bn_inputs(gen, N, C, dev=DEV, res=True)
        for loads in (32, 1):
            nblk = U.bn_blocks(N, C, loads)
            R = U.bn_serial_rows(N, C, nblk)
            for relu, res in CNN_BN_WAYS:
                outs = _bn_run(c, relu, res, loads, monkeypatch, stash=res and relu)
                _judge_bn_case(J, "bn", (gen, N, C, "relu%d res%d nblk%d" % (relu, res, nblk)), c, relu, res, outs, R)
        monkeypatch.setattr(cnn, "_BN_MASK_FROM_X", False)   # ReLU without a residual on mode 1
        outs = _bn_run(c, True, False, 32, monkeypatch)
        _judge_bn_case(J, "bn-mode1", (gen, N, C), c, True, False, outs, U.bn_serial_rows(N, C, U.bn_blocks(N, C)))
        monkeypatch.setattr(cnn, "_BN_MASK_FROM_X", True)
    J.check()


def test_floor_bn_dx_on_the_device():
    """the device's half of what fixes FLOOR_BN_DX (tests/ulp.py): the twin as this device computes it
    holds at the floor and is over its ceiling at half of it on the 35 x 2056 planted case"""
    N, C = 35, 2056
    c = U.bn_inputs("planted", N, C, dev=DEV)
    a = (c["x"], c["gamma"], c["beta"], EPS, MOM, c["rm"], c["rv"], None, True)
    r = U.bn_ref(F64, *a, dy=c["dy"])
    t = U.bn_ref(F32, *a, mask=r["y"] > 0, dy=c["dy"])
    at, half = (U.ulp_err(t["dx"], r["dx"], f * r["S_dx"]) for f in (U.FLOOR_BN_DX, U.FLOOR_BN_DX / 2))
    print("device twin at the floor", at, "at half the floor", half)
    assert at <= U.TWIN_ULP_CEIL < half, (at, half)


def test_batchnorm_many_blocks(monkeypatch):
    """305 row-blocks (the last 9 empty): bn_finalize_kernel and bn_bwd_finalize_kernel wrap their
    256 / 64 threads"""
    N, C = U.CNN_BN_MANY
    nblk = U.bn_blocks(N, C, 1)
    assert nblk > 256 and "empty_block" in U.bn_reduce_branches(N, C, nblk)
    J = U.Judge()
    for gen in ("offset", "planted"):
        c = U.bn_inputs(gen, N, C, dev=DEV, res=True)
        for relu, res in ((True, False), (True, True)):
            outs = _bn_run(c, relu, res, 1, monkeypatch)
            _judge_bn_case(J, "bn-many", (gen, N, C, relu, res), c, relu, res, outs, U.bn_serial_rows(N, C, nblk))
    J.check()


def test_batchnorm_eval_and_batches_tracked():
    J = U.Judge()
    N, C = 231, 192
    c = U.bn_inputs("offset", N, C, dev=DEV, res=True)
    nbt = torch.tensor(41, dtype=torch.int64, device=DEV)
    _bn_run(c, True, False, nbt=nbt)
    assert nbt.item() == 42
    for relu, res in CNN_BN_WAYS:
        outs = _bn_run(c, relu, res, training=False, nbt=nbt)
        a = (c["x"], c["gamma"], c["beta"], EPS, MOM, c["rm"], c["rv"], c["res"] if res else None, relu)
        r, t = (U.bn_ref(dt, *a, training=False) for dt in (F64, F32))
        J.ulp("bn-eval", (N, C, relu, res), "y", outs["y"], r["y"], t["y"], U.FLOOR_BN_Y * r["S_y"])
        assert _same(outs["running_mean"], c["rm"]) and _same(outs["running_var"], c["rv"])
    assert nbt.item() == 42   # evaluation does not count
    J.check()


def _plant_relu_boundary(c, N, C):
    """zeros planted in x (channels c % 3 == 0), statistics from a statistics-only bn_fwd, then beta
    per channel so that the forward's fma argument of chosen elements is 0 (those channels: x = 0 and
    beta = fl(mean ka)) or the rounding residue of x0 ka, of either sign (the others: beta = fl(mean ka)
    - fl(x0 ka)).  That holds to a few fp32 roundings of mean ka, not to one: the kernels form
    kb = beta - mean ka as the compiler contracts it (an fma keeps the residue of mean ka that the
    separately rounded form here drops), so the returned `arg` is this emulation's argument, checked
    for sign and size only.  What the tests assert - mode 2 == mode 1 bit for bit - does not lean on it.
    beta does not move the statistics."""
    ext = _ext()
    x = c["x"].clone()
    rows = torch.arange(C, device=DEV) % N
    cols = torch.arange(C, device=DEV)
    zero_ch = (cols % 3 == 0) & (cols >= 3)            # (channel 0 stays constant: all of it on the boundary)
    x[rows[zero_ch], cols[zero_ch]] = 0
    x[(rows[zero_ch] + 7) % N, cols[zero_ch]] = 0
    mean, rstd = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    ws = torch.empty(2 * C, device=DEV)
    ext.bn_fwd(x, None, None, mean, rstd, c["gamma"], c["beta"], None, None, EPS, MOM, True, True, ws, 1, None, None,
               0, None)
    ka = rstd * c["gamma"]
    mk = mean * ka                                     # fp32, as the kernels form it
    x0 = x[rows, cols].float()
    beta = torch.where(zero_ch, mk, mk - x0 * ka)     # kb = beta - mk
    arg = torch.addcmul((beta - mk).double(), x0.double(), ka.double())   # the fma argument with kb rounded separately
    return x, beta, arg, ((x0 * ka).abs() + mk.abs()).double()   # ... and the size of what cancels in it


@pytest.mark.parametrize("N,C", [(231, 64), (231, 192)])
def test_relu_boundary_mode2_is_mode1(N, C, monkeypatch):
    """on elements planted on the ReLU boundary the mask recomputed from x (mode 2: bn_reduce_kernel,
    bn_bwd_apply_kernel<2>) is the mask of the stored y (mode 1): dx, dgamma and dbeta bit for bit"""
    cnn = _cnn()
    c = U.bn_inputs("planted", N, C, dev=DEV)
    x, beta, arg, size = _plant_relu_boundary(c, N, C)
    # on both sides of 0, and no further from it than a few roundings of the products that cancel
    assert (arg == 0).any() and (arg > 0).any() and (arg < 0).any()
    assert (arg.abs() <= 4 * 2.0 ** -24 * size).all()
    c = dict(c, x=x, beta=beta)
    runs = {}
    for from_x in (True, False):
        monkeypatch.setattr(cnn, "_BN_MASK_FROM_X", from_x)
        runs[from_x] = _bn_run(c, True, False)
    for n in ("y", "dx", "dgamma", "dbeta"):
        assert _same(runs[True][n], runs[False][n]), n
    J = U.Judge()
    _judge_bn_case(J, "bn-boundary", (N, C), c, True, False, runs[True], U.bn_serial_rows(N, C, 1))
    J.check()


# ------------------------------------------------------------------------------- fused statistics
@pytest.mark.parametrize("split", [1, 0])
@pytest.mark.parametrize("case", U.CNN_CONV_STATS, ids=U.conv_case_id)
def test_fused_statistics(case, split, knobs, monkeypatch):
    """conv_tile_stats partials against the stored y, then the merged statistics where they matter:
    in y (ulps) and the running statistics of batch_norm on that tensor, and in
    batch_norm_relu_max_pool (Cout = 64).  st128 has 26 tiles: the split merge runs with S = 4 and a
    partial last split at the default and at _BN_LOADS = 1; split = 0 is RTDC_BN_SPLIT_FINALIZE=0 (one
    finalize block per channel over all 26).  Both tile arms (8 and 4 waves)."""
    cnn = _cnn()
    _, B, H, W, C, Co, k, s, p = case
    J = U.Judge()
    for arm in ("w8", "w4"):
        mask = knobs(RTDC_CONV64_W8=int(arm == "w8"), RTDC_CONV128_W8=int(arm == "w8"), RTDC_BN_SPLIT_FINALIZE=split)
        assert mask == (3 if arm == "w8" else 0) | 8 | (32 if split else 0)
        for gen in U.CNN_GENS:
            c = U.conv_inputs(gen, B, H, W, C, Co, k, k, s, p, dev=DEV)
            y = cnn.conv2d(c["x"], c["w"].clone().requires_grad_(True), s, p, bn_stats=True)
            bm = _judge_tile_stats(J, "stats-" + arm, (case[0], gen), y)
            assert bm == (256 if Co <= 64 else 128)
            N = y.numel() // Co
            tiles = -(-N // bm)
            b = U.bn_inputs("randn", N, Co, dev=DEV)
            for loads in (32, 1):
                plan = U.bn_split(tiles, Co, U.bn_blocks(N, Co, loads), enabled=bool(split))
                assert plan == ((4, 7) if (Co == 128 and split) else None)
                outs = _bn_run(b, True, False, loads, monkeypatch, x=y)
                _judge_bn_case(J, "bn-fused-" + arm, (case[0], gen, "split" if plan else "finalize", loads), b, True,
                               False, outs, U.CNN_STATS_ROWS + tiles, x=y)
            if Co == 64:
                g, be = b["gamma"].clone(), b["beta"].clone()
                pair, fused = [], []
                for fn, keep in ((lambda xi, rm, rv: cnn.max_pool2d(cnn.batch_norm(xi, g, be, rm, rv, True, MOM, EPS,
                                                                                   relu=True), 3, 2, 1), pair),
                                 (lambda xi, rm, rv: cnn.batch_norm_relu_max_pool(xi, g, be, rm, rv, True, MOM, EPS),
                                  fused)):
                    xi = y.detach().clone()
                    xi._rtdc_bn_stats = y._rtdc_bn_stats
                    rm, rv = b["rm"].clone(), b["rv"].clone()
                    keep += [fn(xi, rm, rv), rm, rv]
                for u, v, n in zip(pair, fused, ("y", "running_mean", "running_var")):
                    assert _same(u, v), n
    J.check()


# ------------------------------------------------------------------------------- BN backward statistics in the dgrad
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("C", [64, 128])
def test_bnb_fused_partials(C, residual, monkeypatch):
    """BN + ReLU -> conv2: with RTDC_BNB_FUSED conv2's dgrad epilogue (conv_gemm_bnb) reduces the
    BatchNorm backward's (sum g, sum g xhat) per row tile.  The partials are judged against the kernel's
    own stored gradient and the mask of the stored y (the epilogue recomputes it from x, on the planted
    boundary, or reads y with a residual), over 3 x 13 x 11 = 429 pixels (a partial last tile), and the
    BatchNorm backward built on them is judged per element.  Against the unfused pass the sums run in
    another order (tiles, not row-blocks), so no bits are compared with it; what must be bitwise is the
    mask: without a residual the same launch is repeated with the mask read from y
    (RTDC_BN_MASK_FROM_X=0) and its partials, dgamma, dbeta and dx equal the from-x ones bit for bit."""
    cnn = _cnn()
    B, H, W = 3, 13, 11
    N = B * H * W
    c = U.conv_inputs("randn", B, H, W, C, C, 3, 3, 1, 1, dev=DEV)   # dy, and x as the residual
    w2 = torch.randn(C, C, 3, 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(C)) * (9 * C) ** -0.5
    b = U.bn_inputs("planted", N, C, dev=DEV)
    if not residual:   # the mask comes from x: put elements on the boundary
        xp, beta = _plant_relu_boundary(b, N, C)[:2]
        b = dict(b, x=xp, beta=beta)
    taken, parts = [], []
    orig = cnn._take_bnb

    def spy(g):
        r = orig(g)
        taken.append(r is not None)
        if r is not None:
            parts.append((r, g.detach().clone()))
        return r

    monkeypatch.setattr(cnn, "_take_bnb", spy)
    runs = {}
    for fused in (False, True) + (() if residual else ("from_y",)):
        monkeypatch.setattr(cnn, "_BNB_FUSED", bool(fused))
        monkeypatch.setattr(cnn, "_BN_MASK_FROM_X", fused != "from_y")
        x = b["x"].view(B, H, W, C).clone().requires_grad_(True)
        g, be = b["gamma"].clone().requires_grad_(True), b["beta"].clone().requires_grad_(True)
        res = c["x"] if residual else None
        z = cnn.batch_norm(x, g, be, b["rm"].clone(), b["rv"].clone(), True, MOM, EPS, relu=True, residual=res)
        y = cnn.conv2d(z, w2, 1, 1)
        y.backward(c["dy"])
        torch.cuda.synchronize()
        runs[fused] = {"y": z.detach(), "dx": x.grad, "dgamma": g.grad, "dbeta": be.grad}
    assert taken == [False, True] + ([] if residual else [True])
    ps, gz = parts[0]
    if not residual:   # the mask recomputed from x is the mask of the stored y
        assert _same(parts[1][0], ps) and _same(parts[1][1], gz)
        for n in ("y", "dx", "dgamma", "dbeta"):
            assert _same(runs["from_y"][n], runs[True][n]), n
    bm = 256 if C <= 64 else 128
    nt = -(-N // bm)
    assert ps.shape == (2, nt, C)
    # the partials: per tile sum g mask and sum g mask xhat, from the stored gradient and the stored y
    J = U.Judge()
    mask = runs[True]["y"].reshape(N, C) > 0
    for dt, keep in ((F64, "r"), (F32, "t")):
        a = (b["x"], b["gamma"], b["beta"], EPS, MOM, b["rm"], b["rv"], None, False)
        f = U.bn_ref(dt, *a)
        gm = torch.where(mask, gz.reshape(N, C).to(dt), torch.zeros((), dtype=dt, device=DEV))
        xh = (b["x"].to(dt) - f["mean"]) * f["rstd"]
        pad = lambda v: torch.cat([v, v.new_zeros(nt * bm - N, C)]).view(nt, bm, C)
        runs[keep] = {"s": pad(gm).sum(1), "sx": pad(gm * xh).sum(1), "s_scale": pad(gm.abs()).sum(1),
                      "sx_scale": pad(gm.abs() * f["rstd"] * (b["x"].to(dt).abs() + f["mean"].abs())).sum(1)}
    r, t = runs["r"], runs["t"]
    J.rel("bnb", (C, residual), "sum g", ps[0], r["s"], t["s"], r["s_scale"].clamp_min(U.TINY), U.CNN_STATS_ROWS)
    J.rel("bnb", (C, residual), "sum gx", ps[1], r["sx"], t["sx"], r["sx_scale"].clamp_min(U.TINY), U.CNN_STATS_ROWS)
    # and the BatchNorm backward built on them, per element (dy of the BatchNorm = the stored dgrad)
    bb = dict(b, dy=gz.reshape(N, C), res=c["x"].reshape(N, C) if residual else None)
    outs = dict(runs[True])
    _judge_bn_case(J, "bn-bnb", (C, residual), bb, True, residual, outs, U.CNN_STATS_ROWS + nt)
    J.check()


# ------------------------------------------------------------------------------- pools
@pytest.mark.parametrize("case", U.CNN_POOLS, ids=lambda c: "B%d-%dx%d-C%d-k%ds%dp%d" % c)
def test_max_pool(case):
    """forward bit for bit (the first maximum in (kh, kw) order and its tap), backward per element:
    maxpool3s2_bwd<64> at C = 64 and 3x3/2/1, the generic gather otherwise"""
    ext = _ext()
    B, H, W, C, k, s, p = case
    J = U.Judge()
    for gen in ("randn", "planted"):
        c = U.pool_inputs(gen, B, H, W, C, k, s, p, dev=DEV)
        Ho, Wo = U.out_hw(H, W, k, k, s, p)
        y = torch.full((B, Ho, Wo, C), NAN, dtype=BF16, device=DEV)
        arg = torch.full((B, Ho, Wo, C), 255, dtype=torch.uint8, device=DEV)
        ext.maxpool_fwd(c["x"], y, arg, k, s, p)
        f = U.maxpool_ref(c["x"], k, s, p)
        assert torch.equal(y.float(), f["y"].float()), gen
        assert _same(y, f["y"]), (gen, "the sign of a zero")
        assert torch.equal(arg, f["arg"]), gen
        dx = torch.full((B, H, W, C), NAN, dtype=BF16, device=DEV)
        ext.maxpool_bwd(c["dy"], arg, dx, k, s, p)
        r, t = (U.maxpool_bwd_ref(dt, c["dy"], f["arg"], H, W, k, s, p) for dt in (F64, F32))
        J.ulp("maxpool", case + (gen,), "dx", dx, r["dx"], t["dx"], 0.0)
    J.check()


def _stats_only(x, gamma, beta):
    C = x.shape[-1]
    mean, rstd = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    _ext().bn_fwd(x, None, None, mean, rstd, gamma, beta, None, None, EPS, MOM, True, True,
                  torch.empty(2 * C, device=DEV), 1, None, None, 0, None)
    return mean, rstd


@pytest.mark.parametrize("case", [c for c in U.CNN_POOLS if c[3] == 64 or c[4] == 2], ids=lambda c: "%dx%d-C%d-k%d" % c[1:5])
def test_bn_relu_maxpool_is_the_unfused_pair(case):
    """on planted inputs (ties, all-negative borders, elements on the ReLU boundary) the fused kernel's y
    and argmax are those of bn_apply + maxpool_fwd bit for bit"""
    ext = _ext()
    B, H, W, C, k, s, p = case
    N = B * H * W
    c = U.pool_inputs("planted", B, H, W, C, k, s, p, dev=DEV)
    b = U.bn_inputs("planted", N, C, dev=DEV)
    b = dict(b, x=(c["x"].reshape(N, C).float() * 0.5 + b["x"].float() * 0.25).to(BF16))
    b["x"][:, 0] = 1.5
    x2, beta = _plant_relu_boundary(b, N, C)[:2]
    x = x2.view(B, H, W, C).contiguous()
    mean, rstd = _stats_only(x, b["gamma"], beta)
    Ho, Wo = U.out_hw(H, W, k, k, s, p)
    full = torch.full((B, H, W, C), NAN, dtype=BF16, device=DEV)
    ext.bn_fwd(x, None, full, mean, rstd, b["gamma"], beta, None, None, EPS, MOM, False, True,
               torch.empty(2 * C, device=DEV), 1, None, None, 0, None)
    outs = []
    for fused in (False, True):
        y = torch.full((B, Ho, Wo, C), NAN, dtype=BF16, device=DEV)
        arg = torch.full((B, Ho, Wo, C), 255, dtype=torch.uint8, device=DEV)
        if fused:
            ext.bn_relu_maxpool(x, mean, rstd, b["gamma"], beta, y, arg, k, s, p)
        else:
            ext.maxpool_fwd(full, y, arg, k, s, p)
        outs.append((y, arg))
    assert _same(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    f = U.maxpool_ref(full, k, s, p)
    assert _same(outs[1][0], f["y"]) and torch.equal(outs[1][1], f["arg"])


@pytest.mark.parametrize("blocks", [1024, 3])
@pytest.mark.parametrize("H,W", [(9, 12), (10, 7)])
def test_pool_bn_bwd(H, W, blocks, monkeypatch):
    """the stem backward that never stores the pool gradient (pool_bn_bwd_*_kernel<64>), at the default
    block count and at 3 (every thread loops): dx per element, dgamma / dbeta with Judge.rel, against
    maxpool backward (rounded to bf16 as the kernel rounds it) followed by the BatchNorm backward"""
    cnn = _cnn()
    monkeypatch.setattr(cnn, "_POOL_BN_BLOCKS", blocks)
    B, C = 2, 64
    N = B * H * W
    J = U.Judge()
    for gen in ("randn", "planted"):
        b = U.bn_inputs(gen, N, C, dev=DEV)
        x = b["x"].view(B, H, W, C).clone().requires_grad_(True)
        g, be = b["gamma"].clone().requires_grad_(True), b["beta"].clone().requires_grad_(True)
        y = cnn.batch_norm_relu_max_pool(x, g, be, b["rm"].clone(), b["rv"].clone(), True, MOM, EPS)
        Ho, Wo = y.shape[1:3]
        dy = U.pool_inputs("randn", B, H, W, C, 3, 2, 1, dev=DEV)["dy"]
        y.backward(dy)
        torch.cuda.synchronize()
        # the unfused forward gives the stored BN output (the mask) and the argmax
        mean, rstd = _stats_only(b["x"].view(B, H, W, C), b["gamma"], b["beta"])
        full = torch.empty(B, H, W, C, dtype=BF16, device=DEV)
        _ext().bn_fwd(b["x"].view(B, H, W, C), None, full, mean, rstd, b["gamma"], b["beta"], None, None, EPS, MOM,
                      False, True, torch.empty(2 * C, device=DEV), 1, None, None, 0, None)
        f = U.maxpool_ref(full, 3, 2, 1)
        assert _same(y.detach(), f["y"])
        dz = U.maxpool_bwd_ref(F64, dy, f["arg"], H, W, 3, 2, 1)["dx"].to(BF16)
        bb = dict(b, dy=dz.reshape(N, C))
        outs = {"y": full, "dx": x.grad, "dgamma": g.grad, "dbeta": be.grad}
        a = (b["x"], b["gamma"], b["beta"], EPS, MOM, b["rm"], b["rv"], None, True)
        mask = full.reshape(N, C) > 0
        r, t = (U.bn_ref(dt, *a, mask=mask, dy=bb["dy"]) for dt in (F64, F32))
        rows = -(-N * 8 // (min(blocks, 1024) * 256)) + 32 + -(-blocks // 64)   # a thread's rows, its block, the finalize
        U.judge_bn(J, "pool_bn_bwd", (gen, H, W, blocks), r, t, {n: (v.reshape(-1, C) if v.dim() > 1 else v)
                                                                  for n, v in outs.items()}, rows, fwd=(),
                   bwd=("dx", "dgamma", "dbeta"))
    J.check()


def test_avg_pool_and_classifier():
    cnn = _cnn()
    J = U.Judge()
    B, H, W, C = U.CNN_AVGPOOL
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, H, W, C, generator=g).to(BF16).to(DEV).requires_grad_(True)
    dy = torch.randn(B, C, generator=g).to(BF16).to(DEV)
    y = cnn.global_avg_pool(x)
    y.backward(dy)
    r, t = (U.avgpool_ref(dt, x.detach(), dy) for dt in (F64, F32))
    J.ulp("avgpool", U.CNN_AVGPOOL, "y", y.detach(), r["y"], t["y"], 0.0)
    J.ulp("avgpool", U.CNN_AVGPOOL, "dx", x.grad, r["dx"], t["dx"], 0.0)
    for Bn, N in ((6, 10), (64, 1000)):
        K = 512
        h = torch.randn(Bn, K, generator=g).to(BF16).to(DEV).requires_grad_(True)
        w = (torch.randn(N, K, generator=g) * K ** -0.5).to(DEV).requires_grad_(True)
        b = torch.randn(N, generator=g).to(DEV).requires_grad_(True)
        dl = torch.randn(Bn, N, generator=g).to(BF16).to(DEV)
        y = cnn.classifier(h, w, b)
        y.backward(dl)
        wb = w.detach().to(BF16)
        fw = [U.gemm_ref(dt, h.detach(), wb, True, True, bias=b.detach()) for dt in (F64, F32)]
        J.ulp("classifier", (Bn, N), "y", y.detach(), fw[0]["C"], fw[1]["C"], U.FLOOR_GEMM * fw[0]["S"])
        dxr = [U.gemm_ref(dt, dl, wb, True, False) for dt in (F64, F32)]
        J.ulp("classifier", (Bn, N), "dx", h.grad, dxr[0]["C"], dxr[1]["C"], U.FLOOR_GEMM * dxr[0]["S"])
        dwr = [U.gemm_ref(dt, dl, h.detach(), False, False) for dt in (F64, F32)]
        J.rel("classifier", (Bn, N), "dw", w.grad, dwr[0]["C"], dwr[1]["C"], dwr[0]["S"].clamp_min(U.TINY), 64)
        J.rel("classifier", (Bn, N), "db", b.grad, dl.double().sum(0), dl.float().sum(0), dl.double().abs().sum(0), 64)
    J.check()


def test_knobs_reload_reads_the_environment(knobs):
    """every knob's other value reaches the native launchers without a new process"""
    other = {"RTDC_CONV64_W8": 0, "RTDC_CONV128_W8": 0, "RTDC_CONV64WG_W8": 1, "RTDC_CONV3_WGRAD": 0,
             "RTDC_CONV3_KP": 128, "RTDC_BN_SPLIT_FINALIZE": 0}
    mask = KNOB_DEFAULT
    for k, v in other.items():
        mask ^= KNOB_BITS[k]
        assert knobs(**{k: v}) == mask, k
    assert mask == KNOB_DEFAULT ^ 63
