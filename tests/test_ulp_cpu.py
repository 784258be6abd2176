"""The ulp yardstick of tests/ulp.py, checked without a GPU:

* the metric: an RNE rounding to bf16 scores <= 0.5 ulp, one element moved by one ulp scores >= 1;
* the twin condition: on every case generator that tests/test_row_kernels_gpu.py runs, the fp32
  twin of each reference stays <= 2^-4 ulp (bf16 outputs) / <= 2^-18 relative (fp32 outputs) of
  the fp64 reference, i.e. the FLOOR_* constants and the inputs are well chosen;
* sensitivity: a deliberately wrong twin, rounded to bf16, exceeds the allowance that a kernel is
  given on the same case;
* attention (the last section): the twin with the kernels' bf16 roundings stays inside the derived
  per-element allowance on every case of the table, plain and under every document layout; ten
  deliberate errors leave it; the launch grids of the table meet every branch of xcd_grid; the
  older whole-tensor yardstick accepts three of those errors;
* GEMM (after it): the fp32 twin of `gemm_ref` stays under its ceilings on every case of the GEMM
  table, which fixes FLOOR_GEMM (half of it leaves the ceiling); eight deliberate errors each
  leave the allowance on the output they corrupt, at (520, 392, 192) and at the split-K shape
  (264, 264, 2048); the whole-tensor yardstick accepts four of them on a bf16 output.
"""
import pytest
import torch

from tests import ulp as U

F64, F32 = U.F64, U.F32


# ------------------------------------------------------------------------------- the metric
def test_metric_rne_rounding_is_half_an_ulp_and_one_step_is_one():
    gen = torch.Generator().manual_seed(1)
    ref = torch.cat([torch.randn(4096, generator=gen, dtype=F64) * s for s in (1e-6, 1.0, 3e4)])
    ref = torch.cat([ref, torch.tensor([1.0, 2.0, 0.99999, 1.00001, -255.9, 2.0 ** -30], dtype=F64)])
    ref = ref.float().double()  # fp32 values, so that torch's fp64 -> fp32 -> bf16 conversion rounds once
    out = ref.to(U.BF16)  # torch rounds to nearest even
    e = U.ulp_err(out, ref, U.TINY)
    assert 0.25 < e <= 0.5
    # spacing of the reference's binade
    assert U.ulp_bf16(torch.tensor([1.0, 1.99, 2.0, 0.75], dtype=F64)).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6,
                                                                                     2.0 ** -8]
    moved = out.double().clone()
    moved[17] += U.ulp_bf16(ref[17].abs())
    assert U.ulp_err(moved, ref, U.TINY) >= 1.0
    # the floor: an element far below it is judged in the floor's last place
    assert U.ulp_err(torch.tensor([0.0]), torch.tensor([2.0 ** -20], dtype=F64), 1.0) == 2.0 ** -13
    # a per-row floor broadcasts
    r2 = torch.tensor([[1.0, 2.0 ** -12], [4.0, 1.0]], dtype=F64)
    fl = U.row_floor(r2, 2.0 ** -8)
    assert fl.shape == (2, 1) and fl[1, 0] == 2.0 ** -6
    assert U.ulp_err(r2 + torch.tensor([[0.0, 2.0 ** -15], [0.0, 0.0]], dtype=F64), r2, fl) == 1.0
    # NaN never passes
    assert not U.ulp_err(torch.tensor([float("nan")]), torch.tensor([1.0], dtype=F64), 1.0) <= 1e30


def test_rel_err_and_allowances():
    ref = torch.tensor([10.0, 0.0], dtype=F64)
    assert U.rel_err(torch.tensor([10.5, 0.0]), ref, torch.tensor([100.0, 0.0])) == pytest.approx(0.005)
    assert U.rel_err(torch.tensor([10.0, 1e-30]), ref, torch.tensor([100.0, 0.0])) == float("inf")
    assert U.allow_bf16(0.0) == 0.5 + 2.0 ** -6 and U.allow_bf16(2.0 ** -4, k=2) == 2.0
    assert U.allow_f32(0.0, 5) == 21 * 2.0 ** -24 and U.allow_f32(2.0 ** -18, 1) == 2.0 ** -14


# ------------------------------------------------------------------------------- twin condition
@pytest.mark.parametrize("rms", [False, True], ids=["layernorm", "rmsnorm"])
def test_twin_norm(rms):
    J = U.Judge()
    for M, D, eps in U.norm_cases():
        for dres in ((False, True) if M >= 67 else (True,)):
            c = U.norm_inputs(M, D, dres=dres)
            U.judge_norm(J, "rmsnorm" if rms else "layernorm", (M, D, eps, "dres" if dres else ""), c, eps, rms, {})
    J.check()


def test_twin_xent():
    J = U.Judge()
    for dt, V, ld, arm in U.XENT_ARMS:
        for planted in (False, True):
            c = U.xent_inputs(dt, V, ld, planted)
            for gs in (1.0, 1.0 / 7):
                U.judge_xent(J, "xent", (arm, V, ld, "planted" if planted else "randn", round(gs, 3)), c, gs, {})
    for dt, V in U.XENT_WRAPPER:
        c = U.xent_wrapper_inputs(dt, V)
        r = U.judge_xent(J, "xent-wrap", (str(dt)[6:], V), c, 1.0, {})
        n = int((c["target"] != U.IGNORE_INDEX).sum())
        (m64, sc), (m32, _) = U.mean_loss_ref(F64, r["loss"], n), U.mean_loss_ref(F32, r["loss"], n)
        J.rel("xent-wrap", (str(dt)[6:], V), "mean", None, m64, m32, sc, 1)
    J.check()


def test_twin_softmax():
    J = U.Judge()
    for rows, T, causal in U.SOFTMAX_CASES:
        c = U.softmax_inputs(rows, T, causal)
        _, t = U.judge_softmax_fwd(J, (rows, T, "causal" if causal else "full"), c, T, causal, {})
        # the backward reads the bf16 P that the forward wrote
        U.judge_softmax_bwd(J, (rows, T, "causal" if causal else "full"), t["P"].to(U.BF16), c["dP"], T, causal, None)
    J.check()


def test_twin_swiglu_and_rope():
    J = U.Judge()
    for M, F in U.SWIGLU_CASES:
        U.judge_swiglu(J, (M, F), U.swiglu_inputs(M, F), {})
    for Dh, H, Hkv in U.ROPE_CASES:
        c = U.rope_inputs(Dh, H, Hkv)
        for inverse in (False, True):
            U.judge_rope(J, (Dh, H, Hkv, "inv" if inverse else "fwd"), c["x"], H, Hkv, Dh, inverse, None)
        U.judge_rope(J, (Dh, H, Hkv, "bwd"), c["dy"], H, Hkv, Dh, True, None, "dx")   # apply_rope's backward
    J.check()


# ------------------------------------------------------------------------------- sensitivity
def _ulp_caught(mut, ref, twin, floor, k=1):
    """the mutant, rounded to bf16 like a kernel output, is outside the allowance"""
    allow = U.allow_bf16(U.ulp_err(twin, ref, floor), k)
    e = U.ulp_err(mut.to(U.BF16), ref, floor)
    # the honest twin, rounded the same way, is inside it
    assert U.ulp_err(twin.to(U.BF16), ref, floor) <= allow
    return e > allow


def _rel_caught(mut, ref, twin, scale, R):
    allow = U.allow_f32(U.rel_err(twin, ref, scale), R)
    return U.rel_err(mut, ref, scale) > allow


@pytest.mark.parametrize("mutant,outputs", [("beta", ["y"]), ("var", ["y"]), ("eps", ["y", "dx"]), ("m1", ["dx"]),
                                            ("dres", ["dx"]), ("dgamma", ["dgamma"])])
def test_mutant_layernorm(mutant, outputs):
    M, D, eps = 5, 200, 1e-5
    c = U.norm_inputs(M, D, dres=True)
    a = (c["x"], c["g"], c["b"], eps, c["dy"], c["dres"], False)
    r, t, m = U.norm_ref(F64, *a), U.norm_ref(F32, *a), U.norm_ref(F32, *a, mutant=mutant)
    floors = {"y": U.FLOOR_LN_Y, "dx": U.FLOOR_NORM_DX}
    caught = []
    for n in outputs:
        if n in floors:
            caught.append(_ulp_caught(m[n], r[n], t[n], U.row_floor(r[n], floors[n])))
        else:
            caught.append(_rel_caught(m[n], r[n], t[n], r[n + "_scale"], 1))
    assert any(caught), (mutant, outputs)
    if mutant == "dres":  # only the last row differs
        assert not _ulp_caught(m["dx"][:-1], r["dx"][:-1], t["dx"][:-1], U.row_floor(r["dx"][:-1], U.FLOOR_NORM_DX))


@pytest.mark.parametrize("mutant", ["onehot", "padding", "ignored"])
def test_mutant_xent(mutant):
    V, ld = 333, 344
    c = U.xent_inputs(U.BF16, V, ld, planted=False)
    a = (c["logits"], c["target"], V, 1.0 / 7)
    r, t, m = U.xent_ref(F64, *a), U.xent_ref(F32, *a), U.xent_ref(F32, *a, mutant=mutant)
    assert _ulp_caught(m["grad"], r["grad"], t["grad"], U.xent_grad_floor(r, 1.0 / 7))


def test_planted_rows_tell_first_from_last_argmax():
    """a check on the data: on the planted rows an argmax that took the last of equal maxima would
    differ from first_argmax, which the GPU test compares with torch.equal"""
    for dt, V, ld, _ in [U.XENT_ARMS[0], U.XENT_ARMS[5], U.XENT_ARMS[10], U.XENT_ARMS[13]]:
        c = U.xent_inputs(dt, V, ld, planted=True)
        first, last = U.first_argmax(c["logits"], V), U.last_argmax(c["logits"], V)
        assert (first[:2] != last[:2]).all() and first[3] == 0 and last[3] == V - 1   # the two tie rows, the equal row
        assert first[2] == V - 1 and first[4] == V - 1 and (first <= last).all()
        x = c["logits"][:, :V].double()
        assert (x.gather(1, first[:, None]) == x.amax(1, keepdim=True)).all()


def test_mutant_softmax_diagonal_excluded():
    rows, T = 24, 8
    c = U.softmax_inputs(rows, T, True)
    r, t, m = (U.softmax_ref(F64, c["S"], T, True), U.softmax_ref(F32, c["S"], T, True),
               U.softmax_ref(F32, c["S"], T, True, mutant="diag"))
    assert _ulp_caught(m["P"], r["P"], t["P"], U.row_floor(r["P"], U.FLOOR_SOFTMAX_P))


@pytest.mark.parametrize("mutant", ["ksign", "nowrap"])
def test_mutant_rope(mutant):
    Dh, H, Hkv = 16, 4, 2
    c = U.rope_inputs(Dh, H, Hkv)
    a = (c["x"], U.ROPE_T, H, Hkv, Dh)
    r, t, m = U.rope_ref(F64, *a), U.rope_ref(F32, *a), U.rope_ref(F32, *a, mutant=mutant)
    assert _ulp_caught(m, r, t, U.row_floor(r, U.FLOOR_ROPE))
    if mutant == "ksign":  # only the K heads differ
        assert not _ulp_caught(m[:, :, :H], r[:, :, :H], t[:, :, :H], U.row_floor(r[:, :, :H], U.FLOOR_ROPE))
    else:                  # only the second batch differs
        assert not _ulp_caught(m[:1], r[:1], t[:1], U.row_floor(r[:1], U.FLOOR_ROPE))


def test_mutant_swiglu_halves_swapped():
    c = U.swiglu_inputs(5, 520)
    r, t, m = (U.swiglu_ref(F64, c["gu"], c["dh"]), U.swiglu_ref(F32, c["gu"], c["dh"]),
               U.swiglu_ref(F32, c["gu"], c["dh"], mutant="swap"))
    assert _ulp_caught(m["dgu"], r["dgu"], t["dgu"], U.row_floor(r["dgu"], U.FLOOR_SWIGLU))
    assert not _ulp_caught(m["h"], r["h"], t["h"], U.row_floor(r["h"], U.FLOOR_SWIGLU))


# ------------------------------------------------------------------------------- flash attention
def _attn_docs(layout, T, B):
    return None if layout is None else U.doc_arrays(U.attn_layout(layout, T, B), T)


def _attn_pair(c, layout=None, path="flash"):
    """(fp64 reference with its allowance, fp32 twin with the kernel's roundings) of one case"""
    B, T, H, Hkv, Dh, gen = c
    x = U.attn_inputs(gen, B, T, H, Hkv, Dh)
    docs = _attn_docs(layout, T, B)
    a = (x["qkv"], x["dout"], B, T, H, Hkv, Dh, docs)
    return U.attn_ref(F64, *a, path=path), U.attn_ref(F32, *a, twin=True, path=path)


@pytest.mark.parametrize("c", U.ATTN_CASES, ids=U.attn_case_id)
def test_twin_attention(c):
    """the derivation holds: with the kernel's bf16 roundings in place the fp32 twin stays inside
    the per-element allowance on every output, plain and under every document layout"""
    J = U.Judge()
    fams = dict.fromkeys(U.ATTN_OUTPUTS, "attn")
    for layout in (None,) + U.ATTN_LAYOUTS:
        r, t = _attn_pair(c, layout)
        U.judge_attn(J, fams, (U.attn_case_id(c), layout or "plain"), r, t, {}, U.ATTN_OUTPUTS)
        assert all(bool((r["allow_" + n] > 0).all()) for n in U.ATTN_OUTPUTS)
    J.check()


@pytest.mark.parametrize("c", U.ATTN_GEMM, ids=U.attn_case_id)
def test_twin_attention_composed(c):
    J = U.Judge()
    r, t = _attn_pair(c, path="gemm")
    U.judge_attn(J, dict.fromkeys(U.ATTN_OUTPUTS, "attn-gemm"), U.attn_case_id(c), r, t, {})
    J.check()


def test_attn_layouts_and_masks():
    """the two forms of the document mask (start per query row, end per key row) are one set; the
    layouts have the features their comment names"""
    for T in (64, 128, 192, 256, 384):
        for name in U.ATTN_LAYOUTS:
            lengths = U.attn_layout(name, T, 3)
            st, en = U.doc_arrays(lengths, T)
            kq, kkv, same = U.attn_masks(3, T, (st, en), "cpu")
            assert same and torch.equal(kq, kkv) and bool(kq.diagonal(dim1=1, dim2=2).all())
        a = U.attn_layout("A", T, 3)
        assert a[0][0] == 5 and a[0][2:4] == [1, 1] and a[1] == [T] and a[2] == a[0][::-1]
        assert all(n % 64 == 0 for row in U.attn_layout("aligned", T, 3) for n in row)
    from tests.test_attn_docmask_gpu import LAYOUT_A

    for T, rows in LAYOUT_A.items():
        assert U.attn_layout("A", T, 2) == rows


def test_attn_spikes_straddle_the_lazy_rescale():
    """a check on the data: in the last 64-row block every row's running maximum rises by clearly
    less than 8 (log2 domain) at key tile 1 - against the stale maximum of tile 0, as the kernel
    compares - and by clearly more than 8 at tile 2, at the smallest T with four key tiles"""
    cases = [c for c in U.ATTN_CASES if c[5] == "spikes"]
    assert cases and all(c[1] == 256 for c in cases)
    for B, T, H, Hkv, Dh, gen in cases:
        x = U.attn_inputs(gen, B, T, H, Hkv, Dh)
        r1, r2, r20 = U.attn_spike_rises(x["qkv"], B, T, H, Hkv, Dh)
        assert 1.0 < r1.min().item() and r1.max().item() < 7.0, (r1.min().item(), r1.max().item())
        assert r2.min().item() > 9.0 and r20.min().item() > 9.0


def test_attn_offset_heads():
    """a check on the data: q-head 0's scores lie near +60, the last head's near -40 (log2 domain)"""
    for B, T, H, Hkv, Dh, gen in [c for c in U.ATTN_CASES if c[5] == "offset"]:
        x = U.attn_inputs(gen, B, T, H, Hkv, Dh)
        r = U.attn_ref(F64, x["qkv"], x["dout"], B, T, H, Hkv, Dh)
        lse = r["lse"].view(B, H, T)
        assert (lse[:, 0] - 60).abs().max().item() < 12 and (lse[:, H - 1] + 40).abs().max().item() < 12


def test_attn_grids_meet_every_xcd_branch():
    """every kernel of attn_flash.hip is launched with one and with two row groups per wave (the
    names ending in 2: fwd_kernel and bwd_dq_kernel with G = 2, bwd_dkdv2_kernel), over the case table x variants x head splits, on
    grids that take each branch of xcd_grid: gridDim.y % 8 == 0; n % 8 == 0 with gridDim.y % 8 != 0;
    n % 8 != 0, once with n < 8.  The table also holds every value the issue lists."""
    seen = {}
    for B, T, H, Hkv, Dh, _ in U.ATTN_CASES:
        for v in U.ATTN_VARIANTS:
            for qs in U.attn_head_splits(H, Hkv):
                for fam, gx, gy in U.attn_launches(B, T, H, Hkv, Dh, v, qs):
                    seen.setdefault(fam, set()).add(U.xcd_branch(gx, gy))
    assert set(seen) == {"fwd", "fwd2", "dq", "dq2", "dkdv", "dkdv2"}
    for fam, br in seen.items():
        assert {"rows", "even"} <= br and br & {"ragged", "ragged<8"}, (fam, br)
    for fams in (("fwd", "fwd2"), ("dq", "dq2"), ("dkdv", "dkdv2")):
        assert any("ragged<8" in seen[f] for f in fams), fams
    col = lambda i: {c[i] for c in U.ATTN_CASES}
    assert col(0) == {1, 2, 3} and col(1) == {64, 128, 192, 256, 384} and col(4) == {64, 128}
    assert {(c[2], c[3]) for c in U.ATTN_CASES} == {(1, 1), (4, 4), (4, 2), (8, 2), (8, 1)}
    assert col(5) == set(U.ATTN_GENS)
    assert {qs for c in U.ATTN_CASES for qs in U.attn_head_splits(c[2], c[3])} == {1, 2, 4}
    assert {k for v in U.ATTN_VARIANTS for k in v} == {1, 2} and (1, 1, 1) in U.ATTN_VARIANTS and (2, 2, 2) in U.ATTN_VARIANTS
    assert U.xcd_branch(2, 8) == "rows" and U.xcd_branch(4, 2) == "even" and U.xcd_branch(3, 4) == "ragged"


# mutant -> the outputs on which it must leave the allowance
ATTN_MUTANT_OUTPUTS = {
    "diag_upper": ("out", "dv"), "diag_wave_last": ("dk", "dv"), "drop_key": ("out", "dv"),
    "scores_x102": ("lse", "dv"), "bwd_p_x102": ("dv",), "l_low": ("lse", "dv"),
    "dout_dropped": ("delta", "dq", "dk", "dv"), "group_first_only": ("dk", "dv"), "doc_start_low": ("out", "dq"),
    "doc_end_low": ("dk", "dv"),
}
ATTN_MUTANT_CASES = [(2, 256, 4, 2, 64, "randn"), max(U.ATTN_CASES, key=lambda c: (c[1], c[0] * c[2]))]
_attn_refs: dict = {}


def _attn_mutant_scores(c, mutant):
    layout = "A" if mutant.startswith("doc_") else None
    B, T, H, Hkv, Dh, gen = c
    x = U.attn_inputs(gen, B, T, H, Hkv, Dh)
    a = (x["qkv"], x["dout"], B, T, H, Hkv, Dh, _attn_docs(layout, T, B))
    if (c, layout) not in _attn_refs:
        _attn_refs[(c, layout)] = U.attn_ref(F64, *a)
    r = _attn_refs[(c, layout)]
    t = U.attn_ref(F32, *a, twin=True, mutant=mutant)
    return r, t, {n: U.allow_err(t[n], r[n], r["allow_" + n]) for n in U.ATTN_OUTPUTS}


@pytest.mark.parametrize("c", ATTN_MUTANT_CASES, ids=U.attn_case_id)
@pytest.mark.parametrize("mutant", U.ATTN_MUTANTS)
def test_mutant_attention(mutant, c):
    """each deliberate error, computed like a kernel would (fp32, bf16 roundings), leaves the
    allowance on every output named for it, at T = 256 and at the largest T of the table"""
    assert c[1] in (256, max(k[1] for k in U.ATTN_CASES))
    _, _, s = _attn_mutant_scores(c, mutant)
    print(mutant, {n: round(v, 3) for n, v in s.items()})
    for n in ATTN_MUTANT_OUTPUTS[mutant]:
        assert s[n] > 1.0, (mutant, n, s)


def test_old_yardstick_accepts_attention_mutants():
    """the gap this yardstick closes, kept on record: max |err| <= 2e-2 (out) / 3e-2 (gradients) x
    max |ref| over the whole tensor accepts scores x 1.02, the backward's P x 1.02 and a row sum
    2^-6 low on all four outputs at T = 256, while each leaves the per-element allowance"""
    c = ATTN_MUTANT_CASES[0]
    for mutant in ("scores_x102", "bwd_p_x102", "l_low"):
        r, t, s = _attn_mutant_scores(c, mutant)
        for n, rel in (("out", 2e-2), ("dq", 3e-2), ("dk", 3e-2), ("dv", 3e-2)):
            assert U.old_yardstick(t[n], r[n], rel), (mutant, n)
        assert max(s.values()) > 1.0


# ------------------------------------------------------------------------------- GEMM
def test_twin_gemm():
    """every case of the GEMM table (U.gemm_cpu_cases: tile shapes x K, split-K, epilogues, batched,
    fp32 operands; the persistent, automatic-route and grouped cases cut down to one 256x256 tile
    with their K, epilogue and generator): the fp32 twin under its ceilings on C, the saved
    pre-activation / gelu', and both column-sum arms.  This is what fixes FLOOR_GEMM."""
    J = U.Judge()
    for row in U.gemm_cpu_cases():
        c = U.gemm_cpu_case(*row)
        r, t = U.gemm_ref_of(F64, c), U.gemm_ref_of(F32, c)
        for cs_rows in ((8, None) if c["colsum"] else (None,)):
            U.judge_gemm(J, "gemm-" + row[0], row[1:], c, r, t, {}, cs_rows=cs_rows, aux_fp32=row[0] == "f32")
    J.check()


def test_floor_gemm_is_the_smallest_power_of_two():
    """at half of FLOOR_GEMM the twin leaves its ceiling on the forced-configuration shapes"""
    worst = 0.0
    for row in U.gemm_cpu_cases():
        if row[0] == "tile" and not row[6]:
            c = U.gemm_cpu_case(*row)
            r, t = U.gemm_ref_of(F64, c), U.gemm_ref_of(F32, c)
            assert U.ulp_err(t["C"], r["C"], U.FLOOR_GEMM * r["S"]) <= U.TWIN_ULP_CEIL
            worst = max(worst, U.ulp_err(t["C"], r["C"], U.FLOOR_GEMM / 2 * r["S"]))
    assert worst > U.TWIN_ULP_CEIL, worst


# mutant -> (epilogue that shows it, the output it corrupts)
GEMM_MUTANT_WHERE = {
    "truncate": ("plain", "C"), "drop_k_last": ("plain", "C"), "cols_scaled": ("plain", "C"),
    "bias_shift": ("bias_bf16", "C"), "slab_bf16": ("plain", "C"), "res_after_act": ("gelu_bwd_res", "C"),
    "gelu_of_rounded": ("gelu", "C"), "colsum_rounded": ("gelu_bwd", "colsum"),
}
GEMM_MUTANT_SHAPES = [U.GEMM_EPI_SHAPE, (264, 264, 2048)]   # the second: the split-K shape
_gemm_refs: dict = {}


def _gemm_mutant(mutant, shape, out_fp32):
    """(reference, twin, mutant, case) on one shape"""
    epi = GEMM_MUTANT_WHERE[mutant][0]
    key = (shape, epi, out_fp32)
    if key not in _gemm_refs:
        c = U.gemm_case("randn", *shape, epi, out_fp32)
        _gemm_refs[key] = (c, U.gemm_ref_of(F64, c), U.gemm_ref_of(F32, c))
    c, r, t = _gemm_refs[key]
    return r, t, U.gemm_ref_of(F32, c, mutant=mutant), c


@pytest.mark.parametrize("shape", GEMM_MUTANT_SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("mutant", U.GEMM_MUTANTS)
def test_mutant_gemm(mutant, shape):
    """each deliberate error leaves the allowance on the output it corrupts: bf16 C / aux by
    Judge.ulp's rule (k = 1, FLOOR_GEMM x S), fp32 C by Judge.rel's (R = K), the fused column sums
    with R = 8"""
    name = GEMM_MUTANT_WHERE[mutant][1]
    r, t, m, c = _gemm_mutant(mutant, shape, False)
    if name == "colsum":
        assert _rel_caught(m["colsum"], r["colsum"], t["colsum"], r["colsum_scale"], 8)
        # ... and only there: the mutant's C is the twin's
        assert not _ulp_caught(m["C"], r["C"], t["C"], U.FLOOR_GEMM * r["S"])
        return
    assert _ulp_caught(m["C"], r["C"], t["C"], U.FLOOR_GEMM * r["S"]), mutant
    if mutant not in ("truncate", "gelu_of_rounded"):   # (these two are errors of the bf16 store itself)
        r, t, m, c = _gemm_mutant(mutant, shape, True)
        assert _rel_caught(m["C"], r["C"], t["C"], r["S_rel"].clamp_min(U.TINY), c["K"]), mutant


# the mutants the whole-tensor criterion lets through on a bf16 C at rel = 1e-2, on both shapes
# (bias_shift passes it at K = 2048 only, where |C| ~ 45 dwarfs a bias; drop_k_last and
# res_after_act are caught by it on these shapes too)
GEMM_OLD_ACCEPTS = ("truncate", "cols_scaled", "slab_bf16", "gelu_of_rounded")


def test_old_yardstick_accepts_gemm_mutants():
    """the gap this section closes, kept on record: `_close` of tests/test_kernels_gpu.py (largest
    error <= rel x largest magnitude; 1e-2 for bf16 outputs, 1e-5 for fp32 ones) accepts these
    mutants on a bf16 output at (520, 392, 192) and (264, 264, 2048) (none of them on an fp32 one);
    each leaves the per-element allowance (test_mutant_gemm)"""
    accepted = {}
    for shape in GEMM_MUTANT_SHAPES:
        for mutant in U.GEMM_MUTANTS:
            if GEMM_MUTANT_WHERE[mutant][1] != "C":
                continue
            r, t, m, _ = _gemm_mutant(mutant, shape, False)
            ok16 = U.old_yardstick(m["C"].to(U.BF16), r["C"], 1e-2)
            r, t, m, _ = _gemm_mutant(mutant, shape, True)
            ok32 = U.old_yardstick(m["C"], r["C"], 1e-5)
            accepted[(mutant, shape)] = (ok16, ok32)
            print(mutant, shape, "old criterion accepts: bf16", ok16, "fp32", ok32)
    for mutant in ("truncate", "cols_scaled", "slab_bf16"):
        assert all(accepted[(mutant, s)][0] for s in GEMM_MUTANT_SHAPES), mutant
    both = tuple(m for m in U.GEMM_MUTANTS if GEMM_MUTANT_WHERE[m][1] == "C"
                 and all(accepted[(m, s)][0] for s in GEMM_MUTANT_SHAPES))
    assert set(both) == set(GEMM_OLD_ACCEPTS), both
