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
  (264, 264, 2048); the whole-tensor yardstick accepts four of them on a bf16 output;
* CNN (the last section): the twins of `conv_ref`, `bn_ref` and the pool references stay under
  their ceilings on every case and generator of the CNN tables (the column-path dgrad inside its
  counted allowance), which fixes FLOOR_BN_Y and FLOOR_BN_DX; the tap-loop references equal torch's
  convolution and pooling in float64 and the layout formulas are consistent with one another;
  seven convolution, six BatchNorm and three pooling errors each leave the allowance; the
  whole-tensor yardstick of tests/test_cnn_gpu.py accepts four of them (six at its own sizes);
  mirrors of the launchers' grid arithmetic show that the table meets every branch the GPU tests name;
* optimizers, embedding, dropout (the last section): the twins of `adamw_ref` and `sgd_ref` stay under their
  ceiling over three and seven steps, on the generator's inputs and on the chunk tables the GPU tests launch
  over, with every intermediate a normal number or zero; in float64 both references equal torch.optim.AdamW /
  SGD to 1e-12; `_torch_update` of FusedAdamW and FusedSGD (the CPU paths) is judged like a kernel; five
  AdamW and four SGD errors each leave the allowance; the whole-tensor yardstick of
  tests/test_kernels_gpu.py accepts two of them at lr = 1e-3 and six, `eps_inside` among them, at 2^-15;
* reductions (the last section): on every `offset` case of the REDUCE_* tables the fp32 twin of the column-sum and
  loss-finalize references, and the fp64 twin of the grad-norm sums against math.fsum, stay under their ceilings;
  eight deliberate errors (U.REDUCE_MUTANTS) are each caught at every case where the mutated path is live - on
  `ints` by a single differing bit, on `offset` by the allowance.
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


# ------------------------------------------------------------------------------- CNN (ResNet path)
_cnn_refs: dict = {}


def _conv_case(case, gen="randn"):
    """(inputs, reference, twin) of one row of a CNN_CONV_* table, computed once"""
    key = (case, gen)
    if key not in _cnn_refs:
        _, B, H, W, C, Co, k, s, p = case
        c = U.conv_inputs(gen, B, H, W, C, Co, k, k, s, p, addend=True)
        a = (c["x"], c["w"], s, p, c["dy"], c["addend"])
        _cnn_refs[key] = (c, a, U.conv_ref(F64, *a), U.conv_ref(F32, *a))
    return _cnn_refs[key]


def _wgrad3_as_conv(row, B=3):
    name, H, W, C, Co = row
    return (name, B, H, W, C, Co, 3, 1, 1)


def _bn_case(gen, N, C, res, relu):
    key = ("bn", gen, N, C, res, relu)
    if key not in _cnn_refs:
        c = U.bn_inputs(gen, N, C, res=res)
        a = (c["x"], c["gamma"], c["beta"], 1e-5, 0.1, c["rm"], c["rv"], c["res"], relu)
        r = U.bn_ref(F64, *a, dy=c["dy"])
        t = U.bn_ref(F32, *a, mask=(r["y"] > 0) if relu else None, dy=c["dy"])   # the mask is an input
        _cnn_refs[key] = (c, a, r, t)
    return _cnn_refs[key]


CNN_BN_WAYS = ((False, False), (False, True), (True, True), (True, False))   # (residual, relu)
CNN_BN_FWD = ("y", "running_mean", "running_var")
CNN_BN_BWD = ("dx", "dgamma", "dbeta")


def test_twin_cnn_conv():
    """every convolution case x generator: the twin under its ceilings on y, dx (implicit GEMM, with
    the addend) and dw; the strided cases also through linear_dgrad + col2im, where the twin applies
    the kernels' bf16 roundings and has to stay inside the counted allowance"""
    J = U.Judge()
    cases = U.CNN_CONV_IMPLICIT + U.CNN_CONV_STATS + [_wgrad3_as_conv(r) for r in U.CNN_WGRAD3 + U.CNN_WGRAD3_KP128]
    for gen in U.CNN_GENS:
        for case in cases + [U.CNN_WGRAD_SPLITK]:
            c, a, r, t = _conv_case(case, gen)
            U.judge_conv(J, "conv", (case[0], gen), r, t, {}, pixels=r["y"].numel() // r["y"].shape[-1])
            if case[7] > 1:
                rc = U.conv_ref(F64, *a, path="cols")
                tc = U.conv_ref(F32, *a, path="cols", twin=True)
                J.within("col2im", (case[0], gen), "dx", None, rc["dx"], tc["dx"], rc["allow_dx"])
    J.check()


def test_twin_cnn_batchnorm_and_fused_statistics():
    J = U.Judge()
    for gen in U.CNN_GENS + ("planted",):
        for N, C in U.CNN_BN + [U.CNN_BN_BIG, U.CNN_BN_MANY]:
            for res, relu in CNN_BN_WAYS:
                c, a, r, t = _bn_case(gen, N, C, res, relu)
                U.judge_bn(J, "bn", (gen, N, C, res, relu), r, t, {}, U.bn_serial_rows(N, C, 1), CNN_BN_FWD, CNN_BN_BWD)
                assert torch.equal(t["dres"].to(U.BF16), r["dres"].to(U.BF16))   # a masked copy: exact
    # eval mode: the running statistics as given
    c, a, r, t = _bn_case("offset", 231, 64, False, True)
    ev = lambda dt: U.bn_ref(dt, *a, training=False)
    J.ulp("bn-eval", (231, 64), "y", None, ev(F64)["y"], ev(F32)["y"], U.FLOOR_BN_Y * ev(F64)["S_y"])
    # the per-tile partials of the epilogue, from the twin's stored y
    for gen in U.CNN_GENS:
        for case in U.CNN_CONV_STATS:
            _, _, r, t = _conv_case(case, gen)
            if gen == "offset":   # the output channels carry the offset: mean about 8 x the deviation
                v = r["y"].reshape(-1, case[5])
                ratio = (v.mean(0) / v.std(0)).abs().median().item()
                print("offset", case[0], "output mean / std", ratio)
                assert 7 <= ratio <= 9, ratio
            y = t["y"].to(U.BF16).reshape(-1, case[5])
            bm = 256 if case[5] <= 64 else 128
            sr, st = U.tile_stats_ref(F64, y, bm), U.tile_stats_ref(F32, y, bm)
            for n in ("mean", "m2"):
                J.rel("tilestats", (case[0], gen), n, None, sr[n], st[n], sr[n + "_scale"], U.CNN_STATS_ROWS)
    J.check()


def test_twin_cnn_pools():
    J = U.Judge()
    for B, H, W, C, k, s, p in U.CNN_POOLS:
        for gen in ("randn", "planted"):
            c = U.pool_inputs(gen, B, H, W, C, k, s, p)
            f = U.maxpool_ref(c["x"], k, s, p)
            r, t = (U.maxpool_bwd_ref(dt, c["dy"], f["arg"], H, W, k, s, p) for dt in (F64, F32))
            J.ulp("maxpool", (B, H, W, C, k, s, p, gen), "dx", None, r["dx"], t["dx"], 0.0)
    B, H, W, C = U.CNN_AVGPOOL
    g = torch.Generator().manual_seed(5)
    x, dy = torch.randn(B, H, W, C, generator=g).to(U.BF16), torch.randn(B, C, generator=g).to(U.BF16)
    r, t = U.avgpool_ref(F64, x, dy), U.avgpool_ref(F32, x, dy)
    J.ulp("avgpool", U.CNN_AVGPOOL, "y", None, r["y"], t["y"], 0.0)
    J.ulp("avgpool", U.CNN_AVGPOOL, "dx", None, r["dx"], t["dx"], 0.0)
    J.check()


def test_cnn_references_against_torch_and_each_other():
    """the tap-loop references equal torch's own convolution / pooling in float64, and the layout
    formulas are consistent: the 4x4 / 1 / 2 convolution of the space-to-depth image with the
    rearranged weight IS the 7x7 / 2 / 3 stem, and its weight gradient gathers back"""
    import torch.nn.functional as Fn

    for case in U.CNN_CONV_IMPLICIT:
        c, a, r, _ = _conv_case(case)
        _, B, H, W, C, Co, k, s, p = case
        xr = c["x"].double().permute(0, 3, 1, 2).requires_grad_(True)
        wr = c["w"].to(U.BF16).double().requires_grad_(True)
        y = Fn.conv2d(xr, wr, stride=s, padding=p)
        y.backward(c["dy"].double().permute(0, 3, 1, 2))
        for got, ref in ((r["y"], y.permute(0, 2, 3, 1)), (r["dw"], wr.grad),
                         (r["dx"] - c["addend"].double(), xr.grad.permute(0, 2, 3, 1))):
            assert (got - ref).abs().max().item() <= 1e-12 * (1 + ref.abs().max().item()), case[0]
        cols = U.im2col_ref(c["x"], k, k, s, p, k * k * C + 8, B * r["y"].shape[1] * r["y"].shape[2] + 3)
        unf = Fn.unfold(c["x"].float().permute(0, 3, 1, 2), k, padding=p, stride=s)   # [B, C k k, L], (c, kh, kw)
        unf = unf.view(B, C, k * k, -1).permute(0, 3, 2, 1).reshape(-1, k * k * C)
        assert torch.equal(cols[:unf.shape[0], :k * k * C].float(), unf) and not cols[unf.shape[0]:].any()
        assert not cols[:, k * k * C:].any()
        if s == 1:   # the stride-1 dgrad is the convolution of dy with the flipped, transposed kernel
            wm = c["w"].to(U.BF16).permute(0, 2, 3, 1).reshape(Co, -1)
            wt = U.w_flip_t_ref(wm, Co, k, k, C).view(C, k, k, Co).permute(0, 3, 1, 2)
            d = U.conv_ref(F64, c["dy"], wt, 1, k - 1 - p)["y"]
            assert (d + c["addend"].double() - r["dx"]).abs().max().item() <= 1e-12 * r["dx"].abs().max().item()
    for B, H, W in U.CNN_STEM_S2D:
        g = torch.Generator().manual_seed(H)
        x, w = torch.randn(B, 3, H, W, generator=g), torch.randn(64, 3, 7, 7, generator=g) * 0.1
        wm = w.to(U.BF16).permute(0, 2, 3, 1).reshape(64, 147)
        dy = torch.randn(B, H // 2, W // 2, 64, generator=g).to(U.BF16)
        full = U.conv_ref(F64, U.nhwc_bf16_ref(x), w, 2, 3, dy)
        wp = U.stem_w_s2d_ref(wm).view(64, 4, 4, 16).permute(0, 3, 1, 2)
        # (pad 2 yields one more output row and column than the stem has: the kernel is handed
        # Ho = H / 2, Wo = W / 2 and never computes them)
        dyp = torch.zeros(B, H // 2 + 1, W // 2 + 1, 64, dtype=U.BF16)
        dyp[:, :-1, :-1] = dy
        s2d = U.conv_ref(F64, U.s2d_ref(x), wp, 1, 2, dyp)
        assert (s2d["y"][:, :-1, :-1] - full["y"]).abs().max().item() <= 1e-12
        dwp = s2d["dw"].permute(0, 2, 3, 1).reshape(64, 256)
        assert (U.stem_dw_ref(dwp) - full["dw"].permute(0, 2, 3, 1).reshape(64, 147)).abs().max().item() <= 1e-12
    for B, H, W, C, k, s, p in U.CNN_POOLS:
        c = U.pool_inputs("planted", B, H, W, C, k, s, p)
        f = U.maxpool_ref(c["x"], k, s, p)
        xr = c["x"].double().permute(0, 3, 1, 2).requires_grad_(True)
        y = Fn.max_pool2d(xr, k, s, p)
        assert torch.equal(f["y"].double(), y.permute(0, 2, 3, 1))


def test_floor_bn_is_the_smallest_power_of_two():
    """at half of FLOOR_BN_Y the twin leaves its ceiling on the BatchNorm table; at the floor it holds.
    FLOOR_BN_DX is the smallest power of two at which the twin holds on the CPU and on the device:
    here it holds at the floor and has left the ceiling at a quarter of it; that the device's twin
    is over the ceiling at half of it is held by tests/test_cnn_ulp_gpu.py."""
    for name, S, floor, steps in (("y", "S_y", U.FLOOR_BN_Y, 2), ("dx", "S_dx", U.FLOOR_BN_DX, 4)):
        at, below = 0.0, 0.0
        for gen in U.CNN_GENS + ("planted",):
            for N, C in U.CNN_BN + [U.CNN_BN_BIG, U.CNN_BN_MANY]:
                for res, relu in CNN_BN_WAYS:
                    _, _, r, t = _bn_case(gen, N, C, res, relu)
                    at = max(at, U.ulp_err(t[name], r[name], floor * r[S]))
                    below = max(below, U.ulp_err(t[name], r[name], floor / steps * r[S]))
        print(name, "twin at the floor", at, "at 1 /", steps, "of it", below)
        assert at <= U.TWIN_ULP_CEIL < below, (name, at, below)


# mutant -> (the case that shows it, the output it corrupts)
CNN_CONV_MUTANT_WHERE = {"pad_clamp": ("c64", "y"), "khkw_swapped": ("k5", "y"), "hw_swapped": ("c64", "y"),
                         "col2im_phase": ("s2", "dx_cols"), "dw_last_row": ("c64", "dw"), "truncate": ("c64", "y"),
                         "addend_after": ("c64", "dx")}
_CONV_BY_NAME = {c[0]: c for c in U.CNN_CONV_IMPLICIT}


def _conv_mutant_caught(mutant, case, name):
    c, a, r, t = _conv_case(case)
    if name == "dx_cols":
        rc = U.conv_ref(F64, *a, path="cols")
        m = U.conv_ref(F32, *a, path="cols", twin=True, mutant=mutant)
        return U.allow_err(m["dx"].to(U.BF16), rc["dx"], rc["allow_dx"]) > 1.0, m["dx"], rc["dx"]
    m = U.conv_ref(F32, *a, mutant=mutant)
    if name == "dw":
        return _rel_caught(m["dw"], r["dw"], t["dw"], r["S_dw"], r["y"].numel() // r["y"].shape[-1]), m["dw"], r["dw"]
    return _ulp_caught(m[name], r[name], t[name], U.FLOOR_GEMM * r["S_" + name]), m[name], r[name]


@pytest.mark.parametrize("mutant", U.CONV_MUTANTS)
def test_mutant_conv(mutant):
    case, name = CNN_CONV_MUTANT_WHERE[mutant]
    assert _conv_mutant_caught(mutant, _CONV_BY_NAME[case], name)[0], mutant


CNN_BN_MUTANT_WHERE = {"biased_var": "running_var", "eps": "y", "mask_ge": "dx", "mask_pre_res": "dx",
                       "dbeta_dropped": "dx", "dres_unmasked": "dres"}


def _bn_mutant(mutant, gen="randn", N=231, C=64):
    c, a, r, t = _bn_case(gen, N, C, True, True)
    return r, t, U.bn_ref(F32, *a, dy=c["dy"], mutant=mutant)


@pytest.mark.parametrize("mutant", U.BN_MUTANTS)
def test_mutant_batchnorm(mutant):
    name = CNN_BN_MUTANT_WHERE[mutant]
    r, t, m = _bn_mutant(mutant)
    if name == "dres":
        assert not torch.equal(m["dres"].to(U.BF16), r["dres"].to(U.BF16))
    elif name == "running_var":
        assert _rel_caught(m[name], r[name], t[name], r[name + "_scale"], U.bn_serial_rows(231, 64, 1))
    else:
        S, fl = ("S_y", U.FLOOR_BN_Y) if name == "y" else ("S_dx", U.FLOOR_BN_DX)
        assert _ulp_caught(m[name], r[name], t[name], fl * r[S]), mutant
    if mutant in ("mask_ge", "mask_pre_res"):   # a wrong mask also moves the channel sums
        for n in ("dbeta", "dgamma"):
            assert _rel_caught(m[n], r[n], t[n], r[n + "_scale"], U.bn_serial_rows(231, 64, 1)), (mutant, n)


def _pool_mutant(mutant, case):
    B, H, W, C, k, s, p = case
    c = U.pool_inputs("planted", B, H, W, C, k, s, p)
    f, m = U.maxpool_ref(c["x"], k, s, p), U.maxpool_ref(c["x"], k, s, p, mutant=mutant)
    r, t = (U.maxpool_bwd_ref(dt, c["dy"], f["arg"], H, W, k, s, p) for dt in (F64, F32))
    return f, m, r, t, U.maxpool_bwd_ref(F32, c["dy"], f["arg"], H, W, k, s, p, mutant=mutant)


@pytest.mark.parametrize("mutant", U.POOL_MUTANTS)
def test_mutant_pool(mutant):
    """on the planted windows: the last maximum is another tap, padding read as zero wins the
    all-negative border windows, a dropped window at the (odd) border leaves its gradient out"""
    for case in (U.CNN_POOLS[0], U.CNN_POOLS[1]):
        f, m, r, t, mb = _pool_mutant(mutant, case)
        if mutant == "last_argmax":
            assert not torch.equal(f["arg"], m["arg"])
        elif mutant == "pad_zero":
            assert not torch.equal(f["y"].view(torch.int16), m["y"].view(torch.int16))
        else:
            assert _ulp_caught(mb["dx"], r["dx"], t["dx"], 0.0)


# what `_close` of tests/test_cnn_gpu.py lets through at its tolerances (0.02 y and dw, 0.03 dx, 0.01
# the BatchNorm sums, 1e-4 the running statistics).  No border mutant passes it on the small shapes
# of the table (a wrong border pixel is an O(1) error next to the largest magnitude); the two
# below the line do at the sizes that test itself uses - a 56-row image batch.
CNN_OLD_ACCEPTS = {("conv", "truncate"), ("conv", "addend_after"), ("bn", "eps"), ("bn", "dbeta_dropped")}
CNN_OLD_ACCEPTS_LARGE = {("conv", "dw_last_row"), ("bn", "biased_var")}


def test_old_yardstick_accepts_cnn_mutants():
    """the gap this section closes, kept on record; each of these leaves the per-element allowance
    (test_mutant_conv, test_mutant_batchnorm)"""
    tol = {"y": 0.02, "dx": 0.03, "dx_cols": 0.03, "dw": 0.02, "running_var": 1e-4, "dres": 0.01}
    accepted = set()
    for mutant in U.CONV_MUTANTS:
        case, name = CNN_CONV_MUTANT_WHERE[mutant]
        caught, m, r = _conv_mutant_caught(mutant, _CONV_BY_NAME[case], name)
        ok = U.old_yardstick(m if name == "dw" else m.to(U.BF16), r, tol[name])
        print("conv", mutant, "old criterion accepts:", ok)
        if ok:
            accepted.add(("conv", mutant))
    for mutant in U.BN_MUTANTS:
        name = CNN_BN_MUTANT_WHERE[mutant]
        r, t, m = _bn_mutant(mutant)
        ok = U.old_yardstick(m[name] if name == "running_var" else m[name].to(U.BF16), r[name].double(), tol[name])
        print("bn", mutant, "old criterion accepts:", ok)
        if ok:
            accepted.add(("bn", mutant))
    for mutant in U.POOL_MUTANTS:
        f, m, r, t, mb = _pool_mutant(mutant, U.CNN_POOLS[0])
        ok = U.old_yardstick(m["y"], f["y"].double(), 1e-6) and U.old_yardstick(mb["dx"].to(U.BF16), r["dx"], 0.01)
        print("pool", mutant, "old criterion accepts:", ok)
        if ok and mutant != "last_argmax":   # (the old test never looked at the argmax)
            accepted.add(("pool", mutant))
    assert accepted == CNN_OLD_ACCEPTS, accepted
    # at the old test's own sizes: one dropped pixel row of 12544, the biased variance of 25088 rows
    large = set()
    big = ("big", 4, 56, 56, 64, 64, 3, 1, 1)
    caught, m, r = _conv_mutant_caught("dw_last_row", big, "dw")
    assert caught
    if U.old_yardstick(m, r, 0.02):
        large.add(("conv", "dw_last_row"))
    _cnn_refs.pop((big, "randn"))
    r, t, m = _bn_mutant("biased_var", N=8 * 56 * 56, C=64)
    R = U.bn_serial_rows(8 * 56 * 56, 64, U.bn_blocks(8 * 56 * 56, 64))
    assert _rel_caught(m["running_var"], r["running_var"], t["running_var"], r["running_var_scale"], R)
    if U.old_yardstick(m["running_var"], r["running_var"], 1e-4):
        large.add(("bn", "biased_var"))
    _cnn_refs.pop(("bn", "randn", 8 * 56 * 56, 64, True, True))
    assert large == CNN_OLD_ACCEPTS_LARGE, large


def test_cnn_grids_meet_every_branch():
    """the case table reaches every branch the GPU tests name: mirrors of _bn_blocks, the split merge
    of rtdc_bn_fwd and launch_conv3x3_wgrad"""
    # BatchNorm at _BN_LOADS = 1 (the GPU tests patch it) and at the default
    seen = set()
    for N, C in U.CNN_BN + [U.CNN_BN_BIG, U.CNN_BN_MANY]:
        seen |= U.bn_reduce_branches(N, C, U.bn_blocks(N, C, 1)) | U.bn_reduce_branches(N, C, U.bn_blocks(N, C))
    assert seen >= {"apply_hoisted", "apply_generic", "idle_lanes", "second_gbase", "empty_block", "unrolled",
                    "remainder", "finalize_wraps"}, seen
    assert U.bn_blocks(*U.CNN_BN_MANY, 1) > 256 and U.bn_blocks(*U.CNN_BN_BIG) >= 2
    assert {256 % (C // 8) == 0 for _, C in U.CNN_BN} == {True, False}
    assert all(N % (4 * (256 // min(256, C // 8))) for N, C in U.CNN_BN)
    # the split merge: 26 tiles of 128 rows -> S = 4 splits of 7, the last one of 5; not without the knob
    N, C = U.CNN_BN_BIG
    tiles = -(-N // 128)
    assert tiles == 26 and U.bn_split(tiles, C, U.bn_blocks(N, C, 1)) == (4, 7) and tiles % 7
    assert U.bn_split(tiles, C, U.bn_blocks(N, C)) == (4, 7) and U.bn_split(tiles, C, 216, enabled=False) is None
    assert U.bn_split(2, 64, 1) is None          # the 256-row tiles of st64: the finalize alone
    st = U.CNN_CONV_STATS[1]
    assert st[1] * U.out_hw(st[2], st[3], 3, 3, 1, 1)[0] * U.out_hw(st[2], st[3], 3, 3, 1, 1)[1] == N and st[5] == C
    # conv3x3_wgrad_kernel, B = 3
    plans = {r[0]: U.conv3_wgrad_plan(3, *r[1:]) for r in U.CNN_WGRAD3}
    assert plans["img"] == (64, 5, 1, 3, 1)                      # RC = H: the whole image, 35 of 64 pixels
    assert plans["rows3"][:3] == (64, 3, 6) and 17 % 3           # the last chunk of an image partial
    assert plans["w33"][:3] == (64, 1, 4) and plans["w64"][:3] == (64, 1, 3)
    KP, RC, cpi, S, per = plans["uneven"]
    assert per == 2 and 3 * cpi % per == 1 and S == 35           # chunks split unevenly over the blocks
    for r in U.CNN_WGRAD3_KP128:
        assert U.conv3_wgrad_plan(3, *r[1:], kp_env=128)[0] == 128 and U.conv3_wgrad_plan(3, *r[1:])[0] == 64
    assert U.conv3_wgrad_plan(3, 17, 19, 64, 64, kp_env=128)[0] == 128    # 6 rows of 19 = 114 >= 96
    assert U.conv3_wgrad_plan(3, 5, 7, 64, 64, kp_env=128)[0] == 64       # 35 pixels: the 3/4 rule refuses
    # mode 2 of the implicit GEMM: more than four tiles, a window that is not 3x3, a strided 3x3
    by = _CONV_BY_NAME
    assert U.conv3_wgrad_plan(by["c192"][1], *by["c192"][2:6]) is None
    assert by["k5"][6] == 5 and by["s2"][7] == 2
    # pick_splitk: 37 k-tiles of 64 (padded) pixels under 7 tiles of 64x256 - its time model takes 4 slabs;
    # no other mode-2 case of the table is long enough to split
    _, B, H, W, C, Co, k, s, p = U.CNN_WGRAD_SPLITK
    assert U.pick_splitk(Co, k * k * C, -(-B * H * W // 64) * 64, -(-k * k * C // 256), 64 << 20) == 4
    for _, B, H, W, C, Co, k, s, p in U.CNN_CONV_IMPLICIT:
        Ho, Wo = U.out_hw(H, W, k, k, s, p)
        assert U.pick_splitk(Co, k * k * C, -(-B * Ho * Wo // 64) * 64, 1, 64 << 20) == 1
    # every shape has H != W
    for c in U.CNN_CONV_IMPLICIT + U.CNN_CONV_STATS + [U.CNN_WGRAD_SPLITK]:
        assert c[2] != c[3]
    assert all(r[1] != r[2] for r in U.CNN_WGRAD3 + U.CNN_WGRAD3_KP128)
    assert all(c[1] != c[2] for c in U.CNN_POOLS) and all(H != W for _, H, W in U.CNN_STEM_S2D)


# ------------------------------------------------------------------------------- optimizers, embedding, dropout
ADAMW_HYPER = dict(b1=0.9, b2=0.999, eps=1e-8, wd=0.1)
ADAMW_WAYS = [(None, 1.0), (0.37, 1.0), (None, 0.125), (0.37, 0.125)]     # (clip coefficient, grad_scale)
OPTIM_N = 20000


def _mixed_mask(n):
    return (torch.arange(n) // 61) % 2 == 0


def _adamw_pair(c, mask, step, coef, gs, lr=U.OPTIM_LR, mutant="", f32_scalars=True, **h):
    h = {**ADAMW_HYPER, **h}
    a = (c["p"], c["g"], c["m"], c["v"], mask, lr, h["b1"], h["b2"], h["eps"], h["wd"], step, gs, coef)
    if mutant:
        return U.adamw_ref(F64, *a, mutant=mutant)
    return U.adamw_ref(F64, *a, f32_scalars=f32_scalars), U.adamw_ref(F32, *a, f32_scalars=f32_scalars)


def test_twin_adamw():
    """steps 1 .. 7 (judged at 1, 2 and 7), the state of each step the fp32 twin's previous output - the
    stand-in for the kernel's; every intermediate of the twin is a normal number or zero"""
    J = U.Judge()
    mask = _mixed_mask(OPTIM_N)
    for (coef, gs), h in [(w, {}) for w in ADAMW_WAYS] + [((None, 1.0), dict(b1=0.5, b2=0.75, eps=1e-3))]:
        state = None
        for step in range(1, 8):
            c = U.optim_inputs(OPTIM_N, 0, state)
            r, t = _adamw_pair(c, mask, step, coef, gs, **h)
            assert t["normal"] and r["normal"], (step, coef, gs, h)
            if step in (1, 2, 7):
                U.judge_adamw(J, (OPTIM_N, step, coef, gs, tuple(h.values())), r, t, {})
            state = {"m": t["m"], "v": t["v"]}
    J.check()


def _sgd_pair(c, mask, opt, first, coef, gs, mutant="", f32_scalars=True):
    mom, damp, nest, wd = opt
    a = (c["p"], c["g"], c["buf"], mask, U.OPTIM_LR, mom, damp, wd, nest, first, gs, coef)
    if mutant:
        return U.sgd_ref(F64, *a, mutant=mutant)
    return U.sgd_ref(F64, *a, f32_scalars=f32_scalars), U.sgd_ref(F32, *a, f32_scalars=f32_scalars)


def test_twin_sgd():
    J = U.Judge()
    mask = _mixed_mask(OPTIM_N)
    for opt in U.OPTIM_SGD_OPTIONS:
        for coef, gs in ADAMW_WAYS:
            state = None
            for first in (True, False, False):
                c = U.optim_inputs(OPTIM_N, 1, state)
                r, t = _sgd_pair(c, mask, opt, first, coef, gs)
                assert t["normal"] and r["normal"], (opt, first, coef, gs)
                assert (r["buf"] is None) == (opt[0] == 0)
                U.judge_sgd(J, (OPTIM_N, opt, first, coef, gs), r, t, {})
                state = None if opt[0] == 0 else {"buf": t["buf"]}
    J.check()


def test_twin_optim_on_the_gpu_tables():
    """the inputs tests/test_optim_ulp_gpu.py launches over - its two chunk tables, seeds and options - hold
    the twin conditions too: under the ceiling, every intermediate normal or zero (the state of a later
    step is the twin's, the stand-in for the kernel's)"""
    J = U.Judge()
    for (rows, n), seeds, steps in ((U.optim_table_rows(), (0, 3), (1, 2, 7)), (U.optim_many_rows(), (1, 4), (1, 2))):
        pi, si, dm = U.optim_rows_index(rows, n, n)
        for coef, gs in ADAMW_WAYS:
            for h in ({}, dict(b1=0.5, b2=0.75, eps=1e-3)) if coef is None and gs == 1.0 else ({},):
                m = v = torch.zeros(pi.numel())
                c = U.optim_inputs(n + 64, seeds[0])
                for step in steps:
                    r, t = _adamw_pair({"p": c["p"][pi], "g": c["g"][pi], "m": m, "v": v}, dm, step, coef, gs, **h)
                    assert t["normal"] and r["normal"]
                    U.judge_adamw(J, (n, step, coef, gs, tuple(h.values())), r, t, {})
                    m, v = t["m"], t["v"]
            c = U.optim_inputs(n + 64, seeds[1])
            for opt in U.OPTIM_SGD_OPTIONS:
                buf = None
                for first in (True, False):
                    r, t = _sgd_pair({"p": c["p"][pi], "g": c["g"][pi], "buf": buf}, dm, opt, first, coef, gs)
                    assert t["normal"] and r["normal"]
                    U.judge_sgd(J, (n, opt, first, coef, gs), r, t, {})
                    buf = t["buf"]
    J.check()


def test_twin_optim_on_the_class_inputs():
    """the inputs of test_fused_adamw_class / test_fused_sgd_class (seeds 7 and 8, three steps of g x 1, 1.5, 2,
    every option combination): under the ceiling, every intermediate normal or zero.  The clip coefficient is the
    one of these gradients, min(1, max_norm / (grad_scale |g| + 1e-6)) in float64; the gradless parameter is
    left in (it only adds elements)."""
    J = U.Judge()
    for seed, kind in ((7, "adamw"), (8, "sgd")):
        c = U.optim_class_inputs(seed)
        n = c["p"].numel()
        mask = torch.ones(n, dtype=torch.bool)
        for clip, gs in ((False, 1.0), (True, 1.0), (True, 0.125)):
            for opt in ((0.0,), (0.1,)) if kind == "adamw" else U.OPTIM_SGD_OPTIONS:
                p, st = c["p"], {"m": torch.zeros(n), "v": torch.zeros(n), "buf": None}
                for k in range(3):
                    g = c["g"] * U.optim_class_grad_factor(k)
                    coef = min(1.0, U.OPTIM_CLASS_MAX_NORM / (gs * g.double().norm().item() + 1e-6)) if clip else None
                    assert coef is None or coef < 1.0
                    if kind == "adamw":
                        r, t = _adamw_pair({"p": p, "g": g, **st}, mask, k + 1, coef, gs, wd=opt[0])
                        U.judge_adamw(J, (seed, k + 1, coef, gs, opt), r, t, {})
                        st = {"m": t["m"], "v": t["v"]}
                    else:
                        r, t = _sgd_pair({"p": p, "g": g, **st}, mask, opt, k == 0, coef, gs)
                        U.judge_sgd(J, (seed, k + 1, coef, gs, opt), r, t, {})
                        st = {"buf": t["buf"]}
                    assert t["normal"] and r["normal"], (kind, k, clip, gs, opt)
                    p = t["p"]
    J.check()


def _agree(a, b, rel=1e-12):
    return bool(((a - b).abs() <= rel * b.abs()).all())


def test_optim_refs_against_torch_in_float64():
    """the semantics are torch's: three steps with a fresh gradient each, float64 parameters, the scalars left
    as doubles, grad_scale = coef = 1, every option combination of the GPU class tests"""
    n = 3000
    ones = torch.ones(n, dtype=torch.bool)
    grads = [U.optim_inputs(n, 10 + k)["g"].double() for k in range(3)]
    p0 = U.optim_inputs(n, 10)["p"].double()
    for wd in (0.0, 0.1):
        q = torch.nn.Parameter(p0.clone())
        opt = torch.optim.AdamW([q], lr=1e-2, weight_decay=wd, foreach=False)
        p, m, v = p0.clone(), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
        for k, g in enumerate(grads):
            q.grad = g.clone()
            opt.step()
            r = U.adamw_ref(F64, p, g, m, v, ones, 1e-2, 0.9, 0.999, 1e-8, wd, k + 1, 1.0, f32_scalars=False)
            p, m, v = r["p"], r["m"], r["v"]
            assert _agree(p, q.detach()), (wd, k)
        st = opt.state[q]
        assert _agree(m, st["exp_avg"]) and _agree(v, st["exp_avg_sq"])
    for mom, damp, nest, wd in U.OPTIM_SGD_OPTIONS:
        q = torch.nn.Parameter(p0.clone())
        opt = torch.optim.SGD([q], lr=1e-2, momentum=mom, dampening=damp, nesterov=nest, weight_decay=wd, foreach=False)
        p, buf = p0.clone(), None
        for k, g in enumerate(grads):
            q.grad = g.clone()
            opt.step()
            r = U.sgd_ref(F64, p, g, buf, ones, 1e-2, mom, damp, wd, nest, k == 0, 1.0, f32_scalars=False)
            p, buf = r["p"], r["buf"]
            assert _agree(p, q.detach()), (mom, damp, nest, wd, k)
        if mom:
            assert _agree(buf, opt.state[q]["momentum_buffer"])


def test_cpu_update_paths_of_the_fused_optimizers():
    """`_torch_update` of FusedAdamW and FusedSGD (the per-tensor CPU step and the ZeRO-1 reference path) judged
    like a kernel: three steps from the state it left itself, the decay flag on and off.

    The references take the scalars as this path receives them: Python doubles, each rounded to fp32 once by
    the torch operation that uses it (`f32_scalars=False`), where a native launcher receives them already
    rounded.  The two differ in one constant that is no rounding error: the kernels form 1.f - (float)b2
    = 0.00099998713 for b2 = 0.999, this path (torch.optim's arithmetic, to which other tests hold it bit
    for bit) float(1 - b2) = 0.00100000005, 1.3e-5 apart - so exp_avg_sq of the CPU path and of the kernel
    differ by that much, and the first update by half of it.  Judged against the kernels' constants this
    path scores 1.3e-5 on v and 7.0e-6 on p at step 1, against allowances of 3.6e-6 and 4.3e-6."""
    from ray_torch_distributed_checkpoint_amd.optim import FusedAdamW, FusedSGD

    J = U.Judge()
    n = OPTIM_N
    for decay in (True, False):
        mask = torch.full((n,), decay)
        for coef, gs in ADAMW_WAYS:
            state = None
            for step in (1, 2, 3):
                c = U.optim_inputs(n, 2, state)
                r, t = _adamw_pair(c, mask, step, coef, gs, f32_scalars=False)
                p, m, v = c["p"].clone(), c["m"].clone(), c["v"].clone()
                f = gs * (1.0 if coef is None else coef)
                FusedAdamW._torch_update(p, c["g"] if f == 1.0 else c["g"] * f, m, v, step, U.OPTIM_LR, 0.9, 0.999, 1e-8,
                                         0.1, decay)
                U.judge_adamw(J, ("cpu", decay, step, coef, gs), r, t, {"p": p, "m": m, "v": v}, R=U.OPTIM_R_TORCH)
                state = {"m": m, "v": v}
        for opt in U.OPTIM_SGD_OPTIONS:
            mom, damp, nest, wd = opt
            state = None
            for first in (True, False, False):
                c = U.optim_inputs(n, 3, state)
                r, t = _sgd_pair(c, mask, opt, first, 0.37, 0.125, f32_scalars=False)
                p = c["p"].clone()
                buf = FusedSGD._torch_update(p, c["g"] * (0.125 * 0.37), None if mom == 0 else c["buf"].clone(), first,
                                             U.OPTIM_LR, mom, damp, wd if decay else 0, nest)
                U.judge_sgd(J, ("cpu", decay, opt, first), r, t, {"p": p, "buf": buf}, R=U.OPTIM_R_TORCH)
                state = None if mom == 0 else {"buf": buf}
    J.check()


# (output the mutant must miss, step / first, clip coefficient, grad_scale, SGD options)
ADAMW_MUTANT_WHERE = {"eps_inside": ("p", 1, None, 1.0), "coupled_wd": ("p", 2, None, 1.0),
                      "decay_flag_ignored": ("p", 1, None, 1.0), "coef_dropped": ("m", 2, 0.37, 1.0),
                      "bc_step_off_by_one": ("p", 2, None, 1.0)}
SGD_MUTANT_WHERE = {"nesterov_off": ("p", False, None, 1.0, (0.9, 0.0, True, 0.05)),
                    "first_dampened": ("buf", True, None, 1.0, (0.9, 0.5, False, 0.0)),
                    "wd_after_momentum": ("buf", False, None, 1.0, (0.9, 0.0, False, 0.05)),
                    "grad_scale_on_wd": ("buf", False, 0.37, 0.125, (0.9, 0.0, True, 0.05))}


def _optim_state(kind, seed):
    """a second-step state: the fp32 twin's output of a first step"""
    c = U.optim_inputs(OPTIM_N, seed)
    mask = _mixed_mask(OPTIM_N)
    if kind == "adamw":
        t = _adamw_pair(c, mask, 1, None, 1.0)[1]
        return {"m": t["m"], "v": t["v"]}
    return {"buf": _sgd_pair(c, mask, (0.9, 0.0, False, 0.05), True, None, 1.0)[1]["buf"]}


def _adamw_mutant(mutant, lr=U.OPTIM_LR):
    name, step, coef, gs = ADAMW_MUTANT_WHERE[mutant]
    c = U.optim_inputs(OPTIM_N, 4, None if step == 1 else _optim_state("adamw", 4))
    mask = _mixed_mask(OPTIM_N)
    r, t = _adamw_pair(c, mask, step, coef, gs, lr=lr)
    return name, r, t, _adamw_pair(c, mask, step, coef, gs, lr=lr, mutant=mutant)


def _sgd_mutant(mutant):
    name, first, coef, gs, opt = SGD_MUTANT_WHERE[mutant]
    c = U.optim_inputs(OPTIM_N, 5, None if first else _optim_state("sgd", 5))
    mask = _mixed_mask(OPTIM_N)
    r, t = _sgd_pair(c, mask, opt, first, coef, gs)
    return name, r, t, _sgd_pair(c, mask, opt, first, coef, gs, mutant=mutant)


OPTIM_LR_SMALL = 2.0 ** -15   # a late-schedule learning rate (3e-5): see test_old_yardstick_accepts_optim_mutants


@pytest.mark.parametrize("mutant,lr", [(m, U.OPTIM_LR) for m in U.ADAMW_MUTANTS] + [("eps_inside", OPTIM_LR_SMALL)])
def test_mutant_adamw(mutant, lr):
    """the float64 mutant, taken for a kernel output, misses the allowance on the named output"""
    name, r, t, m = _adamw_mutant(mutant, lr)
    assert _rel_caught(m[name].float(), r[name], t[name], r["S_" + name].clamp_min(U.TINY), U.OPTIM_R["adamw"][name]), mutant
    assert not _rel_caught(t[name], r[name], t[name], r["S_" + name].clamp_min(U.TINY), U.OPTIM_R["adamw"][name])


@pytest.mark.parametrize("mutant", U.SGD_MUTANTS)
def test_mutant_sgd(mutant):
    name, r, t, m = _sgd_mutant(mutant)
    assert _rel_caught(m[name].float(), r[name], t[name], r["S_" + name].clamp_min(U.TINY), U.OPTIM_R["sgd"][name]), mutant
    assert not _rel_caught(t[name], r[name], t[name], r["S_" + name].clamp_min(U.TINY), U.OPTIM_R["sgd"][name])


# what `_close(p, q, 1e-5)` of tests/test_kernels_gpu.py::test_fused_optimizers_match_torch lets through on the
# parameters of the same inputs.  At lr = 1e-3 the planted tiny gradients betray `eps_inside` even to it (the
# update there is wrong by up to 0.7 lr against 1e-5 x max |p| = 4e-5); at lr = 2^-15 they no longer do, while
# the per-element judge catches it at both (test_mutant_adamw).
OPTIM_OLD_ACCEPTS = {U.OPTIM_LR: {"wd_after_momentum", "grad_scale_on_wd"},
                     OPTIM_LR_SMALL: {"eps_inside", "coef_dropped", "decay_flag_ignored", "bc_step_off_by_one",
                                      "wd_after_momentum", "grad_scale_on_wd"}}


def test_old_yardstick_accepts_optim_mutants():
    """the gap this section closes, kept on record.

    That the old yardstick lets `eps_inside` through holds for ordinary gradients, and does NOT hold on these
    inputs at lr = 1e-3, the rate every GPU test runs at: the planted 2^-27 / 2^-30 gradients move the update
    by up to 0.7 lr = 7e-4 against its 1e-5 x max |p| = 4e-5, and it rejects the mutant.  It accepts it only
    from lr <= 6e-5 on; 2^-15 is recorded as such a rate.  At lr = 1e-3 what it does accept are the two SGD
    mutants of the weight-decay term."""
    for lr, want in OPTIM_OLD_ACCEPTS.items():
        accepted = set()
        for mutant in U.ADAMW_MUTANTS:
            _, r, _, m = _adamw_mutant(mutant, lr)
            if U.old_yardstick(m["p"].float(), r["p"], 1e-5):
                accepted.add(mutant)
        for mutant in U.SGD_MUTANTS:   # (at U.OPTIM_LR both times)
            _, r, _, m = _sgd_mutant(mutant)
            if U.old_yardstick(m["p"].float(), r["p"], 1e-5):
                accepted.add(mutant)
        print("lr", lr, "old criterion accepts:", sorted(accepted))
        assert accepted == want, (lr, accepted)


# -- embedding, dropout
def test_twin_embedding():
    J = U.Judge()
    for D in U.EMBED_WIDTHS:
        for B, T in U.EMBED_BT:
            c = U.embed_inputs(B, T, D)
            ids = c["idx"].view(-1)
            assert (ids == U.EMBED_V - 1).any() and ((ids == 0).any() or B * T == 1) and (B * T) % 4
            a = (c["idx"], c["wte"], c["wpe"], T)
            J.ulp("embed_fwd", (B, T, D), "out", None, U.embed_ref(F64, *a), U.embed_ref(F32, *a), 0.0)
        for distinct in (False, True):
            c = U.embed_bwd_inputs(D, distinct)
            for acc in (False, True):
                a = (c["idx"], c["dout"], c["dwte0"], c["dwpe0"], acc, acc)
                r, t = U.embed_bwd_ref(F64, *a), U.embed_bwd_ref(F32, *a)
                assert r["run"] == 1 if distinct else 12 <= r["run"] <= 30
                assert not r["used"].all()
                J.rel("embed_bwd", (D, distinct, acc), "dwte", None, r["dwte"], t["dwte"], r["S_dwte"].clamp_min(U.TINY),
                      r["run"] + acc)
                J.rel("embed_bwd", (D, distinct, acc), "dwpe", None, r["dwpe"], t["dwpe"], r["S_dwpe"], 2 + acc)
    J.check()


def test_dropout_mask_twin_and_references():
    """the mask twin: the kept share is 1 - p within 5 sigma, word e of call q serves element 4 q + e, a shifted
    counter gives another mask; the fp32 twins of the two references stay under their ceiling"""
    J = U.Judge()
    n = 1027
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(n, generator=gen)
    x[x == 0] = 1.0
    for p in (0.25, 0.5):
        keep = U.dropout_keep(7, 1000, n, p)
        big = U.dropout_keep(7, 1000, 1 << 16, p)
        assert torch.equal(big[:n], keep)
        assert abs(big.double().mean().item() - (1 - p)) <= 5 * (p * (1 - p) / (1 << 16)) ** 0.5
        assert torch.equal(U.dropout_keep(7, 1001, n - 4, p), keep[4:])
        r, t = U.dropout_ref(F64, x, keep, p), U.dropout_ref(F32, x, keep, p)
        assert torch.equal(r == 0, ~keep)
        J.rel("dropout", (n, p), "y", None, r, t, r.abs().clamp_min(U.TINY), 3)
        h = x.clone()
        h[::7] = 0.0
        for dy in (None, x.flip(0)):
            r, t = U.relu_dropout_ref(F64, h, keep, p, dy), U.relu_dropout_ref(F32, h, keep, p, dy)
            J.rel("relu_dropout", (n, p, dy is not None), "y", None, r, t, r.abs().clamp_min(U.TINY), 3)
    assert U.relu_dropout_ref(F32, h, torch.ones(n, dtype=torch.bool), 0.0).equal(torch.relu(h))
    J.check()


# ------------------------------------------------------------------------------- reductions
def _reduce_jobs(gen, table, dtype, seed=0, base_fill=None):
    """colsum_multi_ref jobs of a (W, D, accumulate) table; `base` is what the output holds before the launch"""
    jobs = []
    for j, (W, D, acc) in enumerate(table):
        ws = U.reduce_gen(gen, (W, D), seed + 2 * j)
        base = U.reduce_gen(gen, (D,), seed + 2 * j + 1) if acc or base_fill is None else torch.full((D,), base_fill)
        jobs.append((ws, W, D, base, bool(acc)))
    return jobs


def _jobs_abs(jobs):
    return [(ws.abs(), W, D, base.abs(), acc) for ws, W, D, base, acc in jobs]


def test_reduce_generators_and_helpers():
    """`ints` holds no zero and stays inside its bound; the partial reference puts every row into exactly one
    block and leaves the blocks past M exactly 0; the counted R of the tables; `clip_ref` on its branches"""
    v = U.reduce_gen("ints", (4160, 7), 1)
    assert v.dtype == F32 and v.abs().min() == 1 and v.abs().max() == 64 and 4160 * 64 < 2 ** 24
    assert torch.equal(v.bfloat16().float(), v)
    g = U.reduce_gen("ints", (1000,), 2, bound=1 << 10)
    assert g.abs().max() <= 1 << 10 and (1 << 20) * 16384 < 2 ** 53
    for M, nblk, N, ld in U.reduce_partial_cases():
        X = U.reduce_partial_input("ints", F32, M, N, ld, seed=M)
        p = U.colsum_partial_ref(F64, X, M, N, ld, nblk)
        assert p.shape == (nblk, N) and not p.isnan().any()
        assert torch.equal(p.sum(0), X[:, :N].double().sum(0))
        rpb = U.reduce_rpb(M, nblk)
        assert not p[-(-M // rpb):].any()
    assert [U.reduce_R_partial(M, nb) for M, nb in U.REDUCE_PARTIAL_MN] == [1, 1, 1, 5, 17]
    assert [U.reduce_R_wide(W) for W in (1, 16, 17, 192, 193, 4096)] == [1, 1, 2, 12, 13, 256]
    assert [U.reduce_ws_plan(W) for W in U.REDUCE_KNOBS_OFF_W + U.REDUCE_TWO_LAUNCH_W] == \
        [(1, 1), (1, 17), (1, 63), (2, 32), (6, 33), (64, 65), (64, 65)]
    assert U.reduce_R_ws(4097) == 17 + 16 and U.reduce_R_ws(63) == 16
    assert 63 * 65 < 4097 <= 64 * 65 and 5 * 33 < 193   # the last stage-1 block is partial
    assert U.clip_ref(4.0, 3.0, 1.0) == (6.0, U._f32(U._f32(1.0) / 6.000001))
    assert U.clip_ref(4.0, 1.0, 5.0) == (2.0, 1.0) and U.clip_ref(0.0, 1.0, 1.0) == (0.0, 1.0)
    t, c = U.clip_ref(float("nan"), 1.0, 1.0)
    assert t != t and c != c
    assert U.clip_ref(float("inf"), 1.0, 1.0) == (float("inf"), 0.0)
    assert U.ulp_f32(1.0) == 2.0 ** -23 and U.ulp_f32(1.99) == 2.0 ** -23 and U.ulp_f32(0.75) == 2.0 ** -24
    rows, n = U.gradnorm_chunks()
    assert sorted({(s & 3, ln) for s, ln in rows}) == sorted((k, ln) for ln in U.REDUCE_GRADNORM_LENS for k in range(4))
    assert all(a[0] + a[1] < b[0] for a, b in zip(rows, rows[1:])) and rows[-1][0] + rows[-1][1] <= n


def test_twin_reductions():
    """on every `offset` case of the REDUCE_* tables the fp32 twin (fp64 for the grad-norm sums) stays under its
    ceiling"""
    J = U.Judge()
    for dtype in (U.BF16, F32):
        for M, nblk, N, ld in U.reduce_partial_cases():
            X = U.reduce_partial_input("offset", dtype, M, N, ld, seed=N)
            a = (M, N, ld, nblk)
            J.rel("colsum_part", (str(dtype)[6:],) + a, "ws", None, U.colsum_partial_ref(F64, X, *a),
                  U.colsum_partial_ref(F32, X, *a), U.colsum_partial_ref(F64, X.abs(), *a).clamp_min(U.TINY),
                  U.reduce_R_partial(M, nblk))
    for W in U.REDUCE_WIDE_W + U.REDUCE_TWO_LAUNCH_W:
        for D in U.REDUCE_WIDE_D:
            for acc in (False, True):
                (job,) = _reduce_jobs("offset", [(W, D, acc)], F32, seed=W + D)
                (sc,) = U.colsum_multi_ref(F64, _jobs_abs([job]))
                for name, R in (("wide", U.reduce_R_wide(W)), ("ws", U.reduce_R_ws(W))):
                    J.rel("colsum_" + name, (W, D, acc), "out", None, U.colsum_rows_ref(F64, *job),
                          U.colsum_rows_ref(F32, *job), sc, R + acc)
    for table in (U.REDUCE_MULTI_5, U.REDUCE_MULTI_32):
        jobs = _reduce_jobs("offset", table, F32, seed=9)
        for j, (r, t, sc) in enumerate(zip(U.colsum_multi_ref(F64, jobs), U.colsum_multi_ref(F32, jobs),
                                           U.colsum_multi_ref(F64, _jobs_abs(jobs)))):
            J.rel("colsum_multi", (len(table), j) + table[j], "out", None, r, t, sc, U.reduce_R_wide(table[j][0]) + table[j][2])
    rows, n = U.gradnorm_chunks()
    g = U.reduce_gen("offset", (n,), 3)
    ex, tw = U.gradnorm_partial_exact(g, rows), U.gradnorm_partial_ref(F64, g, rows)
    for i, (s, ln) in enumerate(rows):
        J.rel64("gradnorm_part", (s & 3, ln), "partial", None, ex[i], tw[i], ex[i], U.reduce_R_gradnorm(ln))
    for k in U.REDUCE_FINALIZE_N[1:]:
        p = U.reduce_gen("offset", (k,), k, F64).square()
        ex = torch.tensor(U.fsum64(p), dtype=F64)
        J.rel64("gradnorm_fin", (k,), "local", None, ex, p.sum(), ex, U.reduce_R_finalize(k))
    for M in U.REDUCE_XENT_M:
        loss, ce = U.reduce_gen("offset", (M,), M), U.reduce_gen("offset", (M,), M + 1)
        for form in U.REDUCE_XENT_FORMS:
            tg = U.xent_finalize_targets(M, form)
            a = (loss, ce, tg, M + 2.0)
            r = U.xent_finalize_ref(F64, *a)
            J.rel("xent_finalize", (M, form), "out", None, r, U.xent_finalize_ref(F32, *a),
                  U.xent_finalize_scale(loss, ce, r[1]), U.reduce_R_finalize(M) + 1)
    J.check()


def _reduce_caught(gen, m, r, t, scale, R, rel64=False):
    """the float64 mutant m, taken for a kernel output: on `ints` it is not the reference bit for bit, on
    `offset` it is outside the allowance (a NaN is caught by both)"""
    if gen == "ints":
        assert torch.equal(t.double(), r.double())   # the honest twin is exact
        return not torch.equal(m.double(), r.double())
    allow = (U.allow_f64 if rel64 else U.allow_f32)(U.rel_err(t, r, scale), R)
    mk = m if rel64 else m.float()
    return not U.rel_err(mk, r, scale) <= allow


@pytest.mark.parametrize("gen", U.REDUCE_GENS)
@pytest.mark.parametrize("mutant", ["drop_last_row", "no_min", "pad_read"])
def test_mutant_colsum_partial(mutant, gen):
    """live: everywhere / where nblk x rpb > M (a block's range leaves the matrix) / where ld > N"""
    live = 0
    for dtype in (U.BF16, F32):
        for M, nblk, N, ld in U.reduce_partial_cases():
            rpb = U.reduce_rpb(M, nblk)
            if (mutant == "no_min" and nblk * rpb == M) or (mutant == "pad_read" and ld == N):
                continue
            live += 1
            X = U.reduce_partial_input(gen, dtype, M, N, ld, seed=N + M, extra_rows=nblk * rpb - M, pad=1.0)
            a = (M, N, ld, nblk)
            r, t = U.colsum_partial_ref(F64, X, *a), U.colsum_partial_ref(F32, X, *a)
            sc = U.colsum_partial_ref(F64, X.abs(), *a).clamp_min(U.TINY)
            m = U.colsum_partial_ref(F64, X, *a, mutant=mutant)
            assert _reduce_caught(gen, m, r, t, sc, U.reduce_R_partial(M, nblk)), (mutant, dtype, a)
            assert not _reduce_caught(gen, t.double(), r, t, sc, U.reduce_R_partial(M, nblk))
    assert live == {"drop_last_row": 210, "no_min": 168, "pad_read": 140}[mutant]


@pytest.mark.parametrize("gen", U.REDUCE_GENS)
def test_mutant_colsum_accumulate_and_jobs(gen):
    """`acc_ignored` at every accumulating case of the wide / two-launch table and every accumulating job of the
    two job tables; `job_shift` at every job of both tables"""
    for W in U.REDUCE_WIDE_W + U.REDUCE_TWO_LAUNCH_W:
        for D in U.REDUCE_WIDE_D:
            (job,) = _reduce_jobs(gen, [(W, D, 1)], F32, seed=W + D)
            (sc,) = U.colsum_multi_ref(F64, _jobs_abs([job]))
            r, t = U.colsum_rows_ref(F64, *job), U.colsum_rows_ref(F32, *job)
            m = U.colsum_rows_ref(F64, *job, mutant="acc_ignored")
            R = max(U.reduce_R_wide(W), U.reduce_R_ws(W)) + 1
            assert _reduce_caught(gen, m, r, t, sc, R), (W, D)
    for table in (U.REDUCE_MULTI_5, U.REDUCE_MULTI_32):
        jobs = _reduce_jobs(gen, table, F32, seed=9, base_fill=float("nan"))
        r, t, sc = U.colsum_multi_ref(F64, jobs), U.colsum_multi_ref(F32, jobs), U.colsum_multi_ref(F64, _jobs_abs(jobs))
        for mutant in ("acc_ignored", "job_shift"):
            m = U.colsum_multi_ref(F64, jobs, mutant=mutant)
            for j, (W, D, acc) in enumerate(table):
                if mutant == "job_shift" or acc:
                    assert _reduce_caught(gen, m[j], r[j], t[j], sc[j], U.reduce_R_wide(W) + acc), (mutant, len(table), j)
    (one,) = _reduce_jobs(gen, [(17, 64, 1)], F32)   # a single job has no neighbour: `job_shift` is not live
    assert torch.equal(U.colsum_multi_ref(F64, [one], mutant="job_shift")[0], U.colsum_multi_ref(F64, [one])[0])


@pytest.mark.parametrize("gen", U.REDUCE_GENS)
def test_mutant_gradnorm_partial(gen):
    """`tail_dropped` at every chunk on the vector path (start & 3 == 0) whose length is no multiple of 4;
    `f32_acc` at every chunk on `offset`.  `ints` is blind to `f32_acc` by construction wherever the sum stays
    below 2^24 - integer squares add exactly in fp32 too - so it is not asked to catch it."""
    rows, n = U.gradnorm_chunks()
    g = U.reduce_gen(gen, (n,), 3, bound=1 << 10)
    ex, tw = U.gradnorm_partial_exact(g, rows), U.gradnorm_partial_ref(F64, g, rows)
    tail, acc32 = U.gradnorm_partial_ref(F64, g, rows, mutant="tail_dropped"), U.gradnorm_partial_ref(F32, g, rows)
    live = 0
    for i, (s, ln) in enumerate(rows):
        R = U.reduce_R_gradnorm(ln)
        assert not _reduce_caught(gen, tw[i], ex[i], tw[i], ex[i], R, rel64=True)
        if s % 4 == 0 and ln % 4:
            live += 1
            assert _reduce_caught(gen, tail[i], ex[i], tw[i], ex[i], R, rel64=True), (s, ln)
        else:
            assert torch.equal(tail[i], tw[i])
        if gen == "offset":
            assert _reduce_caught(gen, acc32[i].double(), ex[i], tw[i], ex[i], R, rel64=True), (s, ln)
    assert live == 7


@pytest.mark.parametrize("gen", U.REDUCE_GENS)
def test_mutant_xent_finalize_no_clamp(gen):
    """live where every target is ignored (the count is 0): at every M"""
    for M in U.REDUCE_XENT_M:
        loss, ce = U.reduce_gen(gen, (M,), M), U.reduce_gen(gen, (M,), M + 1)
        for form in U.REDUCE_XENT_FORMS:
            a = (loss, ce, U.xent_finalize_targets(M, form), M + 2.0)
            r, t, m = U.xent_finalize_ref(F64, *a), U.xent_finalize_ref(F32, *a), U.xent_finalize_ref(F64, *a, mutant="no_clamp")
            sc = U.xent_finalize_scale(loss, ce, r[1])
            if form == "all_ignored":
                assert r[1] == 1 and _reduce_caught("offset", m, r, t, sc, U.reduce_R_finalize(M) + 1), M
            else:
                assert torch.equal(m, r)
