"""The few-row linear and the fast decode switches, as far as they go without a GPU.

* twin condition: on every case of tests/few_rows_cases.py the fp32 twin of U.gemm_ref alone
  (Judge with no kernel output) stays under its ceiling, so no case of the GPU test is
  ill-conditioned; a rounded copy of the twin is inside the allowance on every case;
* the GEMM_MUTANTS that apply to this kernel each leave the allowance on at least one case;
* the CPU path of ops.linear_few_rows is the ops.linear composition; generate(few_row=True) on the
  CPU is token for token the plain call; captured=True and more than 16 rows raise; the
  command-line flags parse and reach generate().
"""
import pytest
import torch

from tests import few_rows_cases as FR
from tests import ulp as U

F64, F32, BF16 = U.F64, U.F32, U.BF16


@pytest.mark.parametrize("shape", FR.SHAPES, ids=FR.shape_id)
def test_twin_condition_and_rounded_twin(shape):
    J, JR = U.Judge(), U.Judge()
    for gen, M, N, K, epi in FR.cases([shape]):
        c = FR.case(gen, M, N, K, epi)
        r, t = FR.refs(c)
        name = "%dx%dx%d %s %s" % (M, N, K, gen, epi)
        U.judge_gemm(J, "few-twin", name, c, r, t, {})
        U.judge_gemm(JR, "few-rounded", name, c, r, t, {"C": t["C"].to(BF16)})
    J.check()
    JR.check()


# mutant -> the epilogue of the table that shows it
MUTANT_EPI = {"truncate": "plain", "drop_k_last": "plain", "cols_scaled": "plain", "bias_shift": "bias_bf16",
              "res_after_act": "gelu_res", "gelu_of_rounded": "gelu"}


@pytest.mark.parametrize("mutant", sorted(MUTANT_EPI))
def test_mutants_leave_the_allowance(mutant):
    assert mutant in U.GEMM_MUTANTS
    epi = MUTANT_EPI[mutant]
    caught = []
    for N, K in FR.SHAPES[:-1]:
        if mutant == "bias_shift" and N < 16:   # (the mutant moves the last 8 biases from the 8 before them)
            continue
        for M in (1, 16):
            c = FR.case("randn", M, N, K, epi)
            r, t = FR.refs(c)
            m = U.gemm_ref_of(F32, c, mutant=mutant)
            floor = U.FLOOR_GEMM * r["S"]
            allow = U.allow_bf16(U.ulp_err(t["C"], r["C"], floor))
            assert U.ulp_err(t["C"].to(BF16), r["C"], floor) <= allow
            if U.ulp_err(m["C"].to(BF16), r["C"], floor) > allow:
                caught.append((M, N, K))
    assert caught, mutant


# ------------------------------------------------------------------------------- the CPU paths
def test_cpu_path_is_the_linear_composition():
    from ray_torch_distributed_checkpoint_amd import ops
    from ray_torch_distributed_checkpoint_amd.ops import gemm as G
    from ray_torch_distributed_checkpoint_amd.ops.linear import gelu_tanh_ref

    g = torch.Generator().manual_seed(5)
    x, w, b, res = (torch.randn(s, generator=g) for s in ((7, 64), (24, 64), (24,), (7, 24)))
    assert torch.equal(ops.linear_few_rows(x, w), ops.linear(x, w))
    assert torch.equal(ops.linear_few_rows(x, w, bias=b, residual=res), ops.linear(x, w, b, residual=res))
    assert torch.equal(ops.linear_few_rows(x, w, bias=b, act=G.ACT_GELU), gelu_tanh_ref(ops.linear(x, w, b)))
    assert torch.equal(ops.linear_few_rows(x, w, bias=b, act=G.ACT_GELU, residual=res),
                       gelu_tanh_ref(ops.linear(x, w, b, residual=res)))
    out = torch.empty(7, 24)
    assert ops.linear_few_rows(x, w, out=out) is out and torch.equal(out, ops.linear(x, w))
    with pytest.raises(ValueError):
        ops.linear_few_rows(torch.randn(17, 64), w)
    with pytest.raises(ValueError):
        ops.linear_few_rows(x, w, act=G.ACT_RELU)


def _model(name):
    from ray_torch_distributed_checkpoint_amd.generate import build_model

    torch.manual_seed(11)
    return build_model(name, "cpu").eval()


@pytest.mark.parametrize("name", ["gpt2-tiny", "llama3-tiny"])
def test_generate_few_row_on_the_cpu_is_the_plain_call(name):
    from ray_torch_distributed_checkpoint_amd.models.generation import new_cache

    m = _model(name)
    idx = torch.randint(0, m.cfg.vocab_size, (3, 9), generator=torch.Generator().manual_seed(2))
    for kw in ({}, {"temperature": 0.8, "top_k": 50, "seed": 7}):
        assert torch.equal(m.generate(idx, 6, few_row=True, **kw), m.generate(idx, 6, **kw))
    ca, cb = new_cache(m, 3, 12, "cpu"), new_cache(m, 3, 12, "cpu")
    assert torch.equal(m.prefill(idx, ca, few_row=True), m.prefill(idx, cb))
    assert torch.equal(m.decode_step(idx[:, 0], ca, few_row=True), m.decode_step(idx[:, 0], cb))


@pytest.mark.parametrize("name", ["gpt2-tiny", "llama3-tiny"])
def test_argument_errors(name):
    from ray_torch_distributed_checkpoint_amd.models.generation import CapturedDecode, new_cache

    m = _model(name)
    idx = torch.zeros((2, 4), dtype=torch.int64)
    with pytest.raises(ValueError, match="captured"):
        m.generate(idx, 3, captured=True)
    with pytest.raises(RuntimeError):
        CapturedDecode(m, new_cache(m, 2, 8, "cpu"))
    wide = torch.zeros((17, 4), dtype=torch.int64)
    with pytest.raises(ValueError, match="at most 16"):
        m.generate(wide, 3, few_row=True)
    cache = new_cache(m, 17, 8, "cpu")
    with pytest.raises(ValueError, match="at most 16"):
        m.prefill(wide, cache, few_row=True)
    m.prefill(wide, cache)
    with pytest.raises(ValueError, match="at most 16"):
        m.decode_step(wide[:, 0], cache, few_row=True)
    assert m.generate(wide, 2).shape == (17, 6)    # (without the switch 17 rows are fine)


def test_command_line_flags_reach_generate(monkeypatch, capsys):
    from ray_torch_distributed_checkpoint_amd import generate as Gn
    from ray_torch_distributed_checkpoint_amd.models import GPT2

    a = Gn.parse_args([])
    assert (a.few_row, a.captured) == (False, False)
    assert (Gn.parse_args(["--few-row"]).few_row, Gn.parse_args(["--few-row"]).captured) == (True, False)
    assert (Gn.parse_args(["--captured"]).few_row, Gn.parse_args(["--captured"]).captured) == (False, True)
    assert (Gn.parse_args(["--fast"]).few_row, Gn.parse_args(["--fast"]).captured) == (True, True)
    seen = []

    def fake(self, idx, n, **kw):
        seen.append(kw)
        return torch.cat([idx, idx[:, :1].expand(-1, n)], dim=1)

    monkeypatch.setattr(GPT2, "generate", fake)
    for flags in ([], ["--few-row"], ["--captured"], ["--fast"]):
        row = Gn.main(["--model", "gpt2-tiny", "--device", "cpu", "--max-new-tokens", "2", *flags])
        want = ("--few-row" in flags or "--fast" in flags, "--captured" in flags or "--fast" in flags)
        assert (seen[-1]["few_row"], seen[-1]["captured"]) == want == (row["few_row"], row["captured"])
    capsys.readouterr()
    # and for real on the CPU: --few-row runs, --captured is refused
    monkeypatch.undo()
    plain = Gn.main(["--model", "gpt2-tiny", "--device", "cpu", "--max-new-tokens", "3"])
    few = Gn.main(["--model", "gpt2-tiny", "--device", "cpu", "--max-new-tokens", "3", "--few-row"])
    assert few["tokens"] == plain["tokens"]
    with pytest.raises(ValueError, match="captured"):
        Gn.main(["--model", "gpt2-tiny", "--device", "cpu", "--max-new-tokens", "3", "--captured"])
