"""The fp32-grade gate itself, without a GPU (tests/fp32_grade.py): for every case of the table the kink-free weights keep every ReLU
pre-activation >= 1e-4 rms away from zero, change nothing but linear1.bias and leave 30 .. 70 % of the units on; the oracle computed in
fp32 meets the bound, every gradient whose bound is set by its relative term within a quarter of it (that is what fp32-grade arithmetic
looks like; a sum that cancels to the floor term, such as a head bias over a few clips, is held to the bound itself); and the oracle with ONE operand
matrix of layer 0 rounded to bf16 misses it by >= 20x (what a kernel that drops one product to bf16 would look like)."""
import pytest
import torch

from tests import fp32_grade as G


def _relative_term_ratios(m, ref, rtol):
    """Gradient ratios of the gradients whose bound is set by rtol ||ref|| rather than by the sqrt(n) floor."""
    grads = {**ref.get("grads", {}), **ref.get("feat_grads", {})}
    return {k: m["ratio"][k] for k, g in grads.items() if rtol * g.double().norm().item() >= G.GRAD_FLOOR * g.numel() ** 0.5}


@pytest.mark.parametrize("case", G.CASES, ids=[c.id for c in G.CASES])
def test_kink_free_weights_and_the_fp32_oracle(case):
    m0 = G.new_model(case)
    sd0 = {k: v.detach().clone() for k, v in m0.state_dict().items()}
    sd, marg, data = G.prepare(case)
    assert set(sd) == set(sd0)
    changed = {k for k in sd if not torch.equal(sd[k], sd0[k])}
    assert changed == {f"{case.prefix}layers.{l}.linear1.bias" for l in range(case.L)}, changed
    assert all(sd[k].dtype == torch.float32 for k in changed)
    for layer, (margin, on) in marg.items():
        assert margin >= G.MARGIN_MIN, (layer, margin)
        assert 0.3 <= on <= 0.7, (layer, on)
    ref = G.oracle_run(case, sd, data)
    m = G.measure(case, G.oracle_run(case, sd, data, torch.float32), ref)
    assert not m["bad"], m["bad"]
    over = {k: v for k, v in _relative_term_ratios(m, ref, case.rtol).items() if v > 0.25}
    assert not over, over


SENSITIVITY = ["pc-b256-p0-one", "pc-b1-p05-one", "sl-b26", "tl-s450", "rt-ttm3-l2-p05", "ri-ttm3", "hoi-pnr3-f32s", "gen-lta4-d256"]
OPERANDS = ["self_attn.in_proj_weight", "self_attn.out_proj.weight", "linear1.weight", "linear2.weight"]


@pytest.mark.parametrize("cid", SENSITIVITY)
def test_one_bf16_operand_misses_the_bound_by_20x(cid):
    case = G.BY_ID[cid]
    sd, _, data = G.prepare(case)
    ref = G.oracle_run(case, sd, data)
    for op in OPERANDS:
        key = f"{case.prefix}layers.0.{op}"
        bad = dict(sd)
        bad[key] = sd[key].to(torch.bfloat16).to(torch.float32)
        m = G.measure(case, G.oracle_run(case, bad, data), ref)
        assert m["worst"][1] >= 20.0, (op, m["worst"])
