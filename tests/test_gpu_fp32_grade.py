"""-m gpu: every f32 / f32s encoder path held to fp32 grade against the fp64 oracle (tests/fp32_grade.py): per-clip one-launch and cut,
sliced, deterministic with the cross entropy in the forward, the packed weight cache under dropout, ASD rows and the fused lossAV, the HOI
d = 128 recipe, tiled, ragged inference, ragged training and the shape-generic f32 kernels. The weights are kink-free (no ReLU
pre-activation within 1e-4 rms of zero), so the older 1e-3 / 1e-2 allowance for ReLU flips is not needed: outputs within 2e-6, the loss
within 2e-6 relative and every gradient within 2e-5 (with a 2e-7 sqrt(n) floor), under the implementation's own dropout masks. A kernel
that carries one operand of one product in bf16 instead of three parts misses the gradient bound by 20x and more. Each case pins and
asserts the implementation it exercises; one bf16 run per family shows that the comparison is live."""
import pytest

from tests import fp32_grade as G

pytestmark = pytest.mark.gpu


def _run(case, cuda):
    sd, marg, data = G.prepare(case)
    assert all(m >= G.MARGIN_MIN for m, _ in marg.values()), (case.id, marg)
    res = G.gpu_run(case, sd, data, cuda)
    assert res["impl"] == case.expect, (case.id, res["impl"])
    if case.family in ("perclip", "sliced", "hoi"):
        assert res["slices"] == case.slices, (case.id, res["slices"])
    if case.family == "ragged_train":
        assert res["pad_grad_zero"], case.id            # padded frames: exactly zero gradient
    return G.measure(case, res, G.oracle_run(case, sd, data))


@pytest.mark.parametrize("case", G.CASES, ids=[c.id for c in G.CASES])
def test_f32_paths_are_fp32_grade(egx_lib, cuda, case):
    m = _run(case, cuda)
    assert not m["bad"], f"{case.id} over its fp32-grade bound (multiples of the bound): {m['bad']}"


@pytest.mark.parametrize("case", G.CONTROLS, ids=[c.id for c in G.CONTROLS])
def test_bf16_control_misses_the_bound(egx_lib, cuda, case):
    """The same comparison on the bf16 arithmetic of each family misses the bound by >= 10x: gradients where the family has them, the
    outputs of ragged inference."""
    m = _run(case, cuda)
    key = ["out"] if case.family == "ragged_inf" else [k for k in m["ratio"] if k not in ("out", "loss")]
    worst = max(m["ratio"][k] for k in key)
    assert worst >= G.CONTROL_MIN, (case.id, worst)
