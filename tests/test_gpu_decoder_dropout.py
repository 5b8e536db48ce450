"""-m gpu: TRAIN-mode parity of the EgoT2-g sequence decoder at p > 0 - the mode C5 trains and bench.py times - against the fp64 oracle fed
the SAME dropout masks, element by element: logits, d(memory) and the gradient of every decoder, `fc` and `embedding` parameter.

tests/dropmask.py decoder_masks restates the seven sites' keys and (row, column) keying from the kernels (csrc/wide_decoder.hip: the four
attention bodies, the wide NT GEMM epilogues, dec_embed_kernel; csrc/decoder.hip and egx_dropout for the composed f32 decoder) and
oracle/translator_ref.py g_decode(masks=) applies them where nn.TransformerDecoderLayer and PositionalEncoding apply dropout. A backward that
keys a site's mask differently from its forward, a mask on the wrong side of the ReLU or the bias, or a wrong 1 / (1 - p) is an O(1) error
here: tests/test_cpu_decoder_dropout.py shows that each misses the bf16 bar by 3x and more while bf16 rounding stays within half of it.

Cases, weights, bars and the metric: tests/decoder_dropout_gate.py (bars: the project's own for the same paths at p = 0). Each case also
checks that gradients reach every decoder parameter and are finite, and that a second forward and backward with the same seed reproduces
the first bit for bit. "Every element is written" is best effort only: the autograd Functions allocate their own gradients, so the test can
do no more than hand NaN-filled blocks of the same sizes back to the caching allocator just before the run (gate._poison); that reaches the
buffers the Functions take with torch.empty (d(memory), the fused decoder's flat gradient buffer), not those they take with torch.zeros. Measured errors: profiles/
decoder_dropout_parity_report.txt (tools/decoder_dropout_report.py); each test prints its line under -s."""
import pytest
import torch

from tests import decoder_dropout_gate as gt

pytestmark = pytest.mark.gpu

EXPECT_IMPL = {"fused": "fused", "composed": "composed"}


def report_line(case, res, r) -> str:
    b = case.bars
    rep = "bit-identical" if res["repeat_equal"] else "DIFFERS " + ", ".join(f"{k.replace('transformer_decoder.layers.', '')} {v:.1e}" for k, v in res["repeat_diff"].items())
    return (f"{case.id:20s} {res['impl']:9s} logits {r['logits']:8.2e} / {b['logits']:.1e}  d(memory) {r['dmem']:8.2e} / {b['dmem']:.1e}  "
            f"worst gradient {r['grad']:8.2e} / {b['grad']:.1e} ({r['worst_grad']})  x bar {r['miss']:5.2f}  repeat {rep}")


_RUNS = {}


def _run(case, cuda):
    """The case's two GPU runs against its fp64 oracle run, reduced to the figures the tests assert on (the tensors are dropped: a case
    holds ~100 MB of gradients on both sides). Run once per case and shared by the two tests below, a failed run included."""
    if case.id in _RUNS:
        if isinstance(_RUNS[case.id], BaseException):       # nothing is run again after a failure (a GPU fault included)
            pytest.fail(f"the GPU run of {case.id} failed in the case's first test and is not repeated: {_RUNS[case.id]!r}")
        return _RUNS[case.id]
    data = gt.case_data(case)
    try:
        res = gt.gpu_run(case, data, cuda)
    except BaseException as e:
        _RUNS[case.id] = e
        raise
    ref = gt.oracle_run(case, data)
    r = gt.gate(res, ref, case.bars, gt.clip_rows(case))
    out = {"impl": res["impl"], "gate": r, "line": report_line(case, res, r), "n_grads": len(ref["grads"]),
           "finite": bool(torch.isfinite(res["logits"]).all() and torch.isfinite(res["dmem"]).all()),
           "unwritten": [k for k, g in res["grads"].items() if not torch.isfinite(g).all()],
           "repeat_equal": res["repeat_equal"], "repeat_diff": res["repeat_diff"]}
    # ragged: every clip's logits on their own (d(memory) is already the worst clip's)
    lg, lr = res["logits"].double().cpu(), ref["logits"]
    out["clip_logits"] = [(lg[:, b] - lr[:, b]).abs().max().item() / max(1.0, lr[:, b].abs().max().item()) for b in range(case.B)]
    if not r["ok"]:
        # masks or rounding? a site whose mask the kernel keys differently shows as the swap that moves the miss by an order of magnitude
        out["swaps"] = {k: round(v, 2) for k, v in gt.swap_diagnosis(case, data, res, data["masks"]).items()}
    _RUNS[case.id] = out
    return out


@pytest.mark.parametrize("cid", [c.id for c in gt.CASES])
def test_decoder_train_mode_matches_the_oracle_under_the_same_masks(egx_lib, cuda, cid):
    case = gt.BY_ID[cid]
    run = _run(case, cuda)
    r = run["gate"]
    # which path ran: a ragged batch the fused decoder serves must not have fallen back to the grouped path, whose masks differ by design
    assert run["impl"] == ("ragged" if case.lengths else EXPECT_IMPL[case.impl]), run["impl"]
    assert run["n_grads"] == 18 * gt.L + 3          # every decoder, fc and embedding parameter (the gate refuses a missing one)
    print("\n" + run["line"])
    if not r["ok"]:
        print({k: round(v, 2) for k, v in r["ratio"].items() if not v < 1.0})
        print("miss with one site's mask swapped for another seed's:", run.get("swaps"))
    assert run["finite"], "logits / d(memory) not finite"
    assert not run["unwritten"], f"gradient elements not finite (or left unwritten in a NaN-poisoned block): {run['unwritten']}"
    assert r["ok"], {k: f"{v:.2f} x bar" for k, v in r["ratio"].items() if not v < 1.0}
    if case.lengths:        # no clip left out
        assert all(e < case.bars["logits"] for e in run["clip_logits"]), list(zip(case.lengths, run["clip_logits"]))


@pytest.mark.parametrize("cid", [c.id for c in gt.CASES])
def test_a_second_run_with_the_same_seed_has_the_same_bits(egx_lib, cuda, cid):
    """Logits, d(memory) and every gradient of a second forward and backward with the same seed, bit for bit: the backward regenerates the
    forward's masks, and nothing else varies between the runs. The composed decoder got there with this test: its embedding gradient was
    an atomicAdd scatter and the bias gradient of its K | V projection a column sum whose row blocks met in atomicAdd, so
    `embedding.weight` and `multihead_attn.in_proj_bias` differed by 2e-8 .. 9e-8 relative between two runs (measured on an MI355X). The
    scatter now sums a token's rows in row order (csrc/decoder.hip embed_grad_kernel), and the composed decoder's linears take their bias
    gradients from egx_colsum_ordered (functional.linear(ordered_bias=True)); egx_linear_bwd is as it was for every other caller."""
    case = gt.BY_ID[cid]
    run = _run(case, cuda)
    print("\n" + f"{case.id:20s} repeat " + ("bit-identical" if run["repeat_equal"] else f"differs: {run['repeat_diff']}"))
    assert run["repeat_equal"], f"same seed, other bits (relative difference): {run['repeat_diff']}"
