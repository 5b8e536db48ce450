"""-m gpu: the LTA criterion on the device - egx_segmented_ce against the fp64 gate tests/seg_ce_ref.py on every case, run-to-run bits,
the autograd wrapper's two routes, and train.LTACriterion on the small LTA 4-task model, eagerly and under GraphedStep."""
import ctypes as C

import pytest
import torch

from tests import seg_ce_ref as sr
from tests.util import seeded_feats, seeded_state_dict

pytestmark = pytest.mark.gpu

KINDS = ("loss", "loss_terms", "d_logits")
_REF, _RAW = {}, {}


def _ref(i):
    """fp64 reference of case i, computed once."""
    if i not in _REF:
        B, Z, classes, ld, _ = sr.CASES[i]
        logits, labels, ks = sr.seg_inputs(i)
        _REF[i] = sr.segmented_ce(logits.double(), labels, classes, sr.case_col0(sr.CASES[i]), ks)
    return _REF[i]


def _raw(lib, dev, i):
    """Two launches of egx_segmented_ce on case i through the C ABI, every output prefilled with NaN / -1 -> [run 1, run 2] and the scratch."""
    if i in _RAW:
        return _RAW[i]
    B, Z, classes, ld, _ = sr.CASES[i]
    col0 = sr.case_col0(sr.CASES[i])
    logits, labels, ks = sr.seg_inputs(i)
    x, y = logits.to(dev), labels.to(dev)
    H = len(classes)
    nbytes = lib.egx_segmented_ce_scratch(B, Z, H, len(ks))
    assert nbytes >= 64 * (1 + Z)
    scratch = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    ia = lambda v: (C.c_int * len(v))(*v)  # noqa: E731
    runs = []
    for _ in range(2):
        out = {"loss": torch.full((), float("nan"), device=dev), "loss_terms": torch.full((Z, H), float("nan"), device=dev),
               "n_valid": torch.full((Z, H), -1, dtype=torch.int32, device=dev),
               "correct": torch.full((len(ks), Z, H), -1, dtype=torch.int32, device=dev),
               "d_logits": torch.full((B, Z, ld), float("nan"), device=dev)}
        rc = lib.egx_segmented_ce(x.data_ptr(), ld, y.data_ptr(), B, Z, H, ia(col0), ia(classes), ia(ks), len(ks), out["loss"].data_ptr(),
                                  out["loss_terms"].data_ptr(), out["n_valid"].data_ptr(), out["correct"].data_ptr(), out["d_logits"].data_ptr(),
                                  scratch.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.egx_last_error()
        runs.append({k: v.cpu() for k, v in out.items()})
    _RAW[i] = (runs, scratch.cpu())
    return _RAW[i]


CASE_IDS = [sr.case_id(c) for c in sr.CASES]


@pytest.mark.parametrize("i", range(len(sr.CASES)), ids=CASE_IDS)
def test_operator_against_the_fp64_gate(egx_lib, cuda, i):
    """loss, loss_terms and d_logits (every element, gap columns and ignored rows included) within FACTOR x the fp32 reference's own error;
    n_valid and the top-k counts exactly."""
    ref = _ref(i)
    (got, _), _ = _raw(egx_lib, cuda, i)
    errs = {k: sr.rel_err(got[k], ref[k]) for k in KINDS}
    print(sr.case_id(sr.CASES[i]), {k: f"{e:.2e} (bar {sr.BAR[k]:.1e})" for k, e in errs.items()})
    assert torch.equal(got["n_valid"].long(), ref["n_valid"])
    assert torch.equal(got["correct"].long(), ref["correct"])
    for k in KINDS:
        assert errs[k] <= sr.BAR[k], (k, errs[k], sr.BAR[k])
    assert (got["d_logits"][ref["d_logits"] == 0] == 0).all()          # ignored rows, empty pairs, gap columns: exact zeros


@pytest.mark.parametrize("i", range(len(sr.CASES)), ids=CASE_IDS)
def test_two_runs_give_the_same_bits_and_leave_the_counter_zero(egx_lib, cuda, i):
    (a, b), scratch = _raw(egx_lib, cuda, i)
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    assert (scratch[:64 * (1 + sr.CASES[i][1])] == 0).all()             # the header's layout: 64 * (1 + Z) bytes of arrival counters


def _heads(stack, i):
    classes, col0 = sr.CASES[i][2], sr.case_col0(sr.CASES[i])
    return [stack[..., c0:c0 + c] for c0, c in zip(col0, classes)]


@pytest.mark.parametrize("i", [2, 4, 8], ids=[CASE_IDS[2], CASE_IDS[4], CASE_IDS[8]])
def test_zero_copy_and_cat_routes_give_identical_bits(egx_lib, cuda, i):
    """Views of one stack are read in place; separate tensors go through one torch.cat: the same loss, stats and gradients, bit for bit, and
    the raw launch's."""
    from egot2_amd import functional as F_egx
    logits, labels, ks = sr.seg_inputs(i)
    y = labels.to(cuda)
    res = {}
    for route in ("views", "cat"):
        stack = logits.to(cuda).requires_grad_(True)
        preds = _heads(stack, i)
        if route == "cat":
            preds = [p.contiguous() for p in preds]
        assert (F_egx._seg_windows(preds) is not None) == (route == "views")
        egx_lib.egx_launch_count(1)
        loss, stats = F_egx.segmented_cross_entropy(preds, y, ks)
        assert egx_lib.egx_launch_count(0) == 1
        loss.backward(F_egx.unit_grad(cuda))
        res[route] = (loss.detach().cpu(), stats["loss_terms"].cpu(), stats["n_valid"].cpu(), stats["correct"].cpu(), stack.grad.cpu())
    for a, b in zip(res["views"], res["cat"]):
        assert torch.equal(a, b)
    (raw, _), _ = _raw(egx_lib, cuda, i)
    assert torch.equal(res["views"][0], raw["loss"]) and torch.equal(res["views"][3], raw["correct"])
    assert torch.equal(res["views"][4], raw["d_logits"])


def test_shapes_can_alternate_on_the_shared_scratch(egx_lib, cuda):
    """The wrapper keeps one scratch per (device, Z): calls of other shapes in between (another B at the same Z, another Z) leave a shape's
    result bits alone."""
    from egot2_amd import functional as F_egx
    seen = {}
    for i in (2, 8, 4, 2, 5, 8, 4):                                     # Z = 3, 2, 2, 3, 20, 2, 2
        logits, labels, ks = sr.seg_inputs(i)
        loss, stats = F_egx.segmented_cross_entropy(_heads(logits.to(cuda), i), labels.to(cuda), ks)
        got = (loss.cpu(), stats["loss_terms"].cpu(), stats["correct"].cpu())
        (raw, _), _ = _raw(egx_lib, cuda, i)
        assert torch.equal(got[0], raw["loss"]) and torch.equal(got[1], raw["loss_terms"]) and torch.equal(got[2], raw["correct"]), i
        if i in seen:
            assert all(torch.equal(a, b) for a, b in zip(seen[i], got))
        seen[i] = got


def test_zeroed_scratch_rules(egx_lib, cuda, monkeypatch):
    """functional._zeroed_scratch: one buffer per (operator, device, key), zero-filled when created, at least `floor` bytes, an outgrown one
    retired instead of freed, and none created inside a capture."""
    import re
    from egot2_amd import functional as F_egx
    who = "zeroed_scratch_rules"
    a = F_egx._zeroed_scratch(who, cuda, 256, key=(1,))
    assert a.dtype == torch.uint8 and a.numel() == 256 and a.device == cuda and not a.any()
    assert F_egx._zeroed_scratch(who, cuda, 256, key=(1,)) is a
    assert F_egx._zeroed_scratch(who, cuda, 64, key=(1,)) is a                  # a smaller request is served by the same buffer
    z3 = F_egx._zeroed_scratch(who, cuda, 256, key=(3,))
    assert z3 is not a and z3.data_ptr() != a.data_ptr()                        # another key (Z = 1 / Z = 3): another buffer
    assert F_egx._zeroed_scratch(who + "_other", cuda, 256, key=(1,)) is not a  # another operator: another buffer
    a.fill_(0xFF)
    grown = F_egx._zeroed_scratch(who, cuda, 1024, key=(1,))
    assert grown is not a and grown.numel() == 1024 and not grown.any()         # new memory, zero-filled
    assert grown.data_ptr() != a.data_ptr() and any(t is a for t in F_egx._SCRATCH_RETIRED)      # the outgrown one is retired, not freed
    assert bool((a == 0xFF).all())                                              # and untouched: a graph may still replay into it
    assert F_egx._zeroed_scratch(who, cuda, 256, key=(1,)) is grown
    floored = F_egx._zeroed_scratch(who, cuda, 100, key=("floor",), floor=1 << 16)
    assert floored.numel() == 1 << 16 and not floored.any()
    assert F_egx._zeroed_scratch(who, cuda, 1 << 16, key=("floor",), floor=1 << 16) is floored
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    assert F_egx._zeroed_scratch(who, cuda, 1024, key=(1,)) is grown             # an existing buffer serves a capture
    with pytest.raises(RuntimeError, match="^" + re.escape(f"{who}: run one eager step at this problem size before capturing it in a graph") + "$"):
        F_egx._zeroed_scratch(who, cuda, 256, key=("capture",))
    with pytest.raises(RuntimeError, match="run one eager step at this problem size"):
        F_egx._zeroed_scratch(who, cuda, 2048, key=(1,))                        # nor is one grown inside a capture


def test_head_stack_routes(egx_lib, cuda):
    """functional._head_stack: views of one (2, 3, 10) stack are addressed in place (no copy); separate contiguous tensors go through one
    torch.cat with ld = 10 and col0 = [0, 3]; both report the same B, Z, H, widths."""
    from egot2_amd import functional as F_egx
    base = torch.arange(60, dtype=torch.float32, device=cuda).reshape(2, 3, 10)
    views = list(torch.split(base, [3, 7], dim=-1))
    B, Z, H, dev, widths, addr, ld, col0, stack = F_egx._head_stack("lta_validate", views)
    assert (B, Z, H, dev, widths) == (2, 3, 2, cuda, [3, 7])
    assert addr == base.data_ptr() and ld == 10 and list(col0) == [0, 3] and stack is None
    B2, Z2, H2, dev2, widths2, addr2, ld2, col02, stack2 = F_egx._head_stack("lta_validate", [v.contiguous() for v in views])
    assert (B2, Z2, H2, dev2, widths2) == (B, Z, H, dev, widths)
    assert ld2 == 10 and list(col02) == [0, 3]
    assert stack2 is not None and addr2 == stack2.data_ptr() and addr2 != base.data_ptr() and torch.equal(stack2, base)
    with pytest.raises(ValueError, match="^lta_validate takes 1 to 4 heads, got 5$"):
        F_egx._head_stack("lta_validate", views * 2 + views[:1])


def test_upstream_gradient_scales_d_logits(egx_lib, cuda):
    from egot2_amd import functional as F_egx
    logits, labels, ks = sr.seg_inputs(2)
    grads = []
    for scale in (None, 0.5):
        stack = logits.to(cuda).requires_grad_(True)
        loss, _ = F_egx.segmented_cross_entropy(_heads(stack, 2), labels.to(cuda), ks)
        (loss if scale is None else loss * scale).backward()
        grads.append(stack.grad.clone())
    assert grads[0].abs().max().item() > 0 and torch.equal(grads[1], grads[0] * 0.5)


# ---- model level ---------------------------------------------------------------------------------------------------------------------------
def _lta_cfg(n=2, d=256, heads=8, layers=2, nz=3, classes=(5, 7)):
    from types import SimpleNamespace as NS
    return NS(FORECASTING=NS(NUM_INPUT_CLIPS=n, NUM_ACTIONS_TO_PREDICT=nz),
              MODEL=NS(TRANSLATION_HEADS=heads, TRANSLATION_LAYERS=layers, TRANSLATION_INPUT_FEATURES=d, TRANSLATION_DROPOUT=0.0,
                       NUM_CLASSES=list(classes), DROPOUT_RATE=0.0, HEAD_ACT="softmax"), TEST=NS(NO_ACT=False))


def _lta_model(cuda, compute, seed=5):
    from egot2_amd import hoi_lta
    m = hoi_lta.TaskFusionMFTransformerLTA4Task(_lta_cfg())
    m.load_state_dict(seeded_state_dict(m, seed))
    return m.to(cuda).set_compute(compute).train()


def _lta_batch(cuda, B, seed):
    feats = [f.to(cuda) for f in seeded_feats(seed, [(B, 2, 8192), (B, 2, 8192), (B, 2, 256), (B, 2, 2048)])]
    g = torch.Generator().manual_seed(seed)
    labels = torch.stack([torch.randint(0, c, (B, 3), generator=g) for c in (5, 7)], dim=-1)
    labels[0, 1, 0] = -100
    return feats, labels.to(cuda)


def _composed_torch_criterion(preds, labels):
    """The reference's loop (long_term_anticipation.py:182-189) in stock torch."""
    loss = 0
    for h, p in enumerate(preds):
        for z in range(p.shape[1]):
            loss = loss + torch.nn.functional.cross_entropy(p[:, z], labels[:, z, h])
    return loss


@pytest.mark.parametrize("compute,bar", [("f32", 1e-3), ("bf16", 1e-2)])
def test_model_gradients_through_the_criterion_match_the_composed_torch_criterion(egx_lib, cuda, compute, bar):
    """The small LTA 4-task model (d = 256, 2 clips per task, Z = 3, classes (5, 7)): loss and every parameter gradient with LTACriterion
    against the same model under the 6 stock cross-entropy calls."""
    from egot2_amd import functional as F_egx
    from egot2_amd.train import LTACriterion
    m = _lta_model(cuda, compute)
    feats, labels = _lta_batch(cuda, 5, 21)
    crit = LTACriterion()
    res = {}
    for name, fn in (("ours", crit), ("torch", _composed_torch_criterion)):
        m.zero_grad(set_to_none=True)
        preds = m.forward_features(*feats)
        if name == "ours":
            assert F_egx._seg_windows(list(preds)) is not None          # the model's heads are views of one stack: read in place
        loss = fn(preds, labels)
        loss.backward()
        res[name] = (loss.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None})
    assert abs(res["ours"][0].item() - res["torch"][0].item()) <= bar * abs(res["torch"][0].item())
    assert len(res["torch"][1]) > 20 and set(res["ours"][1]) == set(res["torch"][1])
    for k, g in res["torch"][1].items():
        assert (res["ours"][1][k] - g).norm().item() <= bar * g.norm().item() + 1e-9, k
    r = crit.step_result()
    pairs = [(z, h) for z in range(3) for h in range(2)]
    with torch.no_grad():
        preds = [p.detach() for p in m.forward_features(*feats)]
    for z, h in pairs:                                                  # top-1 error against argmax on the valid rows
        ok = labels[:, z, h] >= 0
        want = (1 - (preds[h][ok, z].argmax(-1) == labels[ok, z, h]).float().mean().item()) * 100
        assert abs(r[f"train_{z}_{h}_top1_err"] - want) < 1e-4
    assert abs(r["train_loss"] - res["ours"][0].item()) <= 1e-6 * abs(res["ours"][0].item())
    # the persistent result buffers own no autograd graph: nothing of one step stays alive into the next
    assert all(t.grad_fn is None and not t.requires_grad for t in crit.stats().values())


def test_graphed_step_replays_the_criterion_and_its_statistics(egx_lib, cuda):
    """Forward, LTACriterion, backward and FusedAdam captured once and replayed on two label batches: no synchronising call inside loss_fn (a
    capture fails on one), and the loss and step_result() of each replay are an eager twin's. The first replay starts from identical
    parameters: the same bits. The second follows an update whose bias gradients are atomic sums: 1e-5."""
    from egot2_amd.train import FusedAdam, GraphedStep, LTACriterion
    model, twin = _lta_model(cuda, "f32"), _lta_model(cuda, "f32")
    batches = [_lta_batch(cuda, 4, 31), _lta_batch(cuda, 4, 32)]
    crit, crit_twin = LTACriterion(), LTACriterion()
    step = GraphedStep(lambda f, y: crit(model.forward_features(*f), y), example_inputs=batches[0], params=model.parameters(),
                       optimizer=FusedAdam(model.parameters(), lr=1e-3))
    opt_twin = FusedAdam(twin.parameters(), lr=1e-3)
    for n, (feats, labels) in enumerate(batches):
        loss = step(feats, labels).clone()
        got = crit.step_result()
        twin.zero_grad(set_to_none=True)
        loss_twin = crit_twin(twin.forward_features(*feats), labels)
        loss_twin.backward()
        opt_twin.step()
        want = crit_twin.step_result()
        assert set(got) == set(want) and len(got) == 3 * 2 * 2 + 2 * 2 + 1
        if n == 0:
            assert torch.equal(loss, loss_twin.detach()) and got == want
        else:
            assert abs(loss.item() - loss_twin.item()) <= 1e-5 * abs(loss_twin.item())
            assert all(abs(got[k] - want[k]) <= 1e-5 * max(1.0, abs(want[k])) for k in want), (got, want)
        assert got["train_loss"] == loss.item()
    assert batches[0][1].ne(batches[1][1]).any()

