"""-m gpu: the PNR keyframe criterion on the device - egx_keyframe_criterion against the fp64 gate tests/keyframe_ref.py on every case,
run-to-run bits, the autograd wrapper, the recorded reference step, and train.KeyframeCriterion / OSCCCriterion on the small PNR translator,
eagerly and under GraphedStep."""
import ctypes as C
import math
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tests import keyframe_ref as kr
from tests.util import seeded_feats, seeded_state_dict

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "live", "pnr_criterion.npz")
KIND_ID = {"bce": 0, "ce": 1, "metric": 2}
KIND_NAME = {"bce": "bce", "ce": "cross_entropy", "metric": None}
_REF, _RAW, _SCRATCH = {}, {}, {}


def _ref(i):
    """fp64 reference of case i, computed once."""
    if i not in _REF:
        _REF[i] = kr.evaluate(i, kr.F64)
    return _REF[i]


def _shared_scratch(lib, dev):
    """ONE scratch for every raw launch of this module: every shape shares it, every launch leaves its counter zero."""
    if "t" not in _SCRATCH:
        _SCRATCH["t"] = torch.zeros(lib.egx_keyframe_scratch(1), dtype=torch.uint8, device=dev)
    return _SCRATCH["t"]


def _launch(lib, dev, i, scratch):
    """One launch of egx_keyframe_criterion on case i through the C ABI, every output prefilled with NaN / -7 -> dict of CPU tensors."""
    B, T, ld, cols, V, kind, flags = kr.CASES[i]
    a = kr.kf_inputs(i)
    d = lambda t: None if t is None else t.to(dev)  # noqa: E731
    x, tgt, lab, sc, fps = d(a["logits"]), d(a["target"]), d(a["label"]), d(a["state_change"]), d(a["fps"])
    start, end, pnr = (d(a["info"][k]) for k in ("clip_start_frame", "clip_end_frame", "pnr_frame"))
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    with_loss = kind != "metric"
    out = {"pred": torch.full((B,), -7, dtype=torch.int32, device=dev), "label_frame": torch.full((B,), -7, dtype=torch.int32, device=dev),
           "counts": torch.full((4,), -7, dtype=torch.int32, device=dev), "dist": torch.full((B,), float("nan"), dtype=kr.F64, device=dev),
           "dist_sum": torch.full((), float("nan"), dtype=kr.F64, device=dev)}
    if with_loss:
        out.update(loss=torch.full((), float("nan"), device=dev), loss_rows=torch.full((B,), float("nan"), device=dev),
                   d_logits=torch.full((B, ld), float("nan"), device=dev))
    ca = (C.c_int * T)(*cols) if cols is not None else None
    assert lib.egx_keyframe_scratch(B) <= scratch.numel()
    rc = lib.egx_keyframe_criterion(x.data_ptr(), ld, B, T, ca, V, KIND_ID[kind], p(tgt), p(lab), p(sc), p(fps), p(start), p(end), p(pnr),
                                    p(out.get("loss")), p(out.get("loss_rows")), p(out.get("d_logits")), p(out["pred"]), p(out["label_frame"]),
                                    p(out["counts"]), p(out["dist"]), p(out["dist_sum"]), scratch.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.egx_last_error()
    return {k: v.cpu() for k, v in out.items()}


def _raw(lib, dev, i):
    """Two launches of case i on the shared scratch -> ([run 1, run 2], the scratch's counter bytes afterwards)."""
    if i not in _RAW:
        scratch = _shared_scratch(lib, dev)
        runs = [_launch(lib, dev, i, scratch) for _ in range(2)]
        _RAW[i] = (runs, scratch[:64].cpu())
    return _RAW[i]


CASE_IDS = [kr.case_id(c) for c in kr.CASES]
ALL = range(len(kr.CASES))


def _check_against(got, ref, i):
    """The gate's rules: loss, loss_rows, d_logits within the bars (the saturated +80 / -80 row on the loss only); pred, label_frame, counts
    exact; dist exact at T = 16 and within DIST_TOL elsewhere; dist_sum within DIST_TOL."""
    case = kr.CASES[i]
    B, T, ld, cols, V, kind, flags = case
    for k in kr.EXACT:
        assert torch.equal(got[k].long(), ref[k]), (k, got[k], ref[k])
    assert kr.dist_ok(got["dist"], ref["dist"], T), (got["dist"], ref["dist"])
    assert abs(got["dist_sum"].item() - ref["dist_sum"]) <= kr.DIST_TOL * abs(ref["dist_sum"]), (got["dist_sum"].item(), ref["dist_sum"])
    if kind == "metric":
        return {}
    errs = kr.bar_errors(got, ref, i)
    print(kr.case_id(case), {k: f"{e:.2e} (bar {kr.BAR[k]:.1e})" for k, e in errs.items()})
    for k in kr.KINDS:
        assert errs[k] <= kr.BAR[k], (k, errs[k], kr.BAR[k])
    assert (got["d_logits"][ref["d_logits"] == 0] == 0).all()           # masked clips, gap columns, columns that are no frame: exact zeros
    assert torch.isfinite(got["d_logits"]).all() and torch.isfinite(got["loss_rows"]).all()       # the saturated row included
    return errs


@pytest.mark.parametrize("i", ALL, ids=CASE_IDS)
def test_operator_against_the_fp64_gate(egx_lib, cuda, i):
    (got, _), _ = _raw(egx_lib, cuda, i)
    _check_against(got, _ref(i), i)


@pytest.mark.parametrize("i", ALL, ids=CASE_IDS)
def test_two_runs_give_the_same_bits_and_leave_the_counter_zero(egx_lib, cuda, i):
    (a, b), counter = _raw(egx_lib, cuda, i)
    for k in a:
        assert torch.equal(a[k].reshape(-1).view(torch.uint8), b[k].reshape(-1).view(torch.uint8)), k
    assert (counter == 0).all()


def _functional(dev, i, requires_grad=False, upstream=None):
    """Case i through functional.keyframe_criterion -> (loss, stats, grad or None), CPU tensors."""
    from egot2_amd import functional as F_egx
    B, T, ld, cols, V, kind, flags = kr.CASES[i]
    a = kr.kf_inputs(i)
    d = lambda t: None if t is None else t.to(dev)  # noqa: E731
    x = a["logits"].to(dev).requires_grad_(requires_grad)
    preds = x if ld == V else x[:, :V]                                  # ld > V: a view with the row stride ld, read in place
    loss, stats = F_egx.keyframe_criterion(preds, d(a["target"]), d(a["label"]), d(a["state_change"]), d(a["fps"]),
                                           {k: v.to(dev) for k, v in a["info"].items()}, kind=KIND_NAME[kind], cols=cols)
    grad = None
    if requires_grad:
        (loss if upstream is None else loss * upstream).backward()
        grad = x.grad.cpu()
    return None if loss is None else loss.detach().cpu(), {k: None if v is None else v.cpu() for k, v in stats.items()}, grad


def test_two_cases_alternate_on_the_shared_scratch(egx_lib, cuda):
    """The wrapper keeps one scratch per device: calls of other shapes and kinds in between leave a case's result bits alone, and they are
    the raw launch's."""
    ids = [CASE_IDS.index(n) for n in ("B5_T16_ld16_bce", "B257_T16_ld16_ce", "B5_T16_ld593_metric_cols", "B2_T17_ld20_bce")]
    for i in (ids[0], ids[1], ids[0], ids[2], ids[3], ids[1], ids[2], ids[0]):
        egx_lib.egx_launch_count(1)
        loss, stats, grad = _functional(cuda, i, requires_grad=kr.CASES[i][5] != "metric")
        assert egx_lib.egx_launch_count(0) == 1                         # ONE launch: the backward reuses what it left behind
        (raw, _), _ = _raw(egx_lib, cuda, i)
        for k in ("pred", "label_frame", "counts", "dist", "dist_sum"):
            assert torch.equal(stats[k], raw[k]), (i, k)
        if loss is None:
            assert stats["loss_rows"] is None
            continue
        assert torch.equal(loss, raw["loss"]) and torch.equal(stats["loss_rows"], raw["loss_rows"]) and torch.equal(grad, raw["d_logits"]), i


def test_upstream_gradient_scales_d_logits(egx_lib, cuda):
    i = CASE_IDS.index("B5_T16_ld16_bce")
    _, _, g1 = _functional(cuda, i, requires_grad=True)
    _, _, g2 = _functional(cuda, i, requires_grad=True, upstream=0.5)
    assert g1.abs().max().item() > 0 and torch.equal(g2, g1 * 0.5)


def test_model_shaped_output_is_read_in_place(egx_lib, cuda):
    """The (B, 1, T) tensor forward_features returns - here a view into wider rows - goes to the launch as it lies: ld is its row stride,
    the gradient comes back in its shape, and the bits are those of the contiguous copy."""
    from egot2_amd import functional as F_egx
    i = CASE_IDS.index("B5_T16_ld16_bce")
    a = kr.kf_inputs(i)
    wide = torch.zeros(5, 24, device=cuda)
    wide[:, :16] = a["logits"].to(cuda)
    wide[:, 16:] = 99.0                                                 # must not matter
    wide.requires_grad_(True)
    preds = wide[:, :16].unsqueeze(1)
    assert preds.shape == (5, 1, 16) and not preds.is_contiguous()
    args = (a["target"].to(cuda), None, a["state_change"].to(cuda).view(5, 1), a["fps"].to(cuda), {k: v.to(cuda) for k, v in a["info"].items()})
    loss, stats = F_egx.keyframe_criterion(preds, *args)
    assert loss.grad_fn.saved_tensors[0].shape == (5, 24)               # d_logits of the rows as they lie: nothing was copied
    loss.backward()
    flat = a["logits"].to(cuda).requires_grad_(True)
    loss2, stats2 = F_egx.keyframe_criterion(flat, *args)
    loss2.backward()
    assert torch.equal(loss, loss2) and torch.equal(stats["pred"], stats2["pred"]) and torch.equal(stats["dist_sum"], stats2["dist_sum"])
    assert torch.equal(wide.grad[:, :16], flat.grad) and (wide.grad[:, 16:] == 0).all()


@pytest.mark.parametrize("name", ["a", "b"])
def test_recorded_reference_step_on_the_device(egx_lib, cuda, name):
    """The fixture of tests/golden/make_golden_pnrcrit.py (the REAL BCELoss(sigmoid(.)), masked CE, keyframe_distance, keyframe_accuracy,
    PnrOsccMetric): losses within the bars, metrics exactly."""
    from egot2_amd import functional as F_egx
    z = np.load(GOLDEN)
    t = lambda k: torch.from_numpy(z[f"{name}_{k}"]).to(cuda)  # noqa: E731
    logits, labels, sc, fps = t("logits"), t("labels"), t("sc"), t("fps")
    info = {"clip_start_frame": t("start"), "clip_end_frame": t("end"), "pnr_frame": t("pnr")}
    B = logits.shape[0]
    for kind, key, bar in (("bce", "bce", kr.BAR["loss"]), ("cross_entropy", "ce", kr.BAR["loss"])):
        loss, stats = F_egx.keyframe_criterion(logits, labels, None, sc, fps, info, kind=kind)
        want = float(z[f"{name}_{key}"])
        assert abs(loss.item() - want) <= bar * abs(want), (kind, loss.item(), want)
        n_sc, n_correct, n_outside, n = stats["counts"].tolist()
        assert [n_correct, n_sc] == z[f"{name}_acc"].tolist() and n_outside == 0 and n == B
        assert stats["dist_sum"].item() / n_sc == pytest.approx(float(z[f"{name}_dist"]), rel=kr.DIST_TOL, abs=0)
    dec = t("dec")
    none, pnr = F_egx.keyframe_criterion(dec, fps=fps, info=info, kind=None, cols=z[f"{name}_pnr_cols"].tolist())
    assert none is None
    want_dist, want_err = z[f"{name}_pnr_distance"].tolist()
    assert pnr["dist_sum"].item() / B == pytest.approx(want_dist, rel=kr.DIST_TOL, abs=0) and pnr["counts"][2].item() / B == want_err
    _, oscc = F_egx.keyframe_criterion(dec, label=sc, kind=None, cols=z[f"{name}_oscc_cols"].tolist())
    assert [oscc["counts"][1].item() / B, oscc["counts"][2].item() / B] == z[f"{name}_oscc_acc"].tolist()
    assert oscc["dist"] is None and oscc["dist_sum"] is None


# ---- model level ---------------------------------------------------------------------------------------------------------------------------
def _pnr_model(cuda, task, compute, seed=62):
    """The small PNR translator of test_gpu_fused_hoi.py (_pnr3 with L = 1, p = 0): (B, 1, 16) for the keyframe task, (B, 2, 1) for OSCC."""
    from egot2_amd import hoi_pnr
    cfg = NS(DATA=NS(TASK=task), MODEL=NS(TRANSLATION_INPUT_FEATURES=128, TRANSLATION_LAYERS=1, FEAT_DROPOUT_RATE=0.0, TRANSFORMER_DROPOUT_RATE=0.0))
    m = hoi_pnr.TaskFusionMFTransformer3TaskDropout(cfg)
    m.load_state_dict(seeded_state_dict(m, seed))
    return m.to(cuda).set_compute(compute).train()


def _pnr_batch(cuda, B, seed):
    """-> (feats, one-hot labels fp32, state_change int64 (B, 1), fps fp64, clip_start, clip_end, pnr_frame): device tensors of the dtypes the
    launch reads, so that a captured step records no conversion."""
    feats = [f.to(cuda) for f in seeded_feats(seed, [(B, 16, 8192), (B, 16, 8192), (B, 8, 2048), (B, 8, 256)])]
    g = torch.Generator().manual_seed(seed)
    labels = torch.nn.functional.one_hot(torch.randint(0, 16, (B,), generator=g), 16).float()
    sc = torch.randint(0, 2, (B, 1), generator=g)
    sc[0, 0], sc[1, 0] = 1, 0
    start = torch.randint(0, 100000, (B,), generator=g)
    span = torch.randint(1, 400, (B,), generator=g)
    pnr = start + torch.randint(0, 400, (B,), generator=g)
    fps = torch.where(torch.arange(B) % 2 == 0, torch.tensor(29.97, dtype=kr.F64), torch.tensor(30.0, dtype=kr.F64))
    return tuple([feats] + [t.to(cuda) for t in (labels, sc, fps, start, start + span, pnr)])


def _info(start, end, pnr):
    return {"clip_start_frame": start, "clip_end_frame": end, "pnr_frame": pnr}


@pytest.mark.parametrize("compute,bar", [("f32", 1e-3), ("bf16", 1e-2)])
def test_model_gradients_through_the_criterion_match_stock_bce(egx_lib, cuda, compute, bar):
    """The small PNR translator (d = 128, L = 1, B = 5): loss and every parameter gradient with KeyframeCriterion("bce") against the same
    model under stock BCELoss(sigmoid(.)), and step_result against the reference's loops run on the detached output."""
    from egot2_amd.train import KeyframeCriterion
    m = _pnr_model(cuda, "keyframe_localization", compute)
    feats, labels, sc, fps, start, end, pnr = _pnr_batch(cuda, 5, 71)
    crit = KeyframeCriterion("bce")
    stock = lambda out, y, *_: torch.nn.BCELoss(reduction="mean")(torch.sigmoid(out.squeeze(dim=1)), y)  # noqa: E731
    res = {}
    for name, fn in (("ours", crit), ("torch", stock)):
        m.zero_grad(set_to_none=True)
        out = m.forward_features(*feats)
        assert out.shape == (5, 1, 16)
        loss = fn(out, labels, sc, fps, _info(start, end, pnr))
        loss.backward()
        res[name] = (loss.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}, out.detach().cpu())
    assert abs(res["ours"][0].item() - res["torch"][0].item()) <= bar * abs(res["torch"][0].item())
    assert len(res["torch"][1]) > 15 and set(res["ours"][1]) == set(res["torch"][1])
    for k, g in res["torch"][1].items():
        assert (res["ours"][1][k] - g).norm().item() <= bar * g.norm().item() + 1e-9, k
    r = crit.step_result()
    ref = kr.keyframe_criterion(res["ours"][2][:, 0].double(), labels.cpu(), None, sc.cpu().reshape(5), fps.cpu(),
                                {k: v.cpu() for k, v in _info(start, end, pnr).items()}, 16, None, "bce")
    n_sc, n_correct = int(ref["counts"][0]), int(ref["counts"][1])
    assert n_sc >= 1 and r["pseudo_acc"] == n_correct / n_sc
    assert r["keyframe_loc_metric_time_dist_train"] == pytest.approx(ref["dist_sum"] / n_sc, rel=kr.DIST_TOL, abs=0)
    assert abs(r["loss"] - ref["loss"].item()) <= kr.BAR["loss"] * abs(ref["loss"].item()) and r["loss"] == res["ours"][0].item()
    assert torch.equal(crit.stats()["pred"].cpu().long(), ref["pred"])
    v = crit.step_result("val")
    assert v["keyframe_loc_metric_time_dist_val_neg"] == -r["keyframe_loc_metric_time_dist_train"]
    # the persistent result buffers own no autograd graph: nothing of one step stays alive into the next
    assert all(t.grad_fn is None and not t.requires_grad for t in crit.stats().values())


def test_oscc_criterion_matches_cross_entropy_and_argmax(egx_lib, cuda):
    from egot2_amd.train import OSCCCriterion
    g = torch.Generator().manual_seed(81)
    B = 7
    x = (2 * torch.randn(B, 2, 1, generator=g)).to(cuda)
    y = torch.randint(0, 2, (B, 1), generator=g).to(cuda)
    res = {}
    crit = OSCCCriterion()
    for name in ("ours", "torch"):
        p = x.clone().requires_grad_(True)
        loss = crit(p, y) if name == "ours" else torch.mean(torch.nn.functional.cross_entropy(p.squeeze(), y.long().squeeze(), reduction="none"))
        loss.backward()
        res[name] = (loss.item(), p.grad.clone())
    assert res["ours"][1].shape == (B, 2, 1)
    assert abs(res["ours"][0] - res["torch"][0]) <= 1e-6 * abs(res["torch"][0])
    assert (res["ours"][1] - res["torch"][1]).abs().max().item() <= 1e-6 * res["torch"][1].abs().max().item()
    r = crit.step_result()
    acc = (x.squeeze(-1).argmax(1) == y.squeeze(1)).float().mean().item()
    assert set(r) == {"state_change_loss", "train_loss", "loss", "state_change_metric_train"}
    assert r["state_change_metric_train"] == pytest.approx(acc, abs=1e-7) and r["loss"] == pytest.approx(res["ours"][0], rel=1e-7)
    assert crit.step_result("val") == {"state_change_metric_val": r["state_change_metric_train"]}


def test_graphed_step_replays_the_criterion_and_its_statistics(egx_lib, cuda):
    """Forward, KeyframeCriterion, backward and FusedAdam captured once and replayed on two batches: no synchronising call inside loss_fn (a
    capture fails on one), and the loss and step_result() of each replay are an eager twin's. The first replay starts from identical
    parameters: the same bits. The second follows an update whose bias gradients are atomic sums: 1e-5."""
    from egot2_amd.train import FusedAdam, GraphedStep, KeyframeCriterion
    model, twin = _pnr_model(cuda, "keyframe_localization", "f32"), _pnr_model(cuda, "keyframe_localization", "f32")
    batches = [_pnr_batch(cuda, 4, 91), _pnr_batch(cuda, 4, 92)]
    crit, crit_twin = KeyframeCriterion("bce"), KeyframeCriterion("bce")
    step = GraphedStep(lambda f, y, sc, fps, s, e, p: crit(model.forward_features(*f), y, sc, fps, _info(s, e, p)), example_inputs=batches[0],
                       params=model.parameters(), optimizer=FusedAdam(model.parameters(), lr=1e-3))
    opt_twin = FusedAdam(twin.parameters(), lr=1e-3)
    for n, (feats, y, sc, fps, s, e, p) in enumerate(batches):
        loss = step(feats, y, sc, fps, s, e, p).clone()
        got = crit.step_result()
        twin.zero_grad(set_to_none=True)
        loss_twin = crit_twin(twin.forward_features(*feats), y, sc, fps, _info(s, e, p))
        loss_twin.backward()
        opt_twin.step()
        want = crit_twin.step_result()
        assert set(got) == set(want) and len(got) == 5
        if n == 0:
            assert torch.equal(loss, loss_twin.detach()) and got == want
        else:
            assert abs(loss.item() - loss_twin.item()) <= 1e-5 * abs(loss_twin.item())
            assert all(abs(got[k] - want[k]) <= 1e-5 * max(1.0, abs(want[k])) for k in want if not math.isnan(want[k])), (got, want)
        assert got["train_loss"] == loss.item()
    assert batches[0][1].ne(batches[1][1]).any()
