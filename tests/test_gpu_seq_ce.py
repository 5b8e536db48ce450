"""-m gpu: the EgoT2-g multi-task criterion on the device - egx_sequence_ce against the fp64 gate tests/seq_ce_ref.py on every case,
run-to-run bits, the autograd wrapper (layouts read in place, upstream gradient), the recorded reference step, and
train.TranslationCriterion on a small HHI-g model, eagerly and under GraphedStep."""
import math

import numpy as np
import pytest
import torch

from tests import seq_ce_ref as sr
from tests.test_cpu_seq_ce import GOLDEN, check_against_recording, golden_tasks
from tests.util import hhi_args, seeded_feats, seeded_state_dict

pytestmark = pytest.mark.gpu

N = len(sr.CASES)
_REF, _RAW = {}, {}
COUNTER_BYTES = 9 * 64          # the header's layout: the launch's arrival counter and one per task, for 8 tasks always


def _ref(i):
    """fp64 reference of case i, computed once."""
    if i not in _REF:
        _REF[i] = sr.evaluate(i, sr.F64)
    return _REF[i]


def _laid_out(k, dev, fill=0.0):
    """A task's canonical (B, sy, V) rows in its layout on the device -> (storage, the (B, sy, V) view of it the launch reads)."""
    rows = k["logits"]
    B, sy, V = rows.shape
    if k["layout"] == "perm":                       # the decoder's (sy, B, V) output
        store = rows.permute(1, 0, 2).contiguous().to(dev)
        return store, store.permute(1, 0, 2)
    if k["layout"] == "contig":
        store = rows.contiguous().to(dev)
        return store, store
    store = torch.full((B, sy, V + 1), fill, device=dev)          # rows of stride V + 1: no row but the first is 8-byte aligned
    store[..., :V] = rows.to(dev)
    return store, store[..., :V]


def _targets(k, dev):
    """(B, sy + 1) tokens on the device and the target[:, 1:] view the step passes."""
    full = torch.cat([torch.zeros(k["target"].shape[0], 1, dtype=torch.int64), k["target"]], dim=1).to(dev)
    return full[:, 1:]


def _raw(lib, dev, i):
    """Two launches of egx_sequence_ce on case i through the C ABI, every output prefilled with NaN / -1 -> [run 1, run 2] and the scratch."""
    if i in _RAW:
        return _RAW[i]
    from egot2_amd._lib import SeqTask
    name, V, _ = sr.CASES[i]
    tasks = sr.seq_inputs(i)
    T = len(tasks)
    scratch = torch.zeros(lib.egx_sequence_ce_scratch(), dtype=torch.uint8, device=dev)
    runs = []
    for _ in range(2):
        arr, keep, grads, preds = (SeqTask * T)(), [], [], []
        for t, k in enumerate(tasks):
            store, x = _laid_out(k, dev, fill=99.0)
            tgt = _targets(k, dev)
            B, sy = tgt.shape
            dstore = torch.full_like(store, float("nan")) if k["grad"] else None
            a = arr[t]
            a.logits, a.stride_b, a.stride_s, a.B, a.sy = x.data_ptr(), x.stride(0), x.stride(1), B, sy
            a.target, a.target_stride_b, a.target_stride_s, a.ratio = tgt.data_ptr(), tgt.stride(0), tgt.stride(1), k["ratio"]
            if dstore is not None:
                a.d_logits = dstore.data_ptr() + 4 * (x.storage_offset() - store.storage_offset())
            wl = lab = pred = None
            if k["word_label"] is not None:
                wl, lab = k["word_label"].to(dev), k["labels"].to(dev)
                pred = torch.full((B, sy, 2), -7, dtype=torch.int32, device=dev)
                a.word_label, a.labels, a.labels_stride_b, a.labels_stride_s, a.pred = wl.data_ptr(), lab.data_ptr(), lab.stride(0), lab.stride(1), pred.data_ptr()
            keep.append((store, x, tgt, wl, lab))
            grads.append(dstore)
            preds.append(pred)
        flat = torch.full((1 + 8 * T,), -1, dtype=torch.int32, device=dev)
        rc = lib.egx_sequence_ce(arr, T, V, flat.data_ptr(), scratch.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.egx_last_error()
        torch.cuda.synchronize()
        runs.append({"flat": flat.cpu(), "grads": [None if g is None else g.cpu() for g in grads], "pred": [None if p is None else p.cpu() for p in preds]})
    _RAW[i] = (runs, scratch.cpu())
    return _RAW[i]


def _unpack(run, i):
    """A raw run in the gate's form: loss, loss_terms, counts, d_logits as canonical (B, sy, V) rows (None where not asked for), pred."""
    from egot2_amd.functional import sequence_ce_views
    tasks = sr.seq_inputs(i)
    T = len(tasks)
    v = sequence_ce_views(run["flat"], T)
    out = {k: v[k].clone() for k in ("loss", "loss_terms") + sr.COUNTS}
    out["d_logits"] = []
    for k, g in zip(tasks, run["grads"]):
        V = k["logits"].shape[2]
        if g is None:
            out["d_logits"].append(None)
        elif k["layout"] == "perm":
            out["d_logits"].append(g.permute(1, 0, 2))
        else:
            out["d_logits"].append(g[..., :V])
    out["pred"] = run["pred"]
    return out


@pytest.mark.parametrize("i", range(N), ids=sr.CASE_IDS)
def test_operator_against_the_fp64_gate(egx_lib, cuda, i):
    """loss, loss_terms and d_logits (every row, ignored ones included) within FACTOR x the fp32 reference's own error; the seven counts and
    pred exactly."""
    ref = _ref(i)
    (run, _), _ = _raw(egx_lib, cuda, i)
    got = _unpack(run, i)
    with_grad = [t for t, g in enumerate(got["d_logits"]) if g is not None]
    filled = dict(got, d_logits=[g if g is not None else ref["d_logits"][t] for t, g in enumerate(got["d_logits"])])
    errs = sr.bar_errors(filled, ref, with_grad)
    print(sr.CASE_IDS[i], {k: f"{e:.2e} (bar {sr.BAR[k]:.1e})" for k, e in errs.items()})
    for c in sr.COUNTS:
        assert torch.equal(got[c].long(), ref[c]), (c, got[c].tolist(), ref[c].tolist())
    assert sr.same_counts(got, ref)                                     # ... and pred
    for k in sr.KINDS:
        assert errs[k] <= sr.BAR[k], (k, errs[k], sr.BAR[k])
    for t in with_grad:                                                 # ignored positions, a task without a valid label, ratio 0: exact zeros
        assert (got["d_logits"][t][ref["d_logits"][t] == 0] == 0).all(), t
    for k, g in zip(sr.seq_inputs(i), run["grads"]):                    # the column between unaligned rows is never written
        if g is not None and k["layout"] == "unaligned":
            assert torch.isnan(g[..., -1]).all()


@pytest.mark.parametrize("i", range(N), ids=sr.CASE_IDS)
def test_two_runs_give_the_same_bits_and_leave_the_counters_zero(egx_lib, cuda, i):
    (a, b), scratch = _raw(egx_lib, cuda, i)
    assert torch.equal(a["flat"], b["flat"])
    for x, y in zip(a["grads"] + a["pred"], b["grads"] + b["pred"]):
        assert (x is None and y is None) or torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert (scratch[:COUNTER_BYTES] == 0).all()


def _functional_call(dev, i, upstream=None, want_pred=True):
    """Case i through functional.sequence_cross_entropy with every task in its layout -> (loss, stats, gradients as canonical rows)."""
    from egot2_amd import functional as F_egx
    tasks = sr.seq_inputs(i)
    stores, logits, targets, wls, labs = [], [], [], [], []
    for k in tasks:
        store, x = _laid_out(k, dev)
        store.requires_grad_(k["grad"])
        x = _laid_out_view(store, k)
        stores.append(store)
        logits.append(x.permute(0, 2, 1))                               # (B, V, sy): what the models return
        targets.append(_targets(k, dev))
        wls.append(None if k["word_label"] is None else k["word_label"].to(dev))
        labs.append(None if k["labels"] is None else k["labels"].to(dev))
    loss, stats = F_egx.sequence_cross_entropy(logits, targets, [k["ratio"] for k in tasks], wls, labs, want_pred=want_pred)
    grads = [None] * len(tasks)
    if any(k["grad"] for k in tasks):
        loss.backward(F_egx.unit_grad(dev) if upstream is None else upstream)
        grads = [None if s.grad is None else _laid_out_view(s.grad, k) for s, k in zip(stores, tasks)]
    return loss, stats, grads


def _laid_out_view(store, k):
    V = k["logits"].shape[2]
    return store.permute(1, 0, 2) if k["layout"] == "perm" else store[..., :V]


def test_wrapper_gives_the_raw_launch_bits_and_shapes_alternate_on_the_shared_scratch(egx_lib, cuda):
    """functional.sequence_cross_entropy keeps ONE scratch for every T and shape (the counters and partials are laid out for 8 tasks
    always): cases of T = 3, 6, 1, 8, 2 in turn, twice, give the bits of the raw launches (which had a scratch of their own)."""
    order = [sr.CASE_IDS.index(n) for n in ("hhi", "hoi", "V513", "limits", "many_rows", "hhi", "limits", "hoi", "unaligned", "contig")]
    for i in order:
        egx_lib.egx_launch_count(1)
        loss, stats, grads = _functional_call(cuda, i)
        (raw, _), _ = _raw(egx_lib, cuda, i)
        assert torch.equal(stats["flat"].cpu(), raw["flat"]), sr.CASE_IDS[i]
        assert loss.item() == raw["flat"][0:1].view(torch.float32).item()
        want = _unpack(raw, i)
        for t, g in enumerate(grads):
            assert (g is None) == (want["d_logits"][t] is None)
            if g is not None:
                assert torch.equal(g.cpu(), want["d_logits"][t]), (sr.CASE_IDS[i], t)
        for p, q in zip(stats["pred"], raw["pred"]):
            assert (p is None and q is None) or torch.equal(p.cpu(), q)


def test_one_launch_no_copy_and_the_upstream_gradient_scales_d_logits(egx_lib, cuda):
    """The (B, V, sy) view of the decoder's (sy, B, V) output is read in place - the saved gradient buffer has the view's strides, the call
    is ONE launch of the library and the gradient reaches the decoder output in its own layout - and an upstream gradient scales it."""
    from egot2_amd import functional as F_egx
    i = sr.CASE_IDS.index("hhi")
    tasks = sr.seq_inputs(i)
    outs = [k["logits"].permute(1, 0, 2).contiguous().to(cuda).requires_grad_(True) for k in tasks]         # (sy, B, V) decoder outputs
    targets = [_targets(k, cuda) for k in tasks]
    ratios = [k["ratio"] for k in tasks]
    egx_lib.egx_launch_count(1)
    loss, stats = F_egx.sequence_cross_entropy([o.permute(1, 2, 0) for o in outs], targets, ratios)
    assert egx_lib.egx_launch_count(0) == 1
    saved = loss.grad_fn.saved_tensors
    assert len(saved) == 3
    assert loss.grad_fn.read_ptrs == tuple(o.data_ptr() for o in outs)          # the launch read the decoder outputs themselves
    for o, d in zip(outs, saved):                   # d_logits as the rows lie: (B, sy, V) strided like the view, nothing was copied
        sy, B, V = o.shape
        assert tuple(d.shape) == (B, sy, V) and d.stride() == (V, B * V, 1)
    loss.backward(F_egx.unit_grad(cuda), retain_graph=True)
    unit = [o.grad.clone() for o in outs]
    assert all(g.shape == o.shape and g.is_contiguous() for g, o in zip(unit, outs))
    assert all(torch.equal(g.permute(1, 0, 2), d) for g, d in zip(unit, saved))
    for o in outs:
        o.grad = None
    (loss * 0.375).backward()
    for o, g in zip(outs, unit):
        assert torch.equal(o.grad, g * 0.375)
    ref = _ref(i)
    for t, g in enumerate(unit):
        assert sr.rel_err(g.cpu().permute(1, 0, 2), ref["d_logits"][t]) <= sr.BAR["d_logits"]
    # a class axis that is not unit-stride is made contiguous once: the same results
    copies = [o.detach().permute(1, 2, 0).contiguous().requires_grad_(True) for o in outs]
    loss2, stats2 = F_egx.sequence_cross_entropy(copies, targets, ratios)
    assert torch.equal(stats2["flat"], stats["flat"])
    assert all(p not in (c.data_ptr() for c in copies) for p in loss2.grad_fn.read_ptrs)
    loss2.backward(F_egx.unit_grad(cuda))
    assert all(c.grad.shape == c.shape and torch.equal(c.grad.permute(2, 0, 1), g) for c, g in zip(copies, unit))


@pytest.mark.parametrize("name,T", [("hhi", 3), ("hoi", 6)])
def test_recorded_reference_step_on_the_device(egx_lib, cuda, name, T):
    """The fixture of tests/golden/make_golden_gcrit.py (the REAL nn.CrossEntropyLoss on (B, V, sy), ARMetric, LTAMetric, OSCCMetric,
    PNRMetric) through train.TranslationCriterion on the recorded (sy, B, V) decoder outputs: losses within the bars, metrics exactly."""
    from egot2_amd.train import TranslationCriterion
    z = np.load(GOLDEN)
    tasks = golden_tasks(z, name, T, name == "hoi")
    crit = TranslationCriterion([k["ratio"] for k in tasks], word_labels=[k["word_label"] for k in tasks] if name == "hoi" else None,
                                want_pred=True)
    logits = [torch.from_numpy(z[f"{name}_logits{t}"]).to(cuda).permute(1, 2, 0) for t in range(T)]
    targets = [torch.from_numpy(z[f"{name}_target{t}"]).to(cuda)[:, 1:] for t in range(T)]
    labels = [torch.from_numpy(z[f"{name}_labels{t}"]).to(cuda) for t in range(T)] if name == "hoi" else None      # (B,): position 0
    loss = crit(logits, targets, labels)
    h = crit.host_result()
    want = float(z[f"{name}_loss"])
    assert abs(loss.item() - want) <= sr.BAR["loss"] * abs(want) and h["loss"] == loss.item()
    assert sr.rel_err(torch.from_numpy(h["loss_terms"]), torch.from_numpy(z[f"{name}_loss_terms"])) <= sr.BAR["loss_terms"]
    r = crit.step_result("val")
    assert r["val_loss"] == loss.item() and len([k for k in r if k.startswith("val_loss_")]) == T
    if name == "hoi":
        res = {k: torch.from_numpy(h[k]) for k in ("scored", "invalid", "correct", "correct_restricted")}
        res["pred"] = [p.cpu() for p in crit.stats()["pred"]]
        check_against_recording(res, z, name)
        assert r["val_pnr_err"] == float(z["hoi_pnrmetric"][0]) and r["val_oscc_acc_restricted"] == float(z["hoi_osccmetric"][1])
        assert r["val_lta_verb_acc"] == float(z["hoi_ltametric"][1]) and r["val_lta_noun_err"] == float(z["hoi_ltametric"][2])


# ---- model level ---------------------------------------------------------------------------------------------------------------------------
def _hhi_model(cuda, compute, seed=33):
    """A small EgoT2-g HHI model: d = 256, 4 heads, one layer, p = 0."""
    from egot2_amd import hhi_multitask
    from egot2_amd.synth import HHI_G_VOCAB
    m = hhi_multitask.TaskTranslationPromptTransformer(hhi_args(hidden_dim=256, num_heads=4, num_layers=1, dropout=0.0), HHI_G_VOCAB)
    m.load_state_dict(seeded_state_dict(m, seed))
    m.pos_embed.dropout.p = 0.0
    return m.to(cuda).set_compute(compute).train()


def _hhi_batch(cuda, vocab, B, seed):
    """-> (feats (3 x (B, 5, 256)), targets {task: (B, 3) tokens [task, answer, </s>]}): device tensors of the dtypes the launch reads."""
    feats = [f.to(cuda) for f in seeded_feats(seed, [(B, 5, 256)] * 3)]
    g = torch.Generator().manual_seed(seed)
    targets = []
    for task in ("lam", "ttm", "asd"):
        n = B * 5 if task == "asd" else B               # 'asd': one target row per frame
        ans = torch.randint(0, 2, (n,), generator=g)
        y = torch.stack([torch.full((n,), vocab[task]), torch.where(ans == 1, vocab["1"], vocab["0"]), torch.full((n,), vocab["</s>"])], dim=1)
        targets.append(y.to(cuda))
    return feats, targets


def _three_logits(m, feats, targets):
    """The three task forwards of the HHI step: (B, V, sy) views of the decoder's (sy, B, V) outputs."""
    out = []
    for task, y in zip(("lam", "ttm", "asd"), targets):
        mem = m.encode_features(task, *(feats[:1] if task == "lam" else feats))
        out.append(m.decode(y[:, :-1], mem).permute(1, 2, 0))
    return out


RATIOS = (1.0, 0.5, 2.0)


@pytest.mark.parametrize("compute,bar", [("f32", 1e-3), ("bf16", 1e-2)])
def test_model_gradients_through_the_criterion_match_stock_cross_entropy(egx_lib, cuda, compute, bar):
    """The small HHI-g model (d = 256, 4 heads, L = 1, B = 4, p = 0): loss and every parameter gradient of the three-task step with
    TranslationCriterion against the same model under the summed torch.nn.CrossEntropyLoss, and step_result against the gate run on the
    detached logits."""
    from egot2_amd.train import TranslationCriterion, binary_word_labels
    m = _hhi_model(cuda, compute)
    feats, targets = _hhi_batch(cuda, m.vocab, 4, 71)
    wl = binary_word_labels(m.vocab, len(m.vocab))
    crit = TranslationCriterion(RATIOS, word_labels=[wl, wl, wl])
    labels = [(y[:, 1] == m.vocab["1"]).long() for y in targets]                    # the answer as the original label, scored at position 0
    ce = torch.nn.CrossEntropyLoss()
    res = {}
    for name in ("ours", "torch"):
        m.zero_grad(set_to_none=True)
        logits = _three_logits(m, feats, targets)
        assert [tuple(lg.shape) for lg in logits] == [(4, 7, 2), (4, 7, 2), (20, 7, 2)] and not logits[0].is_contiguous()
        tg = [y[:, 1:] for y in targets]
        loss = crit(logits, tg, labels) if name == "ours" else sum(r * ce(lg, t) for r, lg, t in zip(RATIOS, logits, tg))
        loss.backward()
        res[name] = (loss.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None},
                     [lg.detach().cpu() for lg in logits])
    assert abs(res["ours"][0].item() - res["torch"][0].item()) <= bar * abs(res["torch"][0].item())
    assert len(res["torch"][1]) > 30 and set(res["ours"][1]) == set(res["torch"][1])
    for k, g in res["torch"][1].items():
        assert (res["ours"][1][k] - g).norm().item() <= bar * g.norm().item() + 1e-9, k
    gate = sr.sequence_ce([dict(logits=lg.permute(0, 2, 1).double(), target=y[:, 1:].cpu(), ratio=r, word_label=wl,
                                labels=torch.stack([lab.cpu(), torch.full_like(lab.cpu(), -1)], dim=1))
                           for lg, y, r, lab in zip(res["ours"][2], targets, RATIOS, labels)], 7)
    h = crit.host_result()
    for c in sr.COUNTS:
        assert h[c].tolist() == gate[c].tolist(), c
    r = crit.step_result()
    assert r["train_loss"] == res["ours"][0].item() and abs(r["train_loss"] - gate["loss"].item()) <= sr.BAR["loss"] * abs(gate["loss"].item())
    assert r["train_asd_acc_restricted"] == int(gate["correct_restricted"][2]) / 20 and r["train_lam_seq_acc"] == int(gate["seq_correct"][0]) / 4
    assert all(t.grad_fn is None and not t.requires_grad for t in crit.stats().values() if t is not None)


def test_graphed_step_replays_the_criterion_and_its_statistics(egx_lib, cuda):
    """The three task forwards, TranslationCriterion, backward and FusedAdam captured once and replayed on two batches: no synchronising
    call inside loss_fn (a capture fails on one), and the loss and step_result() of each replay are an eager twin's. The first replay
    starts from identical parameters: the same bits. The second follows an update whose bias gradients are atomic sums: 1e-5."""
    from egot2_amd.train import FusedAdam, GraphedStep, TranslationCriterion, binary_word_labels
    model, twin = _hhi_model(cuda, "f32"), _hhi_model(cuda, "f32")
    wl = binary_word_labels(model.vocab, len(model.vocab))
    crit, crit_twin = TranslationCriterion(RATIOS, word_labels=[wl] * 3), TranslationCriterion(RATIOS, word_labels=[wl] * 3)

    def labels_of(targets):             # (B, 2): the answer at position 0, position 1 not scored - built without a host synchronisation
        return [torch.stack([(y[:, 1] == model.vocab["1"]).long(), torch.full_like(y[:, 1], -1)], dim=1) for y in targets]

    def step_fn(c, mdl):
        return lambda feats, targets: c(_three_logits(mdl, feats, targets), [y[:, 1:] for y in targets], labels_of(targets))

    batches = [_hhi_batch(cuda, model.vocab, 4, 91), _hhi_batch(cuda, model.vocab, 4, 92)]
    step = GraphedStep(step_fn(crit, model), example_inputs=batches[0], params=model.parameters(), optimizer=FusedAdam(model.parameters(), lr=1e-3))
    opt_twin = FusedAdam(twin.parameters(), lr=1e-3)
    for n, (feats, targets) in enumerate(batches):
        loss = step(feats, targets).clone()
        got = crit.step_result()
        twin.zero_grad(set_to_none=True)
        loss_twin = step_fn(crit_twin, twin)(feats, targets)
        loss_twin.backward()
        opt_twin.step()
        want = crit_twin.step_result()
        assert set(got) == set(want) and len(got) == 1 + 3 * 6
        if n == 0:
            assert torch.equal(loss, loss_twin.detach()) and all(got[k] == want[k] or (math.isnan(got[k]) and math.isnan(want[k])) for k in want)
        else:
            assert abs(loss.item() - loss_twin.item()) <= 1e-5 * abs(loss_twin.item())
            assert all(abs(got[k] - want[k]) <= 1e-5 * max(1.0, abs(want[k])) for k in want if not math.isnan(want[k])), (got, want)
        assert got["train_loss"] == loss.item()
    assert any(a.ne(b).any() for a, b in zip(batches[0][1], batches[1][1]))
