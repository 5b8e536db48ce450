"""-m gpu: the LTA validation step on the device - egx_lta_validate against the gate tests/lta_val_ref.py on every case (every draw against the
fp64 cdf, the edit distances exactly), run-to-run bits, the metric-only entry on the recorded AUED, one frequency check, the models' `generate`
switch and train.LTAValidation eagerly and under torch.cuda.graph."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import lta_val_ref as vr
from tests.dropmask import lcg
from tests.util import seeded_feats, seeded_state_dict

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "live", "lta_validation.npz")
SEED, OTHER_SEED = 0x5EED0123456789AB, 0x5EED0123456789AC
CASE_IDS = [vr.case_id(c) for c in vr.CASES]
_RAW, _REF = {}, {}


def _launch(lib, dev, i, seed, x=None, y=None, preds_in=None):
    """One launch of egx_lta_validate on case i through the C ABI, every output prefilled with a value it cannot take."""
    B, Z, classes, K, _, _ = vr.CASES[i]
    ld, col0 = vr.case_layout(vr.CASES[i])
    H = len(classes)
    ia = lambda v: (C.c_int * len(v))(*v)  # noqa: E731
    out = {"preds": torch.full((H, B, K, Z), -7, dtype=torch.int64, device=dev),
           "min_dist": torch.full((B, Z, H), -7, dtype=torch.int32, device=dev),
           "dist_sum": torch.full((Z, H), -7, dtype=torch.int64, device=dev)}
    rc = lib.egx_lta_validate(None if x is None else x.data_ptr(), ld, y.data_ptr(), B, Z, H, ia(col0), ia(classes), K, seed, None,
                              None if preds_in is None else preds_in.data_ptr(), out["preds"].data_ptr(), out["min_dist"].data_ptr(),
                              out["dist_sum"].data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.egx_last_error()
    return {k: v.cpu() for k, v in out.items()}


def _raw(lib, dev, i):
    """case i -> [run 1, run 2] with SEED and one run with OTHER_SEED, launched once."""
    if i not in _RAW:
        stack, labels = vr.val_inputs(i)
        x, y = stack.to(dev), labels.to(dev)
        _RAW[i] = [_launch(lib, dev, i, s, x, y) for s in (SEED, SEED, OTHER_SEED)]
    return _RAW[i]


def _ref_dist(i, tokens):
    """min_dist of the reference on the tokens the kernel returned for case i (SEED), computed once."""
    if i not in _REF:
        _REF[i] = vr.min_dist(list(tokens), vr.val_inputs(i)[1])
    return _REF[i]


@pytest.mark.parametrize("i", range(len(vr.CASES)), ids=CASE_IDS)
def test_tokens_against_the_gate(egx_lib, cuda, i):
    """K = 1: the row argmax with the lowest index among equals. K > 1: EVERY draw inside its bin of the fp64 cdf to TOL, for the uniforms
    the restated generator gives this seed; -1 exactly on the rows that cannot be sampled."""
    B, Z, classes, K, _, _ = vr.CASES[i]
    stack, _ = vr.val_inputs(i)
    got = _raw(egx_lib, cuda, i)[0]["preds"]
    u = vr.uniforms(SEED, B, Z, len(classes), K)
    for h, logits in enumerate(vr.heads_of(stack, vr.CASES[i])):
        assert got[h].min() >= -1 and got[h].max() < classes[h]
        assert torch.equal(got[h] == -1, ~vr.samplable(logits)[:, None, :].expand(B, K, Z))
        if K == 1:
            assert torch.equal(got[h], vr.argmax_lowest(logits)), h
        else:
            ok, worst = vr.check_draws(got[h], logits, u[h])
            print(vr.case_id(vr.CASES[i]), "head", h, f"worst slack {worst:.3e} (tol {vr.TOL:.0e})")
            assert ok, (h, worst)


def test_planted_rows(egx_lib, cuda):
    got = _raw(egx_lib, cuda, vr.PLANTED)[0]["preds"]
    assert (got[0][0, :, 0] == 2).all()                         # +80 / -80
    assert (got[1][0, :, 1] == 32).all()                        # one class at probability 1, the last of its window
    assert (got[1][1, :, 0] % 2 == 1).all()                     # -inf classes are never drawn
    assert (got[0][1, :, 1] == -1).all() and (got[1][2, :, 2] == -1).all()
    ties = _raw(egx_lib, cuda, 1)[0]["preds"]
    assert ties[0][0, 0, 0] == 1 and ties[1][1, 0, 1] == 2 and ties[0][2, 0, 0] == 0


@pytest.mark.parametrize("i", range(len(vr.CASES)), ids=CASE_IDS)
def test_edit_distances_are_exact(egx_lib, cuda, i):
    """min_dist and dist_sum of the launch equal the reference's recurrence, prefix by prefix, on the tokens the launch returned."""
    run = _raw(egx_lib, cuda, i)[0]
    want = _ref_dist(i, run["preds"])
    assert torch.equal(run["min_dist"], want)
    assert torch.equal(run["dist_sum"], want.sum(dim=0, dtype=torch.int64))


@pytest.mark.parametrize("i", range(len(vr.CASES)), ids=CASE_IDS)
def test_same_seed_same_bits_other_seed_other_draws(egx_lib, cuda, i):
    a, b, c = _raw(egx_lib, cuda, i)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    K, classes = vr.CASES[i][3], vr.CASES[i][2]
    if K > 1 and max(classes) > 1:
        assert not torch.equal(a["preds"], c["preds"])
    else:
        assert torch.equal(a["preds"], c["preds"])              # the argmax reads no seed


@pytest.mark.parametrize("i", [3, 4, 7], ids=[CASE_IDS[3], CASE_IDS[4], CASE_IDS[7]])
def test_tokens_handed_in_give_the_same_metric(egx_lib, cuda, i):
    """The metric-only entry (preds_in, logits NULL) on the tokens of the sampling launch: the same min_dist / dist_sum, the tokens copied."""
    run = _raw(egx_lib, cuda, i)[0]
    again = _launch(egx_lib, cuda, i, 0, None, vr.val_inputs(i)[1].to(cuda), run["preds"].to(cuda))
    for k in run:
        assert torch.equal(run[k], again[k]), k


@pytest.mark.parametrize("name", ["a", "b"])
def test_fixture_predictions_give_the_fixture_aued(egx_lib, cuda, name):
    """functional.lta_validate(tokens=...) + LTAValidation's arithmetic on the predictions of the recorded reference AUED: to 1e-12."""
    from egot2_amd import functional as F_egx
    z = np.load(GOLDEN)
    preds, labels = torch.from_numpy(z[f"{name}_preds"]), torch.from_numpy(z[f"{name}_labels"])
    N, Z, K = preds.shape
    tokens, stats = F_egx.lta_validate(None, labels.to(cuda), tokens=[preds.permute(0, 2, 1).contiguous().to(cuda)])
    assert torch.equal(tokens[0].cpu(), preds.permute(0, 2, 1))
    res = vr.step_result(stats["dist_sum"].cpu().numpy(), N)
    assert abs(res["val_0_AUED"] - float(z[f"{name}_AUED"][0])) <= 1e-12
    assert max(abs(res[f"val_0_ED_{i}"] - float(z[f"{name}_ED"][i])) for i in range(Z)) <= 1e-12
    assert torch.equal(stats["min_dist"].cpu(), vr.min_dist([preds.permute(0, 2, 1)], labels))


def test_class_frequencies(egx_lib, cuda):
    """The one check that does not go through the restated generator: 4096 identical rows of 5 classes, K = 8 -> 32768 draws; the count of
    every class within 5 binomial sigma of 32768 p."""
    from egot2_amd import functional as F_egx
    row = torch.tensor([0.3, -1.2, 1.1, 0.0, -0.4])
    p = torch.softmax(row.double(), dim=0)
    logits = row.expand(1024, 4, 5).contiguous().to(cuda)
    tokens, stats = F_egx.lta_validate([logits], None, k=8, seed=SEED)
    assert stats["min_dist"] is None and tokens[0].shape == (1024, 8, 4)
    n = 4096 * 8
    counts = torch.bincount(tokens[0].flatten().cpu(), minlength=5).double()
    sigma = torch.sqrt(n * p * (1 - p))
    print("counts", counts.tolist(), "expected", (n * p).tolist(), "sigma", sigma.tolist())
    assert counts.sum() == n and ((counts - n * p).abs() <= 5 * sigma).all()
    # rows and draws are independent: the K draws of a row are not copies of one another, nor are neighbouring rows
    t = tokens[0].cpu()
    assert (t[:, 0] != t[:, 1]).float().mean() > 0.5 and (t[:-1] != t[1:]).float().mean() > 0.5


def test_zero_copy_and_cat_routes_give_identical_tokens(egx_lib, cuda):
    from egot2_amd import functional as F_egx
    i = 3                                                               # (4, 20, (115, 478), 5): the (B, Z, 593) stack
    stack, labels = vr.val_inputs(i)
    x, y = stack.to(cuda), labels.to(cuda)
    views = vr.heads_of(x, vr.CASES[i])
    assert F_egx._seg_windows(views) is not None and F_egx._seg_windows([v.contiguous() for v in views]) is None
    egx_lib.egx_launch_count(1)
    t_v, s_v = F_egx.lta_validate(views, y, k=5, seed=SEED)
    assert egx_lib.egx_launch_count(0) == 1
    t_c, s_c = F_egx.lta_validate([v.contiguous() for v in views], y, k=5, seed=SEED)
    raw = _raw(egx_lib, cuda, i)[0]
    for h in range(2):
        assert t_v[h].shape == (4, 5, 20) and t_v[h].dtype == torch.int64
        assert torch.equal(t_v[h], t_c[h]) and torch.equal(t_v[h].cpu(), raw["preds"][h])
    assert torch.equal(s_v["dist_sum"].cpu(), raw["dist_sum"]) and torch.equal(s_c["min_dist"].cpu(), raw["min_dist"])
    # seed=None: a fresh host seed per call
    a, b = F_egx.lta_validate(views, None, k=5)[0], F_egx.lta_validate(views, None, k=5)[0]
    assert not torch.equal(a[1], b[1])


# ---- model level ---------------------------------------------------------------------------------------------------------------------------
def _lta_cfg(n=2, d=256, heads=8, layers=2, nz=3, classes=(5, 7)):
    from types import SimpleNamespace as NS
    return NS(FORECASTING=NS(NUM_INPUT_CLIPS=n, NUM_ACTIONS_TO_PREDICT=nz),
              MODEL=NS(TRANSLATION_HEADS=heads, TRANSLATION_LAYERS=layers, TRANSLATION_INPUT_FEATURES=d, TRANSLATION_DROPOUT=0.0,
                       NUM_CLASSES=list(classes), DROPOUT_RATE=0.0, HEAD_ACT="softmax"), TEST=NS(NO_ACT=False))


def _lta_model(cuda, seed=5):
    from egot2_amd import hoi_lta
    m = hoi_lta.TaskFusionMFTransformerLTA4Task(_lta_cfg())
    m.load_state_dict(seeded_state_dict(m, seed))
    return m.to(cuda).set_compute("f32").eval()


def _lta_batch(cuda, B, seed):
    feats = [f.to(cuda) for f in seeded_feats(seed, [(B, 2, 8192), (B, 2, 8192), (B, 2, 256), (B, 2, 2048)])]
    g = torch.Generator().manual_seed(seed)
    labels = torch.stack([torch.randint(0, c, (B, 3), generator=g) for c in (5, 7)], dim=-1)
    return feats, labels.to(cuda)


def test_model_generate_switch(egx_lib, cuda):
    """The small LTA 4-task model: with egx_generate the generation behind generate() returns what the torch path returns in shape, dtype and
    device; at k = 1 the same tokens (the logits are tie-free), at k = 5 draws that pass the gate's range and differ from call to call."""
    m = _lta_model(cuda)
    feats, _ = _lta_batch(cuda, 6, 41)
    with torch.no_grad():
        preds = m.forward_features(*feats)
        assert m.egx_generate is False
        want1, want5 = m._generate(preds, 1), m._generate(preds, 5)
        m.egx_generate = True
        got1, got5, got5b = m._generate(preds, 1), m._generate(preds, 5), m._generate(preds, 5)
    for want, got in ((want1, got1), (want5, got5)):
        assert len(got) == len(want) == 2
        for w, g in zip(want, got):
            assert g.shape == w.shape and g.dtype == w.dtype and g.device == w.device
    for h in range(2):
        assert all(len(torch.unique(r)) == len(r) for r in preds[h].flatten(0, 1).cpu())       # tie-free
        assert torch.equal(got1[h], want1[h])
        assert got5[h].min() >= 0 and got5[h].max() < (5, 7)[h]
    assert any(not torch.equal(a, b) for a, b in zip(got5, got5b))


def test_validation_module_eager_and_under_a_graph(egx_lib, cuda):
    """LTAValidation after one eager call, captured in a torch.cuda.graph and replayed twice: every replay draws with the seed the device word
    held before it (check_draws on every draw), advances the word by the library's step, draws differently from the replay before, and
    step_result() equals the reference on the replayed tokens."""
    from egot2_amd.train import LTAValidation
    m = _lta_model(cuda)
    feats, labels = _lta_batch(cuda, 6, 42)
    with torch.no_grad():
        stack = torch.cat(list(m.forward_features(*feats)), dim=-1)     # a stack of its own: the capture must not depend on the model's
        views = list(torch.split(stack, [5, 7], dim=-1))
    val = LTAValidation(k=5).manual_seed(SEED)
    word = val.seed_word(cuda)

    def check(tokens, seed):
        u = vr.uniforms(seed, 6, 3, 2, 5)
        for h in range(2):
            ok, worst = vr.check_draws(tokens[h].cpu(), views[h].cpu(), u[h])
            assert ok, (h, worst)
        md = vr.min_dist([t.cpu() for t in tokens], labels.cpu())
        st = val.stats()
        assert torch.equal(st["min_dist"].cpu(), md) and torch.equal(st["dist_sum"].cpu(), md.sum(dim=0, dtype=torch.int64))
        got, want = val.step_result(), vr.step_result(md.sum(dim=0, dtype=torch.int64).numpy(), 6)
        assert set(got) == set(want) == {f"val_{h}_ED_{z}" for h in range(2) for z in range(3)} | {"val_0_AUED", "val_1_AUED"}
        assert all(abs(got[k] - want[k]) <= 1e-12 for k in want)

    tokens = val(views, labels)                                         # the eager call: it creates the persistent buffers
    assert (int(word.item()) & (2 ** 64 - 1)) == lcg(SEED)
    check(tokens, SEED)
    rep = val(views, labels, seed=OTHER_SEED)                           # a host seed: repeatable, the word stays
    assert (int(word.item()) & (2 ** 64 - 1)) == lcg(SEED)
    check(rep, OTHER_SEED)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        with pytest.raises(RuntimeError, match="host seed cannot be captured"):
            val(views, labels, seed=OTHER_SEED)
        out = val(views, labels)
    val.manual_seed(SEED + 2)
    seen = []
    seed = SEED + 2
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        check(out, seed)
        seen.append([t.clone() for t in out])
        seed = lcg(seed)
        assert (int(word.item()) & (2 ** 64 - 1)) == seed
    assert any(not torch.equal(a, b) for a, b in zip(*seen))
