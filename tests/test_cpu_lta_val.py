"""CPU suite of the LTA validation step (egx_lta_validate, functional.lta_validate, train.LTAValidation): the gate tests/lta_val_ref.py on
itself and on the recording of the reference's own AUED, the sampler's gate against an fp32 restatement and its perturbed versions, the
host refusals of the C entry point and the arithmetic of LTAValidation.step_result."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from tests import lta_val_ref as vr
from tests.dropmask import lcg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "live", "lta_validation.npz")
SEED, OTHER_SEED = 0x5EED0123456789AB, 0x5EED0123456789AC
SAMPLED = [i for i, c in enumerate(vr.CASES) if c[3] > 1]


# ---- the metric's gate on itself -----------------------------------------------------------------------------------------------------------
def test_levenshtein_on_hand_pairs():
    lv = vr.levenshtein
    assert lv([], []) == 0 and lv([], [1, 2, 3]) == 3 and lv([4, 5], []) == 2           # empty-prefix rows of the table
    assert lv([1, 2, 3], [1, 2, 3]) == 0 and lv([7] * 5, [7] * 5) == 0                    # all equal
    assert lv([1, 2, 3], [4, 5, 6]) == 3 and lv([1] * 4, [2] * 4) == 4                    # all different
    assert lv([1, 2, 3], [2, 3, 4]) == 2                                                 # a shift: delete + insert, not 3 substitutions
    assert lv([1, 2, 3, 4], [1, 3, 4]) == 1 and lv([1, 3, 4], [1, 2, 3, 4]) == 1
    assert lv([1, 2], [2, 1]) == 2                                                       # a transposition costs 2: plain Levenshtein, not Damerau
    assert lv([5, 1, 2, 3], [1, 2, 3, 5]) == 2
    assert lv(np.array([3, 3, 1]), torch.tensor([3, 1, 1])) == 1                         # arrays and tensors as the callers hand them in
    D = vr.levenshtein_table([1, 2], [2, 1, 1])
    assert D[0] == [0, 1, 2, 3] and [r[0] for r in D] == [0, 1, 2] and D[2][3] == 2


def test_table_diagonal_is_the_prefix_distances():
    """All Z prefix distances of a pair are the diagonal of ONE table: what the kernel relies on."""
    g = torch.Generator().manual_seed(11)
    for Z, classes in ((1, 2), (7, 3), (20, 4), (64, 5)):
        a, b = torch.randint(0, classes, (Z,), generator=g).tolist(), torch.randint(0, classes, (Z,), generator=g).tolist()
        D = vr.levenshtein_table(a, b)
        assert [D[z][z] for z in range(1, Z + 1)] == [vr.levenshtein(a[:z], b[:z]) for z in range(1, Z + 1)]


@pytest.mark.parametrize("name", ["a", "b"])
def test_aued_reproduces_the_recorded_reference(name):
    z = np.load(GOLDEN)
    preds, labels = z[f"{name}_preds"], z[f"{name}_labels"]
    out = vr.aued(preds, labels)
    Z = preds.shape[1]
    assert abs(float(out["AUED"][0]) - float(z[f"{name}_AUED"][0])) <= 1e-12
    assert max(abs(float(out[f"ED_{i}"][0]) - float(z[f"{name}_ED"][i])) for i in range(Z)) <= 1e-12
    # and through the integers the kernel returns: min_dist -> dist_sum -> step_result
    tokens = [torch.from_numpy(preds).permute(0, 2, 1).contiguous()]
    md = vr.min_dist(tokens, torch.from_numpy(labels))
    res = vr.step_result(md.sum(dim=0, dtype=torch.int64).numpy(), preds.shape[0])
    assert abs(res["val_0_AUED"] - float(z[f"{name}_AUED"][0])) <= 1e-12
    assert max(abs(res[f"val_0_ED_{i}"] - float(z[f"{name}_ED"][i])) for i in range(Z)) <= 1e-12


def test_aued_of_a_single_step_is_nan():
    out = vr.aued(np.zeros((2, 1, 3), dtype=np.int64), np.zeros((2, 1, 1), dtype=np.int64))
    assert math.isnan(float(out["AUED"][0])) and float(out["ED_0"][0]) == 0.0


def test_negative_tokens_match_no_label():
    tokens = [torch.tensor([[[-1, 2, -1]]])]
    labels = torch.tensor([[[-1], [2], [-1]]])
    assert vr.min_dist(tokens, labels)[0, :, 0].tolist() == [1, 1, 2]


# ---- the sampler's gate ------------------------------------------------------------------------------------------------------------------------
def test_uniforms_are_words_of_the_counter_generator():
    from tests.dropmask import rand_quad, site_key
    u = vr.uniforms(SEED, 3, 4, 2, 5)
    assert u.shape == (2, 3, 4, 5) and (u > 0).all() and (u < 1).all()
    key = site_key(SEED, 0x17A, 1)
    zw, yw = rand_quad(key, np.array([2 * 4 + 3]), np.array([1]))                  # row b = 2, z = 3; words 2 and 3 live in quad 1
    assert u[1, 2, 3, 2] == (float(zw[0]) + 0.5) / 2.0 ** 32 and u[1, 2, 3, 3] == (float(yw[0]) + 0.5) / 2.0 ** 32
    assert len(np.unique(u)) == u.size                                              # heads, rows and draws all read different words
    assert not np.array_equal(u, vr.uniforms(OTHER_SEED, 3, 4, 2, 5))


@pytest.fixture(scope="module")
def drawn():
    """case index -> (stack, heads, uniforms (H, B, Z, K)) of the sampled cases, built once."""
    out = {}
    for i in SAMPLED:
        B, Z, classes, K, _, _ = vr.CASES[i]
        stack, _ = vr.val_inputs(i)
        out[i] = (stack, vr.heads_of(stack, vr.CASES[i]), vr.uniforms(SEED, B, Z, len(classes), K))
    return out


@pytest.mark.parametrize("i", SAMPLED, ids=[vr.case_id(vr.CASES[i]) for i in SAMPLED])
def test_fp32_restatement_meets_the_gate(drawn, i):
    _, heads, u = drawn[i]
    for h, logits in enumerate(heads):
        tok = vr.sample_f32(logits, u[h])
        ok, worst = vr.check_draws(tok, logits, u[h])
        print(vr.case_id(vr.CASES[i]), "head", h, "worst slack", worst)
        assert ok and worst <= vr.TOL / 2, (h, worst)


def test_planted_rows_draw_what_they_must(drawn):
    stack, heads, u = drawn[vr.PLANTED]
    t0, t1 = vr.sample_f32(heads[0], u[0]), vr.sample_f32(heads[1], u[1])
    assert (t0[0, :, 0] == 2).all()                     # +80 / -80
    assert (t1[0, :, 1] == 32).all()                    # the only finite class, the last one
    assert (t1[1, :, 0] % 2 == 1).all()                 # -inf classes are never drawn
    assert (t0[1, :, 1] == -1).all() and (t1[2, :, 2] == -1).all()       # NaN row, row without a finite logit
    assert (t0[1, :, 0] >= 0).all()
    assert (vr.argmax_lowest(heads[0])[1, 0, 1] == -1) and (vr.argmax_lowest(heads[1])[0, 0, 1] == 32)


def test_argmax_lowest_on_the_planted_ties():
    stack, _ = vr.val_inputs(1)
    h0, h1 = vr.heads_of(stack, vr.CASES[1])
    assert vr.argmax_lowest(h0)[0, 0, 0] == 1 and vr.argmax_lowest(h1)[1, 0, 1] == 2 and vr.argmax_lowest(h0)[2, 0, 0] == 0


@pytest.mark.parametrize("perturb", vr.PERTURBATIONS)
def test_perturbed_sampler_misses_the_gate(drawn, perturb):
    """Every deliberate mistake of the sampler is rejected by check_draws on every sampled case it can show on."""
    rejected = 0
    for i in SAMPLED:
        B, Z, classes, K, _, _ = vr.CASES[i]
        stack, heads, u = drawn[i]
        ld, col0 = vr.case_layout(vr.CASES[i])
        u_other = vr.uniforms(OTHER_SEED, B, Z, len(classes), K)
        for h, logits in enumerate(heads):
            Ch = classes[h]
            if perturb == "wrong_window":
                if len(classes) < 2 or h != 1 or col0[0] + Ch > ld:
                    continue                            # head 1 read at head 0's columns
            if perturb == "shift_bin" and Ch == 1:
                continue                                # one class: every draw is 0 whatever the sampler does
            other = stack[..., col0[0]:col0[0] + Ch] if perturb == "wrong_window" else None
            tok = vr.sample_f32(logits, u[h], perturb, u_other=u_other[h], logits_other=other)
            ok, worst = vr.check_draws(tok, logits, u[h])
            if torch.equal(tok, vr.sample_f32(logits, u[h])):
                continue                                # e.g. a window of one class
            assert not ok and worst > 100 * vr.TOL, (perturb, vr.case_id(vr.CASES[i]), h, worst)
            rejected += 1
    assert rejected >= 2, perturb


# ---- host refusals of egx_lta_validate --------------------------------------------------------------------------------------------------------
def _call(lib, logits=0x1000, ld=12, labels=0x1000, B=5, Z=3, col0=(0, 5), classes=(5, 7), K=5, seed=1, seed_ptr=None, preds_in=None,
          preds=0x1000, min_dist=0x1000, dist_sum=0x1000, H=None):
    ia = lambda v: (C.c_int * max(len(v), 1))(*v)  # noqa: E731
    return lib.egx_lta_validate(logits, ld, labels, B, Z, len(classes) if H is None else H, ia(col0), ia(classes), K, seed, seed_ptr,
                                preds_in, preds, min_dist, dist_sum, None)


REFUSALS = [
    (dict(logits=None), "logits and preds_in are both NULL"),
    (dict(preds=None), "null pointer"),
    (dict(labels=None), "null pointer"),                                            # min_dist / dist_sum asked for without labels
    (dict(logits=None, preds_in=0x1000, labels=None, min_dist=None, dist_sum=None), "null pointer"),      # the metric-only entry needs labels
    (dict(B=0), "B >= 1"),
    (dict(Z=0), "1 <= Z <= 64"),
    (dict(Z=65), "1 <= Z <= 64"),
    (dict(K=0), "1 <= K <= 8"),
    (dict(K=9), "1 <= K <= 8"),
    (dict(H=0), "1 <= H <= 4"),
    (dict(H=5, col0=(0, 1, 2, 3, 4), classes=(1, 1, 1, 1, 1)), "1 <= H <= 4"),
    (dict(classes=(0, 7)), "1 <= C <= 2048"),
    (dict(classes=(2049,), col0=(0,), ld=4096), "1 <= C <= 2048"),
    (dict(ld=0), "ld >= 1"),
    (dict(ld=11), "of a row of ld=11"),
    (dict(col0=(-1, 5)), "of a row of ld=12"),
    (dict(col0=(0, 4)), "overlap"),
    (dict(col0=(3, 0)), "overlap"),
    (dict(B=2 ** 28, Z=2), "B * Z <= 268435456"),
    (dict(B=2 ** 31 - 1, Z=64), "B * Z <= 268435456"),
]


@pytest.mark.parametrize("kwargs,message", REFUSALS, ids=[f"{i}_{m.replace(' ', '_')}" for i, (_, m) in enumerate(REFUSALS)])
def test_host_refusals_before_any_device_work(egx_lib, kwargs, message):
    egx_lib.egx_launch_count(1)
    assert _call(egx_lib, **kwargs) != 0
    assert message.encode() in egx_lib.egx_last_error(), egx_lib.egx_last_error()
    assert egx_lib.egx_launch_count(0) == 0


def test_functional_refuses_cpu_tensors_and_bad_arguments(egx_lib):
    from egot2_amd import _lib, functional as F_egx
    with pytest.raises(_lib.EgxError, match="no CPU fallback"):
        F_egx.lta_validate([torch.zeros(2, 3, 5), torch.zeros(2, 3, 7)], torch.zeros(2, 3, 2, dtype=torch.int64), k=5)
    with pytest.raises(ValueError, match="1 to 4 heads"):
        F_egx.lta_validate([], None)
    with pytest.raises(ValueError, match="tokens must be int64"):
        F_egx.lta_validate(None, torch.zeros(2, 3, 1, dtype=torch.int64), tokens=[torch.zeros(2, 5, 3, dtype=torch.int64)])


# ---- LTAValidation ----------------------------------------------------------------------------------------------------------------------------
def test_step_result_arithmetic_and_key_names():
    """Planted dist_sum on CPU stand-in buffers: keys and values of the reference's validation step_result."""
    from egot2_amd.train import LTAValidation
    val = LTAValidation(k=5)
    with pytest.raises(RuntimeError, match="no forward"):
        val.step_result()
    B, Z, H = 4, 3, 2
    b = val._result_buffers(torch.device("cpu"), B, Z, H)
    assert b["preds"].shape == (H, B, 5, Z) and b["preds"].dtype == torch.int64
    assert b["min_dist"].shape == (B, Z, H) and b["min_dist"].dtype == torch.int32 and b["dist_sum"].dtype == torch.int64
    assert val._result_buffers(torch.device("cpu"), B, Z, H) is b                   # persistent per shape
    b["dist_sum"].copy_(torch.tensor([[0, 4], [2, 8], [6, 3]]))
    val._last = b
    r = val.step_result()
    assert set(r) == {f"val_{h}_ED_{z}" for h in range(H) for z in range(Z)} | {f"val_{h}_AUED" for h in range(H)}
    assert r["val_0_ED_0"] == 0.0 and r["val_0_ED_1"] == 2 / 8 and r["val_0_ED_2"] == 6 / 12
    assert r["val_1_ED_0"] == 1.0 and r["val_1_ED_1"] == 1.0 and r["val_1_ED_2"] == 0.25
    assert r["val_0_AUED"] == pytest.approx((0.125 + 0.375) / 2, abs=1e-15) and r["val_1_AUED"] == pytest.approx((1.0 + 0.625) / 2, abs=1e-15)
    assert r == pytest.approx(vr.step_result(b["dist_sum"].numpy(), B), abs=1e-15)
    assert set(val.step_result(prefix="test")) == {k.replace("val", "test", 1) for k in r}
    one = val._result_buffers(torch.device("cpu"), 2, 1, 1)                        # Z = 1: AUED is nan, as numpy gives the reference
    one["dist_sum"].fill_(1)
    val._last = one
    r1 = val.step_result()
    assert math.isnan(r1["val_0_AUED"]) and r1["val_0_ED_0"] == 0.5
    for k in (0, 9):
        with pytest.raises(ValueError, match="1 <= k <= 8"):
            LTAValidation(k=k)


def test_seed_word_and_manual_seed():
    from egot2_amd.train import LTAValidation
    val = LTAValidation(k=2).manual_seed(SEED)
    w = val.seed_word("cpu")
    assert w.dtype == torch.int64 and w.numel() == 1 and (int(w) & (2 ** 64 - 1)) == SEED
    assert val.seed_word("cpu") is w
    val.manual_seed(2 ** 64 - 3)                                                    # the word holds the uint64's bits
    assert (int(w) & (2 ** 64 - 1)) == 2 ** 64 - 3
    assert lcg(SEED) != SEED


def test_buffers_are_not_created_inside_a_capture(monkeypatch):
    from egot2_amd.train import LTAValidation
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="run one eager step at this problem size before capturing it in a graph"):
        LTAValidation()._result_buffers(torch.device("cuda", 0), 4, 3, 2)
    with pytest.raises(RuntimeError, match="run one eager step at this problem size before capturing it in a graph"):
        LTAValidation().seed_word(torch.device("cuda", 0))
    val = LTAValidation(k=5)
    val._bufs[("cuda", 0, 4, 3, 2)] = {}
    with pytest.raises(RuntimeError, match="host seed cannot be captured"):
        val.forward([_FakeCuda(4, 3)] * 2, None, seed=7)


class _FakeCuda:
    """Just enough of a (B, Z, C) device tensor for LTAValidation.forward to reach its capture check."""

    def __init__(self, B, Z):
        self.shape = (B, Z, 5)
        self.device = torch.device("cuda", 0)
