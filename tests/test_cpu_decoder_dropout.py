"""No GPU: the gate of the decoder's train-mode dropout (tests/decoder_dropout_gate.py) tested on the oracle itself, and tests/dropmask.py's
decoder masks on their own.

  - the oracle in fp32 under the right masks meets the f32 bar, on every case of the table;
  - the oracle on bf16-rounded weight matrices and memory (fp64 arithmetic) stays within HALF the bf16 bar under the same masks: the bar is
    reachable by bf16 arithmetic on these weights and seeds;
  - every perturbed oracle (one site's mask from another seed / shifted by one row / with scale 1 instead of 1 / (1 - p), for each of the
    seven sites and both layers; the FFN mask applied before the bias add) misses the bf16 bar by at least 3x on the logits or on a gradient;
  - decoder_masks keeps 1 - p of every site within 3 sigma, and no two sites, layers, seeds or implementations' embed sites share a mask."""
import math

import numpy as np
import pytest
import torch

from tests import decoder_dropout_gate as gt
from tests import dropmask as dm

# the shapes at which the perturbed oracles run: the fewest rows (one target token, one memory token), the bench's shape, both limits of
# the one-wave kernel, the chunked kernel, and the cases whose p_pos shows the embed site's scale
PERTURBED = ["short-sy1-s1", "short-sy2-s45", "short-sy8-s64", "long-s180", "embed-p03-sy1", "embed-p03-sy2"]


def _ref(case):
    """The fp64 oracle run of a case under its own masks."""
    return gt.oracle_run(case, gt.case_data(case))


def test_case_table_holds_every_listed_case():
    ids = set(gt.BY_ID)
    assert {f"short-sy{sy}-s{S}" for sy in (1, 2, 8) for S in (1, 45, 64)} <= ids
    assert {"short-dh32", "long-s65", "long-s180", "composed-sy2-s45", "composed-sy8-s64", "composed-sy3-s180",
            "only-p-drop", "only-p-pos", "devseed-short", "devseed-long", "ragged", "hoi"} <= ids
    # whole chunks only, at least three, at the chunk length read from the kernel; the other long cases end in a partial chunk
    for cid in (f"long-s{3 * gt.CHUNK}-sy2", f"long-s{3 * gt.CHUNK}-sy8"):
        assert gt.BY_ID[cid].S % gt.CHUNK == 0 and gt.BY_ID[cid].S // gt.CHUNK >= 3
    assert gt.BY_ID["long-s65"].S % gt.CHUNK == 1 and gt.BY_ID["long-s180"].S % gt.CHUNK not in (0, 1)
    rg = gt.BY_ID["ragged"]
    assert min(rg.lengths) <= 64 < max(rg.lengths) and {1, 64, 65} <= set(rg.lengths)
    for c in gt.CASES:
        assert c.B <= 5 and (c.p_drop > 0 or c.p_pos > 0) and c.bars == (gt.BF16_BAR if c.impl == "fused" else gt.F32_BAR), c.id
        if c.id not in ("only-p-drop", "only-p-pos") and not c.id.startswith("embed-p03"):
            assert (c.p_drop, c.p_pos) == (0.3, 0.1), c.id
    assert (gt.BY_ID["only-p-drop"].p_pos, gt.BY_ID["only-p-pos"].p_drop) == (0.0, 0.0)


@pytest.mark.parametrize("cid", [c.id for c in gt.CASES])
def test_fp32_oracle_meets_the_f32_bar_and_bf16_weights_half_the_bf16_bar(cid):
    case = gt.BY_ID[cid]
    data, ref = gt.case_data(case), _ref(case)
    rows = gt.clip_rows(case)
    assert all(m > 1e-3 and 0.3 < pos < 0.7 for m, pos in data["margins"].values()), data["margins"]
    f32 = gt.gate(gt.oracle_run(case, data, dtype=torch.float32), ref, gt.F32_BAR, rows)
    bf = gt.gate(gt.oracle_run(case, data, bf16_weights=True), ref, gt.BF16_BAR, rows)
    print(f"{cid}: fp32 oracle {f32['miss']:.2e} x f32 bar; bf16 weights {bf['miss']:.2f} x bf16 bar (logits {bf['logits']:.2e}, d(memory) "
          f"{bf['dmem']:.2e}, worst gradient {bf['grad']:.2e} {bf['worst_grad']})")
    assert f32["ok"], f32["ratio"]
    assert bf["miss"] < gt.BF16_WEIGHTS_MAX, {k: round(v, 3) for k, v in bf["ratio"].items() if v >= gt.BF16_WEIGHTS_MAX}
    # the masks matter: the eval-mode oracle is far from the masked one
    none = {"embed": None, "layers": [None] * gt.L}
    ev = gt.gate(gt.oracle_run(case, data, masks=[none] * len(case.lengths) if case.lengths else none), ref, gt.BF16_BAR, rows)
    assert ev["miss"] > gt.PERTURBED_MIN, ev["miss"]


@pytest.mark.parametrize("cid", PERTURBED)
def test_every_perturbed_oracle_misses_the_bf16_bar_by_3x(cid):
    case = gt.BY_ID[cid]
    data, ref = gt.case_data(case), _ref(case)
    seen, weak = [], {}
    for name, masks, decode in gt.perturbations(case, data):
        r = gt.gate(gt.oracle_run(case, data, masks=masks, decode=decode), ref, gt.BF16_BAR)
        seen.append((r["miss"], name))
        if not r["miss"] >= gt.PERTURBED_MIN:
            weak[name] = round(r["miss"], 2)
    kinds = {n.split("/")[0] for _, n in seen}
    sites = {n.split("/")[1].split(".")[0] for _, n in seen if "/" in n}
    assert kinds == {"other-seed", "row-shift", "scale-1", "ffn-mask-before-bias"} and sites == set(dm.DEC_SITES)
    assert ("scale-1/embed" in {n for _, n in seen}) == (case.p_pos >= gt.EMBED_SCALE_MIN_P)
    print(f"{cid}: {len(seen)} perturbed oracles, smallest miss {min(seen)[0]:.2f} x bf16 bar ({min(seen)[1]})")
    assert not weak, weak


def test_keep_rates_and_distinct_masks():
    B, sy, S, d, H, d_ff, p, p_pos = 5, 8, 192, 256, 4, 2048, 0.3, 0.1
    m = dm.decoder_masks(0xABCDE, "fused", B, sy, S, d, H, d_ff, 2, p, p_pos)
    assert m["embed"].shape == (B, sy, d) and m["embed"].dtype == torch.float64
    shapes = {"self": (B, H, sy, sy), "sa_out": (B, sy, d), "cross": (B, H, sy, S), "ca_out": (B, sy, d), "ffn": (B, sy, d_ff), "ffn_out": (B, sy, d)}
    flat = {"embed": (m["embed"], p_pos)}
    for l, layer in enumerate(m["layers"]):
        assert set(layer) == set(shapes)
        for k, t in layer.items():
            assert t.shape == shapes[k], (k, t.shape)
            flat[f"{k}.{l}"] = (t, p)
    for name, (t, q) in flat.items():
        q16 = dm.drop_threshold(q) / 65536.0                    # the probability the 16-bit threshold realises
        assert set(t.unique().tolist()) == {0.0, dm.inv_keep(q)}, name
        keep, n = (t > 0).double().mean().item(), t.numel()
        assert abs(keep - (1 - q16)) < 3 * math.sqrt(q16 * (1 - q16) / n), (name, keep, n)
    assert abs(dm.inv_keep(p) - 1 / 0.7) < 1e-6 and abs(dm.inv_keep(p_pos) - 1 / 0.9) < 1e-6
    # distinct sites and layers: no two same-shaped masks agree on more elements than independent draws would (p^2 + (1 - p)^2 + 5 sigma)
    names = list(flat)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            ta, tb = flat[a][0], flat[b][0]
            if ta.shape != tb.shape or flat[a][1] != flat[b][1]:
                continue
            q = flat[a][1]
            agree = ((ta > 0) == (tb > 0)).double().mean().item()
            indep = q * q + (1 - q) * (1 - q)
            assert agree < indep + 5 * math.sqrt(indep * (1 - indep) / ta.numel()), (a, b, agree)
    # another seed, and the composed path's embed key, draw other masks; every per-layer site is shared by the two implementations
    o = dm.decoder_masks(0xABCDF, "fused", B, sy, S, d, H, d_ff, 2, p, p_pos)
    c = dm.decoder_masks(0xABCDE, "composed", B, sy, S, d, H, d_ff, 2, p, p_pos)
    assert not torch.equal(o["embed"], m["embed"]) and not torch.equal(c["embed"], m["embed"])
    for l in range(2):
        for k in shapes:
            assert not torch.equal(o["layers"][l][k], m["layers"][l][k]) and torch.equal(c["layers"][l][k], m["layers"][l][k]), (l, k)
    # p = 0 sites are all ones (the oracle multiplies by them: a no-op)
    z = dm.decoder_masks(1, "fused", 2, 2, 3, 256, 4, 2048, 1, 0.0, 0.1)
    assert all(bool((t == 1).all()) for t in z["layers"][0].values()) and not bool((z["embed"] == 1).all())
    with pytest.raises(ValueError):
        dm.decoder_masks(1, "wide", 2, 2, 3, 256, 4, 2048, 1, 0.3, 0.1)
    with pytest.raises(ValueError):
        dm.decoder_masks(1, "fused", 2, 9, 3, 256, 4, 2048, 1, 0.3, 0.1)


def test_a_ragged_clip_draws_the_masks_of_its_batch_position():
    B, sy, d, H, d_ff, p, p_pos, seed = 5, 2, 256, 4, 2048, 0.3, 0.1, 77
    full = dm.decoder_masks(seed, "fused", B, sy, 180, d, H, d_ff, 2, p, p_pos)
    for b, S_b in enumerate((1, 45, 64, 65, 180)):
        clip = dm.decoder_ragged_clip_masks(seed, b, sy, S_b, d, H, d_ff, 2, p, p_pos)
        assert torch.equal(clip["embed"], full["embed"][b:b + 1])
        for l in range(2):
            for k, t in clip["layers"][l].items():
                want = full["layers"][l][k][b:b + 1]
                assert torch.equal(t, want[..., :S_b] if k == "cross" else want), (b, l, k)


def test_masks_none_is_todays_oracle_bit_for_bit():
    """g_decode(masks=None), and masks whose sites are all None, give the bits of the unmasked arithmetic (test_oracle_golden.py pins those)."""
    from oracle import translator_ref as tr
    case = gt.BY_ID["short-sy2-s45"]
    data = gt.case_data(case)
    sd = {k: v.double() for k, v in data["dsd"].items()}
    mem = data["mem"].double()
    a = tr.g_decode(sd, case.H, data["y"], mem)
    b = tr.g_decode(sd, case.H, data["y"], mem, masks={"embed": None, "layers": [None, {}]})
    assert torch.equal(a, b)
    ones = dm.decoder_masks(1, "fused", case.B, case.sy, case.S, case.d, case.H, gt.D_FF, gt.L, 0.0, 0.0)
    assert torch.equal(a, tr.g_decode(sd, case.H, data["y"], mem, masks=ones))


def test_the_gate_reports_what_it_is_given():
    case = gt.BY_ID["short-sy1-s1"]
    ref = _ref(case)
    same = gt.gate(ref, ref, gt.BF16_BAR)
    assert same["ok"] and same["miss"] == 0.0
    off = {"logits": ref["logits"] * 1.1, "dmem": ref["dmem"], "grads": dict(ref["grads"])}
    r = gt.gate(off, ref, gt.BF16_BAR)
    assert not r["ok"] and r["ratio"]["dmem"] == 0.0 and abs(r["logits"] - 0.1 * ref["logits"].abs().max().item() / max(1.0, ref["logits"].abs().max().item())) < 1e-12
    k = next(iter(ref["grads"]))
    nan = {"logits": ref["logits"], "dmem": ref["dmem"], "grads": {**ref["grads"], k: torch.full_like(ref["grads"][k], float("nan"))}}
    assert not gt.gate(nan, ref, gt.BF16_BAR)["ok"]
    missing = {"logits": ref["logits"], "dmem": ref["dmem"], "grads": {n: g for n, g in ref["grads"].items() if n != k}}
    with pytest.raises(AssertionError):
        gt.gate(missing, ref, gt.BF16_BAR)
    assert np.isfinite(same["grad"])
