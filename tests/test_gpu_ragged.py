"""-m gpu: ragged batches (egx_ragged_fwd, functional.encoder_ragged) — one inference forward over clips of their own lengths on the tiled
d = 128 kernels. Clip b's result must be the result of the same model on clip b ALONE, unpadded: that is what the reference computes in its
batch_size=1 validation loops (HHI/tasks/ttm/video_task_2loader.py:84-97, HHI/tasks/asd/video_task_taskspecific.py:69,76). Every parity
case is checked clip by clip against the fp64 oracle at the tiled path's tolerances (tests/test_gpu_tiled.py: logits 1e-3 f32s / 1e-2 bf16;
bf16 per-token rows 1e-2 in the L2 norm, 4e-2 element-wise).
The padded frames of every batch are NaN unless a test says otherwise: a kernel that reads one shows up at once."""
import numpy as np
import pytest
import torch

from oracle import translator_ref as tr
from tests.util import hhi_args, rel_err, seeded_feats, seeded_state_dict

pytestmark = pytest.mark.gpu
TOL = {"f32s": 1e-3, "bf16": 1e-2}
# per-token (ASD) rows: bf16 holds the 1e-2 bar in the L2 sense and 4e-2 element-wise, as in tests/test_gpu_tiled.py
TOL_ROWS = {"f32s": 1e-3, "bf16": 4e-2}


def _model(kind, L, compute, cuda, seed):
    from egot2_amd import hhi_asd, hhi_ttm
    cls = {"ttm3": hhi_ttm.TaskFusionMFTransformer3Task, "ttm2": hhi_ttm.TaskFusionMFTransformer2Task,
           "asd": hhi_asd.TaskFusionMFTransformer3Task}[kind]
    model = cls(hhi_args(num_layers=L))
    sd = seeded_state_dict(model, seed=seed)
    model.load_state_dict(sd)
    model = model.to(cuda).set_compute(compute).eval()
    sd64 = {k: v.double() for k, v in sd.items()}
    return model, sd64


def _clips(seed, tuples):
    """One feature tensor (T_k, 256) per segment of every clip, in argument order."""
    return [[f[0] for f in seeded_feats(seed + i, [(1, T, 256) for T in tup])] for i, tup in enumerate(tuples)]


def _pad(clips, cuda, fill=float("nan")):
    """Padded (B, T_max_k, 256) tensors per argument (padding = `fill`) and the (B, K) lengths."""
    K = len(clips[0])
    feats = []
    for k in range(K):
        Tm = max(c[k].shape[0] for c in clips)
        t = torch.full((len(clips), Tm, 256), fill, dtype=torch.float32)
        for b, c in enumerate(clips):
            t[b, :c[k].shape[0]] = c[k]
        feats.append(t.to(cuda))
    lengths = torch.tensor([[c[k].shape[0] for k in range(K)] for c in clips])
    return feats, lengths


def _rel(a, ref):
    return ((a.detach().double().cpu() - ref).abs() / ref.abs().clamp(min=1.0)).max().item()


def _mix(K, rng, n=40):
    """Length tuples (argument order) covering the tile edges of the tiled kernels, padded out with random ones, in random order."""
    if K == 3:
        edges = [(15, 15, 15), (16, 16, 16), (16, 16, 17), (32, 32, 32), (107, 107, 106), (107, 107, 107), (150, 150, 150), (1, 2, 3)]
    else:   # S = 30, 48, 49, 64, 96, 320, 321, 300
        edges = [(15, 15), (24, 24), (24, 25), (32, 32), (48, 48), (160, 160), (160, 161), (150, 150)]
    tups = edges + [tuple(int(x) for x in rng.integers(15, 151, K)) for _ in range(n - len(edges))]
    return [tups[i] for i in rng.permutation(len(tups))]


def _ragged(model, feats, lengths):
    with torch.no_grad():
        out = model.forward_features(*feats, lengths=lengths)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("compute", ["f32s", "bf16"])
@pytest.mark.parametrize("L", [1, 2])
@pytest.mark.parametrize("kind", ["ttm3", "ttm2"])
def test_ragged_ttm_vs_oracle_clip_by_clip(egx_lib, cuda, kind, L, compute):
    """S_b <= 48 (single tiles), 48 / 49, exactly two tiles, the f32s LDS chunk edge 320 / 321, 450, segments of ONE frame, and random
    per-segment lengths (T_ttm != T_lam != T_asd inside a clip): all in one batch of 40 clips in random order."""
    from egot2_amd import functional as F_egx
    K = 3 if kind == "ttm3" else 2
    model, sd64 = _model(kind, L, compute, cuda, seed=700 + K + L)
    tups = _mix(K, np.random.default_rng(K * 10 + L))
    clips = _clips(900 + L, tups)
    feats, lengths = _pad(clips, cuda)
    logits = _ragged(model, feats, lengths)
    assert F_egx.last_encoder_impl() == "ragged"
    assert tuple(logits.shape) == (len(clips), 2)
    for b, c in enumerate(clips):
        ref = tr.ttm_forward(sd64, 4, *[x[None].double() for x in c])
        err = _rel(logits[b:b + 1], ref)
        assert err < TOL[compute], (b, tups[b], err)


@pytest.mark.parametrize("compute", ["f32s", "bf16"])
def test_ragged_segments_of_different_lengths_inside_a_clip(egx_lib, cuda, compute):
    from egot2_amd import functional as F_egx
    model, sd64 = _model("ttm3", 1, compute, cuda, seed=731)
    tups = [(15, 90, 150), (150, 15, 40), (48, 1, 2), (100, 49, 1), (2, 150, 17)]
    clips = _clips(940, tups)
    feats, lengths = _pad(clips, cuda)
    logits = _ragged(model, feats, lengths)
    assert F_egx.last_encoder_impl() == "ragged"
    for b, c in enumerate(clips):
        assert _rel(logits[b:b + 1], tr.ttm_forward(sd64, 4, *[x[None].double() for x in c])) < TOL[compute], tups[b]


@pytest.mark.parametrize("compute", ["f32s", "bf16"])
@pytest.mark.parametrize("L", [1, 2])
def test_ragged_asd_rows_and_lossav_scores(egx_lib, cuda, compute, L):
    """ASD 3-task: the packed per-frame rows (sum_b T_asd_b, d) against tr.asd_forward per clip; lossAV's scores on the packed rows against
    the scores of the per-clip calls (the reference's batch_size=1 loop)."""
    from egot2_amd import functional as F_egx, hhi_asd
    model, sd64 = _model("asd", L, compute, cuda, seed=760 + L)
    tups = _mix(3, np.random.default_rng(77 + L), n=24)        # argument order (ttm, lam, asd)
    clips = _clips(980 + L, tups)
    feats, lengths = _pad(clips, cuda)
    rows = _ragged(model, feats, lengths)
    assert F_egx.last_encoder_impl() == "ragged"
    assert tuple(rows.shape) == (sum(t[2] for t in tups), 128)
    r0, refs = 0, []
    for b, c in enumerate(clips):
        refs.append(tr.asd_forward(sd64, 4, *[x[None].double() for x in c]))
        n = c[2].shape[0]
        assert _rel(rows[r0:r0 + n], refs[-1]) < TOL_ROWS[compute], (b, tups[b])
        r0 += n
    assert rel_err(rows, torch.cat(refs)) < TOL[compute]
    lossav = hhi_asd.lossAV(128).to(cuda)
    scores = lossav.forward(rows)
    with torch.no_grad():
        per_clip = np.concatenate([lossav.forward(model.forward_features(*[x[None].to(cuda) for x in c])) for c in clips])
    assert scores.shape == per_clip.shape
    assert np.abs(scores - per_clip).max() < TOL_ROWS[compute]


@pytest.mark.parametrize("kind", ["ttm3", "asd"])
def test_ragged_no_leakage_across_clips_or_padding(egx_lib, cuda, kind):
    """Huge values or NaN in the padded frames, and separately in every frame of clip j: every other clip's output is bit-identical."""
    model, _ = _model(kind, 2, "f32s", cuda, seed=790)
    tups = [(15, 15, 15), (150, 150, 150), (16, 16, 17), (60, 20, 107), (107, 107, 107), (33, 150, 2)]
    clips = _clips(1000, tups)
    base_feats, lengths = _pad(clips, cuda, fill=0.0)
    base = _ragged(model, base_feats, lengths)
    assert torch.isfinite(base).all()
    for fill in (1e30, float("nan"), -3e4):
        feats, _ = _pad(clips, cuda, fill=fill)
        assert torch.equal(_ragged(model, feats, lengths), base), fill
    rows = [t[2] for t in tups]         # ASD: rows per clip
    for j in range(len(clips)):
        feats = [f.clone() for f in base_feats]
        for f in feats:
            f[j] = float("nan")
        out = _ragged(model, feats, lengths)
        if kind == "asd":
            r0 = sum(rows[:j])
            keep = torch.ones(out.shape[0], dtype=torch.bool)
            keep[r0:r0 + rows[j]] = False
            assert torch.isnan(out[r0:r0 + rows[j]]).all()
        else:
            keep = torch.ones(out.shape[0], dtype=torch.bool)
            keep[j] = False
            assert torch.isnan(out[j]).all()
        assert torch.equal(out[keep.to(cuda)], base[keep.to(cuda)]), j


@pytest.mark.parametrize("kind", ["ttm3", "asd"])
def test_ragged_permuting_the_clips_permutes_the_outputs(egx_lib, cuda, kind):
    model, _ = _model(kind, 1, "f32s", cuda, seed=800)
    tups = _mix(3, np.random.default_rng(8), n=16)
    clips = _clips(1100, tups)
    feats, lengths = _pad(clips, cuda)
    out = _ragged(model, feats, lengths)
    perm = np.random.default_rng(9).permutation(len(clips))
    pf, pl = _pad([clips[i] for i in perm], cuda)
    pout = _ragged(model, pf, pl)
    if kind == "asd":
        r0 = np.concatenate([[0], np.cumsum([t[2] for t in tups])])
        out = torch.cat([out[r0[i]:r0[i + 1]] for i in perm])
    else:
        out = out[torch.as_tensor(perm, device=cuda)]
    assert torch.equal(pout, out)


def test_ragged_uniform_batch_equals_the_batched_forward(egx_lib, cuda):
    """Every clip at the padded length (S = 180, the tiled path of forward_features): the same kernels, tiles, attention chunking and
    pooled-head arithmetic per clip, but NOT bit-identical: the batched forward staggers the FFN hidden-block walk by the tile's place in
    the grid, the ragged one starts every tile at block 0 (so that a clip's result does not depend on its place in the batch), and the
    FFN output is summed in another order. Within 1e-6."""
    model, _ = _model("ttm3", 2, "f32s", cuda, seed=810)
    feats = [f.to(cuda) for f in seeded_feats(1200, [(12, 60, 256)] * 3)]
    with torch.no_grad():
        uni = model.forward_features(*feats)
    from egot2_amd import functional as F_egx
    assert F_egx.last_encoder_impl() == "tiled"
    rag = _ragged(model, feats, [60] * 12)
    assert F_egx.last_encoder_impl() == "ragged"
    assert (rag - uni).abs().max().item() <= 1e-6


@pytest.mark.parametrize("kind", ["ttm3", "asd"])
def test_ragged_matches_each_clip_alone_through_the_existing_path(egx_lib, cuda, kind):
    """B = 1 calls of forward_features without lengths (per-clip kernels for S <= 48, tiled above): within 1e-5 (f32s)."""
    model, _ = _model(kind, 1, "f32s", cuda, seed=820)
    tups = _mix(3, np.random.default_rng(12), n=14)
    clips = _clips(1300, tups)
    feats, lengths = _pad(clips, cuda)
    out = _ragged(model, feats, lengths)
    with torch.no_grad():
        alone = torch.cat([model.forward_features(*[x[None].to(cuda) for x in c]) for c in clips])
    assert out.shape == alone.shape
    assert (out - alone).abs().max().item() <= 1e-5


def test_ragged_with_a_frozen_weight_cache(egx_lib, cuda):
    """Two consecutive ragged calls with different length sets under enable_weight_cache(frozen=True): the second skips the packing launch
    and both give what the calls without the cache give."""
    model, _ = _model("ttm3", 2, "f32s", cuda, seed=830)
    sets = [_mix(3, np.random.default_rng(20), n=12), _mix(3, np.random.default_rng(21), n=20)]
    batches = [_pad(_clips(1400 + i, t), cuda) for i, t in enumerate(sets)]
    plain = [_ragged(model, f, l) for f, l in batches]
    model.enable_weight_cache(frozen=True)
    cached = [_ragged(model, f, l) for f, l in batches]
    wc = model._egx_wcache
    assert wc.packs == 1 and wc.hits == 1, (wc.packs, wc.hits)
    for a, b in zip(plain, cached):
        assert torch.equal(a, b)
    model.disable_weight_cache()


@pytest.mark.parametrize("case", ["f32", "long_clip"])
def test_ragged_grouped_fallback(egx_lib, cuda, case):
    """Configurations outside the ragged kernels fall back to one batched forward per length group: exact fp32 (set_compute("f32")), and
    a batch with a clip of S_b = 550 > 512 tokens."""
    from egot2_amd import functional as F_egx
    compute = "f32" if case == "f32" else "f32s"
    model, sd64 = _model("ttm3", 1, compute, cuda, seed=840)
    tups = [(15, 15, 15), (60, 60, 60), (15, 15, 15), (20, 30, 40)] + ([(200, 200, 150)] if case == "long_clip" else [])
    clips = _clips(1500, tups)
    feats, lengths = _pad(clips, cuda)
    logits = _ragged(model, feats, lengths)
    assert F_egx.last_encoder_impl() == "grouped"
    for b, c in enumerate(clips):
        assert _rel(logits[b:b + 1], tr.ttm_forward(sd64, 4, *[x[None].double() for x in c])) < 1e-3, tups[b]
    amodel, asd64 = _model("asd", 1, compute, cuda, seed=841)
    rows = _ragged(amodel, feats, lengths)
    assert F_egx.last_encoder_impl() == "grouped"
    ref = torch.cat([tr.asd_forward(asd64, 4, *[x[None].double() for x in c]) for c in clips])
    assert _rel(rows, ref) < 1e-3


def test_ragged_refusals(egx_lib, cuda):
    from egot2_amd import hhi_asd
    model, _ = _model("ttm3", 1, "f32s", cuda, seed=850)
    clips = _clips(1600, [(15, 15, 15), (30, 20, 10)])
    feats, lengths = _pad(clips, cuda, fill=0.0)
    with pytest.raises(ValueError, match="inference-only"):
        model.train().forward_features(*feats, lengths=lengths)
    model.eval()
    with pytest.raises(ValueError, match="inference-only"):
        model.forward_features(*feats, lengths=lengths)                       # grad enabled
    with torch.no_grad():
        with pytest.raises(ValueError, match="inference-only"):
            model.forward_features(*feats, target=torch.zeros(2, dtype=torch.long, device=cuda), lengths=lengths)
        with pytest.raises(ValueError, match="1 .. 20"):
            model.forward_features(*feats, lengths=[[15, 15, 15], [30, 0, 10]])
        with pytest.raises(ValueError, match="1 .. 30"):
            model.forward_features(*feats, lengths=[15, 31])
        amodel, _ = _model("asd", 1, "f32s", cuda, seed=851)
        with pytest.raises(ValueError, match="inference-only"):
            amodel.forward_features(*feats, lossav=hhi_asd.lossAV(128).to(cuda), labels=torch.zeros(25, dtype=torch.long, device=cuda),
                                    lengths=lengths)
