"""-m gpu: ragged training batches (egx_ragged_train_fwd / egx_ragged_bwd, forward_features_ragged): one forward + backward over clips of
their own lengths, every clip keeping all of its frames. The oracle is built per clip on the UNPADDED clip (oracle/translator_ref.py, fp64),
the clips' logits concatenated and the weighted cross entropy taken over the batch. Tolerances are those of tests/test_gpu_tiled.py: logits
1e-3 / 1e-2 and every gradient 1e-2 / 8e-2 relative, for f32s / bf16. Train-mode cases use the masks the ragged kernels draw, restated
by tests/dropmask.py ragged_clip_masks with the ragged keying (row tok0_b + s; attention row 4 tok0_b + h S_b + query).
The padded frames of every batch are NaN unless a test says otherwise: a kernel that reads one shows up at once."""
import numpy as np
import pytest
import torch

from oracle import translator_ref as tr
from tests.dropmask import ragged_clip_masks
from tests.util import hhi_args, max_err, rel_err, seeded_feats, seeded_state_dict

pytestmark = pytest.mark.gpu
CE_W = [0.266, 0.734]
TOL = {"f32s": (1e-3, 1e-2), "bf16": (1e-2, 8e-2)}
EDGES3 = [(10, 10, 10), (15, 15, 15), (16, 16, 16), (16, 16, 17), (32, 32, 32), (32, 32, 33), (107, 107, 107), (150, 150, 150),
          (170, 170, 172), (15, 90, 150), (48, 1, 2), (100, 49, 1)]            # S_b = 30 45 48 49 96 97 321 450 512 255 51 150
EDGES2 = [(15, 15), (22, 23), (24, 24), (24, 25), (48, 48), (48, 49), (160, 161), (225, 225), (256, 256), (1, 150), (90, 7)]


def _model(kind, L, compute, cuda, seed, p=0.1):
    from egot2_amd import hhi_asd, hhi_ttm
    cls = {"ttm3": hhi_ttm.TaskFusionMFTransformer3Task, "ttm2": hhi_ttm.TaskFusionMFTransformer2Task,
           "asd": hhi_asd.TaskFusionMFTransformer3Task}[kind]
    model = cls(hhi_args(num_layers=L, dropout=p))
    sd = seeded_state_dict(model, seed=seed)
    model.load_state_dict(sd)
    model = model.to(cuda).set_compute(compute).train()
    model.pos_embed.dropout.p = 0.1 if p > 0 else 0.0
    return model, sd


def _sd64(sd):
    return {k: v.double().requires_grad_(v.is_floating_point() and not k.endswith(".pe")) for k, v in sd.items()}


def _clips(seed, tuples):
    """One (T_k, 256) feature per segment of every clip, in argument order."""
    return [[f[0] for f in seeded_feats(seed + i, [(1, T, 256) for T in tup])] for i, tup in enumerate(tuples)]


def _pad(clips, cuda, fill=float("nan"), grad=False):
    K = len(clips[0])
    feats = []
    for k in range(K):
        Tm = max(c[k].shape[0] for c in clips)
        t = torch.full((len(clips), Tm, 256), fill, dtype=torch.float32)
        for b, c in enumerate(clips):
            t[b, :c[k].shape[0]] = c[k]
        feats.append(t.to(cuda).requires_grad_(grad))
    return feats, torch.tensor([[c[k].shape[0] for k in range(K)] for c in clips])


def _oracle_ttm(sd, clips, target, L=1, seed=0, p=0.0, p_pos=0.0):
    """fp64 logits of every clip alone (masks keyed as the ragged batch keys them), the weighted CE over the batch, backward."""
    sd64 = _sd64(sd)
    xs = [[x.double().requires_grad_(True) for x in c] for c in clips]
    outs, tok0 = [], 0
    for c in xs:
        S = sum(x.shape[0] for x in c)
        masks = ragged_clip_masks(seed, tok0, S, L, p, p_pos) if (p > 0 or p_pos > 0) else None
        outs.append(tr.ttm_forward(sd64, 4, *[x[None] for x in c], masks=masks))
        tok0 += S
    logits = torch.cat(outs, 0)
    loss = tr.weighted_ce(logits, target, CE_W)
    loss.backward()
    return logits.detach(), loss.detach(), sd64, xs


def _check_grads(model, sd64, tol, skip=()):
    n = 0
    for name, prm in model.named_parameters():
        if name in skip or not prm.requires_grad or name not in sd64 or sd64[name].grad is None:
            continue
        assert prm.grad is not None, name
        e = rel_err(prm.grad, sd64[name].grad)
        assert e < tol, (name, e)
        n += 1
    assert n >= 20


def _run(model, feats, lengths, target, cuda):
    logits, loss = model.forward_features_ragged(*feats, lengths=lengths, target=target.to(cuda),
                                                 class_weight=torch.tensor(CE_W, device=cuda))
    loss.backward()
    torch.cuda.synchronize()
    return logits, loss


@pytest.mark.parametrize("compute", ["f32s", "bf16"])
@pytest.mark.parametrize("L", [1, 2])
@pytest.mark.parametrize("kind", ["ttm3", "ttm2"])
def test_ragged_train_vs_oracle(egx_lib, cuda, kind, L, compute):
    """Logits, loss, every parameter gradient and d(feature) against the per-clip fp64 oracle at p = 0: single-tile clips (30, 45, 48),
    the tile edges 49 / 96 / 97, the f32s LDS chunk edge 321, 450, 512, and segments of very different lengths inside a clip."""
    from egot2_amd import functional as F_egx
    tups = EDGES3 if kind == "ttm3" else EDGES2
    model, sd = _model(kind, L, compute, cuda, seed=800 + L + len(tups[0]), p=0.0)
    clips = _clips(1000 + L, tups)
    feats, lengths = _pad(clips, cuda, grad=True)
    target = torch.from_numpy(np.random.default_rng(L).integers(0, 2, len(clips))).long()
    logits, loss = _run(model, feats, lengths, target, cuda)
    assert F_egx.last_encoder_impl() == "ragged"
    ref, ref_loss, sd64, xs = _oracle_ttm(sd, clips, target, L)
    tl, tg = TOL[compute]
    assert max_err(logits, ref) < tl
    assert abs(loss.item() - ref_loss.item()) < tl
    _check_grads(model, sd64, tg)
    for k, f in enumerate(feats):
        for b, c in enumerate(xs):
            T = c[k].shape[0]
            assert rel_err(f.grad[b, :T], c[k].grad) < tg, (k, b)
            assert torch.all(f.grad[b, T:] == 0), (k, b)


@pytest.mark.parametrize("compute", ["f32s", "bf16"])
def test_ragged_train_mode_masks_vs_oracle(egx_lib, cuda, compute):
    """p = 0.5 + 0.1 positional dropout under the restated ragged keying."""
    model, sd = _model("ttm3", 1, compute, cuda, seed=831, p=0.5)
    seed = 0x5EED0123
    model._egx_seed = lambda: seed
    tups = [(15, 15, 15), (40, 41, 42), (16, 16, 17), (150, 150, 150), (5, 60, 33)]
    clips = _clips(1100, tups)
    feats, lengths = _pad(clips, cuda)
    target = torch.tensor([0, 1, 1, 0, 1])
    logits, loss = _run(model, feats, lengths, target, cuda)
    ref, ref_loss, sd64, _ = _oracle_ttm(sd, clips, target, 1, seed, 0.5, 0.1)
    tl, tg = TOL[compute]
    assert max_err(logits, ref) < tl
    _check_grads(model, sd64, tg)


@pytest.mark.parametrize("compute", ["f32s", "bf16"])
def test_ragged_train_asd_rows_and_lossav(egx_lib, cuda, compute):
    """ASD: the packed per-frame rows against tr.asd_forward per clip, and lossAV (Python module) on them, backward to every parameter."""
    from egot2_amd import hhi_asd
    model, sd = _model("asd", 1, compute, cuda, seed=861, p=0.0)
    tups = [(15, 15, 15), (30, 20, 10), (150, 150, 150), (16, 16, 17), (1, 2, 160)]      # argument order (ttm, lam, asd)
    clips = _clips(1200, tups)
    feats, lengths = _pad(clips, cuda)
    lossav = hhi_asd.lossAV(128).to(cuda)
    labels = torch.from_numpy(np.random.default_rng(3).integers(0, 2, sum(t[2] for t in tups))).long()
    rows = model.forward_features_ragged(*feats, lengths=lengths)
    assert tuple(rows.shape) == (sum(t[2] for t in tups), 128)
    nloss, _, _, _ = lossav(rows, labels.to(cuda))
    nloss.backward()
    torch.cuda.synchronize()
    sd64 = _sd64(sd)
    fc_w = lossav.FC.weight.detach().double().cpu().requires_grad_(True)
    fc_b = lossav.FC.bias.detach().double().cpu().requires_grad_(True)
    ref = torch.cat([tr.asd_forward(sd64, 4, *[x[None].double() for x in c]) for c in clips], 0)
    ref_loss = torch.nn.functional.cross_entropy(ref @ fc_w.t() + fc_b, labels, weight=torch.tensor([1.0, 4.0], dtype=torch.float64))
    ref_loss.backward()
    tl, tg = TOL[compute]
    assert rel_err(rows, ref.detach()) < tl * (4 if compute == "bf16" else 1)
    assert abs(nloss.item() - ref_loss.item()) < tl
    assert rel_err(lossav.FC.weight.grad, fc_w.grad) < tg
    _check_grads(model, sd64, tg, skip=("linear_head.0.weight", "linear_head.0.bias", "linear_head.1.weight", "linear_head.1.bias"))


@pytest.mark.parametrize("compute", ["f32s", "bf16"])
def test_ragged_equal_clips_match_the_tiled_training_call(egx_lib, cuda, compute):
    """Clips of equal S = 60 > 48 in train mode with the same host seed draw the tiled call's masks: same logits and gradients."""
    model, sd = _model("ttm3", 1, compute, cuda, seed=871, p=0.5)
    model._egx_seed = lambda: 0xABCDEF
    feats = [f.to(cuda) for f in seeded_feats(1300, [(5, 20, 256)] * 3)]
    target = torch.tensor([0, 1, 1, 0, 1], device=cuda)
    w = torch.tensor(CE_W, device=cuda)
    from egot2_amd import functional as F_egx
    lt = model.forward_features(*feats)
    assert F_egx.last_encoder_impl() == "tiled"
    torch.nn.functional.cross_entropy(lt, target, weight=w).backward()
    g_t = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    model.zero_grad(set_to_none=True)
    lr = model.forward_features_ragged(*feats, lengths=[20] * 5)
    torch.nn.functional.cross_entropy(lr, target, weight=w).backward()
    torch.cuda.synchronize()
    assert max_err(lr, lt) <= 1e-6
    for n, g in g_t.items():
        assert rel_err(dict(model.named_parameters())[n].grad, g) <= 1e-5, n


def test_ragged_train_no_leakage(egx_lib, cuda):
    """NaN padding changes nothing (bit for bit), padded frames get exactly zero gradient, one clip's loss reaches only its own features."""
    model, _ = _model("ttm3", 1, "f32s", cuda, seed=881, p=0.0)
    tups = [(15, 15, 15), (100, 30, 77), (16, 16, 17), (49, 49, 49)]
    clips = _clips(1400, tups)
    res = []
    for fill in (float("nan"), 0.0):
        feats, lengths = _pad(clips, cuda, fill=fill, grad=True)
        model.zero_grad(set_to_none=True)
        logits = model.forward_features_ragged(*feats, lengths=lengths)
        (logits * torch.arange(1.0, 9.0, device=cuda).view(4, 2)).sum().backward()
        torch.cuda.synchronize()
        res.append((logits.detach().clone(), [f.grad.clone() for f in feats], {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}))
    (l0, f0, g0), (l1, f1, g1) = res
    assert torch.equal(l0, l1)
    for a, b in zip(f0, f1):
        assert torch.equal(a, b)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
    for k, f in enumerate(f0):
        for b, t in enumerate(tups):
            assert torch.all(f[b, t[k]:] == 0)
    feats, lengths = _pad(clips, cuda, grad=True)
    logits = model.forward_features_ragged(*feats, lengths=lengths)
    logits[1].sum().backward()
    torch.cuda.synchronize()
    for f in feats:
        assert torch.all(f.grad[[0, 2, 3]] == 0) and f.grad[1].abs().sum() > 0


def test_ragged_train_permutation_and_determinism(egx_lib, cuda):
    model, _ = _model("ttm3", 2, "f32s", cuda, seed=891, p=0.0)
    tups = [(15, 15, 15), (100, 30, 77), (16, 16, 17), (150, 150, 150), (3, 4, 5), (49, 49, 49)]
    clips = _clips(1500, tups)
    up = torch.from_numpy(np.random.default_rng(5).standard_normal((len(clips), 2), dtype=np.float32)).to(cuda)

    def run(order):
        cs = [clips[i] for i in order]
        feats, lengths = _pad(cs, cuda, grad=True)
        model.zero_grad(set_to_none=True)
        logits = model.forward_features_ragged(*feats, lengths=lengths)
        (logits * up[order]).sum().backward()
        torch.cuda.synchronize()
        return logits.detach(), [f.grad for f in feats], {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}

    ident = list(range(len(clips)))
    l0, f0, g0 = run(ident)
    l0b, f0b, g0b = run(ident)
    for n in g0:                        # determinism: the same batch twice, bit for bit
        assert torch.equal(g0[n], g0b[n]), n
    assert torch.equal(l0, l0b)
    perm = [4, 2, 0, 5, 3, 1]
    l1, f1, g1 = run(perm)
    assert torch.equal(l1, l0[perm])
    for k in range(3):
        for j, b in enumerate(perm):
            T = tups[b][k]
            assert torch.equal(f1[k][j, :T], f0[k][b, :T]), (k, b)
    for n in g0:
        assert rel_err(g1[n], g0[n]) <= 1e-6, n


def test_ragged_train_fused_adam_step_matches_per_clip_loss(egx_lib, cuda):
    """One FusedAdam step on a ragged batch equals one step whose loss is built from per-clip forward_features calls (the same weighted CE
    over the concatenated logits)."""
    from egot2_amd.train import FusedAdam
    tups = [(15, 15, 15), (60, 61, 62), (16, 16, 17), (120, 100, 80)]
    clips = _clips(1600, tups)
    target = torch.tensor([1, 0, 1, 1], device=cuda)
    w = torch.tensor(CE_W, device=cuda)
    after = []
    for ragged in (True, False):
        model, _ = _model("ttm3", 1, "f32s", cuda, seed=901, p=0.0)
        opt = FusedAdam(model.parameters(), lr=1e-3)
        if ragged:
            feats, lengths = _pad(clips, cuda)
            logits = model.forward_features_ragged(*feats, lengths=lengths)
        else:
            logits = torch.cat([model.forward_features(*[x[None].to(cuda) for x in c]) for c in clips], 0)
        torch.nn.functional.cross_entropy(logits, target, weight=w).backward()
        grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
        opt.step()
        torch.cuda.synchronize()
        after.append((grads, {n: p.detach().clone() for n, p in model.named_parameters()}))
    (g0, p0), (g1, p1) = after
    assert set(g0) == set(g1) and len(g0) >= 20
    for n in g0:
        assert rel_err(g0[n], g1[n]) < 1e-2, n
    for n in p0:                    # (a first Adam step moves every weight by ~lr: the parameters agree far below that)
        assert rel_err(p0[n], p1[n]) < 1e-3, n


@pytest.mark.parametrize("case", ["f32", "s513"])
def test_ragged_train_grouped_fallback(egx_lib, cuda, case):
    from egot2_amd import functional as F_egx
    model, sd = _model("ttm3", 1, "f32s", cuda, seed=911, p=0.0)
    tups = [(15, 15, 15), (40, 41, 42), (15, 15, 15)]
    if case == "f32":
        model.set_compute("f32")
    else:
        tups.append((171, 171, 171))                # S = 513: beyond the ragged kernels
    clips = _clips(1700, tups)
    feats, lengths = _pad(clips, cuda)
    target = torch.tensor([0, 1, 1, 0][:len(tups)])
    logits, loss = _run(model, feats, lengths, target, cuda)
    assert F_egx.last_encoder_impl() == "grouped"
    ref, ref_loss, sd64, _ = _oracle_ttm(sd, clips, target, 1)
    assert max_err(logits, ref) < 1e-3
    assert abs(loss.item() - ref_loss.item()) < 1e-3
    _check_grads(model, sd64, 1e-2)


def test_ragged_train_weight_cache_between_forward_and_backward(egx_lib, cuda):
    """A re-packing eval forward between a ragged training forward and its backward leaves the gradients exactly as without it."""
    tups = [(15, 15, 15), (60, 61, 62), (16, 16, 17)]
    clips = _clips(1800, tups)
    grads = []
    for interleave in (False, True):
        model, _ = _model("ttm3", 1, "f32s", cuda, seed=921, p=0.5)
        model.enable_weight_cache()
        model._egx_seed = lambda: 77
        feats, lengths = _pad(clips, cuda)
        logits = model.forward_features_ragged(*feats, lengths=lengths)
        if interleave:
            model.eval()
            with torch.no_grad():
                model.forward_features(*[f.to(cuda) for f in seeded_feats(5, [(4, 15, 256)] * 3)])     # packs p = 0 copies into the cache
            model.train()
        logits.sum().backward()
        torch.cuda.synchronize()
        grads.append({n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
    for n in grads[0]:
        assert torch.equal(grads[0][n], grads[1][n]), n


def test_ragged_train_device_seed_and_host_seed(egx_lib, cuda):
    model, _ = _model("ttm3", 1, "f32s", cuda, seed=931, p=0.5)
    clips = _clips(1900, [(15, 15, 15), (60, 61, 62)])
    feats, lengths = _pad(clips, cuda)
    model._egx_seed = lambda: 99
    a = model.forward_features_ragged(*feats, lengths=lengths).detach()
    b = model.forward_features_ragged(*feats, lengths=lengths).detach()
    assert torch.equal(a, b)                        # the host seed is reproducible
    model.enable_device_seed()
    c = model.forward_features_ragged(*feats, lengths=lengths).detach()
    d = model.forward_features_ragged(*feats, lengths=lengths).detach()
    torch.cuda.synchronize()
    assert not torch.equal(c, d)                    # the device seed advances: fresh masks per call


@pytest.mark.parametrize("compute", ["f32s", "bf16"])
@pytest.mark.parametrize("kind", ["ttm3", "asd"])
def test_ragged_inference_call_matches_the_training_call_in_eval(egx_lib, cuda, kind, compute):
    """Eval mode under no_grad: forward_features(lengths=) (egx_ragged_fwd, filling then hitting the weight cache) and forward_features_ragged
    (egx_ragged_train_fwd with training = 0) run one forward body: bit-identical logits (ttm3, with the head) or rows (asd, head-less)."""
    from egot2_amd import functional as F_egx
    model, _ = _model(kind, 2, compute, cuda, seed=941)
    model.enable_weight_cache().eval()
    feats, lengths = _pad(_clips(1950, [(15, 15, 15), (60, 61, 62), (16, 16, 17), (150, 150, 150), (1, 2, 160)]), cuda)
    with torch.no_grad():
        outs = []
        for _ in range(2):
            outs.append(model.forward_features(*feats, lengths=lengths))
            assert F_egx.last_encoder_impl() == "ragged"
        assert model._egx_wcache.packs == 1 and model._egx_wcache.hits == 1
        outs.append(model.forward_features_ragged(*feats, lengths=lengths))
        assert F_egx.last_encoder_impl() == "ragged"
    torch.cuda.synchronize()
    assert not torch.isnan(outs[0]).any()
    for o in outs[1:]:
        assert torch.equal(o, outs[0])
