"""-m gpu: ragged-batch TRAINING of the EgoT2-g HHI model (egx_ragged_encode_train_fwd / egx_ragged_encode_bwd on the wide bf16 path,
egx_decoder_ragged_train_fwd / egx_decoder_ragged_bwd): one encoder and one decoder forward + backward per batch of clips of their own
lengths, for the training step of HHI/tasks/multitask/video_tasktranslation.py:39-66, which the reference can only feed same-length
mini-batches (:144-156). Padded frames are NaN unless stated, no clip is left out of any comparison. Parity against the oracle is asserted
here at p = 0, and the masks are pinned through the uniform training call (equal lengths reproduce it bit for bit); under p > 0 the wide
encoder's masks are held to the oracle's by test_gpu_dropout_parity.py, the decoder's (uniform and ragged, clip by clip) by
test_gpu_decoder_dropout.py. Bounds
are the project's for this model in bf16 (test_gpu_parity_hygiene.py, test_gpu_ragged_g.py): memory 1e-2 and logits 1.5e-2 (asd logits 4e-2)
relative to max(1, |ref|); per-parameter gradient error < 1.5e-1 for the 3 + 3-layer stack, fc.weight < 2e-2."""
import numpy as np
import pytest
import torch

from tests.test_gpu_ragged_g import TTM_LENGTHS, T_PAD, _bound, _feats, _lengths
from tests.util import hhi_args, seeded_state_dict

pytestmark = pytest.mark.gpu

GRAD_TOL, FC_TOL = 1.5e-1, 2e-2


def _model(cuda, compute="bf16", p=0.0, seed=31):
    from egot2_amd import hhi_multitask
    from egot2_amd.synth import HHI_G_VOCAB
    m = hhi_multitask.TaskTranslationPromptTransformer(hhi_args(hidden_dim=256, num_heads=4, num_layers=3, dropout=p), HHI_G_VOCAB)
    sd = seeded_state_dict(m, seed)
    m.load_state_dict(sd)
    m.pos_embed.dropout.p = p
    m = m.to(cuda).set_compute(compute).train()
    return m, sd


def _targets(n, task, vocab, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.full((n,), vocab[task]), torch.randint(5, 7, (n,), generator=g)], dim=1)


def _lin(t, w=None):
    """A fixed linear functional of all logits."""
    w = torch.linspace(-1, 1, t.numel(), dtype=t.dtype, device=t.device).view_as(t) if w is None else w
    return (t * w).sum()


def _step(m, task, fd, lengths, y, *, step0=0, weight=None, clips=None):
    """One ragged training forward + backward with the dropout counter at `step0`; returns (memory, logits (sy, B, V), gradients, d_memory)."""
    from egot2_amd import functional as F_egx
    m.zero_grad(set_to_none=True)
    m._egx_step = step0
    lens = torch.as_tensor(lengths)
    mem = m.encode_features_ragged(task, *fd, lengths=lens)
    mem.retain_grad()
    if task == "asd":
        logits = m.decode(y, mem)
    else:
        logits = m.decode_ragged(y, mem, F_egx.ragged_lengths(lens, len(lengths), [f.shape[1] for f in fd]).sum(1))
    sel = logits if clips is None else logits[:, clips].contiguous()
    _lin(sel, weight).backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
    return mem.detach(), logits.detach(), grads, mem.grad.detach().clone()


def _grad_errs(grads, ref):
    return {k: ((grads[k].cpu().double() - v).norm() / (v.norm() + 1e-12)).item() for k, v in ref.items() if k in grads and v.norm() > 0}


def _check_grads(grads, ref, tol=GRAD_TOL, fc_tol=FC_TOL, n_min=40):
    errs = _grad_errs(grads, ref)
    worst = max(errs, key=errs.get)
    print(f"gradients: {len(errs)} tensors, worst {worst} {errs[worst]:.3e}, fc.weight {errs.get('fc.weight', float('nan')):.3e}")
    bad = {k: e for k, e in errs.items() if not e < tol}
    assert len(errs) > n_min and not bad, bad
    assert errs["fc.weight"] < fc_tol, errs["fc.weight"]
    return errs


def _oracle_clipwise(sd, task, feats, lengths, y, w, vocab):
    """fp64 oracle clip by clip on the unpadded frames, gradients accumulated over the clips. y / w: per target row ('asd': per frame)."""
    from oracle import translator_ref as tr
    sd64 = {k: v.double().requires_grad_(v.is_floating_point() and not k.endswith(".pe")) for k, v in sd.items()}
    mems, logs, r0 = [], [], 0
    for b, row in enumerate(lengths):
        fs = [f[b:b + 1, :T].double() for f, T in zip(feats, row)]
        rmem = tr.hhi_g_encode(sd64, 4, task, *fs)
        n = rmem.shape[1]                              # 1 clip, or T_b frames for 'asd'
        rlog = tr.g_decode(sd64, 4, y[r0:r0 + n], rmem)
        (rlog * w[:, r0:r0 + n]).sum().backward()
        mems.append(rmem.detach())
        logs.append(rlog.detach())
        r0 += n
    return mems, logs, {k: v.grad for k, v in sd64.items() if v.requires_grad and v.grad is not None}


def _weights(sy, n, V):
    return torch.linspace(-1, 1, sy * n * V, dtype=torch.float64).view(sy, n, V)


def test_ttm_training_matches_the_oracle_clip_by_clip(egx_lib, cuda):
    from egot2_amd import functional as F_egx
    m, sd = _model(cuda)
    lengths = _lengths(24, 5)                    # the 16 edge lengths + 24 random ones, shuffled
    assert len(lengths) == 40 and set(TTM_LENGTHS) <= set(lengths)
    feats = _feats(lengths, 6)
    B, V = len(lengths), len(m.vocab)
    y = _targets(B, "ttm", m.vocab, 4)
    w = _weights(2, B, V)
    mem, logits, grads, _ = _step(m, "ttm", [f.to(cuda) for f in feats], lengths, y.to(cuda), weight=w.float().to(cuda))
    assert F_egx.last_encoder_impl() == "ragged" and F_egx.last_decoder_impl() == "ragged"
    assert torch.isfinite(mem).all() and torch.isfinite(logits).all()
    rmems, rlogs, rgrads = _oracle_clipwise(sd, "ttm", feats, lengths, y, w, m.vocab)
    r0 = 0
    for b, row in enumerate(lengths):
        S = sum(row)
        _bound(mem[r0:r0 + S], rmems[b][:, 0], 1e-2)
        _bound(logits[:, b], rlogs[b][:, 0], 1.5e-2)
        r0 += S
    _check_grads(grads, rgrads)


def test_asd_and_lam_training_match_the_oracle(egx_lib, cuda):
    from egot2_amd import functional as F_egx
    m, sd = _model(cuda)
    V = len(m.vocab)
    # asd: equal segment lengths per clip, the frame-major memory and the S = 3 decoder over sum_b T_b frames
    T = [1, 3, 15, 40, 64, 100, 150, 7]
    lengths = [(t, t, t) for t in T]
    feats = _feats(lengths, 8)
    n = sum(T)
    y = _targets(n, "asd", m.vocab, 5)
    w = _weights(2, n, V)
    mem, logits, grads, _ = _step(m, "asd", [f.to(cuda) for f in feats], T, y.to(cuda), weight=w.float().to(cuda))
    assert F_egx.last_encoder_impl() == "ragged" and mem.shape == (3, n, 256) and logits.shape == (2, n, V)
    rmems, rlogs, rgrads = _oracle_clipwise(sd, "asd", feats, lengths, y, w, m.vocab)
    f0 = 0
    for b, t in enumerate(T):
        _bound(mem[:, f0:f0 + t], rmems[b], 1e-2)
        _bound(logits[:, f0:f0 + t], rlogs[b], 4e-2)       # (the asd decode's bound in test_gpu_ragged_g.py / test_gpu_decoder.py)
        f0 += t
    _check_grads(grads, rgrads)
    # lam: one segment
    TL = [1, 20, 64, 65, 129, 150, 33]
    lam = _feats([(t,) for t in TL], 9, n_seg=1)
    y = _targets(len(TL), "lam", m.vocab, 6)
    w = _weights(2, len(TL), V)
    mem, logits, grads, _ = _step(m, "lam", [lam[0].to(cuda)], TL, y.to(cuda), weight=w.float().to(cuda))
    assert F_egx.last_encoder_impl() == "ragged" and F_egx.last_decoder_impl() == "ragged"
    rmems, rlogs, rgrads = _oracle_clipwise(sd, "lam", lam, [(t,) for t in TL], y, w, m.vocab)
    r0 = 0
    for b, t in enumerate(TL):
        _bound(mem[r0:r0 + t], rmems[b][:, 0], 1e-2)
        _bound(logits[:, b], rlogs[b][:, 0], 1.5e-2)
        r0 += t
    _check_grads(grads, rgrads)


@pytest.mark.parametrize("T", [15, 60])
def test_equal_lengths_reproduce_the_uniform_training_call_bit_for_bit(egx_lib, cuda, T):
    """T = 15: S = 45, the short attention class; T = 60: S = 180, the long class (dropout row stride 512). Same host seed, p_drop = p_pos =
    0.1: memory, logits and every gradient equal the uniform training call's. This pins the dropout masks of the ragged kernels to the uniform
    path's, which are held against the oracle's: the wide encoder's by test_gpu_dropout_parity.py (tests/dropmask.py encoder_masks), the
    fused decoder's by test_gpu_decoder_dropout.py (decoder_masks; its ragged case also compares mixed lengths clip by clip)."""
    from egot2_amd import functional as F_egx
    m, _ = _model(cuda, p=0.1)
    B = 16
    feats = _feats([(T, T, T)] * B, 41)
    fd = [f[:, :T].contiguous().to(cuda) for f in feats]
    y = _targets(B, "ttm", m.vocab, 7).to(cuda)
    mem_r, log_r, g_r, dmem_r = _step(m, "ttm", fd, [T] * B, y)
    assert F_egx.last_encoder_impl() == "ragged" and F_egx.last_decoder_impl() == "ragged"
    m.zero_grad(set_to_none=True)
    m._egx_step = 0
    mem_u = m.encode_features("ttm", *fd)                         # (S, B, d)
    mem_u.retain_grad()
    log_u = m.decode(y, mem_u)
    assert F_egx.last_encoder_impl() == "wide" and F_egx.last_decoder_impl() == "fused"
    _lin(log_u).backward()
    torch.cuda.synchronize()
    assert torch.equal(mem_r, mem_u.detach().permute(1, 0, 2).reshape(-1, 256))
    assert torch.equal(log_r, log_u.detach())
    assert torch.equal(dmem_r, mem_u.grad.permute(1, 0, 2).reshape(-1, 256))
    g_u = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    assert set(g_u) == set(g_r) and len(g_r) > 40
    diff = [k for k in g_r if not torch.equal(g_r[k], g_u[k])]
    assert not diff, {k: (g_r[k] - g_u[k]).abs().max().item() for k in diff}
    # ... and the masks are really drawn: another seed gives other outputs
    mem_o, _, _, _ = _step(m, "ttm", fd, [T] * B, y, step0=100)
    assert not torch.equal(mem_o, mem_r)


def test_dropout_with_mixed_lengths_is_reproducible_and_seeded(egx_lib, cuda):
    m, _ = _model(cuda, p=0.1)
    lengths = _lengths(8, 61)
    feats = _feats(lengths, 62)
    fd = [f.to(cuda) for f in feats]
    y = _targets(len(lengths), "ttm", m.vocab, 8).to(cuda)
    a = _step(m, "ttm", fd, lengths, y)
    b = _step(m, "ttm", fd, lengths, y)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[3], b[3])
    assert all(torch.equal(a[2][k], b[2][k]) for k in a[2]) and len(a[2]) > 40
    c = _step(m, "ttm", fd, lengths, y, step0=50)
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[1], c[1])
    # the device-resident seed: advanced by every training forward, restored -> the first step again
    m.enable_device_seed()
    seed0 = m._egx_seed_dev.clone()
    s1 = _step(m, "ttm", fd, lengths, y)
    s2 = _step(m, "ttm", fd, lengths, y)
    assert not torch.equal(s1[0], s2[0]) and not torch.equal(s1[1], s2[1])
    assert not torch.equal(m._egx_seed_dev, seed0)
    m._egx_seed_dev.copy_(seed0)
    s3 = _step(m, "ttm", fd, lengths, y)
    assert torch.equal(s1[0], s3[0]) and torch.equal(s1[1], s3[1]) and all(torch.equal(s1[2][k], s3[2][k]) for k in s1[2])
    m._egx_seed_dev = None
    # eval mode: the new methods give what the inference calls give, bit for bit
    m.eval()
    lens = torch.tensor(lengths)
    with torch.no_grad():
        mem_i = m.encode_features("ttm", *fd, lengths=lens)
        log_i = m.decode(y, mem_i, memory_lengths=lens.sum(1))
        mem_t = m.encode_features_ragged("ttm", *fd, lengths=lens)
        log_t = m.decode_ragged(y, mem_t, lens.sum(1))
        assert torch.equal(mem_i, mem_t) and torch.equal(log_i, log_t)
        Ta = [3, 40, 150, 7]
        fa = [f.to(cuda) for f in _feats([(t, t, t) for t in Ta], 63)]
        assert torch.equal(m.encode_features("asd", *fa, lengths=Ta), m.encode_features_ragged("asd", *fa, lengths=Ta))
    mem_g = m.encode_features_ragged("ttm", *fd, lengths=lens)         # eval mode under autograd
    assert mem_g.requires_grad and torch.equal(mem_g.detach(), mem_i)


def test_no_leakage_from_padding_or_between_clips(egx_lib, cuda):
    m, _ = _model(cuda, p=0.1)
    lengths = _lengths(4, 21)
    y = _targets(len(lengths), "ttm", m.vocab, 9).to(cuda)
    runs = [_step(m, "ttm", [f.to(cuda) for f in _feats(lengths, 22, pad=pad)], lengths, y) for pad in (float("nan"), 1e30, 0.0)]
    for r in runs[1:]:
        assert torch.equal(runs[0][0], r[0]) and torch.equal(runs[0][1], r[1]) and torch.equal(runs[0][3], r[3])
        assert all(torch.equal(runs[0][2][k], r[2][k]) for k in runs[0][2])
    assert all(torch.isfinite(g).all() for g in runs[0][2].values())
    # perturbing clip a's frames leaves clip b's memory rows and logits bit-identical under dropout (same batch position, same masks)
    a, bclip = 3, 7
    f_mod = _feats(lengths, 22)
    for f, T in zip(f_mod, lengths[a]):
        f[a, :T] = f[a, :T] * 0.5 + 1.0
    mod = _step(m, "ttm", [f.to(cuda) for f in f_mod], lengths, y)
    S = [sum(r) for r in lengths]
    row0 = np.cumsum([0] + S)
    keep = torch.ones(runs[0][0].shape[0], dtype=torch.bool)
    keep[row0[a]:row0[a + 1]] = False
    assert torch.equal(runs[0][0][keep.to(cuda)], mod[0][keep.to(cuda)])
    others = [i for i in range(len(lengths)) if i != a]
    assert torch.equal(runs[0][1][:, others], mod[1][:, others]) and not torch.equal(runs[0][1][:, a], mod[1][:, a])
    assert torch.equal(runs[0][1][:, bclip], mod[1][:, bclip])
    # a loss that reads only clip b's logits: exactly zero d_memory rows for every other clip, and the parameter gradients of clip b trained
    # alone (p = 0: alone, the clip sits at batch position 0 and would draw other masks)
    m0, _ = _model(cuda, p=0.0)
    feats = _feats(lengths, 22)
    fd = [f.to(cuda) for f in feats]
    one = _step(m0, "ttm", fd, lengths, y, clips=[bclip])
    keep = torch.ones(one[3].shape[0], dtype=torch.bool)
    keep[row0[bclip]:row0[bclip + 1]] = False
    assert (one[3][keep.to(cuda)] == 0).all() and one[3][row0[bclip]:row0[bclip + 1]].abs().max().item() > 0
    solo = _step(m0, "ttm", [f[bclip:bclip + 1].to(cuda) for f in feats], [lengths[bclip]], y[bclip:bclip + 1])
    _bound(one[1][:, bclip], solo[1][:, 0].cpu().double(), 1.5e-2)
    _check_grads(one[2], {k: v.cpu().double() for k, v in solo[2].items()})


def _perm_bound(cuda):
    """The summation-order bound of the gradients (fp32 sums over the clips taken in another order): the worst per-parameter relative
    difference between an equal-length batch (24 clips of T = 40) and its permutation through the EXISTING uniform training call, times 2:
    summation order is the only source of a difference in both. Measured on an MI355X (profiles/ragged_train_g_mi355x.json, "permutation"):
    uniform worst 1.16e-6, so the bound is 2.31e-6; the ragged path's worst was 9.9e-7 (fc.bias), the three-task step's 5.6e-8."""
    m, _ = _model(cuda)
    B, T = 24, 40
    feats = _feats([(T, T, T)] * B, 71)
    y = _targets(B, "ttm", m.vocab, 10)
    perm = torch.from_numpy(np.random.default_rng(72).permutation(B))

    w = torch.linspace(-1, 1, 2 * B * len(m.vocab), device=cuda).view(2, B, -1)
    m.zero_grad(set_to_none=True)
    _lin(m.decode(y.to(cuda), m.encode_features("ttm", *[f[:, :T].contiguous().to(cuda) for f in feats])), w).backward()
    g_a = {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
    m.zero_grad(set_to_none=True)
    _lin(m.decode(y[perm].to(cuda), m.encode_features("ttm", *[f[perm, :T].contiguous().to(cuda) for f in feats])), w[:, perm.to(cuda)]).backward()
    torch.cuda.synchronize()
    g_b = {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
    errs = _grad_errs(g_b, {k: v.cpu().double() for k, v in g_a.items()})
    return max(errs.values())


def test_permuting_the_clips_permutes_outputs_and_keeps_gradients(egx_lib, cuda):
    m, _ = _model(cuda)
    lengths = _lengths(8, 31)                    # 24 clips
    feats = _feats(lengths, 32)
    B, V = len(lengths), len(m.vocab)
    y = _targets(B, "ttm", m.vocab, 11)
    w = _weights(2, B, V).float()
    a = _step(m, "ttm", [f.to(cuda) for f in feats], lengths, y.to(cuda), weight=w.to(cuda))
    perm = np.random.default_rng(33).permutation(B)
    pt = torch.from_numpy(perm)
    b = _step(m, "ttm", [f[pt].to(cuda) for f in feats], [lengths[i] for i in perm], y[pt].to(cuda), weight=w[:, pt].to(cuda))
    S = [sum(r) for r in lengths]
    row0 = np.cumsum([0] + S)
    assert torch.equal(b[0], torch.cat([a[0][row0[i]:row0[i] + S[i]] for i in perm]))
    assert torch.equal(b[1], a[1][:, pt.to(cuda)])
    uni = _perm_bound(cuda)
    errs = _grad_errs(b[2], {k: v.cpu().double() for k, v in a[2].items()})
    worst = max(errs, key=errs.get)
    print(f"permutation: uniform worst {uni:.3e}, ragged worst {errs[worst]:.3e} ({worst}), bound {2 * uni:.3e}")
    assert len(errs) > 40 and errs[worst] <= 2 * uni, (worst, errs[worst], uni)


def _three_task_batch(cuda, vocab, seed):
    rng = np.random.default_rng(seed)
    lt = [tuple(int(v) for v in rng.integers(15, T_PAD + 1, 3)) for _ in range(12)]
    la = [int(v) for v in rng.integers(15, T_PAD + 1, 4)]
    ll = [int(v) for v in rng.integers(15, T_PAD + 1, 12)]
    batch = {
        "ttm": ([f.to(cuda) for f in _feats(lt, seed + 1)], torch.tensor(lt), _targets(len(lt), "ttm", vocab, seed + 2)),
        "asd": ([f.to(cuda) for f in _feats([(t, t, t) for t in la], seed + 3)], torch.tensor(la), _targets(sum(la), "asd", vocab, seed + 4)),
        "lam": ([f.to(cuda) for f in _feats([(t,) for t in ll], seed + 5, n_seg=1)], torch.tensor(ll), _targets(len(ll), "lam", vocab, seed + 6)),
    }
    # targets as the reference's (</s>-terminated) sequences: input = [task, answer], labels = [answer, </s>]
    for k, (f, L, y) in batch.items():
        batch[k] = (f, L, y.to(cuda), torch.stack([y[:, 1], torch.zeros_like(y[:, 1])], dim=1).to(cuda))
    return batch


def _task_loss(m, batch, task):
    f, L, y, labels = batch[task]
    fs = f if task != "lam" else [f[0], None, None]
    logits = m.forward_features_ragged(task, *fs, y, lengths=L)       # (B, V, sy)
    return torch.nn.CrossEntropyLoss()(logits, labels)


def test_a_training_step_as_the_reference_takes_it(egx_lib, cuda):
    """ratio1 * loss_lam + ratio2 * loss_ttm + ratio3 * loss_asd of three forward_features_ragged calls, back-propagated into the shared
    parameters (video_tasktranslation.py:39-66). Measured on an MI355X: the summed loss of the fixed batch went 5.10 -> 1.27 over the 20
    FusedAdam steps at lr 1e-4 (p = 0.1)."""
    from egot2_amd.train import FusedAdam
    m, _ = _model(cuda)
    batch = _three_task_batch(cuda, m.vocab, 81)
    ratios = {"lam": 1.0, "ttm": 0.5, "asd": 2.0}
    m.zero_grad(set_to_none=True)
    sum(ratios[t] * _task_loss(m, batch, t) for t in ("lam", "ttm", "asd")).backward()
    torch.cuda.synchronize()
    joint = {k: p.grad.detach().cpu().double() for k, p in m.named_parameters() if p.grad is not None}
    acc = {}
    for t in ("lam", "ttm", "asd"):
        m.zero_grad(set_to_none=True)
        _task_loss(m, batch, t).backward()
        for k, p in m.named_parameters():
            if p.grad is not None:
                acc[k] = acc.get(k, 0) + ratios[t] * p.grad.detach().cpu().double()
    uni = _perm_bound(cuda)
    errs = {k: ((joint[k] - v).norm() / (v.norm() + 1e-12)).item() for k, v in acc.items() if v.norm() > 0}
    worst = max(errs, key=errs.get)
    print(f"three tasks: worst {errs[worst]:.3e} ({worst}), bound {2 * uni:.3e}")
    assert len(errs) > 40 and set(joint) == set(acc) and errs[worst] <= 2 * uni, (worst, errs[worst], uni)
    # 20 optimizer steps on one fixed mixed-length batch end lower than they started (the gradients point downhill)
    m, _ = _model(cuda, p=0.1)
    opt = FusedAdam(m.parameters(), lr=1e-4)
    losses = []
    for _ in range(21):
        opt.zero_grad(set_to_none=True)
        loss = sum(_task_loss(m, batch, t) for t in ("lam", "ttm", "asd"))
        losses.append(loss.item())
        loss.backward()
        opt.step()
    print(f"loss {losses[0]:.4f} -> {losses[-1]:.4f}")
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses


def test_grouped_fallback_and_refusals(egx_lib, cuda):
    from egot2_amd import functional as F_egx
    m, sd = _model(cuda, compute="f32s")
    lengths = [(5, 5, 5), (30, 40, 30), (150, 150, 150), (5, 5, 5), (1, 20, 1)]
    feats = _feats(lengths, 51)
    fd = [f.to(cuda) for f in feats]
    B, V = len(lengths), len(m.vocab)
    y = _targets(B, "ttm", m.vocab, 12)
    w = _weights(2, B, V)
    mem, logits, grads, _ = _step(m, "ttm", fd, lengths, y.to(cuda), weight=w.float().to(cuda))
    assert F_egx.last_encoder_impl() == "grouped" and F_egx.last_decoder_impl() == "grouped"
    rmems, rlogs, rgrads = _oracle_clipwise(sd, "ttm", feats, lengths, y, w, m.vocab)
    r0 = 0
    for b, row in enumerate(lengths):
        _bound(mem[r0:r0 + sum(row)], rmems[b][:, 0], 1e-3)
        _bound(logits[:, b], rlogs[b][:, 0], 1e-3)
        r0 += sum(row)
    _check_grads(grads, rgrads, tol=1e-3, fc_tol=1e-3)
    # a clip beyond the wide attention (S_b = 510): grouped in bf16 too, and differentiable
    m.set_compute("bf16")
    long_l = [(170, 170, 170), (10, 10, 10)]
    rng = np.random.default_rng(52)
    lf = []
    for k in range(3):
        f = torch.from_numpy(rng.standard_normal((2, 170, 256), dtype=np.float32))
        f[1, 10:] = float("nan")
        lf.append(f)
    y2 = _targets(2, "ttm", m.vocab, 13)
    w2 = _weights(2, 2, V)
    mem, logits, grads, _ = _step(m, "ttm", [f.to(cuda) for f in lf], [170, 10], y2.to(cuda), weight=w2.float().to(cuda))
    assert F_egx.last_encoder_impl() == "grouped"
    rmems, rlogs, rgrads = _oracle_clipwise(sd, "ttm", lf, long_l, y2, w2, m.vocab)
    _bound(mem[:510], rmems[0][:, 0], 4e-2)
    _bound(mem[510:], rmems[1][:, 0], 1e-2)
    assert len(grads) > 40 and all(torch.isfinite(g).all() for g in grads.values())
    # refusals, before any device work
    lens = torch.tensor(lengths)
    with pytest.raises(ValueError, match="equal length"):
        m.encode_features_ragged("asd", *fd, lengths=lens)
    with pytest.raises(ValueError, match="integers"):
        m.encode_features_ragged("ttm", *fd, lengths=lens.float())
    with pytest.raises(ValueError, match="1 .. 150"):
        m.encode_features_ragged("ttm", *fd, lengths=[-1, 5, 5, 5, 5])
    with pytest.raises(ValueError, match="1 .. 150"):
        m.encode_features_ragged("ttm", *fd, lengths=[151, 5, 5, 5, 5])
    with pytest.raises(ValueError, match="packed"):
        m.decode_ragged(y.to(cuda), torch.zeros(17, 256, device=cuda), lens.sum(1))
    F_egx.bucket_hook = lambda flat, lo, hi: None
    try:
        with pytest.raises(ValueError, match="bucket_cb"):
            m.encode_features_ragged("ttm", *fd, lengths=lens)
    finally:
        F_egx.bucket_hook = None
