"""-m gpu: ragged batches for the EgoT2-g HHI model (ABI v18: egx_ragged_encode on the wide bf16 path, egx_decoder_ragged_fwd): one encoder and
one decoder call per batch of clips of their own lengths, for the reference's batch_size=1 validation
(HHI/tasks/multitask/video_tasktranslation.py:83-101,176-187). Padded frames are NaN unless stated. Every clip is checked against the fp64
oracle on its unpadded frames at the bounds of test_gpu_parity_hygiene.py (memory 1e-2, logits 1.5e-2, relative to max(1, |ref|))."""
import numpy as np
import pytest
import torch

from tests.util import hhi_args, seeded_state_dict

pytestmark = pytest.mark.gpu

T_PAD = 150
# (lam, ttm, asd) frames per clip: S_b across the kernel edges (<= 64, 65 .. 128, 128 / 129, 3 x 150 = 450), one-frame segments, T_asd != T_ttm
TTM_LENGTHS = [(5, 5, 5), (10, 12, 8), (21, 21, 22), (22, 22, 21), (30, 40, 30), (43, 43, 42), (43, 43, 43), (150, 150, 150), (1, 1, 1),
               (1, 20, 1), (30, 30, 12), (60, 60, 90), (15, 15, 15), (64, 1, 1), (100, 100, 100), (2, 150, 3)]


def _model(cuda, compute="bf16"):
    from egot2_amd import hhi_multitask
    from egot2_amd.synth import HHI_G_VOCAB
    m = hhi_multitask.TaskTranslationPromptTransformer(hhi_args(hidden_dim=256, num_heads=4, num_layers=3, dropout=0.0), HHI_G_VOCAB)
    sd = seeded_state_dict(m, 31)
    m.load_state_dict(sd)
    m.pos_embed.dropout.p = 0.0
    m = m.to(cuda).set_compute(compute).eval()
    sd64 = {k: v.double() for k, v in sd.items()}
    return m, sd64


def _lengths(n_extra, seed):
    rng = np.random.default_rng(seed)
    extra = [tuple(int(v) for v in rng.integers(1, T_PAD + 1, 3)) for _ in range(n_extra)]
    L = TTM_LENGTHS + extra
    order = rng.permutation(len(L))
    return [L[i] for i in order]


def _feats(lengths, seed, pad=float("nan"), n_seg=3):
    """Padded (B, T_PAD, 256) features, frames t >= T_{b,k} set to `pad`."""
    rng = np.random.default_rng(seed)
    B = len(lengths)
    out = []
    for k in range(n_seg):
        f = torch.from_numpy(rng.standard_normal((B, T_PAD, 256), dtype=np.float32))
        for b, row in enumerate(lengths):
            f[b, row[k]:] = pad
        out.append(f)
    return out


def _bound(a, ref, tol):
    err = (a.detach().cpu().double() - ref).abs().max().item()
    assert err < tol * max(1.0, ref.abs().max().item()), err
    return err


def _oracle(sd64, task, feats, b, lens, vocab):
    from oracle import translator_ref as tr
    fs = [f[b:b + 1, :T].double() for f, T in zip(feats, lens)]
    rmem = tr.hhi_g_encode(sd64, 4, task, *fs)
    y = torch.full((rmem.shape[1], 1), vocab[task], dtype=torch.long)
    rlog = tr.g_decode(sd64, 4, y, rmem)
    return rmem, rlog[0, :, -2:]


def test_ttm_ragged_batch_matches_the_oracle_clip_by_clip(egx_lib, cuda):
    from egot2_amd import functional as F_egx
    m, sd64 = _model(cuda)
    lengths = _lengths(24, 5)                    # 40 clips in random order
    feats = _feats(lengths, 6)
    fd = [f.to(cuda) for f in feats]
    with torch.no_grad():
        mem = m.encode_features("ttm", *fd, lengths=torch.tensor(lengths))
        assert F_egx.last_encoder_impl() == "ragged"
        pred = m.predict_features("ttm", *fd, lengths=torch.tensor(lengths))
        assert F_egx.last_encoder_impl() == "ragged" and F_egx.last_decoder_impl() == "ragged"
    torch.cuda.synchronize()
    S = [sum(r) for r in lengths]
    assert mem.shape == (sum(S), 256) and pred.shape == (len(lengths), 2)
    assert torch.isfinite(mem).all() and torch.isfinite(pred).all()
    r0 = 0
    for b, row in enumerate(lengths):
        rmem, rpred = _oracle(sd64, "ttm", feats, b, row, m.vocab)
        _bound(mem[r0:r0 + S[b]], rmem[:, 0], 1e-2)
        _bound(pred[b], rpred[0], 1.5e-2)
        r0 += S[b]


def test_asd_and_lam_ragged_batches_match_the_oracle(egx_lib, cuda):
    from egot2_amd import functional as F_egx
    m, sd64 = _model(cuda)
    T = [1, 3, 15, 40, 64, 100, 150, 7]
    lengths = [(t, t, t) for t in T]
    feats = _feats(lengths, 8)
    fd = [f.to(cuda) for f in feats]
    with torch.no_grad():
        mem = m.encode_features("asd", *fd, lengths=torch.tensor(T))
        assert F_egx.last_encoder_impl() == "ragged" and mem.shape == (3, sum(T), 256)
        pred = m.predict_features("asd", *fd, lengths=torch.tensor(T))
    assert pred.shape == (sum(T), 2) and torch.isfinite(pred).all()
    f0 = 0
    for b, t in enumerate(T):
        rmem, rpred = _oracle(sd64, "asd", feats, b, lengths[b], m.vocab)
        _bound(mem[:, f0:f0 + t], rmem, 1e-2)
        # the asd decode is the existing batched decoder over sum_b T_b frame triples (3 memory rows each); its bf16 error on them
        # reaches 1.9e-2 here, inside the 4e-2 test_gpu_decoder.py allows the asd task
        _bound(pred[f0:f0 + t], rpred, 4e-2)
        f0 += t
    with torch.no_grad():       # ... and each clip's asd logits equal what the existing path gives that clip alone
        f0 = 0
        for b, t in enumerate(T):
            solo = m.predict_features("asd", *[f[b:b + 1, :t].to(cuda) for f in feats])
            assert (solo - pred[f0:f0 + t]).abs().max().item() <= 1e-2
            f0 += t
    # task lam: one segment
    TL = [1, 20, 64, 65, 129, 150, 33]
    lam = _feats([(t,) for t in TL], 9, n_seg=1)[0]
    with torch.no_grad():
        mem = m.encode_features("lam", lam.to(cuda), lengths=TL)
        pred = m.predict_features("lam", lam.to(cuda), lengths=TL)
        assert F_egx.last_encoder_impl() == "ragged" and F_egx.last_decoder_impl() == "ragged"
    r0 = 0
    for b, t in enumerate(TL):
        rmem, rpred = _oracle(sd64, "lam", [lam], b, (t,), m.vocab)
        _bound(mem[r0:r0 + t], rmem[:, 0], 1e-2)
        _bound(pred[b], rpred[0], 1.5e-2)
        r0 += t


def test_ragged_decoder_alone_matches_the_uniform_decoder_and_the_oracle(egx_lib, cuda):
    from egot2_amd import functional as F_egx
    from oracle import translator_ref as tr
    m, sd64 = _model(cuda)
    S = [1, 64, 65, 450, 1024, 64, 1, 450]
    rng = np.random.default_rng(12)
    mem = torch.from_numpy(rng.standard_normal((sum(S), 256), dtype=np.float32))
    y = torch.stack([torch.full((len(S),), m.vocab["ttm"]), torch.from_numpy(rng.integers(5, 7, len(S)))], dim=1)
    with torch.no_grad():
        out = m.decode(y.to(cuda), mem.to(cuda), memory_lengths=S)
        assert F_egx.last_decoder_impl() == "ragged" and out.shape == (2, len(S), len(m.vocab))
        row0 = np.cumsum([0] + S)
        for s in sorted(set(S)):
            idx = [b for b in range(len(S)) if S[b] == s]
            mg = torch.stack([mem[row0[b]:row0[b] + s] for b in idx], dim=1).to(cuda)          # (s, G, d)
            ref = m.decode(y[idx].to(cuda), mg)
            assert F_egx.last_decoder_impl() == "fused"
            assert (out[:, idx] - ref).abs().max().item() <= 1e-6
    for b in (0, 2, 3, 4):
        rlog = tr.g_decode(sd64, 4, y[b:b + 1], mem[row0[b]:row0[b] + S[b], None].double())
        _bound(out[:, b], rlog[:, 0], 1.5e-2)


def _run(m, fd, lengths):
    with torch.no_grad():
        mem = m.encode_features("ttm", *fd, lengths=torch.tensor(lengths))
        pred = m.predict_features("ttm", *fd, lengths=torch.tensor(lengths))
    torch.cuda.synchronize()
    return mem, pred


def test_no_leakage_between_clips_or_from_padding(egx_lib, cuda):
    m, _ = _model(cuda)
    lengths = _lengths(4, 21)
    f_nan = _feats(lengths, 22)
    f_zero = _feats(lengths, 22, pad=0.0)
    mem_a, pred_a = _run(m, [f.to(cuda) for f in f_nan], lengths)
    mem_b, pred_b = _run(m, [f.to(cuda) for f in f_zero], lengths)
    assert torch.isfinite(mem_a).all() and torch.isfinite(pred_a).all()
    assert torch.equal(mem_a, mem_b) and torch.equal(pred_a, pred_b)
    # change clip 3's frames: every other clip's rows and logits stay bit-identical
    f_mod = [f.clone() for f in f_nan]
    for f, T in zip(f_mod, lengths[3]):
        f[3, :T] = f[3, :T] * 0.5 + 1.0
    mem_c, pred_c = _run(m, [f.to(cuda) for f in f_mod], lengths)
    S = [sum(r) for r in lengths]
    r0 = int(sum(S[:3]))
    keep = torch.ones(mem_a.shape[0], dtype=torch.bool)
    keep[r0:r0 + S[3]] = False
    assert torch.equal(mem_a[keep.to(cuda)], mem_c[keep.to(cuda)])
    others = [b for b in range(len(lengths)) if b != 3]
    assert torch.equal(pred_a[others], pred_c[others])
    assert not torch.equal(pred_a[3], pred_c[3])


def test_permuting_the_clips_permutes_the_outputs_bit_for_bit(egx_lib, cuda):
    m, _ = _model(cuda)
    lengths = _lengths(8, 31)
    feats = _feats(lengths, 32)
    mem_a, pred_a = _run(m, [f.to(cuda) for f in feats], lengths)
    perm = np.random.default_rng(33).permutation(len(lengths))
    lp = [lengths[i] for i in perm]
    mem_b, pred_b = _run(m, [f[torch.from_numpy(perm)].to(cuda) for f in feats], lp)
    S = [sum(r) for r in lengths]
    row0 = np.cumsum([0] + S)
    ref = torch.cat([mem_a[row0[i]:row0[i] + S[i]] for i in perm])
    assert torch.equal(mem_b, ref)
    assert torch.equal(pred_b, pred_a[torch.from_numpy(perm).to(cuda)])


def test_full_length_batch_equals_the_uniform_path_and_clips_match_their_solo_runs(egx_lib, cuda):
    m, _ = _model(cuda)
    B, T = 16, 15
    feats = _feats([(T, T, T)] * B, 41)
    fd = [f[:, :T].contiguous().to(cuda) for f in feats]
    with torch.no_grad():
        rag = m.encode_features("ttm", *fd, lengths=[T] * B)
        uni = m.encode_features("ttm", *fd)                               # (S, B, d)
        assert (rag - uni.permute(1, 0, 2).reshape(-1, 256)).abs().max().item() <= 1e-6
        y = torch.full((B, 1), m.vocab["ttm"], dtype=torch.long, device=cuda)
        d_rag = m.decode(y, rag, memory_lengths=[3 * T] * B)
        d_uni = m.decode(y, uni)
        assert (d_rag - d_uni).abs().max().item() <= 1e-6
    # each clip of a ragged batch against the same clip alone through the existing (uniform) path
    lengths = _lengths(0, 43)
    feats = _feats(lengths, 44)
    mem, pred = _run(m, [f.to(cuda) for f in feats], lengths)
    S = [sum(r) for r in lengths]
    r0, worst = 0, 0.0
    with torch.no_grad():
        for b, row in enumerate(lengths):
            solo = m.encode_features("ttm", *[f[b:b + 1, :t].to(cuda) for f, t in zip(feats, row)])
            e = (mem[r0:r0 + S[b]] - solo[:, 0]).abs().max().item()
            worst = max(worst, e)
            r0 += S[b]
    assert worst <= 1e-2, worst


def test_grouped_fallback_matches_and_refusals(egx_lib, cuda):
    from egot2_amd import functional as F_egx
    m, sd64 = _model(cuda)
    lengths = [(5, 5, 5), (30, 40, 30), (150, 150, 150), (5, 5, 5), (1, 20, 1)]
    feats = _feats(lengths, 51)
    fd = [f.to(cuda) for f in feats]
    mem_r, pred_r = _run(m, fd, lengths)
    m.set_compute("f32s")
    mem_g, pred_g = _run(m, fd, lengths)
    assert F_egx.last_encoder_impl() == "grouped" and F_egx.last_decoder_impl() == "grouped"
    assert (mem_g - mem_r).abs().max().item() < 1e-2 * max(1.0, mem_g.abs().max().item())
    assert (pred_g - pred_r).abs().max().item() < 1.5e-2 * max(1.0, pred_g.abs().max().item())
    S = [sum(r) for r in lengths]
    r0 = 0
    for b, row in enumerate(lengths):
        rmem, rpred = _oracle(sd64, "ttm", feats, b, row, m.vocab)
        _bound(mem_g[r0:r0 + S[b]], rmem[:, 0], 1e-3)
        _bound(pred_g[b], rpred[0], 1e-3)
        r0 += S[b]
    # a clip beyond the wide attention (S_b = 510 > 480): grouped in bf16 too
    m.set_compute("bf16")
    long_l = [(170, 170, 170), (10, 10, 10)]
    lf = []
    rng = np.random.default_rng(52)
    for k in range(3):
        f = torch.from_numpy(rng.standard_normal((2, 170, 256), dtype=np.float32))
        f[1, 10:] = float("nan")
        lf.append(f)
    with torch.no_grad():
        mem_l = m.encode_features("ttm", *[f.to(cuda) for f in lf], lengths=[170, 10])
    assert F_egx.last_encoder_impl() == "grouped"
    rmem, _ = _oracle(sd64, "ttm", lf, 0, long_l[0], m.vocab)
    _bound(mem_l[:510], rmem[:, 0], 4e-2)
    rmem, _ = _oracle(sd64, "ttm", lf, 1, long_l[1], m.vocab)
    _bound(mem_l[510:], rmem[:, 0], 1e-2)
    # refusals, before any device work
    with pytest.raises(ValueError, match="inference-only"):
        m.train().encode_features("ttm", *fd, lengths=torch.tensor(lengths))
    m.eval()
    with pytest.raises(ValueError, match="inference-only"):
        m.encode_features("ttm", *fd, lengths=torch.tensor(lengths))      # grad enabled, trainable parameters
    with torch.no_grad(), pytest.raises(ValueError, match="equal length"):
        m.encode_features("asd", *fd, lengths=torch.tensor(lengths))
