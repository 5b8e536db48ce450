"""The decoder's cross-attention weights on the host, without a GPU (egx_cross_attention_weights, egx_decoder_cross_weights,
egx_decoder_generate_attn: additions under ABI v18): symbols, every refusal with its message and no launch, the fp64 oracle of the GPU
tests (tests/attn_ref.py) against the weights recorded from the real classes' forward hooks, attention_by_segment, and the Python
validation. Pure host work (no HIP call)."""
import ctypes as C
import json
import os
import subprocess
import sys
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
NEW = ("egx_cross_attention_weights", "egx_decoder_cross_weights", "egx_decoder_generate_attn")
PTR = 1 << 12       # a non-null, 16-byte aligned marker: every call below is refused before anything is read


def _dcfg(d=256, h=4, L=3, V=7, S=48, compute=1, p_drop=0.0, p_pos=0.0, dff=2048, sy=2):
    from egot2_amd._lib import DecConfig
    return DecConfig(d, h, dff, L, V, sy, S, 1e-5, compute, p_drop, p_pos, None)


def test_abi_stays_18_and_the_three_symbols_resolve(egx_lib):
    from egot2_amd import _lib
    assert _lib.EGX_ABI_VERSION == 18 and egx_lib.egx_abi_version() == 18
    for name in NEW:
        assert hasattr(egx_lib, name) and name in _lib.SIGNATURES, name
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "egot2x.h")).read()
    for name in NEW:
        assert name + "(" in hdr
    for cite in ("task_prompt_model.py:163-172", "video_model_builder.py:20-30", "video_model_builder_2task.py:24", "lta_models_seqdecoder.py:30-39"):
        assert cite in hdr, cite


def test_the_primitive_refuses_on_the_host(egx_lib):
    lib = egx_lib
    lib.egx_launch_count(1)

    def call(q=PTR, ldq=256, k=PTR, ldk=512, bf16=1, mtab=None, B=2, H=4, dh=64, Sq=2, Sk=48, out=PTR, ldo=48):
        return lib.egx_cross_attention_weights(q, ldq, k, ldk, bf16, mtab, B, H, dh, Sq, Sk, out, ldo, None)

    def refused(frag, **kw):
        assert call(**kw) != 0 and frag in lib.egx_last_error(), (kw, frag, lib.egx_last_error())

    refused(b"null pointer", q=None)
    refused(b"null pointer", k=None)
    refused(b"null pointer", out=None)
    for dh in (0, 8, 24, 48, 96, 256):
        refused(b"head dim %d" % dh, dh=dh, H=1)
    refused(b"Sk = 0", Sk=0, ldo=0)
    refused(b"Sk = 1025", Sk=1025, ldo=1025)
    refused(b"Sk = -3", Sk=-3)
    refused(b"ldo = 47 < Sk = 48", ldo=47)
    refused(b"multiples of 8", ldq=260)
    refused(b"multiples of 8", ldk=516)
    refused(b"multiples of 8", ldq=128)                 # below H * dh
    refused(b"16-byte aligned", q=PTR + 4)
    refused(b"Sq = 0", Sq=0)
    refused(b"H = 0", H=0)
    assert lib.egx_launch_count(0) == 0                 # nothing was launched


def test_the_decoder_entries_refuse_on_the_host(egx_lib):
    lib = egx_lib
    lib.egx_launch_count(1)

    def cw(cfg, frag, B=4, ml=None, saved=PTR, out=PTR):
        ml_arr = (C.c_int * len(ml))(*ml) if ml is not None else None
        rc = lib.egx_decoder_cross_weights(C.byref(cfg) if cfg is not None else None, B, ml_arr, saved, out, None)
        assert rc != 0 and frag in lib.egx_last_error(), (frag, lib.egx_last_error())

    cw(None, b"null")
    cw(_dcfg(), b"null pointer", saved=None)
    cw(_dcfg(), b"null pointer", out=None)
    cw(_dcfg(), b"null pointer", ml=[48, 3, 7, 9], saved=None)
    cw(_dcfg(p_drop=0.1), b"inference only")
    cw(_dcfg(p_pos=0.1), b"inference only")
    cw(_dcfg(p_drop=0.1), b"inference only", ml=[48, 3, 7, 9])
    cw(_dcfg(), b"memory of 0 rows", ml=[48, 0, 7, 9])
    cw(_dcfg(), b"memory of 49 rows", ml=[48, 49, 7, 9])
    cw(_dcfg(), b"memory of -1 rows", ml=[-1, 4, 7, 9])
    cw(_dcfg(d=256, h=2), b"head dim 128")              # the fused decoder's own limits
    cw(_dcfg(compute=0), b"bf16")
    cw(_dcfg(S=1025), b"S = 1025")
    cw(_dcfg(sy=9), b"sy = 9")
    cw(_dcfg(), b"B = 0", B=0)

    def gen(cfg, frag, n=2, attn=PTR, others=PTR):
        o = others
        rc = lib.egx_decoder_generate_attn(C.byref(cfg), o, o, o, o, 256, None if o is None else C.cast(o, C.POINTER(
            __import__("egot2_amd._lib", fromlist=["DecLayer"]).DecLayer)), o, o, 4, n, o, None, o, None, 0, None, None, attn)
        assert rc != 0 and frag in lib.egx_last_error(), (frag, lib.egx_last_error())

    gen(_dcfg(), b"null attn_out", attn=None)
    gen(_dcfg(p_drop=0.5), b"inference only")
    gen(_dcfg(), b"n_steps = 65", n=65)
    gen(_dcfg(), b"null pointer", others=None)
    gen(_dcfg(V=1025), b"vocab = 1025")
    assert lib.egx_launch_count(0) == 0


FIXTURES = ["attn_ref_hhi_g", "attn_ref_hoi_g"]


@pytest.mark.parametrize("fixture", FIXTURES)
def test_oracle_reproduces_the_hooked_weights_of_the_real_class(fixture):
    """tests/attn_ref.g_decode_attn against the weights tests/golden/make_golden_attn.py recorded through forward hooks on the real
    classes' multihead_attn: below 1e-9 in fp64; rows sum to 1; the recording is not the uniform answer."""
    from tests import attn_ref as ar
    path = os.path.join(HERE, "golden", "live", fixture + ".npz")
    assert os.path.getsize(path) < (1 << 20)
    z = np.load(path)
    c = json.loads(str(z["config"]))
    assert c == ar.RECORDINGS[fixture]
    _, sd64, y, mem, _ = ar.recording_inputs(c)
    assert np.array_equal(y.numpy(), z["tokens"])
    with torch.no_grad():
        logits, w = ar.g_decode_attn(sd64, c["h"], y, mem)
    rw = torch.from_numpy(z["weights"])
    assert rw.dtype == torch.float64 and rw.shape == (c["L"], c["B"], c["sy"], mem.shape[0])
    assert (w - rw).abs().max().item() < 1e-9 and (logits - torch.from_numpy(z["logits"])).abs().max().item() < 1e-9
    assert (rw.sum(-1) - 1).abs().max().item() < 1e-12
    assert (rw - 1.0 / rw.shape[-1]).abs().max().item() > 1e-2
    # the oracle's logits are g_decode's: the restatement changed nothing else
    from oracle import translator_ref as tr
    with torch.no_grad():
        assert torch.equal(logits, tr.g_decode(sd64, c["h"], y, mem))


@pytest.mark.reference
@pytest.mark.parametrize("fixture", FIXTURES)
def test_recording_reproduces_from_the_live_reference(fixture):
    """A fresh recording (one process per tree) equals the committed one."""
    from oracle import ref_harness as rh
    if not rh.reference_available():
        pytest.skip("the reference tree is not on this machine")
    root = os.path.dirname(HERE)
    r = subprocess.run([sys.executable, os.path.join(HERE, "golden", "make_golden_attn.py"), "--check", fixture], capture_output=True, text=True,
                       cwd=root, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("check ")][-1].split()
    assert line[3] == "True" and float(line[5]) < 1e-12 and float(line[7]) < 1e-12, line


@pytest.mark.parametrize("H,dh", [(4, 64), (8, 32), (8, 16), (2, 128)])
def test_bar_of_the_primitive_is_a_condition(H, dh):
    """The 2e-6 bar of tests/test_gpu_attn_weights.py item 1 on that test's own inputs (tests/attn_ref.primitive_inputs), where no GPU is
    needed. A correct fp32 evaluation (torch's, another summation order than the kernel's) stays within a quarter of the bar on every
    case. An evaluation with the scores rounded to bf16 and the uniform answer 1 / Sk miss the bar on EVERY case with more than one key
    (by 4x at least), and over the shape's cases by at least 3.8e-4 and 4e-2."""
    from tests import attn_ref as ar
    BAR = 2e-6
    worst32, miss16, missu = 0.0, [], []
    for Sq, Sk, B in ar.primitive_cases(H, dh):
        q, k = ar.primitive_inputs(H, dh, Sq, Sk, B)
        q, k = q.view(B, Sq, -1), k.view(B, Sk, -1)
        ref = ar.softmax_weights(q.double(), k.double(), H)
        worst32 = max(worst32, (ar.softmax_weights(q, k, H).double() - ref).abs().max().item())
        if Sk > 1:
            qh = q.double().reshape(B, Sq, H, dh).permute(0, 2, 1, 3)
            kh = k.double().reshape(B, Sk, H, dh).permute(0, 2, 1, 3)
            s16 = ((qh @ kh.transpose(-1, -2)) / dh ** 0.5).bfloat16().double()
            miss16.append((torch.softmax(s16, -1).mean(1) - ref).abs().max().item())
            missu.append((ref - 1.0 / Sk).abs().max().item())
    print(f"H = {H}, dh = {dh}: fp32 {worst32:.2e}; bf16 scores {min(miss16):.2e} .. {max(miss16):.2e}; uniform {min(missu):.2e} .. {max(missu):.2e}")
    assert worst32 < BAR / 4, worst32
    assert min(miss16) > 4 * BAR and max(miss16) >= 3.8e-4, (min(miss16), max(miss16))
    assert min(missu) > 4 * BAR and max(missu) >= 4e-2, (min(missu), max(missu))


def test_attention_by_segment_against_a_hand_sum():
    from egot2_amd.decoder import DecoderMixin as D
    g = torch.Generator().manual_seed(3)
    a = torch.rand(2, 3, 2, 45, generator=g, dtype=torch.float64)
    r = D.attention_by_segment(a, (15, 15, 15))
    assert r.shape == (2, 3, 2, 3)
    for k in range(3):
        assert torch.allclose(r[..., k], a[..., 15 * k:15 * k + 15].sum(-1), atol=1e-14)
    assert torch.allclose(r.sum(-1), a.sum(-1), atol=1e-13)
    r = D.attention_by_segment(a, torch.tensor([[15, 15, 15], [1, 0, 7], [20, 20, 5]]))
    assert r.shape == (2, 3, 2, 3)
    assert torch.allclose(r[:, 1, :, 0], a[:, 1, :, 0], atol=1e-14) and r[:, 1, :, 1].abs().max().item() == 0
    assert torch.allclose(r[:, 1, :, 2], a[:, 1, :, 1:8].sum(-1), atol=1e-14)
    assert torch.allclose(r[:, 2, :, 2], a[:, 2, :, 40:45].sum(-1), atol=1e-14)
    assert D.attention_by_segment(a[0, 0, 0], [45]).shape == (1,)
    for bad, frag in ((([15.0, 30.0]), "integers"), ([[[1]]], "integers"), ([], "integers"), ([-1, 46], "non-negative"), ([40, 6], "at most"),
                      (torch.tensor([[15, 30], [1, 2]]), "B = 2")):
        with pytest.raises(ValueError, match=frag):
            D.attention_by_segment(a, bad)
    with pytest.raises(ValueError, match="floating-point"):
        D.attention_by_segment(torch.zeros(3, 4, dtype=torch.int64), [4])


def _model(h=4):
    from egot2_amd import hoi_multitask
    from tests import greedy_ref as gr
    args = NS(hidden_dim=256, num_heads=h, num_layers=1, dropout=0.0, pnr_cfg_file=None, oscc_cfg_file=None, action_cfg_file=None, lta_cfg_file=None)
    return hoi_multitask.TaskPromptTransformer(args, gr.vocab_of(12))


def test_python_validation_raises_before_any_library_call(egx_lib, monkeypatch):
    from egot2_amd import _lib, hhi_multitask
    m = _model()
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was called")))
    mem, y = torch.zeros(16, 3, 256), torch.zeros(3, 2, dtype=torch.int64)
    with pytest.raises(ValueError, match="inference-only"):
        m.train().decode(y, mem, return_attention=True)
    with pytest.raises(ValueError, match="inference-only"):
        m.train().greedy_decode(mem, 4, 2, return_attention=True)
    m.eval()
    with pytest.raises(ValueError, match="inference-only"):             # eval mode, but an autograd graph over the parameters
        m.decode(y, mem, return_attention=True)
    with pytest.raises(TypeError):                                       # keyword-only
        m.decode(y, mem, True)
    with torch.no_grad():
        with pytest.raises(ValueError, match=r"head dims \(16, 32, 64, 128\).*1\.\.1024.*head dim 256"):
            _model(h=1).eval().decode(y, mem, return_attention=True)
        with pytest.raises(ValueError, match="1025 memory tokens"):
            m.decode(y, torch.zeros(1025, 3, 256), return_attention=True)
    hh = hhi_multitask.TaskTranslationPromptTransformer(NS(hidden_dim=256, num_heads=4, num_layers=1, dropout=0.0, lam_checkpoint=None,
                                                           ttm_checkpoint=None, asd_checkpoint=None),
                                                        {'</s>': 0, '<unk>': 1, 'ttm': 2, 'lam': 3, 'asd': 4, '0': 5, '1': 6})
    with pytest.raises(ValueError, match="inference-only"):
        hh.train().decode(y, torch.zeros(10, 256), torch.tensor([3, 3, 4]), return_attention=True)
    import inspect
    for fn in (hh.decode, m.decode, m.greedy_decode):
        p = inspect.signature(fn).parameters["return_attention"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    assert "discarded" not in hhi_multitask.CustomDecoderLayer.__doc__
