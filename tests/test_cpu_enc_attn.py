"""The encoder's self-attention weights on the host, without a GPU (egx_self_attention_weights, egx_attention_rollout,
egx_encoder_self_weights: additions under ABI v27; functional.self_attention_weights / attention_rollout / encoder_attention,
TranslatorMixin.record_attention): the gate (tests/enc_attn_ref.py) against the weights recorded from the real classes, the symbols, every
host refusal with its text and no launch, the Python refusals before any library call, the condition of every bar, and the perturbed
references each bar has to reject. Pure host work (no HIP call)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import enc_attn_ref as er

HERE = os.path.dirname(os.path.abspath(__file__))
NEW = ("egx_self_attention_weights", "egx_attention_rollout", "egx_attention_rollout_scratch", "egx_encoder_self_weights")
PTR = 1 << 12       # a non-null, 16-byte aligned marker: every call below is refused before anything is read
FIXTURE = os.path.join(HERE, "golden", "live", "enc_attn_ref.npz")


# ---- the gate against the recordings of the real classes ----
@pytest.mark.parametrize("name", list(er.RECORDINGS))
def test_gate_reproduces_the_recorded_weights_of_the_real_class(name):
    """tests/enc_attn_ref.case_oracle against what tests/golden/make_golden_encattn.py recorded (a pre-hook on every encoder layer of the
    real class, the layer's own self_attn called with need_weights=True): fp64 round-off; rows sum to 1; not the uniform answer."""
    z = np.load(FIXTURE)
    c = json.loads(str(z[name + "/config"]))
    assert c == er.RECORDINGS[name]
    rw = torch.from_numpy(z[name + "/weights"])
    w = er.case_oracle(name)[0]
    assert rw.dtype == torch.float64 and rw.shape == w.shape and rw.shape[0] == c["L"] and rw.shape[1] == c["B"]
    assert (w - rw).abs().max().item() < 1e-12
    assert (rw.sum(-1) - 1).abs().max().item() < 1e-12
    assert (rw - 1.0 / rw.shape[-1]).abs().max().item() > er.S_MIN


def test_fixture_holds_arrays_and_seeds_only_and_is_small():
    z = np.load(FIXTURE)
    assert sorted(z.files) == sorted(f"{n}/{k}" for n in er.RECORDINGS for k in ("config", "weights"))
    live = os.path.dirname(FIXTURE)
    others = [os.path.getsize(os.path.join(live, f)) for f in os.listdir(live) if f != "enc_attn_ref.npz"]
    assert os.path.getsize(FIXTURE) <= max(others)


@pytest.mark.reference
def test_recording_reproduces_from_the_live_reference():
    """A fresh recording (one process per model) equals the committed one."""
    from oracle import ref_harness as rh
    if not rh.reference_available():
        pytest.skip("the reference tree is not on this machine")
    r = subprocess.run([sys.executable, os.path.join(HERE, "golden", "make_golden_encattn.py"), "--check"], capture_output=True, text=True,
                       cwd=os.path.dirname(HERE), timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("check ")]
    assert len(lines) == len(er.RECORDINGS)
    for ln in lines:
        assert ln[3] == "True" and float(ln[5]) < 1e-12, ln


# ---- the symbols ----
def test_abi_stays_18_and_the_new_symbols_resolve(egx_lib):
    from egot2_amd import _lib
    assert _lib.EGX_ABI_VERSION == 18 and egx_lib.egx_abi_version() == 18
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "egot2x.h")).read()
    for name in NEW:
        assert hasattr(egx_lib, name) and name in _lib.SIGNATURES, name
        assert name + "(" in hdr, name
    assert "ABI v27 additions" in hdr
    for scope in ("simple_vit", "256 / 512", "egx_ragged_encode", "egx_ragged_cap_"):      # what the header declares out of scope
        assert scope in hdr[hdr.index("ABI v27 additions"):], scope


# ---- the host refusals ----
def test_the_primitive_refuses_on_the_host(egx_lib):
    lib = egx_lib
    lib.egx_launch_count(1)

    def call(q=PTR, ldq=384, k=PTR, ldk=384, bf16=0, rowtab=None, segtab=None, K=0, B=2, H=4, dh=32, S=45, w=PTR, ldw=45, seg=None):
        return lib.egx_self_attention_weights(q, ldq, k, ldk, bf16, rowtab, segtab, K, B, H, dh, S, w, ldw, seg, None)

    def refused(frag, **kw):
        assert call(**kw) != 0 and frag in lib.egx_last_error(), (kw, frag, lib.egx_last_error())

    refused(b"null pointer", q=None)
    refused(b"null pointer", k=None)
    refused(b"null pointer", w=None)                    # neither output
    for dh in (0, 8, 24, 48, 256, 512):
        refused(b"head dim %d" % dh, dh=dh, H=1, ldq=512, ldk=512)
    refused(b"S = 0", S=0, ldw=0)
    refused(b"S = 513", S=513, ldw=513)
    refused(b"S = -3", S=-3)
    refused(b"ldw = 44 < S = 45", ldw=44)
    refused(b"multiples of 8", ldq=388)
    refused(b"multiples of 8", ldk=388)
    refused(b"multiples of 8", ldq=120)                 # below H * dh
    refused(b"multiples of 8", ldk=64)
    refused(b"16-byte aligned", q=PTR + 4)
    refused(b"16-byte aligned", k=PTR + 8)
    refused(b"H = 0", H=0)
    refused(b"B = -1", B=-1)
    refused(b"segment table", seg=PTR, K=3)             # seg_out without the table
    refused(b"K = 0", seg=PTR, segtab=PTR, K=0)
    refused(b"K = 17", seg=PTR, segtab=PTR, K=17)
    assert lib.egx_launch_count(0) == 0                 # nothing was launched


def test_the_rollout_refuses_on_the_host(egx_lib):
    lib = egx_lib
    lib.egx_launch_count(1)

    def refused(frag, w=PTR, L=2, B=2, S=45, rowlen=None, segtab=None, K=0, scratch=PTR, out=PTR, seg=None):
        rc = lib.egx_attention_rollout(w, L, B, S, rowlen, segtab, K, scratch, out, seg, None)
        assert rc != 0 and frag in lib.egx_last_error(), (frag, lib.egx_last_error())

    refused(b"null pointer", w=None)
    refused(b"null pointer", out=None)
    refused(b"null scratch", scratch=None)
    refused(b"L = 0", L=0)
    refused(b"S = 0", S=0)
    refused(b"S = 513", S=513)
    refused(b"B = -2", B=-2)
    refused(b"segment table", seg=PTR, K=3)
    refused(b"K = 17", seg=PTR, segtab=PTR, K=17)
    assert lib.egx_launch_count(0) == 0
    one = (2 * 45 * 45 * 4 + 255) // 256 * 256
    assert lib.egx_attention_rollout_scratch(1, 2, 45) == 0 and lib.egx_attention_rollout_scratch(2, 2, 45) == one
    assert lib.egx_attention_rollout_scratch(3, 2, 45) == lib.egx_attention_rollout_scratch(6, 2, 45) == 2 * one


def _cfg(d=128, h=4, dff=2048, L=1, nseg=3, compute=2, impl=0, p=(0.0, 0.0, 0.0)):
    from egot2_amd._lib import Config
    return Config(d, h, dff, L, nseg, 1e-5, compute, impl, p[0], p[1], p[2])


def _segs(n=3, T=15, d_in=256):
    from egot2_amd._lib import Segment
    segs = (Segment * n)()
    for i in range(n):
        segs[i].T, segs[i].d_in, segs[i].proj_w = T, d_in, PTR
    return segs


def test_the_encoder_entry_refuses_on_the_host(egx_lib):
    lib = egx_lib
    lib.egx_launch_count(1)

    def refused(frag, cfg=None, segs=None, B=4, lengths=None, saved=PTR, mask=1, w=PTR, seg=PTR, null_cfg=False):
        cfg = cfg if cfg is not None else _cfg()
        segs = segs if segs is not None else _segs()
        ln = (C.c_int * len(lengths))(*lengths) if lengths is not None else None
        rc = lib.egx_encoder_self_weights(None if null_cfg else C.byref(cfg), segs, B, ln, 2, saved, mask, w, seg, None)
        assert rc != 0 and frag in lib.egx_last_error(), (frag, lib.egx_last_error())

    refused(b"null config", null_cfg=True)
    refused(b"null pointer", saved=None)
    refused(b"null pointer", w=None, seg=None)
    for i in range(3):      # p_drop, p_pos, p_feat
        refused(b"inference only", cfg=_cfg(p=tuple(0.1 if j == i else 0.0 for j in range(3))))
    refused(b"keeps no Q | K | V", cfg=_cfg(L=0))                                # a configuration whose forward keeps none
    refused(b"layer_mask", mask=0)
    refused(b"layer_mask", mask=2)                                               # layer 1 of a one-layer encoder
    refused(b"head dim 8", cfg=_cfg(d=128, h=16))
    # the d = 2048 recipe: 8 heads of 256 on the wide path (bf16)
    refused(b"head dims 256 / 512", cfg=_cfg(d=2048, h=8, dff=2048, nseg=1, compute=1), segs=_segs(1, 8, 2048))
    refused(b"S = 600", cfg=_cfg(d=256, h=8, nseg=1, compute=0), segs=_segs(1, 600, 256))
    # ragged batches on the wide path (d = 256, bf16)
    refused(b"ragged batches are served on the d = 128 kernels only", cfg=_cfg(d=256, h=8, nseg=1, compute=1), segs=_segs(1, 16, 256),
            lengths=[16, 3, 7, 9])
    # a ragged d = 128 batch with a length outside the padded one: the ragged plan's own text
    refused(b"ragged batch", lengths=[15, 15, 15] * 3 + [15, 16, 15])
    assert lib.egx_launch_count(0) == 0


# ---- the Python refusals: before any library call ----
def _ttm(L=1):
    from egot2_amd import hhi_ttm
    from tests.util import hhi_args
    return hhi_ttm.TaskFusionMFTransformer3Task(hhi_args(num_layers=L))


def test_record_attention_refuses_train_mode_autograd_and_over_budget(monkeypatch):
    from egot2_amd import _lib, functional as F_egx
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was called")))
    m = _ttm()
    feats = [torch.zeros(4, 15, 256)] * 3
    with pytest.raises(ValueError, match="inference-only.*model.eval"):
        with m.train().record_attention():
            pass
    m.eval()
    with pytest.raises(ValueError, match="inference-only.*no_grad"):          # eval mode, but an autograd graph over the parameters
        with m.record_attention():
            pass
    with torch.no_grad():
        with m.record_attention() as rec:
            m.train()
            with pytest.raises(ValueError, match="inference-only"):           # switched to train mode inside the context
                m.forward_features(*feats)
            m.eval()
        # B = 4, S = 45, K = 3, one layer: 4 * 45 * 45 * 4 = 32400 bytes of weights + 4 * 45 * 3 * 4 = 2160 of segment shares
        with m.record_attention(max_bytes=34559) as rec:
            with pytest.raises(ValueError, match=r"B = 4, S = 45, K = 3, 1 of 1 layers need 34560 bytes of outputs and 0 bytes of scratch.*34559"):
                m.forward_features(*feats)
        assert rec.records == []
        with m.record_attention(weights=False, max_bytes=2159):
            with pytest.raises(ValueError, match="2160 bytes of outputs"):
                m.forward_features(*feats)
        with m.record_attention(rollout=True, max_bytes=69119):                 # + rollout (32400 + 2160), no scratch with one layer
            with pytest.raises(ValueError, match="69120 bytes of outputs and 0 bytes of scratch"):
                m.forward_features(*feats)
        m2 = _ttm(L=2)
        m2.eval()
        with m2.record_attention(rollout=True, layers=[1], max_bytes=10 ** 5):  # one layer returned, both computed: a (2, B, S, S) temporary + one product
            with pytest.raises(ValueError, match="1 of 2 layers need 69120 bytes of outputs and 97200 bytes of scratch"):
                m2.forward_features(*[torch.zeros(4, 15, 256)] * 3)
        with m2.record_attention(layers=[2]):
            with pytest.raises(ValueError, match=r"layers = \(2,\) but the encoder has 2 layers"):
                m2.forward_features(*[torch.zeros(4, 15, 256)] * 3)
        with m.record_attention():
            with pytest.raises(ValueError, match="1..512 tokens"):             # S = 3 * 171 = 513
                m.forward_features(*[torch.zeros(1, 171, 256)] * 3)
    for bad in (dict(weights=False, by_segment=False), dict(layers=[]), dict(layers=[1, 0]), dict(layers=[0, 0]), dict(layers=[-1])):
        with pytest.raises(ValueError):
            with torch.no_grad(), m.record_attention(**bad):
                pass
    assert F_egx._attention_sink is None and getattr(m, "_egx_recorder", None) is None      # nothing stays installed


def test_unserved_encoders_are_refused_with_a_text(monkeypatch):
    from types import SimpleNamespace as NS
    from egot2_amd import _lib, hoi_pnr
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was called")))
    vit = hoi_pnr.TaskFusionMFTransformer(NS(DATA=NS(TASK="keyframe_localization"), PRETRAIN=NS(PNR_CFG=None, OSCC_CFG=None))).eval()
    with torch.no_grad(), vit.record_attention():
        with pytest.raises(ValueError, match="pre-LN simple_vit encoder.*not served"):
            vit.forward_features(torch.zeros(2, 16, 8192), torch.zeros(2, 16, 8192))
    from egot2_amd import hhi_multitask
    g = hhi_multitask.TaskTranslationPromptTransformer(NS(hidden_dim=256, num_heads=4, num_layers=1, dropout=0.0, lam_checkpoint=None,
                                                          ttm_checkpoint=None, asd_checkpoint=None), er.HHI_VOCAB).eval()
    with torch.no_grad(), g.record_attention():
        with pytest.raises(ValueError, match="ragged batch on the wide path.*not served"):
            g.encode_features("ttm", *[torch.zeros(2, 15, 256)] * 3, lengths=[15, 7])


def test_primitive_validation_raises_before_any_library_call():
    from egot2_amd import functional as F_egx
    with pytest.raises(ValueError, match="head dims"):
        F_egx.check_self_weights(48, 45)
    with pytest.raises(ValueError, match="513 tokens"):
        F_egx.check_self_weights(32, 513)
    F_egx.check_self_weights(96, 512, 16)
    with pytest.raises(ValueError, match="17 segments"):
        F_egx.check_self_weights(32, 45, 17)


# ---- the conditions of the bars ----
@pytest.mark.parametrize("H,dh", er.PRIM_SHAPES)
def test_bar_of_the_primitive_is_a_condition(H, dh):
    """The kernel-level bar on item 1's own inputs: stock fp32 torch (another summation order than the kernel's) stays below bar / 8 against
    fp64 on every case, or, where the case is listed in YARDSTICK_ABOVE, at its listed yardstick (the case's bar is 8 x that). The uniform
    answer misses every case's bar by 4 x at least (S > 1)."""
    worst = 0.0
    for key, q, k, B, S, first, lengths in er.primitive_layout_cases(H, dh):
        ref = er.ref_weights(q, k, H, B, S, first, lengths)
        y = (er.ref_weights(q, k, H, B, S, first, lengths, dtype=torch.float32).double() - ref).abs().max().item()
        worst = max(worst, y)
        assert y <= er.kernel_bar(key) / 8, (key, y)
        if S > 1:
            n = S if lengths is None else max(lengths)
            live = ref[:, :n, :n] if lengths is None else ref[lengths.index(n), :n, :n]
            assert (live - 1.0 / n).abs().max().item() > 4 * er.kernel_bar(key), key
    print(f"H = {H}, dh = {dh}: worst fp32 yardstick {worst:.2e}")
    assert all(er.kernel_bar(k) >= er.BAR_KERNEL for k in er.YARDSTICK_ABOVE)


def test_bar_of_the_rollout_is_a_condition():
    for L, B, S in er.rollout_cases():
        w = er.rollout_inputs(L, B, S)
        ref = er.rollout(w.double())
        y = (er.rollout(w).double() - ref).abs().max().item()
        assert y <= er.kernel_bar(("rollout", L, S)) / 8, (L, S, y)
        if L > 1 and S > 1:     # the two perturbations of the rollout miss the bar on every case
            for kw in (dict(reverse=True), dict(identity=False)):
                assert (er.rollout(w.double(), **kw) - ref).abs().max().item() > 4 * er.kernel_bar(("rollout", L, S)), (L, S, kw)
        elif S > 1:
            assert (er.rollout(w.double(), identity=False) - ref).abs().max().item() > 4 * er.kernel_bar(("rollout", L, S))


@pytest.mark.parametrize("name", list(er.ALL_CASES))
def test_model_bars_are_conditions_and_reject_the_perturbed_references(name):
    """Per named model case: s >= 0.02; the oracle on bf16-rounded in_proj weights and layer inputs keeps e < s / 16 (the bf16 paths have a
    4 x margin to e < s / 4); the fp32 oracle is far inside the bar; and every perturbed reference misses its bar: the weights' perturbations
    the model-level bar s / 4, the segment shares' and the rollout's the kernel-level bar that holds them to the call's own weights."""
    w, seg, R, Rs, table = er.case_oracle(name)
    L, B, S, _ = w.shape
    uni = er.uniform_answer(L, table, S)
    s = [(a - b).abs().max().item() for a, b in zip((w, seg, R, Rs), uni)]
    assert min(s) >= er.S_MIN, s
    assert (w.sum(-1) - 1).abs().max().item() < 1e-12 and (seg.sum(-1) - 1).abs().max().item() < 1e-12
    assert (R.sum(-1) - 1).abs().max().item() < 1e-12
    e16 = (er.case_variant(name, round_bf16=True) - w).abs().max().item()
    e32 = (er.case_variant(name, dtype=torch.float32) - w).abs().max().item()
    print(f"[{name}] s = {s[0]:.3e} (segments {s[1]:.3e}, rollout {s[2]:.3e}), bf16-rounded oracle e = {e16:.3e}, fp32 oracle e = {e32:.3e}")
    assert e16 < s[0] / 16 and 0 < 8 * e32 < s[0] / 4
    # the derived quantities from given weights in fp32 (torch): inside the kernel-level yardstick
    w32 = w.float()
    assert (er.segment_sums(w32, table).double() - er.segment_sums(w32.double(), table)).abs().max().item() < er.YARDSTICK
    assert (er.rollout(w32).double() - er.rollout(w32.double())).abs().max().item() < er.YARDSTICK
    pert = er.perturbed(name)
    expect = {"softmax of the head-mean score", "no 1/sqrt(dh)", "rollout without identity"}
    if L > 1:
        expect |= {"neighbouring layer", "rollout in reverse order"}
    if table.shape[1] > 1:
        expect |= {"segment boundary shifted"}
    assert set(pert) == expect
    for what, (a, b, qi) in pert.items():
        e = (a - b).abs().max().item()
        bar = s[0] / 4 if qi == 0 else er.BAR_KERNEL
        assert e > bar, (name, what, e, bar)
        if qi == 0:
            with pytest.raises(AssertionError):
                er.model_bar(a, b, uni[0] if b.dim() == 4 else uni[0][0], what)
