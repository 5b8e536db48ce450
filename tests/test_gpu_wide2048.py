"""-m gpu: d_model up to 2048 on the wide bf16 path — the 2048-wide HOI LTA 2-task translator (HOI/configs/lta/ts_lta_2task.yaml:79-82:
4 heads of 512 over S = 4 tokens, dropout 0.5; the config defaults' 8 heads: head dim 256).

Operator level: the attention class for head dim 256 / 512 over S <= 16 tokens (csrc/wide_attn_bighead.hip) through egx_wide_attention_fwd /
_bwd against fp64 autograd on the bf16-rounded operands, tests/test_gpu_wide.py test_wide_attention_fwd_bwd's method and bars.
Model level: TaskFusionMFTransformer2Task against R, the fp64 oracle on bf16-rounded weights and features (tests/wide2048_ref.py says why R
and not the exact oracle E; the distance to E is printed beside it), at the wide path's bars: outputs 1e-2 * max(1, |ref|), every parameter
gradient 6e-2 relative. The measured errors go to profiles/wide2048_report.txt."""
import pytest
import torch

from tests import dropmask as dm
from tests import wide2048_ref as w
from tests.test_gpu_wide import _attn_ref, _ptr, _stream

pytestmark = pytest.mark.gpu
_OPERATOR_LINES = []


# ---- 1: the operator ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S,H,d", [(3, 4, 4, 2048),       # the recipe: head dim 512, S = 4
                                     (2, 16, 4, 2048),      # a full tile
                                     (2, 1, 8, 2048),       # one token, head dim 256
                                     (5, 5, 8, 2048),       # a ragged tile; 40 (clip, head) waves
                                     (1, 16, 2, 1024)])     # head dim 512 at another d; two waves: a partial workgroup
def test_bighead_attention_fwd_bwd(egx_lib, cuda, B, S, H, d):
    g = torch.Generator().manual_seed(S * 7 + d)
    qkv = torch.randn(B * S, 3 * d, generator=g).to(cuda).bfloat16()
    d_out = torch.randn(B * S, d, generator=g).to(cuda).bfloat16()
    out, out2 = (torch.full((B * S, d), float("nan"), device=cuda, dtype=torch.bfloat16) for _ in range(2))
    lse, lse2 = (torch.full((B, H, S), float("nan"), device=cuda) for _ in range(2))
    dqkv = torch.full((B * S, 3 * d), float("nan"), device=cuda, dtype=torch.bfloat16)
    assert egx_lib.egx_wide_attention_fwd(_ptr(qkv), _ptr(out), _ptr(lse), B, S, H, d, 0.0, 0, _stream()) == 0, egx_lib.egx_last_error()
    assert egx_lib.egx_wide_attention_bwd(_ptr(qkv), _ptr(out), _ptr(lse), _ptr(d_out), _ptr(dqkv), None, B, S, H, d, 0.0, 0, _stream()) == 0, egx_lib.egx_last_error()
    assert egx_lib.egx_wide_attention_fwd(_ptr(qkv), _ptr(out2), _ptr(lse2), B, S, H, d, 0.0, 0, _stream()) == 0, egx_lib.egx_last_error()
    ro, rl, rg = _attn_ref(qkv, d_out, B, S, H, d)
    e_lse = (lse.double() - rl).abs().max().item() / max(1.0, rl.abs().max().item())
    e_out = (out.double() - ro).abs().max().item() / ro.abs().max().item()
    finite = torch.isfinite(dqkv.float()).all().item()
    e_g = (dqkv.double() - rg).norm().item() / rg.norm().item() if finite else float("nan")
    line = f"(B, S, H, d) = ({B}, {S}, {H}, {d}): lse {e_lse:.3e} (bar 2e-3) out {e_out:.3e} (1.5e-2) d_qkv {e_g:.3e} (1.5e-2)"
    print("WIDE2048 operator", line)
    _OPERATOR_LINES.append(line)
    w.record("gpu operator: egx_wide_attention_fwd / _bwd against fp64 autograd on the bf16-rounded operands", _OPERATOR_LINES)
    assert e_lse < 2e-3
    assert e_out < 1.5e-2                                   # P and O rounded to bf16
    assert finite                                           # every element written
    assert e_g < 1.5e-2, e_g
    assert torch.equal(out, out2) and torch.equal(lse, lse2)        # bit-reproducible


# ---- 2: the operator's refusal ----------------------------------------------------------------------------------------------------------------
def test_bighead_attention_refuses_longer_sequences(egx_lib, cuda):
    B, S, H, d = 2, 17, 4, 2048
    qkv = torch.zeros(B * S, 3 * d, device=cuda, dtype=torch.bfloat16)
    out = torch.zeros(B * S, d, device=cuda, dtype=torch.bfloat16)
    lse = torch.zeros(B, H, S, device=cuda)
    dqkv = torch.zeros_like(qkv)
    egx_lib.egx_launch_count(1)
    for rc in (egx_lib.egx_wide_attention_fwd(_ptr(qkv), _ptr(out), _ptr(lse), B, S, H, d, 0.0, 0, _stream()),
               egx_lib.egx_wide_attention_bwd(_ptr(qkv), _ptr(out), _ptr(lse), _ptr(out), _ptr(dqkv), None, B, S, H, d, 0.0, 0, _stream())):
        err = egx_lib.egx_last_error().decode()
        assert rc != 0
        assert all(t in err for t in ("S=17", "S <= 16", "256 / 512")), err
    assert egx_lib.egx_launch_count(0) == 0


# ---- the model ------------------------------------------------------------------------------------------------------------------------------
def _run(model, feats, cuda):
    """One training step's worth: (outputs, {parameter: gradient}) of lin(verbs) + lin(nouns). The model holds the bf16-rounded weights
    (make_model(rounded=True)) and is fed the bf16-rounded features: the values R is evaluated on (tests/wide2048_ref.py)."""
    model.zero_grad(set_to_none=True)
    outs = model.forward_features(*[w.bf16_round(f).to(cuda) for f in feats])
    (w.lin(outs[0]) + w.lin(outs[1])).backward()
    torch.cuda.synchronize()
    return [o.detach().clone() for o in outs], {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


def _compare(tag, outs, grads, sd, heads, feats, masks=None):
    """Assert against R at the wide path's bars; the distance to E is printed beside it and both are recorded."""
    ro, rg = w.oracle(sd, heads, feats, rounded=True, masks=masks)
    eo, eg = w.oracle(sd, heads, feats, rounded=False, masks=masks)
    assert set(rg) <= set(grads), sorted(set(rg) - set(grads))
    nonfinite = sorted(k for k, g in grads.items() if not torch.isfinite(g).all())
    assert not nonfinite and all(torch.isfinite(o).all() for o in outs), f"{tag}: non-finite outputs or gradients {nonfinite}"
    o_r, o_e = w.out_err(outs, ro), w.out_err(outs, eo)
    g_r, g_e = w.grad_errs(grads, rg), w.grad_errs(grads, eg)
    kr, ke = max(g_r, key=g_r.get), max(g_e, key=g_e.get)
    line = (f"{tag}: outputs vs R {o_r:.3e} (bar {w.OUT_BAR:g}) vs E {o_e:.3e}; worst gradient vs R {g_r[kr]:.3e} ({kr}, bar {w.GRAD_BAR:g}) "
            f"vs E {g_e[ke]:.3e} ({ke})")
    print("WIDE2048 model", line)
    w.record(f"gpu model: {tag}", [line])
    assert o_r < w.OUT_BAR, line
    bad = {k: v for k, v in g_r.items() if not v < w.GRAD_BAR}
    assert len(g_r) >= 16 and not bad, bad


@pytest.mark.parametrize("n,d,heads,L", [(2, 2048, 4, 1),         # the recipe
                                         (8, 2048, 8, 2),         # head dim 256, a full 16-token tile, two layers
                                         (4, 1536, 12, 1)])       # six float4 per lane in the LayerNorm instance; head dim 128: the S <= 128 attention
def test_lta2_wide_train_mode_against_the_rounded_oracle(egx_lib, cuda, n, d, heads, L):
    from egot2_amd import functional as F_egx
    m, sd = w.make_model(n, d, heads, L, rounded=True)
    m = m.to(cuda).set_compute("bf16").train()
    feats = w.make_feats(w.B_SMALL, n, d)
    outs, grads = _run(m, feats, cuda)
    assert F_egx.last_encoder_impl() == "wide"
    _compare(f"p = 0, train mode, B = {w.B_SMALL}, n = {n}, d = {d}, heads = {heads}, L = {L}", outs, grads, sd, heads, feats)


def test_lta2_recipe_dropout_matches_the_rounded_oracle_under_the_same_masks(egx_lib, cuda):
    """The recipe's dropout 0.5 on all four encoder-layer sites: the masks the call drew (tests/dropmask.py, the wide path's S <= 128 keying:
    attention rows (b * H + h) * 128 + query) handed to the oracle; two runs under one seed are bit-equal."""
    from egot2_amd import functional as F_egx
    n, d, heads, L, p, seed = 2, 2048, 4, 1, 0.5, 0x2048 + 4
    m, sd = w.make_model(n, d, heads, L, p, rounded=True)
    m = m.to(cuda).set_compute("bf16").train()
    m._egx_seed = lambda: seed              # host-seed path: every forward draws its keys from `seed` (tests/test_gpu_dropout_parity.py _pin_seed)
    feats = w.make_feats(w.B_SMALL, n, d)
    outs, grads = _run(m, feats, cuda)
    assert F_egx.last_encoder_impl() == "wide"
    masks = dm.encoder_masks(seed, "wide", 3, [2, 2], 2048, 4, 2048, 1, 0.5)
    _compare(f"p = 0.5 (the recipe), train mode, B = {w.B_SMALL}, n = {n}, d = {d}, heads = {heads}, L = {L}", outs, grads, sd, heads, feats, masks)
    ev, _ = w.oracle(sd, heads, feats, rounded=True, grads=False)
    assert w.out_err(outs, ev) > 10 * w.OUT_BAR            # and the masks matter: the eval-mode oracle is far away
    outs2, grads2 = _run(m, feats, cuda)
    assert all(torch.equal(a, b) for a, b in zip(outs, outs2))
    for k in grads:
        if k.startswith("head."):       # MultiTaskHead runs on the generic linear kernels, whose bias-gradient sums meet in atomics
            assert torch.allclose(grads[k], grads2[k], rtol=1e-4, atol=1e-6), k
        else:
            assert torch.equal(grads[k], grads2[k]), k


def test_lta2_recipe_at_batch_size_against_the_rounded_oracle_on_sampled_clips(egx_lib, cuda):
    """B = 256 (64 workgroups of the attention, the GEMMs' full-size grids), eval mode: the outputs of 8 sampled clips against R on those
    clips alone (clips are independent units). TEST.NO_ACT leaves the head's softmax out, so the outputs are the logits the oracle returns."""
    from egot2_amd import functional as F_egx
    from egot2_amd import hoi_lta
    from tests.util import seeded_state_dict
    B, n, d, heads = 256, 2, 2048, 4
    pick = [0, 1, 37, 101, 128, 200, 254, 255]
    cfg = w.lta_cfg(n, d, heads, 1, 0.5)
    cfg.TEST.NO_ACT = True
    m = hoi_lta.TaskFusionMFTransformer2Task(cfg)
    sd = seeded_state_dict(m, w.W_SEED)
    m.load_state_dict({k: w.bf16_round(v) for k, v in sd.items()})
    m = m.to(cuda).set_compute("bf16").eval()
    feats = w.make_feats(B, n, d, seed=w.F_SEED + 1)
    with torch.no_grad():
        outs = m.forward_features(*[w.bf16_round(f).to(cuda) for f in feats])
    torch.cuda.synchronize()
    assert F_egx.last_encoder_impl() == "wide"
    sub = [f[pick] for f in feats]
    ro, _ = w.oracle(sd, heads, sub, rounded=True, grads=False)
    eo, _ = w.oracle(sd, heads, sub, rounded=False, grads=False)
    got = [o[pick] for o in outs]
    line = f"eval mode, B = {B}, n = {n}, d = {d}, heads = {heads}, 8 sampled clips: outputs vs R {w.out_err(got, ro):.3e} (bar {w.OUT_BAR:g}) vs E {w.out_err(got, eo):.3e}"
    print("WIDE2048 model", line)
    w.record("gpu model: the recipe at batch size", [line])
    assert w.out_err(got, ro) < w.OUT_BAR, line


@pytest.mark.parametrize("S,H,d", [(16, 2, 512), (5, 2, 1024)])
def test_bighead_attention_dropout_is_consistent(egx_lib, cuda, S, H, d):
    """p > 0 at head dim 256 and 512: the backward regenerates the forward's mask (tests/test_gpu_wide.py
    test_wide_attention_dropout_is_consistent's method: with V := 1 the output is the row sum of the dropped probabilities, with dO := 1 dV
    is their column sum; both sum to the same total per (clip, head), and the keep rate is 1 - p)."""
    B, p = 8, 0.25
    g = torch.Generator().manual_seed(11 + S)
    qkv = torch.randn(B * S, 3 * d, generator=g).to(cuda).bfloat16()
    qkv[:, 2 * d:] = 1.0
    out = torch.empty(B * S, d, device=cuda, dtype=torch.bfloat16)
    lse = torch.empty(B, H, S, device=cuda)
    assert egx_lib.egx_wide_attention_fwd(_ptr(qkv), _ptr(out), _ptr(lse), B, S, H, d, p, 1234, _stream()) == 0, egx_lib.egx_last_error()
    rowsum = out.float()[:, ::d // H]              # one column per head: sum_k P_drop[q, k]
    assert abs(rowsum.mean().item() - 1.0) < 0.1 and rowsum.std().item() > 0.01
    d_out = torch.ones(B * S, d, device=cuda, dtype=torch.bfloat16)
    dqkv = torch.full((B * S, 3 * d), float("nan"), device=cuda, dtype=torch.bfloat16)
    assert egx_lib.egx_wide_attention_bwd(_ptr(qkv), _ptr(out), _ptr(lse), _ptr(d_out), _ptr(dqkv), None, B, S, H, d, p, 1234, _stream()) == 0, egx_lib.egx_last_error()
    assert torch.isfinite(dqkv.float()).all()
    dv = dqkv.float()[:, 2 * d::d // H].view(B, S, H)
    assert torch.allclose(dv.sum(1), rowsum.view(B, S, H).sum(1), rtol=2e-2, atol=2e-2)
