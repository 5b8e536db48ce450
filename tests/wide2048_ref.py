"""Shared helpers of tests/test_cpu_wide2048.py and tests/test_gpu_wide2048.py: the 2048-wide HOI LTA 2-task translator
(HOI/configs/lta/ts_lta_2task.yaml:79-82: d = 2048, 4 heads of 512, one layer, dropout 0.5, two streams of NUM_INPUT_CLIPS = 2 clips; the config
defaults' 8 heads give head dim 256) on the wide bf16 path.

Two references, both oracle/translator_ref.py in fp64:
    E   the exact oracle on the weights and features as they are;
    R   the same oracle on weights and features rounded to bf16 and back — what the bf16 path multiplies with. Every floating tensor of the
        state dict and both feature streams are rounded, as the issue's measurement of R against E did (table below).
The device model of the GPU tests HOLDS those rounded values (make_model(rounded=True), bf16_round on the features): R rounds every tensor,
also the ones the wide path keeps in fp32 (identity-segment features into the shared LayerNorm, biases, LayerNorm parameters, `pe`), so
only with the rounded values loaded is R the exact function of what the device multiplies with, and device-vs-R the device's own
arithmetic error. Measured on an MI355X at the recipe (n = 2, heads 4, L = 1, B = 3, p = 0.5): with the unrounded values on the device the
worst gradient is 6.4e-2 from R (in_proj_weight; 4.1e-2 from E), with the rounded values 2.7e-2 (linear1.weight); at p = 0 4.7e-2 against
3.6e-2. E stays the oracle on the unrounded values.
The model-level GPU tests assert against R at the wide path's own bars (tests/test_gpu_wide.py: outputs 1e-2 * max(1, |ref|), per-parameter
relative gradient error 6e-2): R alone already differs from E by most of the gradient bar (ReLU pre-activations that change sign under the
parameter rounding), so a bar against E would leave no room for the device's activation roundings. Measured on the CPU (B = 3, weight seed
33, feature seed 40, p = 0; tests/test_cpu_wide2048.py prints and records them):

    case            outputs   worst gradient (linear1.weight)
    n = 2, h = 4    3.6e-3    5.1e-2
    n = 2, h = 8    4.4e-3    5.2e-2
    n = 8, h = 4    5.1e-3    4.1e-2
"""
from __future__ import annotations

import os
from types import SimpleNamespace as NS

import torch

from oracle import translator_ref as tr
from tests.util import seeded_feats, seeded_state_dict

OUT_BAR, GRAD_BAR = 1e-2, 6e-2          # tests/test_gpu_wide.py: test_c4_real_dimensions_bf16_on_wide_path
W_SEED, F_SEED, B_SMALL = 33, 40, 3
CLASSES = (5, 7)
RE_CASES = [(2, 4), (2, 8), (8, 4)]     # (n, heads) at d = 2048, one layer: the issue's table
REPORT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "wide2048_report.txt")


def lta_cfg(n, d, heads, layers, p=0.0, nz=3, classes=CLASSES):
    """tests/test_gpu_wide.py _lta_cfg with the translator's dropout as an argument."""
    return NS(FORECASTING=NS(NUM_INPUT_CLIPS=n, NUM_ACTIONS_TO_PREDICT=nz),
              MODEL=NS(TRANSLATION_HEADS=heads, TRANSLATION_LAYERS=layers, TRANSLATION_INPUT_FEATURES=d, TRANSLATION_DROPOUT=p,
                       NUM_CLASSES=list(classes), DROPOUT_RATE=0.0, HEAD_ACT="softmax"), TEST=NS(NO_ACT=False))


def lta2_masked(sd, h, feat_action, feat_lta, classes, masks=None, perturb=None):
    """tr.lta2_forward with the dropout masks threaded through: tr.hoi_tokens, tr.encoder(..., masks), the token mean and the head
    projections. masks: None (eval / p = 0) or tests/dropmask.encoder_masks(...).
    perturb (the CPU self-test of the gate): "scale256" computes the scores with the attention scale of head dim 256 whatever the head dim
    (q pre-multiplied), "no_pe" leaves the learned positions out."""
    sd = dict(sd)
    d = sd["ln.weight"].shape[0]
    n_layers = tr.n_layers_of(sd, "transformer.")
    if perturb == "no_pe":
        sd["pe"] = torch.zeros_like(sd["pe"])
    elif perturb == "scale256":
        f = (d // h / 256.0) ** 0.5           # scores / sqrt(dh) * f = scores / sqrt(256)
        for i in range(n_layers):
            w, b = sd[f"transformer.layers.{i}.self_attn.in_proj_weight"].clone(), sd[f"transformer.layers.{i}.self_attn.in_proj_bias"].clone()
            w[:d] *= f
            b[:d] *= f
            sd[f"transformer.layers.{i}.self_attn.in_proj_weight"], sd[f"transformer.layers.{i}.self_attn.in_proj_bias"] = w, b
    elif perturb is not None:
        raise ValueError(perturb)
    x = tr.hoi_tokens(sd, [feat_action, feat_lta], [None, "proj_lta" if "proj_lta.weight" in sd else None], masks)
    x = tr.encoder(x, sd, "transformer.", n_layers, h, masks)
    pooled = x.mean(dim=1)
    z, outs = 0, []
    while f"head.projections.{z}.weight" in sd:
        outs.append(tr.linear(pooled, sd[f"head.projections.{z}.weight"], sd[f"head.projections.{z}.bias"]))
        z += 1
    return list(torch.split(torch.stack(outs, dim=1), list(classes), dim=-1))


def bf16_round(t):
    return t.float().bfloat16().to(t.dtype) if t.is_floating_point() else t


def lin(t):
    return (t * torch.linspace(-1, 1, t.numel(), device=t.device, dtype=t.dtype).view_as(t)).sum()


def make_model(n, d, heads, layers, p=0.0, seed=W_SEED, rounded=False):
    """(model on the CPU with the seeded weights loaded, its state dict). rounded: the model holds the bf16-rounded weights, the values R is
    evaluated on; the state dict returned is the unrounded one either way."""
    from egot2_amd import hoi_lta
    m = hoi_lta.TaskFusionMFTransformer2Task(lta_cfg(n, d, heads, layers, p))
    sd = seeded_state_dict(m, seed)
    m.load_state_dict({k: bf16_round(v) for k, v in sd.items()} if rounded else sd)
    return m, sd


def make_feats(B, n, d, seed=F_SEED):
    return seeded_feats(seed, [(B, n, d), (B, n, 2048)])


def oracle(sd, heads, feats, rounded, masks=None, grads=True, perturb=None):
    """The fp64 oracle: E (rounded False) or R (rounded True). -> (outputs [verbs, nouns] detached, {parameter: gradient of
    lin(verbs) + lin(nouns)} or None)."""
    rd = bf16_round if rounded else (lambda t: t)
    sd64 = {k: rd(v).double().requires_grad_(grads and v.is_floating_point()) for k, v in sd.items()}
    outs = lta2_masked(sd64, heads, *[rd(f).double() for f in feats], CLASSES, masks, perturb)
    g = None
    if grads:
        (lin(outs[0]) + lin(outs[1])).backward()
        g = {k: v.grad for k, v in sd64.items() if v.grad is not None}
    return [o.detach() for o in outs], g


def out_err(outs, ref):
    """max over both outputs of |o - r| / max(1, max |r|): the quantity the 1e-2 bar bounds."""
    return max((o.detach().cpu().double() - r).abs().max().item() / max(1.0, r.abs().max().item()) for o, r in zip(outs, ref))


def grad_errs(grads, ref):
    """{parameter: relative L2 error} over the parameters the reference has a gradient for. grads: {name: tensor}."""
    return {k: (grads[k].detach().cpu().double() - r).norm().item() / (r.norm().item() + 1e-12) for k, r in ref.items()}


_RECORDS = {}


def record(section, lines):
    """Keep `lines` as `section` of profiles/wide2048_report.txt (sections of one process are written together, the other sections
    of the file are kept)."""
    _RECORDS[section] = list(lines)
    old = {}
    if os.path.exists(REPORT):
        cur = None
        for ln in open(REPORT).read().splitlines():
            if ln.startswith("## "):
                cur = ln[3:].strip()
                old[cur] = []
            elif cur is not None:
                old[cur].append(ln)
    old.update(_RECORDS)
    try:
        _write(old)
    except OSError as e:          # a read-only checkout: the figures are still printed by the caller
        print(f"wide2048 report not written: {e}")


def _write(old):
    with open(REPORT, "w") as f:
        f.write("# d_model 2048 on the wide bf16 path: measured errors and times (tests/test_cpu_wide2048.py, tests/test_gpu_wide2048.py,\n"
                "# tools/wide2048_eval.py). E: fp64 oracle; R: the oracle on bf16-rounded weights and features.\n")
        for sec in sorted(old):
            body = [ln for ln in old[sec] if ln.strip()]
            f.write(f"\n## {sec}\n" + "\n".join(body) + "\n")
