"""CPU suite: the oracle restatement (oracle/translator_ref.py) and the stock-module CPU baseline against the golden
fixtures generated from the REAL reference classes (tests/golden/make_golden.py), plus the recorded outputs of the reference
class on seeds of their own (tests/golden/live/)."""
import glob
import json
import os

import numpy as np
import pytest
import torch

from oracle import translator_ref as tr
from tests.util import hhi_args, seeded_feats, seeded_state_dict

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
CE_W = [0.266, 0.734]


def load_fixture(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return json.loads(str(z["config"])), z


def build_ours(c):
    """Our (HIP-backed) module for a fixture config — used here only as the parameter container."""
    from types import SimpleNamespace as NS
    if c["kind"] == "ttm":
        from egot2_amd import hhi_ttm
        cls = hhi_ttm.TaskFusionMFTransformer3Task if c["n_tasks"] == 3 else hhi_ttm.TaskFusionMFTransformer2Task
        return cls(hhi_args(hidden_dim=c["d"], num_heads=c["h"], num_layers=c["L"]))
    if c["kind"] == "asd":
        from egot2_amd import hhi_asd
        return hhi_asd.TaskFusionMFTransformer3Task(hhi_args(hidden_dim=c["d"], num_heads=c["h"], num_layers=c["L"]))
    if c["kind"] == "hhig":
        from egot2_amd import hhi_multitask
        vocab = {'</s>': 0, '<unk>': 1, 'ttm': 2, 'lam': 3, 'asd': 4, '0': 5, '1': 6}
        return hhi_multitask.TaskTranslationPromptTransformer(hhi_args(hidden_dim=c["d"], num_heads=c["h"], num_layers=c["L"]), vocab)
    if c["kind"] == "lta4":
        from egot2_amd import hoi_lta
        cfg = NS(FORECASTING=NS(NUM_INPUT_CLIPS=c["n"], NUM_ACTIONS_TO_PREDICT=c["z"]),
                 MODEL=NS(TRANSLATION_HEADS=c["h"], TRANSLATION_LAYERS=c["L"], TRANSLATION_INPUT_FEATURES=c["d"],
                          TRANSLATION_DROPOUT=0.0, NUM_CLASSES=c["classes"], DROPOUT_RATE=0.0, HEAD_ACT="softmax"),
                 TEST=NS(NO_ACT=False))
        return hoi_lta.TaskFusionMFTransformerLTA4Task(cfg)
    if c["kind"] == "pnr3":
        from egot2_amd import hoi_pnr
        cfg = NS(DATA=NS(TASK=c["task"]),
                 MODEL=NS(TRANSLATION_INPUT_FEATURES=c["d"], TRANSLATION_LAYERS=c["L"], FEAT_DROPOUT_RATE=0.0,
                          TRANSFORMER_DROPOUT_RATE=0.0))
        return hoi_pnr.TaskFusionMFTransformer3TaskDropout(cfg)
    if c["kind"] == "hoig":
        from egot2_amd import hoi_multitask
        from oracle.ref_harness import HOI_G_VOCAB
        return hoi_multitask.TaskTranslationPromptTransformer6Task(
            NS(hidden_dim=c["d"], num_heads=c["h"], num_layers=c["L"], dropout=0.0), HOI_G_VOCAB)
    if c["kind"] == "lta2":
        from egot2_amd import hoi_lta
        cfg = NS(FORECASTING=NS(NUM_INPUT_CLIPS=c["n"], NUM_ACTIONS_TO_PREDICT=c["z"]),
                 MODEL=NS(TRANSLATION_HEADS=c["h"], TRANSLATION_LAYERS=c["L"], TRANSLATION_INPUT_FEATURES=c["d"],
                          TRANSLATION_DROPOUT=0.0, NUM_CLASSES=c["classes"], DROPOUT_RATE=0.0, HEAD_ACT="softmax"),
                 TEST=NS(NO_ACT=False))
        return hoi_lta.TaskFusionMFTransformer2Task(cfg)
    if c["kind"] == "pnrvit":
        from egot2_amd import hoi_pnr
        return hoi_pnr.TaskFusionMFTransformer(NS(DATA=NS(TASK=c["task"])))
    if c["kind"] in ("hoig2", "hoiga"):
        from egot2_amd import hoi_multitask
        from oracle.ref_harness import HOI_G_VOCAB
        cls = hoi_multitask.TaskTranslationPromptTransformer2Task if c["kind"] == "hoig2" else hoi_multitask.TaskTranslationPromptTransformerActionTask
        return cls(NS(hidden_dim=c["d"], num_heads=c["h"], num_layers=c["L"], dropout=0.0, ff_dim=2048), HOI_G_VOCAB)
    if c["kind"] in ("ar3", "ar2"):
        from egot2_amd import hoi_ar
        cfg = NS(FORECASTING=NS(NUM_INPUT_CLIPS=c.get("n", 2), INPUT_OFFSET=0),
                 MODEL=NS(TRANSLATION_INPUT_FEATURES=c["d"], TRANSLATION_LAYERS=c["L"], TRANSLATION_HEADS=c["h"],
                          TRANSLATION_DROPOUT=0.0, NUM_CLASSES=c["classes"]))
        return (hoi_ar.TaskFusionMFTransformer3Task if c["kind"] == "ar3" else hoi_ar.TaskFusionMFTransformer2TaskAR)(cfg)
    raise KeyError(c["kind"])


def g_targets(c, task, batch, vocab_size, sy=2):
    """Decoder inputs of the EgoT2-g fixtures (same recipe as tests/golden/make_golden.py)."""
    import zlib
    rng = np.random.default_rng([c["fseed"], zlib.crc32(task.encode())])
    return torch.from_numpy(rng.integers(0, vocab_size, (batch, sy))).long()


def lta4_frames(c):
    """The raw inputs of the lta4 fixture: PNR frames (B, n, F, 8192), action (B, n, d), lta (B, n, 2048)."""
    return seeded_feats(c["fseed"], [(c["B"], c["n"], c["F"], 8192), (c["B"], c["n"], c["d"]), (c["B"], c["n"], 2048)])


def fixture_feats(c):
    B = c["B"]
    if c["kind"] == "lta4":
        # feature-level view of the reference's forward(x_lta, x_pnr): per-clip mean of the frames (encode_clips_pnr); the
        # OSCC stream of the fixture is the channel-reversed PNR stream (oracle/ref_harness.py _Flip)
        frames, action, lta = lta4_frames(c)
        return [frames.mean(2), frames.flip(-1).mean(2), action, lta]
    if c["kind"] == "pnr3":
        return seeded_feats(c["fseed"], [(B, 16, 8192), (B, 16, 8192), (B, 8, 2048), (B, 8, 256)])
    if c["kind"] == "ar3":
        return seeded_feats(c["fseed"], [(B, 8, 2048), (B, 8, 256), (B, 16, 8192), (B, 16, 8192)])
    if c["kind"] == "ar2":
        return seeded_feats(c["fseed"], [(B, 8, 2048), (B, 8, 256), (B, c["n"], 2048)])
    if c["kind"] == "hoig":
        n, d = c["n"], c["d"]
        f = seeded_feats(c["fseed"], [(B, 16, 8192), (B, 16, 8192), (B, 8, 2048), (B, 8, 256), (B, n, 1, 8192), (B, n, d), (B, n, 2048)])
        # feature-level view of the 'lta' branch: one frame per clip (its mean is itself); the OSCC stream of the fixture
        # is the channel-reversed PNR stream (oracle/ref_harness.py _Flip)
        pnr_clips = f[4][:, :, 0, :].contiguous()
        return f[:4] + [pnr_clips, pnr_clips.flip(-1).contiguous(), f[5], f[6]]
    if c["kind"] == "lta2":
        return seeded_feats(c["fseed"], [(B, c["n"], c["d"]), (B, c["n"], 2048)])
    if c["kind"] in ("pnrvit", "hoig2"):
        return seeded_feats(c["fseed"], [(B, 16, 8192), (B, 16, 8192)])
    if c["kind"] == "hoiga":
        return seeded_feats(c["fseed"], [(B, 2, c["d"]), (B, 2, c["d"])])
    return seeded_feats(c["fseed"], [(c["B"], c["T"], 256)] * c["n_tasks"])


def oracle_run(c, sd, feats, dtype=torch.float64):
    """Outputs dict + scalar loss (same loss definitions as make_golden.py) from the oracle restatement."""
    sdd = {k: v.to(dtype).requires_grad_(v.is_floating_point() and not k.endswith("pos_embed.pe")) for k, v in sd.items()}
    f = [t.to(dtype) for t in feats]
    lin = lambda t: (t * torch.linspace(-1, 1, t.numel()).to(dtype).view_as(t)).sum()  # noqa: E731
    if c["kind"] == "ttm":
        out = tr.ttm_forward(sdd, c["h"], *f)
        target = torch.from_numpy(np.random.default_rng(c["fseed"]).integers(0, 2, c["B"])).long()
        return {"out": out}, tr.weighted_ce(out, target, CE_W), sdd
    if c["kind"] == "asd":
        out = tr.asd_forward(sdd, c["h"], f[0], f[1], f[2])
        return {"out": out}, lin(out), sdd
    if c["kind"] == "hhig":
        outs, loss = {}, 0
        for task in ("lam", "ttm", "asd"):
            lamf = f[1][:, :7] if task == "lam" else f[1]
            enc = tr.hhi_g_encode(sdd, c["h"], task, lamf, f[0], f[2])
            outs[f"out_{task}"] = enc
            dec = tr.g_decode(sdd, c["h"], g_targets(c, task, enc.shape[1], 7), enc)
            outs[f"dec_{task}"] = dec
            loss = loss + lin(enc) + lin(dec)
        return outs, loss, sdd
    if c["kind"] == "lta4":
        o = tr.lta4_forward(sdd, c["h"], *f, c["classes"])
        return {"out_verb": o[0], "out_noun": o[1]}, lin(o[0]) + lin(o[1]), sdd
    if c["kind"] == "pnr3":
        out = tr.pnr3_forward(sdd, c["h"], *f)
        out = out.unsqueeze(1 if "keyframe_localization" in c["task"] else 2)
        return {"out": out}, lin(out), sdd
    if c["kind"] == "hoig":
        outs = {"out_pnr": tr.hoi_g_encode(sdd, c["h"], "pnr", *f[:4]), "out_lta": tr.hoi_g_encode(sdd, c["h"], "lta_verb", *f[4:])}
        for task, sy in (("pnr", 2), ("lta", 4)):
            enc = outs[f"out_{task}"]
            outs[f"dec_{task}"] = tr.g_decode(sdd, c["h"], g_targets(c, task, enc.shape[1], 12, sy), enc)
        return outs, sum(lin(v) for v in outs.values()), sdd
    if c["kind"] == "lta2":
        o = tr.lta2_forward(sdd, c["h"], f[0], f[1], c["classes"])
        return {"out_verb": o[0], "out_noun": o[1]}, lin(o[0]) + lin(o[1]), sdd
    if c["kind"] == "pnrvit":
        out = tr.vit_forward(sdd, 8, f[0], f[1]).unsqueeze(1 if c["task"] == "keyframe_localization" else 2)
        return {"out": out}, lin(out), sdd
    if c["kind"] == "hoig2":
        enc = tr.hoi_g2_encode(sdd, c["h"], f[0], f[1])
        outs = {"out": enc, "dec": tr.g_decode(sdd, c["h"], g_targets(c, "pnr", enc.shape[1], 12, 2), enc)}
        return outs, sum(lin(v) for v in outs.values()), sdd
    if c["kind"] == "hoiga":
        outs = {"out_lta": tr.hoi_ga_encode(sdd, c["h"], "lta_verb", f[0], f[1]),
                "out_action": tr.hoi_ga_encode(sdd, c["h"], "action_verb", f[0][:, 0:1])}
        for task, sy in (("lta", 3), ("action", 2)):
            enc = outs[f"out_{task}"]
            outs[f"dec_{task}"] = tr.g_decode(sdd, c["h"], g_targets(c, task, enc.shape[1], 12, sy), enc)
        return outs, sum(lin(v) for v in outs.values()), sdd
    if c["kind"] == "ar3":
        o = tr.ar_forward(sdd, c["h"], f, ["proj3_slow", "proj3_fast", "proj1", "proj2"])
        return {"out_verb": o[0], "out_noun": o[1]}, lin(o[0]) + lin(o[1]), sdd
    if c["kind"] == "ar2":
        o = tr.ar_forward(sdd, c["h"], f, ["proj_slow", "proj_fast", "proj_lta"])
        return {"out_verb": o[0], "out_noun": o[1]}, lin(o[0]) + lin(o[1]), sdd
    raise KeyError(c["kind"])


ALL_FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*.npz")))
HEAD_FIXTURES = [n for n in ALL_FIXTURES if n.startswith("pnrhead_")]      # row F4: the PNR / OSCC head (producer side)
FIXTURES = [n for n in ALL_FIXTURES if n not in HEAD_FIXTURES]


def check_against_fixture(z, outs, loss, grads, tol_out, tol_grad, tol_dec=None):
    """tol_dec (optional): bound for the `dec*` outputs (sequence decoder + vocabulary head on top of the encoder memory)."""
    for k, v in outs.items():
        ref = torch.from_numpy(z[k]).double()
        err = (v.detach().double().cpu() - ref).abs().max().item()
        tol = tol_dec if (tol_dec is not None and k.startswith("dec")) else tol_out
        assert err < tol * max(1.0, ref.abs().max().item()), f"{k}: max err {err}"
    ref_loss = float(z["loss"])
    assert abs(float(loss) - ref_loss) < tol_out * max(1.0, abs(ref_loss)) * 10, f"loss {float(loss)} vs {ref_loss}"
    gkeys = [k[len("gnorm/"):] for k in z.files if k.startswith("gnorm/")]
    assert set(gkeys) == set(grads), f"gradient key mismatch: {set(gkeys) ^ set(grads)}"
    for k in gkeys:
        g = grads[k].detach().double().cpu().reshape(-1)
        n_ref = float(z["gnorm/" + k])
        head = torch.from_numpy(z["ghead/" + k]).double()
        # error of the stored leading entries relative to their own size AND to the tensor's RMS gradient: leading
        # entries that are 1e-4 of the norm (the decoder's first query rows) carry the fp32 cancellation noise of the
        # reference run that produced the fixture
        typical = n_ref * (head.numel() / g.numel()) ** 0.5
        e_head = (g[:head.numel()] - head).norm().item() / (head.norm().item() + typical + 1e-12)
        e_norm = abs(g.norm().item() - n_ref) / (n_ref + 1e-12)
        assert e_norm < tol_grad and e_head < 3 * tol_grad, f"{k}: norm err {e_norm}, head err {e_head}"
        if "gfull/" + k in z.files:
            # ONE hop to the reference for every element of the large weight gradients: the fixture holds
            # g / max|g| in fp16 (2^-11 of the largest entry per element). A permutation or a dropped block past the stored
            # head that preserved norm and sum would show up here.
            scale = float(z["gfull_scale/" + k])
            full = torch.from_numpy(z["gfull/" + k].astype("float32")).double().reshape(-1) * scale
            assert full.numel() == g.numel(), k
            e_max = (g - full).abs().max().item() / scale
            e_l2 = (g - full).norm().item() / full.norm().item()
            assert e_max < max(3 * tol_grad, 2 ** -10) and e_l2 < max(tol_grad, 2 ** -10), f"{k}: full-gradient max err {e_max} (of max|g|), L2 err {e_l2}"


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_matches_reference_fixture(name):
    c, z = load_fixture(name)
    model = build_ours(c)
    ref_keys = json.loads(str(z["sd_keys"]))
    ours = {k: list(v.shape) for k, v in model.state_dict().items()}
    assert ours == ref_keys, "state_dict keys/shapes differ from the reference module"
    # through load_state_dict: modules that appear under two names (the HOI heads start with the shared `ln`) end up
    # with ONE value, exactly as in the reference
    model.load_state_dict(seeded_state_dict(model, c["wseed"]))
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    outs, loss, sdd = oracle_run(c, sd, fixture_feats(c), torch.float64)
    loss.backward()
    grads = {k: v.grad for k, v in sdd.items() if v.grad is not None}
    check_against_fixture(z, outs, loss, grads, tol_out=2e-5, tol_grad=2e-4)


def head_fixture_cases(c):
    """(tag, classes, pool, softmax dim of the eval-mode activation AFTER the projection, i.e. on (N, T', classes))"""
    return (("kf", c["classes_kf"], (1, 7, 7), 1), ("sc", c["classes_sc"], (c["T"], 7, 7), 2))


@pytest.mark.parametrize("name", HEAD_FIXTURES)
def test_oracle_head_matches_reference_fixture(name):
    """Row F4 producer side: oracle.pnr_head_forward against the REAL ResNetKeyframeLocalizationHead's recorded outputs
    (middle=True rows for kt = 1 and kt = T, the per-clip mean, projection in train and eval mode, projection gradients)."""
    c, z = load_fixture(name)
    fmap = seeded_feats(c["fseed"], [(c["N"], c["C"], c["T"], c["H"], c["W"])])[0]
    lin = lambda o: (o * torch.linspace(-1, 1, o.numel(), dtype=o.dtype).view_as(o)).sum()  # noqa: E731
    for tag, classes, pool, act_dim in head_fixture_cases(c):
        head = torch.nn.Module()
        head.projection = torch.nn.Linear(8192, classes)
        assert {k: list(v.shape) for k, v in head.state_dict().items()} == json.loads(str(z[f"sd_keys_{tag}"]))
        sd = {k: v.double().requires_grad_(True) for k, v in seeded_state_dict(head, c["wseed"]).items()}
        mid = tr.pnr_head_forward(fmap.double(), pool)
        ref_mid = torch.from_numpy(z[f"mid_{tag}"]).double()
        assert mid.shape == ref_mid.shape and (mid - ref_mid).abs().max().item() < 2e-6
        if tag == "kf":
            cm = tr.pnr_head_forward(fmap.double(), pool, clip_mean=True)
            assert (cm - torch.from_numpy(z["mid_kf_clipmean"]).double()).abs().max().item() < 2e-6
        y = tr.pnr_head_forward(fmap.double(), pool, sd["projection.weight"], sd["projection.bias"], middle=False)
        ref_y = torch.from_numpy(z[f"proj_train_{tag}"]).double()
        assert y.shape == ref_y.shape and (y - ref_y).abs().max().item() < 2e-5
        lin(y).backward()
        for k in ("projection.weight", "projection.bias"):
            g = sd[k].grad.reshape(-1)
            assert abs(g.norm().item() - float(z[f"gnorm/{tag}/{k}"])) < 2e-5 * float(z[f"gnorm/{tag}/{k}"])
            head_ref = torch.from_numpy(z[f"ghead/{tag}/{k}"]).double()
            assert (g[:head_ref.numel()] - head_ref).abs().max().item() < 2e-5 * (1.0 + head_ref.abs().max().item())
        with torch.no_grad():
            ye = tr.pnr_head_forward(fmap.double(), pool, sd["projection.weight"], sd["projection.bias"], middle=False, act_dim=act_dim)
        assert (ye - torch.from_numpy(z[f"proj_eval_{tag}"]).double()).abs().max().item() < 2e-6


def test_stock_module_matches_fixture():
    """The CPU-baseline module (oracle/stock_module.py) is the reference class minus backbones."""
    from oracle.stock_module import StockTTMTranslator
    c, z = load_fixture("ttm3_B4_T15_L1")
    m = StockTTMTranslator(3, c["d"], c["h"], dropout=0.0, num_layers=c["L"])
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == json.loads(str(z["sd_keys"]))
    m.load_state_dict(seeded_state_dict(m, c["wseed"]))
    m.train()
    m.pos_embed.dropout.p = 0.0
    feats = fixture_feats(c)
    logits = m(*feats)
    target = torch.from_numpy(np.random.default_rng(c["fseed"]).integers(0, 2, c["B"])).long()
    loss = torch.nn.functional.cross_entropy(logits, target, weight=torch.tensor(CE_W))
    loss.backward()
    check_against_fixture(z, {"out": logits}, loss, {k: p.grad for k, p in m.named_parameters()}, 2e-5, 2e-4)


def test_oracle_matches_live_reference():
    """The real class on seeds of their own (not those of the fixtures above), eval mode: its logits were recorded by
    tests/golden/make_golden.py into golden/live/ttm3_eval_B5_T17_L2.npz; the weights are re-derived from the seed on the stock
    module, whose state_dict keys and shapes must be the reference's."""
    from oracle.stock_module import StockTTMTranslator
    c, z = load_fixture(os.path.join("live", "ttm3_eval_B5_T17_L2"))
    m = StockTTMTranslator(c["n_tasks"], c["d"], c["h"], num_layers=c["L"])
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == json.loads(str(z["sd_keys"]))
    m.load_state_dict(seeded_state_dict(m, c["wseed"]))
    feats = seeded_feats(c["fseed"], [(c["B"], c["T"], 256)] * c["n_tasks"])
    sd = {k: v.detach() for k, v in m.state_dict().items()}
    out = tr.ttm_forward(sd, c["h"], *feats)
    ref = torch.from_numpy(z["out"])
    assert out.shape == ref.shape and (out - ref).abs().max().item() < 1e-5
