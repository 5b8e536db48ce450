#!/usr/bin/env python3
"""Records live/seqdec_*.npz: `forward`, `predict` and, for ForecastingEncoderSeqDecoder, the 40-step `predict` loop (every step's last-row
logits, the fed-back tokens and the top-2 margins) of the REAL LTA sequence-decoder classes (HOI/models/lta/lta_models_seqdecoder.py:65-240,
lta_models_lta_transfer.py:531-659) in fp64, on seeded weights and clip features. Only runnable where the reference tree exists; the
fixtures travel with the repo.

    python tests/golden/make_golden_seqdec.py                 (--check NAME: compare the committed fixture with a fresh recording)

Both reference modules import under oracle.ref_harness' HOI stubs. The backbones are patched out HERE, the way ref_harness.ref_lta2 does
it: SlowFast / MViT return the clip feature they are handed, ForecastingEncoderDecoder the second stream, the checkpoint loaders and
freezers do nothing, vocab_idx_to_orig returns tests/seqdec2048_ref.idx_maps. Everything else is the reference's: __init__, encode (ln,
pos_embed / pe, the encoder), decode (embedding * sqrt(d), pos_embed, the causal mask, the decoder, fc), forward, predict.
Each fixture stores the config (JSON) and the outputs only; weights, features and targets are re-derived from the seeds
(tests/seqdec2048_ref.recording_inputs). The generator asserts that tests/seqdec2048_ref.oracle_recording (the oracle of the CPU and GPU
tests) reproduces the recording below 1e-9."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)


def real_class(c):
    import importlib
    from types import SimpleNamespace as NS
    from oracle import ref_harness as rh
    from tests import seqdec2048_ref as s
    rh.use_tree("HOI")
    rh._install_hoi_stubs()
    seq = importlib.import_module("models.lta.lta_models_seqdecoder")
    tra = importlib.import_module("models.lta.lta_models_lta_transfer")
    rh._patch_decoder_layer(seq)                                     # (torch >= 2 passes is_causal to _mha_block)
    for mod in (seq, tra):
        mod.vocab_idx_to_orig = lambda: s.idx_maps(c["V"])
        mod.SlowFast = lambda cfg, with_head=True: rh._AcPass()
        mod.MViT = lambda cfg, with_head=True: rh._AcPass()
    tra.ForecastingEncoderDecoder = lambda cfg, build_decoder=True: rh._LtaPass2()
    for name in ("load_ckpt", "load_lta_backbone", "freeze_params", "freeze_backbone_params"):
        setattr(tra, name, lambda *a, **k: None)
    if c["kind"] == "lta2":
        cfg = s.lta2_cfg(c["d"], c["h"], c["L"], c["n"])
        cfg.MODEL.NUM_CLASSES, cfg.MODEL.HEAD_ACT = [5], "softmax"
        cfg.CHECKPOINT_FILE_PATH_AR = cfg.CHECKPOINT_FILE_PATH_LTA = None
        return tra.TaskFusionMFTransformer2TaskSeqDecoder(cfg, s.vocab_of(c["V"]))
    cfg = s.fcst_cfg(c["d"], c["h"], c["L"], c["n"])
    cfg.RESNET = NS(WIDTH_PER_GROUP=64)
    cfg.MODEL.ARCH, cfg.MODEL.NUM_CLASSES, cfg.MODEL.HEAD_ACT, cfg.MODEL.FREEZE_BACKBONE = "slowfast", [5], "softmax", False
    seq._POOL1 = {"slowfast": [[1, 1, 1], [1, 1, 1]]}
    return getattr(seq, c["cls"])(cfg, s.vocab_of(c["V"]))


def record(c):
    """{name: fp64 tensor} of the real class for one config of tests/seqdec2048_ref.RECORDINGS."""
    import torch
    from tests import greedy_ref as gr
    from tests import seqdec2048_ref as s
    sd64, feats, y = s.recording_inputs(c)
    m = real_class(c)
    m.load_state_dict(sd64, strict=True)
    m = m.double().eval()
    m.y_mask = m.y_mask.double()
    x = feats                                   # the "video": one pathway list; the stand-ins hand its clips back
    out = {}
    with torch.no_grad():
        out["forward"] = m(x, y)
        rows = []
        if c["steps"]:                          # the loop's own logits: the last row of every decode() call predict() makes
            real_decode = m.decode
            m.decode = lambda yy, enc: (rows.append(real_decode(yy, enc)) or rows[-1])
        pv, pn = m.predict(x)
        out["pred_verb"], out["pred_noun"] = pv, pn
        if c["steps"]:
            assert len(rows) == c["steps"]
            logits = torch.stack([r[-1] for r in rows], 0)                                    # (steps, B, V)
            out["step_logits"], out["step_tokens"], out["step_margins"] = logits, logits.argmax(-1).permute(1, 0).contiguous(), gr.top2_margin(logits)
    return out


def main():
    import numpy as np
    import torch
    from tests import seqdec2048_ref as s
    live = os.path.join(HERE, "live")
    os.makedirs(live, exist_ok=True)
    names = sys.argv[1:]
    if names[:1] == ["--check"]:
        z = np.load(os.path.join(live, names[1] + ".npz"))
        got = record(json.loads(str(z["config"])))
        print(f"check {names[1]}: " + " ".join(f"{k} {np.abs(v.numpy() - z[k]).max():.3e}" for k, v in got.items()))
        return
    for name in names or list(s.RECORDINGS):
        c = s.RECORDINGS[name]
        got = record(c)
        want = s.oracle_recording(c, *s.recording_inputs(c))
        assert set(got) == set(want), sorted(set(got) ^ set(want))
        errs = {k: (got[k].double() - want[k].double()).abs().max().item() for k in got}
        assert all(got[k].shape == want[k].shape for k in got) and max(errs.values()) < 1e-9, f"tests/seqdec2048_ref.py does not reproduce {name}: {errs}"
        assert all(v.dtype in (torch.float64, torch.int64) for v in got.values())
        path = os.path.join(live, name + ".npz")
        np.savez_compressed(path, config=np.array(json.dumps(c)), **{k: v.numpy() for k, v in got.items()})
        print(f"wrote live/{name}: {', '.join(f'{k} {tuple(v.shape)}' for k, v in got.items())}; oracle differs by {max(errs.values()):.1e}; {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
