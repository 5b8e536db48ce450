#!/usr/bin/env python3
"""Records live/enc_attn_ref.npz: the head-averaged self-attention weights of the REAL task-specific translators' encoder layers, in fp64,
on seeded weights and features. The reference's nn.TransformerEncoderLayer calls self_attn(..., need_weights=False)
(torch/nn/modules/transformer.py _sa_block), so a forward pre-hook on every encoder layer records the layer's input and the layer's own
self_attn is then called on it with need_weights=True: what a user who patches the layer sees. Only runnable where the reference tree
exists; the fixture travels with the repo.

    python tests/golden/make_golden_encattn.py              (--check: compare the committed fixture with a fresh recording)

Models (tests/enc_attn_ref.RECORDINGS, at the sizes and seeds of their fixtures in tests/golden/make_golden.py): the HHI TTM 3-task
translator (L = 1), the ASD translator (L = 2), the HOI PNR 3-task translator and the LTA 4-task translator. The file holds, per model,
its config (JSON: shapes and seeds) and the weights (L, B, S, S) fp64; weights, features and tokens are regenerated from the seeds
(tests/util.seeded_state_dict / seeded_feats). The generator asserts that tests/enc_attn_ref.py (the gate of the GPU tests) reproduces
every recording below 1e-9."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)


def record(c):
    """weights (L, B, S, S) fp64 of the real class for one config of tests/enc_attn_ref.RECORDINGS."""
    import torch
    from oracle import ref_harness as rh
    from tests.util import seeded_feats, seeded_state_dict
    B, T, kind = c["B"], c["T"], c["kind"]
    if kind in ("ttm3", "asd"):
        args = rh.hhi_args(hidden_dim=128, num_heads=4, dropout=0.0, num_layers=c["L"])
        m = rh.ref_ttm(3, args) if kind == "ttm3" else rh.ref_asd(args)
        encoder = lambda: m.transformer_encoder  # noqa: E731
        feats = [f.double() for f in seeded_feats(c["fseed"], [(B, T, 256)] * 3)]          # ttm, lam, asd
        if kind == "ttm3":
            run = lambda: rh.ref_ttm_forward(m, *feats)  # noqa: E731
        else:       # video -> lam, audio -> ttm, audio_asd -> asd
            run = lambda: m(feats[1], torch.zeros(B, T, 1, 1, dtype=torch.float64), feats[0], feats[2])  # noqa: E731
    elif kind == "pnr3":
        m = rh.ref_pnr3(rh.hoi_s_cfg(d=128, layers=c["L"], task="state_change_detection"))
        encoder = lambda: m.transformer  # noqa: E731
        feats = [f.double() for f in seeded_feats(c["fseed"], [(B, 16, 8192), (B, 16, 8192), (B, 8, 2048), (B, 8, 256)])]
        run = lambda: m([feats[0], feats[1]], [rh.pathway5d(feats[2]), rh.pathway5d(feats[3])])  # noqa: E731
    else:
        m = rh.ref_lta4(rh.hoi_cfg(d=c["d"], heads=c["h"], layers=c["L"], n_clips=T, num_classes=[5, 7], z=3))
        encoder = lambda: m.transformer  # noqa: E731
        frames, action, lta = [f.double() for f in seeded_feats(c["fseed"], [(B, T, c["F"], 8192), (B, T, c["d"]), (B, T, 2048)])]
        run = lambda: m([action, lta], frames)  # noqa: E731  REAL forward(x_lta, x_pnr)
    m.load_state_dict(seeded_state_dict(m, c["wseed"]))
    m = m.double().eval()
    seen = []

    def pre_hook(layer, args, kwargs=None):
        x = args[0].detach()
        assert x.shape[0 if layer.self_attn.batch_first else 1] == B, "batch axis"        # HHI layers take (S, B, d), HOI (B, S, d)
        seen.append(layer.self_attn(x, x, x, need_weights=True)[1].detach().clone())        # head-averaged, (B, S, S)

    hooks = [layer.register_forward_pre_hook(pre_hook) for layer in encoder().layers]
    with torch.no_grad():
        run()
    for h in hooks:
        h.remove()
    assert len(seen) == c["L"], f"the hooks fired {len(seen)} times for {c['L']} layers"
    return torch.stack(seen, 0)


def main():
    import numpy as np
    import torch
    from tests import enc_attn_ref as er
    live = os.path.join(HERE, "live")
    path = os.path.join(live, "enc_attn_ref.npz")
    argv = sys.argv[1:]
    if argv[:1] == ["--one"]:       # one process per recording: the HHI and HOI reference trees cannot be imported into one
        name, out = argv[1], argv[2]
        np.save(out, record(er.RECORDINGS[name]).numpy())
        return
    import subprocess
    import tempfile
    fresh = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in er.RECORDINGS:
            out = os.path.join(tmp, name + ".npy")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--one", name, out], check=True, cwd=ROOT)
            fresh[name] = np.load(out)
    if argv[:1] == ["--check"]:     # tests/test_cpu_enc_attn.py: the committed fixture against a fresh recording
        z = np.load(path)
        for name, w in fresh.items():
            same = json.loads(str(z[name + "/config"])) == er.RECORDINGS[name]
            print(f"check {name}: config {same} weights {np.abs(w - z[name + '/weights']).max():.3e}")
        return
    arrays = {}
    for name, w in fresh.items():
        c = er.RECORDINGS[name]
        ref = er.case_oracle(name)[0]
        w = torch.from_numpy(w)
        assert w.dtype == torch.float64 and w.shape == ref.shape, (name, w.shape, ref.shape)
        e = (w - ref).abs().max().item()
        assert e < 1e-9, f"tests/enc_attn_ref.py does not reproduce the recorded weights of {name}: {e:.2e}"
        arrays[name + "/config"] = np.array(json.dumps(c))
        arrays[name + "/weights"] = w.numpy()
        print(f"{name}: weights {tuple(w.shape)}, gate differs by {e:.1e}, max |w - 1/S| = {(w - 1.0 / w.shape[-1]).abs().max().item():.3e}")
    os.makedirs(live, exist_ok=True)
    np.savez_compressed(path, **arrays)
    print(f"wrote live/enc_attn_ref.npz: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
