#!/usr/bin/env python3
"""Records live/attn_ref_*.npz: the head-averaged cross-attention weights of the REAL EgoT2-g classes, taken by forward hooks on every
transformer_decoder.layers[i].multihead_attn (CustomDecoderLayer._mha_block calls it with need_weights=True:
HHI/models/multitask/task_prompt_model.py:163-172, HOI/models/multitask/video_model_builder.py:20-30), in fp64, on seeded weights and
features. Only runnable where the reference tree exists; the fixtures travel with the repo.

    python tests/golden/make_golden_attn.py                 (--check NAME: compare the committed fixture with a fresh recording)

Each fixture stores the config (JSON: shape, task, seeds), the target tokens (B, sy), the decode() logits (sy, B, V) and the hooked
weights (L, B, sy, S), all fp64. Weights: tests/util.seeded_state_dict(model, wseed); features: tests/util.seeded_feats(fseed, ...);
tokens: a seeded generator (tests/attn_ref.recording_inputs). The generator asserts that tests/attn_ref.g_decode_attn (the oracle of the
GPU tests) reproduces the recording below 1e-9."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)


def record(name, c):
    """(tokens, logits (sy, B, V), weights (L, B, sy, S)) of the real class for one config of tests/attn_ref.RECORDINGS."""
    import torch
    from oracle import ref_harness as rh
    from tests import attn_ref as ar
    _, _, y, _, feats = ar.recording_inputs(c)
    if c["kind"] == "hhi":
        m = rh.ref_hhi_g(rh.hhi_args(hidden_dim=c["d"], num_heads=c["h"], dropout=0.0, num_layers=c["L"]), ar.HHI_VOCAB)
    else:
        m = rh.ref_hoi_g(rh.hoi_g_args(hidden_dim=c["d"], num_heads=c["h"], num_layers=c["L"]), rh.HOI_G_VOCAB)
    from tests.util import seeded_state_dict
    m.load_state_dict(seeded_state_dict(m, c["wseed"]))
    m = m.double().eval()
    seen = []
    hooks = [layer.multihead_attn.register_forward_hook(lambda mod, args, out: seen.append(out[1].detach().clone()))
             for layer in m.transformer_decoder.layers]
    with torch.no_grad():
        if c["kind"] == "hhi":      # video -> lam, audio -> ttm, audio_asd -> asd (oracle order: lam, ttm, asd)
            enc = m.encode(feats[0], torch.zeros(c["B"], c["T"], 1, 1, dtype=torch.float64), feats[1], feats[2], c["task"])
        else:
            enc = rh.hoi_g_encode_other(m, c["task"], *feats)
        logits = m.decode(y, enc)
    for h in hooks:
        h.remove()
    assert len(seen) == c["L"] and all(w is not None for w in seen), "the hooks saw no weights"
    return y, logits, torch.stack(seen, 0)


def main():
    import numpy as np
    import torch
    from tests import attn_ref as ar
    live = os.path.join(HERE, "live")
    os.makedirs(live, exist_ok=True)
    names = sys.argv[1:]
    if names[:1] == ["--check"]:    # tests/test_cpu_attn_weights.py: the committed fixture against a fresh recording
        z = np.load(os.path.join(live, names[1] + ".npz"))
        y, logits, w = record(names[1], json.loads(str(z["config"])))
        print(f"check {names[1]}: tokens {bool((y.numpy() == z['tokens']).all())} weights {np.abs(w.numpy() - z['weights']).max():.3e} "
              f"logits {np.abs(logits.numpy() - z['logits']).max():.3e}")
        return
    if not names:       # one process per recording: the HHI and HOI reference trees cannot be imported into one
        import subprocess
        for name in ar.RECORDINGS:
            subprocess.run([sys.executable, os.path.abspath(__file__), name], check=True)
        return
    for name in names:
        c = ar.RECORDINGS[name]
        y, logits, w = record(name, c)
        _, sd64, y2, mem, _ = ar.recording_inputs(c)
        assert torch.equal(y, y2)
        with torch.no_grad():
            l2, w2 = ar.g_decode_attn(sd64, c["h"], y, mem)
        assert w.dtype == torch.float64 and w.shape == w2.shape == (c["L"], c["B"], c["sy"], mem.shape[0]), (w.shape, w2.shape)
        ew, el = (w - w2).abs().max().item(), (logits - l2).abs().max().item()
        assert ew < 1e-9 and el < 1e-9, f"tests/attn_ref.py does not reproduce the hooked weights: {ew:.2e} (logits {el:.2e})"
        np.savez_compressed(os.path.join(live, name + ".npz"), config=np.array(json.dumps(c)), tokens=y.numpy(), logits=logits.numpy(),
                            weights=w.numpy())
        print(f"wrote live/{name}: weights {tuple(w.shape)}, oracle differs by {ew:.1e}, max |w - 1/S| = {(w - 1.0 / w.shape[-1]).abs().max().item():.3e}, "
              f"{os.path.getsize(os.path.join(live, name + '.npz'))} bytes")


if __name__ == "__main__":
    main()
