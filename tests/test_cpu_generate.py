"""Greedy generation on the host, without a GPU (egx_decoder_generate_workspace / egx_decoder_generate, added under ABI v18 as the ragged
entry points were): symbols, the workspace query, the library's refusals, the model methods' validation, and the fp64 greedy helper of the
GPU tests against the recorded predict_ac of the reference class. Pure host work (no HIP call)."""
import ctypes as C
import json
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

NEW = ("egx_decoder_generate_workspace", "egx_decoder_generate")


def _dcfg(d=256, h=4, L=3, V=7, S=48, compute=1, p_drop=0.0, p_pos=0.0, dff=2048, sy=0):
    from egot2_amd._lib import DecConfig
    return DecConfig(d, h, dff, L, V, sy, S, 1e-5, compute, p_drop, p_pos, None)


def _ws(lib, cfg, B, n):
    nb = C.c_size_t(0)
    return lib.egx_decoder_generate_workspace(C.byref(cfg), B, n, C.byref(nb)), nb.value


def test_abi_stays_18_and_the_two_symbols_resolve(egx_lib):
    from egot2_amd import _lib
    assert _lib.EGX_ABI_VERSION == 18 and egx_lib.egx_abi_version() == 18
    for name in NEW:
        assert hasattr(egx_lib, name) and name in _lib.SIGNATURES, name


@pytest.mark.parametrize("d,L", [(256, 3), (512, 3), (256, 1)])
def test_workspace_grows_with_steps_through_the_cache_only(egx_lib, d, L):
    B = 40

    def slope(B, S):
        rc1, a = _ws(egx_lib, _dcfg(d=d, h=d // 64, L=L, S=S), B, 32)
        rc2, b = _ws(egx_lib, _dcfg(d=d, h=d // 64, L=L, S=S), B, 64)
        assert rc1 == 0 and rc2 == 0
        assert (b - a) % 32 == 0
        return (b - a) // 32

    s = slope(B, 48)
    assert L * B * 2 * d * 2 <= s <= L * B * 3 * d * 4, (s, L * B * 2 * d * 2, L * B * 3 * d * 4)
    assert slope(2 * B, 48) == 2 * s                                    # it doubles from B to 2B
    assert slope(B, 1) == s == slope(B, 1024)                           # the memory's K | V is counted once, not per step
    # linear in n_steps: the same slope on every interval
    vals = [_ws(egx_lib, _dcfg(d=d, h=d // 64, L=L), B, n)[1] for n in (1, 2, 3, 17, 64)]
    assert [(vals[i + 1] - vals[i]) for i in range(4)] == [s, s, 14 * s, 47 * s]
    # no transposed weight copies: below the fused decoder's `saved` at sy = 1
    sv, sc = C.c_size_t(0), C.c_size_t(0)
    assert egx_lib.egx_decoder_workspace(C.byref(_dcfg(d=d, h=d // 64, L=L, sy=1)), B, C.byref(sv), C.byref(sc)) == 0
    assert _ws(egx_lib, _dcfg(d=d, h=d // 64, L=L), B, 1)[1] < sv.value


def test_refusals_carry_their_message(egx_lib):
    def refused(cfg, frag, B=4, n=2):
        rc, _ = _ws(egx_lib, cfg, B, n)
        assert rc != 0 and frag in egx_lib.egx_last_error(), (frag, egx_lib.egx_last_error())

    assert _ws(egx_lib, _dcfg(sy=77), 4, 2)[0] == 0                     # cfg->sy is not read
    refused(_dcfg(p_drop=0.1), b"inference only")
    refused(_dcfg(p_pos=0.1), b"inference only")
    for compute in (0, 2):
        refused(_dcfg(compute=compute), b"bf16")
    refused(_dcfg(), b"n_steps = 0", n=0)
    refused(_dcfg(), b"n_steps = 65", n=65)
    assert _ws(egx_lib, _dcfg(), 4, 64)[0] == 0
    refused(_dcfg(V=1025), b"vocab = 1025")
    refused(_dcfg(V=0), b"vocab = 0")
    assert _ws(egx_lib, _dcfg(V=1024), 4, 2)[0] == 0
    refused(_dcfg(d=192, h=3), b"d_model = 192")
    refused(_dcfg(d=1152, h=18), b"d_model = 1152")
    refused(_dcfg(d=256, h=2), b"head dim 128")
    refused(_dcfg(dff=100), b"d_ff = 100")
    refused(_dcfg(L=17), b"17 layers")
    refused(_dcfg(S=1025), b"S = 1025")
    refused(_dcfg(S=0), b"S = 0")
    refused(_dcfg(), b"B = 0", B=0)
    nb = C.c_size_t(0)
    assert egx_lib.egx_decoder_generate_workspace(None, 4, 2, C.byref(nb)) != 0 and b"null" in egx_lib.egx_last_error()
    # the call itself: the same checks, then null pointers, before any device work
    cfg = _dcfg()
    assert egx_lib.egx_decoder_generate(C.byref(cfg), None, None, None, None, 256, None, None, None, 4, 2, None, None, None, None) != 0
    assert b"null pointer" in egx_lib.egx_last_error()
    assert egx_lib.egx_decoder_generate(C.byref(_dcfg(p_drop=0.5)), None, None, None, None, 256, None, None, None, 4, 2, None, None, None, None) != 0
    assert b"inference only" in egx_lib.egx_last_error()
    assert egx_lib.egx_decoder_generate(C.byref(cfg), None, None, None, None, 256, None, None, None, 4, 65, None, None, None, None) != 0
    assert b"n_steps = 65" in egx_lib.egx_last_error()


def test_supported_predicate_matches_the_library(egx_lib):
    from egot2_amd import functional as F_egx
    for compute, d, h, dff, S, L, V, n in [("bf16", 512, 8, 2048, 48, 3, 12, 2), ("bf16", 256, 4, 2048, 200, 2, 600, 40), ("bf16", 256, 4, 2048, 8, 2, 1024, 64),
                                           ("bf16", 256, 4, 2048, 8, 2, 1025, 2), ("bf16", 256, 4, 2048, 8, 2, 12, 65), ("f32s", 256, 4, 2048, 8, 2, 12, 2),
                                           ("bf16", 128, 4, 2048, 8, 2, 12, 2), ("bf16", 256, 4, 2048, 1025, 2, 12, 2), ("bf16", 256, 2, 2048, 8, 2, 12, 2)]:
        want = F_egx.decoder_generate_supported(compute, d, h, dff, S, L, V, n)
        rc, _ = _ws(egx_lib, _dcfg(d=d, h=h, L=L, V=V, S=S, dff=dff, compute={"bf16": 1, "f32": 0, "f32s": 2}[compute]), 3, n)
        assert want == (rc == 0), (compute, d, h, dff, S, L, V, n)


def _model(V=12):
    from egot2_amd import hoi_multitask
    from tests import greedy_ref as gr
    args = NS(hidden_dim=256, num_heads=4, num_layers=1, dropout=0.0, pnr_cfg_file=None, oscc_cfg_file=None, action_cfg_file=None, lta_cfg_file=None)
    return hoi_multitask.TaskPromptTransformer(args, gr.vocab_of(V))


def test_python_validation_raises_before_any_library_call(egx_lib, monkeypatch):
    from egot2_amd import _lib
    m = _model()
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was called")))
    mem = torch.zeros(16, 3, 256)
    with pytest.raises(ValueError, match="inference-only"):
        m.train().greedy_decode(mem, 4, 2)
    m.eval()
    with pytest.raises(ValueError, match="inference-only"):             # eval mode, but an autograd graph over the parameters
        m.greedy_decode(mem, 4, 2)
    with torch.no_grad():
        with pytest.raises(ValueError, match="start must be a \\(3,\\)"):
            m.greedy_decode(mem, torch.zeros(4, dtype=torch.int64), 2)
        with pytest.raises(ValueError, match="start must be a \\(3,\\)"):
            m.greedy_decode(mem, torch.zeros(3, 1, dtype=torch.int64), 2)
        with pytest.raises(ValueError, match="int64"):
            m.greedy_decode(mem, torch.zeros(3, dtype=torch.int32), 2)
        with pytest.raises(ValueError, match="start_token"):
            m.greedy_decode(mem, 4.0, 2)
        with pytest.raises(ValueError, match="positional table"):
            m.greedy_decode(mem, 4, 201)
        with pytest.raises(ValueError, match="n_steps"):
            m.greedy_decode(mem, 4, 0)
        with pytest.raises(ValueError, match="\\(S, B, d\\)"):
            m.greedy_decode(mem[0], 4, 2)
        with pytest.raises(ValueError, match="GPU only"):               # CPU tensors: no CPU fallback
            m.greedy_decode(mem, 4, 2)
    assert m.egx_generate is False                                       # predict_ac keeps the loop unless the user opts in


FIXTURES = ["hoig_predict_ac_d256_h8_L2_V12", "hoig_predict_ac_d256_h4_L2_V40", "hoig_predict_ac_d512_h8_L3_V40"]


@pytest.mark.parametrize("fixture", FIXTURES)
def test_greedy_ref_reproduces_the_recorded_predict_ac(fixture):
    """tests/greedy_ref.py (the oracle loop of the GPU tests) against the REAL predict_ac recorded by tests/golden/make_golden_generate.py:
    tokens exactly, logits and margins to 1e-9 in fp64; and the recording gives the strict-token check something to hold."""
    from egot2_amd import hoi_multitask
    from tests import greedy_ref as gr
    from tests.util import seeded_feats, seeded_state_dict
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "live", fixture + ".npz")
    assert os.path.getsize(path) < (1 << 20)
    z = np.load(path)
    c = json.loads(str(z["config"]))
    vocab = gr.vocab_of(c["V"])
    args = NS(hidden_dim=c["d"], num_heads=c["h"], num_layers=c["L"], dropout=0.0, pnr_cfg_file=None, oscc_cfg_file=None, action_cfg_file=None,
              lta_cfg_file=None)
    m = hoi_multitask.TaskTranslationPromptTransformer6Task(args, vocab)
    sd64 = {k: v.double() for k, v in seeded_state_dict(m, c["wseed"]).items()}
    slow, fast = [f.double() for f in seeded_feats(c["fseed"], [(c["B"], 8, 2048), (c["B"], 8, 256)])]
    mem = gr.hoi_action_memory(sd64, c["h"], slow, fast)
    tokens, logits, margins = gr.greedy(sd64, c["h"], torch.full((c["B"],), vocab["action"], dtype=torch.int64), mem, 2)
    rt, rl, rm = torch.from_numpy(z["tokens"]), torch.from_numpy(z["logits"]), torch.from_numpy(z["margins"])
    assert rl.dtype == torch.float64 and torch.equal(tokens, rt)
    assert (logits - rl).abs().max().item() < 1e-9 and (margins - rm).abs().max().item() < 1e-9
    # teacher forcing the recorded tokens gives the same rows (row t of a causal decoder does not see later rows)
    tf = gr.teacher_forced(sd64, c["h"], torch.full((c["B"],), vocab["action"], dtype=torch.int64), rt, mem)
    assert (tf - rl).abs().max().item() < 1e-9
    dec = gr.decided(rm, 4e-2 * max(1.0, rl.abs().max().item()))
    assert dec.float().mean().item() >= 0.5 and len(set(rt[dec].flatten().tolist())) >= 2


def test_argmax_helper_takes_the_lowest_index_on_ties():
    from tests import greedy_ref as gr
    from egot2_amd.decoder import _argmax_lowest
    x = torch.tensor([[1.0, 3.0, 3.0, 2.0], [5.0, 5.0, 5.0, 5.0], [0.0, -1.0, 2.0, 2.0]])
    assert gr.argmax_lowest(x).tolist() == [1, 0, 2] == _argmax_lowest(x).tolist()
    assert gr.top2_margin(x).tolist() == [0.0, 0.0, 0.0] and gr.top2_margin(torch.tensor([[1.0, 4.0, 2.5]])).tolist() == [1.5]


def test_host_planning_against_the_product_library(egx_lib):
    from tests import host_paths_generate as hp
    assert hp.exercise(egx_lib) == 144


def test_generate_planning_under_address_and_ub_sanitizers():
    """The host planning of the generation entry points (tests/host_paths_generate.py) against the host-sanitized build in a child process,
    as tests/test_cpu_ragged_g_train.py runs the ragged training calls': host code on a CPU build only."""
    import subprocess
    import sys
    from egot2_amd import build as egx_build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = egx_build.build_sanitized()
    env = dict(os.environ, LD_PRELOAD=egx_build.asan_runtime(), ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", PYTHONPATH=root)
    env.pop("EGX_LIB", None)
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "host_paths_generate.py"), lib], capture_output=True, text=True,
                       env=env, timeout=900, cwd=root)
    assert r.returncode == 0 and "generate host ok: 144" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
