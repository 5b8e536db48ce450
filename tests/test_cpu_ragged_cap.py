"""The capacity plan of ragged d = 128 training batches (egx_ragged_cap_*, egx_ragged_table_host: ABI v24) on the host, without a GPU: the
host export of the batch table against a numpy restatement, the capacity arithmetic of the workspace query, the refusals of the new calls
(each before any device work: every device pointer is null or a marker that is only compared with null) and train.pad_ragged_batch."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import ragged_cap_ref as ref

NEW = ("egx_ragged_table_host", "egx_ragged_cap_workspace", "egx_ragged_cap_table", "egx_ragged_cap_train_fwd", "egx_ragged_cap_bwd")


def _cfg(compute=2, L=1, p_drop=0.1, p_pos=0.1, p_feat=0.0, nseg=3):
    from egot2_amd._lib import Config
    return Config(128, 4, 2048, L, nseg, 1e-5, compute, 0, p_drop, p_pos, p_feat)


def _segs(T=150, nseg=3):
    from egot2_amd._lib import Segment
    segs = (Segment * nseg)()
    for s in segs:
        s.T, s.d_in, s.proj_w = T, 256, 1     # non-null marker: the queries read no weight
    return segs


def _host_table(lib, lengths, T=150, train=1):
    lengths = np.asarray(lengths, dtype=np.int32)
    B, K = lengths.shape
    arr = (C.c_int * lengths.size)(*lengths.reshape(-1).tolist())
    n = C.c_size_t(0)
    cfg = _cfg(nseg=K) if train else _cfg(nseg=K, p_drop=0.0, p_pos=0.0)        # (the inference plan refuses dropout)
    rc = lib.egx_ragged_table_host(C.byref(cfg), _segs(T, K), B, arr, train, None, C.byref(n))
    if rc:
        return rc, None
    out = (C.c_int * n.value)()
    assert lib.egx_ragged_table_host(C.byref(cfg), _segs(T, K), B, arr, train, out, C.byref(n)) == 0
    return 0, np.asarray(list(out), dtype=np.int32)


def test_new_symbols_are_exported_bound_and_declared(egx_lib):
    from egot2_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "egot2x.h")).read()
    for name in NEW:
        assert hasattr(egx_lib, name) and name in _lib.SIGNATURES and name + "(" in hdr, name


@pytest.mark.parametrize("lengths", [
    [(48, 1, 2)],
    [(16, 16, 16), (16, 16, 17)],
    [(150, 150, 150)],
    [(7, 7, 7)],                                            # one clip only, one tile
    [(15, 15, 15), (150, 150, 150), (16, 16, 16), (1, 1, 1), (16, 16, 17), (100, 49, 1)],
], ids=["48-1-2", "48|49", "450", "one", "mixed"])
def test_host_table_matches_the_numpy_restatement(egx_lib, lengths):
    rc, got = _host_table(egx_lib, lengths)
    assert rc == 0
    want = ref.words(lengths, train=True)
    assert got.shape == want.shape and np.array_equal(got, want)
    rc, got = _host_table(egx_lib, lengths, train=0)       # the inference table: no packed first rows
    assert rc == 0 and np.array_equal(got, ref.words(lengths, train=False))


def test_host_table_two_segments(egx_lib):
    lengths = [(24, 25), (1, 150), (48, 48)]
    rc, got = _host_table(egx_lib, lengths)
    assert rc == 0 and np.array_equal(got, ref.words(lengths))


def test_host_plan_still_refuses_an_empty_clip(egx_lib):
    """Empty clips exist in the capacity plan only: the HOST plan keeps its 1 .. T_pad rule."""
    rc, _ = _host_table(egx_lib, [(15, 15, 15), (0, 0, 0)])
    assert rc != 0 and b"1 .. 150" in egx_lib.egx_last_error()


def _cap_ws(lib, B_cap, tok_cap, cfg=None, segs=None):
    sv, sc = C.c_size_t(0), C.c_size_t(0)
    rc = lib.egx_ragged_cap_workspace(C.byref(cfg or _cfg()), segs if segs is not None else _segs(), B_cap, tok_cap, C.byref(sv), C.byref(sc))
    return rc, sv.value, sc.value


def _train_ws(lib, lengths):
    flat = [t for c in lengths for t in c]
    sv, sc = C.c_size_t(0), C.c_size_t(0)
    assert lib.egx_ragged_train_workspace(C.byref(_cfg()), _segs(), len(lengths), (C.c_int * len(flat))(*flat), C.byref(sv), C.byref(sc)) == 0
    return sv.value, sc.value


def test_capacity_workspace_covers_every_batch_that_fits_and_is_monotone(egx_lib):
    """The capacity layout is egx_ragged_train_workspace's for B_cap clips, tok_cap tokens and ceil(tok_cap / 48) + B_cap tiles. No real
    batch reaches that tile count (sum_b ceil(S_b / 48) <= (N + 47 B) / 48 < ceil(N / 48) + B) nor min(tok_cap, B_cap T_k) packed rows in
    every segment at once, so the two queries cannot be EQUAL for any batch; what must hold is that the capacity covers every batch that
    fits - the one that fills it exactly included - and stays within the tile and row surplus of it."""
    # batches that fill (B_cap, tok_cap) = (8, 400) exactly, at different tile counts
    fills = [[(16, 16, 17)] * 7 + [(19, 19, 19)],                          # 7 * 49 + 57 = 400: 16 tiles
             [(1, 1, 1)] * 7 + [(127, 126, 126)],                          # 21 + 379: 7 + 8 tiles
             [(16, 16, 16)] * 7 + [(22, 21, 21)]]                          # 336 + 64: 7 + 2 tiles
    rc, sv_c, sc_c = _cap_ws(egx_lib, 8, 400)
    assert rc == 0 and sv_c > 0 and sc_c > 0
    for lengths in fills:
        assert sum(sum(c) for c in lengths) == 400
        sv, sc = _train_ws(egx_lib, lengths)
        assert sv <= sv_c and sc <= sc_c, (lengths, sv, sv_c, sc, sc_c)
    # and no more than the layout of a batch with one tile per 48 tokens more clips' worth of tiles: within 2x of the fullest real batch
    sv, sc = _train_ws(egx_lib, fills[0])
    assert sv_c < 2 * sv and sc_c < 2 * sc
    # monotone in both capacities
    prev = (0, 0)
    for tok in (24, 48, 49, 400, 401, 1300, 5000):
        rc, sv, sc = _cap_ws(egx_lib, 8, tok)
        assert rc == 0 and sv >= prev[0] and sc >= prev[1], tok
        prev = (sv, sc)
    prev = (0, 0)
    for B in (1, 2, 8, 26, 100, 433):
        rc, sv, sc = _cap_ws(egx_lib, B, 1300)
        assert rc == 0 and sv >= prev[0] and sc >= prev[1], B
        prev = (sv, sc)
    # the table words of a capacity: records, tile capacity, packed first rows, 8 totals
    n = C.c_size_t(0)
    assert egx_lib.egx_ragged_cap_table(C.byref(_cfg()), _segs(), 8, 400, None, None, None, None, None, C.byref(n), None) == 0
    assert n.value == 8 * 16 + ref.tile_capacity(8, 400) + 8 * 4 + 8


def test_capacity_refusals_carry_their_message(egx_lib):
    from egot2_amd._lib import Head, Layer, LayerGrads

    def refused(what, B_cap=8, tok_cap=400, cfg=None, segs=None):
        rc, _, _ = _cap_ws(egx_lib, B_cap, tok_cap, cfg, segs)
        assert rc != 0, what
        assert what in egx_lib.egx_last_error(), egx_lib.egx_last_error()

    assert _cap_ws(egx_lib, 8, 400)[0] == 0
    refused(b"at least 1", B_cap=0)
    refused(b"at least 1", tok_cap=0)
    refused(b"cannot hold", B_cap=8, tok_cap=23)                      # tok_cap < B_cap * K
    assert _cap_ws(egx_lib, 8, 24)[0] == 0
    refused(b"p_feat", cfg=_cfg(p_feat=0.1))
    cfg = _cfg()
    cfg.token_ce = 8                                                   # (any non-null egx_token_ce)
    refused(b"token_ce", cfg=cfg)
    cfg = _cfg()
    cfg.bwd_stage = 1
    refused(b"bwd_stage", cfg=cfg)
    cfg = _cfg()
    cfg.out_tokens = 15
    refused(b"out_tokens", cfg=cfg)
    refused(b"compute", cfg=_cfg(compute=0))                           # exact fp32: not on the tiled kernels
    sv = C.c_size_t(0)
    assert egx_lib.egx_ragged_cap_workspace(None, _segs(), 8, 400, C.byref(sv), C.byref(sv)) != 0
    assert b"null" in egx_lib.egx_last_error()

    layers, lgr = (Layer * 1)(), (LayerGrads * 1)()
    mark = C.c_void_p(256)          # a DEVICE pointer as far as the host is concerned: only compared with null
    head = Head(mark, mark, mark, mark, 2)
    fwd, bwd = egx_lib.egx_ragged_cap_train_fwd, egx_lib.egx_ragged_cap_bwd
    # head-less: refused (the ASD rows stay on the host-length calls)
    assert fwd(C.byref(_cfg()), _segs(), mark, mark, mark, layers, None, 8, 400, None, mark, mark, None, mark, 1, 7, None) != 0
    assert b"head" in egx_lib.egx_last_error()
    assert bwd(C.byref(_cfg()), _segs(), mark, mark, mark, layers, None, 8, 400, None, mark, mark, mark, None, None, None, lgr, None, mark,
               1, 7, None) != 0
    assert b"head" in egx_lib.egx_last_error()
    # null pointers, with a head
    assert fwd(C.byref(_cfg()), _segs(), None, None, None, layers, C.byref(head), 8, 400, None, None, None, None, None, 1, 7, None) != 0
    assert b"null" in egx_lib.egx_last_error()
    assert fwd(C.byref(_cfg()), _segs(), mark, mark, mark, layers, C.byref(head), 8, 400, mark, None, mark, None, None, 1, 7, None) != 0
    assert b"null" in egx_lib.egx_last_error()                         # (the status word)
    assert bwd(C.byref(_cfg()), _segs(), None, None, None, layers, C.byref(head), 8, 400, None, None, None, None, None, None, None, lgr, None,
               None, 1, 7, None) != 0
    assert b"null" in egx_lib.egx_last_error()
    # the configuration refusals reach the two calls as well
    assert fwd(C.byref(_cfg(p_feat=0.1)), _segs(), mark, mark, mark, layers, C.byref(head), 8, 400, mark, None, mark, None, mark, 1, 7, None) != 0
    assert b"p_feat" in egx_lib.egx_last_error()
    assert bwd(C.byref(_cfg(compute=0)), _segs(), mark, mark, mark, layers, C.byref(head), 8, 400, mark, None, mark, mark, None, None, None, lgr,
               None, mark, 1, 7, None) != 0
    assert b"compute" in egx_lib.egx_last_error()
    assert fwd(C.byref(_cfg()), _segs(), mark, mark, mark, layers, C.byref(head), 8, 23, mark, None, mark, None, mark, 1, 7, None) != 0
    assert b"cannot hold" in egx_lib.egx_last_error()


def test_pad_ragged_batch_shapes_and_fills():
    from egot2_amd.train import pad_ragged_batch
    feats = [torch.randn(3, 12, 256), torch.randn(3, 9, 256)]
    lengths = [[12, 9], [5, 5], [1, 9]]
    target = torch.tensor([1, 0, 1])
    f, l, t = pad_ragged_batch(feats, lengths, target, (8, 400), T_pad=17)
    assert [tuple(x.shape) for x in f] == [(8, 17, 256), (8, 17, 256)]
    assert torch.equal(f[0][:3, :12], feats[0]) and torch.equal(f[1][:3, :9], feats[1])
    assert f[0][:3, 12:].abs().sum() == 0 and f[0][3:].abs().sum() == 0 and f[1][3:].abs().sum() == 0
    assert l.dtype == torch.int32 and tuple(l.shape) == (8, 2)
    assert l[:3].tolist() == lengths and l[3:].abs().sum() == 0
    assert t.dtype == torch.int64 and t.tolist() == [1, 0, 1, -1, -1, -1, -1, -1]
    # (B,) lengths spread over the segments; the tensors' own T by default
    f, l, t = pad_ragged_batch([feats[0], feats[0]], [12, 3, 7], target, (3, 44))
    assert [tuple(x.shape) for x in f] == [(3, 12, 256)] * 2 and l.tolist() == [[12, 12], [3, 3], [7, 7]] and t.tolist() == [1, 0, 1]
    with pytest.raises(ValueError, match="B_cap"):
        pad_ragged_batch(feats, lengths, target, (2, 400), T_pad=17)
    with pytest.raises(ValueError, match="tok_cap"):
        pad_ragged_batch(feats, lengths, target, (8, 40), T_pad=17)
    with pytest.raises(ValueError, match="1 .. 9"):
        pad_ragged_batch(feats, [[12, 10], [5, 5], [1, 9]], target, (8, 400), T_pad=17)
    with pytest.raises(ValueError, match="1 .. 12"):
        pad_ragged_batch(feats, [[12, 9], [0, 5], [1, 9]], target, (8, 400), T_pad=17)
    with pytest.raises(ValueError, match="T_pad"):
        pad_ragged_batch(feats, lengths, target, (8, 400), T_pad=10)


def test_device_lengths_are_checked_before_device_work():
    """The functional entry refuses a capacity without device lengths and host lengths with a capacity on the host (CPU tensors: any
    device work would fail differently)."""
    from egot2_amd import hhi_ttm
    from egot2_amd.synth import hhi_args
    m3 = hhi_ttm.TaskFusionMFTransformer3Task(hhi_args()).train()
    f = [torch.zeros(2, 20, 256)] * 3
    with pytest.raises(ValueError, match="capacity"):
        m3.forward_features_ragged(*f, lengths=[15, 20], capacity=(2, 200))
    assert m3.ragged_status() == 0
