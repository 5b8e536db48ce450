"""-m gpu: ragged d = 128 training steps with the batch table built on the device (egx_ragged_cap_train_fwd / egx_ragged_cap_bwd,
forward_features_ragged(..., lengths=<device tensor>, capacity=)): ONE captured train.GraphedStep replayed over batches of different clip
counts and lengths. The yardstick is the eager forward_features_ragged of the same clips with HOST lengths (the code this path must agree
with: the same table, word for word, hence the same logits and d(feature) bits; the loss and the weight gradients are the same fixed-order
sums regrouped over capacity-sized ranges) and, in train mode and bf16, the per-clip fp64 oracle of tests/test_gpu_ragged_train.py at that
file's TOL. Shapes are the smallest that reach each branch: padded T = 17 per segment (S <= 51: one or two tiles) unless said otherwise.
The padded frames and the rows of empty clips are NaN: a kernel that reads one shows up at once. A batch is a list of B_cap entries, each
the per-segment lengths of a clip or None for an empty one.

Measured on MI355X (tools/ragged_capture_eval.py writes the full record to profiles/ragged_capture_report.txt): see that report."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import dropmask as dm
from tests import ragged_cap_ref as ref
from tests.test_gpu_ragged_train import CE_W, TOL, _check_grads, _clips, _model, _oracle_ttm
from tests.util import max_err, rel_err

pytestmark = pytest.mark.gpu
T17 = 17
X = [(16, 16, 16), (16, 16, 17), (17, 17, 17), (1, 1, 1), (5, 9, 12), (15, 15, 15), (10, 3, 17), (2, 16, 7)]     # S = 48 49 51 3 26 45 30 25
Y = [(1, 1, 1)] + [None] * 7
Z = [(16, 16, 17), None, (7, 7, 7), None, None, (17, 17, 16), None, None]


def _cap_batch(batch, seed, cuda, T_pad=T17, fill=float("nan")):
    """-> (feats [(B_cap, T_pad, 256)] * K NaN-padded, lengths int32 (B_cap, K) on the device, target int64 (B_cap,) on the device with a
    VALID label in the rows of empty clips (the effective targets must mask them), clips of the non-empty slots, their slots)."""
    slots = [b for b, t in enumerate(batch) if t is not None]
    clips = _clips(seed, [batch[b] for b in slots])
    K = len(batch[slots[0]])
    feats = [torch.full((len(batch), T_pad, 256), fill, dtype=torch.float32) for _ in range(K)]
    lengths = torch.zeros((len(batch), K), dtype=torch.int32)
    for c, b in zip(clips, slots):
        for k in range(K):
            feats[k][b, :c[k].shape[0]] = c[k]
            lengths[b, k] = c[k].shape[0]
    target = torch.from_numpy(np.random.default_rng(seed).integers(0, 2, len(batch))).long()
    return [f.to(cuda) for f in feats], lengths.to(cuda), target.to(cuda), clips, slots


def _grads_of(model):
    return {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


def _eager(model, feats, lengths, target, slots, cuda):
    """The yardstick: forward_features_ragged of the batch's own clips with HOST lengths, backward. -> (logits, loss, d(feature), grads)."""
    idx = torch.tensor(slots, device=cuda)
    f = [x[idx].detach().clone().requires_grad_(True) for x in feats]
    for p in model.parameters():
        p.grad = None
    logits, loss = model.forward_features_ragged(*f, lengths=lengths[idx].cpu(), target=target[idx], class_weight=torch.tensor(CE_W, device=cuda))
    loss.backward()
    torch.cuda.synchronize()
    out = (logits.detach().clone(), loss.detach().clone(), [x.grad.clone() for x in f], _grads_of(model))
    for p in model.parameters():
        p.grad = None
    return out


class _Step:
    """One GraphedStep over forward_features_ragged with device lengths; the captured logits, d(feature) and parameter gradients stay
    reachable (they are rewritten in place by every replay)."""

    def __init__(self, model, example, capacity, cuda, optimizer=None):
        from egot2_amd.train import GraphedStep
        self.model, self.hold = model, {}
        w = torch.tensor(CE_W, device=cuda)

        def loss_fn(feats, lengths, target):
            f = [x.detach().requires_grad_(True) for x in feats]
            logits, loss = model.forward_features_ragged(*f, lengths=lengths, target=target, class_weight=w, capacity=capacity)
            self.hold["logits"], self.hold["feats"] = logits, f
            return loss

        self.step = GraphedStep(loss_fn, example, list(model.parameters()), optimizer=optimizer, warmup=1)
        self.grads = {n: p.grad for n, p in model.named_parameters() if p.grad is not None}

    def __call__(self, feats, lengths, target):
        loss = self.step(feats, lengths, target)
        torch.cuda.synchronize()
        return (self.hold["logits"].detach().clone(), loss.clone(), [x.grad.clone() for x in self.hold["feats"]],
                {n: g.clone() for n, g in self.grads.items()})


def _same_bits(a, b):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.equal(x, y) for x, y in zip(a[2], b[2]))
    assert set(a[3]) == set(b[3]) and all(torch.equal(a[3][n], b[3][n]) for n in a[3])


def _against_eager(got, want, lengths, slots, grad_bar=1e-6, report=None):
    """The issue's comparison of a captured replay with the eager call on the same clips."""
    logits, loss, dfeat, grads = got
    e_logits, e_loss, e_dfeat, e_grads = want
    empty = [b for b in range(logits.shape[0]) if b not in slots]
    assert torch.equal(logits[slots], e_logits)
    assert torch.all(logits[empty] == 0)
    lens = lengths.cpu()
    for k, (g, e) in enumerate(zip(dfeat, e_dfeat)):
        valid = torch.arange(g.shape[1])[None, :] < lens[:, k][:, None]                    # (B_cap, T_pad)
        assert torch.equal(g[slots].cpu()[valid[slots]], e.cpu()[valid[slots]]), k
        assert torch.all(g.cpu()[~valid] == 0), k
    print("loss", loss.item(), e_loss.item(), abs(loss.item() - e_loss.item()))
    assert abs(loss.item() - e_loss.item()) <= 2e-6              # tests/fp32_grade.py's loss bar
    assert set(grads) == set(e_grads) and len(grads) >= 20
    worst = max(rel_err(grads[n], e_grads[n]) for n in grads)
    print("worst parameter-gradient rel_err, captured vs eager:", worst)
    if report is not None:
        report.append(worst)
    if grad_bar is not None:
        for n in grads:     # the bar test_ragged_train_permutation_and_determinism sets for a regrouping of the same fixed-order sums
            assert rel_err(grads[n], e_grads[n]) <= grad_bar, (n, rel_err(grads[n], e_grads[n]))


# ---- 1. the table ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [
    [(5, 9, 12)] + [None] * 7,                                                                    # n = 1
    X,                                                                                            # n = B_cap
    Z,                                                                                            # empty clips in the middle
    [(16, 16, 16), (16, 16, 17), (1, 1, 1), (17, 17, 17), None, None, None, None],
    # 1 500 slots: the table kernel's 1 024 threads own two clips each (and the last ones none), every fifth slot empty
    [(1 + b * 7 % 17, 1 + b * 5 % 17, 1 + b * 3 % 17) if b % 5 else None for b in range(1500)],
], ids=["one", "full", "holes", "edges", "many"])
def test_device_table_equals_the_host_table(egx_lib, cuda, batch):
    from egot2_amd._lib import Config, Segment
    B_cap, tok_cap, K = len(batch), 400 if len(batch) <= 8 else 60000, 3
    cfg = Config(128, 4, 2048, 1, K, 1e-5, 2, 0, 0.0, 0.0, 0.0)
    segs = (Segment * K)()
    for s in segs:
        s.T, s.d_in, s.proj_w = T17, 256, 1
    slots = [b for b, t in enumerate(batch) if t is not None]
    full = np.asarray([t if t is not None else (0,) * K for t in batch], dtype=np.int32)
    lengths = torch.from_numpy(full).to(cuda)
    target = torch.arange(B_cap, device=cuda) % 2 + 0                                             # int64
    n = C.c_size_t(0)
    assert egx_lib.egx_ragged_cap_table(C.byref(cfg), segs, B_cap, tok_cap, None, None, None, None, None, C.byref(n), None) == 0
    tile_cap = ref.tile_capacity(B_cap, tok_cap)
    assert n.value == B_cap * 20 + tile_cap + 8
    tab = torch.full((n.value,), -7, dtype=torch.int32, device=cuda)
    eff = torch.full((B_cap,), -7, dtype=torch.int64, device=cuda)
    status = torch.zeros(1, dtype=torch.int32, device=cuda)
    rc = egx_lib.egx_ragged_cap_table(C.byref(cfg), segs, B_cap, tok_cap, lengths.data_ptr(), target.data_ptr(), tab.data_ptr(), eff.data_ptr(),
                                      status.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, egx_lib.egx_last_error()
    torch.cuda.synchronize()
    tab = tab.cpu().numpy()
    rec, tmap = tab[:B_cap * 16].reshape(B_cap, 16), tab[B_cap * 16:B_cap * 16 + tile_cap]
    rseg, meta = tab[B_cap * 16 + tile_cap:B_cap * 20 + tile_cap].reshape(B_cap, 4), tab[-8:]
    # the host table of the batch's own clips (egx_ragged_table_host), word for word
    own = full[slots]
    arr = (C.c_int * own.size)(*own.reshape(-1).tolist())
    hn = C.c_size_t(0)
    tcfg = Config(128, 4, 2048, 1, K, 1e-5, 2, 0, 0.1, 0.1, 0.0)
    assert egx_lib.egx_ragged_table_host(C.byref(tcfg), segs, len(slots), arr, 1, None, C.byref(hn)) == 0
    host = (C.c_int * hn.value)()
    assert egx_lib.egx_ragged_table_host(C.byref(tcfg), segs, len(slots), arr, 1, host, C.byref(hn)) == 0
    host = np.asarray(list(host), dtype=np.int32)
    tiles = hn.value - len(slots) * 20
    h_rec, h_map, h_rseg = host[:len(slots) * 16].reshape(-1, 16), host[len(slots) * 16:len(slots) * 16 + tiles], host[-len(slots) * 4:].reshape(-1, 4)
    assert np.array_equal(rec[slots], h_rec)
    assert np.array_equal(tmap[:tiles], np.asarray(slots, dtype=np.int32)[h_map])                 # the host's clip i is slot slots[i]
    assert np.array_equal(rseg[slots], h_rseg)
    assert np.all(tmap[tiles:] == -1)                                                             # surplus tiles
    empty = [b for b in range(B_cap) if b not in slots]
    assert np.all(rec[empty] == 0)                                                                # empty records
    # and the whole table against the numpy restatement, empty clips included
    n_rec, n_map, n_rseg = ref.table(full)
    assert np.array_equal(rec, n_rec) and np.array_equal(tmap[:tiles], n_map) and np.array_equal(rseg, n_rseg)
    want_eff = target.cpu().clone()
    want_eff[empty] = -1
    assert torch.equal(eff.cpu(), want_eff)                                                       # effective targets
    assert meta.tolist() == [int(own.sum()), tiles, 1, *own.sum(0).tolist(), 0, 0]
    assert status.item() == 0


# ---- 2. one capture, many batches -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 2])
def test_one_capture_serves_many_batches(egx_lib, cuda, L):
    """X (8 clips, tile edges 48 / 49), Y (1 clip of 3 tokens), Z (3 clips between empty ones), X again through ONE captured step at
    (B_cap, tok_cap) = (8, 400), each against the eager call on its clips; X's second replay repeats its first bit for bit (nothing of
    Y or Z is left in the slack)."""
    from egot2_amd import functional as F_egx
    model, _ = _model("ttm3", L, "f32s", cuda, seed=930 + L, p=0.0)
    data = {k: _cap_batch(b, 2000 + 10 * i, cuda) for i, (k, b) in enumerate((("X", X), ("Y", Y), ("Z", Z)))}
    want = {k: _eager(model, f, l, t, slots, cuda) for k, (f, l, t, _, slots) in data.items()}
    step = _Step(model, data["X"][:3], (8, 400), cuda)
    assert F_egx.last_encoder_impl() == "ragged_cap"
    first = None
    for k in ("X", "Y", "Z", "X"):
        f, l, t, _, slots = data[k]
        got = step(f, l, t)
        _against_eager(got, want[k], l, slots)
        if k == "X" and first is None:
            first = got
    _same_bits(got, first)
    assert model.ragged_status() == 0


# ---- 3. tight capacity ------------------------------------------------------------------------------------------------------------------
def test_capacity_exactly_the_batch(egx_lib, cuda):
    """No empty clip, no slack token: (B_cap, tok_cap) = (n, N)."""
    batch = [(16, 16, 17), (17, 17, 17), (1, 1, 1), (16, 16, 16)]
    N = sum(sum(t) for t in batch)
    model, _ = _model("ttm3", 1, "f32s", cuda, seed=941, p=0.0)
    f, l, t, _, slots = _cap_batch(batch, 2100, cuda)
    want = _eager(model, f, l, t, slots, cuda)
    step = _Step(model, (f, l, t), (len(batch), N), cuda)
    _against_eager(step(f, l, t), want, l, slots)
    assert model.ragged_status() == 0


@pytest.mark.parametrize("compute", ["f32s", "bf16"])
def test_long_clips_chunk_edge_and_450(egx_lib, cuda, compute):
    """Padded T = 150: clips of S = 321 (the f32s attention's LDS chunk edge) and 450 with one empty slot, (B_cap, tok_cap) = (3, 900).
    f32s: the comparisons of the other cases against the eager call. bf16: logits, loss and gradients against the fp64 oracle at TOL; the
    captured-vs-eager gradient difference is printed for the report (no bar is set on it)."""
    batch = [(107, 107, 107), None, (150, 150, 150)]
    model, sd = _model("ttm3", 1, compute, cuda, seed=951, p=0.0)
    f, l, t, clips, slots = _cap_batch(batch, 2200, cuda, T_pad=150)
    want = _eager(model, f, l, t, slots, cuda)
    step = _Step(model, (f, l, t), (3, 900), cuda)
    got = step(f, l, t)
    if compute == "f32s":
        _against_eager(got, want, l, slots)
    else:
        _against_eager(got, want, l, slots, grad_bar=None)
        ref_logits, ref_loss, sd64, xs = _oracle_ttm(sd, clips, t[slots].cpu(), 1)
        tl, tg = TOL[compute]
        assert max_err(got[0][slots], ref_logits) < tl
        assert abs(got[1].item() - ref_loss.item()) < tl
        for p in model.parameters():
            p.grad = None
        for n, p in model.named_parameters():
            if n in got[3]:
                p.grad = got[3][n]
        _check_grads(model, sd64, tg)
        for k in range(3):
            for i, b in enumerate(slots):
                T = xs[i][k].shape[0]
                assert rel_err(got[2][k][b, :T], xs[i][k].grad) < tg, (k, b)
    assert model.ragged_status() == 0


# ---- 4. train mode ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compute", ["f32s", "bf16"])
def test_train_mode_masks_of_a_replay_vs_oracle(egx_lib, cuda, compute):
    """p = 0.5, p_pos = 0.1 with the device seed: the replay's logits and gradients against the fp64 oracle under the masks of the seed that
    replay read (the forward advances the word once before it draws); two replays of the same batch draw different masks."""
    batch = [(15, 15, 15), None, (16, 16, 17), (5, 9, 12), (17, 17, 17), None]
    model, sd = _model("ttm3", 1, compute, cuda, seed=961, p=0.5)
    model.enable_device_seed()
    f, l, t, clips, slots = _cap_batch(batch, 2300, cuda)
    step = _Step(model, (f, l, t), (6, 200), cuda)
    s0 = 0x5EED0123
    model._egx_seed_dev.fill_(s0)
    got = step(f, l, t)
    assert (model._egx_seed_dev.item() & dm.M64) == dm.lcg(s0)
    ref_logits, ref_loss, sd64, _ = _oracle_ttm(sd, clips, t[slots].cpu(), 1, dm.lcg(s0), 0.5, 0.1)
    tl, tg = TOL[compute]
    assert max_err(got[0][slots], ref_logits) < tl
    empty = [b for b in range(len(batch)) if b not in slots]
    assert torch.all(got[0][empty] == 0)
    for p in model.parameters():
        p.grad = None
    for n, p in model.named_parameters():
        if n in got[3]:
            p.grad = got[3][n]
    _check_grads(model, sd64, tg)
    again = step(f, l, t)                        # the word moved on: fresh masks
    assert not torch.equal(again[0][slots], got[0][slots])
    assert model.ragged_status() == 0


def test_capture_with_a_host_seed_is_refused(egx_lib, cuda):
    model, _ = _model("ttm3", 1, "f32s", cuda, seed=971, p=0.5)
    f, l, t, _, _ = _cap_batch([(15, 15, 15), None], 2400, cuda)
    w = torch.tensor(CE_W, device=cuda)
    model.forward_features_ragged(*f, lengths=l, target=t, class_weight=w, capacity=(2, 100))[1].backward()      # eager: a host seed is fine
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        with pytest.raises(RuntimeError, match="host seed cannot be captured"):
            model.forward_features_ragged(*f, lengths=l, target=t, class_weight=w, capacity=(2, 100))
        keep = w + 1                                                                                           # (the graph is not empty)
    del keep


# ---- 5. the optimizer in the graph ------------------------------------------------------------------------------------------------------
def test_fused_adam_in_the_graph_matches_eager_ragged_steps(egx_lib, cuda):
    from egot2_amd.train import FusedAdam
    data = [_cap_batch(b, 2500 + i, cuda) for i, b in enumerate((X, Z, [(17, 17, 17), (3, 3, 3)] + [None] * 6))]
    w = torch.tensor(CE_W, device=cuda)
    cap, _ = _model("ttm3", 1, "f32s", cuda, seed=981, p=0.0)
    step = _Step(cap, data[0][:3], (8, 400), cuda, optimizer=FusedAdam(cap.parameters(), lr=1e-3))
    for f, l, t, _, _ in data:
        step.step(f, l, t)
    eager, _ = _model("ttm3", 1, "f32s", cuda, seed=981, p=0.0)
    opt = FusedAdam(eager.parameters(), lr=1e-3)
    for f, l, t, _, slots in data:
        idx = torch.tensor(slots, device=cuda)
        opt.zero_grad(set_to_none=True)
        eager.forward_features_ragged(*[x[idx] for x in f], lengths=l[idx].cpu(), target=t[idx], class_weight=w)[1].backward()
        opt.step()
    torch.cuda.synchronize()
    p_e = dict(eager.named_parameters())
    for n, p in cap.named_parameters():          # (three Adam steps move every weight by ~3 lr: the parameters agree far below that)
        assert rel_err(p.detach(), p_e[n].detach()) < 1e-3, n
    assert cap.ragged_status() == 0


# ---- 6. refused on the device, never a fault ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad,bit", [
    ([(16, 16, T17 + 1), (5, 9, 12)], 1),                          # a length of T_pad + 1
    ([(16, 16, 17), (5, 0, 5)], 2),                                # a clip with an empty segment among others
    ([(17, 17, 17), (16, 17, 17)], 8),                             # sum S_b = tok_cap + 1
], ids=["length", "partial", "tokens"])
def test_a_batch_that_does_not_fit_runs_as_the_empty_batch(egx_lib, cuda, bad, bit):
    """These inputs are refused by construction (the table kernel builds the table of an empty batch, so no length indexes anything): the
    status bit is set and stays, logits / loss / every gradient are exactly 0, and the next valid replay repeats the one before."""
    model, _ = _model("ttm3", 1, "f32s", cuda, seed=991, p=0.0)
    good = [(16, 16, 17), (5, 9, 12), None, None]
    f, l, t, _, _ = _cap_batch(good, 2600, cuda)
    step = _Step(model, (f, l, t), (4, 100), cuda)
    before = step(f, l, t)
    assert model.ragged_status() == 0 and before[0].abs().sum() > 0
    lb = l.clone()
    for b, tup in enumerate(bad):
        lb[b] = torch.tensor(tup, dtype=torch.int32)
    logits, loss, dfeat, grads = step(f, lb, t)
    assert model.ragged_status() == bit
    assert torch.all(logits == 0) and loss.item() == 0.0
    assert all(torch.all(g == 0) for g in dfeat) and all(torch.all(g == 0) for g in grads.values()) and len(grads) >= 20
    after = step(f, l, t)
    _same_bits(after, before)
    assert model.ragged_status() == bit                             # sticky until cleared
    assert model.ragged_status(clear=True) == bit and model.ragged_status() == 0


# ---- 7. eval mode -----------------------------------------------------------------------------------------------------------------------
def test_eval_mode_equals_the_host_length_call(egx_lib, cuda):
    model, _ = _model("ttm3", 2, "f32s", cuda, seed=995, p=0.1)
    model.eval()
    f, l, t, _, slots = _cap_batch(Z, 2700, cuda)
    idx = torch.tensor(slots, device=cuda)
    with torch.no_grad():
        got = model.forward_features_ragged(*f, lengths=l, capacity=(8, 400))
        want = model.forward_features_ragged(*[x[idx] for x in f], lengths=l[idx].cpu())
    torch.cuda.synchronize()
    assert tuple(got.shape) == (8, 2) and torch.equal(got[idx], want)
    assert torch.all(got[[b for b in range(8) if b not in slots]] == 0)
    assert model.ragged_status() == 0
