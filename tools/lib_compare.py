"""Bit-for-bit comparison of two builds of libegot2x.so on the d = 128 paths: has a refactor of the HOST code left every result alone?
(tools/isa_diff.py answers the same question for device code.)
usage: python tools/lib_compare.py <lib_a.so> <lib_b.so> [--out DIR] [--host] [--keep]
       python tools/lib_compare.py --trees <dir_a> <dir_b> [--lib libegot2x.so] [--out DIR] [--keep]

--trees compares two checkouts of the PYTHON bridge on ONE library (has a refactor of egot2_amd/functional.py left every result alone?): the
children import egot2_amd from <dir_a> (twice) and <dir_b> (`git worktree add --detach <dir_a> <commit>` exports the commit to compare
against) and all load --lib (default: this checkout's egot2_amd/libegot2x.so). Besides the arrays below every case then also records where
its gradients live: last_grad_layout["late_floats"], the size of the latest encoder backward's flat buffer, and per gradient its offset in
and the size of the flat storage behind it, so that "the gradient layout did not move" is compared and not assumed.

For each of the runs a0 = lib_a, a1 = lib_a again, b = lib_b one FRESH child process is started with EGX_LIB set, one at a time, each under its
own `timeout`; the first child that exits non-zero ends the comparison and nothing is started after it. A child runs the fixed case list
below through the public model classes (fixed weights, features and host dropout seeds) and writes every output, loss, gradient and the
library's launch count per forward and per backward to DIR/<run>.npz (default DIR: build/lib_compare; removed after the comparison
unless --keep). The parent then compares the files byte for byte:
  * which arrays repeat a0 = a1 is MEASURED; only the scalar loss of a case with the fused cross entropy may differ (per-clip float atomics),
    and never in the tiled and ragged cases (d, e, g, h), whose loss has a launch of its own;
  * every array with a0 = a1 must have a0 = b, and every launch count must be equal;
  * arrays that do not repeat are listed with their a0 / a1 and a0 / b maximum differences side by side.
Exit status 1 when any of this fails. (Known: case f without the deterministic mode — stage 2 of the staged backward runs small_dw without tiles,
which sums dW_in / dW_o with float atomics, fused.h — does not repeat and is reported as such; f_det is its bit-comparable twin.)

Cases (d = 128, three segments of d_in 256, d_ff 2048, 4 heads; f32s and bf16 each):
  a one-launch (EGX_FFN_CUT=0 EGX_FFN_SLICES=1), B 3, T 15, L 2, p 0.1, head + fused CE    b cut (EGX_FFN_CUT=1 EGX_FFN_SLICES=1), L 1; again deterministic
  c sliced (default slice count), B 3, L 1                                               d tiled T 17 (S 51), B 3, L 2, p 0.1, head + CE; head-less with a learned position table
  e tiled T 110 (S 330: across the 320-row chunk), B 2, L 1                              f staged backward (bwd_stage 1, then 2) on shape a; again deterministic
  g ragged inference, lengths LENS at T_pad 16, L 2, with head and head-less             h ragged training, LENS, L 2, p 0.1, head + CE, feature gradients; L 1 head-less
  i ASD rows (out_tokens) with the fused token loss, B 3, T 15, L 2, weight cache (two steps: the cache filled, then valid)
  n generic implementation forced: TTM logits with feature gradients; ASD rows (out_tokens sliced behind the library call), B 3, T 15, L 2,
    deterministic (the generic backward sums its bias and LayerNorm gradients with float atomics otherwise: they would not repeat)
  s ragged training in the capacity form (device lengths, the batch table built on the device): LENS padded to capacity (6 clips, 112 tokens),
    L 2, p 0.1, head + CE, feature gradients, eager; the status word is recorded too
  t the per-length-group fallback on LENS with compute "f32", which the ragged kernels refuse (once, outside the f32s / bf16 loop): inference
    with head and head-less; training, L 2, p 0.1, head + CE, feature gradients, deterministic (as case n)
Case on the wide encoder alone (functional.encoder, bf16, eager, forward + backward), for what the EgoT2-g cases do not reach:
  v an HOI-style stack, d 256, 8 heads (head dim 32), L 2, d_ff 256, B 3, four segments of T 5: projected fp32 with p_feat 0.1, projected with
    pool 2, projected bf16 features used in place, identity with a feature gradient; learned positional table and task rows with their
    gradients; p_drop = p_pos = 0.1
Cases on the EgoT2-g HHI model (d 256, 4 heads, L 3 + 3, bf16, seeded weights; B 4, T_pad 16, lengths LENS, 2 target tokens):
  j uniform encode_features + decode, p 0.1, forward + backward with d_memory; again under a recording functional.bucket_hook (its (lo, hi) calls compared)
  k encode_features_ragged + decode_ragged, p 0.1, with d_memory: 'ttm' (packed rows) and 'asd' (frame-major tuples, decode() on S = 3)
  l the calls of k under no_grad (their `saved` in the shared workspace), and eval-mode ragged inference (encode_features / decode with lengths)
  m greedy_decode, 4 steps, with logits
  u encode_features_ragged with compute "f32" (the per-length-group fallback of the wide ragged path), p 0.1: 'ttm' (packed rows) and 'asd'
    (frame-major tuples), forward + backward of the memory, and again under no_grad. The deterministic mode does not reach this entry point, so
    the backward runs on one-clip groups ('asd': frame counts ASD_T), which repeat; the two-clip group of LENS' first column runs under no_grad
Cases on the cached step (egx_decoder_generate / _beam / _forced) with the seeded models of tests/greedy_ref.py (hhi_model d 256, 4 heads, L 2,
V 40; B 4, S 19; eager; every returned tensor and the call's launch count):
  o greedy_decode, 5 steps, a period-2 schedule, logits and return_attention
  p beam_decode, 5 steps, with scores and trace: W 3 under the schedule, W 5 free (the two beam_head_kernel instantiations)
  q forced_decode, 9 tokens, targets and logits: one sequence per clip (R 1) and three (R 3)
  r greedy_decode on hoi_model d 256 with 8 heads (head dim 32: the other instances of the cached self-attention), 4 steps, with logits

--host: no GPU. The children drive the host-only calls of tests/host_paths*.py (workspace sizes, implementation / slice answers, refusals)
and the ragged workspace queries through a recording proxy, then a grid over the three generation workspace queries (tests/host_paths_generate.py's
models x B 1, 37, 256 x S 1, 48, 1024 x steps 1, 2, 40, 64 x W = R 1, 3, 8) and the early refusals of the six generation entry points (those of
tests/test_cpu_beam.py and tests/test_cpu_forced.py, null pointers, pe_stride, schedules); the parent compares return values, sizes and
egx_last_error() texts."""
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = [[1, 1, 1], [16, 16, 16], [15, 7, 16], [16, 1, 1]]      # S_b = 3, 48 (one full tile), 38, 18
ASD_T = [1, 16, 15, 7]      # case u, 'asd': frame counts that are all different (one clip per length group)
CAPACITY = (6, 112)        # case s: B_cap clips, tok_cap tokens (LENS has 4 clips of 107 tokens)
CE_W = [0.266, 0.734]
CHILD_TIMEOUT = 420


# ---- child: GPU cases -------------------------------------------------------------------------------------------------------------------
def gpu_child(path):
    import numpy as np
    import torch
    from torch import nn
    import egot2_amd
    from egot2_amd import _lib, functional as F_egx, hhi_asd, hhi_multitask, hhi_ttm
    from egot2_amd.synth import HHI_G_VOCAB, hhi_args
    from egot2_amd.train import pad_ragged_batch
    import importlib.util
    spec = importlib.util.spec_from_file_location("egx_tests_util", os.path.join(ROOT, "tests", "util.py"))   # this checkout's, whichever tree is compared
    util = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(util)
    seeded_state_dict = util.seeded_state_dict
    tree = os.environ.get("EGX_COMPARE_TREE")
    assert tree is None or os.path.samefile(os.path.dirname(os.path.dirname(egot2_amd.__file__)), tree), egot2_amd.__file__
    print(f"child: egot2_amd from {os.path.dirname(egot2_amd.__file__)}, library {_lib.LIB_PATH}")
    lib = _lib.load()
    cuda = torch.device("cuda")
    out = {}

    def tune(**env):
        for k in ("EGX_FFN_CUT", "EGX_FFN_SLICES"):
            os.environ.pop(k, None)
        os.environ.update({k: str(v) for k, v in env.items()})
        lib.egx_tuning_reload()

    def model_of(cls, L, p, compute, seed, det=False, learned_pe=False, impl="auto"):
        torch.manual_seed(seed)
        m = cls(hhi_args(num_layers=L, dropout=p))
        if learned_pe:
            pe = m.pos_embed._buffers.pop("pe")
            m.pos_embed.pe = nn.Parameter(pe.clone())
        m = m.to(cuda).set_compute(compute, impl).set_deterministic(det).train()
        m.pos_embed.dropout.p = 0.1 if p > 0 else 0.0
        m._egx_seed = lambda: 0x5EED0000 + seed
        return m

    def feats_of(seed, B, T, grad=False):
        rng = np.random.default_rng(seed)
        return [torch.from_numpy(rng.standard_normal((B, T, 256), dtype=np.float32)).to(cuda).requires_grad_(grad) for _ in range(3)]

    def keep(tag, name, t):
        out[f"{tag}/{name}"] = t.detach().float().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)

    def step(tag, m, fwd, feats=(), finish=None):
        """forward -> (outputs..., scalar to differentiate last); backward; everything recorded under tag/"""
        lib.egx_launch_count(1)
        res = fwd()
        torch.cuda.synchronize()
        keep(tag, "launches_fwd", lib.egx_launch_count(1))
        res = res if isinstance(res, tuple) else (res,)
        for i, r in enumerate(res):
            keep(tag, f"out{i}", r)
        if not torch.is_grad_enabled():
            return
        res[-1].backward() if res[-1].dim() == 0 else (res[-1] * torch.linspace(-1, 1, res[-1].numel(), device=cuda).view_as(res[-1])).sum().backward()
        torch.cuda.synchronize()
        keep(tag, "launches_bwd", lib.egx_launch_count(1))
        if finish is not None:
            finish()
            torch.cuda.synchronize()
            keep(tag, "launches_bwd2", lib.egx_launch_count(1))
        flat = F_egx.last_grad_layout.get("flat")
        keep(tag, "layout", [F_egx.last_grad_layout.get("late_floats", -1), -1 if flat is None else flat.numel()])
        for n, q in m.named_parameters():
            if q.grad is not None:
                keep(tag, "grad/" + n, q.grad)
                st = q.grad.untyped_storage()       # (offset in, size of) the flat buffer this gradient is a view of
                keep(tag, "where/" + n, [(q.grad.data_ptr() - st.data_ptr()) // 4, st.nbytes() // 4])
        for k, f in enumerate(feats):
            if f.grad is not None:
                keep(tag, f"dfeat{k}", f.grad)

    w = torch.tensor(CE_W, device=cuda)
    lens = torch.tensor(LENS)
    TTM, ASD = hhi_ttm.TaskFusionMFTransformer3Task, hhi_asd.TaskFusionMFTransformer3Task
    for ci, compute in enumerate(("f32s", "bf16")):
        s0 = 100 * ci
        tgt3, tgt2, tgt4 = torch.tensor([0, 1, 1], device=cuda), torch.tensor([1, 0], device=cuda), torch.tensor([0, 1, 1, 0], device=cuda)
        f15 = feats_of(11, 3, 15)

        def ttm_ce(m, feats, tgt):
            return lambda: m.forward_features(*feats, target=tgt, class_weight=w)

        tune(EGX_FFN_CUT=0, EGX_FFN_SLICES=1)
        m = model_of(TTM, 2, 0.1, compute, s0 + 1)
        step(f"a_{compute}", m, ttm_ce(m, f15, tgt3))
        for det in (False, True):       # (the staged backward sums with float atomics unless deterministic)
            m = model_of(TTM, 2, 0.1, compute, s0 + 6, det=det)
            m.egx_defer_small = True
            step(f"f{'_det' if det else ''}_{compute}", m, ttm_ce(m, f15, tgt3), finish=F_egx.run_deferred)
        m = model_of(ASD, 2, 0.1, compute, s0 + 9).enable_weight_cache()
        lossav = hhi_asd.lossAV(128).to(cuda)
        labels = (torch.arange(45, device=cuda) * 7 // 3) % 2
        for rep in (0, 1):
            m.zero_grad(set_to_none=True)
            step(f"i{rep}_{compute}", m, lambda: tuple(reversed(m.forward_features(*f15, lossav=lossav, labels=labels))))
            assert F_egx.last_encoder_impl() == "fused", F_egx.last_encoder_impl()
        tune(EGX_FFN_CUT=1, EGX_FFN_SLICES=1)
        for det in (False, True):
            m = model_of(TTM, 1, 0.1, compute, s0 + 2, det=det)
            step(f"b{'_det' if det else ''}_{compute}", m, ttm_ce(m, f15, tgt3))
        tune()
        m = model_of(TTM, 1, 0.1, compute, s0 + 3)
        step(f"c_{compute}", m, ttm_ce(m, f15, tgt3))
        assert F_egx.last_encoder_impl() == "fused", F_egx.last_encoder_impl()
        f17 = feats_of(12, 3, 17)
        m = model_of(TTM, 2, 0.1, compute, s0 + 4)
        step(f"d_{compute}", m, ttm_ce(m, f17, tgt3))
        assert F_egx.last_encoder_impl() == "tiled", F_egx.last_encoder_impl()
        m = model_of(ASD, 2, 0.1, compute, s0 + 4, learned_pe=True)
        step(f"d_rows_{compute}", m, lambda: m.forward_features(*f17))
        assert m.pos_embed.pe.grad is not None and F_egx.last_encoder_impl() == "tiled"
        f110 = feats_of(13, 2, 110)
        m = model_of(TTM, 1, 0.1, compute, s0 + 5)
        step(f"e_{compute}", m, ttm_ce(m, f110, tgt2))
        f16 = feats_of(14, 4, 16)
        with torch.no_grad():
            m = model_of(TTM, 2, 0.0, compute, s0 + 7).eval()
            step(f"g_{compute}", m, lambda: m.forward_features(*f16, lengths=lens))
            m = model_of(ASD, 2, 0.0, compute, s0 + 7).eval()
            step(f"g_rows_{compute}", m, lambda: m.forward_features(*f16, lengths=lens))
        f16g = feats_of(14, 4, 16, grad=True)
        m = model_of(TTM, 2, 0.1, compute, s0 + 8)
        step(f"h_{compute}", m, lambda: m.forward_features_ragged(*f16g, lengths=lens, target=tgt4, class_weight=w), feats=f16g)
        assert F_egx.last_encoder_impl() == "ragged", F_egx.last_encoder_impl()
        m = model_of(ASD, 1, 0.1, compute, s0 + 8)
        step(f"h_rows_{compute}", m, lambda: m.forward_features_ragged(*f16, lengths=lens))
        fcap, lcap, tcap = pad_ragged_batch(f16, lens, tgt4, CAPACITY)
        fcap = [f.requires_grad_(True) for f in fcap]
        m = model_of(TTM, 2, 0.1, compute, s0 + 11)
        step(f"s_{compute}", m, lambda: m.forward_features_ragged(*fcap, lengths=lcap, target=tcap, class_weight=w, capacity=CAPACITY), feats=fcap)
        assert F_egx.last_encoder_impl() == "ragged_cap", F_egx.last_encoder_impl()
        keep(f"s_{compute}", "status", m.ragged_status())
        f15g = feats_of(11, 3, 15, grad=True)
        m = model_of(TTM, 2, 0.1, compute, s0 + 10, det=True, impl="generic")
        step(f"n_{compute}", m, lambda: m.forward_features(*f15g), feats=f15g)
        assert F_egx.last_encoder_impl() == "generic", F_egx.last_encoder_impl()
        m = model_of(ASD, 2, 0.1, compute, s0 + 10, det=True, impl="generic")
        step(f"n_rows_{compute}", m, lambda: m.forward_features(*f15))
        assert F_egx.last_encoder_impl() == "generic", F_egx.last_encoder_impl()

    # the per-length-group fallback of the d = 128 ragged entry points: exact fp32, which the ragged kernels refuse
    f16, tgt4 = feats_of(14, 4, 16), torch.tensor([0, 1, 1, 0], device=cuda)
    with torch.no_grad():
        m = model_of(TTM, 2, 0.0, "f32", 207).eval()
        step("t_f32", m, lambda: m.forward_features(*f16, lengths=lens))
        assert F_egx.last_encoder_impl() == "grouped", F_egx.last_encoder_impl()
        m = model_of(ASD, 2, 0.0, "f32", 207).eval()
        step("t_rows_f32", m, lambda: m.forward_features(*f16, lengths=lens))
        assert F_egx.last_encoder_impl() == "grouped", F_egx.last_encoder_impl()
    f16g = feats_of(14, 4, 16, grad=True)
    m = model_of(TTM, 2, 0.1, "f32", 208, det=True)
    step("t_train_f32", m, lambda: m.forward_features_ragged(*f16g, lengths=lens, target=tgt4, class_weight=w), feats=f16g)
    assert F_egx.last_encoder_impl() == "grouped", F_egx.last_encoder_impl()

    # an HOI-style stack on the wide encoder, through functional.encoder: what the EgoT2-g cases below do not reach
    class WideStack(nn.Module):
        """d 256, 8 heads, L 2, d_ff 256; four segments of 5 tokens: projected fp32 (cast copy, p_feat), projected with pool 2, projected
        bf16 (used in place), identity (its features take a gradient); a learned positional table and task-embedding rows"""

        def __init__(self, seed, d=256, dff=256, L=2, T=5):
            super().__init__()
            g = torch.Generator().manual_seed(seed)
            rnd = lambda *s: nn.Parameter(torch.randn(*s, generator=g) * 0.05)       # noqa: E731
            self.dims = [256, 128, 256, d]
            self.spec = F_egx.EncoderSpec(d, 8, dff, L, [F_egx.SegmentSpec(T, k, i < 3, add_row=i, pos_row0=i * T, pool=2 if i == 1 else 1)
                                                          for i, k in enumerate(self.dims)],
                                          compute="bf16", p_drop=0.1, p_pos=0.1, p_feat=0.1, training=True, seed=0x5EED0000 + seed)
            self.task_embed, self.pos, self.ln_w, self.ln_b = rnd(1, 4, d), rnd(4 * T, d), nn.Parameter(torch.ones(d)), rnd(d)
            self.proj = nn.ParameterList([q for k in self.dims[:3] for q in (rnd(d, k), rnd(d))])
            shapes = [(3 * d, d), (3 * d,), (d, d), (d,), (dff, d), (dff,), (d, dff), (d,), (d,), (d,), (d,), (d,)]
            self.layers = nn.ParameterList([rnd(*s) for _ in range(L) for s in shapes])

        def forward(self, feats):
            return F_egx.encoder(self.spec, feats, self.task_embed, self.pos, self.ln_w, self.ln_b, list(self.proj), list(self.layers))

    m = WideStack(41).to(cuda)
    rng = np.random.default_rng(42)
    fv = [torch.from_numpy(rng.standard_normal((3, 5 * (2 if i == 1 else 1), k), dtype=np.float32)).to(cuda) for i, k in enumerate(m.dims)]
    fv[2], fv[3] = fv[2].to(torch.bfloat16), fv[3].requires_grad_(True)
    step("v", m, lambda: m(fv), feats=fv)
    assert F_egx.last_encoder_impl() == "wide" and m.pos.grad is not None and fv[3].grad is not None, F_egx.last_encoder_impl()

    # EgoT2-g HHI model: the wide encoder and the fused decoder, uniform and ragged
    def g_model(seed, p=0.1, compute="bf16"):
        m = hhi_multitask.TaskTranslationPromptTransformer(hhi_args(hidden_dim=256, num_heads=4, num_layers=3, dropout=p), HHI_G_VOCAB)
        m.load_state_dict(seeded_state_dict(m, seed))
        m.pos_embed.dropout.p = p
        m = m.to(cuda).set_compute(compute).train()
        m._egx_seed = lambda: 0x5EED0000 + seed
        return m

    def targets(n, task, seed):
        g = torch.Generator().manual_seed(seed)
        return torch.stack([torch.full((n,), HHI_G_VOCAB[task]), torch.randint(5, 7, (n,), generator=g)], dim=1).to(cuda)

    def g_step(tag, m, fwd):
        """fwd() -> (memory, logits); the memory's gradient is recorded as dfeat0"""
        held = []

        def run():
            mem, logits = fwd()
            if torch.is_grad_enabled():
                mem.retain_grad()
            held.append(mem)
            return mem, logits
        step(tag, m, run, feats=held)

    y4, frames = targets(4, "ttm", 21), lens[:, 0]
    y_asd = targets(int(frames.sum()), "asd", 22)
    S = F_egx.ragged_lengths(lens, 4, [16, 16, 16]).sum(1)

    def uniform(m):
        mem = m.encode_features("ttm", *f16)
        return mem, m.decode(y4, mem)

    def ragged_ttm(m):
        mem = m.encode_features_ragged("ttm", *f16, lengths=lens)
        return mem, m.decode_ragged(y4, mem, S)

    def ragged_asd(m):
        mem = m.encode_features_ragged("asd", *f16, lengths=frames)
        return mem, m.decode(y_asd, mem)

    m = g_model(31)
    g_step("j", m, lambda: uniform(m))
    assert F_egx.last_encoder_impl() == "wide" and F_egx.last_decoder_impl() == "fused", (F_egx.last_encoder_impl(), F_egx.last_decoder_impl())
    buckets = []
    F_egx.bucket_hook = lambda flat, lo, hi: buckets.append((flat.numel(), lo, hi))
    try:
        m.zero_grad(set_to_none=True)
        g_step("j_hook", m, lambda: uniform(m))
    finally:
        F_egx.bucket_hook = None
    keep("j_hook", "buckets", buckets)
    for tag, fwd in (("k_ttm", ragged_ttm), ("k_asd", ragged_asd)):
        m = g_model(32)
        g_step(tag, m, lambda: fwd(m))
        assert F_egx.last_encoder_impl() == "ragged", F_egx.last_encoder_impl()
    # both out_layouts of the grouped fallback. encode_features_ragged does not hand the deterministic mode down, and the generic backward of a
    # group of several clips sums its bias and LayerNorm gradients with float atomics: the backward runs on one-clip groups ('asd': ASD_T), the
    # two-clip group of `frames` under no_grad
    for tag, task, ln, ln_fwd in (("u_ttm", "ttm", lens, lens), ("u_asd", "asd", torch.tensor(ASD_T), frames)):
        m = g_model(33, compute="f32")
        step(tag, m, lambda: m.encode_features_ragged(task, *f16, lengths=ln))
        assert F_egx.last_encoder_impl() == "grouped", F_egx.last_encoder_impl()
        with torch.no_grad():
            step(tag + "_nograd", m, lambda: m.encode_features_ragged(task, *f16, lengths=ln_fwd))
    with torch.no_grad():
        m = g_model(32)
        g_step("l_ttm", m, lambda: ragged_ttm(m))
        g_step("l_asd", m, lambda: ragged_asd(m))
        m.eval()

        def infer():
            mem = m.encode_features("ttm", *f16, lengths=lens)
            return mem, m.decode(y4, mem, memory_lengths=S)
        g_step("l_infer", m, infer)
        assert F_egx.last_encoder_impl() == "ragged" and F_egx.last_decoder_impl() == "ragged"
        mem = m.encode_features("ttm", *f16)
        step("m", m, lambda: m.greedy_decode(mem, HHI_G_VOCAB["ttm"], 4, return_logits=True))
        assert F_egx.last_decoder_impl() == "generate", F_egx.last_decoder_impl()

        # the cached-step calls on the seeded models of tests/greedy_ref.py, eagerly: every returned tensor and the launch count of the call
        from tests import greedy_ref as gr

        def cached(build, d, h, L, V, S, wseed):
            mdl, _, start = build(d, h, L, V, wseed)
            return mdl.to(cuda).set_compute("bf16").eval(), start, util.seeded_feats(96, [(S, 4, d)])[0].to(cuda)

        def flat(res):
            """a call's results as a tuple of tensors (a BeamTrace as its four)"""
            res = res if isinstance(res, tuple) else (res,)
            return tuple(t for r in res for t in ([getattr(r, k) for k in r.__slots__] if isinstance(r, F_egx.BeamTrace) else [r]))

        mg, start, memg = cached(gr.hhi_model, 256, 4, 2, 40, 19, 130)
        allowed = torch.zeros((2, 40), dtype=torch.bool)
        allowed[0, 5:17], allowed[1, 12:40] = True, True
        sched = mg.token_schedule(allowed)
        step("o", mg, lambda: flat(mg.greedy_decode(memg, start, 5, return_logits=True, schedule=sched, return_attention=True)))
        step("p_w3", mg, lambda: flat(mg.beam_decode(memg, start, 5, 3, return_scores=True, return_trace=True, schedule=sched)))
        assert F_egx.last_decoder_impl() == "beam", F_egx.last_decoder_impl()
        step("p_w5", mg, lambda: flat(mg.beam_decode(memg, start, 5, 5, return_scores=True, return_trace=True)))
        g = torch.Generator().manual_seed(23)
        y = torch.randint(0, 40, (4, 3, 9), generator=g).to(cuda)
        tg = torch.randint(-1, 40, (4, 3, 9), generator=g).to(cuda)            # (-1: outside the vocabulary, logprob exactly 0)
        step("q_r1", mg, lambda: flat(mg.forced_decode(memg, y[:, 0].contiguous(), targets=tg[:, 0].contiguous())))
        assert F_egx.last_decoder_impl() == "forced", F_egx.last_decoder_impl()
        step("q_r3", mg, lambda: flat(mg.forced_decode(memg, y, targets=tg)))
        m32, start32, mem32 = cached(gr.hoi_model, 256, 8, 2, 12, 16, 95)      # head dim 32: the other instances of the cached self-attention
        step("r", m32, lambda: flat(m32.greedy_decode(mem32, start32, 4, return_logits=True)))
        assert F_egx.last_decoder_impl() == "generate", F_egx.last_decoder_impl()
    np.savez(path, **out)
    print(f"{os.path.relpath(path, ROOT)}: {len(out)} arrays")


# ---- child: host-only calls ------------------------------------------------------------------------------------------------------------------
class Recorder:
    """ctypes library proxy: every call is logged with its return value, the size_t results behind its byref arguments and the error text"""

    def __init__(self, lib):
        self._lib, self.log = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            r = fn(*args)
            if name != "egx_last_error":
                failed = fn.restype is C.c_int and r != 0       # (or an answer such as an implementation id: the text is then the last failure's)
                sizes = [] if failed else [a._obj.value for a in args if isinstance(getattr(a, "_obj", None), C.c_size_t)]
                self.log.append([name, r.decode() if isinstance(r, bytes) else r, sizes, self._lib.egx_last_error().decode() if failed else ""])
            return r
        return call


def host_child(path):
    sys.path.insert(0, ROOT)
    from egot2_amd import _lib
    from egot2_amd._lib import Config, Segment
    from tests import host_paths, host_paths_generate, host_paths_ragged_g_train
    rec = Recorder(host_paths.bind(_lib.LIB_PATH))
    for mod in (host_paths, host_paths_generate, host_paths_ragged_g_train):
        mod.exercise(rec)
    nb, sv, sc = C.c_size_t(), C.c_size_t(), C.c_size_t()
    for T_pad, lens in ((16, [[1, 1, 1], [15, 7, 15], [16, 16, 16]]), (150, [[150, 150, 150]])):
        segs = (Segment * 3)()
        for s in segs:
            s.T, s.d_in, s.proj_w = T_pad, 256, 1
        arr = (C.c_int * (3 * len(lens)))(*[t for clip in lens for t in clip])
        for compute in (0, 1, 2):
            for L in (1, 2, 6, 7):
                for p in (0.0, 0.1):
                    for det in (0, 1):
                        cfg = Config(128, 4, 2048, L, 3, 1e-5, compute, 0, p, p, 0.0)
                        cfg.deterministic = det
                        rec.egx_ragged_workspace(C.byref(cfg), segs, len(lens), arr, C.byref(nb))
                        rec.egx_ragged_train_workspace(C.byref(cfg), segs, len(lens), arr, C.byref(sv), C.byref(sc))
    # the cached-step calls (greedy, beam, forced; k = W = R): every workspace size, and every refusal that comes before the first device call
    from egot2_amd._lib import DecConfig, DecLayer
    PTR = 1 << 12       # a non-null marker: a call that gets it is refused before anything is read

    def dcfg(d=256, h=4, L=3, V=40, S=48, compute=1, p_drop=0.0, p_pos=0.0, dff=2048, sy=0):
        return DecConfig(d, h, dff, L, V, sy, S, 1e-5, compute, p_drop, p_pos, None)

    def queries(cfg, B, n, k):
        c = C.byref(cfg) if cfg is not None else None
        rec.egx_decoder_generate_workspace(c, B, n, C.byref(nb))
        rec.egx_decoder_beam_workspace(c, B, n, k, C.byref(nb))
        rec.egx_decoder_forced_workspace(c, B, k, n, C.byref(nb))

    def calls(cfg, B, n, k, p=None, stride=256, period=0, counts=None, forced=None):
        """the six entry points with every pointer p (None: the null-pointer refusal at the latest); forced: egx_decoder_forced's
        (tokens, targets, logits, logprob, workspace) when they differ from p"""
        c = C.byref(cfg) if cfg is not None else None
        lay = C.cast(p, C.POINTER(DecLayer)) if p else None
        cnt = (C.c_int * len(counts))(*counts) if counts else None
        head, gen, beam = (c, p, p, p, p, stride, lay, p, p, B, n), (p, p, p, None), (k, p, p, p, p, p, p, p, None)
        rec.egx_decoder_generate(*head, *gen)
        rec.egx_decoder_generate_sched(*head, *gen, period, cnt, p)
        rec.egx_decoder_generate_attn(*head, *gen, period, cnt, p, p)
        rec.egx_decoder_generate_attn(*head, *gen, period, cnt, p, PTR)
        rec.egx_decoder_beam(*head, *beam)
        rec.egx_decoder_beam_sched(*head, *beam, period, cnt, p)
        tok, tgt, lg, lp, ws = forced or (p,) * 5
        rec.egx_decoder_forced(c, tok, tgt, p, p, p, stride, lay, p, p, B, k, n, lg, lp, ws, None)

    for d, h, L, V in [(256, 4, 2, 7), (512, 8, 3, 600), (1024, 16, 16, 1024), (384, 12, 1, 1)]:       # tests/host_paths_generate.py's list
        for B in (1, 37, 256):
            for S in (1, 48, 1024):
                for n in (1, 2, 40, 64):
                    for k in (1, 3, 8):
                        cfg = dcfg(d=d, h=h, L=L, V=V, S=S, sy=99)
                        queries(cfg, B, n, k)
                        calls(cfg, B, n, k, stride=d)
    # the refusals of tests/test_cpu_beam.py and tests/test_cpu_forced.py, through the queries and through the calls
    for kw, B, n, k in [(dict(sy=77), 4, 2, 3), ({}, 4, 2, 0), ({}, 4, 2, 9), ({}, 4, 2, -1), ({}, 4, 2, 8), ({}, 4, 2, 1), (dict(V=6), 4, 2, 7),
                        (dict(V=6), 4, 2, 6), (dict(V=2), 4, 2, 8), (dict(V=2), 4, 2, 3), ({}, 4, 0, 3), ({}, 4, 65, 3), ({}, 4, 64, 3),
                        (dict(V=1025), 4, 2, 3), (dict(V=0), 4, 2, 3), (dict(V=1024, d=1024, h=16), 4, 2, 8), (dict(p_drop=0.1), 4, 2, 3),
                        (dict(p_pos=0.1), 4, 2, 3), (dict(p_drop=0.5), 4, 2, 3), (dict(compute=0), 4, 2, 3), (dict(compute=2), 4, 2, 3),
                        (dict(d=192, h=3), 4, 2, 3), (dict(d=256, h=2), 4, 2, 3), (dict(dff=100), 4, 2, 3), (dict(L=17), 4, 2, 3),
                        (dict(S=1025), 4, 2, 3), ({}, 0, 2, 3), (dict(d=1024, h=16), 100000, 2, 8), (None, 4, 2, 3)]:
        cfg = None if kw is None else dcfg(**kw)
        queries(cfg, B, n, k)
        calls(cfg, B, n, k)
        if cfg is not None:     # with every pointer given: the same first refusal, at the latest the pe_stride's (128 < d_model)
            calls(cfg, B, n, k, p=PTR, stride=128)
    rec.egx_decoder_generate_workspace(C.byref(dcfg()), 4, 2, None)             # queries for the verdict alone
    rec.egx_decoder_beam_workspace(C.byref(dcfg()), 4, 2, 3, None)
    rec.egx_decoder_forced_workspace(C.byref(dcfg()), 4, 3, 2, None)
    for stride in (128, 258):
        calls(dcfg(), 4, 2, 3, p=PTR, stride=stride)
    for forced in ((PTR, PTR, None, None, PTR), (PTR, None, PTR, PTR, PTR), (None, PTR, PTR, PTR, PTR), (PTR, PTR, PTR, PTR, None)):
        calls(dcfg(), 4, 2, 3, p=PTR, stride=128, forced=forced)                # (the stride refuses the calls `forced` does not)
    # token schedules: checked before the pointers (a schedule that passes ends at the pe_stride)
    for period, counts in ((65, None), (-1, None), (2, None), (2, [0, 3]), (2, [3, 41]), (2, [2, 40]), (1, [40])):
        calls(dcfg(), 4, 2, 3, period=period, counts=counts)
        calls(dcfg(), 4, 2, 3, p=PTR, stride=128, period=period, counts=counts)
    json.dump(rec.log, open(path, "w"))
    print(f"{os.path.relpath(path, ROOT)}: {len(rec.log)} calls")


# ---- parent ----------------------------------------------------------------------------------------------------------------------------------
def run_children(libs, out_dir, host, trees=None):
    """libs: (run, library) pairs; trees: {run: checkout the child imports egot2_amd (and tests.util) from}, default this one"""
    paths = {}
    for run, lib in libs:
        paths[run] = os.path.join(out_dir, run + (".json" if host else ".npz"))
        tree = os.path.abspath(trees[run]) if trees else ROOT
        env = dict(os.environ, EGX_LIB=os.path.abspath(lib), PYTHONPATH=tree + os.pathsep + os.environ.get("PYTHONPATH", ""))
        if trees:
            env["EGX_COMPARE_TREE"] = tree
        cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable, os.path.abspath(__file__), "--host-child" if host else "--child", paths[run]]
        rc = subprocess.run(cmd, env=env, cwd=ROOT).returncode
        if rc != 0:
            print(f"child {run} ({lib}) exited with {rc}: stopping, nothing else is run")
            sys.exit(2)
    return paths


def compare_host(paths):
    a0, a1, b = (json.load(open(paths[k])) for k in ("a0", "a1", "b"))
    bad = 0
    if a0 != a1:
        print("a0 / a1: the host calls of lib_a do not repeat")
        bad += 1
    if len(a0) != len(b):
        print(f"call counts differ: {len(a0)} / {len(b)}")
        bad += 1
    for i, (x, y) in enumerate(zip(a0, b)):
        if x != y:
            bad += 1
            if bad < 20:
                print(f"call {i} differs:\n  a: {x}\n  b: {y}")
    names = sorted({x[0] for x in a0})
    print(f"host calls compared: {len(a0)} ({sum(1 for x in a0 if x[3])} with an error text) over {len(names)} entry points; differing: {bad}")
    return 1 if bad else 0


def compare_gpu(paths):
    import numpy as np
    a0, a1, b = (dict(np.load(paths[k])) for k in ("a0", "a1", "b"))
    bad = 0
    if not (set(a0) == set(a1) == set(b)):
        print("array names differ:", sorted(set(a0) ^ set(b)) + sorted(set(a0) ^ set(a1)))
        bad += 1

    def same(x, y):
        return x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()

    def maxdiff(x, y):
        return float(np.max(np.abs(x.astype(np.float64) - y.astype(np.float64)))) if x.shape == y.shape and x.size else float("nan")

    cases = sorted({k.split("/")[0] for k in a0})
    print(f"{'case':<16}{'arrays':>7}{'a0=a1':>7}{'a0=b':>7}  launches fwd / bwd (a | b)")
    for c in cases:
        keys = [k for k in sorted(a0) if k.split("/")[0] == c and k in a1 and k in b]
        aa = [k for k in keys if same(a0[k], a1[k])]
        ab = [k for k in keys if same(a0[k], b[k])]
        ln = lambda d: " / ".join(str(int(d[k])) for k in keys if "/launches_" in k)   # noqa: E731
        print(f"{c:<16}{len(keys):>7}{len(aa):>7}{len(ab):>7}  {ln(a0)} | {ln(b)}")
        for k in keys:
            if "/launches_" in k and int(a0[k]) != int(b[k]):
                print(f"  LAUNCH COUNT {k}: {int(a0[k])} / {int(b[k])}")
                bad += 1
            if k in aa and k not in ab:
                print(f"  DIFFERENT {k}: repeats a0 = a1, but a0 / b max |diff| {maxdiff(a0[k], b[k]):.3e}")
                bad += 1
            if k not in aa:
                loss_only = a0[k].size == 1 and "/out" in k and c[0] in "abcfi"
                print(f"  not reproducible {k}: a0 / a1 max |diff| {maxdiff(a0[k], a1[k]):.3e}, a0 / b {maxdiff(a0[k], b[k]):.3e}"
                      + ("" if loss_only else "  <- NOT a fused-loss scalar of a per-clip case: the comparison cannot be trusted"))
                bad += 0 if loss_only else 1
    print(f"arrays compared: {len(a0)}; failures: {bad}")
    return 1 if bad else 0


def main(argv):
    if argv[1] == "--child":
        return gpu_child(argv[2])
    if argv[1] == "--host-child":
        return host_child(argv[2])
    host = "--host" in argv
    out_dir = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "build", "lib_compare")
    os.makedirs(out_dir, exist_ok=True)
    if "--trees" in argv:
        i = argv.index("--trees")
        lib_a = lib_b = argv[argv.index("--lib") + 1] if "--lib" in argv else os.path.join(ROOT, "egot2_amd", "libegot2x.so")
        trees = {"a0": argv[i + 1], "a1": argv[i + 1], "b": argv[i + 2]}
        print(f"# tree_a = {os.path.relpath(argv[i + 1], ROOT)}, tree_b = {os.path.relpath(argv[i + 2], ROOT)}, both on {os.path.relpath(lib_a, ROOT)} (GPU cases)")
    else:
        lib_a, lib_b = [x for x in argv[1:] if x.endswith(".so")][:2]
        trees = None
        print(f"# lib_a = {os.path.relpath(lib_a, ROOT)}, lib_b = {os.path.relpath(lib_b, ROOT)} ({'host calls' if host else 'GPU cases'})")
    paths = run_children([("a0", lib_a), ("a1", lib_a), ("b", lib_b)], out_dir, host, trees)
    rc = compare_host(paths) if host else compare_gpu(paths)
    if "--keep" not in argv:        # (a few hundred MB of gradients)
        for f in paths.values():
            os.remove(f)
    return rc


if __name__ == "__main__":
    sys.exit(main(sys.argv))
