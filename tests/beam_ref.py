"""fp64 reference of beam search for the tests (no GPU, no reference tree), on oracle.translator_ref.g_decode as tests/greedy_ref.py is:
fixed-length beams (no end-of-sequence word, no length penalty); a hypothesis' score is the sum over its steps of
log_softmax(logits)[token]; at step 0 only slot 0 is live (score 0, the others -inf); at every step the W * V candidates
score[w] + logp[w][v] of a clip are ranked, the W best survive in descending order, ties to the lowest flat index w * V + v. Below it: the
helpers tests/test_gpu_beam.py and tools/beam_eval.py share (backtracking a selection trace, the cases)."""
import torch

from oracle import translator_ref as tr


def rank(cand: torch.Tensor, k: int):
    """cand (B, N) -> values and flat indices (B, k) of the k best entries in descending order, the lowest index first among equals; a NaN
    ranks as -inf."""
    c = torch.where(torch.isnan(cand), torch.full_like(cand, float("-inf")), cand)
    vals, idx = torch.sort(c, dim=-1, descending=True, stable=True)
    return vals[:, :k], idx[:, :k]


def beam(sd64, n_heads: int, start: torch.Tensor, memory: torch.Tensor, n_steps: int, W: int):
    """start (B,) int64, memory (S, B, d) fp64 -> tokens (B, W, n_steps), scores (B, W), trace, gaps.
    trace: dict of step_tokens / step_parents / step_scores (n_steps, B, W) of every surviving slot (the parent's slot at the step before)
    and step_logits (n_steps, B, W, V), the logits row of each PARENT slot; gaps (n_steps, B, W): the differences between consecutive
    entries of the step's top W + 1 candidates (inf where fewer are finite)."""
    B = start.shape[0]
    mem = memory.repeat_interleave(W, dim=1)                        # row b * W + w
    seqs = start[:, None, None].expand(B, W, 1).clone()             # [start, tokens so far] of every slot
    scores = torch.full((B, W), float("-inf"), dtype=torch.float64)
    scores[:, 0] = 0.0
    keys = ("step_tokens", "step_parents", "step_scores", "step_logits")
    trace, gaps = {k: [] for k in keys}, []
    with torch.no_grad():
        for t in range(n_steps):
            logits = tr.g_decode(sd64, n_heads, seqs.reshape(B * W, t + 1), mem)[-1].view(B, W, -1)
            V = logits.shape[-1]
            cand = (scores[..., None] + torch.log_softmax(logits, dim=-1)).view(B, W * V)
            vals, idx = rank(cand, min(W + 1, W * V))
            if vals.shape[1] < W + 1:
                vals = torch.cat((vals, torch.full((B, W + 1 - vals.shape[1]), float("-inf"), dtype=vals.dtype)), dim=1)
            gaps.append(torch.nan_to_num(vals[:, :-1] - vals[:, 1:], nan=float("inf")))
            par, tok = idx[:, :W] // V, idx[:, :W] % V
            scores = vals[:, :W].clone()
            seqs = torch.cat((seqs.gather(1, par[..., None].expand(B, W, t + 1)), tok[..., None]), dim=2)
            for k, v in zip(keys, (tok, par.to(torch.int32), scores, logits)):
                trace[k].append(v)
    return seqs[:, :, 1:].contiguous(), scores, {k: torch.stack(v, 0) for k, v in trace.items()}, torch.stack(gaps, 0)


def backtrack(step_tokens: torch.Tensor, step_parents: torch.Tensor, t_last: int = None):
    """The sequences a selection trace ends in: step_tokens / step_parents (n, B, W) -> tokens (B, W, t_last + 1) of the slots surviving step
    t_last (default: the last step) and parents (t_last + 1, B, W): parents[t][b][k] the slot whose row produced token t of that sequence."""
    n = step_tokens.shape[0] if t_last is None else t_last + 1
    slot = torch.arange(step_tokens.shape[2]).expand(step_tokens.shape[1:]).clone()
    toks, pars = [None] * n, [None] * n
    for t in range(n - 1, -1, -1):
        toks[t] = step_tokens[t].gather(1, slot)
        slot = step_parents[t].long().gather(1, slot)
        pars[t] = slot
    return torch.stack(toks, 2), torch.stack(pars, 0)


# name: (d, heads, layers, V, S, B, n_steps, W): seeded random memories (feature seed 96), weights of greedy_ref.hoi_model (weight seed 95)
CASES = {
    "base": (256, 4, 2, 40, 16, 9, 4, 3),
    "wide_beam_long_mem": (256, 8, 2, 12, 200, 5, 3, 8),
    "lta_schedule": (512, 8, 3, 600, 8, 6, 40, 5),
    "steps64": (256, 4, 2, 40, 16, 3, 64, 2),
    "lds_extreme": (1024, 16, 1, 1024, 4, 2, 2, 8),
    "one_clip_one_step": (256, 4, 2, 12, 16, 1, 1, 2),
}
WSEED, FSEED = 95, 96


def build_case(name):
    """(model on the CPU, fp64 state dict, start token, fp64 memory (S, B, d))."""
    from tests import greedy_ref as gr
    from tests.util import seeded_feats
    d, h, L, V, S, B, n, W = CASES[name]
    m, sd64, start = gr.hoi_model(d, h, L, V, WSEED)
    return m, sd64, start, seeded_feats(FSEED, [(S, B, d)])[0].double()
