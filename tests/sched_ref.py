"""fp64 reference of scheduled greedy generation and beam search for the tests (no GPU, no reference tree), on
oracle.translator_ref.g_decode as tests/greedy_ref.py and tests/beam_ref.py are. `allowed` is the (P, V) bool table of a token schedule:
step t (0-based) may emit the words of row t % P, every other word's logit is -inf BEFORE the argmax (greedy) or the log_softmax and the
ranking (beam), so the normaliser sums the set's words only: Categorical(logits=head_x[..., v_idx]) of
HOI/models/lta/lta_models_seqdecoder.py:190-216. Unlike that loop the fed-back word is the subset's argmax. Below them: the standard
verb / noun alternation of the tests."""
import torch

from oracle import translator_ref as tr
from tests import beam_ref as br, greedy_ref as gr

NEG_INF = float("-inf")


def mask(logits: torch.Tensor, allowed: torch.Tensor, t: int) -> torch.Tensor:
    """logits (..., V) with -inf outside row t % P of `allowed`."""
    return logits.masked_fill(~allowed[t % allowed.shape[0]], NEG_INF)


def finite_margin(logits: torch.Tensor) -> torch.Tensor:
    """Largest minus second-largest FINITE entry of every row (inf where a row has one finite entry)."""
    if logits.shape[-1] < 2:
        return torch.full(logits.shape[:-1], float("inf"), dtype=logits.dtype)
    top = logits.topk(2, dim=-1).values
    return torch.where(torch.isfinite(top[..., 1]), top[..., 0] - top[..., 1], torch.full_like(top[..., 0], float("inf")))


def greedy(sd64, n_heads: int, start: torch.Tensor, memory: torch.Tensor, n_steps: int, allowed: torch.Tensor):
    """greedy_ref.greedy under a schedule: tokens (B, n_steps), masked logits (n_steps, B, V), margins (n_steps, B) = the top-2 margin over
    the finite entries of each row."""
    B = start.shape[0]
    toks = torch.empty((B, n_steps + 1), dtype=torch.int64)
    toks[:, 0] = start
    rows = []
    with torch.no_grad():
        for t in range(n_steps):
            last = mask(tr.g_decode(sd64, n_heads, toks[:, :t + 1], memory)[-1], allowed, t)
            rows.append(last)
            toks[:, t + 1] = gr.argmax_lowest(last)
    logits = torch.stack(rows, 0)
    return toks[:, 1:].contiguous(), logits, finite_margin(logits)


def beam(sd64, n_heads: int, start: torch.Tensor, memory: torch.Tensor, n_steps: int, W: int, allowed: torch.Tensor):
    """beam_ref.beam under a schedule (same returns; step_logits are the masked rows): log_softmax after masking, ranked by beam_ref.rank."""
    B = start.shape[0]
    mem = memory.repeat_interleave(W, dim=1)
    seqs = start[:, None, None].expand(B, W, 1).clone()
    scores = torch.full((B, W), NEG_INF, dtype=torch.float64)
    scores[:, 0] = 0.0
    keys = ("step_tokens", "step_parents", "step_scores", "step_logits")
    trace, gaps = {k: [] for k in keys}, []
    with torch.no_grad():
        for t in range(n_steps):
            logits = mask(tr.g_decode(sd64, n_heads, seqs.reshape(B * W, t + 1), mem)[-1].view(B, W, -1), allowed, t)
            V = logits.shape[-1]
            cand = (scores[..., None] + torch.log_softmax(logits, dim=-1)).view(B, W * V)
            vals, idx = br.rank(cand, min(W + 1, W * V))
            if vals.shape[1] < W + 1:
                vals = torch.cat((vals, torch.full((B, W + 1 - vals.shape[1]), NEG_INF, dtype=vals.dtype)), dim=1)
            gaps.append(torch.nan_to_num(vals[:, :-1] - vals[:, 1:], nan=float("inf")))
            par, tok = idx[:, :W] // V, idx[:, :W] % V
            scores = vals[:, :W].clone()
            seqs = torch.cat((seqs.gather(1, par[..., None].expand(B, W, t + 1)), tok[..., None]), dim=2)
            for k, v in zip(keys, (tok, par.to(torch.int32), scores, logits)):
                trace[k].append(v)
    return seqs[:, :, 1:].contiguous(), scores, {k: torch.stack(v, 0) for k, v in trace.items()}, torch.stack(gaps, 0)


def alternation(V: int, first: range, second: range) -> torch.Tensor:
    """(2, V) bool: row 0 the words of `first`, row 1 the words of `second`."""
    allowed = torch.zeros((2, V), dtype=torch.bool)
    allowed[0, list(first)] = True
    allowed[1, list(second)] = True
    return allowed


def standard_alternation() -> torch.Tensor:
    """The tests' alternation at V = 40: row 0 = words 5..16, row 1 = words 17..39."""
    return alternation(40, range(5, 17), range(17, 40))


def strict_case():
    """The strict-token case the CPU and the GPU tests share: d 256, 4 heads, 2 layers, V 40, weight seed 98, S 16, B 32, memory
    seeded_feats(96, [(16, 32, 256)]), 3 steps, the standard alternation, start tokens randint(0, 40, (32,), manual_seed(3)).
    Returns (model on the CPU, fp64 state dict, start (32,), fp64 memory, allowed, n_steps)."""
    from tests.util import seeded_feats
    m, sd64, _ = gr.hoi_model(256, 4, 2, 40, 98)
    start = torch.randint(0, 40, (32,), generator=torch.Generator().manual_seed(3))
    return m, sd64, start, seeded_feats(96, [(16, 32, 256)])[0].double(), standard_alternation(), 3
