"""Reference of egx_lta_validate (include/egot2x.h), its cases and planted inputs: the gate of test_gpu_lta_val.py.

Three parts, none of which calls the library:
  * the metric: the textbook Levenshtein recurrence and `aued`, the literal loop of HOI/evaluation/lta/lta_metrics.py:86-114 (per prefix
    length, per clip, the minimum over the K sequences of distance / prefix length; the mean over clips; trapz over the prefix lengths);
    `min_dist` / `dist_sum` are the integers behind it in the layouts the kernel writes;
  * the sampler's gate: `uniforms` restates which word of the library's counter generator (tests/dropmask.py: site_key, rand_quad) draw k
    of row (b, z) of head h reads, `cdf64` is the running sum of the fp64 softmax, and `check_draws` holds EVERY draw j to
    cdf64[j - 1] - tol <= u <= cdf64[j] + tol. TOL = 1e-5 is the one tolerance: about 5x the worst |cdf32 - cdf64| of a plain sequential
    fp32 chain over 2048 classes (1.7e-6 on 3 * randn logits; 64-chunk blocked accumulation gives 3.3e-7 at C = 2048, 5.4e-7 at C = 478),
    which leaves room for the device's exp. No draw is exempt;
  * `sample_f32` (inverse-cdf sampling restated in fp32 torch) and its perturbed versions, which test_cpu_lta_val.py holds against the gate.
"""
from __future__ import annotations

import numpy as np
import torch

from tests.dropmask import rand_quad, site_key

TOL = 1e-5
_trapz = getattr(np, "trapezoid", None) or np.trapz        # np.trapz of the reference; renamed in numpy 2
LTA_VAL_KEY_LAYER = 0x17A          # csrc/lta_val.hip: key = site_key(seed, 0x17A, site = h)
MAX_K, MAX_Z, MAX_C, MAX_H = 8, 64, 2048, 4

# (B, Z, classes, K, ld, col0): ld / col0 None = the heads side by side in a row of sum(classes) columns (what decode() builds)
CASES = [
    (1, 1, (1,), 1, None, None),                    # one class, Z = 1
    (3, 2, (5, 7), 1, None, None),                  # planted ties: the lowest index wins
    (6, 3, (5, 7), 5, None, None),                  # the small LTA model of the tests
    (4, 20, (115, 478), 5, None, None),             # the recipe's heads, read in place from a (B, Z, 593) stack
    (2, 64, (2048, 1), 8, None, None),              # every limit at once
    (257, 2, (5,), 2, None, None),                  # more clips than any workgroup holds
    (5, 4, (5, 7), 3, 19, (1, 9)),                  # odd ld, uncovered columns 0, 6..8 and 16..18
    (6, 3, (9, 33), 4, None, None),                 # the planted rows: +80 / -80, probability 1, -inf classes, a NaN row
]
PLANTED = 7


def case_id(case) -> str:
    B, Z, classes, K, ld, _ = case
    return f"B{B}_Z{Z}_C{'x'.join(map(str, classes))}_K{K}" + (f"_ld{ld}" if ld else "")


def case_layout(case):
    B, Z, classes, K, ld, col0 = case
    if ld is None:
        ld, col0 = sum(classes), tuple(int(c) for c in np.cumsum((0,) + tuple(classes))[:-1])
    return ld, col0


def val_inputs(i: int):
    """-> (stack (B, Z, ld) fp32, labels (B, Z, H) int64) of case i, seeded. Columns no head covers hold 1e30 (reading one would show)."""
    B, Z, classes, K, _, _ = CASES[i]
    ld, col0 = case_layout(CASES[i])
    g = torch.Generator(device="cpu").manual_seed(7300 + i)
    stack = torch.full((B, Z, ld), 1e30, dtype=torch.float32)
    for c0, c in zip(col0, classes):
        stack[..., c0:c0 + c] = 3 * torch.randn(B, Z, c, generator=g)
    labels = torch.stack([torch.randint(0, c, (B, Z), generator=g) for c in classes], dim=-1)
    if i == 1:          # ties at the maximum: classes 1 and 3 of head 0, 2 / 4 / 6 of head 1, and an all-equal row
        stack[0, 0, col0[0] + 1] = stack[0, 0, col0[0] + 3] = 9.0
        stack[1, 1, col0[1] + 2] = stack[1, 1, col0[1] + 4] = stack[1, 1, col0[1] + 6] = 11.0
        stack[2, 0, col0[0]:col0[0] + classes[0]] = 0.25
    if i == PLANTED:
        w0, w1 = slice(col0[0], col0[0] + classes[0]), slice(col0[1], col0[1] + classes[1])
        stack[0, 0, w0] = -80.0
        stack[0, 0, col0[0] + 2] = 80.0                         # +80 / -80: class 2 at probability 1 (to 1e-69)
        stack[0, 1, w1] = -float("inf")
        stack[0, 1, col0[1] + 32] = 0.5                         # one class at probability 1: the LAST one (u * S can round to S)
        stack[1, 0, w1] = 3 * torch.randn(classes[1], generator=g)
        stack[1, 0, col0[1]:col0[1] + 33:2] = -float("inf")     # -inf classes, the first and the last among them
        stack[1, 1, w0] = 1.0
        stack[1, 1, col0[0] + 4] = float("nan")                 # a NaN row: token -1
        stack[2, 2, w1] = -float("inf")                         # no finite logit: token -1
        labels[1, 1, 0] = -1                                    # a label of -1 does not match the token -1
    return stack, labels


def heads_of(stack, case):
    ld, col0 = case_layout(case)
    return [stack[..., c0:c0 + c] for c0, c in zip(col0, case[2])]


# ---- the metric -------------------------------------------------------------------------------------------------------------------------
def levenshtein(a, b) -> int:
    """Insertions, deletions and substitutions that turn sequence a into b: the textbook recurrence, row by row."""
    a, b = [int(x) for x in a], [int(x) for x in b]
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[-1]


def levenshtein_table(a, b):
    """The whole (len(a) + 1, len(b) + 1) table D; D[i][j] = levenshtein(a[:i], b[:j])."""
    a, b = [int(x) for x in a], [int(x) for x in b]
    D = [list(range(len(b) + 1))]
    for i, x in enumerate(a, 1):
        row = [i]
        for j, y in enumerate(b, 1):
            row.append(min(D[i - 1][j] + 1, row[j - 1] + 1, D[i - 1][j - 1] + (x != y)))
        D.append(row)
    return D


def edit_distance(preds, labels) -> float:
    """lta_metrics.py:86-96. preds (N, Z, K), labels (N, Z) -> mean over n of min over k of distance / Z."""
    N, Z, K = preds.shape
    dists = []
    for n in range(N):
        dists.append(min([levenshtein(preds[n, :, k], labels[n]) / Z for k in range(K)]))
    return np.mean(dists)


def aued(preds, labels) -> dict:
    """lta_metrics.py:103-114, literally. preds (N, Z, K), labels (N, Z, 1) integer arrays / tensors -> {"AUED", "ED_0", ...} (arrays (1,))."""
    preds, labels = np.asarray(preds), np.asarray(labels)
    N, Z, K = preds.shape
    labels = labels.squeeze(-1)
    ED = np.vstack([edit_distance(preds[:, :z], labels[:, :z]) for z in range(1, Z + 1)])
    with np.errstate(invalid="ignore", divide="ignore"):
        AUED = _trapz(y=ED, axis=0) / (Z - 1)
    output = {"AUED": AUED}
    output.update({f"ED_{z}": ED[z] for z in range(Z)})
    return output


def min_dist(tokens, labels) -> torch.Tensor:
    """tokens: list of H (B, K, Z) int64, labels (B, Z, H) -> int32 (B, Z, H): min over k of levenshtein(tokens[h][b, k, :z + 1],
    labels[b, :z + 1, h]), every prefix computed on its own; a negative token equals no label."""
    B, K, Z = tokens[0].shape
    out = torch.zeros(B, Z, len(tokens), dtype=torch.int32)
    for h, t in enumerate(tokens):
        t = t.clone()
        t[t < 0] = -(2 ** 62)                       # matches no label, -1 included
        for b in range(B):
            lab = labels[b, :, h].tolist()
            rows = [t[b, k].tolist() for k in range(K)]
            for z in range(Z):
                out[b, z, h] = min(levenshtein(r[:z + 1], lab[:z + 1]) for r in rows)
    return out


def step_result(dist_sum, B: int, prefix: str = "val") -> dict:
    """The reference's validation step_result from dist_sum (Z, H): ED_z = dist_sum[z, h] / (B (z + 1)), AUED = trapz / (Z - 1)."""
    ds = np.asarray(dist_sum, dtype=np.float64)
    Z, H = ds.shape
    res = {}
    for h in range(H):
        ed = ds[:, h] / (B * np.arange(1, Z + 1, dtype=np.float64))
        with np.errstate(invalid="ignore", divide="ignore"):
            res[f"{prefix}_{h}_AUED"] = float(_trapz(y=ed) / (Z - 1))
        for z in range(Z):
            res[f"{prefix}_{h}_ED_{z}"] = float(ed[z])
    return res


# ---- the sampler's gate -------------------------------------------------------------------------------------------------------------------
def uniforms(seed: int, B: int, Z: int, H: int, K: int) -> np.ndarray:
    """-> float64 (H, B, Z, K): u of draw k of row b * Z + z of head h = (w + 0.5) / 2^32, w = word k of the row: rand_quad(key, row, k >> 1),
    its first word for even k, its second for odd k; key = site_key(seed, LTA_VAL_KEY_LAYER, h)."""
    rows = np.arange(B * Z, dtype=np.int64).reshape(B, Z, 1)
    k = np.arange(K, dtype=np.int64).reshape(1, 1, K)
    out = np.empty((H, B, Z, K), dtype=np.float64)
    for h in range(H):
        zw, yw = rand_quad(site_key(seed, LTA_VAL_KEY_LAYER, h), rows, k >> 1)
        w = np.where((k & 1) != 0, yw, zw)
        out[h] = (w.astype(np.float64) + 0.5) / 4294967296.0
    return out


def cdf64(logits: torch.Tensor) -> torch.Tensor:
    """Running sum over the last axis of the fp64 softmax of `logits` (promoted). A row that cannot be sampled gives NaNs."""
    return torch.cumsum(torch.softmax(logits.double(), dim=-1), dim=-1)


def samplable(logits: torch.Tensor) -> torch.Tensor:
    """Rows with a distribution: no NaN, no +inf, a finite logit. The others yield token -1."""
    m = logits.max(dim=-1).values
    return ~torch.isnan(logits).any(dim=-1) & torch.isfinite(m)


def check_draws(tokens: torch.Tensor, logits: torch.Tensor, u, tol: float = TOL):
    """tokens (B, K, Z) int64 of ONE head, logits (B, Z, C), u (B, Z, K) -> (ok, worst): every draw j = tokens[b, k, z] must satisfy
    cdf64[j - 1] - tol <= u <= cdf64[j] + tol (cdf64[-1] = 0), must be a class in [0, C) and must not be a class of probability 0; on a row
    that cannot be sampled it must be -1. `worst` is the largest amount by which a draw leaves [cdf64[j - 1], cdf64[j]] (0: inside); a
    draw that is not a class at all counts as inf."""
    B, Z, C = logits.shape
    tok = tokens.permute(0, 2, 1)                                   # (B, Z, K)
    u = torch.as_tensor(np.asarray(u), dtype=torch.float64)
    good = samplable(logits)
    cdf = torch.cat([torch.zeros(B, Z, 1, dtype=torch.float64), cdf64(torch.where(good[..., None], logits, torch.zeros_like(logits)))], dim=-1)
    prob0 = torch.isneginf(logits)
    in_range = (tok >= 0) & (tok < C)
    j = tok.clamp(0, C - 1)
    lo, hi = torch.gather(cdf, 2, j), torch.gather(cdf, 2, j + 1)
    slack = torch.maximum(lo - u, u - hi).clamp_min(0.0)
    slack = torch.where(in_range & ~torch.gather(prob0, 2, j), slack, torch.full_like(slack, float("inf")))
    slack = torch.where(good[..., None], slack, torch.where(tok == -1, torch.zeros_like(slack), torch.full_like(slack, float("inf"))))
    worst = float(slack.max())
    return worst <= tol, worst


def sample_f32(logits: torch.Tensor, u, perturb: str | None = None, u_other=None, logits_other=None) -> torch.Tensor:
    """Inverse-cdf sampling restated in fp32 torch: logits (B, Z, C) fp32, u (B, Z, K) -> tokens (B, K, Z). The cdf is a plain fp32 cumsum of
    the fp32 max-subtracted exponentials, compared unnormalised (u * total). perturb: one deliberate mistake -
      "shift_bin"    every draw one class further (wrapping);
      "other_seed"   the uniforms of another seed (u_other);
      "reuse_draw0"  draw k reads draw 0's uniform;
      "wrong_window" the logits of another head's columns (logits_other, C columns of it)."""
    u = torch.as_tensor(np.asarray(u_other if perturb == "other_seed" else u), dtype=torch.float64)
    if perturb == "reuse_draw0":
        u = u[..., :1].expand_as(u)
    x = (logits_other if perturb == "wrong_window" else logits).float()
    good = samplable(x)
    xs = torch.where(good[..., None], x, torch.zeros_like(x))
    e = torch.exp(xs - xs.max(dim=-1, keepdim=True).values)
    cdf = torch.cumsum(e, dim=-1, dtype=torch.float32)
    t = (u * cdf[..., -1:].double()).float()
    j = (cdf[..., None, :] <= t[..., :, None]).sum(dim=-1)          # (B, Z, K): classes whose cdf is <= u * total
    last = (torch.arange(x.shape[-1]) * (e > 0)).max(dim=-1).values
    j = torch.minimum(j, last[..., None])
    if perturb == "shift_bin":
        j = (j + 1) % x.shape[-1]
    j = torch.where(good[..., None], j, torch.full_like(j, -1))
    return j.permute(0, 2, 1).contiguous()


PERTURBATIONS = ("shift_bin", "other_seed", "reuse_draw0", "wrong_window")


def argmax_lowest(logits: torch.Tensor) -> torch.Tensor:
    """(B, Z, C) -> (B, 1, Z): the row argmax, the lowest index among equal logits (decoder._argmax_lowest); -1 on a row that cannot be sampled."""
    C = logits.shape[-1]
    good = samplable(logits)
    x = torch.where(good[..., None], logits, torch.zeros_like(logits))
    idx = torch.arange(C).expand_as(x)
    j = torch.where(x == x.max(dim=-1, keepdim=True).values, idx, C).min(dim=-1).values
    return torch.where(good, j, torch.full_like(j, -1)).unsqueeze(1)
