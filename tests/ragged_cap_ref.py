"""The batch table of a ragged d = 128 batch restated in numpy (fused.h RAGGED_REC: what ragged_plan() builds on the host and the table
kernel of the capacity plan builds on the device), for tests/test_cpu_ragged_cap.py and tests/test_gpu_ragged_cap.py.

Words: B records of 16 ints | the clip of each of the sum_b ceil(S_b / 48) tiles | B * 4 packed first rows (rseg, training tables).
Record: [tile0, S, tok0, out0, outn, T_0 .. T_3, off_0 .. off_3, 0, 0, 0]; with a head out0 = tok0 and outn = S. A clip whose lengths are
all 0 (capacity plan only) is empty: a zero record, no tile, no token; its rseg entries are the running packed rows."""
import numpy as np

REC, TILE, MAX_SEG = 16, 48, 4
RG_TILE0, RG_S, RG_TOK0, RG_OUT0, RG_OUTN, RG_T, RG_OFF = 0, 1, 2, 3, 4, 5, 9


def table(lengths, train=True):
    """lengths: (B, K) ints -> (records (B, 16), tile map (tiles,), rseg (B, 4)) int32."""
    lengths = np.asarray(lengths, dtype=np.int64)
    B, K = lengths.shape
    rec = np.zeros((B, REC), dtype=np.int32)
    rseg = np.zeros((B, MAX_SEG), dtype=np.int32)
    tmap = []
    tiles = tok = 0
    rows = [0] * K
    for b in range(B):
        S = int(lengths[b].sum())
        rseg[b, :K] = rows
        if S == 0:
            continue
        off = 0
        for k in range(K):
            rec[b, RG_T + k], rec[b, RG_OFF + k] = lengths[b, k], off
            off += int(lengths[b, k])
            rows[k] += int(lengths[b, k])
        rec[b, RG_TILE0], rec[b, RG_S], rec[b, RG_TOK0], rec[b, RG_OUT0], rec[b, RG_OUTN] = tiles, S, tok, tok, S
        n = -(-S // TILE)
        tmap += [b] * n
        tiles += n
        tok += S
    return rec, np.asarray(tmap, dtype=np.int32), rseg if train else rseg[:0]


def words(lengths, train=True):
    """The flat table as egx_ragged_table_host returns it."""
    rec, tmap, rseg = table(lengths, train)
    return np.concatenate([rec.reshape(-1), tmap, rseg.reshape(-1)]).astype(np.int32)


def tile_capacity(B_cap, tok_cap):
    return -(-tok_cap // TILE) + B_cap
