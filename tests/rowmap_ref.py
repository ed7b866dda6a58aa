"""Host restatement (numpy) of the row-map kernels' contract (include/pianobart_hip.h, "row maps for the packed step").

A position is visible when its mask value is not zero (2.0 and -1.0 are visible, -0.0 is not), and carries a loss term when any of the 8
columns of its loss-mask row is not zero. Every function works batch by batch on Python lists of positions; outputs that the kernels
leave alone keep the value they are given in `fill`, so a test compares whole buffers, gaps and guards included.
"""
import numpy as np


def visible(mask):
    return np.asarray(mask) != 0


def has_loss(loss_mask, B, S):
    return np.zeros((B, S), dtype=bool) if loss_mask is None else (np.asarray(loss_mask).reshape(B, S, 8) != 0).any(-1)


def count(emask, dmask, loss_mask):
    """counts (B,8) int32 of pb_rowmap_count."""
    B, S = dmask.shape
    ev, dv, hl = visible(emask), visible(dmask), has_loss(loss_mask, B, S)
    out = np.zeros((B, 8), dtype=np.int32)
    for b in range(B):
        pos = [s for s in range(S) if dv[b, s]]
        out[b, :5] = [int(ev[b].sum()), len(pos), sum(1 for s in range(S) if dv[b, s] or hl[b, s]), int(pos == list(range(len(pos)))),
                      int(hl[b].sum())]
    return out


def build(mask, loss_mask, off, length, row_src, row_pos, inv):
    """pb_rowmap_build on copies of the three output buffers (row_src, row_pos: 1-D; inv: (B*S,)); returns the copies."""
    B, S = mask.shape
    vis, hl = visible(mask), has_loss(loss_mask, B, S)
    row_src, row_pos, inv = row_src.copy(), row_pos.copy(), inv.copy()
    for b in range(B):
        first = [s for s in range(S) if vis[b, s]]
        second = [s for s in range(S) if not vis[b, s] and hl[b, s]]
        dead = [s for s in range(S) if not vis[b, s] and not hl[b, s]]
        order = first + second + dead
        inv[b * S:(b + 1) * S] = -1
        for n, s in enumerate(order[:int(length[b])]):
            row_src[off[b] + n] = b * S + s
            row_pos[off[b] + n] = s
            inv[b * S + s] = off[b] + n
    return row_src, row_pos, inv


def build_sub(loss_mask, present, off, length, row_src, row_idx):
    """pb_rowmap_build_sub on copies of the two output buffers; present (B*S,) is the `inv` of the existing packing."""
    B, S = np.asarray(loss_mask).shape[:2]
    hl = has_loss(loss_mask, B, S)
    row_src, row_idx = row_src.copy(), row_idx.copy()
    for b in range(B):
        first = [s for s in range(S) if hl[b, s]]
        second = [s for s in range(S) if not hl[b, s] and present[b * S + s] >= 0]
        for n, s in enumerate((first + second)[:int(length[b])]):
            row_src[off[b] + n] = b * S + s
            row_idx[off[b] + n] = present[b * S + s]
    return row_src, row_idx


def pos_grad(x, inv, out, B, S):
    """out (S,d) float64 + the sum over the batch rows b with inv[b][s] >= 0 of x[inv[b][s]], in float64."""
    acc = np.asarray(out, dtype=np.float64).copy()
    x = np.asarray(x, dtype=np.float64)
    inv = np.asarray(inv).reshape(B, S)
    for b in range(B):
        keep = inv[b] >= 0
        acc[keep] += x[inv[b][keep]]
    return acc


def shift_right(ids, sos_row):
    """(B,S,8): every sequence moved one position to the right behind the SOS row; its last row drops out."""
    out = np.roll(ids, 1, axis=1)
    out[:, 0] = sos_row
    return out
