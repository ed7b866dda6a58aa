"""Host restatement (numpy) of pb_augment (include/pianobart_hip.h, csrc/pb_augment.hip): table look-ups, the piece's extremes, the clamp,
the multiply-high draw from the Philox stream that tests/philox_ref.py restates, and the apply pass. Integer arithmetic: the GPU tests
compare every byte and every shift with ==.

  coord, id_at  (3, 1088) int16 arrays, plan (3, 6) integers (lo, hi, blo, bhi, ncoord, thresh): the fields of augment.AugmentPlan
  reference(ids, coord, id_at, plan, seed) -> (out, shifts)       ids (B, S, 8) integers; out like ids, shifts (B, 3) int64
"""
import numpy as np

from tests.philox_ref import philox4x32

HEADS = (3, 5, 7)                 # the head of axis 0 pitch, 1 velocity, 2 tempo
HEAD_MAX = 1088                   # the stride of the tables
ALWAYS = 0xFFFFFFFF
ROUNDS = 7                        # pb_common.h's philox4x32


def coords(ids, coord, plan, a):
    """(B, S) int64: the coordinate of every position on axis a, -1 where the id has none (or lies outside the tables)."""
    col = np.asarray(ids)[:, :, HEADS[a]].astype(np.int64) & 0xFFFF             # the kernel reads the 16 bits as unsigned
    inside = col < HEAD_MAX
    c = np.where(inside, np.asarray(coord)[a].astype(np.int64)[np.where(inside, col, 0)], -1)
    return np.where(c < int(plan[a][4]), c, -1)


def draw(seed, B, a):
    """(x, y) uint64 arrays of B words each: the first two words of philox4x32(0, b, a, 0xA06) under the key (seed low, seed high)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    b = np.arange(B, dtype=np.uint64)
    w = philox4x32(np.zeros(B, dtype=np.uint64), b, np.full(B, a, dtype=np.uint64), np.full(B, 0xA06, dtype=np.uint64),
                   np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32), ROUNDS)
    return w[0], w[1]


def shifts_of(ids, coord, plan, seed):
    """(B, 3) int64: steps 1 - 4 of the contract."""
    B = np.asarray(ids).shape[0]
    out = np.zeros((B, 3), dtype=np.int64)
    for a in range(3):
        lo, hi, blo, bhi, _, thresh = (int(v) for v in plan[a])
        thresh &= 0xFFFFFFFF
        c = coords(ids, coord, plan, a)
        x, y = draw(seed, B, a)
        some = (c >= 0).any(axis=1)
        cmin, cmax = np.where(c >= 0, c, HEAD_MAX).min(axis=1), c.max(axis=1)
        flo, fhi = np.maximum(lo, blo - cmin), np.minimum(hi, bhi - cmax)
        ok = some & (flo <= 0) & (fhi >= 0)
        w = np.where(ok, fhi - flo + 1, 1).astype(np.uint64)                    # <= 1088: the 32 x 11 bit product fits uint64
        s = flo + ((x * w) >> np.uint64(32)).astype(np.int64)
        if thresh != ALWAYS:
            s = np.where(y >= np.uint64(thresh), 0, s)
        out[:, a] = np.where(ok, s, 0)
    return out


def apply_shifts(ids, coord, id_at, plan, shifts):
    """Step 5: every id with a coordinate moves by its piece's shift; everything else, the other five heads included, is copied."""
    ids = np.asarray(ids)
    out = ids.copy()
    for a in range(3):
        c = coords(ids, coord, plan, a)
        moved = np.asarray(id_at)[a].astype(np.int64)[np.clip(c + np.asarray(shifts)[:, a][:, None], 0, HEAD_MAX - 1)]
        out[:, :, HEADS[a]] = np.where(c >= 0, moved, ids[:, :, HEADS[a]]).astype(ids.dtype)
    return out


def reference(ids, coord, id_at, plan, seed):
    s = shifts_of(ids, coord, plan, seed)
    return apply_shifts(ids, coord, id_at, plan, s), s
