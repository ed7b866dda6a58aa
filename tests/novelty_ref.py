"""A loop-and-numpy restatement of copy detection, written from the definitions: the yardstick of tests/test_novelty_cpu.py
and tests/test_novelty_gpu.py. It imports nothing of the product.

  keys_ref(ids, pad8, pitch_of, mode, start)   the key rows and key counts of (N, S, 8) ids
  runs_ref(a, b)                               the full run(p, q) table of two key lists
  outputs_ref(A, alen, B, blen, ...)           R, run_end and best of pb_shared_runs, from runs_ref
  coverage_ref(run_end_row, K)                 the share of covered keys, by the rule itself"""
import numpy as np

NO_KEY = 0xFFFFFFFF
HEAD_MAX = 1088


def length(piece, pad8):
    for r in range(piece.shape[0]):
        if any(int(piece[r, h]) >= pad8[h] for h in range(8)):
            return r
    return piece.shape[0]


def keys_one(piece, pad8, pitch_of, mode, start=0):
    """The list of keys of one (S, 8) piece: key t describes note row start + t relative to row start + t - 1."""
    L = length(piece, pad8)
    notes = [tuple(int(v) for v in piece[r]) for r in range(start, L)]
    out = []
    for t in range(1, len(notes)):
        bar, pos, _, pit = notes[t][:4]
        pbar, _, _, ppit = notes[t - 1][:4]
        if mode == 'exact':
            field = pit
        else:
            k, kp = int(pitch_of[pit]), int(pitch_of[ppit])
            field = HEAD_MAX + k - kp if k >= 0 and kp >= 0 else 2304 + pit
        step = bar - pbar
        if not 0 <= step <= 2:
            step = 3
        assert 0 <= field < 4096 and 0 <= pos < 2048
        out.append(field | (pos << 12) | (step << 23))
    return out


def keys_ref(ids, pad8, pitch_of, mode='exact', start=None):
    """(keys (N, S) uint32 with NO_KEY behind the piece's keys, klen (N))."""
    ids = np.asarray(ids)
    N, S = ids.shape[:2]
    keys = np.full((N, S), NO_KEY, dtype=np.uint32)
    klen = np.zeros(N, dtype=np.int64)
    for n in range(N):
        ks = keys_one(ids[n], pad8, pitch_of, mode, 0 if start is None else int(np.broadcast_to(start, (N,))[n]))
        keys[n, :len(ks)] = ks
        klen[n] = len(ks)
    return keys, klen


def runs_ref(a, b):
    """run[p, q] = a[p] == b[q] ? run[p - 1, q - 1] + 1 : 0 for two key lists; "no key" matches nothing."""
    run = np.zeros((len(a), len(b)), dtype=np.int64)
    for p in range(len(a)):
        for q in range(len(b)):
            if int(a[p]) == int(b[q]) and int(a[p]) != NO_KEY:
                run[p, q] = (run[p - 1, q - 1] if p > 0 and q > 0 else 0) + 1
    return run


def runs_fast(a, b):
    """runs_ref one row at a time (numpy over q): the same table for the longer rows of the device tests."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    run = np.zeros((len(a), len(b)), dtype=np.int64)
    prev = np.zeros(len(b) + 1, dtype=np.int64)
    for p in range(len(a)):
        eq = (b == a[p]) & (a[p] != NO_KEY)
        cur = np.where(eq, prev[:-1] + 1, 0)
        run[p] = cur
        prev[1:] = cur
    return run


def row_maxima(a, b):
    """max over q of run[p, q] for every p, as runs_fast computes it, without keeping the table (rows of thousands of keys)."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    out = np.zeros(len(a), dtype=np.int64)
    prev = np.zeros(len(b) + 1, dtype=np.int64)
    if len(b):
        for p in range(len(a)):
            cur = np.where((b == a[p]) & (a[p] != NO_KEY), prev[:-1] + 1, 0)
            out[p] = cur.max()
            prev[1:] = cur
    return out


class _Rows:
    """What outputs_ref needs of a run table, from its row maxima alone."""

    def __init__(self, a, b):
        self.rows = row_maxima(a, b)
        self.size = len(a) * len(b)

    def max(self, axis=None):
        return self.rows if axis == 1 else self.rows.max()


def outputs_ref(A, alen, B, blen, min_run=1, exclude_self=False, j_base=0, table=_Rows):
    """(R (N, M), run_end (N, Sa), best (N) int64) as pb_shared_runs defines them. table: runs_ref, runs_fast (the whole run table of
    a pair) or the default, their row maxima."""
    N, M, Sa = len(A), len(B), np.asarray(A).shape[1]
    R = np.zeros((N, M), dtype=np.int64)
    run_end = np.zeros((N, Sa), dtype=np.int64)
    best = np.zeros(N, dtype=np.int64)
    for i in range(N):
        top, who = 0, -1
        for j in range(M):
            if exclude_self and i == j + j_base:
                continue
            run = table(A[i][:alen[i]], B[j][:blen[j]])
            if run.size:
                R[i, j] = run.max()
                run_end[i, :alen[i]] = np.maximum(run_end[i, :alen[i]], run.max(axis=1))
            if R[i, j] > top:
                top, who = int(R[i, j]), j + j_base
        run_end[i][run_end[i] < min_run] = 0
        best[i] = (top << 32) | (0xFFFFFFFF - who) if top > 0 else 0
    return R, run_end, best


def coverage_ref(run_end_row, K):
    """Key p is covered if some e >= p has run_end[e] >= e - p + 1. nan for K = 0."""
    if K == 0:
        return float('nan')
    covered = 0
    for p in range(K):
        if any(int(run_end_row[e]) >= e - p + 1 for e in range(p, K)):
            covered += 1
    return covered / K


def synth_pieces(pad8, N, S, seed, pitches=None, positions=None, bars_step=(0, 0, 0, 1)):
    """N pieces of S rows with ragged lengths: bars that never go back, ordinary ids everywhere, an EOS row and a PAD tail. A small
    `pitches` / `positions` alphabet makes shared runs happen by chance."""
    rng = np.random.default_rng(seed)
    pad8 = np.asarray(pad8)
    ids = np.zeros((N, S, 8), dtype=np.int64)
    for n in range(N):
        L = S if n == 0 else int(rng.integers(0, S + 1))
        rows = np.stack([rng.integers(0, pad8[h], size=L) for h in range(8)], axis=1)
        if L:
            rows[:, 0] = np.minimum(np.cumsum(rng.choice(bars_step, size=L)), pad8[0] - 1)
            if pitches is not None:
                rows[:, 3] = rng.choice(pitches, size=L)
            if positions is not None:
                rows[:, 1] = rng.choice(positions, size=L)
        ids[n, :L] = rows
        if L < S:
            ids[n, L] = pad8 + 3
            ids[n, L + 1:] = pad8
    return ids
