"""A loop-and-numpy restatement of local alignment for copy detection, written from the contract: the yardstick of
tests/test_align_cpu.py and tests/test_align_gpu.py. It imports nothing of the product.

  table_ref(a, b, match, mismatch, gap)        the full table of packed cells P(p, q) of two key lists, by the plain triple loop
  pair_ref(a, b, ...)                          (score, the row maxima of P over match cells) of a pair, from table_ref
  batch_fast(A, alen, B, blen, ...)            the same two for every pair of two sets of rows, one anti-diagonal at a time (numpy)
  pair_fast(a, b, ...)                         batch_fast for one pair
  sw_unpacked(a, b, ...)                       textbook Smith-Waterman scores, no packing, no start: what P >> 12 must equal
  outputs_ref(A, alen, B, blen, ...)           score, align_end and best of pb_local_align
  coverage_ref(align_end_row, K)               the share of covered keys, by the rule itself"""
import numpy as np

NO_KEY = 0xFFFFFFFF
DEFAULTS = (1, 2, 2)                           # match, mismatch, gap; min_score = 8


def _is_match(x, y):
    return int(x) == int(y) and not (int(x) >> 31) & 1


def table_ref(a, b, match=1, mismatch=2, gap=2):
    """P[p, q] = H << 12 | (4095 - start), 0 = no alignment ends here; the recurrence of DESIGN.md 12, cell by cell."""
    P = np.zeros((len(a), len(b)), dtype=np.int64)
    for p in range(len(a)):
        for q in range(len(b)):
            s = match if _is_match(a[p], b[q]) else -mismatch
            diag = P[p - 1, q - 1] if p > 0 and q > 0 else 0
            up = P[p - 1, q] if p > 0 else 0
            left = P[p, q - 1] if q > 0 else 0
            d = max(diag, 4095 - p) + s * 4096
            r = max(d, up - gap * 4096, left - gap * 4096)
            P[p, q] = r if r >= 4096 else 0
    return P


def match_cells(a, b):
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    return (a[:, None] == b[None, :]) & ((a[:, None] >> 31) & 1 == 0)


def pair_ref(a, b, match=1, mismatch=2, gap=2):
    """(score, rows): the maximum of H over match cells and, for every p, the maximum of P over the match cells of row p."""
    if not len(a) or not len(b):
        return 0, np.zeros(len(a), dtype=np.int64)
    P = np.where(match_cells(a, b), table_ref(a, b, match, mismatch, gap), 0)
    return int(P.max()) >> 12, P.max(axis=1)


def batch_fast(A, alen, B, blen, match=1, mismatch=2, gap=2):
    """(score (N, M), rows (N, M, Sa)) of every pair of the key rows A (N, Sa) and B (M, Sb): pair_ref without the tables. The cells of
    one anti-diagonal t = p + q depend on the two diagonals before only, so they are computed together (numpy over p, and over the
    pairs). Keys behind a row's length are replaced by NO_KEY: such a cell never matches, so it is never recorded, and it feeds only
    cells further right or further down, which lie outside the pair's rectangle too. Arrays are indexed by p + 1; entry 0 is the row
    above the table."""
    A, B = np.asarray(A, dtype=np.int64), np.asarray(B, dtype=np.int64)
    (N, Sa), M = A.shape, len(B)
    Sb = B.shape[1] if M else 0
    rows = np.zeros((N, M, Sa), dtype=np.int64)
    if not N or not M or not Sb:
        return np.zeros((N, M), dtype=np.int64), rows
    Ka, Kb = np.clip(np.asarray(alen, dtype=np.int64), 0, Sa), np.clip(np.asarray(blen, dtype=np.int64), 0, Sb)
    A = np.where(np.arange(Sa)[None, :] < Ka[:, None], A, NO_KEY)
    B = np.where(np.arange(Sb)[None, :] < Kb[:, None], B, NO_KEY)
    key_ok = (A >> 31) & 1 == 0
    prev1, prev2 = np.zeros((N, M, Sa + 1), dtype=np.int64), np.zeros((N, M, Sa + 1), dtype=np.int64)      # diagonals t - 1 and t - 2
    for t in range(int(Ka.max()) + int(Kb.max()) - 1):
        lo, hi = max(0, t - Sb + 1), min(Sa - 1, t)                  # the rows p of this diagonal
        p = np.arange(lo, hi + 1)
        eq = (A[:, None, lo:hi + 1] == B[None, :, t - p]) & key_ok[:, None, lo:hi + 1]
        s = np.where(eq, match, -mismatch) * 4096
        diag, up, left = prev2[:, :, lo:hi + 1], prev1[:, :, lo:hi + 1], prev1[:, :, lo + 1:hi + 2]      # (p - 1, q - 1), (p - 1, q), (p, q - 1)
        r = np.maximum(np.maximum(diag, 4095 - p) + s, np.maximum(up, left) - gap * 4096)
        r = np.where(r >= 4096, r, 0)
        cur = np.zeros((N, M, Sa + 1), dtype=np.int64)
        cur[:, :, lo + 1:hi + 2] = r
        rows[:, :, lo:hi + 1] = np.maximum(rows[:, :, lo:hi + 1], np.where(eq, r, 0))
        prev2, prev1 = prev1, cur
    return rows.max(axis=2) >> 12, rows


def pair_fast(a, b, match=1, mismatch=2, gap=2):
    """pair_ref by batch_fast, for one pair of key lists."""
    if not len(a) or not len(b):
        return 0, np.zeros(len(a), dtype=np.int64)
    score, rows = batch_fast([a], [len(a)], [b], [len(b)], match, mismatch, gap)
    return int(score[0, 0]), rows[0, 0]


def sw_unpacked(a, b, match=1, mismatch=2, gap=2):
    """H[p, q] of textbook Smith-Waterman with a linear gap penalty: max(0, diagonal + s, up - gap, left - gap)."""
    H = np.zeros((len(a) + 1, len(b) + 1), dtype=np.int64)
    for p in range(1, len(a) + 1):
        for q in range(1, len(b) + 1):
            s = match if _is_match(a[p - 1], b[q - 1]) else -mismatch
            H[p, q] = max(0, H[p - 1, q - 1] + s, H[p - 1, q] - gap, H[p, q - 1] - gap)
    return H[1:, 1:]


def outputs_ref(A, alen, B, blen, match=1, mismatch=2, gap=2, min_score=1, exclude_self=False, j_base=0, pair=None):
    """(score (N, M), align_end (N, Sa), best (N) int64) as pb_local_align defines them, from batch_fast or, with pair=pair_ref, from the
    plain loops pair by pair."""
    N, M, Sa = len(A), len(B), np.asarray(A).shape[1]
    Sb = np.asarray(B).shape[1] if M else 0
    if pair is None:
        score, rows = batch_fast(A, alen, B, blen, match, mismatch, gap)
    else:
        score, rows = np.zeros((N, M), dtype=np.int64), np.zeros((N, M, Sa), dtype=np.int64)
        for i in range(N):
            Ka = min(max(int(alen[i]), 0), Sa)
            for j in range(M):
                score[i, j], rows[i, j, :Ka] = pair(A[i][:Ka], B[j][:min(max(int(blen[j]), 0), Sb)], match, mismatch, gap)
    align_end = np.zeros((N, Sa), dtype=np.int64)
    best = np.zeros(N, dtype=np.int64)
    for i in range(N):
        top, who = 0, -1
        for j in range(M):
            if exclude_self and i == j + j_base:
                score[i, j] = 0
                continue
            align_end[i] = np.maximum(align_end[i], rows[i, j])
            if score[i, j] > top:
                top, who = int(score[i, j]), j + j_base
        align_end[i][(align_end[i] >> 12) < min_score] = 0
        best[i] = (top << 32) | (0xFFFFFFFF - who) if top > 0 else 0
    return score, align_end, best


def split_ref(v):
    """(H, start) of one packed value; start is None for 0."""
    v = int(v)
    return (v >> 12, 4095 - (v & 4095)) if v else (0, None)


def coverage_ref(align_end_row, K):
    """Key p is covered if some e >= p has a non-zero align_end[e] whose start is <= p. nan for K = 0."""
    if K == 0:
        return float('nan')
    covered = 0
    for p in range(K):
        if any(int(align_end_row[e]) != 0 and split_ref(align_end_row[e])[1] <= p for e in range(p, K)):
            covered += 1
    return covered / K


# ---- inputs of the device tests ----------------------------------------------------------------------------------------------------------
ALPHABET = np.array([pit | pos << 12 for pit in (60, 62, 64) for pos in (0, 4)], dtype=np.uint32)      # 3 pitches x 2 positions
GENTLE = (2, 1, 1)                             # the scoring under which random rows over ALPHABET align beyond their exact runs


def rows(rng, lens, S, alphabet=ALPHABET):
    """Key rows of the given lengths over the alphabet, NO_KEY behind."""
    keys = np.full((len(lens), S), NO_KEY, dtype=np.uint32)
    for n, K in enumerate(lens):
        keys[n, :K] = rng.choice(alphabet, size=K)
    return keys


def distinct_keys(n, lo=0):
    """n keys lo, lo + 1, ... spread over the pitch and position fields: all different, bit 31 clear. The ground for planted copies:
    nothing matches by chance."""
    x = np.arange(lo, lo + n, dtype=np.int64)
    assert lo + n <= 1 << 23
    return ((x % 4096) | ((x // 4096) << 12)).astype(np.uint32)


def longest_runs(a, b):
    """The longest exact run two key lists share (the R of pb_shared_runs), one row at a time."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    prev = np.zeros(len(b) + 1, dtype=np.int64)
    top = 0
    if len(b):
        for p in range(len(a)):
            cur = np.where((b == a[p]) & ((a[p] >> 31) & 1 == 0), prev[:-1] + 1, 0)
            top = max(top, int(cur.max()))
            prev[1:] = cur
    return top


def edge_lengths(W):
    """The row lengths of the device test over every pair: nothing, under a lane's columns, a lane's columns and one more, on both
    sides of one block (W columns), two blocks and one more, four blocks less one."""
    c = W // 64
    return [0, 1, 2, c, c + 1, W - 1, W, W + 1, 2 * W + 1, 1023]


def edge_set(W, seed=31):
    """(A, alen, B, blen): random rows over ALPHABET of every length of edge_lengths(W), in windows of 1 023 and 1 024 keys."""
    rng = np.random.default_rng(seed)
    lens = edge_lengths(W)
    return rows(rng, lens, 1023), np.array(lens), rows(rng, lens, 1024), np.array(lens)


def tile_set(N, M, seed, S=64):
    """(A, alen, B, blen): N x M random rows over ALPHABET of 48 .. S keys in windows of S and S - 3 keys. With M > 2 corpus row 1 fills
    its window and the last corpus row repeats it, and generated row 0 repeats it too: wherever row 1 holds the best score there is a
    tie across j, and for row 0 it does."""
    rng = np.random.default_rng(seed)
    alen, blen = rng.integers(48, S + 1, size=N), rng.integers(48, S - 2, size=M)
    A, B = rows(rng, alen, S), rows(rng, blen, S - 3)
    if M > 2:
        B[1], blen[1] = rows(rng, [S - 3], S - 3)[0], S - 3
        B[M - 1], blen[M - 1] = B[1], blen[1]
        A[0, :S - 3], alen[0] = B[1], S - 3
        A[0, S - 3:] = NO_KEY
    return A, alen, B, blen


_CACHE = {}


def cached(key, make):
    """make() once per key: the tests share a reference output and leave it unchanged."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def at_min_score(align_end, min_score):
    """The align_end of a larger min_score from that of min_score = 1: entries whose score falls short are 0."""
    return np.where((align_end >> 12) >= min_score, align_end, 0)


def edge_outputs(W):
    """edge_set(W) and its (score, align_end, best) under GENTLE at min_score = 1, computed once."""
    def make():
        s = edge_set(W)
        return s + outputs_ref(*s, *GENTLE, min_score=1)
    return cached(('edge', W), make)


def tile_outputs(N, M, seed):
    """tile_set(N, M, seed) and its (score, align_end, best) under GENTLE at min_score = 1, computed once."""
    def make():
        s = tile_set(N, M, seed)
        return s + outputs_ref(*s, *GENTLE, min_score=1)
    return cached(('tile', N, M, seed), make)
