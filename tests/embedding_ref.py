"""float64 / int64 numpy restatement of csrc/pb_embed.hip and of pianobart_amd.embedding: the reference of tests/test_embedding_gpu.py and
tests/test_embedding_cpu.py. Every function takes what the kernel takes (float32 values are read as float64) and states the result in the
plainest form; nothing here is shared with the code under test."""
import math

import numpy as np


def pool_rows(H, mask=None):
    """(out (B, d) float32, count (B) int64): float32(float64 sum over the rows with mask != 0 / count); a zero row where count is 0."""
    H = np.asarray(H, dtype=np.float64)
    B, S, d = H.shape
    m = np.ones((B, S), dtype=bool) if mask is None else (np.asarray(mask) != 0)
    out = np.zeros((B, d), dtype=np.float32)
    count = m.sum(1).astype(np.int64)
    for b in range(B):
        if count[b]:
            out[b] = H[b, m[b]].sum(0) / float(count[b])
    return out, count


def pool_rows_f64(H, mask=None):
    """The same mean without the last rounding, and the mean of |h| over the pooled rows (the tests' error scale)."""
    H = np.asarray(H, dtype=np.float64)
    B, S, d = H.shape
    m = np.ones((B, S), dtype=bool) if mask is None else (np.asarray(mask) != 0)
    ref, mag = np.zeros((B, d)), np.zeros((B, d))
    for b in range(B):
        if m[b].any():
            ref[b] = H[b, m[b]].sum(0) / m[b].sum()
            mag[b] = np.abs(H[b, m[b]]).sum(0) / m[b].sum()
    return ref, mag


def moments(X):
    """(mean (d), C (d, d)) float64: C = sum_n (x_n - mean)(x_n - mean)^T, two-pass."""
    X = np.asarray(X, dtype=np.float64)
    mean = X.sum(0) / X.shape[0]
    c = X - mean
    return mean, c.T @ c


def sqdist(A, B):
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    out = np.empty((A.shape[0], B.shape[0]))
    for i in range(A.shape[0]):
        out[i] = ((A[i][None, :] - B) ** 2).sum(-1)
    return out


def knn_radius(D2, k, r0=0):
    """The k-th smallest of every row of the (n, N) block with the entry of its own piece (column r0 + i) removed: numpy.sort."""
    D2 = np.asarray(D2)
    out = np.empty(D2.shape[0], dtype=D2.dtype)
    for i in range(D2.shape[0]):
        out[i] = np.sort(np.delete(D2[i], r0 + i))[k - 1]
    return out


def ball_counts(D2, rad_ref, rad_gen, strict=True):
    """(row_hits (n), col_hits (M), col_hits_gen (M)) int64 of a block D2 (n, M); strict: < (the definition), else <= (to show a case tells them apart)."""
    D2, rad_ref, rad_gen = np.asarray(D2), np.asarray(rad_ref), np.asarray(rad_gen)
    in_ref = D2 < rad_ref[None, :] if strict else D2 <= rad_ref[None, :]
    in_gen = D2 < rad_gen[:, None] if strict else D2 <= rad_gen[:, None]
    return in_ref.sum(1).astype(np.int64), in_ref.sum(0).astype(np.int64), in_gen.sum(0).astype(np.int64)


def prdc_from_d2(d2_gen, d2_ref, d2_inter, k, strict=True):
    """precision, recall, density, coverage from the three squared-distance matrices (gen x gen, ref x ref, gen x ref)."""
    rad_gen, rad_ref = knn_radius(d2_gen, k), knn_radius(d2_ref, k)
    row_hits, col_hits, col_hits_gen = ball_counts(d2_inter, rad_ref, rad_gen, strict)
    n_gen, n_ref = d2_inter.shape
    return dict(precision=int((row_hits > 0).sum()) / n_gen, recall=int((col_hits_gen > 0).sum()) / n_ref,
                density=int(row_hits.sum()) / (k * n_gen), coverage=int((col_hits > 0).sum()) / n_ref)


def frechet_svd(A, B):
    """The Frechet distance of the Gaussians of two sets of rows by the nuclear-norm form: with A_c, B_c the centred sets over sqrt(n - 1),
    tr (S1 S2)^1/2 = the sum of the singular values of A_c B_c^T. No covariance matrix is formed for the cross term."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    ma, mb = A.mean(0), B.mean(0)
    Ac, Bc = (A - ma) / math.sqrt(A.shape[0] - 1), (B - mb) / math.sqrt(B.shape[0] - 1)
    t = np.linalg.svd(Ac @ Bc.T, compute_uv=False).sum()
    return float(((ma - mb) ** 2).sum() + (Ac ** 2).sum() + (Bc ** 2).sum() - 2.0 * t)


def cross_norm(A, B):
    """||S1^1/2 S2 S1^1/2||_2 = the largest singular value of A_c B_c^T, squared."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    Ac, Bc = (A - A.mean(0)) / math.sqrt(A.shape[0] - 1), (B - B.mean(0)) / math.sqrt(B.shape[0] - 1)
    return float(np.linalg.svd(Ac @ Bc.T, compute_uv=False)[0] ** 2)


def rank_deficient_bound(A, B):
    """2 d sqrt(d 2^-52 ||M||_2): what the square roots of d eigenvalues of M = S1^1/2 S2 S1^1/2, each known to d eps ||M||_2, can lose."""
    d = np.asarray(A).shape[1]
    return 2.0 * d * math.sqrt(d * 2.0 ** -52 * cross_norm(A, B))


def cov(A):
    A = np.asarray(A, dtype=np.float64)
    c = A - A.mean(0)
    return A.mean(0), c.T @ c / (A.shape[0] - 1)


def lattice(n, d, seed):
    """(n, d) float32 points with small integer coordinates: distances tie often, so < and <= give different counts."""
    rng = np.random.default_rng(seed)
    span = 3 if d > 1 else max(4, n // 2)
    return rng.integers(-span, span + 1, size=(n, d)).astype(np.float32)


def arrange(ids, pad8, pad_row, start=0):
    """The host restatement of embedding.arrange: per piece L = its first row with an id >= its head's PAD, the rows start .. L - 1 moved to the
    front, the rest pad_row; pieces without such a row dropped. Returns (rows (n, S, 8), lengths, empty)."""
    ids = np.asarray(ids, dtype=np.int64)
    rows, lens, empty = [], [], 0
    for piece in ids:
        L = piece.shape[0]
        for r in range(piece.shape[0]):
            if any(piece[r, h] >= pad8[h] for h in range(8)):
                L = r
                break
        live = piece[start:L]
        if len(live) == 0:
            empty += 1
            continue
        out = np.tile(np.asarray(pad_row, dtype=np.int64), (piece.shape[0], 1))
        out[:len(live)] = live
        rows.append(out)
        lens.append(len(live))
    return np.array(rows, dtype=np.int64).reshape(-1, ids.shape[1], 8), np.array(lens, dtype=np.int64), empty
