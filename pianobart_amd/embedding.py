"""Embedding-space set metrics: does a generated set look like the data to the trained encoder?

A piece becomes one vector, the mean of the encoder's last hidden rows over its notes (pb_pool_rows behind PianoBart.embed). Two sets of
such vectors are compared by
  * a Frechet distance between the Gaussians of their float64 moments (pb_embed_moments; the form of FID, FAD and the Frechet Music
    Distance: |m1 - m2|^2 + tr(S1 + S2 - 2 (S1 S2)^1/2)), and
  * precision, recall, density and coverage (Naeem et al., "Reliable Fidelity and Diversity Metrics for Generative Models", 2020) over the
    k-nearest-neighbour balls of both sets (pb_sqdist, pb_knn_radius, pb_ball_counts).
The embeddings also serve retrieval: ops.sqdist of one piece's vector against a corpus'.

This is NOT the reference's "FAD" / "FAD(BAR)" of finetune_generation, which compares shapes of token curves through the third-party
`shapesimilarity`; those lines stay n/a. The embedder is the model's own encoder and nothing else.

EmbeddingMixin is the embedding part of pianobart_amd.engine.Engine, beside scoring.ScoringMixin; nothing here imports engine.py.

Bar ids are NOT rebased: a piece cut at `start` keeps the bar numbers it had, as the generator's prime does."""
from collections import OrderedDict

import numpy as np
import torch

from . import ops, pieces
from ._lib import PBError

STAGES = ('encode', 'pool', 'moments', 'distances', 'knn', 'counts')
D2_BLOCK_BYTES = 64 << 20                     # a block of squared distances on the device stays under this


def _run(timer, stage, fn, *args, **kw):
    return fn(*args, **kw) if timer is None else timer.run(stage, fn, *args, **kw)


# ---- one vector per piece ------------------------------------------------------------------------------------------------------------------
class EmbeddingMixin:
    def embed(self, enc16, emask, timer=None):
        """(emb (B, d) f32, count (B) int32) of enc16 (B, S, 8) int16 device ids and emask (B, S) or None: one encoder-only forward
        without dropout and without an autograd graph, then the mean of the last hidden state over the rows whose mask is not 0.
        Raises IndexError for an id outside its embedding table. timer (pieces.Timer): the stages 'encode' and 'pool'."""
        if enc16.device.type != 'cuda':
            raise PBError('pianobart_amd needs HIP device tensors (got %s); there is no CPU path' % enc16.device)
        B, S = int(enc16.shape[0]), int(enc16.shape[1])
        if emask is not None and tuple(emask.shape) != (B, S):
            raise PBError('embed: encoder_attention_mask of shape %s for ids of (%d, %d, 8)' % (tuple(emask.shape), B, S))
        self.bind(enc16.device)
        self._await_updates(2)
        with torch.no_grad():
            enc16 = self.note_ids(enc16.contiguous(), owned=False)
            em = emask.to(torch.float32).contiguous() if emask is not None else None
            _, enc_h = _run(timer, 'encode', self.forward_hidden, enc16, None, em, None, False, 0)
            emb, count = _run(timer, 'pool', ops.pool_rows, enc_h.view(B, S, self.d), em)
        self.check_ids(collective=False)          # a rank may embed by itself: local verdict (synchronises; an offending id was read as 0)
        return emb, count


def _backbone(model):
    pb = getattr(model, 'pianobart', model)
    if not hasattr(pb, 'embed') or not hasattr(pb, 'layout'):
        raise PBError('embedding: the model must be a PianoBart or a model that holds one as .pianobart (got %s)' % type(model).__name__)
    return pb


def arrange(ids, layout, pad_word, start=None):
    """Host: what the encoder sees of a set. ids (N, S, 8) integers -> (rows (n, S, 8) int64, lengths (n) int64, empty): of every piece with a
    live row (pieces.live_rows: the rows start .. L - 1) those rows moved to the front and every other row set to pad_word (8 ids); pieces
    without one are left out and counted in empty."""
    a = pieces.host_ids(ids, layout)
    live = pieces.live_rows(a, layout, start)[1]
    order = np.argsort(~live, axis=1, kind='stable')
    moved = np.take_along_axis(a, order[:, :, None], 1)
    n_live = live.sum(1)
    moved[np.arange(a.shape[1])[None, :] >= n_live[:, None]] = np.asarray(pad_word, dtype=np.int64)
    keep = n_live > 0
    return moved[keep], n_live[keep].astype(np.int64), int((~keep).sum())


def _embed_rows(pb, rows, batch_size, timer=None):
    """emb (n, d) f32 on the model's device of arranged rows (n, S, 8): PianoBart.embed in batches, encoder mask bar != Bar <PAD>."""
    if isinstance(batch_size, bool) or not isinstance(batch_size, (int, np.integer)) or batch_size < 1:
        raise PBError('embedding: batch_size = %r must be an integer >= 1' % (batch_size,))
    S = rows.shape[1]
    if S > pb.bartConfig.max_position_embeddings:
        raise PBError('embedding: pieces of %d rows exceed max_position_embeddings %d' % (S, pb.bartConfig.max_position_embeddings))
    dev = next(pb.parameters()).device
    if dev.type != 'cuda':
        raise PBError('pianobart_amd needs the model on a HIP device (it is on %s); there is no CPU path' % dev)
    eng = pb._get_engine()
    out = torch.empty((rows.shape[0], pb.hidden_size), dtype=torch.float32, device=dev)
    for b0 in range(0, rows.shape[0], int(batch_size)):
        x = torch.from_numpy(rows[b0:b0 + int(batch_size)]).to(dev)
        mask = (x[:, :, 0] != int(pb.bar_pad_word)).to(torch.float32)
        emb, count = eng.embed(ops.ids_to_i16(x), mask, timer)
        bad = torch.nonzero(count == 0).flatten().tolist()
        if bad:
            raise PBError('embedding: piece %d of the non-empty pieces has no visible position' % (b0 + bad[0]))
        out[b0:b0 + emb.shape[0]] = emb
    return out


def embed_set(model, ids, start=None, batch_size=16, timer=None):
    """(emb (n, d) f32 device tensor, empty) of a set of pieces ids (N, S, 8): arrange() then PianoBart.embed in batches with the encoder
    mask bar != Bar <PAD>. Bar ids are not rebased. empty: the pieces without a live row, which have no vector."""
    pb = _backbone(model)
    rows, _, empty = arrange(ids, pb.layout, pb.pad_word_np, start)
    return _embed_rows(pb, rows, batch_size, timer), empty


# ---- Frechet distance ----------------------------------------------------------------------------------------------------------------------
def set_moments(emb, timer=None):
    """(mean (d), cov (d, d)) float64 host arrays of emb (n, d) f32 on the device, n >= 2: pb_embed_moments, the scatter matrix divided by
    n - 1 on the host. cov is symmetric bit for bit."""
    mean, C = _run(timer, 'moments', ops.embed_moments, emb)
    return mean.cpu().numpy(), C.cpu().numpy() / float(emb.shape[0] - 1)


def frechet_terms(mean1, cov1, mean2, cov2):
    """(|m1 - m2|^2, tr S1 + tr S2 - 2 t) in float64 numpy, t = tr (S1 S2)^1/2 as the sum of the square roots of the eigenvalues of
    R S2 R with R = S1^1/2 from an eigendecomposition, every eigenvalue clamped at 0. Nothing else is clamped."""
    m1, m2 = np.asarray(mean1, dtype=np.float64), np.asarray(mean2, dtype=np.float64)
    s1, s2 = np.asarray(cov1, dtype=np.float64), np.asarray(cov2, dtype=np.float64)
    d = m1.shape[0] if m1.ndim == 1 else -1
    if m1.ndim != 1 or m2.shape != (d,) or s1.shape != (d, d) or s2.shape != (d, d):
        raise PBError('frechet_distance: means of %s and %s, covariances of %s and %s: expected (d), (d), (d, d), (d, d)'
                      % (m1.shape, m2.shape, s1.shape, s2.shape))
    w, V = np.linalg.eigh(s1)
    R = (V * np.sqrt(np.maximum(w, 0.0))) @ V.T
    M = R @ s2 @ R
    M = 0.5 * (M + M.T)
    t = float(np.sqrt(np.maximum(np.linalg.eigvalsh(M), 0.0)).sum())
    diff = m1 - m2
    return float(diff @ diff), float(np.trace(s1) + np.trace(s2) - 2.0 * t)


def frechet_distance(mean1, cov1, mean2, cov2):
    """|m1 - m2|^2 + tr S1 + tr S2 - 2 tr (S1 S2)^1/2 (frechet_terms), as computed: a value slightly below 0 is not clamped."""
    mean_term, trace_term = frechet_terms(mean1, cov1, mean2, cov2)
    return mean_term + trace_term


# ---- precision, recall, density, coverage ------------------------------------------------------------------------------------------------------
def _block_rows(n, cols, block_bytes):
    return max(1, min(n, int(block_bytes) // (4 * cols)))


def knn_radii(emb, k, block_bytes=D2_BLOCK_BYTES, timer=None):
    """rad (n) f32 on the device: the squared distance of every row of emb (n, d) to its k-th nearest other row, in row blocks."""
    n = emb.shape[0]
    rb = _block_rows(n, n, block_bytes)
    buf = torch.empty((rb, n), dtype=torch.float32, device=emb.device)
    rad = torch.empty(n, dtype=torch.float32, device=emb.device)
    for r0 in range(0, n, rb):
        m = min(rb, n - r0)
        D2 = _run(timer, 'distances', ops.sqdist, emb[r0:r0 + m], emb, buf[:m])
        rad[r0:r0 + m] = _run(timer, 'knn', ops.knn_radius, D2, k, r0)
    return rad


def ball_hits(emb_gen, emb_ref, rad_gen, rad_ref, block_bytes=D2_BLOCK_BYTES, timer=None):
    """(row_hits (n_gen), col_hits (n_ref), col_hits_gen (n_ref)) int32 on the device (pb_ball_counts), the generated rows fed in blocks."""
    n, M = emb_gen.shape[0], emb_ref.shape[0]
    rb = _block_rows(n, M, block_bytes)
    buf = torch.empty((rb, M), dtype=torch.float32, device=emb_gen.device)
    row_hits = torch.zeros(n, dtype=torch.int32, device=emb_gen.device)
    col_hits = torch.zeros(M, dtype=torch.int32, device=emb_gen.device)
    col_hits_gen = torch.zeros(M, dtype=torch.int32, device=emb_gen.device)
    for r0 in range(0, n, rb):
        m = min(rb, n - r0)
        D2 = _run(timer, 'distances', ops.sqdist, emb_gen[r0:r0 + m], emb_ref, buf[:m])
        _run(timer, 'counts', ops.ball_counts, D2, rad_ref, rad_gen[r0:r0 + m], row_hits[r0:r0 + m], col_hits, col_hits_gen)
    return row_hits, col_hits, col_hits_gen


def check_counts(n_gen, n_ref, k):
    """A set needs 2 pieces with a vector, and k-th neighbours need 1 <= k < min(n_gen, n_ref), k <= 64."""
    for name, n in (('generated', n_gen), ('reference', n_ref)):
        if n < 2:
            raise PBError('embedding: the %s set holds %d non-empty pieces; a set needs at least 2 (its covariance and its neighbours)' % (name, n))
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= ops.KNN_MAX_K or k >= min(n_gen, n_ref):
        raise PBError('embedding: k = %r; it takes 1 <= k <= %d and k < min(n_gen, n_ref) = %d' % (k, ops.KNN_MAX_K, min(n_gen, n_ref)))


def check_sets(emb_gen, emb_ref, k):
    """The refusals of a pair of embedding sets, on their shapes alone: 2-D, equal widths, at least 2 rows each, 1 <= k < min(n_gen, n_ref)
    and k <= 64. Returns (n_gen, n_ref, d)."""
    for name, e in (('generated', emb_gen), ('reference', emb_ref)):
        if len(e.shape) != 2 or e.shape[1] < 1:
            raise PBError('embedding: the %s embeddings have the shape %s; expected (n, d)' % (name, tuple(e.shape)))
    if emb_gen.shape[1] != emb_ref.shape[1]:
        raise PBError('embedding: embedding widths differ: generated d = %d, reference d = %d' % (emb_gen.shape[1], emb_ref.shape[1]))
    n_gen, n_ref = int(emb_gen.shape[0]), int(emb_ref.shape[0])
    check_counts(n_gen, n_ref, k)
    return n_gen, n_ref, int(emb_gen.shape[1])


def _device_f32(e):
    if torch.is_tensor(e):
        ops._p(e)                                     # a host tensor is refused as every op refuses it
        return e.to(torch.float32).contiguous()
    a = np.asarray(e)
    if a.dtype.kind != 'f':
        raise PBError('embedding: embeddings must be floating-point (got %s)' % a.dtype)
    if not torch.cuda.is_available():
        raise PBError('pianobart_amd has no CPU execution path: the set kernels need an MI355X')
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.device('cuda', torch.cuda.current_device()))


def prdc(emb_gen, emb_ref, k=5, block_bytes=D2_BLOCK_BYTES, timer=None):
    """OrderedDict(precision, recall, density, coverage) of two embedding sets ((n, d) device f32 tensors or host arrays), k-nearest-neighbour
    balls with a strict <: precision = the share of generated rows inside a reference ball, density = the balls a generated row lies in /
    k on average, coverage = the share of reference rows with a generated row inside their ball, recall = the share of reference rows
    inside a generated ball. The counts are integers: the four numbers are exact by definition."""
    n_gen, n_ref, _ = check_sets(emb_gen, emb_ref, k)
    g, r = _device_f32(emb_gen), _device_f32(emb_ref)
    rad_ref = knn_radii(r, int(k), block_bytes, timer)
    rad_gen = knn_radii(g, int(k), block_bytes, timer)
    row_hits, col_hits, col_hits_gen = (t.cpu().numpy().astype(np.int64) for t in ball_hits(g, r, rad_gen, rad_ref, block_bytes, timer))
    return OrderedDict(precision=int((row_hits > 0).sum()) / n_gen, recall=int((col_hits_gen > 0).sum()) / n_ref,
                       density=int(row_hits.sum()) / (int(k) * n_gen), coverage=int((col_hits > 0).sum()) / n_ref)


# ---- the comparison --------------------------------------------------------------------------------------------------------------------------
def compare_embedded(emb_gen, emb_ref, k=5, empty_gen=0, empty_ref=0, precision_mode=None, timer=None):
    """compare_embeddings for two ready (n, d) embedding sets (device tensors or host arrays) and no model."""
    n_gen, n_ref, d = check_sets(emb_gen, emb_ref, k)
    g, r = _device_f32(emb_gen), _device_f32(emb_ref)
    timer = timer or pieces.Timer(STAGES)
    m1, s1 = set_moments(g, timer)
    m2, s2 = set_moments(r, timer)
    mean_term, trace_term = frechet_terms(m1, s1, m2, s2)
    res = OrderedDict(n_gen=n_gen, n_ref=n_ref, empty_gen=int(empty_gen), empty_ref=int(empty_ref), d=d, precision_mode=precision_mode, k=int(k),
                      fmd=mean_term + trace_term, mean_term=mean_term, trace_term=trace_term, rank_deficient=bool(min(n_gen, n_ref) - 1 < d))
    res.update(prdc(g, r, int(k), timer=timer))
    res['device_ms'] = timer.totals()
    return res


def compare_embeddings(model, gen_ids, ref_ids, k=5, start=None, batch_size=16):
    """A generated set against a reference set in the embedding space of `model` (a PianoBart or PianoBartLM on the device). gen_ids,
    ref_ids: (N, S, 8) integers; start: the first rows of every piece that do not count (one row index or one per piece, for both sets
    alike when it is one number). Returns an OrderedDict: n_gen, n_ref (pieces with a vector), empty_gen, empty_ref, d, precision_mode,
    k, fmd = mean_term + trace_term, rank_deficient (min(n_gen, n_ref) - 1 < d: a covariance cannot have full rank, and fmd then says
    little), precision, recall, density, coverage, and device_ms per stage."""
    pb = _backbone(model)
    rows_g, _, empty_gen = arrange(gen_ids, pb.layout, pb.pad_word_np, start)
    rows_r, _, empty_ref = arrange(ref_ids, pb.layout, pb.pad_word_np, start)
    check_counts(rows_g.shape[0], rows_r.shape[0], k)                 # before any device work
    timer = pieces.Timer(STAGES)
    g, r = _embed_rows(pb, rows_g, batch_size, timer), _embed_rows(pb, rows_r, batch_size, timer)
    return compare_embedded(g, r, k, empty_gen, empty_ref, pb.precision, timer)
