"""Copy detection: did the generator copy its training data? For every generated piece, the longest run of consecutive notes that also
occurs in some corpus piece, how much of the piece such runs cover, and which corpus piece is nearest.

A note after the first of a piece becomes one 32-bit key: its pitch (or, with transpose=True, the interval to the note before), its
position in the bar and the bar step from the note before. Instrument, duration, velocity, time signature and tempo are NOT part of a
key: the identity tested is "the same pitches at the same places in the bar". Two pieces share a run of r keys where r + 1 consecutive
notes of one equal r + 1 consecutive notes of the other in that sense.

The keys (pb_piece_keys) and the N x M x K_a x K_b cell comparisons (pb_shared_runs) run in pb_runs.hip; the host turns run ends into
coverage and summarises. A copy with edits (a changed pitch, an added or a dropped note) breaks an exact run; local_alignments
(pb_local_align, pb_align.hip) aligns the same keys with penalties for mismatches and gaps and finds it whole. There is
no CPU path. The set metrics (pianobart_amd.metrics) cannot see copying: a set of verbatim training
pieces is distributed exactly like the data."""
from collections import OrderedDict

import numpy as np
import torch

from . import ops, pieces
from ._lib import PBError

STAGES = ('keys', 'runs')
ALIGN_DEFAULTS = OrderedDict([('match', 1), ('mismatch', 2), ('gap', 2), ('min_score', 8)])


def piece_keys(ids, e2w=None, start=None, transpose=False, device=None):
    """(keys, klen): the (N, S) int32 device tensor of uint32 keys and the (N) int32 key counts of (N, S, 8) ids (integer or
    integer-valued float arrays or device tensors; every id is checked against its head's size as the set metrics check it), S <= 4096.
    start: the first row that counts, one number or one per piece. transpose: interval keys, which a transposed copy keeps."""
    return ops.piece_keys(mode=int(bool(transpose)), **pieces.upload(ids, pieces.tables(e2w), start, device, max_S=ops.RUNS_MAX_S))


def shared_runs(keys_a, klen_a, keys_b, klen_b, min_run=8, exclude_self=False, chunk=4096, want_matrix=False):
    """(R, run_end, best) of pb_shared_runs for device key rows, the corpus side fed in chunks of `chunk` pieces (one call with
    exclude_self, which compares a set with itself). R is None without want_matrix."""
    if int(min_run) < 1 or int(chunk) < 1:
        raise PBError('novelty: min_run = %r and chunk = %r must be >= 1' % (min_run, chunk))
    N, M = keys_a.shape[0], keys_b.shape[0]
    if exclude_self and N != M:
        raise PBError('novelty: exclude_self compares a set with itself (got %d and %d pieces)' % (N, M))
    step = max(M, 1) if exclude_self else int(chunk)
    run_end = best = None
    Rs = []
    for j0 in range(0, max(M, 1), step):
        R, run_end, best = ops.shared_runs(keys_a, klen_a, keys_b[j0:j0 + step], klen_b[j0:j0 + step], min_run=min_run, exclude_self=exclude_self,
                                           j_base=j0, want_matrix=want_matrix, run_end=run_end, best=best)
        Rs.append(R)
    return (torch.cat(Rs, dim=1) if want_matrix else None), run_end, best


def coverage(run_end, klen):
    """Host: coverage[i] = the share of piece i's keys that lie inside a shared run: key p is covered if some e >= p has
    run_end[i, e] >= e - p + 1. nan for a piece without keys."""
    re = run_end.detach().cpu().numpy() if torch.is_tensor(run_end) else np.asarray(run_end)
    kl = klen.detach().cpu().numpy() if torch.is_tensor(klen) else np.asarray(klen)
    if re.ndim != 2 or kl.shape != (re.shape[0],):
        raise PBError('coverage: run_end (N, S) and klen (N) (got %s and %s)' % (re.shape, kl.shape))
    out = np.full(re.shape[0], np.nan)
    for i, K in enumerate(np.minimum(kl, re.shape[1])):
        if K < 1:
            continue
        row = re[i, :K].astype(np.int64)
        e = np.nonzero(row)[0]
        diff = np.zeros(K + 1, dtype=np.int64)                      # run e covers the keys e - run + 1 .. e
        np.add.at(diff, np.maximum(e - row[e] + 1, 0), 1)
        np.add.at(diff, e + 1, -1)
        out[i] = float((np.cumsum(diff[:K]) > 0).sum()) / K
    return out


def local_alignments(keys_a, klen_a, keys_b, klen_b, match=1, mismatch=2, gap=2, min_score=8, exclude_self=False, chunk=4096, want_matrix=False):
    """(score, align_end, best) of pb_local_align for device key rows, the corpus side fed in chunks of `chunk` pieces (one call with
    exclude_self). score is None without want_matrix. Penalties are positive numbers: match 1 .. 8, mismatch and gap 1 .. 16."""
    match, mismatch, gap, min_score = ops.align_params(match, mismatch, gap, min_score, who='novelty')
    if int(chunk) < 1:
        raise PBError('novelty: chunk = %r must be >= 1' % (chunk,))
    N, M = keys_a.shape[0], keys_b.shape[0]
    if exclude_self and N != M:
        raise PBError('novelty: exclude_self compares a set with itself (got %d and %d pieces)' % (N, M))
    step = max(M, 1) if exclude_self else int(chunk)
    align_end = best = None
    scores = []
    for j0 in range(0, max(M, 1), step):
        sc, align_end, best = ops.local_align(keys_a, klen_a, keys_b[j0:j0 + step], klen_b[j0:j0 + step], match, mismatch, gap, min_score,
                                              exclude_self=exclude_self, j_base=j0, want_matrix=want_matrix, align_end=align_end, best=best)
        scores.append(sc)
    return (torch.cat(scores, dim=1) if want_matrix else None), align_end, best


def split_align_end(align_end):
    """(score, start) int64 arrays of an `align_end` tensor: the score of the best alignment that ends at each key and the key it starts
    at (-1 where none ends): the aligned region covers the keys start .. p."""
    v = (align_end.detach().cpu().numpy() if torch.is_tensor(align_end) else np.asarray(align_end)).astype(np.int64)
    return v >> 12, np.where(v != 0, 4095 - (v & 4095), -1)


def align_coverage(align_end, klen):
    """Host: align_coverage[i] = the share of piece i's keys that lie inside an aligned region: key p is covered if some e >= p has a
    non-zero align_end[i, e] whose start is <= p. The edited keys inside a region count: the region is a copy with edits. nan for a
    piece without keys."""
    ae = align_end.detach().cpu().numpy() if torch.is_tensor(align_end) else np.asarray(align_end)
    kl = klen.detach().cpu().numpy() if torch.is_tensor(klen) else np.asarray(klen)
    if ae.ndim != 2 or kl.shape != (ae.shape[0],):
        raise PBError('align_coverage: align_end (N, S) and klen (N) (got %s and %s)' % (ae.shape, kl.shape))
    _, start = split_align_end(ae)
    out = np.full(ae.shape[0], np.nan)
    for i, K in enumerate(np.minimum(kl, ae.shape[1])):
        if K < 1:
            continue
        e = np.nonzero(ae[i, :K])[0]
        diff = np.zeros(K + 1, dtype=np.int64)                      # the region that ends at e covers the keys start .. e
        np.add.at(diff, np.minimum(start[i, e], e), 1)
        np.add.at(diff, e + 1, -1)
        out[i] = float((np.cumsum(diff[:K]) > 0).sum()) / K
    return out


def split_best(best):
    """(longest, nearest) int64 arrays of a `best` tensor: the run length and the corpus piece that holds it (-1 if none)."""
    b = (best.detach().cpu().numpy() if torch.is_tensor(best) else np.asarray(best)).astype(np.int64)
    longest = b >> 32
    nearest = np.where(b != 0, 0xFFFFFFFF - (b & 0xFFFFFFFF), -1)
    return longest, nearest


def _align_params(align):
    """None, or the four parameters of local_alignments as an ordered dict: True = the defaults, a dict overrides some of them."""
    if align is None or align is False:
        return None
    par = OrderedDict(ALIGN_DEFAULTS)
    if align is not True:
        if not isinstance(align, dict) or set(align) - set(par):
            raise PBError('novelty: align is None, True or a dict with keys of %s (got %r)' % (list(par), align))
        par.update(align)
    return OrderedDict(zip(par, ops.align_params(who='novelty', **par)))


def compare_to_corpus(gen_ids, corpus_ids, e2w=None, start=None, min_run=8, transpose=False, exclude_self=False, chunk=4096, want_matrix=False,
                      align=None):
    """Compare generated pieces with a corpus, both (N, S, 8) ids (S may differ). Per generated piece: `keys` (its key count), `longest`
    (the longest run of keys shared with any corpus piece; r keys = r + 1 notes), `nearest` (the first corpus piece that holds it, -1 if
    none) and `coverage` (the share of its keys inside shared runs of at least min_run keys). Set lines: longest_mean / _median / _max,
    coverage_mean (over pieces with keys), share_half_covered (coverage >= 0.5), share_with_run (longest >= min_run), device_ms per
    stage. exclude_self: compare gen_ids with itself, a piece never with itself (corpus_ids is ignored): the diversity of one set.
    start: one value or a (gen, corpus) pair. want_matrix: add `matrix`, the (N, M) longest runs.
    align: None leaves everything above as it is. True (match 1, mismatch 2, gap 2, min_score 8) or a dict of some of these four adds
    the local alignment of the same keys, which finds a copy with edits whole: `align_params`, per piece `align_score`
    (the best alignment with any corpus piece), `align_nearest` (the first corpus piece that holds it, -1 if none), `align_coverage`
    (the share of its keys inside aligned regions of at least min_score, edited keys included) and `align_span` (the keys of the longest
    such region); set lines align_score_mean / _median / _max, align_coverage_mean, share_half_aligned, share_with_alignment
    (align_score >= min_score); device_ms['align']; with want_matrix `align_matrix`, the (N, M) scores."""
    tab = pieces.tables(e2w)
    par = _align_params(align)
    s_gen, s_cor = start if isinstance(start, tuple) else (start, start)
    for ids in (gen_ids, corpus_ids):
        if torch.is_tensor(ids):
            ops._p(ids)                               # a host tensor is refused before the first device call
    timer = pieces.Timer(STAGES + (('align',) if par is not None else ()))
    ka, la = timer.run('keys', piece_keys, gen_ids, tab, s_gen, transpose)
    kb, lb = (ka, la) if exclude_self else timer.run('keys', piece_keys, corpus_ids, tab, s_cor, transpose, ka.device)
    R, run_end, best = timer.run('runs', shared_runs, ka, la, kb, lb, min_run, exclude_self, chunk, want_matrix)
    if par is not None:
        al_score, al_end, al_best = timer.run('align', local_alignments, ka, la, kb, lb, par['match'], par['mismatch'], par['gap'], par['min_score'],
                                              exclude_self, chunk, want_matrix)
    ms = timer.totals()
    klen = la.cpu().numpy().astype(np.int64)
    longest, nearest = split_best(best)
    cov = coverage(run_end, klen)
    has = klen > 0
    n = len(klen)
    share = lambda mask: float(mask.sum()) / n if n else float('nan')
    res = OrderedDict([('n_gen', n), ('n_corpus', int(kb.shape[0])), ('min_run', int(min_run)), ('transpose', bool(transpose)),
                       ('exclude_self', bool(exclude_self)),
                       ('keys', klen), ('longest', longest), ('nearest', nearest), ('coverage', cov),
                       ('longest_mean', float(longest.mean()) if n else float('nan')),
                       ('longest_median', float(np.median(longest)) if n else float('nan')),
                       ('longest_max', int(longest.max()) if n else 0),
                       ('coverage_mean', float(cov[has].mean()) if has.any() else float('nan')),
                       ('share_half_covered', share(has & (np.nan_to_num(cov) >= 0.5))),
                       ('share_with_run', share(longest >= int(min_run))),
                       ('device_ms', ms)])
    if want_matrix:
        res['matrix'] = R.cpu().numpy()
    if par is not None:
        a_score, a_nearest = split_best(al_best)
        a_cov = align_coverage(al_end, klen)
        end_score, end_start = split_align_end(al_end)
        span = np.where(end_score > 0, np.arange(end_score.shape[1])[None, :] - end_start + 1, 0)
        res.update([('align_params', par), ('align_score', a_score), ('align_nearest', a_nearest), ('align_coverage', a_cov),
                    ('align_span', span.max(axis=1) if n else np.zeros(0, dtype=np.int64)),
                    ('align_score_mean', float(a_score.mean()) if n else float('nan')),
                    ('align_score_median', float(np.median(a_score)) if n else float('nan')),
                    ('align_score_max', int(a_score.max()) if n else 0),
                    ('align_coverage_mean', float(a_cov[has].mean()) if has.any() else float('nan')),
                    ('share_half_aligned', share(has & (np.nan_to_num(a_cov) >= 0.5))),
                    ('share_with_alignment', share(a_score >= par['min_score']))])
        if want_matrix:
            res['align_matrix'] = al_score.cpu().numpy()
    return res
