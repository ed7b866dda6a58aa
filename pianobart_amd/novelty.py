"""Copy detection: did the generator copy its training data? For every generated piece, the longest run of consecutive notes that also
occurs in some corpus piece, how much of the piece such runs cover, and which corpus piece is nearest.

A note after the first of a piece becomes one 32-bit key: its pitch (or, with transpose=True, the interval to the note before), its
position in the bar and the bar step from the note before. Instrument, duration, velocity, time signature and tempo are NOT part of a
key: the identity tested is "the same pitches at the same places in the bar". Two pieces share a run of r keys where r + 1 consecutive
notes of one equal r + 1 consecutive notes of the other in that sense.

The keys (pb_piece_keys) and the N x M x K_a x K_b cell comparisons (pb_shared_runs) run in pb_runs.hip; the host turns run ends into
coverage and summarises. There is no CPU path. The set metrics (pianobart_amd.metrics) cannot see copying: a set of verbatim training
pieces is distributed exactly like the data."""
from collections import OrderedDict

import numpy as np
import torch

from . import metrics, ops
from ._lib import PBError

STAGES = ('keys', 'runs')


def _tables(e2w):
    return e2w if isinstance(e2w, metrics.Tables) else metrics.tables(e2w)


def piece_keys(ids, e2w=None, start=None, transpose=False, device=None):
    """(keys, klen): the (N, S) int32 device tensor of uint32 keys and the (N) int32 key counts of (N, S, 8) ids (integer or
    integer-valued float arrays or device tensors; every id is checked against its head's size as the set metrics check it), S <= 4096.
    start: the first row that counts, one number or one per piece. transpose: interval keys, which a transposed copy keeps."""
    tab = _tables(e2w)
    a = metrics._host_ids(ids, tab.layout)
    if a.shape[1] > ops.RUNS_MAX_S:
        raise PBError('novelty: pieces of %d rows; the kernels take 1 .. %d' % (a.shape[1], ops.RUNS_MAX_S))
    dev = torch.device(device) if device is not None else ids.device if torch.is_tensor(ids) else torch.device('cuda', torch.cuda.current_device())
    s = metrics._host_start(start, a.shape[0])
    up = lambda x: torch.from_numpy(x).to(dev)
    return ops.piece_keys(up(a.astype(np.int16)), up(tab.pitch_of), start=None if s is None else up(s), layout=tab.layout, mode=int(bool(transpose)))


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


def split_best(best):
    """(longest, nearest) int64 arrays of a `best` tensor: the run length and the corpus piece that holds it (-1 if none)."""
    b = (best.detach().cpu().numpy() if torch.is_tensor(best) else np.asarray(best)).astype(np.int64)
    longest = b >> 32
    nearest = np.where(b != 0, 0xFFFFFFFF - (b & 0xFFFFFFFF), -1)
    return longest, nearest


class _Timer(metrics._Timer):
    def totals(self):
        torch.cuda.synchronize()
        ms = OrderedDict((stage, 0.0) for stage in STAGES)
        for stage, a, b in self.pairs:
            ms[stage] += a.elapsed_time(b)
        ms['total'] = sum(ms.values())
        return ms


def compare_to_corpus(gen_ids, corpus_ids, e2w=None, start=None, min_run=8, transpose=False, exclude_self=False, chunk=4096, want_matrix=False):
    """Compare generated pieces with a corpus, both (N, S, 8) ids (S may differ). Per generated piece: `keys` (its key count), `longest`
    (the longest run of keys shared with any corpus piece; r keys = r + 1 notes), `nearest` (the first corpus piece that holds it, -1 if
    none) and `coverage` (the share of its keys inside shared runs of at least min_run keys). Set lines: longest_mean / _median / _max,
    coverage_mean (over pieces with keys), share_half_covered (coverage >= 0.5), share_with_run (longest >= min_run), device_ms per
    stage. exclude_self: compare gen_ids with itself, a piece never with itself (corpus_ids is ignored): the diversity of one set.
    start: one value or a (gen, corpus) pair. want_matrix: add `matrix`, the (N, M) longest runs."""
    tab = _tables(e2w)
    s_gen, s_cor = start if isinstance(start, tuple) else (start, start)
    for ids in (gen_ids, corpus_ids):
        if torch.is_tensor(ids):
            ops._p(ids)                               # a host tensor is refused before the first device call
    timer = _Timer()
    ka, la = timer.run('keys', piece_keys, gen_ids, tab, s_gen, transpose)
    kb, lb = (ka, la) if exclude_self else timer.run('keys', piece_keys, corpus_ids, tab, s_cor, transpose, ka.device)
    R, run_end, best = timer.run('runs', shared_runs, ka, la, kb, lb, min_run, exclude_self, chunk, want_matrix)
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
    return res
