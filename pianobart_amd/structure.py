"""Repetition structure of generated pieces: does a PIECE hold together? Per piece, how much of a bar returns 1 .. 64 bars later: the
onsets of the bar (the groove profile) and its notes, onset and pitch (the repetition profile), as pooled Dice similarities of the bar
pairs a lag apart. The definition is this project's own, in the family of the grooving-pattern similarity of Wu & Yang's
"Jazz Transformer" evaluation (MusDr) and of self-similarity lag profiles; it is neither of them number for number.

The lag sums (pb_piece_structure) run in pb_structure.hip, the set comparison in the kernels of pianobart_amd.metrics; the host divides
integer columns. There is no CPU path."""
from collections import OrderedDict
from functools import partial

import numpy as np
import torch

from . import metrics, ops, pieces
from ._lib import PBError
from .pieces import bar_spans

LAGS, COLS = ops.STRUCTURE_LAGS, ops.STRUCTURE_COLS
C_IO, C_TO, C_IN, C_TN = 8, 8 + LAGS, 8 + 2 * LAGS, 8 + 3 * LAGS
GROUPS = ('groove_profile', 'repeat_profile', 'groove_mean', 'repeat_mean', 'repeat_period')
SCALAR_GROUPS = GROUPS[2:]


def _op(pitch_class):
    return partial(ops.piece_structure, mode=int(bool(pitch_class)))


def piece_structure(ids, e2w=None, start=None, device=None, pitch_class=False):
    """The (N, 264) int32 device tensor of pb_piece_structure for (N, S, 8) ids, S <= 4096: integer or integer-valued float arrays or device
    tensors, checked as metrics.piece_features checks them. start: the first row that counts, one number or one per piece. e2w: a
    dictionary, None (the default one) or metrics.tables(). pitch_class: a note is (position, pitch class), percussion stays itself."""
    return _op(pitch_class)(**pieces.upload(ids, pieces.tables(e2w), start, device))


def _columns(cols):
    c = cols.detach().cpu().numpy() if torch.is_tensor(cols) else np.asarray(cols)
    if c.ndim != 2 or c.shape[1] != COLS or c.dtype.kind not in 'iu':
        raise PBError('structure: need an (N, %d) integer array of lag sums (got %s %s)' % (COLS, c.shape, c.dtype))
    return c.astype(np.int64)


def _dice(i, t, zero):
    """2 i / t in float64; `zero` where t == 0."""
    out = np.full(np.broadcast(i, t).shape, zero, dtype=np.float64)
    np.divide(2.0 * i, t, out=out, where=t != 0)
    return out


def lag_profiles(cols):
    """Host, float64: (groove, repeat), each (N, 64): D_O[l] and D_N[l] = 2 I[l] / T[l] of every piece for l = 1 .. 64, nan where T[l] == 0
    (no bar pair that far apart holds a note)."""
    c = _columns(cols)
    nan = float('nan')
    return _dice(c[:, C_IO:C_IO + LAGS], c[:, C_TO:C_TO + LAGS], nan), _dice(c[:, C_IN:C_IN + LAGS], c[:, C_TN:C_TN + LAGS], nan)


def _check_lags(lags):
    if isinstance(lags, bool) or int(lags) != lags or not 1 <= int(lags) <= LAGS:
        raise PBError('structure: lags = %r; 1 .. %d' % (lags, LAGS))
    return int(lags)


def structure_groups(cols, lags=16):
    """(groups, short): the five structure groups of an (N, 264) array of lag sums as float32 arrays over the n pieces that span at least
    two bars (W >= 2); short = the number of pieces left out. Divisions in float64, a zero divisor gives zeros.
      groove_profile, repeat_profile (n, lags)   D_O[l], D_N[l] for l = 1 .. lags
      groove_mean, repeat_mean (n,)              2 sum_l I[l] / sum_l T[l] over the same lags
      repeat_period (n,)                         the lag with the largest D_N, the smallest one on ties, 0 when all are 0"""
    lags = _check_lags(lags)
    c = _columns(cols)
    keep = c[:, 1] >= 2
    short = int((~keep).sum())
    c = c[keep]
    io, to, i_n, tn = (c[:, o:o + lags] for o in (C_IO, C_TO, C_IN, C_TN))
    g = OrderedDict()
    g['groove_profile'] = _dice(io, to, 0.0)
    g['repeat_profile'] = _dice(i_n, tn, 0.0)
    g['groove_mean'] = _dice(io.sum(1), to.sum(1), 0.0)
    g['repeat_mean'] = _dice(i_n.sum(1), tn.sum(1), 0.0)
    d = g['repeat_profile']
    g['repeat_period'] = np.where(d.max(1) > 0, d.argmax(1) + 1, 0).astype(np.float64) if len(d) else np.zeros(0)
    return OrderedDict((k, v.astype(np.float32)) for k, v in g.items()), short


def pooled_profiles(cols):
    """Host: {'groove', 'repeat'}: per lag 1 .. 64 the pooled 2 sum_pieces I[l] / sum_pieces T[l] of a set as lists of floats, nan where no
    piece of the set has a bar pair that far apart."""
    c = _columns(cols)
    nan = float('nan')
    s = c.sum(0)
    return OrderedDict([('groove', _dice(s[C_IO:C_IO + LAGS], s[C_TO:C_TO + LAGS], nan).tolist()),
                        ('repeat', _dice(s[C_IN:C_IN + LAGS], s[C_TN:C_TN + LAGS], nan).tolist())])


def describe_set(ids, e2w=None, lags=16, start=None, device=None, pitch_class=False):
    """One set alone: {'n', 'short', 'device_ms', 'profile' (pooled_profiles), 'means'}: means = the mean over the n pieces of W >= 2 of the
    scalar groups of structure_groups (nan when n = 0)."""
    lags = _check_lags(lags)
    return metrics.describe_pieces('structure', _op(pitch_class), lambda c: structure_groups(c, lags), SCALAR_GROUPS, pooled_profiles, ids,
                                   pieces.tables(e2w), start, device)


def compare_structure(gen_ids, ref_ids, e2w=None, lags=16, grid=1024, start=None, device=None, pitch_class=False):
    """Compare the repetition structure of a generated set with a reference set, both (N, S, 8) ids with S <= 4096. Per group of
    structure_groups (over the pieces of W >= 2) the record of metrics.compare_sets: mean_* and std_* (of the row norm for the two
    profile groups), dist_gen / dist_ref / dist_inter, kl, oa, kl_gen, oa_gen, with the same degenerate rule. start: one value or a
    (gen, ref) pair. Returns {'n_gen', 'n_ref', 'short_gen', 'short_ref', 'device_ms', 'profile_gen', 'profile_ref', 'groups'}."""
    lags = _check_lags(lags)
    return metrics.compare_pieces('compare_structure', 'structure', _op(pitch_class), lambda c: structure_groups(c, lags), GROUPS, gen_ids, ref_ids,
                                  pieces.tables(e2w), grid, start, device, profile=pooled_profiles)
