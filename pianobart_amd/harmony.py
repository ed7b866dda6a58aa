"""Harmony of generated pieces: which pitch classes a piece uses, bar by bar. Per piece the pitch-class entropy of its bars and of its
four-bar windows, how well one diatonic set (a key) holds the piece and its windows and how often the best one changes, and, for lags of
1 .. 64 bars, the pooled Dice similarity of the bars' pitch-class histograms that far apart: as they are (the harmonic repetition profile)
and up to transposition (the sequence profile). The definition is this project's own, in the family of the pitch-class
entropies H1 / H4 of Wu & Yang's "Jazz Transformer" evaluation (MusDr), of the scale consistency of the C-RNN-GAN / MuseGAN evaluations and
of self-similarity lag profiles; it is none of them number for number.

The integer columns (pb_piece_harmony) come from pb_harmony.hip, the set comparison from the kernels of pianobart_amd.metrics; the host
divides integer columns. There is no CPU path."""
from collections import OrderedDict

import numpy as np
import torch

from . import metrics, ops, pieces
from ._lib import PBError

LAGS, COLS = ops.HARMONY_LAGS, ops.HARMONY_COLS
C_G, C_W1, C_W4, C_IH, C_TH, C_IX = 8, 20, 28, 36, 36 + LAGS, 36 + 2 * LAGS
W_WINDOWS, W_SOME, W_N, W_X, W_BEST, W_AGREE, W_CHANGES, W_CLASSES = range(8)         # the eight values of a window block
GROUPS = ('pc_entropy_1', 'pc_entropy_4', 'scale_consistency', 'local_scale_1', 'local_scale_4', 'key_stability', 'key_change_rate',
          'classes_per_bar', 'harmony_profile', 'sequence_profile', 'harmony_mean', 'sequence_gain')
SCALAR_GROUPS = tuple(g for g in GROUPS if not g.endswith('_profile'))


def piece_harmony(ids, e2w=None, start=None, device=None):
    """The (N, 228) int64 device tensor of pb_piece_harmony for (N, S, 8) ids, S <= 4096: integer or integer-valued float arrays or device
    tensors, checked as metrics.piece_features checks them. start: the first row that counts, one number or one per piece. e2w: a
    dictionary, None (the default one) or metrics.tables()."""
    return ops.piece_harmony(**pieces.upload(ids, pieces.tables(e2w), start, device))


def kept_pieces(ids, tab=None, start=None):
    """Host: per piece of an (N, S, 8) integer array whether harmony_groups keeps it: its notes span two bars or more (W >= 2) and one of
    them at least is pitched (P >= 1)."""
    tab = pieces.tables(tab)
    live = pieces.live_rows(ids, tab.layout, start)[1]
    pit = np.where(live, np.asarray(ids)[:, :, 3], 0).astype(np.int64)
    return (pieces.bar_spans(ids, tab.layout, start) >= 2) & (live & (np.asarray(tab.pitch_of)[pit] >= 0)).any(1)


def _columns(cols):
    c = cols.detach().cpu().numpy() if torch.is_tensor(cols) else np.asarray(cols)
    if c.ndim != 2 or c.shape[1] != COLS or c.dtype.kind not in 'iu':
        raise PBError('harmony: need an (N, %d) integer array of harmony columns (got %s %s)' % (COLS, c.shape, c.dtype))
    return c.astype(np.int64)


def _ratio(a, b, zero, scale=1.0):
    """scale a / b in float64; `zero` where b == 0."""
    out = np.full(np.broadcast(a, b).shape, zero, dtype=np.float64)
    np.divide(scale * a, b, out=out, where=b != 0)
    return out


def lag_profiles(cols):
    """Host, float64: (harmony, sequence), each (N, 64): D_H[l] = 2 I_H[l] / T_H[l] and D_X[l] = 2 I_X[l] / T_H[l] of every piece for
    l = 1 .. 64, nan where T_H[l] == 0 (no bar pair that far apart holds a pitched note)."""
    c = _columns(cols)
    nan = float('nan')
    t = c[:, C_TH:C_TH + LAGS]
    return _ratio(c[:, C_IH:C_IH + LAGS], t, nan, 2.0), _ratio(c[:, C_IX:C_IX + LAGS], t, nan, 2.0)


def _check_lags(lags):
    if isinstance(lags, bool) or int(lags) != lags or not 1 <= int(lags) <= LAGS:
        raise PBError('harmony: lags = %r; 1 .. %d' % (lags, LAGS))
    return int(lags)


def harmony_groups(cols, lags=16):
    """(groups, short): the twelve harmony groups of an (N, 228) array of harmony columns as float32 arrays over the n pieces that span at
    least two bars and hold a pitched note (W >= 2 and P >= 1); short = the number of pieces left out. Divisions in float64, a zero divisor
    gives zeros.
      pc_entropy_1, pc_entropy_4 (n,)            H_w = sum X / (2^20 sum n) over the windows of 1 and of 4 bars: bits, note-weighted
      scale_consistency (n,)                     SC / P: the share of the piece's pitched notes inside its best diatonic set
      local_scale_1, local_scale_4 (n,)          sum best / sum n over the windows
      key_stability (n,)                         w = 4: the non-empty windows whose key is the piece's / the non-empty windows
      key_change_rate (n,)                       w = 1: key changes / (non-empty bars - 1)
      classes_per_bar (n,)                       w = 1: sum of the classes present / non-empty bars
      harmony_profile, sequence_profile (n, lags)   D_H[l], D_X[l] for l = 1 .. lags
      harmony_mean (n,)                          2 sum_l I_H / sum_l T_H over the same lags
      sequence_gain (n,)                         2 sum_l (I_X - I_H) / sum_l T_H: what transposition adds"""
    lags = _check_lags(lags)
    c = _columns(cols)
    keep = (c[:, 1] >= 2) & (c[:, 2] >= 1)
    short = int((~keep).sum())
    c = c[keep]
    w1, w4 = c[:, C_W1:C_W1 + 8], c[:, C_W4:C_W4 + 8]
    ih, th, ix = (c[:, o:o + lags] for o in (C_IH, C_TH, C_IX))
    one = float(1 << ops.HARMONY_SHIFT)
    g = OrderedDict()
    g['pc_entropy_1'] = _ratio(w1[:, W_X], one * w1[:, W_N], 0.0)
    g['pc_entropy_4'] = _ratio(w4[:, W_X], one * w4[:, W_N], 0.0)
    g['scale_consistency'] = _ratio(c[:, 6], c[:, 2], 0.0)
    g['local_scale_1'] = _ratio(w1[:, W_BEST], w1[:, W_N], 0.0)
    g['local_scale_4'] = _ratio(w4[:, W_BEST], w4[:, W_N], 0.0)
    g['key_stability'] = _ratio(w4[:, W_AGREE], w4[:, W_SOME], 0.0)
    g['key_change_rate'] = _ratio(w1[:, W_CHANGES], w1[:, W_SOME] - 1, 0.0)
    g['classes_per_bar'] = _ratio(w1[:, W_CLASSES], w1[:, W_SOME], 0.0)
    g['harmony_profile'] = _ratio(ih, th, 0.0, 2.0)
    g['sequence_profile'] = _ratio(ix, th, 0.0, 2.0)
    g['harmony_mean'] = _ratio(ih.sum(1), th.sum(1), 0.0, 2.0)
    g['sequence_gain'] = _ratio((ix - ih).sum(1), th.sum(1), 0.0, 2.0)
    return OrderedDict((k, g[k].astype(np.float32)) for k in GROUPS), short


def pooled_profiles(cols):
    """Host: {'harmony', 'sequence'}: per lag 1 .. 64 the pooled 2 sum_pieces I[l] / sum_pieces T_H[l] of a set as lists of floats, nan where
    no piece of the set has a bar pair that far apart."""
    c = _columns(cols)
    nan = float('nan')
    s = c.sum(0)
    return OrderedDict([('harmony', _ratio(s[C_IH:C_IH + LAGS], s[C_TH:C_TH + LAGS], nan, 2.0).tolist()),
                        ('sequence', _ratio(s[C_IX:C_IX + LAGS], s[C_TH:C_TH + LAGS], nan, 2.0).tolist())])


def describe_set(ids, e2w=None, lags=16, start=None, device=None):
    """One set alone: {'n', 'short', 'device_ms', 'profile' (pooled_profiles), 'means'}: means = the mean over the n kept pieces of the
    scalar groups of harmony_groups (nan when n = 0)."""
    lags = _check_lags(lags)
    return metrics.describe_pieces('harmony', ops.piece_harmony, lambda c: harmony_groups(c, lags), SCALAR_GROUPS, pooled_profiles, ids,
                                   pieces.tables(e2w), start, device)


def compare_harmony(gen_ids, ref_ids, e2w=None, lags=16, grid=1024, start=None, device=None):
    """Compare the harmony of a generated set with a reference set, both (N, S, 8) ids with S <= 4096. Per group of harmony_groups (over
    the kept pieces) the record of metrics.compare_sets: mean_* and std_* (of the row norm for the two profile groups), dist_gen /
    dist_ref / dist_inter, kl, oa, kl_gen, oa_gen, with the same degenerate rule. start: one value or a (gen, ref) pair. Returns
    {'n_gen', 'n_ref', 'short_gen', 'short_ref', 'device_ms', 'profile_gen', 'profile_ref', 'groups'}."""
    lags = _check_lags(lags)
    return metrics.compare_pieces('compare_harmony', 'harmony', ops.piece_harmony, lambda c: harmony_groups(c, lags), GROUPS, gen_ids, ref_ids,
                                  pieces.tables(e2w), grid, start, device, profile=pooled_profiles)
