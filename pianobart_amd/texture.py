"""Texture of generated pieces: what sounds at once, in absolute time. A bar is as long as its time signature says, a note sounds from its
onset for its duration, and per piece that gives: how many pitches sound at each step (the polyphony histogram, its mean, the share of
silence), how much notes of one pitch overlap or collide, how often a note is written twice, how many notes run over their bar line or sit
behind the end of their bar, how many pitches start together and how far apart the onsets lie. The definitions are this
project's own, in the family of the polyphony and polyphonic-rate measures of the MuseGAN and MusDr evaluations; they are none of them
number for number.

The integer columns (pb_piece_texture) come from pb_texture.hip, the set comparison from the kernels of pianobart_amd.metrics; the host
divides integer columns. There is no CPU path."""
from collections import OrderedDict

import numpy as np
import torch

from . import metrics, ops, pieces
from ._lib import PBError

COLS = ops.TEXTURE_COLS
C_NOTES, C_P, C_W, C_T, C_U1, C_U2, C_A, C_MAXC, C_D, C_X, C_Y, C_O, C_TIED, C_OFFBAR, C_G = range(15)
C_POLY, N_POLY, C_CHORD, N_CHORD, C_IOI, N_IOI = 16, 17, 33, 9, 42, 16
SCALAR_GROUPS = ('silence_ratio', 'polyphony_mean', 'polyphonic_rate', 'max_polyphony', 'overlap_ratio', 'collision_rate', 'duplicate_rate',
                 'tie_rate', 'offbar_rate', 'chord_size_mean')
GROUPS = SCALAR_GROUPS + ('polyphony_hist', 'chord_hist', 'ioi_hist')


def _tables(e2w):
    """pieces.tables(e2w) whose every time signature has a bar length: the time axis is a sum of them."""
    tab = pieces.tables(e2w)
    bad = np.flatnonzero(np.asarray(tab.bar_pos) <= 0)
    if bad.size:
        raise PBError("texture: the time-signature id %d has no bar length: its word is not 'TimeSig n/d' with n * 64 // d in 1 .. %d"
                      % (int(bad[0]), pieces.MAX_BAR_POS))
    return tab


def piece_texture(ids, e2w=None, start=None, device=None):
    """The (N, 64) int32 device tensor of pb_piece_texture for (N, S, 8) ids, S <= 4096: integer or integer-valued float arrays or device
    tensors, checked as metrics.piece_features checks them. start: the first row that counts, one number or one per piece. e2w: a
    dictionary, None (the default one) or pieces.tables(); a time-signature word without a bar length is a PBError that names its id."""
    tab = _tables(e2w)
    return ops.piece_texture(**pieces.upload(ids, tab, start, device, max_S=ops.RUNS_MAX_S, dur_pos=tab.dur_pos, bar_pos=tab.bar_pos))


def kept_pieces(ids, tab=None, start=None):
    """Host: per piece of an (N, S, 8) integer array whether texture_groups keeps it: one of its notes at least is pitched (P >= 1)."""
    tab = pieces.tables(tab)
    live = pieces.live_rows(ids, tab.layout, start)[1]
    pit = np.where(live, np.asarray(ids)[:, :, 3], 0).astype(np.int64)
    return (live & (np.asarray(tab.pitch_of)[pit] >= 0)).any(1)


def _columns(cols):
    c = cols.detach().cpu().numpy() if torch.is_tensor(cols) else np.asarray(cols)
    if c.ndim != 2 or c.shape[1] != COLS or c.dtype.kind not in 'iu':
        raise PBError('texture: need an (N, %d) integer array of texture columns (got %s %s)' % (COLS, c.shape, c.dtype))
    return c.astype(np.int64)


def _ratio(a, b):
    """a / b in float64; 0 where b == 0."""
    out = np.zeros(np.broadcast(a, b).shape, dtype=np.float64)
    np.divide(a, b, out=out, where=b != 0)
    return out


def texture_groups(cols):
    """(groups, unpitched): the thirteen texture groups of an (N, 64) array of texture columns as float32 arrays over the n pieces that
    hold a pitched note (P >= 1); unpitched = the number of pieces left out. Divisions in float64, a zero divisor gives zeros.
      silence_ratio (n,)       the steps of [first onset, last end) at which nothing sounds / T
      polyphony_mean (n,)      A / U1: the pitches that sound, averaged over the steps at which one does
      polyphonic_rate (n,)     U2 / U1: the share of those steps at which two or more sound
      max_polyphony (n,)       the most pitches that sound at one step
      overlap_ratio (n,)       (D - A) / D: the share of the written note lengths that lies under another note of the same pitch
      collision_rate (n,)      X / G: the distinct (pitch, onset) struck while an earlier note of that pitch still sounds
      duplicate_rate (n,)      Y / P: the notes written once more on a (pitch, onset) that a note already has
      tie_rate (n,)            the notes that end behind the end of their bar / P
      offbar_rate (n,)         the notes whose position lies at or behind the end of their bar / P
      chord_size_mean (n,)     G / O: distinct pitches per distinct onset
      polyphony_hist (n, 17)   the steps with 0, 1, .., 15, >= 16 pitches sounding / T
      chord_hist (n, 9)        the onsets at which 1, .., 8, >= 9 distinct pitches start / O
      ioi_hist (n, 16)         the gaps g between consecutive onsets by min(floor(log2 g), 15) / max(O - 1, 1)"""
    c = _columns(cols)
    keep = c[:, C_P] >= 1
    unpitched = int((~keep).sum())
    c = c[keep]
    col = lambda i: c[:, i:i + 1]
    g = OrderedDict()
    g['silence_ratio'] = _ratio(c[:, C_POLY], c[:, C_T])
    g['polyphony_mean'] = _ratio(c[:, C_A], c[:, C_U1])
    g['polyphonic_rate'] = _ratio(c[:, C_U2], c[:, C_U1])
    g['max_polyphony'] = c[:, C_MAXC].astype(np.float64)
    g['overlap_ratio'] = _ratio(c[:, C_D] - c[:, C_A], c[:, C_D])
    g['collision_rate'] = _ratio(c[:, C_X], c[:, C_G])
    g['duplicate_rate'] = _ratio(c[:, C_Y], c[:, C_P])
    g['tie_rate'] = _ratio(c[:, C_TIED], c[:, C_P])
    g['offbar_rate'] = _ratio(c[:, C_OFFBAR], c[:, C_P])
    g['chord_size_mean'] = _ratio(c[:, C_G], c[:, C_O])
    g['polyphony_hist'] = _ratio(c[:, C_POLY:C_POLY + N_POLY], col(C_T))
    g['chord_hist'] = _ratio(c[:, C_CHORD:C_CHORD + N_CHORD], col(C_O))
    g['ioi_hist'] = _ratio(c[:, C_IOI:C_IOI + N_IOI], np.maximum(col(C_O) - 1, 1))
    return OrderedDict((k, g[k].astype(np.float32)) for k in GROUPS), unpitched


def pooled_profiles(cols):
    """Host: {'polyphony' (17), 'chord' (9)} of a set as lists of floats: the polyphony histogram summed over the pieces / the sum of T,
    the chord sizes summed / the sum of O; nan where the divisor is 0."""
    s = _columns(cols).sum(0)
    nan = float('nan')
    div = lambda a, b: [float(v) / float(b) if b else nan for v in a]
    return OrderedDict([('polyphony', div(s[C_POLY:C_POLY + N_POLY], s[C_T])), ('chord', div(s[C_CHORD:C_CHORD + N_CHORD], s[C_O]))])


def describe_set(ids, e2w=None, start=None, device=None):
    """One set alone: {'n', 'unpitched', 'device_ms', 'profile' (pooled_profiles), 'means'}: means = the mean over the n kept pieces of the
    scalar groups of texture_groups (nan when n = 0)."""
    tab = _tables(e2w)
    res = metrics.describe_pieces('texture', ops.piece_texture, texture_groups, SCALAR_GROUPS, pooled_profiles, ids, tab, start, device,
                                  dur_pos=tab.dur_pos, bar_pos=tab.bar_pos)
    return OrderedDict(('unpitched' if k == 'short' else k, v) for k, v in res.items())


def compare_texture(gen_ids, ref_ids, e2w=None, grid=1024, start=None, device=None):
    """Compare the texture of a generated set with a reference set, both (N, S, 8) ids with S <= 4096. Per group of texture_groups (over
    the kept pieces) the record of metrics.compare_sets: mean_* and std_* (of the row norm for the three histogram groups), dist_gen /
    dist_ref / dist_inter, kl, oa, kl_gen, oa_gen, with the same degenerate rule. start: one value or a (gen, ref) pair. Returns
    {'n_gen', 'n_ref', 'unpitched_gen', 'unpitched_ref', 'device_ms', 'profile_gen', 'profile_ref', 'groups'}."""
    tab = _tables(e2w)
    return metrics.compare_pieces('compare_texture', 'texture', ops.piece_texture, texture_groups, GROUPS, gen_ids, ref_ids, tab, grid, start,
                                  device, left_out='unpitched', profile=pooled_profiles, dur_pos=tab.dur_pos, bar_pos=tab.bar_pos)
