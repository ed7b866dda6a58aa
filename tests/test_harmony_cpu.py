"""CPU: the host half of the harmony metrics (pianobart_amd.harmony, eval_harmony), the entropy table and the yardstick itself
(tests/harmony_ref.py).

  * the table ops.harmony_table() against k log2(k) 2^20 evaluated with `decimal` at 60 digits, and the distance of every entry from a
    rounding tie (at least 1.47e-4, so any correct evaluation rounds alike);
  * the Counter form of the restatement against the note-list form on seeded pieces, with a start, a terminator and percussion;
  * hand-computed answers: only the class C (the key ties, the smallest k wins, entropy 0); the seven classes of C major equally often
    (scale_consistency 1, H_1 = log2 7 within the table's 13 * 2^-21); a two-bar motif written 2 semitones higher each time
    (I_X[2] = T_H[2] / 2, I_H[2] = 0); the window blocks of a small piece with an empty bar, by hand;
  * lag_profiles, harmony_groups and pooled_profiles on hand-made column arrays (T = 0, W < 2, P = 0, one non-empty bar, lags = 1 and
    64) and against the restatement on the restatement's own table; kept_pieces against the columns;
  * the C entry's argument checks (-2, the field named), the exported queries, the CLI's refusals and the refusal of a host tensor,
    none of which needs a device."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from pianobart_amd import _lib, ops
from pianobart_amd._lib import PBError
from tests import harmony_ref as R
from tests import metrics_ref as M
from tests import structure_ref as SR
from tests.vocab_layout_util import D_DEFAULT

PAD8, PITCH_OF, _ = M.tables_for(D_DEFAULT, 128)


def piece_of(notes, S=None):
    """(S, 8) rows from (bar, pitch id) pairs, an EOS row and a PAD tail behind them."""
    pad = np.asarray(PAD8)
    S = S or len(notes) + 2
    rows = np.tile(pad, (S, 1)).astype(np.int64)
    for r, (bar, pit) in enumerate(notes):
        rows[r] = [bar, 4 * (r % 16), 0, pit, 8, 20, 9, 30]
    rows[len(notes)] = pad + 3
    return rows


# ---- the table ------------------------------------------------------------------------------------------------------------------------
def test_table_against_60_digits():
    want, margin = R.table()
    got = ops.harmony_table()
    assert got.dtype == torch.int64 and tuple(got.shape) == (4097,) and not got.is_cuda
    assert got.tolist() == want
    assert want[0] == want[1] == 0 and want[2] == 2 << 20 and want[4096] == 4096 * 12 << 20
    assert margin >= 1.47e-4, margin                                      # no entry near a rounding tie: any correct evaluation gives these integers
    assert [int(round(k * math.log2(k) * 2.0 ** 20)) for k in range(2, 4097)] == want[2:]
    assert ops.HARMONY_LAGS == 64 and ops.HARMONY_COLS == 228 == R.COLS
    assert 1082 * 4096 * 12 * 2 ** 20 < 2 ** 46                           # the bound of every int64 sum


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def test_reference_counter_form_against_the_note_list_form():
    pieces = np.concatenate([M.synth_pieces(D_DEFAULT, 5, 90, seed=31), SR.motif_pieces(D_DEFAULT, 3, 90, seed=32, mb=(1, 2, 4), edit=0.3)])
    pieces[6, 70] = np.asarray(PAD8) + 3
    pieces[7, 10:30, 3] = 200                                             # a run of percussion
    start = np.array([0, 3, 40, 0, 89, 0, 0, 7])
    a, b = R.harmony(pieces, PAD8, PITCH_OF, start), R.harmony_notes(pieces, PAD8, PITCH_OF, start)
    bad = np.argwhere(a != b)
    assert not len(bad), (bad[:8], [(int(a[i, j]), int(b[i, j])) for i, j in bad[:8]])
    assert a[:, R.C_IH:R.C_TH].sum() > 0 and (a[:, R.C_IX:] >= a[:, R.C_IH:R.C_TH]).all() and (a[:, R.C_IX:] > a[:, R.C_IH:R.C_TH]).any()
    assert (a[:, 2] + a[:, 3] == a[:, 0]).all() and a[:, 3].sum() > 0 and (a[:, 8:20].sum(1) == a[:, 2]).all()
    assert (a[:, 4] == a[:, R.C_W1 + 1]).all() and (a[:, R.C_W1 + 2] == a[:, 2]).all() and (a[:, 7] == 0).all()
    rng = np.random.default_rng(5)
    shuffled = pieces.copy()
    shuffled[7, 7:] = pieces[7, 7:][rng.permutation(83)]                  # row order does not matter
    assert np.array_equal(R.harmony(shuffled, PAD8, PITCH_OF, start)[7], a[7])


def test_reference_only_the_class_c():
    c = R.harmony_one(piece_of([(b, 60 + 12 * (i % 2)) for b in range(4) for i in range(3)]), PAD8, PITCH_OF)
    assert c[:8] == [12, 4, 12, 0, 4, 0, 12, 0] and c[8:20] == [12] + [0] * 11          # K* = 0: D_0, 1, 3, 5, 7, 8, 10 all hold C, the smallest wins
    assert c[20:28] == [4, 4, 12, 0, 12, 4, 0, 4] and c[28:36] == [1, 1, 12, 0, 12, 1, 0, 1]
    assert c[36:39] == [9, 6, 3] and c[100:103] == [18, 12, 6] and c[164:167] == [9, 6, 3] and sum(c[39:100]) == 0
    g, short = R.groups(np.array([c]))
    assert short == 0 and g['pc_entropy_1'][0] == 0 and g['pc_entropy_4'][0] == 0 and g['scale_consistency'][0] == 1 and g['key_stability'][0] == 1
    assert g['harmony_mean'][0] == 1 and g['sequence_gain'][0] == 0 and g['classes_per_bar'][0] == 1 and g['key_change_rate'][0] == 0


def test_reference_c_major_equally_often():
    scale = [60, 62, 64, 65, 67, 69, 71]
    c = R.harmony_one(piece_of([(b, p) for b in range(3) for p in scale]), PAD8, PITCH_OF)
    assert c[:8] == [21, 3, 21, 0, 3, 0, 21, 0]
    g, _ = R.groups(np.array([c]))
    assert g['scale_consistency'][0] == 1 and g['local_scale_1'][0] == 1 and g['key_stability'][0] == 0          # W = 3: no window of 4, 0 / 0 gives 0
    h1 = c[R.C_W1 + 3] / (2.0 ** 20 * c[R.C_W1 + 2])
    assert abs(h1 - math.log2(7)) <= 13 * 2.0 ** -21 and abs(float(g['pc_entropy_1'][0]) - math.log2(7)) <= 13 * 2.0 ** -21 + 2.0 ** -22
    assert c[R.C_W4] == 0 and g['pc_entropy_4'][0] == 0
    c = R.harmony_one(piece_of([(b, p + 7) for b in range(5) for p in scale]), PAD8, PITCH_OF)                   # G major
    TL = R.table()[0]
    assert c[5] == 7 and c[6] == 35 and c[R.C_W4:R.C_W4 + 8] == [2, 2, 56, 2 * (TL[28] - 7 * TL[4]), 56, 2, 0, 14]
    h4 = c[R.C_W4 + 3] / (2.0 ** 20 * 56)
    assert abs(h4 - math.log2(7)) <= 13 * 2.0 ** -21


def test_reference_transposing_motif():
    piece = R.sequence_piece(D_DEFAULT, 6, step=2)
    c = R.harmony_one(piece, PAD8, PITCH_OF)
    assert c[:5] == [48, 12, 48, 0, 12]
    assert c[R.C_TH + 1] == 2 * 40 and c[R.C_IX + 1] == 40 and c[R.C_IH + 1] == 0                                # lag 2: the same bar, 2 semitones up
    assert 2 * c[R.C_IX + 1] == c[R.C_TH + 1] and c[R.C_IX + 3] * 2 == c[R.C_TH + 3]                             # lag 4 as well
    assert c[R.C_IX] * 2 < c[R.C_TH]                                                                             # lag 1: 5 notes against 3
    h, x = R.profiles(np.array([c]))
    assert x[0, 1] == 1.0 and h[0, 1] == 0.0 and math.isnan(x[0, 11]) and (x[0, :11] >= h[0, :11]).all()
    assert c[R.C_W1 + 6] > 0                                                                                     # the key moves


def test_reference_window_blocks_by_hand():
    # bars: 0 {C, E, G}, 1 empty, 2 {C, C, F#}, 3 {D}, 4 percussion only
    notes = [(0, 60), (0, 64), (0, 67), (2, 60), (2, 72), (2, 66), (3, 62), (4, 200)]
    TL = R.table()[0]
    c = R.harmony_one(piece_of(notes), PAD8, PITCH_OF)
    assert c[:5] == [8, 5, 7, 1, 3]
    assert c[8:20] == [3, 0, 1, 0, 1, 0, 1, 1, 0, 0, 0, 0]
    assert (c[5], c[6]) == (7, 7)                                          # G major holds C D E F# G: all 7; no smaller k does (C major misses F#)
    x1 = TL[3] + (TL[3] - TL[2]) + 0
    # keys: bar 0 {C, E, G}: D_0 holds all three, key 0; bar 2 {C, C, F#}: the smallest k whose D_k holds C and F# is 1; bar 3 {D}: key 0
    assert c[20:28] == [5, 3, 7, x1, 3 + 3 + 1, 0, 2, 3 + 2 + 1]
    # windows of 4: bars 0 .. 3 = all pitched notes (best 7, key 7); bars 1 .. 4 = {C, C, F#, D}: G major holds all four, no smaller k does
    x4 = (TL[7] - TL[3]) + (TL[4] - TL[2])
    assert c[28:36] == [2, 2, 11, x4, 7 + 4, 2, 0, 5 + 3]
    assert c[R.C_IH:R.C_IH + 5] == [0, 1, 0, 0, 0] and c[R.C_TH:R.C_TH + 5] == [3 + 3 + 4 + 1, 6 + 1 + 3, 4 + 0, 3, 0]
    assert c[R.C_IX:R.C_IX + 5] == [1, 1, 1, 0, 0]                         # lag 1: {C, C, F#} against {D}; lag 2: no two of C, E, G lie a tritone apart


# ---- the host half -------------------------------------------------------------------------------------------------------------------
def hand_columns():
    """Rows: 0 an ordinary piece; 1 W = 1; 2 no note; 3 percussion only (W = 6, P = 0); 4 one non-empty bar, nothing at any lag; 5 only lag 64."""
    c = np.zeros((6, 228), dtype=np.int64)
    c[0, :8] = [40, 9, 36, 4, 8, 7, 30, 0]
    c[0, 20:28] = [9, 8, 36, 50 << 20, 33, 5, 3, 20]
    c[0, 28:36] = [6, 6, 130, 300 << 20, 110, 4, 1, 30]
    c[0, 36:39], c[0, 100:103], c[0, 164:167] = [5, 9, 0], [50, 44, 38], [7, 9, 4]
    c[1, :8] = [12, 1, 12, 0, 1, 0, 12, 0]
    c[1, 20:28] = [1, 1, 12, 0, 12, 1, 0, 1]
    c[3, :5] = [30, 6, 0, 30, 0]
    c[3, 20], c[3, 28] = 6, 3
    c[4, :8] = [8, 3, 8, 0, 1, 2, 6, 0]
    c[4, 20:28] = [3, 1, 8, 9 << 20, 6, 1, 0, 4]
    c[4, 100:102] = [8, 8]
    c[5, :8] = [9, 70, 9, 0, 3, 0, 9, 0]
    c[5, 20:28] = [70, 3, 9, 0, 9, 3, 0, 3]
    c[5, 28:36] = [67, 12, 36, 40 << 20, 36, 12, 0, 12]
    c[5, 36 + 63], c[5, 100 + 63], c[5, 164 + 63] = 1, 6, 2
    return c


def test_lag_profiles():
    from pianobart_amd import harmony
    c = hand_columns()
    h, x = harmony.lag_profiles(c)
    assert h.dtype == np.float64 and h.shape == x.shape == (6, 64)
    assert h[0, 0] == 10 / 50 and h[0, 1] == 18 / 44 and h[0, 2] == 0.0 and x[0, 0] == 14 / 50 and x[0, 2] == 8 / 38
    assert np.isnan(h[0, 3:]).all() and np.isnan(h[1]).all() and np.isnan(x[2]).all() and h[4, 0] == 0 and np.isnan(h[4, 2])
    assert h[5, 63] == 2 / 6 and x[5, 63] == 4 / 6
    want = R.profiles(c)
    assert np.array_equal(h, want[0], equal_nan=True) and np.array_equal(x, want[1], equal_nan=True)
    assert np.array_equal(harmony.lag_profiles(torch.from_numpy(c))[1], x, equal_nan=True)
    for bad in (c[:, :227], c.astype(np.float64), c[0]):
        with pytest.raises(PBError):
            harmony.lag_profiles(bad)


@pytest.mark.parametrize('lags', [1, 2, 16, 64])
def test_harmony_groups(lags):
    from pianobart_amd import harmony
    c = hand_columns()
    g, short = harmony.harmony_groups(c, lags)
    assert short == 3 and list(g) == list(harmony.GROUPS) == list(R.GROUPS)                        # W = 1, no note, P = 0
    assert g['harmony_profile'].shape == g['sequence_profile'].shape == (3, lags) and g['pc_entropy_1'].shape == (3,)
    assert all(v.dtype == np.float32 for v in g.values())
    assert g['pc_entropy_1'][0] == np.float32(50 / 36) and g['pc_entropy_4'][0] == np.float32(300 / 130)
    assert g['scale_consistency'][0] == np.float32(30 / 36) and g['local_scale_1'][0] == np.float32(33 / 36) and g['local_scale_4'][0] == np.float32(110 / 130)
    assert g['key_stability'][0] == np.float32(4 / 6) and g['key_change_rate'][0] == np.float32(3 / 7) and g['classes_per_bar'][0] == np.float32(20 / 8)
    assert g['key_change_rate'][1] == 0 and g['key_stability'][1] == 0                             # one non-empty bar: 0 / 0 gives 0; no window of 4
    if lags >= 3:
        assert g['harmony_mean'][0] == np.float32(2 * 14 / 132) and g['sequence_gain'][0] == np.float32(2 * 6 / 132)
        assert g['harmony_profile'][1, 2] == 0                                                     # a zero divisor gives zero, not nan
    if lags == 1:
        assert g['harmony_mean'][0] == np.float32(10 / 50) and g['sequence_gain'][0] == np.float32(4 / 50)
    assert g['sequence_gain'][2] == (np.float32(2 / 6) if lags == 64 else 0)
    want, want_short = R.groups(c, lags)
    assert want_short == short
    for k in g:
        assert np.array_equal(g[k], want[k]), k


def test_harmony_groups_on_the_restatements_table_and_refusals():
    from pianobart_amd import harmony
    pieces = np.concatenate([SR.motif_pieces(D_DEFAULT, 6, 120, seed=41, mb=(1, 2, 3), edit=0.4), M.synth_pieces(D_DEFAULT, 4, 120, seed=42)])
    pieces[2, 1:, 0] = pieces[2, 0, 0]                                                             # one bar only: W = 1
    pieces[4, :, 3] = 200                                                                          # percussion only: P = 0
    c = R.harmony(pieces, PAD8, PITCH_OF)
    for lags in (1, 7, 64):
        g, short = harmony.harmony_groups(c, lags)
        want, want_short = R.groups(c, lags)
        assert short == want_short == 2 and all(np.array_equal(g[k], want[k]) for k in g)
    got, want = harmony.pooled_profiles(c), R.pooled(c)
    assert np.array_equal(got['harmony'], want['harmony'], equal_nan=True) and np.array_equal(got['sequence'], want['sequence'], equal_nan=True)
    from pianobart_amd import metrics
    tab = metrics.tables()
    assert (tab.pitch_of == PITCH_OF).all()
    assert np.array_equal(harmony.kept_pieces(pieces, tab), (c[:, 1] >= 2) & (c[:, 2] >= 1))
    c100 = R.harmony(pieces, PAD8, PITCH_OF, 100)
    assert np.array_equal(harmony.kept_pieces(pieces, tab, start=100), (c100[:, 1] >= 2) & (c100[:, 2] >= 1))
    for lags in (0, 65, 2.5, True):
        with pytest.raises(PBError, match='lags'):
            harmony.harmony_groups(c, lags)
    empty, short = harmony.harmony_groups(c[2:3], 4)
    assert short == 1 and empty['harmony_profile'].shape == (0, 4) and empty['key_stability'].shape == (0,)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_host_tensors_are_refused():
    from pianobart_amd import harmony
    with pytest.raises(PBError, match='no CPU path'):
        ops.piece_harmony(torch.zeros(2, 4, 8, dtype=torch.int16), torch.zeros(256, dtype=torch.int16))
    with pytest.raises(PBError, match='no CPU path'):
        harmony.piece_harmony(torch.zeros(2, 4, 8, dtype=torch.int64))
    with pytest.raises(PBError, match=r'\(N, S, 8\)'):
        harmony.piece_harmony(np.zeros((2, 4, 7), dtype=np.int64))
    with pytest.raises(PBError, match=r'head 0 \(Bar\)'):
        harmony.piece_harmony(np.full((1, 4, 8), 262, dtype=np.int64))


PTR = 0x10000
_PAD8 = (ctypes.c_int32 * 8)(*ops.DEFAULT_LAYOUT.pad8)
_WIDE_PAD8 = (ctypes.c_int32 * 8)(1100, 128, 129, 256, 128, 32, 254, 49)
_ENTRY_REFUSALS = [
    ((PTR + 2, None, _PAD8, PTR, PTR, PTR, 4, 16, None), 'ids16'),
    ((None, None, _PAD8, PTR, PTR, PTR, 4, 16, None), 'ids16'),
    ((PTR, PTR + 2, _PAD8, PTR, PTR, PTR, 4, 16, None), 'start'),
    ((PTR, None, None, PTR, PTR, PTR, 4, 16, None), 'pad8'),
    ((PTR, None, _PAD8, None, PTR, PTR, 4, 16, None), 'pitch_of'),
    ((PTR, None, _PAD8, PTR, None, PTR, 4, 16, None), 'table'),
    ((PTR, None, _PAD8, PTR, PTR + 4, PTR, 4, 16, None), 'table'),
    ((PTR, None, _PAD8, PTR, PTR, None, 4, 16, None), 'out'),
    ((PTR, None, _PAD8, PTR, PTR, PTR + 4, 4, 16, None), 'out'),
    ((PTR, None, _PAD8, PTR, PTR, PTR, -1, 16, None), 'N = -1'),
    ((PTR, None, _PAD8, PTR, PTR, PTR, 4, 0, None), 'S = 0'),
    ((PTR, None, _PAD8, PTR, PTR, PTR, 4, 4097, None), 'S = 4097'),
    ((PTR, None, _WIDE_PAD8, PTR, PTR, PTR, 4, 16, None), 'pad8[0] = 1100'),
]


@pytest.mark.parametrize('args,names', _ENTRY_REFUSALS, ids=['%d-%s' % (i, n) for i, (_, n) in enumerate(_ENTRY_REFUSALS)])
def test_the_entry_checks_its_arguments_before_any_device_call(args, names):
    with pytest.raises(PBError) as e:
        _lib.LIB.call('pb_piece_harmony', *args)
    assert 'pb_piece_harmony' in str(e.value) and '(-2)' in str(e.value) and names in str(e.value), str(e.value)


def test_abi_version_is_still_10_and_the_entries_are_exported():
    decls = _lib.parse_header()
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    assert decls['pb_piece_harmony'] == (ctypes.c_int, [vp] * 6 + [i32, i32, vp])
    assert decls['pb_harmony_lags'] == (ctypes.c_int, []) and decls['pb_harmony_cols'] == (ctypes.c_int, [])
    assert _lib.LIB.query('pb_abi_version') == 10
    assert _lib.LIB.query('pb_harmony_lags') == ops.HARMONY_LAGS and _lib.LIB.query('pb_harmony_cols') == ops.HARMONY_COLS
    _lib.LIB.call('pb_piece_harmony', None, None, _PAD8, PTR, PTR, None, 0, 16, None)              # N = 0 is no error (and no launch)


# ---- the CLI ----------------------------------------------------------------------------------------------------------------------------
def _files(tmp_path, gen, ref=None):
    g, r = str(tmp_path / 'g.npy'), str(tmp_path / 'r.npy')
    np.save(g, gen)
    argv = ['--generated', g, '--output', str(tmp_path / 'h.json')]
    if ref is not None:
        np.save(r, ref)
        argv += ['--reference', r]
    return argv


def test_cli_refusals(tmp_path):
    from pianobart_amd import eval_harmony
    ok = SR.motif_pieces(D_DEFAULT, 4, 24, seed=1).astype(np.float32)
    argv = _files(tmp_path, ok, ok)
    with pytest.raises(PBError, match='--cpu'):
        eval_harmony.main(argv + ['--cpu'])
    with pytest.raises(PBError, match='--cpu'):
        eval_harmony.main(_files(tmp_path, ok) + ['--cpu'])
    with pytest.raises(PBError, match='no file'):
        eval_harmony.main(['--generated', str(tmp_path / 'missing.npy')] + argv[2:])
    with pytest.raises(PBError, match='no file'):
        eval_harmony.main(argv[:4] + ['--reference', str(tmp_path / 'missing.npy')])
    with pytest.raises(PBError, match='no file'):
        eval_harmony.main(argv + ['--dict_file', str(tmp_path / 'missing.json')])
    with pytest.raises(PBError, match='rows of 8 ids'):
        eval_harmony.main(_files(tmp_path, ok[:, :, :7], ok))
    with pytest.raises(PBError, match='rows of 8 ids'):
        eval_harmony.main(_files(tmp_path, ok[0, 0]))
    with pytest.raises(PBError, match='at most 4096'):
        eval_harmony.main(_files(tmp_path, np.zeros((1, 4097, 8), dtype=np.int16)))
    for flags in (['--lags', '0'], ['--lags', '65'], ['--grid', '1'], ['--grid', '5000'], ['--skip', '-1'], ['--max_pieces', '0']):
        with pytest.raises(PBError, match=flags[0]):
            eval_harmony.main(argv + flags)
        with pytest.raises(PBError, match=flags[0]):
            eval_harmony.main(_files(tmp_path, ok) + flags)
    flat = ok.copy()
    flat[1:, :, 0] = 5                                                     # one piece of two bars or more left
    with pytest.raises(PBError, match=r'--generated holds 1 pieces'):
        eval_harmony.main(_files(tmp_path, flat, ok))
    with pytest.raises(PBError, match=r'--reference holds 1 pieces'):
        eval_harmony.main(_files(tmp_path, ok, flat))
    drums = ok.copy()
    drums[1:, :, 3] = 200                                                  # one piece with a pitched note left
    with pytest.raises(PBError, match=r'--reference holds 1 pieces'):
        eval_harmony.main(_files(tmp_path, ok, drums))
    with pytest.raises(PBError, match=r'--generated holds 0 pieces'):
        eval_harmony.main(_files(tmp_path, ok, ok) + ['--skip', '24'])
    with pytest.raises(PBError, match=r'--generated holds 1 pieces'):
        eval_harmony.main(_files(tmp_path, ok, ok) + ['--max_pieces', '1'])
    assert not os.path.exists(str(tmp_path / 'h.json'))
