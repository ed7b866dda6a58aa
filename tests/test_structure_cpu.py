"""CPU: the host half of the repetition structure metrics (pianobart_amd.structure, eval_structure) and the yardstick itself
(tests/structure_ref.py).

  * hand-computed answers for the restatement: a two-bar motif written four times (D_N[2] = D_N[4] = 1, D_N[1] = D_O[1] = 14 / 35), the
    same motif an octave up in every second copy (D_N[2] = 0 by pitch, 1 by pitch class), one note on three instruments counts once;
  * the set form against the note-pair loop on seeded pieces, both modes, with a start and a terminator;
  * lag_profiles and structure_groups on hand-made column arrays (T = 0, W < 2, the tie rule of repeat_period, lags = 1 and 64) and
    against the restatement on the restatement's own table; bar_spans against column 1;
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
from tests import metrics_ref as M
from tests import structure_ref as R
from tests.vocab_layout_util import D_DEFAULT

PAD8, PITCH_OF, _ = M.tables_for(D_DEFAULT, 128)


def piece_of(notes, S=None):
    """(S, 8) rows from (bar, position, instrument, pitch id) tuples, an EOS row and a PAD tail behind them."""
    pad = np.asarray(PAD8)
    S = S or len(notes) + 2
    rows = np.tile(pad, (S, 1)).astype(np.int64)
    for r, (bar, pos, ins, pit) in enumerate(notes):
        rows[r] = [bar, pos, ins, pit, 8, 20, 9, 30]
    rows[len(notes)] = pad + 3
    return rows


BAR_A, BAR_B = [(0, 60), (16, 64)], [(0, 60), (32, 67), (48, 64)]


def motif_four_times(octave_up=False):
    notes = []
    for copy in range(4):
        for b, bar in enumerate((BAR_A, BAR_B)):
            notes += [(2 * copy + b, p, 0, pit + (12 if octave_up and copy % 2 else 0)) for p, pit in bar]
    return piece_of(notes)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def test_reference_two_bar_motif_written_four_times():
    c = R.structure_one(motif_four_times(), PAD8, PITCH_OF)
    assert c[:8] == [20, 8, 20, 20, 8, 0, 0, 0]
    assert (c[136 + 1], c[200 + 1]) == (15, 30) and (c[136 + 3], c[200 + 3]) == (10, 20)          # lags 2 and 4: every bar meets itself
    assert (c[136], c[200]) == (7, 35) and (c[8], c[72]) == (7, 35)                                # lag 1: A and B share (0, 60) only
    assert (c[8 + 7], c[72 + 7], c[136 + 7], c[200 + 7]) == (0, 0, 0, 0)                           # lag 8 = W: no pair
    groove, repeat = R.lag_profiles(np.array([c]))
    assert repeat[0, 1] == 1.0 and repeat[0, 3] == 1.0 and repeat[0, 0] == 14 / 35 and groove[0, 0] == 14 / 35
    assert math.isnan(repeat[0, 7]) and math.isnan(groove[0, 63])


def test_reference_octave_up_in_every_second_copy():
    piece = motif_four_times(octave_up=True)
    exact, by_class = R.structure_one(piece, PAD8, PITCH_OF, 0, 0), R.structure_one(piece, PAD8, PITCH_OF, 0, 1)
    assert (exact[136 + 1], exact[200 + 1]) == (0, 30) and (by_class[136 + 1], by_class[200 + 1]) == (15, 30)
    assert (exact[136 + 3], exact[200 + 3]) == (10, 20)                                            # four bars on, the same octave again
    assert exact[8:136] == by_class[8:136] == R.structure_one(motif_four_times(), PAD8, PITCH_OF)[8:136]      # the onsets do not care


def test_reference_one_note_on_three_instruments_counts_once():
    c = R.structure_one(piece_of([(3, 0, 0, 60), (3, 0, 1, 60), (3, 0, 2, 60), (4, 0, 0, 60)]), PAD8, PITCH_OF)
    assert c[:8] == [4, 2, 2, 2, 2, 0, 0, 0]
    assert (c[8], c[72], c[136], c[200]) == (1, 2, 1, 2) and sum(c[8:]) == 6
    drums = R.structure_one(piece_of([(0, 0, 0, 130), (1, 0, 0, 142)]), PAD8, PITCH_OF, 0, 1)      # 142 - 130 = 12: percussion is no pitch class
    assert (drums[8], drums[136], drums[200]) == (1, 0, 2)


@pytest.mark.parametrize('mode', [0, 1])
def test_reference_set_form_against_the_pair_loop(mode):
    pieces = np.concatenate([M.synth_pieces(D_DEFAULT, 5, 90, seed=31), R.motif_pieces(D_DEFAULT, 3, 90, seed=32, mb=(1, 2, 4), edit=0.3)])
    pieces[6, 70] = np.asarray(PAD8) + 3
    start = np.array([0, 3, 40, 0, 89, 0, 0, 7])
    a, b = R.structure(pieces, PAD8, PITCH_OF, start, mode), R.structure_pairs(pieces, PAD8, PITCH_OF, start, mode)
    assert np.array_equal(a, b) and a[:, 8:].sum() > 0 and a[:, 136:200].sum() > 0
    assert (a[:, 136:200] <= a[:, 8:72]).all() and (a[:, 2] <= a[:, 3]).all() and (a[:, 3] <= a[:, 0]).all()
    rng = np.random.default_rng(5)
    shuffled = pieces.copy()
    shuffled[7, 7:] = pieces[7, 7:][rng.permutation(83)]                   # row order does not matter
    assert np.array_equal(R.structure(shuffled, PAD8, PITCH_OF, start, mode)[7], a[7])


# ---- the host half -------------------------------------------------------------------------------------------------------------------
def hand_columns():
    """Rows: 0 an ordinary piece; 1 W = 1; 2 no note; 3 ties (lags 2 and 4 both 2 * 3 / 8 = 2 * 6 / 16); 4 nothing repeats; 5 only lag 64."""
    c = np.zeros((6, 264), dtype=np.int64)
    c[0, :5] = [40, 9, 30, 36, 9]
    c[0, 8:11], c[0, 72:75] = [5, 9, 0], [50, 44, 38]
    c[0, 136:139], c[0, 200:203] = [2, 9, 0], [60, 52, 46]
    c[1, :5] = [12, 1, 5, 7, 1]
    c[3, :5] = [30, 6, 10, 10, 6]
    c[3, 136:140], c[3, 200:204] = [1, 3, 0, 6], [16, 8, 0, 16]
    c[3, 8:12], c[3, 72:76] = [1, 3, 0, 6], [16, 8, 0, 16]
    c[4, :5] = [8, 3, 8, 8, 3]
    c[4, 72:74], c[4, 200:202] = [10, 5], [10, 5]
    c[5, :5] = [9, 70, 9, 9, 3]
    c[5, 8 + 63], c[5, 72 + 63], c[5, 136 + 63], c[5, 200 + 63] = 2, 6, 1, 6
    return c


def test_lag_profiles():
    from pianobart_amd import structure
    c = hand_columns()
    groove, repeat = structure.lag_profiles(c)
    assert groove.dtype == np.float64 and groove.shape == repeat.shape == (6, 64)
    assert groove[0, 0] == 10 / 50 and groove[0, 1] == 18 / 44 and groove[0, 2] == 0.0 and repeat[0, 1] == 18 / 52
    assert np.isnan(groove[0, 3:]).all() and np.isnan(groove[1]).all() and np.isnan(repeat[2]).all()
    assert repeat[3, 1] == repeat[3, 3] == 0.75 and np.isnan(repeat[3, 2]) and repeat[5, 63] == 2 / 6 and groove[5, 63] == 4 / 6
    want = R.lag_profiles(c)
    assert np.array_equal(groove, want[0], equal_nan=True) and np.array_equal(repeat, want[1], equal_nan=True)
    assert np.array_equal(structure.lag_profiles(torch.from_numpy(c.astype(np.int32)))[1], repeat, equal_nan=True)
    for bad in (c[:, :263], c.astype(np.float64), c[0]):
        with pytest.raises(PBError):
            structure.lag_profiles(bad)


@pytest.mark.parametrize('lags', [1, 2, 16, 64])
def test_structure_groups(lags):
    from pianobart_amd import structure
    c = hand_columns()
    g, short = structure.structure_groups(c, lags)
    assert short == 2 and list(g) == list(structure.GROUPS) == list(R.GROUPS)
    assert g['groove_profile'].shape == g['repeat_profile'].shape == (4, lags) and g['repeat_period'].shape == (4,)
    assert all(v.dtype == np.float32 for v in g.values())
    period = {1: [1, 1, 0, 0], 2: [2, 2, 0, 0], 16: [2, 2, 0, 0], 64: [2, 2, 0, 64]}[lags]        # row 0: 4 / 60 < 18 / 52; row 3: the tie goes to lag 2
    assert list(g['repeat_period']) == period
    assert g['repeat_profile'][2].sum() == 0 and g['groove_mean'][2] == 0                          # T > 0, I = 0; and T = 0 behind lag 2
    if lags >= 3:
        assert g['repeat_mean'][0] == np.float32(2 * 11 / 158) and g['groove_mean'][0] == np.float32(2 * 14 / 132)
        assert g['repeat_profile'][1, 2] == 0                                                      # a zero divisor gives zero, not nan
    if lags == 1:
        assert g['repeat_mean'][0] == np.float32(4 / 60) and g['repeat_mean'][1] == np.float32(2 / 16)
    want, want_short = R.groups(c, lags)
    assert want_short == short
    for k in g:
        assert np.array_equal(g[k], want[k]), k


def test_structure_groups_on_the_restatements_table_and_refusals():
    from pianobart_amd import structure
    pieces = np.concatenate([R.motif_pieces(D_DEFAULT, 6, 120, seed=41, mb=(1, 2, 3), edit=0.4), M.synth_pieces(D_DEFAULT, 4, 120, seed=42)])
    pieces[2, 1:, 0] = pieces[2, 0, 0]                                                             # one bar only: W = 1
    c = R.structure(pieces, PAD8, PITCH_OF)
    for lags in (1, 7, 64):
        g, short = structure.structure_groups(c, lags)
        want, want_short = R.groups(c, lags)
        assert short == want_short == 1 and all(np.array_equal(g[k], want[k]) for k in g)
    got, want = structure.pooled_profiles(c), R.pooled(c)
    assert np.array_equal(got['groove'], want['groove'], equal_nan=True) and np.array_equal(got['repeat'], want['repeat'], equal_nan=True)
    assert np.array_equal(structure.bar_spans(pieces), c[:, 1]) and np.array_equal(structure.bar_spans(pieces, start=100), R.structure(pieces, PAD8, PITCH_OF, 100)[:, 1])
    for lags in (0, 65, 2.5, True):
        with pytest.raises(PBError, match='lags'):
            structure.structure_groups(c, lags)
    empty, short = structure.structure_groups(c[2:3], 4)
    assert short == 1 and empty['repeat_profile'].shape == (0, 4) and empty['repeat_period'].shape == (0,)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_host_tensors_are_refused():
    from pianobart_amd import structure
    with pytest.raises(PBError, match='no CPU path'):
        ops.piece_structure(torch.zeros(2, 4, 8, dtype=torch.int16), torch.zeros(256, dtype=torch.int16))
    with pytest.raises(PBError, match='no CPU path'):
        structure.piece_structure(torch.zeros(2, 4, 8, dtype=torch.int64))
    with pytest.raises(PBError, match=r'\(N, S, 8\)'):
        structure.piece_structure(np.zeros((2, 4, 7), dtype=np.int64))
    with pytest.raises(PBError, match=r'head 0 \(Bar\)'):
        structure.piece_structure(np.full((1, 4, 8), 262, dtype=np.int64))
    assert ops.STRUCTURE_LAGS == 64 and ops.STRUCTURE_COLS == 264


PTR = 0x10000
_PAD8 = (ctypes.c_int32 * 8)(*ops.DEFAULT_LAYOUT.pad8)
_WIDE_PAD8 = (ctypes.c_int32 * 8)(1100, 128, 129, 256, 128, 32, 254, 49)
_ENTRY_REFUSALS = [
    ((PTR + 2, None, _PAD8, PTR, PTR, 4, 16, 0, None), 'ids16'),
    ((None, None, _PAD8, PTR, PTR, 4, 16, 0, None), 'ids16'),
    ((PTR, PTR + 2, _PAD8, PTR, PTR, 4, 16, 0, None), 'start'),
    ((PTR, None, None, PTR, PTR, 4, 16, 0, None), 'pad8'),
    ((PTR, None, _PAD8, None, PTR, 4, 16, 0, None), 'pitch_of'),
    ((PTR, None, _PAD8, PTR, None, 4, 16, 0, None), 'out'),
    ((PTR, None, _PAD8, PTR, PTR, -1, 16, 0, None), 'N = -1'),
    ((PTR, None, _PAD8, PTR, PTR, 4, 0, 0, None), 'S = 0'),
    ((PTR, None, _PAD8, PTR, PTR, 4, 4097, 0, None), 'S = 4097'),
    ((PTR, None, _PAD8, PTR, PTR, 4, 16, 2, None), 'mode = 2'),
    ((PTR, None, _WIDE_PAD8, PTR, PTR, 4, 16, 0, None), 'pad8[0] = 1100'),
]


@pytest.mark.parametrize('args,names', _ENTRY_REFUSALS, ids=['%d-%s' % (i, n) for i, (_, n) in enumerate(_ENTRY_REFUSALS)])
def test_the_entry_checks_its_arguments_before_any_device_call(args, names):
    with pytest.raises(PBError) as e:
        _lib.LIB.call('pb_piece_structure', *args)
    assert 'pb_piece_structure' in str(e.value) and '(-2)' in str(e.value) and names in str(e.value), str(e.value)


def test_abi_version_is_still_10_and_the_entries_are_exported():
    decls = _lib.parse_header()
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    assert decls['pb_piece_structure'] == (ctypes.c_int, [vp] * 5 + [i32, i32, i32, vp])
    assert decls['pb_structure_lags'] == (ctypes.c_int, []) and decls['pb_structure_cols'] == (ctypes.c_int, [])
    assert _lib.LIB.query('pb_abi_version') == 10
    assert _lib.LIB.query('pb_structure_lags') == ops.STRUCTURE_LAGS and _lib.LIB.query('pb_structure_cols') == ops.STRUCTURE_COLS
    _lib.LIB.call('pb_piece_structure', None, None, _PAD8, PTR, None, 0, 16, 0, None)              # N = 0 is no error (and no launch)


# ---- the CLI ----------------------------------------------------------------------------------------------------------------------------
def _files(tmp_path, gen, ref=None):
    g, r = str(tmp_path / 'g.npy'), str(tmp_path / 'r.npy')
    np.save(g, gen)
    argv = ['--generated', g, '--output', str(tmp_path / 's.json')]
    if ref is not None:
        np.save(r, ref)
        argv += ['--reference', r]
    return argv


def test_cli_refusals(tmp_path):
    from pianobart_amd import eval_structure
    ok = R.motif_pieces(D_DEFAULT, 4, 24, seed=1).astype(np.float32)
    argv = _files(tmp_path, ok, ok)
    with pytest.raises(PBError, match='--cpu'):
        eval_structure.main(argv + ['--cpu'])
    with pytest.raises(PBError, match='--cpu'):
        eval_structure.main(_files(tmp_path, ok) + ['--cpu'])
    with pytest.raises(PBError, match='no file'):
        eval_structure.main(['--generated', str(tmp_path / 'missing.npy')] + argv[2:])
    with pytest.raises(PBError, match='no file'):
        eval_structure.main(argv[:4] + ['--reference', str(tmp_path / 'missing.npy')])
    with pytest.raises(PBError, match='no file'):
        eval_structure.main(argv + ['--dict_file', str(tmp_path / 'missing.json')])
    with pytest.raises(PBError, match='rows of 8 ids'):
        eval_structure.main(_files(tmp_path, ok[:, :, :7], ok))
    with pytest.raises(PBError, match='rows of 8 ids'):
        eval_structure.main(_files(tmp_path, ok[0, 0]))
    with pytest.raises(PBError, match='at most 4096'):
        eval_structure.main(_files(tmp_path, np.zeros((1, 4097, 8), dtype=np.int16)))
    for flags in (['--lags', '0'], ['--lags', '65'], ['--grid', '1'], ['--grid', '5000'], ['--skip', '-1'], ['--max_pieces', '0']):
        with pytest.raises(PBError, match=flags[0]):
            eval_structure.main(argv + flags)
        with pytest.raises(PBError, match=flags[0]):
            eval_structure.main(_files(tmp_path, ok) + flags)
    flat = ok.copy()
    flat[1:, :, 0] = 5                                                     # one piece of two bars or more left
    with pytest.raises(PBError, match=r'--generated holds 1 pieces'):
        eval_structure.main(_files(tmp_path, flat, ok))
    with pytest.raises(PBError, match=r'--reference holds 1 pieces'):
        eval_structure.main(_files(tmp_path, ok, flat))
    with pytest.raises(PBError, match=r'--generated holds 0 pieces'):
        eval_structure.main(_files(tmp_path, ok, ok) + ['--skip', '24'])
    with pytest.raises(PBError, match=r'--generated holds 1 pieces'):
        eval_structure.main(_files(tmp_path, ok, ok) + ['--max_pieces', '1'])
    assert not os.path.exists(str(tmp_path / 's.json'))
