"""GPU: the kernel of csrc/pb_structure.hip and pianobart_amd.structure against the Python-set restatement of tests/structure_ref.py.
Every comparison of the 264 columns is ==, in both modes, and two runs of every case give equal bytes.

  * rows and length: S = 1, L = 0, start = 0 / mid-bar / L - 1 / L / past L, a special id in one head only with note-like rows behind it;
  * bar span: W = 1 with 300 notes, W = 2, W = 64, 65, 66 (the lag cap's three sides), 70 empty bars inside a piece, the last bar id of the
    default dictionary and of the wide one (there with W = 1 024: both ends of the id range in one piece);
  * sets: one note on three instruments, one onset with five pitches, percussion rows, chords (the synthetic pieces of metrics_ref);
  * order: a piece and three row permutations of it give equal bytes;
  * row loop and grid: motif pieces of S = 255, 256, 257, 1 024, 4 096 rows (the kernel's blocks of 64 notes: four with the last one
    short, exactly four, a fifth that holds one note, 16 = one row of tiles per wave, 64 = the most), 4 096 rows of one note, 4 096
    distinct notes in two bars in shuffled row order (no tile can be skipped), 300 pieces of 7 rows (36 pieces per workgroup), 1 025
    pieces of 256 rows (one more than the 1 024 workgroups of the grid cap), N = 0;
  * no hollow pass: on the restatement alone, every motif case of S >= 257 has I_N[l] > 0 on at least half of its reported lags and
    D_N >= 0.5 at the motif's period;
  * compare_structure on 24 motif pieces at edit rate 0.1 against 31 at 0.5: counts, group arrays and pooled profiles ==, distance
    means within (F + 8) 2^-24 relative, kl / oa within KLOA_TOL = four times the measured KLOA_MEASURED; the CLI with and
    without a reference."""
import json
import math

import numpy as np
import pytest
import torch

from tests import metrics_ref as M
from tests import structure_ref as R
from tests.vocab_layout_util import D_DEFAULT, D_WIDE, make_dict

pytestmark = pytest.mark.gpu

KLOA_MEASURED = 1.46e-7       # the kl_gen of repeat_profile; the largest oa error is 2.2e-8
KLOA_TOL = 4 * KLOA_MEASURED
GRID_CAP = 1024               # workgroups of pb_piece_structure (include/pianobart_hip.h)
_CACHE = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


def _terminate(ids, n, L, pad):
    if L < ids.shape[1]:
        ids[n, L] = pad + 3
        ids[n, L + 1:] = pad


def _from_notes(notes, S, pad, seed=0):
    """(S, 8): rows of (bar, position, instrument, pitch id), the other heads random, then an EOS row and a PAD tail."""
    rng = np.random.default_rng(seed)
    rows = np.stack([rng.integers(0, pad[h], size=S) for h in range(8)], axis=1).astype(np.int64)
    for r, (bar, pos, ins, pit) in enumerate(notes):
        rows[r, :4] = [bar, pos, ins, pit]
    if len(notes) < S:
        rows[len(notes)] = pad + 3
        rows[len(notes) + 1:] = pad
    return rows


def _span_piece(W, S, pad, seed, first_bar=0):
    """Two or three notes in every one of W bars, a third of them repeated from the bar before."""
    rng = np.random.default_rng(seed)
    notes, prev = [], []
    for b in range(W):
        cur = [(int(rng.integers(0, 16)) * 4, int(rng.integers(40, 52))) for _ in range(int(rng.integers(2, 4)))]
        if prev and rng.random() < 0.6:
            cur[0] = prev[0]
        notes += [(first_bar + b, p, 0, pit) for p, pit in cur]
        prev = cur
    return _from_notes(notes, S, pad, seed)


def _cases():
    """{name: (sizes, percussion ids, ids, start)}"""
    pad, wpad = np.asarray(D_DEFAULT) - 6, np.asarray(D_WIDE) - 6
    cases = {}
    ids = M.synth_pieces(D_DEFAULT, 3, 1, seed=50)
    ids[1, 0] = pad + 3
    ids[2, 0, 5] = pad[5]
    cases['S1'] = (D_DEFAULT, 128, ids, None)
    S = 65
    ids = np.repeat(R.motif_pieces(D_DEFAULT, 1, S, seed=51), 4, axis=0)
    for n, L in enumerate((0, 1, S - 1, S)):
        _terminate(ids, n, L, pad)
    cases['lengths'] = (D_DEFAULT, 128, ids, None)
    ids = np.repeat(R.motif_pieces(D_DEFAULT, 1, 300, seed=52), 7, axis=0)
    for n in range(7):
        _terminate(ids, n, 280, pad)
    cases['start'] = (D_DEFAULT, 128, ids, np.array([0, 1, 131, 279, 280, 299, 5000], dtype=np.int32))      # 131: the middle of a bar
    ids = np.repeat(R.motif_pieces(D_DEFAULT, 1, 64, seed=53), 8, axis=0)
    for h in range(8):
        ids[h, 20 + h, h] = pad[h] + (h % 6)           # one special id in head h only; the rows behind it look like notes
    cases['one_head_special'] = (D_DEFAULT, 128, ids, None)
    ids = M.synth_pieces(D_DEFAULT, 2, 300, seed=54)
    ids[:, :, 0] = 7
    _terminate(ids, 1, 300, pad)
    cases['W1_300_notes'] = (D_DEFAULT, 128, ids[:1], None)
    cases['W2'] = (D_DEFAULT, 128, np.stack([_span_piece(2, 8, pad, 55), _span_piece(2, 8, pad, 56, first_bar=254)]), None)
    cases['W64_65_66'] = (D_DEFAULT, 128, np.stack([_span_piece(W, 210, pad, 57 + W) for W in (63, 64, 65, 66, 67)]), None)
    a = _span_piece(100, 300, pad, 58)
    a = a[~((a[:, 0] >= 12) & (a[:, 0] < 82) & (a[:, 1] < pad[1]))]                                       # bars 12 .. 81 lose their notes
    cases['gap_of_70_bars'] = (D_DEFAULT, 128, np.stack([np.concatenate([a, np.tile(pad, (300 - len(a), 1))])]), None)
    cases['last_bar_default'] = (D_DEFAULT, 128, np.stack([R.motif_piece(D_DEFAULT, 130, 59, mb=2, edit=0.2, first_bar=236),
                                                           _span_piece(30, 130, pad, 60, first_bar=226)]), None)
    ids = M.synth_pieces(D_WIDE, 3, 130, seed=61, n_perc=0)
    ids[0, :, 0] = np.random.default_rng(61).integers(960, wpad[0], size=130)
    ids[0, 5, 0], ids[0, 6, 3] = wpad[0] - 1, wpad[3] - 1
    ids[1, :, 0] = np.where(np.arange(130) % 2 == 0, np.arange(130) % 6, wpad[0] - 1 - (np.arange(130) - 1) % 6)   # W = 1 024
    ids[2] = R.motif_piece(D_WIDE, 130, 62, mb=3, edit=0.2, first_bar=990)
    cases['wide_dictionary'] = (D_WIDE, 0, ids, None)
    notes = [(3, 0, 0, 60), (3, 0, 1, 60), (3, 0, 2, 60), (4, 0, 0, 60)]
    notes += [(4, 8, 0, 60 + 4 * i) for i in range(5)] + [(5, 8, 1, 60 + 4 * i) for i in (0, 2, 4, 6)] + [(6, 8, 0, 72)]      # one onset, five pitches
    notes += [(b, 16, 128, 130 + b % 2) for b in range(3, 9)] + [(7, 16, 128, 142), (8, 0, 0, 72)]                            # drums; 130 + 12 is no octave
    cases['sets'] = (D_DEFAULT, 128, np.stack([_from_notes(notes, 40, pad, 63), M.synth_pieces(D_DEFAULT, 1, 40, seed=64)[0]]), None)
    one = R.motif_piece(D_DEFAULT, 200, 65, mb=2, edit=0.3)
    rng = np.random.default_rng(65)
    cases['order'] = (D_DEFAULT, 128, np.stack([one] + [one[rng.permutation(200)] for _ in range(3)]), None)
    for S in (255, 256, 257, 1024, 4096):
        cases['motif_S%d' % S] = (D_DEFAULT, 128, np.stack([R.motif_piece(D_DEFAULT, S, 100 + S, mb=2, edit=0.2),
                                                           R.motif_piece(D_DEFAULT, S, 200 + S, mb=1, edit=0.2)]), None)
    ids = np.repeat(M.synth_pieces(D_DEFAULT, 1, 4096, seed=66)[:, :1], 4096, axis=1)
    cases['S4096_one_note'] = (D_DEFAULT, 128, ids, None)
    r = np.arange(4096)
    ids = np.repeat(M.synth_pieces(D_DEFAULT, 1, 4096, seed=67)[:, :1], 4096, axis=1)
    ids[0, :, 0], ids[0, :, 1], ids[0, :, 3] = 100 + r // 2048, r % 128, (r % 2048) // 128 * 7 + r // 2048      # bar 101 holds bar 100's notes one id higher
    ids[0] = ids[0][np.random.default_rng(67).permutation(4096)]
    cases['S4096_distinct_in_two_bars'] = (D_DEFAULT, 128, ids, None)
    cases['sweep_300_pieces_of_7'] = (D_DEFAULT, 128, R.motif_pieces(D_DEFAULT, 300, 7, seed=68, mb=(1, 2), edit=0.3), np.arange(300, dtype=np.int32) % 3)
    ids = np.tile(pad, (GRID_CAP + 1, 256, 1)).astype(np.int64)
    ids[:, :6] = R.motif_pieces(D_DEFAULT, GRID_CAP + 1, 6, seed=69, mb=(1, 2), edit=0.3)
    ids[GRID_CAP, 6:200] = R.motif_piece(D_DEFAULT, 194, 70, mb=2, edit=0.2, first_bar=3)                 # the piece behind the cap is the long one
    cases['one_past_the_grid_cap'] = (D_DEFAULT, 128, ids, None)
    return cases


CASES = _cases()
MOTIF_PERIOD = {'motif_S257': (2, 1), 'motif_S1024': (2, 1), 'motif_S4096': (2, 1)}


def _tables(sizes, n_perc):
    from pianobart_amd import metrics
    key = ('tab', tuple(sizes))
    if key not in _CACHE:
        tab = metrics.tables(None if list(sizes) == D_DEFAULT else make_dict(sizes)[0])
        pad8, pitch_of, _ = M.tables_for(sizes, n_perc)
        assert list(tab.layout.pad8) == pad8 and (tab.pitch_of == pitch_of).all()
        _CACHE[key] = (tab, pad8, pitch_of)
    return _CACHE[key]


def _want(name, mode):
    key = ('want', name, mode)
    if key not in _CACHE:
        sizes, n_perc, ids, start = CASES[name]
        _, pad8, pitch_of = _tables(sizes, n_perc)
        _CACHE[key] = R.structure(ids, pad8, pitch_of, start, mode)
    return _CACHE[key]


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('name', list(CASES))
def test_columns_equal_the_restatement(name, mode):
    _need_gpu()
    from pianobart_amd import structure
    sizes, n_perc, ids, start = CASES[name]
    tab = _tables(sizes, n_perc)[0]
    want = _want(name, mode)
    got = structure.piece_structure(ids, tab, start=start, pitch_class=bool(mode))
    again = structure.piece_structure(ids.astype(np.float32), tab, start=start, pitch_class=bool(mode))      # the float32 that eval_generation writes
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(ids), 264) and got.is_cuda
    got = got.cpu().numpy()
    bad = np.argwhere(got != want)
    assert not len(bad), (name, mode, bad[:8], [(int(got[i, j]), int(want[i, j])) for i, j in bad[:8]])
    assert again.cpu().numpy().tobytes() == got.tobytes()
    if name == 'lengths':
        assert list(got[:, 0]) == [0, 1, 64, 65]
    if name == 'start':
        assert list(got[:, 0]) == [280, 279, 149, 1, 0, 0, 0]
    if name == 'W1_300_notes':
        assert got[0, 0] == 300 and got[0, 1] == 1 and got[0, 8:].sum() == 0 and 0 < got[0, 2] < got[0, 3] < 300
    if name == 'W64_65_66':
        assert list(got[:, 1]) == [63, 64, 65, 66, 67]
        assert [int(got[i, 72 + 63]) > 0 for i in range(5)] == [False, False, True, True, True]          # T_O[64] needs W >= 65
        assert (got[:3, 72 + 62] > 0).tolist() == [False, True, True]
    if name == 'gap_of_70_bars':
        assert got[0, 1] == 100 and got[0, 4] == 30
    if name == 'wide_dictionary':
        assert got[1, 1] == 1024 and got[0, 1] <= 64
    if name == 'order':
        assert got[0].tobytes() == got[1].tobytes() == got[2].tobytes() == got[3].tobytes()
    if name == 'S4096_one_note':
        assert list(got[0, :5]) == [4096, 1, 1, 1, 1]
    if name == 'S4096_distinct_in_two_bars':
        assert list(got[0, :3]) == [4096, 2, 256] and got[0, 4] == 2 and got[0, 8] == 128 and got[0, 72] == 256
        if mode == 0:                                                      # by pitch class the 16 pitches of a bar fall onto 12 classes
            assert got[0, 3] == 4096 and got[0, 136] == 0 and got[0, 200] == 4096


def test_no_hollow_pass():
    """On the restatement alone: the motif cases exercise the lag sums, they do not compare zeros with zeros."""
    for name, periods in MOTIF_PERIOD.items():
        want = _want(name, 0)
        _, repeat = R.lag_profiles(want)
        for n, period in enumerate(periods):
            lags = min(64, int(want[n, 1]) - 1)
            hits = int((want[n, 136:136 + lags] > 0).sum())
            print('%s piece %d: W %d, I_N > 0 on %d of %d lags, D_N[%d] = %.3f' % (name, n, want[n, 1], hits, lags, period, repeat[n, period - 1]))
            assert 2 * hits >= lags and repeat[n, period - 1] >= 0.5


def test_empty_batch():
    _need_gpu()
    from pianobart_amd import ops, structure
    tab = _tables(D_DEFAULT, 128)[0]
    out = structure.piece_structure(np.zeros((0, 16, 8), dtype=np.int64), tab)
    assert tuple(out.shape) == (0, 264) and out.dtype == torch.int32
    with pytest.raises(structure.PBError, match='4096'):
        ops.piece_structure(torch.zeros((1, 4097, 8), dtype=torch.int16, device='cuda'), torch.from_numpy(tab.pitch_of).cuda())


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def _sets():
    if 'sets' not in _CACHE:
        gen = R.motif_pieces(D_DEFAULT, 26, 96, seed=81, mb=(1, 2, 4), edit=0.1)
        ref = R.motif_pieces(D_DEFAULT, 32, 96, seed=82, mb=(1, 2, 4), edit=0.5)
        gen[3, :, 0], gen[11, :, 0], ref[5, :, 0] = 9, 0, 200                  # single-bar pieces: 24 and 31 are left
        _CACHE['sets'] = (gen, ref)
    return _CACHE['sets']


def test_compare_structure_against_the_restatement():
    _need_gpu()
    from pianobart_amd import structure
    gen, ref = _sets()
    _, pad8, pitch_of = _tables(D_DEFAULT, 128)
    res = structure.compare_structure(gen, ref, grid=1024)
    want = R.compare(gen, ref, pad8, pitch_of, lags=16, grid=1024)
    assert (res['n_gen'], res['n_ref'], res['short_gen'], res['short_ref']) == (24, 31, 2, 1)
    for k in ('n_gen', 'n_ref', 'short_gen', 'short_ref'):
        assert res[k] == want[k], k
    assert set(res['device_ms']) == {'structure', 'distances', 'moments', 'kde', 'total'} and res['device_ms']['structure'] > 0
    for tag in ('gen', 'ref'):
        for k in ('groove', 'repeat'):
            assert len(res['profile_' + tag][k]) == 64 and np.array_equal(res['profile_' + tag][k], want['profile_' + tag][k], equal_nan=True), (tag, k)
        assert res['profile_' + tag]['repeat'][1] > 0
    tab = _tables(D_DEFAULT, 128)[0]
    for cols, arrays in zip((structure.piece_structure(gen, tab), structure.piece_structure(ref, tab)), want['group_arrays']):
        g, _ = structure.structure_groups(cols, 16)
        for k in structure.GROUPS:
            assert g[k].dtype == np.float32 and np.array_equal(g[k], arrays[k]), k
    assert list(res['groups']) == list(structure.GROUPS) == list(want['groups'])
    worst = 0.0
    for name, w in want['groups'].items():
        g = res['groups'][name]
        assert set(g) == {'mean_gen', 'std_gen', 'mean_ref', 'std_ref', 'dist_gen', 'dist_ref', 'dist_inter', 'kl', 'oa', 'kl_gen', 'oa_gen'}
        F = 16 if name.endswith('_profile') else 1
        for k in ('mean_gen', 'mean_ref', 'std_gen', 'std_ref'):
            assert abs(g[k] - w[k]) <= 1e-12 * max(1.0, abs(w[k])), (name, k, g[k], w[k])
        for k in ('dist_gen', 'dist_ref', 'dist_inter'):
            assert abs(g[k] - w[k]) <= (F + 8) * 2.0 ** -24 * w[k], (name, k, g[k], w[k])
        assert not math.isnan(w['kl']) and not math.isnan(g['kl']) and not math.isnan(g['kl_gen']), name
        print('compare_structure %-15s kl %.9g (ref %.9g)  oa %.9g (ref %.9g)  kl_gen %.9g (ref %.9g)  oa_gen %.9g (ref %.9g)'
              % (name, g['kl'], w['kl'], g['oa'], w['oa'], g['kl_gen'], w['kl_gen'], g['oa_gen'], w['oa_gen']))
        worst = max([worst] + [abs(g[k] - w[k]) for k in ('kl', 'oa', 'kl_gen', 'oa_gen')])
    print('compare_structure: largest absolute kl / oa error %.4g (KLOA_TOL %.4g)' % (worst, KLOA_TOL))
    assert worst <= KLOA_TOL
    assert res['groups']['repeat_mean']['mean_gen'] > res['groups']['repeat_mean']['mean_ref']             # fewer edits, more repetition
    again = structure.compare_structure(gen, ref, grid=1024)
    assert all(again['groups'][n][k] == v or (math.isnan(v) and math.isnan(again['groups'][n][k])) for n, g in res['groups'].items() for k, v in g.items())


def test_cli(tmp_path, capsys):
    _need_gpu()
    from pianobart_amd import eval_structure, structure
    gen, ref = _sets()
    g4 = gen[:24].reshape(12, 2, 96, 8).astype(np.float32)                 # what eval_generation --samples 2 writes
    gp, rp, out = str(tmp_path / 'g.npy'), str(tmp_path / 'r.npy'), str(tmp_path / 's.json')
    np.save(gp, g4)
    np.save(rp, ref)
    res = eval_structure.main(['--generated', gp, '--reference', rp, '--output', out, '--grid', '128', '--skip', '2', '--max_pieces', '20', '--lags', '8'])
    js = json.load(open(out))
    assert set(js) == {'n_gen', 'n_ref', 'short_gen', 'short_ref', 'device_ms', 'profile_gen', 'profile_ref', 'groups'} and list(js['groups']) == list(structure.GROUPS)
    assert (js['n_gen'], js['short_gen'], js['n_ref'], js['short_ref']) == (18, 2, 19, 1)
    direct = structure.compare_structure(gen[:20], ref[:20], lags=8, grid=128, start=2)
    assert all(js['groups'][n]['oa'] == g['oa'] and res['groups'][n]['kl'] == g['kl'] for n, g in direct['groups'].items())
    assert js['profile_gen']['repeat'][:27] == direct['profile_gen']['repeat'][:27] and js['profile_gen']['repeat'][63] is None
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith('   [structure]')]
    assert len(lines) == 2 * 4 + 5 + 1
    one = eval_structure.main(['--generated', gp, '--output', out, '--pitch_class', '--max_pieces', '20'])
    js = json.load(open(out))
    assert set(js) == {'n', 'short', 'device_ms', 'profile', 'means'} and (js['n'], js['short']) == (18, 2)
    assert set(js['means']) == {'groove_mean', 'repeat_mean', 'repeat_period'} and js['means'] == dict(one['means'])
    by_class = structure.pooled_profiles(structure.piece_structure(gen[:20], pitch_class=True))
    assert js['profile']['repeat'][:16] == by_class['repeat'][:16] and 0 < js['profile']['repeat'][1] <= js['profile']['groove'][1] <= 1
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith('   [structure]')]
    assert len(lines) == 4 + 1
