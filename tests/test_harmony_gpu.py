"""GPU: the kernel of csrc/pb_harmony.hip and pianobart_amd.harmony against the restatement of tests/harmony_ref.py. Every comparison of
the 228 columns is ==, and two runs of every case give equal bytes.

  * rows and length: S = 1, L = 0, 1, S - 1, S, start = 0 / mid-bar / L - 1 / L / past S, a special id in one head only with note-like
    rows behind it;
  * bar span: W = 1, 3, 4, 5 (the three sides of the window of 4 bars), W = 63 .. 67 (the lag cap), 70 empty bars inside a piece, the last
    bar id of the default dictionary and of the wide one (there with W = 1 024: both ends of the id range in one piece);
  * notes: percussion only, percussion mixed in (the synthetic pieces of metrics_ref), 4 096 rows of one class in one bar (TL[4096], a
    16-bit count at its largest), 4 096 rows over two bars, a motif that rises two semitones with every copy;
  * order: a piece and three row permutations of it give equal bytes;
  * row loop and grid: motif pieces of S = 255, 256, 257, 1 024 and 4 096 rows, of 512 and 513 rows (the last S with workgroups of 4 waves
    and the first with 16), 300 pieces of 7 rows (36 pieces per workgroup), 1 025 pieces of 256 rows (one more than the 1 024 workgroups
    of the grid cap), N = 0;
  * columns 0 and 1 equal those of pb_piece_structure on the same input;
  * no hollow pass: on the restatement alone, the two-bar motif pieces have D_H of 0.75 .. 0.80 at every multiple of the motif's period
    (above 0.75 at 4 096 rows, where 16 voices lie over the same bars) and below 0.05 at every other lag, and I_X > I_H on the transposing
    piece;
  * compare_harmony on 24 motif pieces at edit rate 0.1 against 31 at 0.5: counts, group arrays and pooled profiles ==, distance means
    within (F + 8) 2^-24 relative, kl / oa within KLOA_TOL = four times the measured KLOA_MEASURED; the CLI with and without
    a reference."""
import json
import math

import numpy as np
import pytest
import torch

from tests import harmony_ref as R
from tests import metrics_ref as M
from tests import structure_ref as SR
from tests.vocab_layout_util import D_DEFAULT, D_WIDE, make_dict

pytestmark = pytest.mark.gpu

KLOA_MEASURED = 2.44e-7       # the kl of sequence_profile (5.27); the largest oa error is 2.0e-8
KLOA_TOL = 4 * KLOA_MEASURED
GRID_CAP = 1024               # workgroups of pb_piece_harmony (include/pianobart_hip.h)
MOTIF_SEED = {255: 773, 256: 448, 257: 1252, 1024: 1445, 4096: 4209}      # two-bar motifs whose two bars share no pitch class
_CACHE = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


def _terminate(ids, n, L, pad):
    if L < ids.shape[1]:
        ids[n, L] = pad + 3
        ids[n, L + 1:] = pad


def _from_notes(notes, S, pad, seed=0):
    """(S, 8): rows of (bar, pitch id), the other heads random, then an EOS row and a PAD tail."""
    rng = np.random.default_rng(seed)
    rows = np.stack([rng.integers(0, pad[h], size=S) for h in range(8)], axis=1).astype(np.int64)
    for r, (bar, pit) in enumerate(notes):
        rows[r, 0], rows[r, 3] = bar, pit
    if len(notes) < S:
        rows[len(notes)] = pad + 3
        rows[len(notes) + 1:] = pad
    return rows


def _span_piece(W, S, pad, seed, first_bar=0):
    """Two to four notes in every one of W bars from a scale that moves now and then, one of them often repeated from the bar before."""
    rng = np.random.default_rng(seed)
    notes, prev, root = [], [], int(rng.integers(0, 12))
    for b in range(W):
        if rng.random() < 0.2:
            root = (root + int(rng.choice([5, 7, 2]))) % 12
        cur = [36 + root + int(rng.choice(R.MAJOR)) + 12 * int(rng.integers(0, 3)) for _ in range(int(rng.integers(2, 5)))]
        if prev and rng.random() < 0.6:
            cur[0] = prev[0]
        notes += [(first_bar + b, pit) for pit in cur]
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
    ids = np.repeat(SR.motif_pieces(D_DEFAULT, 1, S, seed=51), 4, axis=0)
    for n, L in enumerate((0, 1, S - 1, S)):
        _terminate(ids, n, L, pad)
    cases['lengths'] = (D_DEFAULT, 128, ids, None)
    ids = np.repeat(SR.motif_pieces(D_DEFAULT, 1, 300, seed=52), 7, axis=0)
    for n in range(7):
        _terminate(ids, n, 280, pad)
    cases['start'] = (D_DEFAULT, 128, ids, np.array([0, 1, 131, 279, 280, 299, 5000], dtype=np.int32))      # 131: the middle of a bar
    ids = np.repeat(SR.motif_pieces(D_DEFAULT, 1, 64, seed=53), 8, axis=0)
    for h in range(8):
        ids[h, 20 + h, h] = pad[h] + (h % 6)           # one special id in head h only; the rows behind it look like notes
    cases['one_head_special'] = (D_DEFAULT, 128, ids, None)
    cases['W1_3_4_5'] = (D_DEFAULT, 128, np.stack([_span_piece(W, 24, pad, 54 + W, first_bar=3 * W) for W in (1, 3, 4, 5)]), None)
    cases['W63_to_67'] = (D_DEFAULT, 128, np.stack([_span_piece(W, 280, pad, 57 + W) for W in (63, 64, 65, 66, 67)]), None)
    a = _span_piece(100, 400, pad, 58)
    a = a[~((a[:, 0] >= 12) & (a[:, 0] < 82) & (a[:, 1] < pad[1]))]                                       # bars 12 .. 81 lose their notes
    cases['gap_of_70_bars'] = (D_DEFAULT, 128, np.stack([np.concatenate([a, np.tile(pad, (400 - len(a), 1))])]), None)
    cases['last_bar_default'] = (D_DEFAULT, 128, np.stack([SR.motif_piece(D_DEFAULT, 130, 59, mb=2, edit=0.2, first_bar=236),
                                                           _span_piece(30, 130, pad, 60, first_bar=226)]), None)
    ids = M.synth_pieces(D_WIDE, 3, 130, seed=61, n_perc=0)
    ids[0, :, 0] = np.random.default_rng(61).integers(960, wpad[0], size=130)
    ids[0, 5, 0], ids[0, 6, 3] = wpad[0] - 1, wpad[3] - 1
    ids[1, :, 0] = np.where(np.arange(130) % 2 == 0, np.arange(130) % 6, wpad[0] - 1 - (np.arange(130) - 1) % 6)   # W = 1 024
    ids[2] = SR.motif_piece(D_WIDE, 130, 62, mb=3, edit=0.2, first_bar=990)
    cases['wide_dictionary'] = (D_WIDE, 0, ids, None)
    ids = M.synth_pieces(D_DEFAULT, 2, 120, seed=63)
    ids[:, :, 3] = np.where(ids[:, :, 3] < pad[3], 128 + ids[:, :, 3] % 128, ids[:, :, 3])
    cases['percussion_only'] = (D_DEFAULT, 128, ids, None)
    cases['percussion_mixed_in'] = (D_DEFAULT, 128, M.synth_pieces(D_DEFAULT, 4, 150, seed=64), None)
    ids = np.repeat(M.synth_pieces(D_DEFAULT, 1, 4096, seed=66)[:, :1], 4096, axis=1)
    ids[0, :, 0], ids[0, :, 3] = 7, 36 + 12 * (np.arange(4096) % 5)
    cases['S4096_one_class_one_bar'] = (D_DEFAULT, 128, ids, None)
    r = np.arange(4096)
    ids = np.repeat(M.synth_pieces(D_DEFAULT, 1, 4096, seed=67)[:, :1], 4096, axis=1)
    ids[0, :, 0], ids[0, :, 3] = 100 + (r % 3 == 0), 30 + (r * 7) % 90 + (r % 3 == 0)                        # a third of the rows in the second bar
    ids[0] = ids[0][np.random.default_rng(67).permutation(4096)]
    cases['S4096_two_bars'] = (D_DEFAULT, 128, ids, None)
    seq = R.sequence_piece(D_DEFAULT, 40, step=2, first_bar=5)
    cases['transposing_motif'] = (D_DEFAULT, 128, np.stack([seq, R.sequence_piece(D_DEFAULT, 40, step=1, first_bar=0, low=30)]), None)
    one = SR.motif_piece(D_DEFAULT, 200, 65, mb=2, edit=0.3)
    one[::9, 3] = 130 + np.arange(len(one[::9])) % 7                                                         # some percussion
    rng = np.random.default_rng(65)
    cases['order'] = (D_DEFAULT, 128, np.stack([one] + [one[rng.permutation(200)] for _ in range(3)]), None)
    for S in (255, 256, 257, 1024, 4096):
        cases['motif_S%d' % S] = (D_DEFAULT, 128, np.stack([SR.motif_piece(D_DEFAULT, S, MOTIF_SEED[S], mb=2, edit=0.2),
                                                           SR.motif_piece(D_DEFAULT, S, 200 + S, mb=1, edit=0.2)]), None)
    for S in (512, 513):                                                   # the two sides of the workgroup size: 4 waves up to 512 rows, 16 above
        cases['workgroup_S%d' % S] = (D_DEFAULT, 128, SR.motif_pieces(D_DEFAULT, 5, S, seed=300 + S, mb=(1, 2, 4), edit=0.2), None)
    cases['sweep_300_pieces_of_7'] = (D_DEFAULT, 128, SR.motif_pieces(D_DEFAULT, 300, 7, seed=68, mb=(1, 2), edit=0.3), np.arange(300, dtype=np.int32) % 3)
    ids = np.tile(pad, (GRID_CAP + 1, 256, 1)).astype(np.int64)
    ids[:, :6] = SR.motif_pieces(D_DEFAULT, GRID_CAP + 1, 6, seed=69, mb=(1, 2), edit=0.3)
    ids[GRID_CAP, 6:200] = SR.motif_piece(D_DEFAULT, 194, 70, mb=2, edit=0.2, first_bar=3)                 # the piece behind the cap is the long one
    cases['one_past_the_grid_cap'] = (D_DEFAULT, 128, ids, None)
    return cases


CASES = _cases()


def _tables(sizes, n_perc):
    from pianobart_amd import metrics
    key = ('tab', tuple(sizes))
    if key not in _CACHE:
        tab = metrics.tables(None if list(sizes) == D_DEFAULT else make_dict(sizes)[0])
        pad8, pitch_of, _ = M.tables_for(sizes, n_perc)
        assert list(tab.layout.pad8) == pad8 and (tab.pitch_of == pitch_of).all()
        _CACHE[key] = (tab, pad8, pitch_of)
    return _CACHE[key]


def _want(name):
    key = ('want', name)
    if key not in _CACHE:
        sizes, n_perc, ids, start = CASES[name]
        pad8, pitch_of, _ = M.tables_for(sizes, n_perc)
        _CACHE[key] = R.harmony(ids, pad8, pitch_of, start)
    return _CACHE[key]


@pytest.mark.parametrize('name', list(CASES))
def test_columns_equal_the_restatement(name):
    _need_gpu()
    from pianobart_amd import harmony, structure
    sizes, n_perc, ids, start = CASES[name]
    tab = _tables(sizes, n_perc)[0]
    want = _want(name)
    got = harmony.piece_harmony(ids, tab, start=start)
    again = harmony.piece_harmony(ids.astype(np.float32), tab, start=start)                # the float32 that eval_generation writes
    assert got.dtype == torch.int64 and tuple(got.shape) == (len(ids), 228) and got.is_cuda
    got = got.cpu().numpy()
    bad = np.argwhere(got != want)
    assert not len(bad), (name, bad[:8], [(int(got[i, j]), int(want[i, j])) for i, j in bad[:8]])
    assert again.cpu().numpy().tobytes() == got.tobytes()
    st = structure.piece_structure(ids, tab, start=start).cpu().numpy()
    assert np.array_equal(st[:, :2], got[:, :2])                                           # notes and W: the same rows, the same bars
    TL = R.table()[0]
    if name == 'S1':
        assert list(got[:, 0]) == [1, 0, 0]
    if name == 'lengths':
        assert list(got[:, 0]) == [0, 1, 64, 65]
    if name == 'start':
        assert list(got[:, 0]) == [280, 279, 149, 1, 0, 0, 0]
    if name == 'W1_3_4_5':
        assert list(got[:, 1]) == [1, 3, 4, 5] and list(got[:, 20]) == [1, 3, 4, 5] and list(got[:, 28]) == [0, 0, 1, 2]
        assert list(got[:, 100 + 2] > 0) == [False, False, True, True] and got[0, 36:].sum() == 0
    if name == 'W63_to_67':
        assert list(got[:, 1]) == [63, 64, 65, 66, 67]
        assert [int(got[i, 100 + 63]) > 0 for i in range(5)] == [False, False, True, True, True]             # T_H[64] needs W >= 65
        assert (got[:3, 100 + 62] > 0).tolist() == [False, True, True]
    if name == 'gap_of_70_bars':
        assert got[0, 1] == 100 and got[0, 4] == 30 and got[0, 28] == 97 and got[0, 29] < 97 - 60
    if name == 'wide_dictionary':
        assert got[1, 1] == 1024 and got[0, 1] <= 64
    if name == 'percussion_only':
        assert (got[:, 2] == 0).all() and (got[:, 3] == got[:, 0]).all() and (got[:, 1] > 1).all() and got[:, 4:20].sum() == 0 and got[:, 21:28].sum() == 0
        assert got[:, 36:].sum() == 0
    if name == 'percussion_mixed_in':
        assert (got[:, 3] > 0).all() and (got[:, 2] > got[:, 3]).all()
    if name == 'order':
        assert got[0].tobytes() == got[1].tobytes() == got[2].tobytes() == got[3].tobytes() and got[0, 3] == 23
    if name == 'S4096_one_class_one_bar':
        assert list(got[0, :8]) == [4096, 1, 4096, 0, 1, 0, 4096, 0] and got[0, 8] == 4096
        assert list(got[0, 20:28]) == [1, 1, 4096, TL[4096] - TL[4096], 4096, 1, 0, 1] and got[0, 28:].sum() == 0
    if name == 'S4096_two_bars':
        assert list(got[0, :5]) == [4096, 2, 4096, 0, 2] and got[0, 100] == 4096 and 0 < got[0, 36] < got[0, 164] <= 1366 and got[0, 23] > TL[1000]
    if name == 'transposing_motif':
        assert (got[:, 164 + 1] * 2 == got[:, 100 + 1]).all() and got[0, 36 + 1] == 0           # lag 2: the same bar, transposed


def test_no_hollow_pass():
    """On the restatement alone: the motif cases exercise the lag sums, they do not compare zeros with zeros, and the transposing case
    separates I_X from I_H."""
    for S in (255, 256, 257, 1024, 4096):
        want = _want('motif_S%d' % S)
        h, _ = R.profiles(want)
        lags = min(64, int(want[0, 1]) - 1)
        on, off = h[0, 1:lags:2], h[0, 0:lags:2]                                # the two-bar motif: lags 2, 4, .. and lags 1, 3, ..
        print('motif_S%d: W %d, D_H at the even lags %.3f .. %.3f, at the odd lags at most %.3f; one-bar motif %.3f .. %.3f'
              % (S, want[0, 1], on.min(), on.max(), off.max(), h[1, :lags].min(), h[1, :lags].max()))
        assert lags == 64 and on.min() >= 0.75 and off.max() < 0.05 and (on.max() <= 0.80 or S == 4096)
        assert h[1, :64].min() >= 0.5
    want = _want('transposing_motif')
    assert (want[:, 164:228] >= want[:, 36:100]).all() and (want[:, 164:164 + 11] > want[:, 36:36 + 11]).all()      # lag 12 of piece 0 is an octave: equal there
    assert want[0, 164 + 11] == want[0, 36 + 11] > 0


def test_empty_batch():
    _need_gpu()
    from pianobart_amd import harmony, ops
    tab = _tables(D_DEFAULT, 128)[0]
    out = harmony.piece_harmony(np.zeros((0, 16, 8), dtype=np.int64), tab)
    assert tuple(out.shape) == (0, 228) and out.dtype == torch.int64
    pitch_of = torch.from_numpy(tab.pitch_of).cuda()
    with pytest.raises(harmony.PBError, match='4096'):
        ops.piece_harmony(torch.zeros((1, 4097, 8), dtype=torch.int16, device='cuda'), pitch_of)
    with pytest.raises(harmony.PBError, match='table'):
        ops.piece_harmony(torch.zeros((1, 4, 8), dtype=torch.int16, device='cuda'), pitch_of, table=ops.harmony_table('cuda')[:4096].contiguous())
    assert ops.harmony_table('cuda').cpu().tolist() == R.table()[0]


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def _sets():
    if 'sets' not in _CACHE:
        gen = SR.motif_pieces(D_DEFAULT, 26, 96, seed=81, mb=(1, 2, 4), edit=0.1)
        ref = SR.motif_pieces(D_DEFAULT, 32, 96, seed=82, mb=(1, 2, 4), edit=0.5)
        gen[3, :, 0], gen[11, :, 3], ref[5, :, 0] = 9, 200, 200                # a single-bar piece, a percussion piece: 24 and 31 are left
        _CACHE['sets'] = (gen, ref)
    return _CACHE['sets']


def test_compare_harmony_against_the_restatement():
    _need_gpu()
    from pianobart_amd import harmony
    gen, ref = _sets()
    _, pad8, pitch_of = _tables(D_DEFAULT, 128)
    res = harmony.compare_harmony(gen, ref, grid=1024)
    want = R.compare(gen, ref, pad8, pitch_of, lags=16, grid=1024)
    assert (res['n_gen'], res['n_ref'], res['short_gen'], res['short_ref']) == (24, 31, 2, 1)
    for k in ('n_gen', 'n_ref', 'short_gen', 'short_ref'):
        assert res[k] == want[k], k
    assert set(res['device_ms']) == {'harmony', 'distances', 'moments', 'kde', 'total'} and res['device_ms']['harmony'] > 0
    for tag in ('gen', 'ref'):
        for k in ('harmony', 'sequence'):
            assert len(res['profile_' + tag][k]) == 64 and np.array_equal(res['profile_' + tag][k], want['profile_' + tag][k], equal_nan=True), (tag, k)
        assert res['profile_' + tag]['sequence'][1] >= res['profile_' + tag]['harmony'][1] > 0
    tab = _tables(D_DEFAULT, 128)[0]
    for cols, arrays in zip((harmony.piece_harmony(gen, tab), harmony.piece_harmony(ref, tab)), want['group_arrays']):
        g, _ = harmony.harmony_groups(cols, 16)
        for k in harmony.GROUPS:
            assert g[k].dtype == np.float32 and np.array_equal(g[k], arrays[k]), k
    assert list(res['groups']) == list(harmony.GROUPS) == list(want['groups'])
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
        print('compare_harmony %-17s kl %.9g (ref %.9g)  oa %.9g (ref %.9g)  kl_gen %.9g (ref %.9g)  oa_gen %.9g (ref %.9g)'
              % (name, g['kl'], w['kl'], g['oa'], w['oa'], g['kl_gen'], w['kl_gen'], g['oa_gen'], w['oa_gen']))
        worst = max([worst] + [abs(g[k] - w[k]) for k in ('kl', 'oa', 'kl_gen', 'oa_gen')])
    print('compare_harmony: largest absolute kl / oa error %.4g (KLOA_TOL %.4g)' % (worst, KLOA_TOL))
    assert worst <= KLOA_TOL
    assert res['groups']['harmony_mean']['mean_gen'] > res['groups']['harmony_mean']['mean_ref']             # fewer edits, more repetition
    again = harmony.compare_harmony(gen, ref, grid=1024)
    assert all(again['groups'][n][k] == v or (math.isnan(v) and math.isnan(again['groups'][n][k])) for n, g in res['groups'].items() for k, v in g.items())


def test_cli(tmp_path, capsys):
    _need_gpu()
    from pianobart_amd import eval_harmony, harmony
    gen, ref = _sets()
    g4 = gen[:24].reshape(12, 2, 96, 8).astype(np.float32)                 # what eval_generation --samples 2 writes
    gp, rp, out = str(tmp_path / 'g.npy'), str(tmp_path / 'r.npy'), str(tmp_path / 'h.json')
    np.save(gp, g4)
    np.save(rp, ref)
    res = eval_harmony.main(['--generated', gp, '--reference', rp, '--output', out, '--grid', '128', '--skip', '2', '--max_pieces', '20', '--lags', '8'])
    js = json.load(open(out))
    assert set(js) == {'n_gen', 'n_ref', 'short_gen', 'short_ref', 'device_ms', 'profile_gen', 'profile_ref', 'groups'} and list(js['groups']) == list(harmony.GROUPS)
    assert (js['n_gen'], js['short_gen'], js['n_ref'], js['short_ref']) == (18, 2, 19, 1)
    direct = harmony.compare_harmony(gen[:20], ref[:20], lags=8, grid=128, start=2)
    assert all(js['groups'][n]['oa'] == g['oa'] and res['groups'][n]['kl'] == g['kl'] for n, g in direct['groups'].items())
    assert js['profile_gen']['harmony'][:27] == direct['profile_gen']['harmony'][:27] and js['profile_gen']['harmony'][63] is None
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith('   [harmony]')]
    assert len(lines) == 2 * 5 + 12 + 1
    one = eval_harmony.main(['--generated', gp, '--output', out, '--max_pieces', '20'])
    js = json.load(open(out))
    assert set(js) == {'n', 'short', 'device_ms', 'profile', 'means'} and (js['n'], js['short']) == (18, 2)
    assert set(js['means']) == set(harmony.SCALAR_GROUPS) and js['means'] == dict(one['means'])
    pooled = harmony.pooled_profiles(harmony.piece_harmony(gen[:20]))
    assert js['profile']['harmony'][:16] == pooled['harmony'][:16] and 0 < js['profile']['harmony'][1] <= js['profile']['sequence'][1] <= 1
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith('   [harmony]')]
    assert len(lines) == 5 + 1
