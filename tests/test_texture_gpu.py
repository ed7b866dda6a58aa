"""GPU: the kernel of csrc/pb_texture.hip and pianobart_amd.texture against the restatement of tests/texture_ref.py. Every comparison of
the 64 columns is ==, two runs of every case give equal bytes, and so does every case with the note rows of each piece permuted.

  * rows and length: S = 1, 7, 255, 256, 257, 512, 513 (the last S with workgroups of 4 waves and the first with 16), 1 024, 4 096, each
    with L = 0, 1, S - 1, S; a special id in one head only with note-like rows behind it;
  * pitched notes on both sides of every sort size: P = 1, 2, 3, 63, 64, 65, 1 023, 1 024, 1 025, 4 095, 4 096, with percussion rows
    interleaved (runs of 300 among them) that carry time signatures of their own;
  * time: bars of 3/4, 4/4, 1/64 and 2/1 in one piece, empty bars behind the first bar, between the others and in runs of 48, 68, 100 and
    496, b_lo = 200, the last bar id of the default dictionary (255) and of the wide one (1 023, there with W = 1 024 bars of 2/1: the
    largest time), bar ids out of row order, two time signatures at the first position of a bar, positions behind the end of the bar;
  * durations and overlaps: duration id 0 (one step) and the largest (3 952), touching notes of one pitch, an overlap of one step, short
    notes nested in a long one, 100 notes on one (pitch, onset), 100 pitches on one onset, one note alone, inter-onset gaps of 1,
    2^k - 1, 2^k and 2^15;
  * start as one value and per piece (0, inside, L - 1, L, past S), 1 028 pieces of 7 rows (more pieces than the 1 024 workgroups), N = 0;
  * no hollow pass: every one of the 58 defined columns is non-zero in some case and differs between two rows;
  * notes, P and W equal those of pb_piece_structure and pb_piece_features on the same arrays;
  * compare_texture on 24 against 31 pieces: counts, group arrays and pooled profiles ==, means and stds to 1e-12, distance means within
    (F + 8) 2^-24 relative, kl / oa within KLOA_TOL = four times the measured KLOA_MEASURED; the CLI with and without a
    reference."""
import json
import math

import numpy as np
import pytest
import torch

from tests import metrics_ref as M
from tests import texture_ref as R
from tests.vocab_layout_util import D_DEFAULT, D_WIDE, SPECIALS, make_dict

pytestmark = pytest.mark.gpu

KLOA_MEASURED = 4.23e-8       # 4.221e-8 measured: the kl of tie_rate (0.564); the largest oa error is 1.4e-8
KLOA_TOL = 4 * KLOA_MEASURED
GRID_CAP = 1024               # workgroups of pb_piece_texture (include/pianobart_hip.h)
DEFINED = list(range(15)) + list(range(16, 58))
SIZES = {'default': D_DEFAULT, 'wide': D_WIDE}
_CACHE = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


def _with_percussion(pitched, runs, singles, seed, bars):
    """The pitched rows with percussion rows between them: `runs` runs of 300 and `singles` single rows, each with a time signature of its
    own choice, so that percussion rows take part in the time axis."""
    rng = np.random.default_rng(seed)
    perc = lambda: (int(rng.integers(0, bars)), int(rng.integers(0, 40)), 128 + int(rng.integers(0, 128)), int(rng.integers(0, 60)),
                    int(rng.choice([R.TS_44, R.TS_34, R.TS_68])))
    out = list(pitched)
    for _ in range(singles):
        out.insert(int(rng.integers(0, len(out) + 1)), perc())
    for _ in range(runs):
        at = int(rng.integers(0, len(out) + 1))
        out[at:at] = [perc() for _ in range(300)]
    return out


def _gap_onsets():
    gaps = [1]
    for k in range(1, 14):
        gaps += [2 ** k - 1, 2 ** k]
    gaps += [2 ** 14 - 1, 2 ** 14, 2 ** 15]
    times = [0]
    for g in gaps:
        times.append(times[-1] + g)
    assert times[-1] < 1023 * 128
    return gaps, times


def _cases():
    """{name: (dictionary, ids, start)}"""
    pad, wpad = np.asarray(D_DEFAULT) - 6, np.asarray(D_WIDE) - 6
    cases = {}
    for S in (1, 7, 255, 256, 257, 512, 513, 1024, 4096):
        notes = R.piano_notes(S, 100 + S)
        cases['rows_S%d' % S] = ('default', np.stack([R.from_notes(notes, S, pad, L) for L in (0, 1, S - 1, S)]), None)
    ids = np.repeat(R.from_notes(R.piano_notes(64, 7), 64, pad)[None], 8, axis=0)
    for h in range(8):
        ids[h, 20 + h, h] = pad[h] + (h % 6)               # one special id in head h only; the rows behind it look like notes
    cases['one_head_special'] = ('default', ids, None)
    for S, Ps, runs in ((1024, (1, 2, 3, 63, 64, 65), 1), (2048, (1023, 1024, 1025), 2)):
        cases['pitched_%s' % '_'.join(map(str, Ps))] = ('default', np.stack([
            R.from_notes(_with_percussion(R.piano_notes(P, 200 + P, n_perc_ids=0, bars=40), runs, 50, 300 + P, 40), S, pad) for P in Ps]), None)
    cases['pitched_4095_4096'] = ('default', np.stack([
        R.from_notes(_with_percussion(R.piano_notes(4095, 210, n_perc_ids=0), 0, 1, 310, 200), 4096, pad),
        R.from_notes(R.piano_notes(4096, 211, n_perc_ids=0, first_bar=56), 4096, pad)]), None)

    a = [(200, 0, 60, 20, R.TS_44), (200, 32, 64, 30, R.TS_44), (204, 0, 62, 16, R.TS_34), (204, 0, 65, 16, R.TS_44), (204, 30, 60, 40, R.TS_21),
         (205, 0, 60, 0, R.TS_164), (205, 5, 67, 3, R.TS_164), (206, 127, 70, 127, R.TS_21), (206, 0, 60, 50, R.TS_21), (255, 10, 60, 8, R.TS_44),
         (255, 70, 72, 127, R.TS_44), (204, 50, 61, 2, R.TS_34)]
    b = [(0, 0, 60, 16, R.TS_34), (0, 47, 64, 4, R.TS_34), (1, 63, 60, 4, R.TS_44), (102, 0, 62, 0, R.TS_164), (102, 3, 130, 0, R.TS_44),
         (171, 100, 65, 60, R.TS_21), (180, 0, 60, 127, R.TS_44), (180, 0, 200, 5, R.TS_34)]
    rng = np.random.default_rng(3)
    cases['time_default'] = ('default', np.stack([R.from_notes([a[i] for i in rng.permutation(len(a))], 64, pad),
                                                  R.from_notes([b[i] for i in rng.permutation(len(b))], 64, pad)]), None)
    a = [(0, 100, 60, 20, R.TS_21), (3, 0, 64, 0, R.TS_164), (3, 2, 65, 1, R.TS_164), (500, 0, 60, 40, R.TS_164), (1023, 60, 400, 290, R.TS_44),
         (1023, 0, 511, 3, R.TS_44)]
    b = [(0, 0, 60, 127, R.TS_21), (1023, 127, 61, 293, R.TS_21), (1023, 127, 60, 0, R.TS_21), (512, 64, 60, 100, R.TS_21)]
    c = [(1023 - int(v), int(p), 300 + int(v) % 7, int(d), R.TS_68) for v, p, d in zip(rng.permutation(124)[:60], rng.integers(0, 60, 60), rng.integers(0, 90, 60))]
    cases['time_wide'] = ('wide', np.stack([R.from_notes(a, 64, wpad), R.from_notes(b, 64, wpad), R.from_notes(c, 64, wpad)]), None)

    edges = [[(0, 0, 60, 16, R.TS_44), (0, 16, 60, 16, R.TS_44), (0, 32, 60, 16, R.TS_44)],                       # touching
             [(0, 0, 60, 17, R.TS_44), (0, 17, 60, 16, R.TS_44)],                                                 # an overlap of one step
             [(0, 0, 60, 36, R.TS_44), (0, 4, 60, 2, R.TS_44), (0, 9, 60, 2, R.TS_44), (0, 9, 60, 3, R.TS_44)],   # nested
             [(1, 8, 60, 3, R.TS_44)] * 100,                                                                      # one (pitch, onset)
             [(0, 0, i, 8, R.TS_44) for i in range(100)],                                                         # 100 pitches on one onset
             [(9, 9, 60, 9, R.TS_44)],                                                                            # one note
             [(0, 0, 60, 0, R.TS_44), (0, 1, 60, 127, R.TS_44), (0, 2, 61, 0, R.TS_44)]]                          # duration ids 0 and 127
    cases['edges'] = ('default', np.stack([R.from_notes(e, 128, pad) for e in edges]), None)
    _, times = _gap_onsets()
    cases['gaps'] = ('wide', np.stack([R.from_notes([(t // 128, t % 128, 60 + i % 3, 2, R.TS_21) for i, t in enumerate(times)], 64, wpad)]), None)

    notes = R.piano_notes(90, 8)
    ids = np.repeat(R.from_notes(notes, 100, pad)[None], 5, axis=0)
    cases['start_one_value'] = ('default', ids, 37)
    cases['start_per_piece'] = ('default', ids, np.array([0, 41, 89, 90, 5000], dtype=np.int32))
    N = GRID_CAP + 4
    cases['sweep_1028_pieces_of_7'] = ('default', np.stack([R.from_notes(R.piano_notes(7, 1000 + n, bars=3), 7, pad, n % 8) for n in range(N)]), None)
    return cases


CASES = _cases()


def _tables(which):
    """(the module's tables, pad8, pitch_of, dur_pos, bar_pos of the restatement)"""
    from pianobart_amd import pieces
    if which not in _CACHE:
        sizes = SIZES[which]
        e2w = None
        if which == 'wide':                                                                  # make_dict's sizes with real time-signature words
            e2w = make_dict(sizes)[0]
            e2w['TimeSig'] = {w: i for i, w in enumerate(R.ts_words() + ['TimeSig <%s>' % s for s in SPECIALS])}
        tab = pieces.tables(e2w)
        pad8, pitch_of, dur_pos = M.tables_for(sizes, 128 if which == 'default' else 0)
        bar_pos = R.bar_pos_default()
        assert list(tab.layout.pad8) == pad8 and (tab.pitch_of == pitch_of).all() and (tab.dur_pos == dur_pos).all() and (tab.bar_pos == bar_pos).all()
        _CACHE[which] = (tab, pad8, pitch_of, dur_pos, bar_pos)
    return _CACHE[which]


def _want(name):
    key = ('want', name)
    if key not in _CACHE:
        which, ids, start = CASES[name]
        _CACHE[key] = R.texture(ids, *_tables(which)[1:], start=start)
    return _CACHE[key]


def _permuted(ids, pad8, start, seed):
    """Every piece with its note rows (the rows from start up to its first special row) in another order."""
    rng = np.random.default_rng(seed)
    out = ids.copy()
    first = np.zeros(len(ids), dtype=np.int64) if start is None else np.broadcast_to(np.asarray(start), (len(ids),))
    for n in range(len(ids)):
        lo, L = int(first[n]), M.length(ids[n], pad8)
        if lo < L:
            out[n, lo:L] = ids[n, lo + rng.permutation(L - lo)]
    return out


def _check_case(name, got, S):
    """What a case is there for, read off its columns."""
    if name.startswith('rows_S'):
        assert list(got[:, 0]) == [0, 1, S - 1, S]
    if name == 'one_head_special':
        assert list(got[:, 0]) == list(range(20, 28))
    if name.startswith('pitched_'):
        assert list(got[:, 1]) == [int(p) for p in name.split('_')[1:]] and (got[:, 0] > got[:, 1])[:-1].all()
    if name == 'time_default':
        # bars 200 (64), 201 - 203 (64 each), 204 (3/4 by the smaller id: 48), 205 (1), 206 (128), 207 - 254 (128 each), 255 (64)
        assert got[0, 2] == 56 and got[0, 3] == 4 * 64 + 48 + 1 + 49 * 128 + 70 + 3952 and got[0, 13] == 3 and got[0, 12] >= 3
        assert got[1, 2] == 181 and got[1, 3] == 48 + 101 * 64 + 69 * 1 + 9 * 128 + 3952 and got[1, 13] == 0
    if name == 'time_wide':
        assert list(got[:2, 2]) == [1024, 1024] and 100 < got[2, 2] <= 124
        assert got[1, 3] == 1023 * 128 + 127 + 3952 and got[0, 3] == 3 * 128 + 1020 + 60 + 3952 - 100
    if name == 'edges':
        assert [list(r) for r in got[:3, [9, 10, 16, 3]]] == [[0, 0, 0, 48], [1, 0, 0, 33], [2, 1, 0, 64]]
        assert list(got[3, [1, 10, 14, 7, 11, 33]]) == [100, 99, 1, 1, 1, 1]
        assert list(got[4, [7, 32, 41, 11, 14]]) == [100, 8, 1, 1, 100] and got[4, 16:32].sum() == 0
        assert list(got[5, [11, 14, 3]]) == [1, 1, 9] and got[5, 42:58].sum() == 0
        assert list(got[6, [3, 8, 6, 7, 9]]) == [3953, 1 + 3952 + 1, 3953 + 1, 2, 0]
    if name == 'gaps':
        gaps, _ = _gap_onsets()
        assert list(got[0, 42:58]) == [sum(1 for g in gaps if min(g.bit_length() - 1, 15) == b) for b in range(16)] and got[0, 57] == 1 and got[0, 42] == 2
    if name == 'start_one_value':
        assert (got[:, 0] == 53).all() and got.tobytes() == np.tile(got[0], 5).tobytes()
    if name == 'start_per_piece':
        assert list(got[:, 0]) == [90, 49, 1, 0, 0] and got[3:].sum() == 0
    if name == 'sweep_1028_pieces_of_7':
        assert list(got[:16, 0]) == [0, 1, 2, 3, 4, 5, 6, 7] * 2 and len(got) == GRID_CAP + 4


@pytest.mark.parametrize('name', list(CASES))
def test_columns_equal_the_restatement(name):
    _need_gpu()
    from pianobart_amd import metrics, structure, texture
    which, ids, start = CASES[name]
    tab, pad8 = _tables(which)[:2]
    want = _want(name)
    got = texture.piece_texture(ids, tab, start=start)
    again = texture.piece_texture(ids.astype(np.float32), tab, start=start)                  # the float32 that eval_generation writes
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(ids), 64) and got.is_cuda
    got = got.cpu().numpy()
    bad = np.argwhere(got != want)
    assert not len(bad), (name, bad[:8], [(int(got[i, j]), int(want[i, j])) for i, j in bad[:8]])
    assert again.cpu().numpy().tobytes() == got.tobytes()
    shuffled = _permuted(ids, pad8, start, 17)
    assert len(ids) == 0 or ids.shape[1] < 3 or (shuffled != ids).any()
    assert texture.piece_texture(shuffled, tab, start=start).cpu().numpy().tobytes() == got.tobytes()
    st = structure.piece_structure(ids, tab, start=start).cpu().numpy()
    ft = metrics.piece_features(ids, tab, start=start).cpu().numpy()
    assert np.array_equal(st[:, :2], got[:, [0, 2]]) and np.array_equal(ft[:, [0, 1, 3]], got[:, :3])    # notes, P, W: the same rows and bars
    _check_case(name, got, ids.shape[1])


def test_no_hollow_pass():
    """On the restatement alone: over the cases together every defined column is non-zero somewhere and takes two values; the undefined
    ones stay zero."""
    rows = np.concatenate([_want(name) for name in CASES])
    for j in DEFINED:
        assert rows[:, j].any() and len(np.unique(rows[:, j])) >= 2, j
    assert not rows[:, [15] + list(range(58, 64))].any()
    assert (rows[:, 16:33].sum(1) == rows[:, 3]).all() and (rows[:, 33:42].sum(1) == rows[:, 11]).all()
    assert (rows[:, 42:58].sum(1) == np.maximum(rows[:, 11] - 1, 0)).all() and (rows[:, 6] <= rows[:, 8]).all()
    assert (rows[rows[:, 1] == 0][:, 3:] == 0).all()


def test_empty_batch_and_refusals():
    _need_gpu()
    from pianobart_amd import ops, texture
    tab = _tables('default')[0]
    out = texture.piece_texture(np.zeros((0, 16, 8), dtype=np.int64), tab)
    assert tuple(out.shape) == (0, 64) and out.dtype == torch.int32
    dev = lambda x: torch.from_numpy(x).cuda()
    pitch_of, dur_pos, bar_pos = dev(tab.pitch_of), dev(tab.dur_pos), dev(tab.bar_pos)
    with pytest.raises(texture.PBError, match='4096'):
        ops.piece_texture(torch.zeros((1, 4097, 8), dtype=torch.int16, device='cuda'), pitch_of, dur_pos, bar_pos)
    with pytest.raises(texture.PBError, match='4096'):
        texture.piece_texture(np.zeros((1, 4097, 8), dtype=np.int64), tab)
    ids = torch.zeros((1, 4, 8), dtype=torch.int16, device='cuda')
    with pytest.raises(texture.PBError, match='bar_pos holds 253 entries'):
        ops.piece_texture(ids, pitch_of, dur_pos, bar_pos[:253].contiguous())
    with pytest.raises(texture.PBError, match='dur_pos holds 127 entries'):
        ops.piece_texture(ids, pitch_of, dur_pos[:127].contiguous(), bar_pos)
    with pytest.raises(texture.PBError, match='bar_pos'):
        ops.piece_texture(ids, pitch_of, dur_pos, bar_pos.to(torch.int64))
    # a device table with values out of range is clamped, not followed: a bar of 1 .. 1024 positions, a note of 1 .. 4096
    wild_bar, wild_dur = torch.full_like(bar_pos, 1 << 30), torch.full_like(dur_pos, -5)
    row = ops.piece_texture(dev(CASES['time_default'][1].astype(np.int16)), pitch_of, wild_dur, wild_bar).cpu().numpy()[0]
    assert row[2] == 56 and row[8] == row[1] and row[3] == 55 * 1024 + 70 + 1 and row[13] == 0


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def _sets():
    if 'sets' not in _CACHE:
        pad = np.asarray(D_DEFAULT) - 6
        gen = np.stack([R.from_notes(R.piano_notes(96, 500 + n, style=0), 96, pad, 40 + (7 * n) % 57) for n in range(26)])
        ref = np.stack([R.from_notes(R.piano_notes(96, 600 + n, style=1), 96, pad, 40 + (5 * n) % 57) for n in range(32)])
        for a, n in ((gen, 3), (gen, 11), (ref, 5)):                                          # percussion pieces: 24 and 31 are left
            a[n, :, 3] = np.where(a[n, :, 3] < 128, a[n, :, 3] + 128, a[n, :, 3])
        _CACHE['sets'] = (gen, ref)
    return _CACHE['sets']


def test_compare_texture_against_the_restatement():
    _need_gpu()
    from pianobart_amd import texture
    gen, ref = _sets()
    tab, pad8, pitch_of, dur_pos, bar_pos = _tables('default')
    res = texture.compare_texture(gen, ref, grid=1024)
    want = R.compare(gen, ref, pad8, pitch_of, dur_pos, bar_pos, grid=1024)
    assert (res['n_gen'], res['n_ref'], res['unpitched_gen'], res['unpitched_ref']) == (24, 31, 2, 1)
    for k in ('n_gen', 'n_ref', 'unpitched_gen', 'unpitched_ref'):
        assert res[k] == want[k], k
    assert set(res['device_ms']) == {'texture', 'distances', 'moments', 'kde', 'total'} and res['device_ms']['texture'] > 0
    for tag in ('gen', 'ref'):
        assert list(res['profile_' + tag]) == ['polyphony', 'chord']
        for k, width in (('polyphony', 17), ('chord', 9)):
            assert len(res['profile_' + tag][k]) == width and res['profile_' + tag][k] == want['profile_' + tag][k], (tag, k)
        assert abs(sum(res['profile_' + tag]['polyphony']) - 1) < 1e-12 and res['profile_' + tag]['polyphony'][2] > 0
    for cols, arrays in zip((texture.piece_texture(gen, tab), texture.piece_texture(ref, tab)), want['group_arrays']):
        g, _ = texture.texture_groups(cols)
        for k in texture.GROUPS:
            assert g[k].dtype == np.float32 and np.array_equal(g[k], arrays[k]), k
    assert list(res['groups']) == list(texture.GROUPS) == list(R.GROUPS)
    worst = 0.0
    for name in R.GROUPS:
        g, w = res['groups'][name], want['groups'][name]
        assert set(g) == {'mean_gen', 'std_gen', 'mean_ref', 'std_ref', 'dist_gen', 'dist_ref', 'dist_inter', 'kl', 'oa', 'kl_gen', 'oa_gen'}
        F = {'polyphony_hist': 17, 'chord_hist': 9, 'ioi_hist': 16}.get(name, 1)
        for k in ('mean_gen', 'mean_ref', 'std_gen', 'std_ref'):
            assert abs(g[k] - w[k]) <= 1e-12 * max(1.0, abs(w[k])), (name, k, g[k], w[k])
        for k in ('dist_gen', 'dist_ref', 'dist_inter'):
            assert abs(g[k] - w[k]) <= (F + 8) * 2.0 ** -24 * w[k], (name, k, g[k], w[k])
        assert not math.isnan(w['kl']) and not math.isnan(g['kl']) and not math.isnan(g['kl_gen']), name
        print('compare_texture %-17s kl %.9g (ref %.9g)  oa %.9g (ref %.9g)  kl_gen %.9g (ref %.9g)  oa_gen %.9g (ref %.9g)'
              % (name, g['kl'], w['kl'], g['oa'], w['oa'], g['kl_gen'], w['kl_gen'], g['oa_gen'], w['oa_gen']))
        worst = max([worst] + [abs(g[k] - w[k]) for k in ('kl', 'oa', 'kl_gen', 'oa_gen')])
    print('compare_texture: largest absolute kl / oa error %.4g (KLOA_TOL %.4g)' % (worst, KLOA_TOL))
    assert worst <= KLOA_TOL
    again = texture.compare_texture(gen, ref, grid=1024)
    assert all(again['groups'][n][k] == v or (math.isnan(v) and math.isnan(again['groups'][n][k])) for n, g in res['groups'].items() for k, v in g.items())


def test_cli(tmp_path, capsys):
    _need_gpu()
    from pianobart_amd import eval_texture, texture
    gen, ref = _sets()
    g4 = gen[:24].reshape(12, 2, 96, 8).astype(np.float32)                 # what eval_generation --samples 2 writes
    gp, rp, out = str(tmp_path / 'g.npy'), str(tmp_path / 'r.npy'), str(tmp_path / 't.json')
    np.save(gp, g4)
    np.save(rp, ref)
    res = eval_texture.main(['--generated', gp, '--reference', rp, '--output', out, '--grid', '128', '--skip', '2', '--max_pieces', '20'])
    js = json.load(open(out))
    assert set(js) == {'n_gen', 'n_ref', 'unpitched_gen', 'unpitched_ref', 'device_ms', 'profile_gen', 'profile_ref', 'groups'}
    assert list(js['groups']) == list(texture.GROUPS) and (js['n_gen'], js['unpitched_gen'], js['n_ref'], js['unpitched_ref']) == (18, 2, 19, 1)
    direct = texture.compare_texture(gen[:20], ref[:20], grid=128, start=2)
    assert all(js['groups'][n]['oa'] == g['oa'] and res['groups'][n]['kl'] == g['kl'] for n, g in direct['groups'].items())
    assert js['profile_gen'] == json.loads(json.dumps(direct['profile_gen']))
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith('   [texture]')]
    assert len(lines) == 2 * 4 + 13 + 1 and 'polyphony' in lines[1] and '>=8' in lines[1]
    one = eval_texture.main(['--generated', gp, '--output', out, '--max_pieces', '20'])
    js = json.load(open(out))
    assert set(js) == {'n', 'unpitched', 'device_ms', 'profile', 'means'} and (js['n'], js['unpitched']) == (18, 2)
    assert set(js['means']) == set(texture.SCALAR_GROUPS) and js['means'] == dict(one['means'])
    assert js['profile'] == json.loads(json.dumps(texture.pooled_profiles(texture.piece_texture(gen[:20]))))
    assert 0 < js['means']['polyphonic_rate'] < 1 < js['means']['polyphony_mean'] <= js['means']['max_polyphony']
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith('   [texture]')]
    assert len(lines) == 4 + 1
