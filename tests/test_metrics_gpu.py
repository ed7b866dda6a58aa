"""GPU: the kernels of csrc/pb_metrics.hip and pianobart_amd.metrics against the float64 restatement of tests/metrics_ref.py.

  * features: exact integer equality, at every S where the row loop changes shape (1, 7, 64, 65, 257, 1 024: under one wave, one chunk of
    256 rows and its edges, four chunks), L = 0, 1, S - 1, S, a special id in one head only, all-percussion pieces, one pitched note,
    pitched / 300 percussion / pitched (the previous pitched note lies a chunk back), bars out of order, the last bar id of the default
    and of the wide dictionary, more than 32 notes in a bar, start = 0 / mid / >= L, N = 1, and N = 64 at S = 7 and S = 64, where a
    workgroup takes 292 and 32 pieces, so that the sweep runs. Two runs give the same bytes.
  * distances: |got - ref| <= (F + 8) 2^-24 ref against float64 on the same f32 rows: F terms of three roundings each and F - 1
    additions, halved by the square root, is (F / 2 + 3) units; doubled for a 1-ulp sqrtf. A row shared by both sets gives exactly 0.
  * moments: n, min and max exact; sum and sum of squares within n 2^-52 relative of the exactly rounded float64 sums (math.fsum).
  * KDE: |got - ref| <= RTOL ref + 2^-100 max(ref), the absolute term admitting a flush to zero where every f32 term underflows.
    Measured on the MI355X over these cases: the largest relative error is KDE_MEASURED; RTOL is four times that, the
    margin for another compiler's expansion of exp (the kernel itself is deterministic). The f32 argument error alone, 4 roundings of
    2^-24 on an exponent of up to 87, is 2e-5; a measured value above 2.5e-4 would be a bug.
  * end to end: compare_sets on seeded sets of 24 and 31 pieces against the restatement's pipeline: counts exact, feature means and
    stds to 1e-12, distance means within the distance bound, kl / oa within KLOA_TOL = four times the measured KLOA_MEASURED; a set
    against itself gives oa > 0.5 (the inter density holds the zero diagonal, the intra density does not); the CLI on an (N, S, 8) and an
    (N, n, S, 8) file."""
import json
import math

import numpy as np
import pytest
import torch

from tests import metrics_ref as R
from tests.vocab_layout_util import D_DEFAULT, D_WIDE, make_dict

pytestmark = pytest.mark.gpu

KDE_MEASURED = 4.84e-6        # at (8, 8), G = 1 024, h = 1e-3 of the spread
RTOL = 4 * KDE_MEASURED
KLOA_MEASURED = 6.01e-8       # the kl of avg_duration; the largest oa error is 2.3e-8
KLOA_TOL = 4 * KLOA_MEASURED
_CACHE = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- features ---------------------------------------------------------------------------------------------------------------------------
def _terminate(ids, n, L, pad):
    if L < ids.shape[1]:
        ids[n, L] = pad + 3
        ids[n, L + 1:] = pad


def _feature_cases():
    """{name: (sizes, percussion ids, ids, start)}"""
    pad = np.asarray(D_DEFAULT) - 6
    wpad = np.asarray(D_WIDE) - 6
    cases = {}
    for S in (1, 7, 64, 65, 257, 1024):
        cases['S%d' % S] = (D_DEFAULT, 128, R.synth_pieces(D_DEFAULT, 4, S, seed=100 + S), None)
    S = 65
    ids = np.repeat(R.synth_pieces(D_DEFAULT, 1, S, seed=7), 4, axis=0)
    for n, L in enumerate((0, 1, S - 1, S)):
        _terminate(ids, n, L, pad)
    cases['lengths'] = (D_DEFAULT, 128, ids, None)
    ids = np.repeat(R.synth_pieces(D_DEFAULT, 1, 64, seed=8), 8, axis=0)
    for h in range(8):
        ids[h, 20 + h, h] = pad[h] + (h % 6)           # one special id in head h only; the rows behind it are ordinary
    cases['one_head_special'] = (D_DEFAULT, 128, ids, None)
    ids = np.repeat(R.synth_pieces(D_DEFAULT, 1, 70, seed=9), 3, axis=0)
    ids[:, :, 3] = np.random.default_rng(9).integers(128, 256, size=(3, 70))
    ids[1, 33, 3] = 61                                 # one pitched note
    ids[2, 0, 3], ids[2, 69, 3] = 5, 100               # a pitched pair with 68 drums between
    cases['percussion'] = (D_DEFAULT, 128, ids, None)
    ids = np.repeat(R.synth_pieces(D_DEFAULT, 1, 400, seed=10), 2, axis=0)
    ids[:, :, 3] = np.random.default_rng(10).integers(0, 128, size=(2, 400))
    ids[:, 50:350, 3] = np.random.default_rng(11).integers(128, 256, size=(2, 300))
    ids[1, 49, 3] = 200                                # the last pitched note in front of the drums one row earlier
    cases['pitched_300_drums_pitched'] = (D_DEFAULT, 128, ids, None)
    ids = R.synth_pieces(D_DEFAULT, 3, 300, seed=12)
    ids[:, :, 0] = np.random.default_rng(12).integers(0, 256, size=(3, 300))
    ids[0, 17, 0] = 255                                # pad8[0] - 1
    cases['bars_out_of_order'] = (D_DEFAULT, 128, ids, None)
    ids = R.synth_pieces(D_WIDE, 3, 130, seed=13, n_perc=0)
    ids[:, :, 0] = np.random.default_rng(13).integers(0, wpad[0], size=(3, 130))
    ids[0, 5, 0], ids[1, 129, 0], ids[0, 6, 3] = wpad[0] - 1, wpad[0] - 1, wpad[3] - 1
    cases['wide_dictionary'] = (D_WIDE, 0, ids, None)
    ids = R.synth_pieces(D_DEFAULT, 2, 140, seed=14)
    ids[0, :, 0] = np.repeat([0, 1, 2, 3], [32, 33, 40, 35])
    ids[1, :, 0] = 9
    cases['crowded_bars'] = (D_DEFAULT, 128, ids, None)
    ids = np.repeat(R.synth_pieces(D_DEFAULT, 1, 300, seed=15), 6, axis=0)
    for n in range(6):
        _terminate(ids, n, 280, pad)
    cases['start'] = (D_DEFAULT, 128, ids, np.array([0, 1, 131, 279, 280, 299], dtype=np.int32))
    cases['N1'] = (D_DEFAULT, 128, R.synth_pieces(D_DEFAULT, 1, 33, seed=16), None)
    cases['sweep_S7'] = (D_DEFAULT, 128, R.synth_pieces(D_DEFAULT, 64, 7, seed=17), None)
    cases['sweep_S64'] = (D_DEFAULT, 128, R.synth_pieces(D_DEFAULT, 64, 64, seed=18), np.arange(64, dtype=np.int32) % 5)
    return cases


FEATURE_CASES = _feature_cases()


def _tables(sizes, n_perc):
    from pianobart_amd import metrics
    key = ('tab', tuple(sizes))
    if key not in _CACHE:
        tab = metrics.tables(None if list(sizes) == D_DEFAULT else make_dict(sizes)[0])
        pad8, pitch_of, dur_pos = R.tables_for(sizes, n_perc)
        assert list(tab.layout.pad8) == pad8 and (tab.pitch_of == pitch_of).all() and (tab.dur_pos == dur_pos).all()
        _CACHE[key] = (tab, pad8, pitch_of, dur_pos)
    return _CACHE[key]


@pytest.mark.parametrize('name', list(FEATURE_CASES))
def test_features_equal_the_restatement(name):
    _need_gpu()
    from pianobart_amd import metrics
    sizes, n_perc, ids, start = FEATURE_CASES[name]
    tab, pad8, pitch_of, dur_pos = _tables(sizes, n_perc)
    want = R.features(ids, pad8, pitch_of, dur_pos, start)
    got = metrics.piece_features(ids, tab, start=start)
    again = metrics.piece_features(ids.astype(np.float32), tab, start=start)       # the float32 that eval_generation writes
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(ids), 288) and got.is_cuda
    got = got.cpu().numpy()
    bad = np.argwhere(got != want)
    assert not len(bad), (name, bad[:8], [(int(got[i, j]), int(want[i, j])) for i, j in bad[:8]])
    assert np.array_equal(again.cpu().numpy(), got)
    if name == 'lengths':
        assert list(got[:, 0]) == [0, 1, 64, 65]
    if name == 'start':
        assert list(got[:, 0]) == [280, 279, 149, 1, 0, 0]
    if name == 'crowded_bars':
        assert got[0, 252 + 31] == 4 and got[1, 252 + 31] == 1 and got[:, 252:284].sum() == 5


# ---- distances ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(1, 1), (3, 5), (64, 65), (130, 7)])
@pytest.mark.parametrize('F', [1, 12, 16, 32, 143, 144])
def test_pairwise_l2(F, shape):
    _need_gpu()
    from pianobart_amd import ops
    N, M = shape
    rng = np.random.default_rng(1000 * F + N)
    for kind in ('normal', 'histogram'):
        A, B = (rng.standard_normal((n, F)) if kind == 'normal' else rng.dirichlet(np.ones(F) * 0.3, size=n) for n in (N, M))
        A, B = A.astype(np.float32), B.astype(np.float32)
        B[M - 1] = A[N // 2]                           # a row that both sets hold
        D = ops.pairwise_l2(_dev(A), _dev(B))
        assert D.dtype == torch.float32 and tuple(D.shape) == (N, M)
        got = D.cpu().numpy().astype(np.float64)
        ref = R.pairwise(A, B)
        assert got[N // 2, M - 1] == 0.0
        err = np.abs(got - ref)
        worst = float((err / np.where(ref > 0, ref, 1.0)).max())
        print('pairwise_l2 F=%d %s %s: largest relative error %.3g (bound %.3g)' % (F, shape, kind, worst, (F + 8) * 2.0 ** -24))
        assert (err <= (F + 8) * 2.0 ** -24 * ref).all()
        assert torch.equal(ops.pairwise_l2(_dev(A), _dev(B)), D)


# ---- moments and KDE ------------------------------------------------------------------------------------------------------------------------
SAMPLE_SHAPES = [((1, 1), False), ((1, 2), False), ((7, 9), False), ((8, 8), False), ((5, 13), False), ((63, 64), False),      # n = 1, 2, 63, 64, 65, 4 032
                 ((2, 2), True), ((3, 3), True), ((17, 17), True)]                                                              # n = 1, 3, 136


def _matrix(shape, upper):
    key = ('D', shape, upper)
    if key not in _CACHE:
        rng = np.random.default_rng(shape[0] * 100 + shape[1] + upper)
        _CACHE[key] = np.abs(rng.standard_normal(shape) * 2.0 + 3.0).astype(np.float32)
    return _CACHE[key]


@pytest.mark.parametrize('shape,upper', SAMPLE_SHAPES)
def test_sample_moments(shape, upper):
    _need_gpu()
    from pianobart_amd import ops
    D = _matrix(shape, upper)
    s = R.samples(D, upper).astype(np.float64)
    d = _dev(D)
    out = ops.sample_moments(d, upper)
    got = out.cpu().numpy()
    n = len(s)
    want_sum, want_sq = math.fsum(s), math.fsum(s * s)                     # the products of two f32 values are exact in f64
    print('moments %s upper=%d: n %d, relative errors %.3g %.3g (bound %.3g)' % (shape, upper, n, abs(got[1] - want_sum) / want_sum,
                                                                                  abs(got[2] - want_sq) / want_sq, n * 2.0 ** -52))
    assert got[0] == n and got[3] == 0 and got[4] == s.min() and got[5] == s.max()
    assert abs(got[1] - want_sum) <= n * 2.0 ** -52 * want_sum and abs(got[2] - want_sq) <= n * 2.0 ** -52 * want_sq
    assert torch.equal(ops.sample_moments(d, upper), out)


def kde_cases():
    """(label, D, upper, grid f32, h) for every sample shape, G in 1, 7, 64, 65, 1 024 and h = 1e-3 .. 10 times the spread; the grid runs
    from 3 h below the smallest sample to 3 h above the largest (G = 1: the point 3 h below)."""
    for shape, upper in SAMPLE_SHAPES:
        D = _matrix(shape, upper)
        s = R.samples(D, upper).astype(np.float64)
        spread = float(s.max() - s.min()) or 1.0
        for G in (1, 7, 64, 65, 1024):
            for scale in (1e-3, 3e-2, 0.3, 10.0):
                h = scale * spread
                grid = np.linspace(s.min() - 3 * h, s.max() + 3 * h, G).astype(np.float32) if G > 1 else np.array([s.min() - 3 * h], dtype=np.float32)
                yield '%s%s G=%d h=%g' % (shape, 'u' if upper else '', G, scale), D, upper, grid, h


def kde_errors(case):
    """(got, ref, the largest relative error left after the absolute term) of one case."""
    from pianobart_amd import ops
    label, D, upper, grid, h = case
    d, g = _dev(D), _dev(grid)
    dens = ops.kde_eval(d, g, h, upper)
    assert dens.dtype == torch.float64 and tuple(dens.shape) == (len(grid),)
    assert torch.equal(ops.kde_eval(d, g, h, upper), dens), label
    got = dens.cpu().numpy()
    ref = R.kde(R.samples(D, upper), grid, h)
    assert ref.max() > 0, label
    excess = np.abs(got - ref) - 2.0 ** -100 * ref.max()
    rel = float(np.max(np.where(ref > 0, excess / np.where(ref > 0, ref, 1.0), np.where(excess > 0, np.inf, 0.0))))
    return got, ref, max(rel, 0.0)


def test_kde_eval():
    _need_gpu()
    worst = (0.0, '')
    failed = []
    for case in kde_cases():
        got, ref, rel = kde_errors(case)
        worst = max(worst, (rel, case[0]))
        if not (np.abs(got - ref) <= RTOL * ref + 2.0 ** -100 * ref.max()).all():
            failed.append((case[0], rel))
    print('kde_eval: largest relative error %.4g at %s (RTOL %.4g)' % (worst[0], worst[1], RTOL))
    assert worst[0] <= 2.5e-4, 'a relative error above 2.5e-4 is a bug, not a tolerance: %r' % (worst,)
    assert not failed, failed[:10]


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------
def _sets():
    if 'sets' not in _CACHE:
        pad = np.asarray(D_DEFAULT) - 6
        gen, ref = R.synth_pieces(D_DEFAULT, 26, 96, seed=21, style=1), R.synth_pieces(D_DEFAULT, 32, 96, seed=22, style=0)
        gen[3, 0] = gen[11, 0] = ref[5, 0] = pad + 3                       # empty pieces: 24 and 31 are left
        _CACHE['sets'] = (gen, ref)
    return _CACHE['sets']


def kloa_errors(gen, ref, res):
    """The largest absolute kl / oa error of a compare_sets result against the restatement's pipeline, after the exact checks."""
    pad8, pitch_of, dur_pos = R.tables_for(D_DEFAULT, 128)
    key = ('want', id(gen), id(ref))
    if key not in _CACHE:
        _CACHE[key] = R.compare(gen, ref, pad8, pitch_of, dur_pos)
    want = _CACHE[key]
    for k in ('n_gen', 'n_ref', 'empty_gen', 'empty_ref'):
        assert res[k] == want[k], k
    assert list(res['groups']) == list(want['groups']) and len(res['groups']) == 14
    worst = 0.0
    for name, w in want['groups'].items():
        g = res['groups'][name]
        F = {'pch': 12, 'pctm': 144, 'beat_grid': 16}.get(name, 32 if name.endswith('_hist') else 1)
        for k in ('mean_gen', 'mean_ref', 'std_gen', 'std_ref'):
            assert abs(g[k] - w[k]) <= 1e-12 * max(1.0, abs(w[k])), (name, k, g[k], w[k])
        for k in ('dist_gen', 'dist_ref', 'dist_inter'):
            assert abs(g[k] - w[k]) <= (F + 8) * 2.0 ** -24 * w[k], (name, k, g[k], w[k])
        assert not math.isnan(w['kl']) and not math.isnan(g['kl']), name
        print('compare_sets %-17s kl %.9g (ref %.9g)  oa %.9g (ref %.9g)' % (name, g['kl'], w['kl'], g['oa'], w['oa']))
        worst = max(worst, abs(g['kl'] - w['kl']), abs(g['oa'] - w['oa']))
    return worst


def test_compare_sets_against_the_restatement():
    _need_gpu()
    from pianobart_amd import metrics
    gen, ref = _sets()
    res = metrics.compare_sets(gen, ref)
    assert res['n_gen'] == 24 and res['n_ref'] == 31 and res['empty_gen'] == 2 and res['empty_ref'] == 1
    assert set(res['device_ms']) == {'features', 'distances', 'moments', 'kde', 'total'} and res['device_ms']['total'] > 0
    worst = kloa_errors(gen, ref, res)
    print('compare_sets: largest absolute kl / oa error %.4g (KLOA_TOL %.4g)' % (worst, KLOA_TOL))
    assert worst <= KLOA_TOL
    again = metrics.compare_sets(gen, ref)
    assert all(again['groups'][n][k] == v for n, g in res['groups'].items() for k, v in g.items())


def test_a_set_against_itself_and_the_degenerate_rule():
    _need_gpu()
    from pianobart_amd import metrics
    gen, _ = _sets()
    res = metrics.compare_sets(gen, gen, grid=256)
    for name, g in res['groups'].items():
        assert 0.5 < g['oa'] < 1.0 + 1e-3, (name, g)
        assert g['mean_gen'] == g['mean_ref'] and g['dist_gen'] == g['dist_ref']
    same = np.repeat(gen[:1], 5, axis=0)                                   # five equal pieces: no distance has any spread
    res = metrics.compare_sets(same, same, grid=64)
    assert res['n_gen'] == 5 and all(math.isnan(g['kl']) and math.isnan(g['oa']) and g['dist_inter'] == 0.0 for g in res['groups'].values())
    res = metrics.compare_sets(gen[:1], gen[:9], grid=64)                  # one generated piece: no intra-gen sample
    assert res['n_gen'] == 1 and all(math.isnan(g['kl']) and math.isnan(g['dist_gen']) and g['dist_ref'] > 0 for g in res['groups'].values())


def test_cli(tmp_path, capsys):
    _need_gpu()
    from pianobart_amd import eval_metrics, metrics
    gen, ref = _sets()
    g4 = gen[:24].reshape(12, 2, 96, 8).astype(np.float32)                 # what eval_generation --samples 2 writes
    gp, rp, out = str(tmp_path / 'g.npy'), str(tmp_path / 'r.npy'), str(tmp_path / 'm.json')
    np.save(gp, g4)
    np.save(rp, ref)
    res = eval_metrics.main(['--generated', gp, '--reference', rp, '--output', out, '--grid', '128', '--skip', '2', '--max_pieces', '20'])
    js = json.load(open(out))
    assert set(js) == {'n_gen', 'n_ref', 'empty_gen', 'empty_ref', 'device_ms', 'groups'} and list(js['groups']) == list(metrics.GROUPS)
    assert (js['n_gen'], js['empty_gen'], js['n_ref'], js['empty_ref']) == (18, 2, 19, 1)
    for g in js['groups'].values():
        assert set(g) == {'mean_gen', 'std_gen', 'mean_ref', 'std_ref', 'dist_gen', 'dist_ref', 'dist_inter', 'kl', 'oa', 'kl_gen', 'oa_gen'}
    direct = metrics.compare_sets(gen[:20], ref[:20], grid=128, start=2)
    assert all(js['groups'][n]['oa'] == g['oa'] and res['groups'][n]['kl'] == g['kl'] for n, g in direct['groups'].items())
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith('   [metrics]')]
    assert len(lines) == 14 + 2
