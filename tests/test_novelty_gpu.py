"""GPU: the kernels of csrc/pb_runs.hip and pianobart_amd.novelty against the restatement of tests/novelty_ref.py. Everything is an
integer: every comparison is ==, there is no tolerance.

  * keys: both modes, the default dictionary and the 2 470-id one, S = 1, 2, 63, 64, 65, 257, 1 024 (under a wave, one sweep of 256
    threads and its edges, four sweeps), start = None, one number, and one per piece with values >= L; N chosen so that a workgroup
    takes several pieces (the grid sweep), N = 1, and 1 030 pieces of 1 025 rows, more pieces than the grid has workgroups.
  * runs: key rows over a 3-pitch x 2-position alphabet (random runs of 5 to 15 keys; rows over the whole vocabulary would test zeros),
    one call over rows of 0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 1 023 and 4 095 keys on both sides (every pair, so K_a != K_b both
    ways; Sa != Sb), with planted copies: on a diagonal behind the first 256, on a diagonal before the main one, ending in the last key
    of both rows, of a whole row, and of a whole row at the end of a longer one. min_run = 1, 4, longest, longest + 1. Corpus windows on
    both sides of every workgroup size and of the step from one to two diagonals per thread. Then N = 1, 3
    against M = 1, T - 1, T, T + 1, 2 T + 1 with duplicated corpus rows (a tie in best: the smallest j wins), R = NULL, exclude_self,
    chunked accumulation equal to the one-shot call bit for bit, two calls giving equal bytes, empty sides.
  * end to end: compare_to_corpus and the CLI on 24 x 40 pieces of 96 rows against the restatement: an (N, n, S, 8) file, --skip,
    --transpose, --self."""
import json

import numpy as np
import pytest
import torch

from tests import novelty_ref as R
from tests.vocab_layout_util import D_DEFAULT, D_WIDE, make_dict

pytestmark = pytest.mark.gpu

_CACHE = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _u32(t):
    """A device int32 key tensor as the uint32 array it holds."""
    return t.cpu().numpy().view(np.uint32)


def _tables(sizes):
    """(pad8, pitch_of, e2w): the default dictionary's last 128 pitch ids are percussion; the wide one has none."""
    pad8 = [n - 6 for n in sizes]
    if sizes == D_DEFAULT:
        return pad8, np.array([i if i < 128 else -1 for i in range(pad8[3])]), None
    return pad8, np.arange(pad8[3]), make_dict(sizes)[0]


# ---- keys -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S', [1, 2, 63, 64, 65, 257, 1024])
@pytest.mark.parametrize('sizes', [D_DEFAULT, D_WIDE], ids=['default', 'wide'])
@pytest.mark.parametrize('mode', ['exact', 'interval'])
def test_keys(mode, sizes, S):
    _need_gpu()
    from pianobart_amd import novelty
    pad8, pitch_of, e2w = _tables(sizes)
    N = 70 if S <= 65 else 17 if S == 257 else 5                           # a workgroup takes 2048 / S pieces: 1 to 3 workgroups, each sweeping
    ids = R.synth_pieces(pad8, N, S, seed=S + len(mode), pitches=None if S % 2 else [60, 62, 130, pad8[3] - 1])
    rng = np.random.default_rng(S)
    for start in (None, 1, rng.integers(0, S + 2, size=N)):
        want_keys, want_len = R.keys_ref(ids, pad8, pitch_of, mode, start)
        keys, klen = novelty.piece_keys(ids, e2w, start=start, transpose=mode == 'interval')
        assert keys.dtype == torch.int32 and tuple(keys.shape) == (N, S) and klen.dtype == torch.int32
        assert np.array_equal(klen.cpu().numpy(), want_len) and np.array_equal(_u32(keys), want_keys)
    one_keys, one_len = novelty.piece_keys(ids[:1], e2w, transpose=mode == 'interval')                    # N = 1: one workgroup, no sweep
    assert np.array_equal(_u32(one_keys), R.keys_ref(ids[:1], pad8, pitch_of, mode)[0]) and int(one_len[0]) == S - 1      # piece 0 fills the window


def test_keys_more_pieces_than_workgroups():
    _need_gpu()
    from pianobart_amd import novelty
    pad8, pitch_of, _ = _tables(D_DEFAULT)
    N, S = 1030, 1025                                                      # one piece per workgroup, a grid of 1 024: six workgroups take two
    rng = np.random.default_rng(5)
    ids = np.tile(np.asarray(pad8), (N, S, 1))
    for n in range(N):
        L = S if n in (0, 1024, N - 1) else int(rng.integers(0, 6))
        ids[n, :L] = np.stack([rng.integers(0, pad8[h], size=L) for h in range(8)], axis=1)
    want_keys, want_len = R.keys_ref(ids, pad8, pitch_of, 'interval')
    keys, klen = novelty.piece_keys(ids.astype(np.int16), transpose=True)
    assert want_len[0] == S - 1 and np.array_equal(klen.cpu().numpy(), want_len) and np.array_equal(_u32(keys), want_keys)


# ---- runs -------------------------------------------------------------------------------------------------------------------------------
ALPHABET = np.array([pit | pos << 12 for pit in (60, 62, 64) for pos in (0, 4)], dtype=np.uint32)
KS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 1023, 4095]


def _rows(rng, lens, S):
    keys = np.full((len(lens), S), R.NO_KEY, dtype=np.uint32)
    for n, K in enumerate(lens):
        keys[n, :K] = rng.choice(ALPHABET, size=K)
    return keys


def _call(A, alen, B, blen, **kw):
    from pianobart_amd import ops
    t = lambda k: _dev(np.ascontiguousarray(k).view(np.int32))
    l = lambda n: _dev(np.asarray(n, dtype=np.int32))
    return ops.shared_runs(t(A), l(alen), t(B), l(blen), **kw)


def _same(got, want):
    return got.dtype in (torch.int32, torch.int64) and np.array_equal(got.cpu().numpy().astype(np.int64), want)


def _edges():
    """The call over every pair of lengths of KS with its planted copies, and the restatement's outputs at min_run = 1."""
    if 'edges' not in _CACHE:
        rng = np.random.default_rng(11)
        A, B = _rows(rng, KS, 4096), _rows(rng, KS, 4095)
        a, b = A[12], B[12]
        a[700:740] = b[1000:1040]                                          # diagonal +300: behind the first 256 diagonals
        a[2300:2340] = b[2000:2040]                                        # diagonal -300: before the main diagonal
        a[4095 - 30:4095] = b[4095 - 30:4095]                              # ends in the last key of both rows
        A[9, :511] = B[9, :511]                                            # a whole row
        A[5, :65] = B[10, 513 - 65:513]                                    # a whole row at the end of a longer one
        _CACHE['edges'] = (A, B) + R.outputs_ref(A, KS, B, KS)
    return _CACHE['edges']


def test_runs_at_every_length_edge():
    _need_gpu()
    A, B, want_R, want_end, want_best = _edges()
    assert want_R[9, 9] == 511 and want_R[5, 10] >= 65 and want_R[12, 12] >= 40 and want_end[12, 4094] >= 30 and want_end[12, 739] >= 40
    assert 5 <= np.median(want_R[8:, 8:]) <= 15                            # the alphabet does what it is there for
    got_R, got_end, got_best = _call(A, KS, B, KS, min_run=1)
    assert _same(got_R, want_R) and _same(got_end, want_end) and _same(got_best, want_best)


def test_runs_min_run():
    _need_gpu()
    A, B, want_R, want_end, want_best = _edges()
    rows = [8, 11, 12]                                                     # their longest run is the threshold: one row keeps one entry, then none
    longest = int(want_R[rows].max())
    for min_run in (4, longest, longest + 1):
        got_R, got_end, got_best = _call(A[rows], [KS[r] for r in rows], B, KS, min_run=min_run)
        want = np.where(want_end[rows] >= min_run, want_end[rows], 0)
        assert (want > 0).any() == (min_run <= longest)
        assert _same(got_R, want_R[rows]) and _same(got_end, want) and _same(got_best, want_best[rows])


def _small(N, M, seed, S=96):
    rng = np.random.default_rng(seed)
    alen, blen = rng.integers(0, S + 1, size=N), rng.integers(0, S - 4, size=M)
    A, B = _rows(rng, alen, S), _rows(rng, blen, S - 5)
    if M > 2:
        B[1], blen[1] = _rows(rng, [S - 5], S - 5)[0], S - 5               # a row that fills its window ...
        B[M - 1], blen[M - 1] = B[1], blen[1]                              # ... twice: a tie wherever it holds the longest run,
        A[0, :S], alen[0] = np.resize(B[1], S), S                          # and in piece 0, which repeats it, it does
    return A, alen, B, blen


@pytest.mark.parametrize('N', [1, 3])
@pytest.mark.parametrize('M', ['1', 'T-1', 'T', 'T+1', '2T+1'])
def test_runs_tiles_ties_and_no_matrix(N, M):
    _need_gpu()
    from pianobart_amd import novelty, ops
    T = ops.RUNS_TILE
    M = {'1': 1, 'T-1': T - 1, 'T': T, 'T+1': T + 1, '2T+1': 2 * T + 1}[M]
    A, alen, B, blen = _small(N, M, seed=100 * N + M)
    want_R, want_end, want_best = R.outputs_ref(A, alen, B, blen, min_run=4)
    got_R, got_end, got_best = _call(A, alen, B, blen, min_run=4)
    assert _same(got_R, want_R) and _same(got_end, want_end) and _same(got_best, want_best)
    if M > 2:
        assert novelty.split_best(got_best)[1][0] == 1 and want_R[0, 1] == want_R[0, M - 1] == want_R[0].max() == 91
    none_R, none_end, none_best = _call(A, alen, B, blen, min_run=4, want_matrix=False)                   # R = NULL
    assert none_R is None and torch.equal(none_end, got_end) and torch.equal(none_best, got_best)
    again = _call(A, alen, B, blen, min_run=4)                                                            # equal inputs, equal bytes
    assert all(torch.equal(x, y) for x, y in zip(again, (got_R, got_end, got_best)))


@pytest.mark.parametrize('Sb', [63, 64, 127, 128, 191, 192, 256, 257, 382, 384])
def test_runs_workgroup_sizes(Sb):
    """Up to Sb = 256 a thread takes one diagonal, beyond it two, and the workgroup has as many waves as the Sb + 1 diagonals need, four
    at the most: 1, 2, 3 and 4 waves of the first form, 3 and 4 of the second, on both sides of each step."""
    _need_gpu()
    rng = np.random.default_rng(Sb)
    alen, blen = [200, 77], [Sb, Sb - 1, Sb // 2]
    A, B = _rows(rng, alen, 200), _rows(rng, blen, Sb)
    A[1, 40:77] = B[0, Sb - 37:Sb]                                         # ends in the window's last key: the last diagonals of the last wave
    want = R.outputs_ref(A, alen, B, blen, min_run=3)
    got = _call(A, alen, B, blen, min_run=3)
    assert want[0][1, 0] >= 37 and all(_same(g, w) for g, w in zip(got, want))


def test_runs_exclude_self():
    _need_gpu()
    from pianobart_amd import ops
    N = ops.RUNS_TILE + 1
    A, alen, _, _ = _small(N, 1, seed=3)
    A[20], alen[20] = _rows(np.random.default_rng(4), [96], 96)[0], 96
    A[7], alen[7] = A[20], alen[20]                                        # a duplicate: each finds the other, not itself
    want = R.outputs_ref(A, alen, A, alen, min_run=2, exclude_self=True)
    got = _call(A, alen, A, alen, min_run=2, exclude_self=True)
    assert all(_same(g, w) for g, w in zip(got, want))
    assert (np.diag(want[0]) == 0).all() and want[0][7, 20] == alen[20] and want[2][7] == (alen[20] << 32) | (0xFFFFFFFF - 20)
    full = _call(A, alen, A, alen, min_run=2)
    assert (np.diag(full[0].cpu().numpy()) == alen).all()


def test_runs_chunked_accumulation_is_the_one_shot_call():
    _need_gpu()
    from pianobart_amd import novelty, ops
    N, M = 3, 2 * ops.RUNS_TILE + 1
    A, alen, B, blen = _small(N, M, seed=9)
    want = R.outputs_ref(A, alen, B, blen, min_run=3)
    one = _call(A, alen, B, blen, min_run=3)
    assert all(_same(g, w) for g, w in zip(one, want))
    for order in ((0, 20, 40, 60), (60, 40, 0, 20)):                       # chunks of 20 (and 5) pieces, in two orders
        run_end = best = None
        Rs = {}
        for j0 in order:
            Rs[j0], run_end, best = _call(A, alen, B[j0:j0 + 20], blen[j0:j0 + 20], min_run=3, j_base=j0, run_end=run_end, best=best)
        assert torch.equal(torch.cat([Rs[j0] for j0 in sorted(Rs)], dim=1), one[0]) and torch.equal(run_end, one[1]) and torch.equal(best, one[2])
    t = lambda k: _dev(np.ascontiguousarray(k).view(np.int32))
    l = lambda n: _dev(np.asarray(n, dtype=np.int32))
    host = novelty.shared_runs(t(A), l(alen), t(B), l(blen), min_run=3, chunk=20, want_matrix=True)
    assert all(torch.equal(x, y) for x, y in zip(host, one))


def test_runs_empty_sides():
    _need_gpu()
    A, alen, B, blen = _small(3, 4, seed=2)
    got_R, got_end, got_best = _call(A, alen, B[:0], blen[:0], min_run=1)
    assert tuple(got_R.shape) == (3, 0) and int(got_end.abs().sum()) == 0 and int(got_best.abs().sum()) == 0      # cleared, on the stream
    got_R, got_end, got_best = _call(A[:0], alen[:0], B, blen, min_run=1)
    assert tuple(got_R.shape) == (0, 4) and tuple(got_end.shape) == (0, 96) and tuple(got_best.shape) == (0,)
    got_R, got_end, got_best = _call(A, np.zeros(3), B, blen, min_run=1)   # pieces without keys
    assert int(got_R.abs().sum()) == 0 and int(got_end.abs().sum()) == 0 and int(got_best.abs().sum()) == 0


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
def _sets():
    pad8, pitch_of, _ = _tables(D_DEFAULT)
    kw = dict(pitches=[60, 62, 64, 130], positions=[0, 4, 8])
    gen, cor = R.synth_pieces(pad8, 24, 96, seed=21, **kw), R.synth_pieces(pad8, 40, 96, seed=22, **kw)
    cor[0, :, 3] = np.where(cor[0, :, 3] == 130, 60, cor[0, :, 3])         # no drum: the key behind one holds an absolute pitch
    cor[7], gen[2] = R.synth_pieces(pad8, 1, 96, seed=23, **kw)[0], R.synth_pieces(pad8, 1, 96, seed=24, **kw)[0]      # both fill the window
    gen[3] = cor[7]                                                        # a verbatim piece
    gen[5, 10:40] = cor[0, 20:50]                                          # thirty notes of the piece that fills its window
    gen[6] = cor[0]
    gen[6, :, 3] = np.where(gen[6, :, 3] < 128, gen[6, :, 3] + 2, gen[6, :, 3])      # the same piece two semitones up
    gen[8] = gen[2]                                                        # a duplicate inside the generated set
    return pad8, pitch_of, gen, cor


def _expect(gen, cor, pad8, pitch_of, mode, skip, min_run, exclude_self=False):
    ka, la = R.keys_ref(gen, pad8, pitch_of, mode, skip)
    kb, lb = (ka, la) if exclude_self else R.keys_ref(cor, pad8, pitch_of, mode)
    Rm, run_end, best = R.outputs_ref(ka, la, kb, lb, min_run=min_run, exclude_self=exclude_self)
    longest = Rm.max(axis=1)
    nearest = np.where(longest > 0, Rm.argmax(axis=1), -1)
    cov = np.array([R.coverage_ref(run_end[i], int(la[i])) for i in range(len(la))])
    return la, longest, nearest, cov, Rm


def _check(res, want, min_run):
    la, longest, nearest, cov, Rm = want
    assert np.array_equal(res['keys'], la) and np.array_equal(res['longest'], longest) and np.array_equal(res['nearest'], nearest)
    assert np.array_equal(np.asarray(res['coverage'], dtype=np.float64), cov, equal_nan=True)
    has = la > 0
    assert res['longest_max'] == longest.max() and res['longest_mean'] == float(longest.mean()) and res['longest_median'] == float(np.median(longest))
    assert res['coverage_mean'] == float(cov[has].mean())
    assert res['share_half_covered'] == float((cov[has] >= 0.5).sum()) / len(la) and res['share_with_run'] == float((longest >= min_run).sum()) / len(la)


def test_compare_to_corpus():
    _need_gpu()
    from pianobart_amd import novelty
    pad8, pitch_of, gen, cor = _sets()
    for mode, skip, min_run in (('exact', None, 8), ('interval', 4, 5)):
        want = _expect(gen, cor, pad8, pitch_of, mode, skip, min_run)
        res = novelty.compare_to_corpus(gen, cor, start=(skip, None), min_run=min_run, transpose=mode == 'interval', chunk=16, want_matrix=True)
        _check(res, want, min_run)
        assert np.array_equal(res['matrix'], want[4]) and res['n_gen'] == 24 and res['n_corpus'] == 40
        assert list(res['device_ms']) == ['keys', 'runs', 'total'] and res['device_ms']['total'] > 0
        if skip is None:
            assert res['longest'][3] == res['keys'][3] and res['nearest'][3] == 7 and res['coverage'][3] == 1.0 and res['longest'][5] >= 29
            assert res['longest'][6] < 29                                  # the transposed piece is not found by exact keys ...
        else:
            assert res['longest'][6] == res['keys'][6] and res['nearest'][6] == 0      # ... and whole by interval keys
    want = _expect(gen, None, pad8, pitch_of, 'exact', None, 8, exclude_self=True)
    res = novelty.compare_to_corpus(gen, None, exclude_self=True)
    _check(res, want, 8)
    assert res['nearest'][8] == 2 and res['nearest'][2] == 8 and res['longest'][2] == res['keys'][2]


def test_cli(tmp_path, capsys):
    _need_gpu()
    from pianobart_amd import eval_novelty
    pad8, pitch_of, gen, cor = _sets()
    g, g4, c, out = (str(tmp_path / n) for n in ('g.npy', 'g4.npy', 'c.npy', 'n.json'))
    np.save(g, gen.astype(np.float32))
    np.save(g4, gen.astype(np.float32).reshape(6, 4, 96, 8))               # what eval_generation --samples 4 writes
    np.save(c, cor.astype(np.int64))
    for argv, want in (
            (['--generated', g, '--corpus', c], _expect(gen, cor, pad8, pitch_of, 'exact', None, 8)),
            (['--generated', g4, '--corpus', c, '--skip', '4', '--transpose', '--min_run', '5'], _expect(gen, cor, pad8, pitch_of, 'interval', 4, 5)),
            (['--generated', g4, '--self', '--max_pieces', '20'], _expect(gen[:20], None, pad8, pitch_of, 'exact', None, 8, exclude_self=True))):
        res = eval_novelty.main(argv + ['--output', out])
        min_run = 5 if '--min_run' in argv else 8
        _check(res, want, min_run)
        text = capsys.readouterr().out
        assert text.count('[novelty]') >= 4 and 'max %d keys' % want[1].max() in text
        saved = json.load(open(out))
        assert saved['longest'] == want[1].tolist() and saved['nearest'] == want[2].tolist() and saved['keys'] == want[0].tolist()
        assert [None if v is None else float(v) for v in saved['coverage']] == [None if np.isnan(v) else float(v) for v in want[3]]
