"""CPU: the host half of local alignment for copy detection (pianobart_amd.novelty, eval_novelty) and the yardstick
itself (tests/align_ref.py).

  * the two restatements (plain loops, anti-diagonals over all pairs at once) agree on random rows, and P >> 12 is textbook Smith-Waterman;
  * the contract's properties: score >= match * longest exact run, score(a, b) == score(b, a), a piece against itself scores match * K,
    every non-zero align_end has start <= p;
  * hand-worked cases whose numbers are written out here: a 12-key copy with one substitution, one inserted key, one deleted key, two
    alignments of equal score ending on one key (the smaller start wins), two corpus pieces of equal score (the smaller j + j_base wins);
  * novelty.split_align_end and novelty.align_coverage against the restatement's rule;
  * the header declares and the library exports the entries, the ABI version is still 10, pb_align_block == ops.ALIGN_BLOCK;
  * the C entry's argument checks (-2, the field named) before any device call, empty sides being no error; host and CLI refusals;
  * the random sets of the device tests are not trivially zero: at least 90 % of their pairs align beyond their longest exact run, and at
    least half of the align_end entries are non-zero at min_score = 8 (asserted on the restatement's own outputs)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from pianobart_amd import _lib, novelty, ops
from pianobart_amd._lib import PBError
from tests import align_ref as R

SCORINGS = [(1, 2, 2), (2, 1, 1), (8, 16, 16), (8, 1, 1), (1, 16, 1), (3, 2, 16)]


def pack(H, start):
    return H << 12 | (4095 - start)


def keys(*vals):
    return np.array(vals, dtype=np.uint32)


# ---- the restatements ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('scoring', SCORINGS)
def test_the_two_restatements_agree_and_the_score_is_smith_waterman(scoring):
    rng = np.random.default_rng(sum(scoring))
    for Ka, Kb in ((1, 1), (1, 9), (9, 1), (7, 12), (30, 17), (40, 40)):
        a, b = R.rows(rng, [Ka], Ka)[0], R.rows(rng, [Kb], Kb + 2)[0][:Kb]
        if Ka > 8:
            a[3] = R.NO_KEY                                              # a "no key" inside a row matches nothing, not even another one
            b[min(5, Kb - 1)] = R.NO_KEY
        P = R.table_ref(a, b, *scoring)
        assert np.array_equal(P >> 12, R.sw_unpacked(a, b, *scoring))
        score, rows = R.pair_ref(a, b, *scoring)
        fast_score, fast_rows = R.pair_fast(a, b, *scoring)
        assert score == fast_score and np.array_equal(rows, fast_rows)
        assert P.max() < 1 << 27
    A, B = R.rows(rng, [5, 0, 20, 13], 20), R.rows(rng, [11, 20, 0], 22)      # all pairs at once, ragged, against the plain loops pair by pair
    want = R.outputs_ref(A, [5, 0, 20, 13], B, [11, 20, 0], *scoring, min_score=3, pair=R.pair_ref)
    got = R.outputs_ref(A, [5, 0, 20, 13], B, [11, 20, 0], *scoring, min_score=3)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize('scoring', SCORINGS)
def test_properties(scoring):
    match = scoring[0]
    rng = np.random.default_rng(7 + sum(scoring))
    for Ka, Kb in ((12, 30), (33, 33), (50, 21)):
        a, b = R.rows(rng, [Ka], Ka)[0], R.rows(rng, [Kb], Kb)[0]
        score, rows = R.pair_fast(a, b, *scoring)
        assert score >= match * R.longest_runs(a, b)                     # an exact run is an alignment
        assert score == R.pair_fast(b, a, *scoring)[0]                   # the score is symmetric
        assert R.pair_fast(a, a, *scoring)[0] == match * Ka              # a piece against itself
        for p, v in enumerate(rows):
            H, start = R.split_ref(v)
            assert v == 0 or (H >= match and 0 <= start <= p)


# ---- hand-worked cases, default scoring (match 1, mismatch 2, gap 2) ---------------------------------------------------------------------
B12 = keys(*range(100, 112))                                             # twelve different keys


def _one(a, b=B12, **kw):
    score, align_end, best = R.outputs_ref(np.array([a]), [len(a)], np.array([b]), [len(b)], **kw)
    slow = R.outputs_ref(np.array([a]), [len(a)], np.array([b]), [len(b)], pair=R.pair_ref, **kw)
    assert np.array_equal(score, slow[0]) and np.array_equal(align_end, slow[1]) and np.array_equal(best, slow[2])
    return int(score[0, 0]), [R.split_ref(v) for v in align_end[0]], int(best[0])


def test_a_copy_with_one_substitution():
    a = B12.copy()
    a[5] = 999
    score, ends, best = _one(a)
    # five matches (5), the changed key (5 - 2 = 3), six matches more (9); the changed key itself is no match cell and records nothing
    assert score == 9 and best == 9 << 32 | 0xFFFFFFFF
    assert ends == [(1, 0), (2, 0), (3, 0), (4, 0), (5, 0), (0, None), (4, 0), (5, 0), (6, 0), (7, 0), (8, 0), (9, 0)]
    _, align_end, _ = R.outputs_ref(np.array([a]), [12], np.array([B12]), [12], min_score=8)
    assert align_end[0].tolist() == [0] * 10 + [pack(8, 0), pack(9, 0)] and R.coverage_ref(align_end[0], 12) == 1.0
    assert R.longest_runs(a, B12) == 6                                   # the exact measure sees 5 and 6: nothing from min_run = 8 on


def test_a_copy_with_one_inserted_key():
    a = np.concatenate([B12[:6], keys(999), B12[6:]])
    score, ends, _ = _one(a)
    # six matches (6), one gap (4), six matches more (10)
    assert score == 10 and ends == [(1, 0), (2, 0), (3, 0), (4, 0), (5, 0), (6, 0), (0, None), (5, 0), (6, 0), (7, 0), (8, 0), (9, 0), (10, 0)]


def test_a_copy_with_one_deleted_key():
    a = np.concatenate([B12[:6], B12[7:]])
    score, ends, _ = _one(a)
    # six matches (6), one gap over the corpus key that is missing (4), five matches more (9)
    assert score == 9 and ends == [(1, 0), (2, 0), (3, 0), (4, 0), (5, 0), (6, 0), (5, 0), (6, 0), (7, 0), (8, 0), (9, 0)]


def test_of_two_alignments_of_equal_score_the_smaller_start_wins():
    a = keys(1, 2, 3, 4, 5, 6, 7)
    whole = keys(1, 2, 3, 99, 5, 6, 7)                                   # keys 0 .. 6 with one substitution: 3 - 2 + 3 = 4, start 0
    tail = keys(4, 5, 6, 7)                                              # keys 3 .. 6 exactly: 4, start 3
    for B, blen in (([np.concatenate([tail, keys(50, 51, 52)]), whole], [4, 7]), ([np.concatenate([whole, keys(50, 51), tail])], [13])):
        score, align_end, _ = R.outputs_ref(np.array([a]), [7], np.array(B), blen, min_score=4)
        assert score.max() == 4 and (score == 4).all()
        assert align_end[0].tolist() == [0, 0, 0, 0, 0, 0, pack(4, 0)]   # as two corpus pieces and as two places in one
        assert R.coverage_ref(align_end[0], 7) == 1.0
    score, align_end, _ = R.outputs_ref(np.array([a]), [7], np.array([tail]), [4], min_score=4)
    assert align_end[0].tolist() == [0, 0, 0, 0, 0, 0, pack(4, 3)] and R.coverage_ref(align_end[0], 7) == 4 / 7
    assert [a.tolist() for a in novelty.split_align_end(align_end)] == [[[0, 0, 0, 0, 0, 0, 4]], [[-1, -1, -1, -1, -1, -1, 3]]]


def test_of_two_corpus_pieces_of_equal_score_the_smaller_j_wins():
    a = keys(1, 2, 3, 4, 5, 6, 7, R.NO_KEY)
    B = np.array([keys(R.NO_KEY, 9, 9, 9, 9, 9, 9, 9), keys(1, 2, 3, 99, 5, 6, 7, 0), keys(4, 5, 6, 7, 0, 0, 0, 0), keys(1, 2, 3, 4, 5, 0, 0, 0)])
    score, align_end, best = R.outputs_ref(np.array([a]), [8], B[:3], [8, 8, 8], j_base=10)
    assert score.tolist() == [[0, 4, 4]] and best[0] == 4 << 32 | (0xFFFFFFFF - 11)      # j = 1 and j = 2 tie: 1 + j_base wins
    assert novelty.split_best(best)[0].tolist() == [4] and novelty.split_best(best)[1].tolist() == [11]
    score, _, best = R.outputs_ref(np.array([a]), [8], B, [8, 8, 8, 8])
    assert score.tolist() == [[0, 4, 4, 5]] and best[0] == 5 << 32 | (0xFFFFFFFF - 3)
    score, _, best = R.outputs_ref(np.array([a, a, a, a]), [8, 8, 8, 8], B, [8, 8, 8, 8], exclude_self=True)
    assert score.tolist() == [[0, 4, 4, 5], [0, 0, 4, 5], [0, 4, 0, 5], [0, 4, 4, 0]] and best[3] == 4 << 32 | (0xFFFFFFFF - 1)


# ---- coverage ------------------------------------------------------------------------------------------------------------------------------
_COVER = [
    ([0, 0, pack(3, 0), 0, 0, 0, 0, 0, 0, 0], 10, 0.3),                   # one region, keys 0 .. 2
    ([0, 0, 0, 0, pack(3, 1), 0, pack(2, 3), 0, 0, 0], 10, 0.6),          # keys 1 .. 4 and 3 .. 6 overlap: 1 .. 6
    ([0, 0, 0, 0, 0, 0, 0, pack(9, 3), 0, 0], 10, 0.5),                   # the score says nothing about the extent: keys 3 .. 7
    ([0, 0, 0, 0, 0, pack(8, 5), 0, 0, 0, 0], 10, 0.1),                   # a region of one key
    ([0, 0, 0, 0, 0, 0, 0, 0, 0, 0], 10, 0.0),
    ([pack(1, 0), pack(2, 0), pack(3, 0), pack(4, 0)], 4, 1.0),
    ([0, 0, 0, pack(4, 0), pack(9, 0)], 4, 1.0),                          # entries behind the piece's keys do not count
    ([pack(5, 0)] * 3, 0, float('nan')),
]


@pytest.mark.parametrize('row,K,want', _COVER)
def test_coverage_rule(row, K, want):
    ref = R.coverage_ref(row, K)
    got = novelty.align_coverage(np.array([row, row]), np.array([K, K]))
    if math.isnan(want):
        assert math.isnan(ref) and np.isnan(got).all()
    else:
        assert ref == want and (got == want).all()


def test_coverage_and_split_on_the_restatements_outputs():
    A, alen, B, blen = R.tile_set(3, 5, seed=77)
    _, align_end, _ = R.outputs_ref(A, alen, B, blen, *R.GENTLE, min_score=8)
    got = novelty.align_coverage(torch.from_numpy(align_end), torch.from_numpy(alen))
    assert got.tolist() == [R.coverage_ref(align_end[i], int(alen[i])) for i in range(3)] and 0 < got.min()
    H, start = novelty.split_align_end(align_end)
    for i in range(3):
        assert [(int(h), None if s < 0 else int(s)) for h, s in zip(H[i], start[i])] == [R.split_ref(v) for v in align_end[i]]
    with pytest.raises(PBError):
        novelty.align_coverage(np.zeros((2, 3)), np.zeros(3))


# ---- the header and the library ---------------------------------------------------------------------------------------------------------
def test_the_entries_are_declared_and_exported():
    decls = _lib.parse_header()
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    assert decls['pb_local_align'] == (ctypes.c_int, [vp, vp, i32, i32, vp, vp, i32, i32] + [i32] * 6 + [vp, vp, vp, i32, vp])
    assert decls['pb_align_block'] == (ctypes.c_int, [])
    dll = _lib.LIB.load()
    assert dll.pb_local_align.argtypes == decls['pb_local_align'][1] and dll.pb_local_align.restype == ctypes.c_int
    assert _lib.LIB.query('pb_abi_version') == 10
    assert _lib.LIB.query('pb_align_block') == ops.ALIGN_BLOCK and ops.ALIGN_BLOCK % 64 == 0 and ops.ALIGN_TILE == ops.RUNS_TILE


PTR = 0x10000


def _align(**kw):
    a = dict(A=PTR, alen=PTR, N=4, Sa=16, B=PTR, blen=PTR, M=4, Sb=16, match=1, mismatch=2, gap=2, min_score=8, exclude_self=0, j_base=0,
             score=None, align_end=PTR, best=PTR, accumulate=0, stream=None)
    a.update(kw)
    return tuple(a.values())


_ENTRY_REFUSALS = [
    (_align(Sa=0), 'Sa = 0'),
    (_align(Sa=4097), 'Sa = 4097'),
    (_align(Sb=0), 'Sb = 0'),
    (_align(Sb=4097), 'Sb = 4097'),
    (_align(N=-1), 'N = -1'),
    (_align(M=-1), 'M = -1'),
    (_align(match=0), 'match = 0'),
    (_align(match=9), 'match = 9'),
    (_align(mismatch=0), 'mismatch = 0'),
    (_align(mismatch=17), 'mismatch = 17'),
    (_align(gap=0), 'gap = 0'),
    (_align(gap=17), 'gap = 17'),
    (_align(min_score=0), 'min_score = 0'),
    (_align(exclude_self=1, M=5), 'exclude_self needs N == M'),
    (_align(exclude_self=2), 'exclude_self = 2'),
    (_align(accumulate=2), 'accumulate = 2'),
    (_align(j_base=-1), 'j_base = -1'),
    (_align(A=None), 'A and alen'),
    (_align(A=PTR + 2), 'A and alen'),
    (_align(alen=None), 'A and alen'),
    (_align(B=PTR + 1), 'B and blen'),
    (_align(blen=None), 'B and blen'),
    (_align(score=PTR + 1), 'score must'),
    (_align(align_end=None), 'align_end'),
    (_align(align_end=PTR + 2), 'align_end'),
    (_align(best=None), 'best'),
    (_align(best=PTR + 4), 'best'),
]


@pytest.mark.parametrize('args,names', _ENTRY_REFUSALS, ids=['%s-%d' % (n, i) for i, (_, n) in enumerate(_ENTRY_REFUSALS)])
def test_the_entry_checks_its_arguments_before_any_device_call(args, names):
    with pytest.raises(PBError) as e:
        _lib.LIB.call('pb_local_align', *args)
    assert 'pb_local_align' in str(e.value) and '(-2)' in str(e.value) and names in str(e.value), str(e.value)


def test_empty_sides_are_no_error():
    _lib.LIB.call('pb_local_align', *_align(N=0, A=None, alen=None, align_end=None, best=None))
    _lib.LIB.call('pb_local_align', *_align(N=0, M=0, exclude_self=1))
    _lib.LIB.call('pb_local_align', *_align(M=0, B=None, blen=None, accumulate=1))       # nothing to max in, nothing to clear: no device call


# ---- host refusals ------------------------------------------------------------------------------------------------------------------------
def test_host_tensors_and_parameters_are_refused():
    k, n = torch.zeros(2, 4, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    for call in (lambda: ops.local_align(k, n, k, n), lambda: novelty.local_alignments(k, n, k, n)):
        with pytest.raises(PBError, match='no CPU path'):
            call()
    for kw, names in ((dict(match=0), 'match = 0'), (dict(match=9), 'match = 9'), (dict(mismatch=17), 'mismatch = 17'), (dict(gap=0), 'gap = 0'),
                      (dict(min_score=0), 'min_score = 0'), (dict(gap=1.5), 'gap = 1.5')):
        for fn in (ops.local_align, novelty.local_alignments):
            with pytest.raises(PBError, match=names):
                fn(k, n, k, n, **kw)
    with pytest.raises(PBError, match='exclude_self'):
        novelty.local_alignments(k, n, k[:1], n[:1], exclude_self=True)
    with pytest.raises(PBError, match='chunk'):
        novelty.local_alignments(k, n, k, n, chunk=0)
    ids = np.zeros((2, 4, 8), dtype=np.int64)
    for align in ({'match': 9}, {'bonus': 1}, 'yes'):
        with pytest.raises(PBError, match='match = 9|align is None'):
            novelty.compare_to_corpus(ids, ids, align=align)


# ---- the CLI --------------------------------------------------------------------------------------------------------------------------------
def test_cli_refusals(tmp_path):
    from pianobart_amd import eval_novelty
    g, c, out = str(tmp_path / 'g.npy'), str(tmp_path / 'c.npy'), str(tmp_path / 'n.json')
    np.save(g, np.zeros((2, 12, 8), dtype=np.float32))
    np.save(c, np.zeros((2, 12, 8), dtype=np.float32))
    argv = ['--generated', g, '--corpus', c, '--output', out]
    for flags, names in ((['--align_scores', '9,2,2'], 'match = 9'), (['--align_scores', '1,0,2'], 'mismatch = 0'), (['--align_scores', '1,2,17'], 'gap = 17'),
                         (['--align_scores', '1,2'], 'three integers'), (['--align_scores', '1,2,x'], 'three integers'),
                         (['--min_score', '0'], 'min_score = 0'), (['--align', '--min_score', '-3'], 'min_score = -3')):
        with pytest.raises(PBError, match=names):
            eval_novelty.main(argv + flags)
    assert not os.path.exists(out)
    args = eval_novelty.get_args(argv)
    assert eval_novelty._align_arg(args) is None                          # without the flags nothing is added to the call
    assert eval_novelty._align_arg(eval_novelty.get_args(argv + ['--align'])) == dict(match=1, mismatch=2, gap=2, min_score=8)
    assert eval_novelty._align_arg(eval_novelty.get_args(argv + ['--min_score', '5'])) == dict(match=1, mismatch=2, gap=2, min_score=5)
    assert eval_novelty._align_arg(eval_novelty.get_args(argv + ['--align_scores', '2,1,3'])) == dict(match=2, mismatch=1, gap=3, min_score=8)


# ---- the random sets of the device tests are worth testing -----------------------------------------------------------------------------------
def _not_trivial(A, alen, B, blen, score, align_end, best, pairs):
    align_end = R.at_min_score(align_end, 8)
    beyond = [score[i, j] > R.GENTLE[0] * R.longest_runs(A[i][:alen[i]], B[j][:blen[j]]) for i, j in pairs]
    assert np.mean(beyond) >= 0.9, np.mean(beyond)
    filled = np.concatenate([align_end[i, :alen[i]] != 0 for i in sorted({i for i, _ in pairs})])
    assert filled.mean() >= 0.5, filled.mean()


def test_the_edge_set_aligns_beyond_its_exact_runs():
    """Of the pairs of the device test over every pair of lengths, those with at least 64 keys on both sides: a row of 0 .. 5 keys cannot
    score beyond its few keys, whatever the other side holds."""
    out = R.edge_outputs(ops.ALIGN_BLOCK)
    alen, blen = out[1], out[3]
    assert list(alen) == [0, 1, 2, 4, 5, 255, 256, 257, 513, 1023]
    _not_trivial(*out, [(i, j) for i in range(len(alen)) for j in range(len(blen)) if alen[i] >= 64 and blen[j] >= 64])


@pytest.mark.parametrize('N', [1, 3])
@pytest.mark.parametrize('M', [1, 31, 32, 33, 65])
def test_the_tile_sets_align_beyond_their_exact_runs(N, M):
    assert ops.ALIGN_TILE == 32
    _not_trivial(*R.tile_outputs(N, M, seed=100 * N + M), [(i, j) for i in range(N) for j in range(M)])
