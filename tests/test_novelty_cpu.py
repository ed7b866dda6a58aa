"""CPU: the host half of copy detection (pianobart_amd.novelty, eval_novelty) and the yardstick itself (tests/novelty_ref.py).

  * the restatement on hand-written pieces whose answers are stated here: a copy at the start, at the end and of the whole piece, a
    transposed copy (found by interval keys only), a copy whose second half is one bar late (the bar step breaks it), percussion, an
    early special id, start behind L;
  * the coverage rule on hand-built run_end rows (the restatement and novelty.coverage): overlapping runs, a run shorter than min_run,
    K = 0 -> nan;
  * the header declares and the library exports the new entries, the ABI version is still 10;
  * the C entries' argument checks (-2, the field named) before any device call, N = 0 / M = 0 being no error;
  * the CLI's refusals, and ops / novelty refusing host tensors."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from pianobart_amd import _lib, novelty, ops
from pianobart_amd._lib import PBError
from tests import novelty_ref as R

PAD8 = [256, 128, 129, 256, 128, 32, 254, 49]                             # the default dictionary: 128 pitched ids, then 128 percussion ids
PITCH_OF = np.array([i if i < 128 else -1 for i in range(256)], dtype=np.int16)


def piece(notes, S=12, extra=(0, 0, 0, 0, 0)):
    """(S, 8) ids: one row (bar, pos, ins, pitch, dur, vel, ts, tempo) per (bar, pos, pitch) note, an EOS row, PAD behind."""
    ins, dur, vel, ts, tempo = extra
    rows = [[bar, pos, ins, pit, dur, vel, ts, tempo] for bar, pos, pit in notes]
    rows.append([p + 3 for p in PAD8])
    rows += [list(PAD8)] * (S - len(rows))
    return np.array(rows[:S], dtype=np.int64)


# the corpus piece of the hand-written cases: eight notes over two bars, so seven keys
C = [(0, 0, 60), (0, 4, 62), (0, 8, 64), (0, 12, 65), (1, 0, 67), (1, 4, 69), (1, 8, 71), (1, 12, 72)]


def longest(gen_notes, mode, corpus_notes=C, **kw):
    a = R.keys_one(piece(gen_notes, **kw), PAD8, PITCH_OF, mode)
    b = R.keys_one(piece(corpus_notes), PAD8, PITCH_OF, mode)
    run = R.runs_ref(a, b)
    assert np.array_equal(run, R.runs_fast(a, b))
    return run, len(a)


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def test_key_layout():
    k = R.keys_one(piece([(3, 5, 60), (4, 7, 64), (4, 7, 200), (9, 0, 1), (8, 1, 2)]), PAD8, PITCH_OF, 'exact')
    assert k == [64 | 7 << 12 | 1 << 23, 200 | 7 << 12 | 0 << 23, 1 | 0 << 12 | 3 << 23, 2 | 1 << 12 | 3 << 23]      # steps 1, 0, 5 -> 3, -1 -> 3
    k = R.keys_one(piece([(3, 5, 60), (4, 7, 64), (4, 7, 200), (9, 0, 1), (8, 1, 2)]), PAD8, PITCH_OF, 'interval')
    assert [x & 0xFFF for x in k] == [1088 + 4, 2304 + 200, 2304 + 1, 1088 + 1] and all(x >> 25 == 0 for x in k)
    assert ops.HEAD_MAX == R.HEAD_MAX == 1088 and ops.NO_KEY == R.NO_KEY


def test_copy_at_the_start():
    run, K = longest(C[:4] + [(1, 0, 10), (1, 4, 11), (1, 8, 12)], 'exact')
    assert K == 6 and run.max() == 3 and list(run.max(axis=1)) == [1, 2, 3, 0, 0, 0]       # four notes = three keys


def test_copy_at_the_end():
    run, K = longest([(1, 0, 10), (1, 4, 11), (1, 8, 12)] + C[4:], 'exact')
    # the key of C's note 4 holds the bar step 1 from note 3; here the note before is in the same bar: that key differs, three are left
    assert K == 6 and run.max() == 3 and list(run.max(axis=1)) == [0, 0, 0, 1, 2, 3]


def test_copy_of_the_whole_piece_ignores_instrument_duration_velocity():
    run, K = longest(C, 'exact', extra=(5, 17, 9, 3, 20))
    assert K == 7 and run.max() == 7 and run[6, 6] == 7 and list(run.max(axis=1)) == [1, 2, 3, 4, 5, 6, 7]


def test_transposed_copy_is_found_by_interval_keys_only():
    up = [(bar, pos, pit + 5) for bar, pos, pit in C]
    assert longest(up, 'exact')[0].max() == 0
    assert longest(up, 'interval')[0].max() == 7
    assert longest(C, 'interval')[0].max() == 7


def test_second_half_one_bar_late_breaks_the_run():
    late = C[:4] + [(bar + 1, pos, pit) for bar, pos, pit in C[4:]]        # bars 0 0 0 0 2 2 2 2: the step into note 4 is 2, not 1
    run, K = longest(late, 'exact')
    assert K == 7 and run.max() == 3 and list(run.max(axis=1)) == [1, 2, 3, 0, 1, 2, 3]
    moved = [(bar + 1, pos, pit) for bar, pos, pit in C]                   # the whole piece one bar later keeps every step: still a copy
    assert longest(moved, 'exact')[0].max() == 7


def test_percussion():
    corpus = [(0, 0, 60), (0, 4, 62), (0, 8, 130), (0, 12, 64), (1, 0, 65)]
    same = longest(corpus, 'interval', corpus)[0]
    assert same.max() == 4
    up = [(0, 0, 65), (0, 4, 67), (0, 8, 130), (0, 12, 69), (1, 0, 70)]    # the pitched notes up by 5, the drum as it is
    run, K = longest(up, 'interval', corpus)
    # keys: interval +2 (same), drum id 130 (same), pitch id after a drum 69 vs 64 (differs), interval +1 (same)
    assert K == 4 and list(run.max(axis=1)) == [1, 2, 0, 1]
    assert longest(up, 'exact', corpus)[0].max() == 1                      # the drum alone


def test_an_early_special_id_and_start_behind_L():
    p = piece(C)
    p[3, 5] = PAD8[5]                                                      # one special id, one head: L = 3
    assert len(R.keys_one(p, PAD8, PITCH_OF, 'exact')) == 2
    keys, klen = R.keys_ref(np.stack([p, piece(C), piece(C), piece(C), piece([])]), PAD8, PITCH_OF, 'exact', start=[0, 6, 7, 11, 0])
    assert list(klen) == [2, 1, 0, 0, 0]                                   # start = L - 2, L - 1, behind L; a piece without a note
    assert (keys[0, 2:] == R.NO_KEY).all() and (keys[2:] == R.NO_KEY).all() and keys[1, 0] == R.keys_one(piece(C), PAD8, PITCH_OF, 'exact')[6]


def test_no_key_matches_nothing_and_ties_go_to_the_smallest_j():
    A = np.array([[5, 6, 7, R.NO_KEY]], dtype=np.uint32)
    B = np.array([[R.NO_KEY, 9, 9, 9], [6, 7, 1, 2], [5, 6, 3, 4], [5, 6, 7, 8]], dtype=np.uint32)
    Rm, run_end, best = R.outputs_ref(A, [4], B, [4, 4, 4, 4], table=R.runs_ref)
    assert Rm.tolist() == [[0, 2, 2, 3]] and run_end.tolist() == [[1, 2, 3, 0]] and best[0] == (3 << 32) | (0xFFFFFFFF - 3)
    Rm, run_end, best = R.outputs_ref(A, [4], B[:3], [4, 4, 4], min_run=2, j_base=10, table=R.runs_ref)
    assert run_end.tolist() == [[0, 2, 2, 0]] and best[0] == (2 << 32) | (0xFFFFFFFF - 11)      # j = 1 and j = 2 tie: 1 + j_base wins
    for table in (R.runs_fast, R._Rows):                                   # the restatement's quicker forms give what the plain loops give
        fast = R.outputs_ref(A, [4], B[:3], [4, 4, 4], min_run=2, j_base=10, table=table)
        assert all(np.array_equal(x, y) for x, y in zip(fast, (Rm, run_end, best)))
    assert novelty.split_best(best)[0].tolist() == [2] and novelty.split_best(best)[1].tolist() == [11]
    assert novelty.split_best(np.zeros(2, dtype=np.int64))[1].tolist() == [-1, -1]


# ---- coverage --------------------------------------------------------------------------------------------------------------------------
_COVER = [
    ([0, 0, 3, 0, 0, 0, 0, 0, 0, 0], 10, 0.3),                             # one run of 3 ending at key 2
    ([0, 0, 0, 0, 4, 0, 4, 0, 0, 0], 10, 0.6),                             # keys 1..4 and 3..6 overlap: 1..6
    ([0, 0, 0, 0, 0, 3, 4, 5, 0, 0], 10, 0.5),                             # one run of 5 ending at key 7, seen from min_run = 3 on: 3..7
    ([0, 0, 0, 0, 0, 0, 0, 0, 0, 0], 10, 0.0),
    ([1, 2, 3, 4], 4, 1.0),
    ([0, 0, 0, 9], 4, 1.0),                                                # a run longer than the row has keys before it
    ([5, 5, 5], 0, float('nan')),
]


@pytest.mark.parametrize('row,K,want', _COVER)
def test_coverage_rule(row, K, want):
    ref = R.coverage_ref(row, K)
    got = novelty.coverage(np.array([row, row]), np.array([K, K]))
    if math.isnan(want):
        assert math.isnan(ref) and np.isnan(got).all()
    else:
        assert ref == want and (got == want).all()


def test_a_run_shorter_than_min_run_covers_nothing():
    a = R.keys_one(piece(C[:4] + [(1, 0, 10), (1, 4, 11), (1, 8, 12)]), PAD8, PITCH_OF, 'exact')
    b = R.keys_one(piece(C), PAD8, PITCH_OF, 'exact')
    for min_run, want in ((3, 0.5), (4, 0.0)):
        _, run_end, _ = R.outputs_ref(np.array([a]), [6], np.array([b]), [7], min_run=min_run, table=R.runs_ref)
        assert R.coverage_ref(run_end[0], 6) == want and novelty.coverage(run_end, np.array([6]))[0] == want
    with pytest.raises(PBError):
        novelty.coverage(np.zeros((2, 3)), np.zeros(3))


# ---- the header and the library ---------------------------------------------------------------------------------------------------------
def test_the_entries_are_declared_and_exported():
    decls = _lib.parse_header()
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    assert decls['pb_piece_keys'] == (ctypes.c_int, [vp] * 6 + [i32] * 3 + [vp])
    assert decls['pb_shared_runs'] == (ctypes.c_int, [vp, vp, i32, i32, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, i32, vp])
    assert decls['pb_runs_tile'] == (ctypes.c_int, [])
    assert _lib.LIB.query('pb_abi_version') == 10
    assert _lib.LIB.query('pb_runs_tile') == ops.RUNS_TILE and ops.RUNS_MAX_S == 4096


PTR = 0x10000
_PAD = (ctypes.c_int32 * 8)(*PAD8)
_WIDE_PAD = (ctypes.c_int32 * 8)(256, 128, 129, 1100, 128, 32, 254, 49)


def _keys(**kw):
    a = dict(ids16=PTR, start=None, pad8=_PAD, pitch_of=PTR, keys=PTR, klen=PTR, N=4, S=16, mode=0, stream=None)
    a.update(kw)
    return tuple(a.values())


def _runs(**kw):
    a = dict(A=PTR, alen=PTR, N=4, Sa=16, B=PTR, blen=PTR, M=4, Sb=16, min_run=8, exclude_self=0, j_base=0, R=None, run_end=PTR, best=PTR,
             accumulate=0, stream=None)
    a.update(kw)
    return tuple(a.values())


_ENTRY_REFUSALS = [
    ('pb_piece_keys', _keys(S=0), 'S = 0'),
    ('pb_piece_keys', _keys(S=4097), 'S = 4097'),
    ('pb_piece_keys', _keys(mode=2), 'mode = 2'),
    ('pb_piece_keys', _keys(N=-1), 'N = -1'),
    ('pb_piece_keys', _keys(ids16=PTR + 8), 'ids16'),
    ('pb_piece_keys', _keys(pitch_of=None), 'pitch_of'),
    ('pb_piece_keys', _keys(keys=None), 'keys'),
    ('pb_piece_keys', _keys(keys=PTR + 2), 'keys'),
    ('pb_piece_keys', _keys(klen=None), 'klen'),
    ('pb_piece_keys', _keys(pad8=_WIDE_PAD), 'pad8[3] = 1100'),
    ('pb_shared_runs', _runs(Sa=0), 'Sa = 0'),
    ('pb_shared_runs', _runs(Sa=4097), 'Sa = 4097'),
    ('pb_shared_runs', _runs(Sb=0), 'Sb = 0'),
    ('pb_shared_runs', _runs(Sb=4097), 'Sb = 4097'),
    ('pb_shared_runs', _runs(min_run=0), 'min_run = 0'),
    ('pb_shared_runs', _runs(exclude_self=1, M=5), 'exclude_self needs N == M'),
    ('pb_shared_runs', _runs(exclude_self=2), 'exclude_self = 2'),
    ('pb_shared_runs', _runs(accumulate=2), 'accumulate = 2'),
    ('pb_shared_runs', _runs(j_base=-1), 'j_base = -1'),
    ('pb_shared_runs', _runs(N=-1), 'N = -1'),
    ('pb_shared_runs', _runs(run_end=None), 'run_end'),
    ('pb_shared_runs', _runs(best=None), 'best'),
    ('pb_shared_runs', _runs(best=PTR + 4), 'best'),
    ('pb_shared_runs', _runs(A=PTR + 2), 'A and alen'),
    ('pb_shared_runs', _runs(blen=None), 'B and blen'),
    ('pb_shared_runs', _runs(R=PTR + 1), 'R must'),
]


@pytest.mark.parametrize('entry,args,names', _ENTRY_REFUSALS, ids=['%s-%s-%d' % (e, n, i) for i, (e, _, n) in enumerate(_ENTRY_REFUSALS)])
def test_entries_check_their_arguments_before_any_device_call(entry, args, names):
    with pytest.raises(PBError) as e:
        _lib.LIB.call(entry, *args)
    assert entry in str(e.value) and '(-2)' in str(e.value) and names in str(e.value), str(e.value)


def test_empty_sides_are_no_error():
    _lib.LIB.call('pb_piece_keys', *_keys(N=0, ids16=None, keys=None, klen=None))
    _lib.LIB.call('pb_shared_runs', *_runs(N=0, A=None, alen=None, run_end=None, best=None))
    _lib.LIB.call('pb_shared_runs', *_runs(N=0, M=0, exclude_self=1))
    _lib.LIB.call('pb_shared_runs', *_runs(M=0, B=None, blen=None, accumulate=1))      # nothing to max in, nothing to clear: no device call


# ---- host refusals ------------------------------------------------------------------------------------------------------------------------
def test_host_tensors_are_refused():
    ids16, tab = torch.zeros(2, 4, 8, dtype=torch.int16), torch.zeros(256, dtype=torch.int16)
    k, n = torch.zeros(2, 4, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    for call in (lambda: ops.piece_keys(ids16, tab), lambda: ops.shared_runs(k, n, k, n),
                 lambda: novelty.piece_keys(torch.zeros(2, 4, 8, dtype=torch.int64)),
                 lambda: novelty.compare_to_corpus(torch.zeros(2, 4, 8, dtype=torch.int64), np.zeros((2, 4, 8), dtype=np.int64))):
        with pytest.raises(PBError, match='no CPU path'):
            call()


def test_host_checks():
    with pytest.raises(PBError, match=r'\(N, S, 8\)'):
        novelty.piece_keys(np.zeros((2, 4, 7), dtype=np.int64))
    with pytest.raises(PBError, match=r'head 3 \(Pitch\)'):
        novelty.piece_keys(np.full((1, 2, 8), 0, dtype=np.int64) + np.array([0, 0, 0, 300, 0, 0, 0, 0]))
    with pytest.raises(PBError, match='4097 rows'):
        novelty.piece_keys(np.zeros((1, 4097, 8), dtype=np.int64))
    k, n = torch.zeros(2, 4, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(PBError, match='min_run'):
        novelty.shared_runs(k, n, k, n, min_run=0)
    with pytest.raises(PBError, match='exclude_self'):
        novelty.shared_runs(k, n, k[:1], n[:1], exclude_self=True)


# ---- the CLI --------------------------------------------------------------------------------------------------------------------------------
def test_cli_refusals(tmp_path):
    from pianobart_amd import eval_novelty
    ok = R.synth_pieces(PAD8, 4, 12, seed=1).astype(np.float32)
    g, c, out = str(tmp_path / 'g.npy'), str(tmp_path / 'c.npy'), str(tmp_path / 'n.json')
    np.save(g, ok)
    np.save(c, ok)
    argv = ['--generated', g, '--corpus', c, '--output', out]
    with pytest.raises(PBError, match='--cpu'):
        eval_novelty.main(argv + ['--cpu'])
    with pytest.raises(PBError, match='no file'):
        eval_novelty.main(['--generated', str(tmp_path / 'missing.npy')] + argv[2:])
    with pytest.raises(PBError, match='no file'):
        eval_novelty.main(['--generated', g, '--corpus', str(tmp_path / 'missing.npy'), '--output', out])
    with pytest.raises(PBError, match='no file'):
        eval_novelty.main(argv + ['--dict_file', str(tmp_path / 'missing.json')])
    for flags in (['--min_run', '0'], ['--skip', '-1'], ['--max_pieces', '0'], ['--self']):
        with pytest.raises(PBError, match=flags[0]):
            eval_novelty.main(argv + flags)
    with pytest.raises(PBError, match='--corpus'):
        eval_novelty.main(['--generated', g, '--output', out])
    bad = str(tmp_path / 'bad.npy')
    np.save(bad, ok[:, :, :7])
    with pytest.raises(PBError, match='rows of 8 ids'):
        eval_novelty.main(['--generated', bad, '--corpus', c, '--output', out])
    with pytest.raises(PBError, match='rows of 8 ids'):
        eval_novelty.main(['--generated', g, '--corpus', bad, '--output', out])
    long = str(tmp_path / 'long.npy')
    np.save(long, np.zeros((1, 4097, 8), dtype=np.float32))
    with pytest.raises(PBError, match='4097 rows'):
        eval_novelty.main(['--generated', long, '--corpus', c, '--output', out])
    assert not os.path.exists(out)
