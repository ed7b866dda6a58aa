"""GPU: pb_local_align (csrc/pb_align.hip) and the alignment half of pianobart_amd.novelty against the restatement of tests/align_ref.py
(DESIGN.md 12). Everything is an integer: every comparison is ==, there is no tolerance. W = ops.ALIGN_BLOCK is the B columns one sweep
of a wave covers, c = W / 64 the columns of a lane, T = ops.ALIGN_TILE the corpus pieces of a workgroup.

  * every pair of K_a, K_b in 0, 1, 2, c, c + 1, W - 1, W, W + 1, 2 W + 1, 1 023 in one call (Sa != Sb), random rows over a 3-pitch x
    2-position alphabet under the gentle scoring (2, 1, 1) (tests/test_align_cpu.py shows that these rows align far beyond their exact
    runs), and one pair of 4 095 x 4 095 keys;
  * planted copies of 40 keys among keys that are all different, default scoring: one substitution, one inserted key, one deleted key,
    two adjacent substitutions, the edited corpus column at q = 0, c - 1, c, W - 1, W, W + 1 and K_b - 1, and a generated piece that is
    nothing but the copy (it starts at p = 0 and ends at K_a - 1); away from the edges the scores are 37, 38, 37 and 34;
  * N = 1, 3 against M = 1, T - 1, T, T + 1, 2 T + 1 with a duplicated corpus row (a tie in best: the smallest j wins), score = NULL, two
    calls giving equal bytes; min_score = 1, best, best + 1 and beyond every score; the extremes (8, 16, 16); a 4 095-key piece against
    itself (H = 32 760); exclude_self; chunks in two orders bit-equal to one shot; empty sides;
  * score >= match * R against pb_shared_runs on the same keys, and score(a, b) == score(b, a);
  * end to end: compare_to_corpus(align=...) and the CLI on 24 x 40 pieces of 96 rows against the restatement, with and without
    --transpose; a verbatim copy, a copy with every 7th pitch changed and an unrelated piece; without `align` the result holds exactly
    the keys it held before."""
import json

import numpy as np
import pytest
import torch

from tests import align_ref as R
from tests import novelty_ref as NR
from tests.vocab_layout_util import D_DEFAULT

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _t(k):
    return _dev(np.ascontiguousarray(k).view(np.int32))


def _l(n):
    return _dev(np.asarray(n, dtype=np.int32))


def _call(A, alen, B, blen, scoring=R.GENTLE, **kw):
    from pianobart_amd import ops
    return ops.local_align(_t(A), _l(alen), _t(B), _l(blen), *scoring, **kw)


def _same(got, want):
    return got.dtype in (torch.int32, torch.int64) and np.array_equal(got.cpu().numpy().astype(np.int64), want)


def _all_same(got, want):
    return all(_same(g, w) for g, w in zip(got, want))


# ---- every length edge ------------------------------------------------------------------------------------------------------------------
def test_every_pair_of_lengths():
    _need_gpu()
    from pianobart_amd import ops
    A, alen, B, blen, want_score, want_end, want_best = R.edge_outputs(ops.ALIGN_BLOCK)
    assert want_score[9, 9] > 300 and want_score[1, 4] == 2 and (want_score[0] == 0).all()
    got = _call(A, alen, B, blen, min_score=1)
    assert _all_same(got, (want_score, want_end, want_best))
    got = _call(A, alen, B, blen, min_score=8)
    assert _all_same(got, (want_score, R.at_min_score(want_end, 8), want_best))


def _long_pair():
    def make():
        rng = np.random.default_rng(41)
        A, B = R.rows(rng, [4095], 4096), R.rows(rng, [4095], 4095)
        A[0, 3000:3100] = B[0, 500:600]                                    # a copy far off the main diagonal, blocks apart
        return (A, B) + R.outputs_ref(A, [4095], B, [4095], *R.GENTLE, min_score=1)
    return R.cached('long', make)


def test_one_pair_of_4095_keys():
    _need_gpu()
    A, B, want_score, want_end, want_best = _long_pair()
    assert want_score[0, 0] > 1000
    got = _call(A, [4095], B, [4095], min_score=1)
    assert _all_same(got, (want_score, want_end, want_best))
    got = _call(A, [5000], B, [4096], min_score=1)                         # lengths are clamped to the windows
    assert _same(got[0], R.outputs_ref(A, [4096], B, [4095], *R.GENTLE)[0]) and got[0][0, 0] == want_score[0, 0]      # A's last entry is no key


def test_a_piece_of_4095_keys_against_itself():
    _need_gpu()
    A = _long_pair()[0]
    want = R.cached('self', lambda: R.outputs_ref(A, [4095], A, [4095], 8, 16, 16, min_score=1))
    assert want[0][0, 0] == 8 * 4095 == 32760 and want[2][0] == 32760 << 32 | 0xFFFFFFFF
    got = _call(A, [4095], A, [4095], scoring=(8, 16, 16), min_score=1)
    assert _all_same(got, want)
    assert _same(_call(A, [4095], A, [4095], scoring=(8, 16, 16), min_score=32760)[1], R.at_min_score(want[1], 32760))
    assert int(_call(A, [4095], A, [4095], scoring=(8, 16, 16), min_score=32761)[1].abs().sum()) == 0


# ---- planted copies with edits -------------------------------------------------------------------------------------------------------------
EDITS = ('substitution', 'insertion', 'deletion', 'two adjacent')
INTERIOR = {'substitution': 37, 'insertion': 38, 'deletion': 37, 'two adjacent': 34}      # 39 - 2, 40 - 2, 39 - 2, 38 - 4


def _planted(W):
    """(cases, A, alen, B, blen): per case a corpus row of 2 W + 40 different keys and a generated row that holds 40 of them with one
    edit, the edited corpus column at q. No key occurs in two rows, so the pairs i != j share nothing."""
    c, Kb = W // 64, 2 * W + 40
    cases = [(e, q, False) for e in EDITS for q in (0, c - 1, c, W - 1, W, W + 1, Kb - 1)] + [(e, W, True) for e in EDITS]
    n, Sa = len(cases), 104
    B = R.distinct_keys(n * Kb).reshape(n, Kb)
    fresh = iter(R.distinct_keys(n * 80, lo=n * Kb))
    A, alen = np.full((n, Sa), R.NO_KEY, dtype=np.uint32), np.zeros(n, dtype=np.int64)
    for k, (edit, q, bare) in enumerate(cases):
        qs = min(max(q - 20, 0), Kb - 40)
        copy, at = list(B[k, qs:qs + 40]), q - qs
        if edit == 'substitution':
            copy[at] = next(fresh)
        elif edit == 'insertion':
            copy.insert(at, next(fresh))
        elif edit == 'deletion':
            del copy[at]
        else:
            copy[at], copy[at + 1 if at < 39 else at - 1] = next(fresh), next(fresh)
        row = copy if bare else [next(fresh) for _ in range(30)] + copy + [next(fresh) for _ in range(30)]
        A[k, :len(row)], alen[k] = row, len(row)
    return cases, A, alen, B, np.full(n, Kb)


def test_planted_copies_with_one_edit():
    _need_gpu()
    from pianobart_amd import ops
    cases, A, alen, B, blen = _planted(ops.ALIGN_BLOCK)
    n = len(cases)
    want_score, want_end, want_best = np.zeros((n, n), dtype=np.int64), np.zeros(A.shape, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for k in range(n):                                                     # the pairs i != j share no key: they score 0
        s, e, b = R.outputs_ref(A[k:k + 1], alen[k:k + 1], B[k:k + 1], blen[k:k + 1], min_score=8, j_base=k)
        want_score[k, k], want_end[k], want_best[k] = s[0, 0], e[0], b[0]
    for k, (edit, q, bare) in enumerate(cases):
        if 5 <= q - min(max(q - 20, 0), blen[k] - 40) <= 33:               # the edit is inside the copy, more than its price from both ends
            assert want_score[k, k] == INTERIOR[edit], (edit, q, want_score[k, k])
            p_end = int(np.nonzero(want_end[k])[0].max())
            assert R.split_ref(want_end[k, p_end]) == (INTERIOR[edit], 0 if bare else 30) and p_end == alen[k] - (1 if bare else 31)
        assert want_score[k, k] >= 33
    got = _call(A, alen, B, blen, scoring=R.DEFAULTS, min_score=8)
    assert _all_same(got, (want_score, want_end, want_best))


# ---- tiles, ties, no matrix ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [1, 3])
@pytest.mark.parametrize('M', ['1', 'T-1', 'T', 'T+1', '2T+1'])
def test_tiles_ties_and_no_matrix(N, M):
    _need_gpu()
    from pianobart_amd import novelty, ops
    T = ops.ALIGN_TILE
    M = {'1': 1, 'T-1': T - 1, 'T': T, 'T+1': T + 1, '2T+1': 2 * T + 1}[M]
    A, alen, B, blen, want_score, want_end, want_best = R.tile_outputs(N, M, seed=100 * N + M)
    want = (want_score, R.at_min_score(want_end, 8), want_best)
    got = _call(A, alen, B, blen, min_score=8)
    assert _all_same(got, want)
    if M > 2:                                                              # corpus rows 1 and M - 1 are equal and generated row 0 repeats them
        assert novelty.split_best(got[2])[1][0] == 1 and want_score[0, 1] == want_score[0, M - 1] == want_score[0].max() == 2 * 61
    none = _call(A, alen, B, blen, min_score=8, want_matrix=False)         # score = NULL
    assert none[0] is None and torch.equal(none[1], got[1]) and torch.equal(none[2], got[2])
    again = _call(A, alen, B, blen, min_score=8)                           # equal inputs, equal bytes
    assert all(torch.equal(x, y) for x, y in zip(again, got))


def test_min_score():
    _need_gpu()
    A, alen, B, blen, want_score, want_end, want_best = R.tile_outputs(3, 33, seed=333)
    rows = [1, 2]                                                          # row 0 holds a whole corpus row; these two hold what chance gives
    top = int(want_score[rows].max())
    for min_score in (1, top, top + 1, 2 ** 31 - 1):
        got = _call(A[rows], alen[rows], B, blen, min_score=min_score)
        want = R.at_min_score(want_end[rows], min_score)
        assert (want > 0).any() == (min_score <= top)
        assert _all_same(got, (want_score[rows], want, want_best[rows]))


def test_the_extreme_scoring():
    _need_gpu()
    A, alen, B, blen = R.tile_set(3, 5, seed=88)
    A[2, 10:40] = B[3, 5:35]                                               # thirty keys of a corpus row, with two of them changed
    A[2, 20], A[2, 30] = R.NO_KEY, 7
    for scoring in ((8, 16, 16), (8, 1, 1), (1, 16, 16)):
        want = R.outputs_ref(A, alen, B, blen, *scoring, min_score=8)
        assert want[0].max() >= 8
        assert _all_same(_call(A, alen, B, blen, scoring=scoring, min_score=8), want)


def test_exclude_self():
    _need_gpu()
    from pianobart_amd import ops
    N = ops.ALIGN_TILE + 1
    A, alen, _, _ = R.tile_set(N, 1, seed=3)
    A[7], alen[7] = A[20], alen[20]                                        # a duplicate: each finds the other, not itself
    want = R.outputs_ref(A, alen, A, alen, *R.GENTLE, min_score=8, exclude_self=True)
    got = _call(A, alen, A, alen, min_score=8, exclude_self=True)
    assert _all_same(got, want)
    assert (np.diag(want[0]) == 0).all() and want[0][7, 20] == 2 * alen[20] and want[2][7] == (2 * alen[20] << 32) | (0xFFFFFFFF - 20)
    full = _call(A, alen, A, alen, min_score=8)
    assert (np.diag(full[0].cpu().numpy()) == 2 * alen).all()              # a piece against itself scores match * K


def test_chunked_accumulation_is_the_one_shot_call():
    _need_gpu()
    from pianobart_amd import novelty, ops
    N, M = 3, 2 * ops.ALIGN_TILE + 1
    A, alen, B, blen, want_score, want_end, want_best = R.tile_outputs(N, M, seed=100 * N + M)
    one = _call(A, alen, B, blen, min_score=8)
    assert _all_same(one, (want_score, R.at_min_score(want_end, 8), want_best))
    for order in ((0, 20, 40, 60), (60, 40, 0, 20)):                       # chunks of 20 (and 5) pieces, in two orders
        align_end = best = None
        scores = {}
        for j0 in order:
            scores[j0], align_end, best = _call(A, alen, B[j0:j0 + 20], blen[j0:j0 + 20], min_score=8, j_base=j0, align_end=align_end, best=best)
        assert torch.equal(torch.cat([scores[j0] for j0 in sorted(scores)], dim=1), one[0])
        assert torch.equal(align_end, one[1]) and torch.equal(best, one[2])
    host = novelty.local_alignments(_t(A), _l(alen), _t(B), _l(blen), *R.GENTLE, min_score=8, chunk=20, want_matrix=True)
    assert all(torch.equal(x, y) for x, y in zip(host, one))


def test_empty_sides():
    _need_gpu()
    A, alen, B, blen = R.tile_set(3, 4, seed=2)
    score, align_end, best = _call(A, alen, B[:0], blen[:0], min_score=1)
    assert tuple(score.shape) == (3, 0) and int(align_end.abs().sum()) == 0 and int(best.abs().sum()) == 0      # cleared, on the stream
    score, align_end, best = _call(A[:0], alen[:0], B, blen, min_score=1)
    assert tuple(score.shape) == (0, 4) and tuple(align_end.shape) == (0, 64) and tuple(best.shape) == (0,)
    score, align_end, best = _call(A, np.zeros(3), B, blen, min_score=1)   # pieces without keys
    assert int(score.abs().sum()) == 0 and int(align_end.abs().sum()) == 0 and int(best.abs().sum()) == 0
    score, align_end, best = _call(A, alen, B, np.zeros(4), min_score=1)
    assert int(score.abs().sum()) == 0 and int(align_end.abs().sum()) == 0 and int(best.abs().sum()) == 0


def test_an_exact_run_is_an_alignment_and_the_score_is_symmetric():
    _need_gpu()
    from pianobart_amd import ops
    A, alen, B, blen = R.edge_set(ops.ALIGN_BLOCK)[:4]
    for scoring in (R.GENTLE, R.DEFAULTS):
        score = _call(A, alen, B, blen, scoring=scoring, min_score=1)[0]
        runs = ops.shared_runs(_t(A), _l(alen), _t(B), _l(blen), min_run=1)[0]
        assert bool((score >= scoring[0] * runs).all()) and int(runs.max()) >= 7
        back = _call(B, blen, A, alen, scoring=scoring, min_score=1)[0]
        assert torch.equal(back.t().contiguous(), score)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
def _sets():
    pad8 = [n - 6 for n in D_DEFAULT]
    pitch_of = np.array([i if i < 128 else -1 for i in range(pad8[3])])
    kw = dict(pitches=[60, 62, 64, 130], positions=[0, 4, 8])
    gen, cor = NR.synth_pieces(pad8, 24, 96, seed=21, **kw), NR.synth_pieces(pad8, 40, 96, seed=22, **kw)
    cor[7], cor[9] = NR.synth_pieces(pad8, 1, 96, seed=23, **kw)[0], NR.synth_pieces(pad8, 1, 96, seed=25, **kw)[0]      # both fill the window
    gen[3] = cor[7]                                                        # a verbatim piece
    gen[4] = cor[9]
    gen[4, 3::7, 3] = np.where(gen[4, 3::7, 3] == 62, 64, 62)              # a piece with every 7th pitch changed
    gen[5, 10:40] = cor[7, 20:50]                                          # thirty notes of a corpus piece ...
    gen[5, 25] = gen[5, 24]                                                # ... one of them replaced
    gen[6] = np.delete(np.concatenate([cor[9], cor[9][-1:]]), 40, axis=0)  # a piece with one note dropped
    return pad8, pitch_of, gen, cor


def _expect(gen, cor, pad8, pitch_of, mode, skip, par, exclude_self=False):
    ka, la = NR.keys_ref(gen, pad8, pitch_of, mode, skip)
    kb, lb = (ka, la) if exclude_self else NR.keys_ref(cor, pad8, pitch_of, mode)
    score, align_end, best = R.outputs_ref(ka, la, kb, lb, par['match'], par['mismatch'], par['gap'], par['min_score'], exclude_self=exclude_self)
    top = score.max(axis=1)
    nearest = np.where(top > 0, score.argmax(axis=1), -1)
    cov = np.array([R.coverage_ref(align_end[i], int(la[i])) for i in range(len(la))])
    span = np.array([max([p - R.split_ref(v)[1] + 1 for p, v in enumerate(align_end[i]) if v] or [0]) for i in range(len(la))])
    return la, top, nearest, cov, span, score


def _check(res, want, par):
    la, top, nearest, cov, span, score = want
    assert dict(res['align_params']) == par and list(res['align_params']) == ['match', 'mismatch', 'gap', 'min_score']
    assert np.array_equal(res['keys'], la) and np.array_equal(res['align_score'], top) and np.array_equal(res['align_nearest'], nearest)
    assert np.array_equal(np.asarray(res['align_coverage'], dtype=np.float64), cov, equal_nan=True) and np.array_equal(res['align_span'], span)
    has = la > 0
    assert res['align_score_max'] == top.max() and res['align_score_mean'] == float(top.mean()) and res['align_score_median'] == float(np.median(top))
    assert res['align_coverage_mean'] == float(cov[has].mean())
    assert res['share_half_aligned'] == float((cov[has] >= 0.5).sum()) / len(la)
    assert res['share_with_alignment'] == float((top >= par['min_score']).sum()) / len(la)
    assert list(res['device_ms']) == ['keys', 'runs', 'align', 'total'] and res['device_ms']['align'] > 0


OLD_KEYS = ['n_gen', 'n_corpus', 'min_run', 'transpose', 'exclude_self', 'keys', 'longest', 'nearest', 'coverage', 'longest_mean', 'longest_median',
            'longest_max', 'coverage_mean', 'share_half_covered', 'share_with_run', 'device_ms']
DEFAULT_PAR = dict(match=1, mismatch=2, gap=2, min_score=8)


def test_compare_to_corpus():
    _need_gpu()
    from pianobart_amd import novelty
    pad8, pitch_of, gen, cor = _sets()
    plain = novelty.compare_to_corpus(gen, cor)
    assert list(plain) == OLD_KEYS and list(plain['device_ms']) == ['keys', 'runs', 'total']      # without align: exactly the keys of before
    assert list(novelty.compare_to_corpus(gen, cor, want_matrix=True)) == OLD_KEYS + ['matrix']
    for mode, skip, align in (('exact', None, True), ('interval', 4, dict(match=2, mismatch=1, gap=1, min_score=12))):
        par = dict(DEFAULT_PAR) if align is True else align
        want = _expect(gen, cor, pad8, pitch_of, mode, skip, par)
        res = novelty.compare_to_corpus(gen, cor, start=(skip, None), transpose=mode == 'interval', chunk=16, want_matrix=True, align=align)
        _check(res, want, par)
        assert list(res)[:len(OLD_KEYS)] == OLD_KEYS and np.array_equal(res['align_matrix'], want[5])
        for k in OLD_KEYS[:-1]:                                            # what was there is what it was
            same = np.array_equal(res[k], plain[k], equal_nan=True) if isinstance(plain[k], np.ndarray) else res[k] == plain[k] or plain[k] != plain[k]
            assert same or mode == 'interval'
        if mode == 'exact':
            K = res['keys']
            assert res['align_score'][3] == K[3] == 95 and res['align_nearest'][3] == 7 and res['align_coverage'][3] == 1.0 and res['align_span'][3] == 95
            assert res['align_nearest'][4] == 9 and res['align_coverage'][4] >= 0.9 and res['longest'][4] < 8 <= res['align_score'][4]
            assert res['align_nearest'][6] == 9 and res['align_score'][6] >= 90 and res['longest'][6] < 60
            assert res['align_score'][5] >= 29 - 2 - 2                     # the replaced note changes its own key and the step of the next
    par = dict(DEFAULT_PAR)
    want = _expect(gen, None, pad8, pitch_of, 'exact', None, par, exclude_self=True)
    res = novelty.compare_to_corpus(gen, None, exclude_self=True, align=True)
    _check(res, want, par)
    assert res['align_nearest'][4] == 6 and res['align_nearest'][6] == 4   # the two edited copies of one corpus piece find each other


def test_cli(tmp_path, capsys):
    _need_gpu()
    from pianobart_amd import eval_novelty
    pad8, pitch_of, gen, cor = _sets()
    g, c, out, old = (str(tmp_path / n) for n in ('g.npy', 'c.npy', 'n.json', 'old.json'))
    np.save(g, gen.astype(np.float32))
    np.save(c, cor.astype(np.int64))
    plain = eval_novelty.main(['--generated', g, '--corpus', c, '--output', old])
    assert list(plain) == OLD_KEYS and list(json.load(open(old))) == OLD_KEYS and capsys.readouterr().out.count('[novelty]') == 5
    for argv, mode, skip, par in (
            (['--align'], 'exact', None, dict(DEFAULT_PAR)),
            (['--transpose', '--skip', '4', '--align_scores', '2,1,1', '--min_score', '12'], 'interval', 4, dict(match=2, mismatch=1, gap=1, min_score=12)),
            (['--min_score', '20'], 'exact', None, dict(DEFAULT_PAR, min_score=20))):
        want = _expect(gen, cor, pad8, pitch_of, mode, skip, par)
        res = eval_novelty.main(['--generated', g, '--corpus', c, '--output', out] + argv)
        _check(res, want, par)
        text = capsys.readouterr().out
        assert text.count('[novelty]') == 7 and 'max %d;' % want[1].max() in text and 'alignment >= %d' % par['min_score'] in text
        saved = json.load(open(out))
        assert list(saved)[:len(OLD_KEYS)] == OLD_KEYS and saved['align_params'] == par
        assert saved['align_score'] == want[1].tolist() and saved['align_nearest'] == want[2].tolist() and saved['align_span'] == want[4].tolist()
        assert [None if v is None else float(v) for v in saved['align_coverage']] == [None if np.isnan(v) else float(v) for v in want[3]]
        if mode == 'exact':
            assert all(saved[k] == json.load(open(old))[k] for k in OLD_KEYS[:-1])


def test_a_copy_with_every_7th_pitch_changed_is_found():
    """A verbatim copy, a copy with every 7th pitch changed and an unrelated piece, default flags: the first two are aligned with a
    coverage near 1, the third is not, and only the verbatim one holds an exact run that counts."""
    _need_gpu()
    from pianobart_amd import novelty
    pad8 = [n - 6 for n in D_DEFAULT]
    cor = NR.synth_pieces(pad8, 6, 96, seed=51)
    cor[2] = NR.synth_pieces(pad8, 1, 96, seed=52)[0]
    cor[2, :, 3] %= 120
    gen = np.stack([cor[2], cor[2], NR.synth_pieces(pad8, 1, 96, seed=53)[0]])
    gen[1, 6::7, 3] += 1
    res = novelty.compare_to_corpus(gen, cor, align=True)
    assert res['keys'].tolist() == [95, 95, 95]
    assert res['longest'].tolist()[:2] == [95, 6] and res['longest'][2] <= 1 and res['share_with_run'] == 1 / 3
    assert res['align_score'].tolist()[:2] == [95, 95 - 13 - 2 * 13] and res['align_nearest'].tolist() == [2, 2, -1 if res['align_score'][2] == 0 else res['align_nearest'][2]]
    assert res['align_coverage'][0] == 1.0 and res['align_coverage'][1] == 1.0 and res['align_coverage'][2] == 0.0 and res['align_score'][2] <= 1
    assert res['share_with_alignment'] == 2 / 3 and res['share_half_aligned'] == 2 / 3 and res['align_span'].tolist() == [95, 95, 0]
