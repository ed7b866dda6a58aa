"""GPU: the corruption kernel (csrc/pb_corrupt.hip) against tests/corrupt_ref.py, exactly, at every length edge.

The kernel is an integer kernel: every comparison here is np.array_equal and there is no tolerance anywhere. `out` and `loss_mask` are
views inside larger allocations whose guards hold a sentinel (int16 -31111, float 1.5 * 2^-20); the inside starts as the sentinel
(int16) or NaN (float). After every call the guards are untouched, every inside element is written, the input ids are unchanged and
the 8 columns of every loss row are equal.
  * Philox path: pb_corrupt == apply(decide()) for the five choices and the in-kernel choice draw (choice 0 and choice NULL, choice_out
    compared), B = 6, at the lengths of corrupt_ref.GRID: both sides of one, two, four and eight trips of the 256-thread loops, and
    where S * 0.15 lands on .5; p = 0.5 and 0.9 at S = 3, 64, 257 (spans pass the end; at S = 3 a first attempt overflows). One launch
    of B = 300 mixed choices, each sample under its own index. The seeds whose keys hold a tie (found on the CPU): two positions at
    S = 2048, under a mask_percent that puts the cut between the two, and two bar values.
  * Replay path: pb_corrupt_replay == apply() on hand-made decisions at S = 64, 257, 1024, 2048: infilling that overflows on all ten
    attempts, on nine, by exactly one row, that fits exactly, a span past the end and one at the last step; deletion from index 0 and
    of index S - 1 alone; rotation by 0, 1, S - 1; one bar, 256 bars reversed, the identity order; every position a random row, no
    position selected. S = 0 and S = 2049 are refused.
  * The oracle differential of test_corrupt_gpu.py at S = 257 and S = 1024, a dozen sequences each.

Scratch builds of the library, one change each, and what fails on them of the 30 tests of this file (tests/test_corrupt_gpu.py passes
on (a), (c) and (d); its test_token_mask_counts fails on (b)):
  (a) the APPLY loop of the mask (`for (i = t; i < S; i += CT)` behind the kinds) takes a single trip: 14 fail, every Philox case above
      S = 256 (8), the tie test, the hand-made replay at S = 257, 1024, 2048 and the oracle differential at S = 257 and 1024;
  (b) `rank < k80` becomes `rank <= k80`: 17 fail, every Philox case with k80 < k (15), the B = 300 launch and the tie test;
  (c) the Poisson recurrence uses `2.0f / pz`: 17 fail, every Philox case in which some sample starts a span (16) and the B = 300 launch;
  (d) rank_of breaks ties by `j > i`: 1 fails, the tie test (sample 2, deletion under tie_percent()).
"""
import numpy as np
import pytest
import torch

from tests import corrupt_ref as R
from tests.golden_util import N_TOK, PAD

pytestmark = pytest.mark.gpu
MASK, EOS = PAD + 1, PAD + 3
GUARD = 256
I16_SENTINEL, F32_SENTINEL = -31111, 1.5 * 2.0 ** -20


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from pianobart_amd import ops as o
    return o


def _guarded(n, dtype):
    sentinel = I16_SENTINEL if dtype == torch.int16 else F32_SENTINEL
    buf = torch.full((GUARD + n + GUARD,), sentinel, dtype=dtype, device='cuda')
    if dtype != torch.int16:
        buf[GUARD:GUARD + n] = float('nan')
    return buf, buf[GUARD:GUARD + n]


def _guards_hold(buf, n):
    sentinel = I16_SENTINEL if buf.dtype == torch.int16 else F32_SENTINEL
    g = torch.cat([buf[:GUARD], buf[GUARD + n:]])
    return bool((g == sentinel).all())


def _launch(ops, ids, p, choice=None, seed=None, dec=None, rand_rows=None, want_choice=True):
    """One pb_corrupt (seed given) or pb_corrupt_replay (dec given) call on ids (B,S,8) with every buffer check of the module docstring.
    Returns (out (B,S,8) int64, loss (B,S) int64, choice_out or None)."""
    B, S = ids.shape[:2]
    n = B * S * 8
    ids16 = torch.from_numpy(ids.astype(np.int16)).cuda().reshape(B, S, 8)
    before = ids16.clone()
    obuf, oin = _guarded(n, torch.int16)
    lbuf, lin = _guarded(n, torch.float32)
    ch = None if choice is None else torch.tensor(choice, dtype=torch.int32, device='cuda')
    cho = torch.full((B + 2,), -9, dtype=torch.int32, device='cuda')
    if dec is None:
        ops.corrupt(ids16, oin.view(B, S, 8), lin.view(B, S, 8), ch, cho[1:B + 1] if want_choice else None, p, seed, PAD, MASK, N_TOK)
    else:
        rr = None if rand_rows is None else torch.from_numpy(rand_rows.astype(np.int16)).cuda()
        ops.corrupt_replay(ids16, oin.view(B, S, 8), lin.view(B, S, 8), ch, p, torch.from_numpy(dec).cuda(), rr, PAD, MASK)
    torch.cuda.synchronize()
    assert _guards_hold(obuf, n) and _guards_hold(lbuf, n), 'a guard was written'
    assert torch.equal(ids16, before), 'the input ids changed'
    out = oin.view(B, S, 8).cpu().numpy().astype(np.int64)
    lm = lin.view(B, S, 8).cpu().numpy()
    assert (out != I16_SENTINEL).all() and not np.isnan(lm).any(), 'an element was not written'
    assert np.array_equal(lm, np.repeat(lm[:, :, :1], 8, axis=2)), 'the columns of a loss row differ'
    assert np.isin(lm, (0.0, 1.0)).all()
    c = cho.cpu().numpy()
    assert c[0] == -9 and c[-1] == -9 and (want_choice and dec is None or (c == -9).all())
    return out, lm[:, :, 0].astype(np.int64), c[1:B + 1]


class _Refs:
    """apply(decide()) of (seed, sample, choice) over one batch, computed once per choice."""

    def __init__(self, seed, S, p, rows):
        self.seed, self.S, self.p, self.rows, self.memo = seed, S, p, rows, {}

    def get(self, b, choice):
        if not 1 <= choice <= 5:
            choice = R.draw_choice(self.seed, b)
        if (b, choice) not in self.memo:
            out, loss, _, amb = R.reference(self.seed, b, choice, self.S, self.p, self.rows[b], N_TOK, PAD, MASK)
            assert amb == 0
            self.memo[b, choice] = (out, loss, choice)
        return self.memo[b, choice]


def _compare(got, refs, choices):
    out, loss, cho = got
    for b, choice in enumerate(choices):
        want_out, want_loss, want_choice = refs.get(b, choice)
        assert np.array_equal(out[b], want_out), ('rows', b, choice)
        assert np.array_equal(loss[b], want_loss), ('loss mask', b, choice)
        if cho is not None:
            assert cho[b] == want_choice, ('choice_out', b, choice)


@pytest.mark.parametrize('S,p', R.GRID)
def test_philox_path_equals_the_host_restatement(ops, S, p):
    seed, B = R.grid_seed(S, p), R.GRID_B
    rows = R.six_pieces(S, PAD, EOS)
    refs = _Refs(seed, S, p, rows)
    for choice in (1, 2, 3, 4, 5, 0):
        _compare(_launch(ops, rows, p, choice=[choice] * B, seed=seed), refs, [choice] * B)
    _compare(_launch(ops, rows, p, choice=None, seed=seed), refs, [0] * B)                      # choice NULL: drawn in the kernel
    got = _launch(ops, rows, p, choice=[7, -1, 6, 0, 99, -5], seed=seed, want_choice=False)      # out of range: drawn; no choice_out
    _compare((got[0], got[1], None), refs, [0] * B)


def test_philox_path_many_samples_mixed_choices(ops):
    """B = 300 workgroups in one launch: every sample is corrupted under its own index."""
    B, S, p = R.MANY
    seed = R.grid_seed(S, p)
    rng = np.random.default_rng(300)
    rows = np.stack([R.piece(rng, S, int(rng.integers(0, S + 1)), ('walk', 'one', 'every')[b % 3], PAD, EOS) for b in range(B)])
    choices = [b % 7 for b in range(B)]                                                          # 0 and 6 are drawn in the kernel
    refs = _Refs(seed, S, p, rows)
    _compare(_launch(ops, rows, p, choice=choices, seed=seed), refs, choices)
    drawn = {refs.get(b, 0)[2] for b in range(B) if choices[b] in (0, 6)}
    assert drawn == {1, 2, 3, 4, 5}


def test_philox_path_breaks_key_ties_by_index_and_by_bar_value(ops):
    S, B = 2048, 4
    rng = np.random.default_rng(2048)
    rows = rng.integers(0, [256, 128, 129, 256, 128, 32, 254, 49], size=(B, S, 8))
    rows[:, :, 3] = np.arange(S) % 256; rows[:, :, 1] = np.arange(S) // 256                      # no two rows of a sample are equal
    seed, i, j = R.TIE_POS
    for p in (R.tie_percent(), 0.15):
        refs = _Refs(seed, S, p, rows)
        for choice in (1, 2):
            _compare(_launch(ops, rows, p, choice=[choice] * B, seed=seed), refs, [choice] * B)
    seed, i, j = R.TIE_BAR
    rows[:, :, 0] = np.arange(S)                                                                 # every row a bar of its own, 0 .. 2047
    refs = _Refs(seed, S, 0.15, rows)
    got = _launch(ops, rows, 0.15, choice=[3] * B, seed=seed)
    _compare(got, refs, [3] * B)
    place = {int(bar): n for n, bar in enumerate(got[0][R.TIE_BAR_SAMPLE][:, 0])}
    assert place[j] == place[i] + 1


# ---------------------------------------------------------------- replay path, hand-made decisions
def _replay(ops, cases, S, p, with_rand_rows=True):
    B, stride = len(cases), R.replay_stride(S)
    dec = np.zeros((B, stride), dtype=np.int32)
    rr = np.zeros((B, S, 8), dtype=np.int16)
    for b, c in enumerate(cases):
        dec[b, :len(c['dec'])] = c['dec']
        if c.get('rand_rows') is not None:
            rr[b] = c['rand_rows']
    assert with_rand_rows or not any((dec[b, :S] == 2).any() for b, c in enumerate(cases) if c['choice'] == 2)
    ids = np.stack([c['ids'] for c in cases])
    out, loss, _ = _launch(ops, ids, p, choice=[c['choice'] for c in cases], dec=dec, rand_rows=rr if with_rand_rows else None)
    for b, c in enumerate(cases):
        if 'masked' in c:
            want_out, want_loss = c['masked'], c['pos']
        else:
            want_out, want_loss = R.apply(c['ids'], c['choice'], dec[b], rr[b], S, p, PAD, MASK)
        assert np.array_equal(out[b], want_out), ('rows', c.get('name'), c['choice'], b)
        assert np.array_equal(loss[b], want_loss), ('loss mask', c.get('name'), c['choice'], b)
    return out, loss


def _hand_made(S):
    """(cases at p = 0.15, cases at p = 1.5 / S, where deletion takes one position)."""
    rng = np.random.default_rng(S)
    walk = R.piece(rng, S, S, 'walk', PAD, EOS)
    short = R.piece(rng, S, max(2, S // 3), 'walk', PAD, EOS)
    every = R.piece(rng, S, S, 'every', PAD, EOS)
    every[-1, 0] = (S - 1) % 256                                      # the EOS row keeps its place in the cycle of bars
    one = R.piece(rng, S, S, 'one', PAD, EOS)
    one[-1, 0] = 3
    copy = np.full(S, -1, dtype=np.int32)

    def infill(*attempts):
        d = np.zeros(10 * S, dtype=np.int32)                          # an attempt of zeros doubles every row: it overflows
        for att, v in attempts:
            d[att * S:(att + 1) * S] = v
        return d

    def steps(**at):
        v = copy.copy()
        for s, length in at.items():
            v[int(s[1:]) % S] = length
        return v
    k = int(S * 0.15)
    dele0 = np.zeros(S, dtype=np.int32); dele0[0] = 1; dele0[S - (k - 1):] = 1
    dele_mid = np.zeros(S, dtype=np.int32); dele_mid[rng.permutation(S)[:k]] = 1
    only = lambda i: np.eye(1, S, i, dtype=np.int32)[0]
    rand_rows = rng.integers(0, N_TOK, size=(S, 8)).astype(np.int16)
    kinds = rng.integers(0, 4, size=S).astype(np.int32)
    a = [dict(name='infilling overflows ten times', ids=walk, choice=4, dec=infill()),
         dict(name='infilling fits on the last attempt', ids=walk, choice=4, dec=infill((9, steps(s5=3, s10=0, s20=1)))),
         dict(name='infilling overflows by one row, then copies', ids=walk, choice=4, dec=infill((0, steps(**{'s%d' % (S - 1): 0})), (1, copy))),
         dict(name='infilling fits exactly', ids=walk, choice=4, dec=infill((0, steps(s3=2, **{'s%d' % (S - 2): 0})))),
         dict(name='a span past the end', ids=walk, choice=4, dec=infill((0, steps(**{'s%d' % (S - 2): 7})))),
         dict(name='a span at the last step', ids=walk, choice=4, dec=infill((0, steps(**{'s%d' % (S - 1): 2})))),
         dict(name='a span over everything', ids=short, choice=4, dec=infill((3, steps(s0=S + 5)))),
         dict(name='deletion from index 0', ids=walk, choice=1, dec=dele0),
         dict(name='deletion anywhere', ids=short, choice=1, dec=dele_mid),
         dict(name='rotation by 0', ids=walk, choice=5, dec=np.array([0], dtype=np.int32)),
         dict(name='rotation by 1', ids=walk, choice=5, dec=np.array([1], dtype=np.int32)),
         dict(name='rotation by S - 1', ids=short, choice=5, dec=np.array([S - 1], dtype=np.int32)),
         dict(name='one bar', ids=one, choice=3, dec=np.zeros(4, dtype=np.int32)),
         dict(name='256 bars reversed', ids=every, choice=3, dec=(255 - np.arange(256)).astype(np.int32)),
         dict(name='identity order', ids=walk, choice=3, dec=np.arange(300, dtype=np.int32)),
         dict(name='every position a random row', ids=walk, choice=2, dec=np.full(S, 2, dtype=np.int32), rand_rows=rand_rows),
         dict(name='all four kinds', ids=short, choice=2, dec=kinds, rand_rows=rand_rows),
         dict(name='no position selected', ids=walk, choice=2, dec=np.zeros(S, dtype=np.int32))]
    b = [dict(name='deletion of index 0 alone', ids=walk, choice=1, dec=only(0)),
         dict(name='deletion of index S - 1 alone', ids=walk, choice=1, dec=only(S - 1)),
         dict(name='no position selected, no random rows', ids=short, choice=2, dec=np.zeros(S, dtype=np.int32)),
         dict(name='MASK rows only, no random rows', ids=short, choice=2, dec=(kinds % 2).astype(np.int32)),
         dict(name='infilling overflows ten times', ids=short, choice=4, dec=infill())]
    return a, b


@pytest.mark.parametrize('S', [64, 257, 1024, 2048])
def test_replay_path_on_hand_made_decisions(ops, S):
    a, b = _hand_made(S)
    out, loss = _replay(ops, a, S, 0.15)
    by = {c['name']: n for n, c in enumerate(a)}
    walk = a[0]['ids']
    # what the cases are about, stated outright
    n = by['infilling overflows ten times']
    assert np.array_equal(out[n], walk) and not loss[n].any()
    n = by['infilling overflows by one row, then copies']
    assert np.array_equal(out[n], walk) and not loss[n].any()
    n = by['a span at the last step']
    assert np.array_equal(out[n, :-1], walk[:-1]) and np.array_equal(out[n, -1], MASK) and loss[n].tolist() == [0] * (S - 1) + [1]
    n = by['a span past the end']
    assert np.array_equal(out[n, -2], MASK) and np.array_equal(out[n, -1], PAD)
    n = by['a span over everything']
    assert np.array_equal(out[n, 0], MASK) and (out[n, 1:] == PAD).all()
    n = by['identity order']
    assert np.array_equal(out[n], walk) and not loss[n].any()
    n = by['rotation by 0']
    assert np.array_equal(out[n], walk) and not loss[n].any()
    n = by['deletion from index 0']
    assert loss[n].all()
    out, loss = _replay(ops, b, S, 1.5 / S, with_rand_rows=False)
    assert int(S * (1.5 / S)) == 1
    assert loss[0].all() and np.array_equal(out[0, :-1], walk[1:]) and np.array_equal(out[0, -1], PAD)
    assert loss[1].tolist() == [0] * (S - 1) + [1] and np.array_equal(out[1, :-1], walk[:-1]) and np.array_equal(out[1, -1], PAD)


@pytest.mark.parametrize('S', [0, 2049])
def test_lengths_outside_1_to_2048_are_refused(ops, S):
    from pianobart_amd._lib import PBError
    B, n = 2, 2 * S * 8
    ids16 = torch.zeros(B, S, 8, dtype=torch.int16, device='cuda')
    obuf, oin = _guarded(n, torch.int16)
    lbuf, lin = _guarded(n, torch.float32)
    ch = torch.ones(B, dtype=torch.int32, device='cuda')
    dec = torch.zeros(B, R.replay_stride(max(S, 1)), dtype=torch.int32, device='cuda')
    with pytest.raises(PBError):
        ops.corrupt_replay(ids16, oin.view(B, S, 8), lin.view(B, S, 8), ch, 0.15, dec, None, PAD, MASK)
    with pytest.raises(PBError):
        ops.corrupt(ids16, oin.view(B, S, 8), lin.view(B, S, 8), ch, None, 0.15, 1, PAD, MASK, N_TOK)
    torch.cuda.synchronize()
    assert bool((obuf == I16_SENTINEL).all()) and _guards_hold(lbuf, n) and bool(torch.isnan(lin).all())


@pytest.mark.parametrize('S', [257, 1024])
def test_replay_against_the_oracle_at_full_length(ops, S):
    """The oracle differential of test_corrupt_gpu.py beyond one trip of the kernel's loops: a dozen sequences x 5 corruptions, each
    corrupted by the oracle's gen_mask under its own seed, its decisions replayed: rows and loss mask bit for bit."""
    rng = np.random.default_rng(5000 + S)
    seqs = R.piece_set(rng, S, PAD, EOS) + [R.piece(rng, S, int(rng.integers(2, S + 1)), 'walk', PAD, EOS) for _ in range(5)]
    assert len(seqs) == 12
    cases = R.oracle_cases(R.oracle_corruptor(S), seqs, 2000 + S)
    for lo in range(0, len(cases), 30):
        _replay(ops, cases[lo:lo + 30], S, 0.15)
