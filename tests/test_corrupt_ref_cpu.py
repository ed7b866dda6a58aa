"""CPU: tests/corrupt_ref.py, the host restatement of the corruption kernel that tests/test_corrupt_kernels_gpu.py compares it with.

apply() is held to the oracle's gen_mask (which tests/golden/g6_gen_mask.npz ties to the reference) on the oracle's own traced
decisions; decide() to the structure its contract states, to the Poisson(3) mean, and to the condition that no configuration the GPU
test names has an ambiguous Poisson draw (the float32 cdf of the kernel and the float64 one then agree on every draw, whatever the
compiler fuses). The searches for a (seed, sample) whose keys hold a tie (about 5e-4 per try at 2048 keys) are repeated here: the GPU test takes their results as
constants. A tie between two bar keys turned up within the budget as well (TIE_BAR), so the GPU test has that case too.
"""
import numpy as np
import pytest

from tests import corrupt_ref as R
from tests.golden_util import N_TOK, PAD

MASK, EOS = PAD + 1, PAD + 3
LENGTHS = [1, 2, 3, 10, 30, 50, 64, 255, 256, 257, 1024]


@pytest.mark.parametrize('S', LENGTHS)
def test_apply_on_the_oracles_decisions_is_the_oracles_gen_mask(S):
    """All five corruptions on the piece shapes of test_corrupt_gpu.py (walk, one bar, every row a new bar, all PAD) at every length."""
    rng = np.random.default_rng(100 + S)
    corr = R.oracle_corruptor(S)
    seqs = [R.piece(rng, S, L, b, PAD, EOS) for L, b in ((S, 'walk'), (max(1, S // 2), 'walk'), (S, 'one'), (S, 'every'), (0, 'walk'))]
    cases = R.oracle_cases(corr, seqs, 3000 + S)
    assert len(cases) == 25
    for n, c in enumerate(cases):
        out, loss = R.apply(c['ids'], c['choice'], c['dec'], c['rand_rows'], S, 0.15, PAD, MASK)
        assert np.array_equal(out, c['masked']), ('rows', c['choice'], n)
        assert np.array_equal(loss, c['pos']), ('loss mask', c['choice'], n)


def test_apply_on_the_golden_decisions_is_the_reference():
    from tests.golden_util import g6_replay_cases
    single, batch = g6_replay_cases()
    assert len(single) == 25
    for c in single + batch:
        out, loss = R.apply(c['ids'], c['choice'], c['dec'], c['rand_rows'], 64, 0.15, PAD, MASK)
        assert np.array_equal(out, c['masked']) and np.array_equal(loss, c['pos']), c['choice']


@pytest.mark.parametrize('S,p', R.GRID + [R.MANY[1:]])
def test_decide_has_the_stated_structure(S, p):
    seed = R.grid_seed(S, p)
    rows = R.six_pieces(S, PAD, EOS)
    for b in range(R.GRID_B):
        dec, _, _ = R.decide(seed, b, 1, S, p, rows[b], N_TOK)
        assert dec.shape == (R.replay_stride(S),) and dec.dtype == np.int32
        assert int((dec[:S] != 0).sum()) == int(S * p) and not dec[S:].any()
        dec, rr, _ = R.decide(seed, b, 2, S, p, rows[b], N_TOK)
        k = round(S * p); k80 = round(0.8 * k); k10 = round(0.1 * k)
        assert int((dec[:S] != 0).sum()) == k and int((dec[:S] == 1).sum()) == k80 and int((dec[:S] == 2).sum()) == min(k10, k - k80)
        assert set(dec[:S].tolist()) <= {0, 1, 2, 3} and not dec[S:].any()
        assert rr.shape == (S, 8) and rr.dtype == np.int16 and (rr >= 0).all() and (rr < np.array(N_TOK)).all()
        dec, _, _ = R.decide(seed, b, 3, S, p, rows[b], N_TOK)
        bars = np.unique(rows[b][:, 0])
        assert sorted(dec[bars].tolist()) == list(range(len(bars)))                  # a bijection of the bars onto their places
        dec, _, _ = R.decide(seed, b, 4, S, p, rows[b], N_TOK)
        assert dec[:10 * S].min() >= -1 and dec[:10 * S].max() <= 64 and not dec[10 * S:].any()
        dec, _, _ = R.decide(seed, b, 5, S, p, rows[b], N_TOK)
        assert 0 <= dec[0] < S and not dec[1:].any()
        assert 1 <= R.draw_choice(seed, b) <= 5


def test_python_rounds_halves_to_even_where_the_grid_puts_them():
    """S * 0.15 = 1.5, 4.5, 7.5 at S = 10, 30, 50: k = 2, 4, 8; and k * 0.1 = 0.5 at k = 5 gives no random row."""
    assert [R.mask_counts(S, 0.15)[0] for S in (10, 30, 50)] == [2, 4, 8]
    assert R.mask_counts(10, 0.5) == (5, 4, 0) and R.mask_counts(3, 0.9) == (3, 2, 0) and R.mask_counts(1024, 0.15) == (154, 123, 15)


def test_choice_draws_cover_all_five_evenly():
    n = 5000
    cnt = np.bincount([R.draw_choice(77, b) for b in range(n)], minlength=6)
    assert cnt[0] == 0 and (np.abs(cnt[1:] - n / 5) < 5 * (n * 0.2 * 0.8) ** 0.5).all()


def test_poisson_inversion_has_mean_3():
    x, y, _, _ = R.words(12345, 3, 4, np.arange(100000))
    z, amb = R.poisson3(R._u01(y))
    assert abs(z.mean() - 3.0) < 3 * (3.0 / len(z)) ** 0.5                            # three standard errors of a Poisson(3) mean
    assert abs(z.var() - 3.0) < 0.1 and z.max() < 20 and amb.sum() < 20               # the band holds about 6 * 2^-18 of the draws
    assert np.array_equal(R.CDF32[:20], R.CDF64[:20].astype(np.float32)) or np.abs(R.CDF32 - R.CDF64).max() < 2.0 ** -20
    start = R._u01(x) < np.float32(0.15 / 3)
    assert abs(start.mean() - 0.05) < 5 * (0.05 * 0.95 / len(x)) ** 0.5


def test_no_gpu_configuration_has_an_ambiguous_poisson_draw():
    """Every sample is counted as if it drew infilling: the launches with in-kernel choices are covered whatever they draw."""
    for S, p in R.GRID:
        rows = R.six_pieces(S, PAD, EOS)
        assert sum(R.decide(R.grid_seed(S, p), b, 4, S, p, rows[b], N_TOK)[2] for b in range(R.GRID_B)) == 0, (S, p)
    B, S, p = R.MANY
    rows = np.zeros((S, 8), dtype=np.int64)
    assert sum(R.decide(R.grid_seed(S, p), b, 4, S, p, rows, N_TOK)[2] for b in range(B)) == 0


def test_infilling_retries_where_the_grid_says_it_does():
    """At S = 3 some sample of the grid fails its first attempt (the seeds were chosen for it); at p = 0.9 spans run past the end."""
    retried = past_end = 0
    for S, p in [(3, 0.5), (3, 0.9), (64, 0.9), (257, 0.9), (257, 0.5)]:
        for b in range(R.GRID_B):
            dec, _, _ = R.decide(R.grid_seed(S, p), b, 4, S, p, np.zeros((S, 8), dtype=np.int64), N_TOK)
            retried += R.walk_spans(dec[:S], S) is None
            for att in range(10):
                i = s = 0
                while i < S:
                    i += max(1, int(dec[att * S + s])); s += 1
                past_end += i > S
    assert retried >= 2 and past_end > 0


def test_tie_searches_find_the_exported_seeds():
    assert R.search_tie(R.TIE_SEED0, R.TIE_POS_SAMPLE, 1) == R.TIE_POS
    assert R.search_tie(R.TIE_SEED0, R.TIE_BAR_SAMPLE, 3) == R.TIE_BAR
    seed, i, j = R.TIE_POS
    key = R.words(seed, R.TIE_POS_SAMPLE, 1, np.arange(2048))[0]
    assert key[i] == key[j] and i < j
    p = R.tie_percent()
    for choice in (1, 2):                                                             # the tie decides: i is taken, j is not
        dec, _, _ = R.decide(seed, R.TIE_POS_SAMPLE, choice, 2048, p, None, N_TOK)
        assert dec[i] != 0 and dec[j] == 0
    seed, i, j = R.TIE_BAR
    rows = np.zeros((2048, 8), dtype=np.int64); rows[:, 0] = np.arange(2048)
    dec, _, _ = R.decide(seed, R.TIE_BAR_SAMPLE, 3, 2048, 0.15, rows, N_TOK)
    assert dec[j] == dec[i] + 1                                                       # equal keys: the lower bar value goes first
