"""CPU: the host half of pianobart_amd.embedding and eval_embedding, and the argument checks of the K27 entries.

  * frechet_distance at full rank (n >= 4 d) against the nuclear-norm SVD form of tests/embedding_ref.py, which forms no covariance for
    the cross term. Measured here over FULL_RANK, both argument orders and the self distances: the largest relative difference is
    FRECHET_MEASURED = 1.35e-11, the self distance of the 400-row set of (256, 400, d = 64), whose covariance is the worst conditioned
    (a small eigenvalue w of S enters M = S^2 as w^2, known to eps ||M||_2 only: the square root loses eps cond(S)); the same case gives
    2.8e-13 and 4.1e-13 against the SVD form, every other case 1e-16 .. 4.2e-14. "Relative" is to the value for two different sets and to
    |m1 - m2|^2 + tr S1 + tr S2, the terms that cancel, for a set against itself. Held with a margin of 16 for another LAPACK.
  * frechet_distance when a covariance is rank deficient: |difference| <= 2 d sqrt(d 2^-52 ||M||_2), M = S1^1/2 S2 S1^1/2: the recipe takes
    square roots of d eigenvalues that are known to d eps ||M||_2 and may be zero. Measured: 2e-6 .. 1.1e-5 against bounds of 7e-5 .. 6e-4.
  * symmetry and the self distance within the same bounds; every refusal by name; the header's K27 entries in the library, each refusing
    a bad field with -2 before any HIP call."""
import numpy as np
import pytest

from tests import embedding_ref as R

FRECHET_MEASURED = 1.35e-11
FRECHET_TOL = 16 * FRECHET_MEASURED
FULL_RANK = [(300, 280, 64, 1), (256, 400, 64, 2), (64, 100, 16, 3), (40, 36, 8, 4), (1200, 1100, 256, 5), (16, 12, 3, 6)]
DEFICIENT = [(20, 24, 64, 7), (10, 300, 32, 8), (300, 12, 32, 9), (24, 26, 64, 10)]


def _sets(n1, n2, d, seed):
    """Two correlated Gaussian clouds with different means and scales, as float32 values."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n1, d)) @ (np.eye(d) + 0.3 * rng.standard_normal((d, d))) + rng.standard_normal(d)
    B = 1.2 * rng.standard_normal((n2, d)) @ (np.eye(d) + 0.3 * rng.standard_normal((d, d))) + rng.standard_normal(d) * 0.5
    return A.astype(np.float32).astype(np.float64), B.astype(np.float32).astype(np.float64)


def _frechet(A, B):
    from pianobart_amd.embedding import frechet_distance
    (ma, ca), (mb, cb) = R.cov(A), R.cov(B)
    return frechet_distance(ma, ca, mb, cb)


def _scale(A, B):
    (ma, ca), (mb, cb) = R.cov(A), R.cov(B)
    return float(((ma - mb) ** 2).sum() + np.trace(ca) + np.trace(cb))


@pytest.mark.parametrize('n1,n2,d,seed', FULL_RANK)
def test_frechet_full_rank(n1, n2, d, seed):
    A, B = _sets(n1, n2, d, seed)
    assert min(n1, n2) >= 4 * d
    ref = R.frechet_svd(A, B)
    ab, ba = _frechet(A, B), _frechet(B, A)
    rel = [abs(ab - ref) / ref, abs(ba - ref) / ref, abs(ab - ba) / ref, abs(_frechet(A, A)) / _scale(A, A), abs(_frechet(B, B)) / _scale(B, B)]
    print('frechet full rank (%d, %d, %d): value %.6f, relative differences %s' % (n1, n2, d, ref, ' '.join('%.2e' % r for r in rel)))
    assert ref > 0 and max(rel) <= FRECHET_TOL, rel


@pytest.mark.parametrize('n1,n2,d,seed', DEFICIENT)
def test_frechet_rank_deficient(n1, n2, d, seed):
    A, B = _sets(n1, n2, d, seed)
    assert min(n1, n2) - 1 < d
    ref, bound = R.frechet_svd(A, B), R.rank_deficient_bound(A, B)
    ab, ba = _frechet(A, B), _frechet(B, A)
    print('frechet rank deficient (%d, %d, %d): value %.6f, differences %.2e %.2e, bound %.2e' % (n1, n2, d, ref, abs(ab - ref), abs(ba - ref), bound))
    assert abs(ab - ref) <= bound and abs(ba - ref) <= bound and abs(ab - ba) <= 2 * bound
    for X in (A, B):                                             # a set against itself: 0 within its own bound, and not clamped
        assert abs(_frechet(X, X)) <= R.rank_deficient_bound(X, X)


def test_frechet_terms_and_shapes():
    from pianobart_amd._lib import PBError
    from pianobart_amd.embedding import frechet_distance, frechet_terms
    A, B = _sets(64, 100, 16, 3)
    (ma, ca), (mb, cb) = R.cov(A), R.cov(B)
    mean_term, trace_term = frechet_terms(ma, ca, mb, cb)
    assert mean_term == float((ma - mb) @ (ma - mb)) and frechet_distance(ma, ca, mb, cb) == mean_term + trace_term
    assert frechet_terms(ma, ca, ma, cb)[0] == 0.0
    with pytest.raises(PBError, match='expected'):
        frechet_distance(ma, ca, mb[:-1], cb)
    with pytest.raises(PBError, match='expected'):
        frechet_distance(ma, ca[:-1], mb, cb)


def test_arrange_moves_live_rows_to_the_front():
    from pianobart_amd import embedding, ops
    from tests.metrics_ref import synth_pieces
    from tests.vocab_layout_util import D_DEFAULT
    lay = ops.DEFAULT_LAYOUT
    pad = np.asarray(lay.pad8)
    assert list(pad) == [n - 6 for n in D_DEFAULT]
    ids = synth_pieces(D_DEFAULT, 9, 32, seed=4)
    ids[1, 0], ids[1, 1:] = pad + 3, pad                         # no note at all
    ids[2, 3], ids[2, 4:] = pad + 1, pad                         # three notes
    for start in (None, 0, 3, 5):
        rows, lens, empty = embedding.arrange(ids, lay, pad, start)
        want = R.arrange(ids, pad, pad, start or 0)
        assert np.array_equal(rows, want[0]) and np.array_equal(lens, want[1]) and empty == want[2] == (1 if not start else 2)
        assert ((rows[:, :, 0] != pad[0]).sum(1) == lens).all()  # the encoder mask bar != PAD sees exactly the moved rows
    assert embedding.arrange(ids, lay, pad, np.array([0, 0, 3, 0, 0, 0, 0, 0, 0]))[2] == 2          # one start per piece


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def _files(tmp_path, **arrays):
    out = {}
    for name, a in arrays.items():
        out[name] = str(tmp_path / (name + '.npy'))
        np.save(out[name], a)
    return out


TINY = ['--nopretrain', '--hs', '64', '--layers', '1', '--ffn_dims', '64', '--heads', '2', '--max_seq_len', '16']


def test_cli_refusals(tmp_path):
    from pianobart_amd import eval_embedding
    from pianobart_amd._lib import PBError
    from tests.metrics_ref import synth_pieces
    from tests.vocab_layout_util import D_DEFAULT
    pad = np.asarray(D_DEFAULT) - 6
    pieces = synth_pieces(D_DEFAULT, 6, 16, seed=1)
    one = pieces.copy()
    one[1:, 0], one[1:, 1:] = pad + 3, pad                       # one piece with a note
    rng = np.random.default_rng(0)
    f = _files(tmp_path, g=pieces, r=pieces[:5], one=one, seven=np.zeros((4, 16, 7)), e8=rng.standard_normal((8, 12)).astype(np.float32),
               e6=rng.standard_normal((6, 12)).astype(np.float32), e6w=rng.standard_normal((6, 13)).astype(np.float32),
               e1=rng.standard_normal((1, 12)).astype(np.float32), ids=np.zeros((6, 12), dtype=np.int64))
    out = ['--output', str(tmp_path / 'o.json')]
    sets = ['--generated', f['g'], '--reference', f['r']]
    cases = [
        (sets + ['--cpu'], r'--cpu: .*no CPU path'),
        (['--generated', str(tmp_path / 'none.npy'), '--reference', f['r']], r"--generated: no file"),
        (['--generated', f['g'], '--reference', str(tmp_path / 'none.npy')], r"--reference: no file"),
        (['--generated', f['seven'], '--reference', f['r']], r'rows of 8 ids'),
        (sets + ['--ckpt', str(tmp_path / 'none.ckpt')], r'--ckpt: no file'),
        (['--generated', f['one'], '--reference', f['r']] + TINY, r'generated set holds 1 non-empty pieces'),
        (['--generated', f['g'], '--reference', f['one']] + TINY, r'reference set holds 1 non-empty pieces'),
        (sets + TINY + ['--k', '5'], r'k = 5.*k < min\(n_gen, n_ref\) = 5'),
        (sets + TINY + ['--k', '0'], r'--k takes'),
        (sets + TINY + ['--skip', '-1'], r'--skip takes'),
        (['--generated', f['g']], r'give --generated and --reference'),
        (['--embeddings_generated', f['e8']], r'come together'),
        (['--embeddings_generated', f['e8'], '--embeddings_reference', f['e6']] + sets, r'not with --generated'),
        (['--embeddings_generated', f['e8'], '--embeddings_reference', str(tmp_path / 'none.npy')], r'--embeddings_reference: no file'),
        (['--embeddings_generated', f['e8'], '--embeddings_reference', f['e6w']], r'embedding widths differ: generated d = 12, reference d = 13'),
        (['--embeddings_generated', f['e8'], '--embeddings_reference', f['e6'], '--k', '6'], r'k = 6.*= 6'),
        (['--embeddings_generated', f['e8'], '--embeddings_reference', f['e6'], '--k', '65'], r'k = 65'),
        (['--embeddings_generated', f['e8'], '--embeddings_reference', f['e1']], r'reference set holds 1 non-empty pieces'),
        (['--embeddings_generated', f['ids'], '--embeddings_reference', f['e6']], r'embeddings are \(n, d\) floats'),
    ]
    for argv, pattern in cases:
        with pytest.raises(PBError, match=pattern):
            eval_embedding.main(argv + out)


def test_module_refusals():
    import torch
    from pianobart_amd import embedding, ops
    from pianobart_amd._lib import PBError
    from pianobart_amd.model import BartConfig, PianoBart, PianoBartLM
    from tests.golden_util import load_vocab
    from tests.metrics_ref import synth_pieces
    from tests.vocab_layout_util import D_DEFAULT
    rng = np.random.default_rng(0)
    a, b = rng.standard_normal((8, 12)).astype(np.float32), rng.standard_normal((6, 12)).astype(np.float32)
    for fn in (embedding.prdc, embedding.compare_embedded):
        with pytest.raises(PBError, match='widths differ'):
            fn(a, b[:, :5], 3)
        with pytest.raises(PBError, match='k = 6'):
            fn(a, b, 6)
        with pytest.raises(PBError, match='k = True'):
            fn(a, b, True)
        with pytest.raises(PBError, match='holds 1 non-empty'):
            fn(a[:1], b, 1)
        with pytest.raises(PBError, match=r'expected \(n, d\)'):
            fn(a[0], b, 1)
        with pytest.raises(PBError, match='HIP device tensors'):
            fn(torch.from_numpy(a), torch.from_numpy(b), 3)
    e2w, w2e = load_vocab()
    m = PianoBartLM(PianoBart(BartConfig(max_position_embeddings=16, d_model=64, encoder_layers=1, decoder_layers=1, encoder_ffn_dim=64,
                                         decoder_ffn_dim=64, encoder_attention_heads=2, decoder_attention_heads=2), e2w, w2e, precision='fp32'))
    ids = synth_pieces(D_DEFAULT, 6, 16, seed=1)
    with pytest.raises(PBError, match='no CPU path'):
        embedding.embed_set(m, ids)
    with pytest.raises(PBError, match='no CPU path'):
        m.embed(torch.from_numpy(ids))
    with pytest.raises(PBError, match=r'\(B, S, 8\) integers'):
        m.pianobart.embed(torch.zeros(2, 16, 8))
    with pytest.raises(PBError, match='exceed max_position_embeddings 16'):
        embedding.embed_set(m, synth_pieces(D_DEFAULT, 3, 24, seed=1))
    with pytest.raises(PBError, match='batch_size'):
        embedding.embed_set(m, ids, batch_size=0)
    with pytest.raises(PBError, match='k = 6'):
        embedding.compare_embeddings(m, ids, ids, k=6)
    with pytest.raises(PBError, match='must be a PianoBart'):
        embedding.embed_set(torch.nn.Linear(2, 2), ids)
    with pytest.raises(PBError, match='head 0'):
        embedding.embed_set(m, np.full((2, 16, 8), 5000))
    x = torch.zeros(4, 4)
    for call in (lambda: ops.sqdist(x, x), lambda: ops.knn_radius(x, 1), lambda: ops.embed_moments(x),
                 lambda: ops.pool_rows(torch.zeros(2, 3, 4)), lambda: ops.ball_counts(x, x[0], x[0], x[0].int(), x[0].int(), x[0].int())):
        with pytest.raises(PBError, match='HIP device tensors'):
            call()
    for call, pattern in ((lambda: ops.sqdist(x, torch.zeros(4, 5)), 'same width'), (lambda: ops.sqdist(torch.zeros(2, 5000), torch.zeros(2, 5000)), 'd = 5000'),
                          (lambda: ops.knn_radius(x, 4), 'k = 4'), (lambda: ops.knn_radius(x[:2], 1, 3), 'rows r0 = 3'),
                          (lambda: ops.embed_moments(x[:1]), 'at least 2 rows'), (lambda: ops.sqdist(x.double(), x.double()), '2-D f32'),
                          (lambda: ops.pool_rows(x), r'\(B, S, d\)'), (lambda: ops.sqdist(x.t(), x), 'contiguous rows')):
        with pytest.raises(PBError, match=pattern):
            call()


# ---- ABI -----------------------------------------------------------------------------------------------------------------------------------------
K27 = ('pb_embed_ws_bytes', 'pb_pool_rows', 'pb_embed_moments', 'pb_sqdist', 'pb_knn_radius', 'pb_ball_counts')


def test_k27_entries_are_exported_and_abi_stays_10():
    import ctypes
    from pianobart_amd import _lib
    decls = _lib.parse_header()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in K27:
        assert name in decls and hasattr(dll, name), name
    assert _lib.LIB.query('pb_abi_version') == 10
    q = lambda N, d: _lib.LIB.query('pb_embed_ws_bytes', N, d)
    assert q(1, 64) == 0 and q(2, 0) == 0 and q(2, 4097) == 0 and q(2, 64) == (64 + 4096) * 8
    assert q(2048, 768) == 8 * (768 + 78 * 4096) * 8 and q(256, 65) == q(2, 65) == (65 + 3 * 4096) * 8 and q(257, 65) == 2 * q(256, 65)


P = 0x10000          # a dummy, 16-byte aligned address: only good for calls that are refused before any HIP call
_BAD = [
    ('pb_pool_rows', (P, 64, 7, None, P, 64, P, 2, 8, 64), 'dtype = 7'),
    ('pb_pool_rows', (None, 64, 0, None, P, 64, P, 2, 8, 64), 'H must be'),
    ('pb_pool_rows', (P, 64, 0, None, P, 64, P, 0, 8, 64), 'B = 0'),
    ('pb_pool_rows', (P, 64, 0, None, P, 64, P, 2, 0, 64), 'S = 0'),
    ('pb_pool_rows', (P, 64, 0, None, P, 64, P, 2, 8, 0), 'd = 0'),
    ('pb_pool_rows', (P, 63, 0, None, P, 64, P, 2, 8, 64), 'ldh = 63'),
    ('pb_pool_rows', (P, 64, 0, None, P, 63, P, 2, 8, 64), 'ldo = 63'),
    ('pb_pool_rows', (P, 64, 0, P + 2, P, 64, P, 2, 8, 64), 'mask must be'),
    ('pb_pool_rows', (P, 64, 0, None, None, 64, P, 2, 8, 64), 'out must be'),
    ('pb_pool_rows', (P, 64, 0, None, P, 64, None, 2, 8, 64), 'count must be'),
    ('pb_embed_moments', (None, 64, 8, 64, P, P, 64, P), 'X must be'),
    ('pb_embed_moments', (P, 64, 1, 64, P, P, 64, P), 'N = 1'),
    ('pb_embed_moments', (P, 64, 8, 4097, P, P, 4097, P), 'd = 4097'),
    ('pb_embed_moments', (P, 63, 8, 64, P, P, 64, P), 'ldx = 63'),
    ('pb_embed_moments', (P, 64, 8, 64, P, P, 63, P), 'ldc = 63'),
    ('pb_embed_moments', (P, 64, 8, 64, P + 4, P, 64, P), 'mean must be'),
    ('pb_embed_moments', (P, 64, 8, 64, P, None, 64, P), 'C must be'),
    ('pb_embed_moments', (P, 64, 8, 64, P, P, 64, None), 'ws must be'),
    ('pb_sqdist', (P, 8, P, 8, None, 4, 4, 4, 8), 'A, B and D2'),
    ('pb_sqdist', (P, 8, P, 8, P + 64, 4, 0, 4, 8), 'N = 0'),
    ('pb_sqdist', (P, 8, P, 8, P + 64, 4, 4, 4, 4097), 'd = 4097'),
    ('pb_sqdist', (P, 7, P, 8, P + 64, 4, 4, 4, 8), 'lda = 7'),
    ('pb_sqdist', (P, 8, P, 8, P + 64, 3, 4, 4, 8), 'ldd = 3'),
    ('pb_sqdist', (P, 8, P, 8, P, 4, 4, 4, 8), 'aliases'),
    ('pb_knn_radius', (None, 8, 8, 8, 0, 1, P), 'D2 and rad'),
    ('pb_knn_radius', (P, 8, 8, 1, 0, 1, P), 'N = 1'),
    ('pb_knn_radius', (P, 8, 4, 8, 5, 1, P), 'r0 = 5'),
    ('pb_knn_radius', (P, 8, 8, 8, 0, 8, P), 'k = 8'),
    ('pb_knn_radius', (P, 100, 8, 100, 0, 65, P), 'k = 65'),
    ('pb_knn_radius', (P, 7, 8, 8, 0, 1, P), 'ldd = 7'),
    ('pb_ball_counts', (P, 8, 4, 8, None, P, P, P, P), 'rad_ref'),
    ('pb_ball_counts', (P, 8, 0, 8, P, P, P, P, P), 'n = 0'),
    ('pb_ball_counts', (P, 8, 4, 0, P, P, P, P, P), 'M = 0'),
    ('pb_ball_counts', (P, 7, 4, 8, P, P, P, P, P), 'ldd = 7'),
    ('pb_ball_counts', (P, 8, 4, 8, P, P, P, None, P), 'col_hits'),
]


@pytest.mark.parametrize('entry,args,names', _BAD, ids=['%s-%s' % (e, n.replace(' ', '_')) for e, _, n in _BAD])
def test_k27_entries_refuse_without_a_gpu(entry, args, names):
    """Every entry checks its arguments before the first HIP call: a bad value planted in one field comes back by name."""
    from pianobart_amd import _lib
    with pytest.raises(_lib.PBError) as e:
        _lib.LIB.call(entry, *args, None)
    assert entry in str(e.value) and '(-2)' in str(e.value) and names in str(e.value), str(e.value)
