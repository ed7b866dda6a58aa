"""GPU: the kernels of csrc/pb_embed.hip and pianobart_amd.embedding against the float64 / int64 restatement of tests/embedding_ref.py.

Exact cases (torch.equal): operands are small integers in -8 .. 8, so every f32 sum stays far below 2^24 and every f64 sum, mean, centred value
and product is exact: any correct order gives the same bytes.
  * pb_sqdist: N, M over {1, 2, 63, 64, 65, 127, 128, 129, 257} (both sides of the 64-row tile) and d over {1, 3, 4, 5, 31, 32, 33, 63, 64, 65,
    145, 768, 1030} (both sides of the 4-float load and of the 32-feature slab), dense and as column slices of wider buffers at a 16-byte
    aligned and an odd offset (the wide and the element loads), A and B the same and different buffers, guard bands around D2.
  * pb_knn_radius against numpy.sort with the diagonal removed, blocks with r0 > 0 that end at the last row, a d = 1 lattice where radii tie.
  * pb_ball_counts against the restatement, one-shot and fed in blocks, on lattices where < and <= give different counts.
  * pb_pool_rows: out == float32(float64 sum / count) for bf16 and f32, every S, d and mask shape, guard bands, leading dimensions.
  * pb_embed_moments: mean and C == the restatement for N a power of two; C symmetric bit for bit.
Real-valued cases against float64, bounds from the arithmetic (u32 = 2^-24, u64 = 2^-53):
  * pb_sqdist: x = fl(a - b) carries (1 + u32), x^2 twice that, and d fused additions of non-negative terms at most d u32 more:
    |got - ref| <= (d + 3) 2^-24 ref.
  * pb_pool_rows: a sum of S terms in any order errs by at most (S - 1) u64 sum|h|, the division adds u64 |ref| and the rounding to f32
    2^-24 |ref|; the float64 reference has an error of the first kind itself: |got - ref| <= 2^-24 |ref| + S 2^-52 mean_s|h|.
  * pb_embed_moments: mean within e_c = N 2^-52 mean_n|x_c| for the same reason. C[i][j]: the products of the centred values and their sum
    give (N + 4) 2^-52 sum_n |c_ni c_nj|; the kernel centres with ITS mean, mean + delta, |delta_c| <= e_c, and sum_n (c_ni - delta_i)
    (c_nj - delta_j) - sum_n c_ni c_nj = -delta_j sum_n c_ni - delta_i sum_n c_nj + N delta_i delta_j, by the triangle inequality at most
    e_j sum_n |c_ni| + e_i sum_n |c_nj| + N e_i e_j: the carried term of the tests below.
End to end on a 2 + 2 layer model, d = 64, S = 32: PianoBart.embed against the pooled forward(...).last_hidden_state in all three
precisions, compare_embeddings against the restatement (precision, recall, density, coverage with ==; the Frechet distance within the
rank-deficient bound of tests/test_embedding_cpu.py), and the CLI with --save_embeddings and then --embeddings_*."""
import json

import numpy as np
import pytest
import torch

from tests import embedding_ref as R

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 257)
_CACHE = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ints(shape, seed):
    return np.random.default_rng(seed).integers(-8, 9, size=shape).astype(np.float32)


def _int_sqdist(A, B):
    """Exact squared distances of integer-valued rows in int64, by the expanded form (exact in integers; the kernel never uses it)."""
    a, b = A.astype(np.int64), B.astype(np.int64)
    return ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2 * (a @ b.T)).astype(np.float32)


def _in_wide(a, offset, multiple=4):
    """a (n, d) as the column slice [offset, offset + d) of a wider device buffer whose leading dimension is a multiple of `multiple`."""
    n, d = a.shape
    ld = d + 8 + (-d) % multiple
    wide = torch.full((n, ld), 99.0, dtype=torch.float32, device='cuda')
    view = wide[:, offset:offset + d]
    view.copy_(_dev(a))
    return view


def _guarded(n, m):
    """An (n, m) view inside a buffer of sentinels, one row above and below, 3 columns left and 5 right."""
    buf = torch.full((n + 2, m + 8), -7.0, dtype=torch.float32, device='cuda')
    return buf, buf[1:n + 1, 3:3 + m]


def _band_intact(buf, n, m):
    chk = buf.clone()
    chk[1:n + 1, 3:3 + m] = -7.0
    return bool((chk == -7.0).all())


# ---- pb_sqdist ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', [1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 145, 768, 1030])
def test_sqdist_exact(d):
    from pianobart_amd import ops
    A, B = _ints((257, d), 10 + d), _ints((257, d), 500 + d)
    B[:5] = A[:5]                                                # rows both sets share
    ref_ab, ref_aa = _dev(_int_sqdist(A, B)), _dev(_int_sqdist(A, A))
    forms = {'dense': (_dev(A), _dev(B)), 'aligned': (_in_wide(A, 4), _in_wide(B, 4)), 'odd': (_in_wide(A, 1), _in_wide(B, 3))}
    for name, (a, b) in forms.items():
        for N in SIZES:
            for M in SIZES if name == 'dense' else (1, 64, 65, 257):
                buf, out = _guarded(N, M)
                ops.sqdist(a[:N], b[:M], out)
                assert torch.equal(out, ref_ab[:N, :M]), (name, N, M)
                assert _band_intact(buf, N, M), (name, N, M)
        for N, M in ((65, 65), (257, 129), (2, 257)):            # A and B the same buffer: equal rows give exactly 0
            got = ops.sqdist(a[:N], a[:M])
            assert torch.equal(got, ref_aa[:N, :M]), (name, N, M)
            assert bool((got.diagonal() == 0).all())
    assert bool((ops.sqdist(forms['dense'][0][:5], forms['dense'][1][:5]).diagonal() == 0).all())


@pytest.mark.parametrize('N,M,d', [(65, 129, 33), (129, 65, 768), (257, 64, 1030), (3, 2, 4096)])
def test_sqdist_real(N, M, d):
    from pianobart_amd import ops
    rng = np.random.default_rng(N * 7 + d)
    A, B = rng.standard_normal((N, d)).astype(np.float32), (rng.standard_normal((M, d)) * 1.5 + 0.25).astype(np.float32)
    B[0] = A[0]
    a, b = _dev(A), _dev(B)
    got = ops.sqdist(a, b)
    again = ops.sqdist(a, b)
    assert torch.equal(got, again)                               # two runs, equal bytes
    ref = R.sqdist(A, B)
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
    bound = (d + 3) * 2.0 ** -24 * ref
    print('sqdist real (%d, %d, %d): largest error / bound %.3f' % (N, M, d, float((err / np.maximum(bound, 1e-300)).max())))
    assert (err <= bound).all()
    assert float(got[0, 0]) == 0.0
    same = ops.sqdist(a, a)                                      # a set against itself: a zero diagonal, whatever the values
    assert bool((same.diagonal() == 0).all())


# ---- pb_knn_radius ----------------------------------------------------------------------------------------------------------------------------
def _knn_matrix(kind, N):
    if kind == 'lattice1':
        X = R.lattice(N, 1, 3)
        return R.sqdist(X, X).astype(np.float32)
    rng = np.random.default_rng(N)
    D = (rng.random((N, N)) * 50).astype(np.float32)
    D[rng.random((N, N)) < 0.1] = 7.25                           # ties
    return D


@pytest.mark.parametrize('kind', ['random', 'lattice1'])
@pytest.mark.parametrize('N', [2, 3, 64, 65, 129, 1000])
def test_knn_radius(kind, N):
    from pianobart_amd import ops
    D = _knn_matrix(kind, N)
    dD = _dev(D)
    for k in sorted({k for k in (1, 2, 5, 16, 64, N - 1) if 1 <= k <= min(N - 1, 64)}):
        ref = R.knn_radius(D, k)
        assert torch.equal(ops.knn_radius(dD, k), _dev(ref)), (N, k)
        for r0 in {N // 2, N - 1}:                               # blocks that end at the last row
            assert torch.equal(ops.knn_radius(dD[r0:], k, r0), _dev(ref[r0:])), (N, k, r0)
        if N > 3:                                                # a block in the middle, as a row slice with the matrix' leading dimension
            assert torch.equal(ops.knn_radius(dD[1:3], k, 1), _dev(ref[1:3])), (N, k)
    if kind == 'lattice1' and N == 65:
        rad = R.knn_radius(D, 5)
        assert len(rad) - len(np.unique(rad)) >= 32              # most radii tie


def test_knn_radius_negative_and_special_values():
    """The selection orders the bits as floats are ordered: negative values, zeros of both signs and infinities."""
    from pianobart_amd import ops
    row = np.array([[3.0, -1.5, 0.0, -0.0, np.inf, -np.inf, 2.5, -7.0, 1e-40, 9.0]], dtype=np.float32)
    D = np.repeat(row, 10, axis=0)
    for k in range(1, 10):
        ref = R.knn_radius(D, k)
        assert np.array_equal(ops.knn_radius(_dev(D), k).cpu().numpy(), ref), k


# ---- pb_ball_counts -----------------------------------------------------------------------------------------------------------------------------
def _lattice_case(d, n_gen=63, n_ref=65, k=5):
    key = ('lat', d, n_gen, n_ref)
    if key not in _CACHE:
        G, Rf = R.lattice(n_gen, d, 100 + d), R.lattice(n_ref, d, 200 + d)
        d2 = lambda a, b: R.sqdist(a, b).astype(np.float32)      # integers: exact
        _CACHE[key] = (d2(G, G), d2(Rf, Rf), d2(G, Rf), G, Rf)
    return _CACHE[key]


@pytest.mark.parametrize('d,n_gen,n_ref', [(1, 63, 65), (7, 63, 65), (145, 63, 65), (768, 63, 65), (7, 70, 300)])
def test_ball_counts(d, n_gen, n_ref):
    from pianobart_amd import ops
    k = 5
    gg, rr, gr, _, _ = _lattice_case(d, n_gen, n_ref)
    rad_gen, rad_ref = R.knn_radius(gg, k), R.knn_radius(rr, k)
    ref = R.ball_counts(gr, rad_ref, rad_gen)
    loose = R.ball_counts(gr, rad_ref, rad_gen, strict=False)
    assert any(not np.array_equal(a, b) for a, b in zip(ref, loose))          # the case tells < from <=
    p = R.prdc_from_d2(gg, rr, gr, k)
    assert 0 < p['coverage'] <= 1 and 0 < p['precision'] <= 1
    D, rg, rf = _dev(gr), _dev(rad_gen), _dev(rad_ref)
    zeros = lambda: (torch.zeros(n_gen, dtype=torch.int32, device='cuda'), torch.zeros(n_ref, dtype=torch.int32, device='cuda'),
                     torch.zeros(n_ref, dtype=torch.int32, device='cuda'))
    one = zeros()
    ops.ball_counts(D, rf, rg, *one)
    for got, want in zip(one, ref):
        assert np.array_equal(got.cpu().numpy().astype(np.int64), want)
    for step in (16, 33):                                        # blocked feeding, blocks that do not divide n
        blk = zeros()
        for r0 in range(0, n_gen, step):
            m = min(step, n_gen - r0)
            ops.ball_counts(D[r0:r0 + m], rf, rg[r0:r0 + m], blk[0][r0:r0 + m], blk[1], blk[2])
        assert all(torch.equal(a, b) for a, b in zip(one, blk)), step


@pytest.mark.parametrize('d', [1, 7, 145, 768])
def test_prdc_on_lattices(d):
    """embedding.prdc (the three kernels and the host's ratios, block feeding included) == the restatement."""
    from pianobart_amd import embedding
    gg, rr, gr, G, Rf = _lattice_case(d)
    want = R.prdc_from_d2(gg, rr, gr, 5)
    got = embedding.prdc(_dev(G), _dev(Rf), 5)
    assert dict(got) == want
    assert dict(embedding.prdc(G, Rf, 5, block_bytes=4 * 65 * 7)) == want       # 7 rows to a block


# ---- pb_pool_rows ------------------------------------------------------------------------------------------------------------------------------
def _masks(B, S):
    every_other = np.zeros((B, S), dtype=np.float32)
    every_other[:, ::2] = 1.0
    first, last = np.zeros((B, S), dtype=np.float32), np.zeros((B, S), dtype=np.float32)
    first[:, 0], last[:, -1] = 1.0, 2.5                          # any non-zero value counts
    mixed = np.stack([np.ones(S), every_other[0], np.zeros(S)])[:B].astype(np.float32) if B == 3 else None
    return {'all': np.ones((B, S), dtype=np.float32), 'first': first, 'last': last, 'every_other': every_other,
            'none': np.zeros((B, S), dtype=np.float32), 'None': None, 'mixed': mixed}


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('d', [1, 7, 8, 63, 64, 65, 768])
def test_pool_rows_exact(dtype, d):
    from pianobart_amd import ops
    B = 3
    for S in (1, 2, 63, 64, 65, 257):
        H = _ints((B, S, d), S * 1000 + d)
        forms = {'dense': _dev(H).to(dtype)}
        for name, off in (('aligned', 8), ('odd', 1)):
            v = torch.full((B, S, d + 16), 55.0, dtype=dtype, device='cuda')[:, :, off:off + d]
            v.copy_(_dev(H))
            forms[name] = v
        for mname, mask in _masks(B, S).items():
            want, cnt = R.pool_rows(H, mask)
            for name, h in forms.items():
                buf, out = _guarded(B, d)
                got, count = ops.pool_rows(h, None if mask is None else _dev(mask), out)
                assert got.data_ptr() == out.data_ptr()
                assert torch.equal(out, _dev(want)), (S, mname, name)
                assert np.array_equal(count.cpu().numpy().astype(np.int64), cnt), (S, mname, name)
                assert _band_intact(buf, B, d), (S, mname, name)
            if mname == 'none':
                assert not want.any() and not cnt.any()


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('S,d', [(65, 64), (257, 7), (1024, 768)])
def test_pool_rows_real(dtype, S, d):
    from pianobart_amd import ops
    B = 2
    rng = np.random.default_rng(S + d)
    h = _dev((rng.standard_normal((B, S, d)) * 3 + 0.5).astype(np.float32)).to(dtype)
    mask = (rng.random((B, S)) < 0.7).astype(np.float32)
    mask[:, 0] = 1.0
    got, count = ops.pool_rows(h, _dev(mask))
    again, _ = ops.pool_rows(h, _dev(mask))
    assert torch.equal(got, again)
    ref, mag = R.pool_rows_f64(h.float().cpu().numpy(), mask)
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
    bound = 2.0 ** -24 * np.abs(ref) + S * 2.0 ** -52 * mag
    print('pool real (%d, %d) %s: largest error / bound %.3f' % (S, d, dtype, float((err / np.maximum(bound, 1e-300)).max())))
    assert (err <= bound).all()
    assert np.array_equal(count.cpu().numpy(), (mask != 0).sum(1))


# ---- pb_embed_moments ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', [1, 7, 64, 65, 130, 768])
def test_embed_moments_exact(d):
    from pianobart_amd import ops
    for N in (2, 64, 256, 1024):
        X = _ints((N, d), N + d)
        mean_ref, C_ref = R.moments(X)
        for name, x in (('dense', _dev(X)), ('slice', _in_wide(X, 3))):
            mean, C = ops.embed_moments(x)
            assert torch.equal(mean, _dev(mean_ref)), (N, name)
            assert torch.equal(C, _dev(C_ref)), (N, name)
            assert torch.equal(C, C.t()), (N, name)


@pytest.mark.parametrize('N', [3, 65, 257, 1000])
@pytest.mark.parametrize('d', [7, 130])
def test_embed_moments_real(N, d):
    from pianobart_amd import ops
    rng = np.random.default_rng(N * 3 + d)
    X = (rng.standard_normal((N, d)) * rng.uniform(0.5, 4.0, size=d) + rng.uniform(-20, 20, size=d)).astype(np.float32)
    mean, C = ops.embed_moments(_dev(X))
    mean2, C2 = ops.embed_moments(_dev(X))
    assert torch.equal(mean, mean2) and torch.equal(C, C2) and torch.equal(C, C.t())
    mean_ref, C_ref = R.moments(X)
    x64 = X.astype(np.float64)
    e = N * 2.0 ** -52 * np.abs(x64).mean(0)                     # the mean's bound, per column
    err_m = np.abs(mean.cpu().numpy() - mean_ref)
    assert (err_m <= e).all()
    c = np.abs(x64 - mean_ref)
    own = (N + 4) * 2.0 ** -52 * (c.T @ c)
    s = c.sum(0)
    carried = e[None, :] * s[:, None] + e[:, None] * s[None, :] + N * e[:, None] * e[None, :]
    err_c = np.abs(C.cpu().numpy() - C_ref)
    print('moments real (%d, %d): mean error / bound %.3f, C error / bound %.3f'
          % (N, d, float((err_m / e).max()), float((err_c / (own + carried)).max())))
    assert (err_c <= own + carried).all()


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------------
S_MODEL, D_MODEL = 32, 64
MODEL_KW = dict(max_position_embeddings=S_MODEL, d_model=D_MODEL, encoder_layers=2, decoder_layers=2, encoder_ffn_dim=128, decoder_ffn_dim=128,
                encoder_attention_heads=4, decoder_attention_heads=4, dropout=0.1)


def _model(precision):
    if ('model', precision) not in _CACHE:
        from pianobart_amd.model import BartConfig, PianoBart, PianoBartLM
        from tests.golden_util import load_vocab, randomize_params
        e2w, w2e = load_vocab()
        m = PianoBartLM(PianoBart(BartConfig(**MODEL_KW), e2w, w2e, precision=precision))
        randomize_params(m, 11)
        _CACHE['model', precision] = m.cuda().eval()
    return _CACHE['model', precision]


def _sets():
    """Two sets of 24 and 26 pieces of 32 rows: piece 0 fills the window, piece 1 has no note, another is empty behind row 2."""
    if 'sets' not in _CACHE:
        from tests.metrics_ref import synth_pieces
        from tests.vocab_layout_util import D_DEFAULT
        pad = np.asarray(D_DEFAULT) - 6
        gen, ref = synth_pieces(D_DEFAULT, 24, S_MODEL, seed=5, style=1), synth_pieces(D_DEFAULT, 26, S_MODEL, seed=6)
        for a in (gen, ref):
            a[1, 0], a[1, 1:] = pad + 3, pad
        gen[2, 2], gen[2, 3:] = pad + 3, pad                     # two notes: empty with start = 2
        _CACHE['sets'] = (gen, ref, pad)
    return _CACHE['sets']


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3', 'bf16'])
def test_embed_is_the_pooled_encoder_state(precision):
    m = _model(precision)
    gen, _, pad = _sets()
    ids = torch.from_numpy(gen[[0, 2, 3, 4, 5]]).cuda()
    mask = (ids[:, :, 0] != int(pad[0])).float()
    for msk in (mask, None):
        emb, count = m.embed(ids, msk, return_counts=True)
        assert emb.dtype == torch.float32 and tuple(emb.shape) == (5, D_MODEL) and emb.is_cuda and not emb.requires_grad
        assert torch.equal(m.pianobart.embed(ids, msk), emb)     # both routes, equal bytes
        with torch.no_grad():
            h = m.pianobart(ids, encoder_attention_mask=msk).last_hidden_state
        ref, mag = R.pool_rows_f64(h.float().cpu().numpy(), None if msk is None else msk.cpu().numpy())
        err = np.abs(emb.cpu().numpy().astype(np.float64) - ref)
        assert (err <= 2.0 ** -24 * np.abs(ref) + S_MODEL * 2.0 ** -52 * mag).all(), precision
        assert count.tolist() == ([S_MODEL] * 5 if msk is None else mask.sum(1).int().tolist())
    assert m.training is False


def test_compare_embeddings_against_the_restatement():
    from pianobart_amd import embedding, ops
    m = _model('fp32')
    gen, ref, pad = _sets()
    k, start = 3, 2
    res = embedding.compare_embeddings(m, gen, ref, k=k, start=start, batch_size=7)
    assert list(res) == ['n_gen', 'n_ref', 'empty_gen', 'empty_ref', 'd', 'precision_mode', 'k', 'fmd', 'mean_term', 'trace_term', 'rank_deficient',
                         'precision', 'recall', 'density', 'coverage', 'device_ms']
    assert (res['n_gen'], res['empty_gen'], res['n_ref'], res['empty_ref']) == (22, 2, 25, 1)
    assert (res['d'], res['precision_mode'], res['k'], res['rank_deficient']) == (D_MODEL, 'fp32', k, True)
    assert list(res['device_ms']) == list(embedding.STAGES) + ['total'] and all(v > 0 for v in res['device_ms'].values())
    # the restatement: the rows the encoder sees, then the pipeline on the device's own vectors
    rows, lens, empty = R.arrange(gen, pad, m.pianobart.pad_word_np, start)
    got_rows, got_lens, got_empty = embedding.arrange(gen, m.pianobart.layout, m.pianobart.pad_word_np, start)
    assert np.array_equal(rows, got_rows) and np.array_equal(lens, got_lens) and empty == got_empty == 2
    g, eg = embedding.embed_set(m, gen, start, batch_size=7)    # the batches of the call above: the same bytes
    r, er = embedding.embed_set(m, ref, start, batch_size=7)
    assert (eg, er) == (2, 1) and tuple(g.shape) == (22, D_MODEL) and tuple(r.shape) == (25, D_MODEL)
    G, Rf = g.cpu().numpy(), r.cpu().numpy()
    d2 = {}
    for name, (a, b, A, B) in dict(gg=(g, g, G, G), rr=(r, r, Rf, Rf), gr=(g, r, G, Rf)).items():
        d2[name] = ops.sqdist(a, b).cpu().numpy()                # the device's distances, held to their bound here and exact cases above
        want = R.sqdist(A, B)
        assert (np.abs(d2[name] - want) <= (D_MODEL + 3) * 2.0 ** -24 * want).all()
    want = R.prdc_from_d2(d2['gg'], d2['rr'], d2['gr'], k)
    assert {n: res[n] for n in want} == want
    fmd_ref = R.frechet_svd(G, Rf)
    assert abs(res['fmd'] - fmd_ref) <= R.rank_deficient_bound(G, Rf)
    assert res['fmd'] == res['mean_term'] + res['trace_term']
    again = embedding.compare_embedded(G, Rf, k=k)               # the form without a model, from host arrays
    assert all(again[n] == res[n] for n in ('fmd', 'precision', 'recall', 'density', 'coverage', 'n_gen', 'n_ref', 'd'))


def test_cli_round_trip(tmp_path, capsys):
    from pianobart_amd import eval_embedding
    m = _model('fp32')
    gen, ref, _ = _sets()
    ck, gp, rp = str(tmp_path / 'pre.ckpt'), str(tmp_path / 'g.npy'), str(tmp_path / 'r.npy')
    torch.save({'state_dict': m.state_dict()}, ck)
    np.save(gp, gen.reshape(12, 2, S_MODEL, 8).astype(np.float32))        # what eval_generation --samples 2 writes
    np.save(rp, ref)
    model_flags = ['--ckpt', ck, '--hs', str(D_MODEL), '--layers', '2', '--ffn_dims', '128', '--heads', '4', '--max_seq_len', str(S_MODEL),
                   '--precision', 'fp32']
    out1, out2, prefix = str(tmp_path / 'a.json'), str(tmp_path / 'b.json'), str(tmp_path / 'emb')
    res = eval_embedding.main(['--generated', gp, '--reference', rp, '--k', '3', '--skip', '2', '--batch_size', '6', '--output', out1,
                               '--save_embeddings', prefix] + model_flags)
    assert (res['n_gen'], res['empty_gen'], res['n_ref'], res['empty_ref']) == (22, 2, 25, 1)
    saved = np.load(prefix + '_generated.npy')
    assert saved.shape == (22, D_MODEL) and saved.dtype == np.float32 and np.load(prefix + '_reference.npy').shape == (25, D_MODEL)
    eval_embedding.main(['--embeddings_generated', prefix + '_generated.npy', '--embeddings_reference', prefix + '_reference.npy', '--k', '3',
                         '--output', out2])
    a, b = json.load(open(out1)), json.load(open(out2))
    for n in ('n_gen', 'n_ref', 'd', 'k', 'fmd', 'mean_term', 'trace_term', 'rank_deficient', 'precision', 'recall', 'density', 'coverage'):
        assert a[n] == b[n], n
    assert (a['empty_gen'], b['empty_gen'], a['precision_mode'], b['precision_mode']) == (2, 0, 'fp32', None)
    assert len([l for l in capsys.readouterr().out.splitlines() if l.startswith('   [embedding]')]) == 8
