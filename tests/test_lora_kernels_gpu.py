"""GPU: the four kernels of csrc/pb_lora.hip, each alone, through pianobart_amd.ops, against the float64 / int64 restatements of
tests/lora_ref.py.

Shapes (the smallest at which the indexing can go wrong): M in {1, 63, 64, 65, 257} and on both sides of each kernel's rows per workgroup
(pb_lora_down_rows, pb_lora_up_rows) and of the weight-gradient's rows per slot (pb_lora_wgrad_chunk: a last slot left short, a workgroup
whose other waves have no slot, a chunk above the 64-row floor); r in {4, 8, 16, 64}; K, N, C in {8, 48, 72, 320, 768}; both storage dtypes;
both layouts of the small matrix; alpha 1 and 2/3; the whole matrix (ld = width), the q and the v slice of an (M, 3d) buffer and layer 1's K
slice of an (M, 2 * 2d) buffer. Every (M, r, width) meets every dtype; layout, alpha and slice rotate over the triples so that each value
meets many others.

  exact   integer operands of magnitude <= 8 (M <= 4096: every partial sum is an integer below 2^24), torch.equal to the int64 restatement in
          whatever order the kernel sums; a bf16 read-modify-write is that integer rounded once. For `up` every byte of Y outside the slice
          and behind row M is unchanged; X / Y pads hold NaN, so a read outside the slice poisons a sum.
  real    every element within (n + 2) 2^-24 sum |a_i b_i| of float64, n = the terms of the element's sum (K, r, M; for `up` the prior Y is a
          summand too), plus 2^-8 |result| for the final rounding of a bf16 read-modify-write. The bound follows from f32 accumulation; it
          was not taken from the kernels. alpha is the float32 the entry receives.
"""
import itertools

import pytest
import torch

from tests import lora_ref as R

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
RANKS = (4, 8, 16, 64)
WIDTHS = (8, 48, 72, 320, 768)
ALPHAS = (1.0, float(torch.tensor(2.0 / 3.0, dtype=torch.float32)))


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from pianobart_amd import ops as o
    return o


def _slices(w):
    return [(w, 0), (3 * w, 0), (3 * w, 2 * w), (4 * w, 2 * w)]       # whole | q of (M, 3d) | v of (M, 3d) | layer 1's K of (M, 2 * 2d)


def _ms(ops, kernel):
    q = int(ops.LIB.query('pb_lora_%s_rows' % kernel))
    return sorted({1, 63, 64, 65, 257, q - 1, q, q + 1})


def _cases(ms):
    """(M, r, width, layout flag, alpha, (ld, off)) over every (M, r, width), the rest rotating."""
    out = []
    for i, (M, r, w) in enumerate(itertools.product(ms, RANKS, WIDTHS)):
        out.append((M, r, w, bool((i + i // 2) & 1), ALPHAS[(i // 3) & 1], _slices(w)[(i + i // 5) % 4]))
    return out


def _ints(shape, lim, dtype, gen):
    return torch.randint(-lim, lim + 1, shape, generator=gen).to(dtype).cuda()


def _act(M, ld, off, w, dtype, gen, integer, extra_rows=0):
    """An (M + extra_rows, ld) activation buffer whose (M, w) slice at column `off` holds the operand and everything else NaN."""
    buf = torch.full((M + extra_rows, ld), float('nan'), dtype=dtype, device='cuda')
    val = _ints((M, w), 8, dtype, gen) if integer else torch.randn(M, w, generator=gen).to(dtype).cuda()
    buf[:M, off:off + w] = val
    return buf, val


def _small(shape, gen, integer):
    return _ints(shape, 8, F32, gen) if integer else torch.randn(shape, generator=gen).cuda()


def _check(got, ref, mag, n, integer, bf16=False, what=''):
    got = got.detach().cpu()
    if integer:
        exp = ref.to(torch.float64).to(F32)
        exp = exp.to(BF16) if bf16 else exp
        assert torch.equal(got, exp), what
        return
    err = (got.double() - ref).abs()
    bnd = R.bound(n, mag, ref, bf16)
    assert bool((err <= bnd).all()), (what, float((err / bnd.clamp_min(1e-300)).max()))


@pytest.mark.parametrize('integer', [True, False], ids=['exact', 'real'])
@pytest.mark.parametrize('dtype', [F32, BF16], ids=['f32', 'bf16'])
def test_down(ops, dtype, integer):
    gen = torch.Generator().manual_seed(11)
    for M, r, K, w_kr, alpha, (ld, off) in _cases(_ms(ops, 'down')):
        if integer:
            alpha = 1.0
        X, x = _act(M, ld, off, K, dtype, gen, integer)
        W = _small((K, r) if w_kr else (r, K), gen, integer)
        T = torch.full((M + 2, r), float('nan'), dtype=F32, device='cuda')
        ops.lora_down(X, W, T, M, K, alpha=alpha, x_off=off, w_kr=w_kr)
        ref, mag = R.down(x, W, alpha, w_kr, integer)
        _check(T[:M], ref, mag, K, integer, what=(M, r, K, w_kr, alpha, ld, off))
        assert bool(torch.isnan(T[M:]).all())


@pytest.mark.parametrize('integer', [True, False], ids=['exact', 'real'])
@pytest.mark.parametrize('dtype', [F32, BF16], ids=['f32', 'bf16'])
def test_up(ops, dtype, integer):
    gen = torch.Generator().manual_seed(12)
    for M, r, N, w_nr, alpha, (ld, off) in _cases(_ms(ops, 'up')):
        if integer:
            alpha = 1.0
        # rows behind M and columns outside the slice hold finite sentinels here: every byte of them must survive
        Y = (torch.arange((M + 3) * ld, dtype=F32) % 251 - 125).view(M + 3, ld).to(dtype).cuda()
        y0 = _ints((M, N), 8, dtype, gen) if integer else torch.randn(M, N, generator=gen).to(dtype).cuda()
        Y[:M, off:off + N] = y0
        before = Y.clone()
        T = _small((M, r), gen, integer)
        W = _small((N, r) if w_nr else (r, N), gen, integer)
        ops.lora_up(Y, T, W, M, N, alpha=alpha, y_off=off, w_nr=w_nr)
        term, mag = R.up_term(T, W, alpha, w_nr, integer)
        ref = term + (y0.cpu().to(torch.int64) if integer else y0.cpu().double())
        _check(Y[:M, off:off + N], ref, mag + y0.cpu().double().abs(), r, integer, bf16=dtype == BF16, what=(M, r, N, w_nr, alpha, ld, off))
        keep = torch.ones_like(Y, dtype=torch.bool)
        keep[:M, off:off + N] = False
        bits = torch.int32 if dtype == F32 else torch.int16
        assert torch.equal(Y.view(bits)[keep], before.view(bits)[keep]), ('bytes outside the slice changed', M, r, N, ld, off)


def _wgrad_ms(ops, r):
    c = int(ops.LIB.query('pb_lora_wgrad_chunk', 257, r))
    return sorted({1, 63, 64, 65, 257, c - 1, c, c + 1, 2 * c, 5 * c + 1})      # 257 / 5 c + 1: a short last slot in a workgroup with idle waves


@pytest.mark.parametrize('integer', [True, False], ids=['exact', 'real'])
@pytest.mark.parametrize('dtype', [F32, BF16], ids=['f32', 'bf16'])
def test_wgrad(ops, dtype, integer):
    gen = torch.Generator().manual_seed(13)
    ms = sorted(set(m for r in RANKS for m in _wgrad_ms(ops, r)))
    extra = [(4096, 16, 72), (4096, 64, 48)] if integer else [(8196, 16, 72), (8200, 64, 8)]      # many slots | a chunk above the 64-row floor
    cases = _cases(ms) + [(M, r, C, bool(i), ALPHAS[i], _slices(C)[1 + i]) for i, (M, r, C) in enumerate(extra)]
    for M, r, C, g_cr, alpha, (ld, off) in cases:
        if integer:
            alpha = 1.0
        X, x = _act(M, ld, off, C, dtype, gen, integer)
        T = _small((M, r), gen, integer)
        G = torch.full((C, r) if g_cr else (r, C), float('nan'), dtype=F32, device='cuda')
        ws = torch.full((max(4, int(ops.LIB.query('pb_lora_wgrad_ws_floats', M, r, C))),), float('nan'), dtype=F32, device='cuda')
        ops.lora_wgrad(T, X, G, M, C, alpha=alpha, x_off=off, g_cr=g_cr, ws=ws)
        ref, mag = R.wgrad(T, x, alpha, g_cr, integer)
        _check(G, ref, mag, M, integer, what=(M, r, C, g_cr, alpha, ld, off))
        G2 = torch.zeros_like(G)
        ops.lora_wgrad(T, X, G2, M, C, alpha=alpha, x_off=off, g_cr=g_cr)                # a fresh workspace, the same bytes
        assert torch.equal(G.view(torch.int32), G2.view(torch.int32)), ('two runs differ', M, r, C)


def test_wgrad_slots_follow_the_query(ops):
    """The chunk is at least 64 rows, a multiple of 4, and the workspace is slots x r x C floats."""
    for M, r in ((1, 4), (257, 16), (4096, 16), (8196, 16), (32768, 16), (32768, 64)):
        c = int(ops.LIB.query('pb_lora_wgrad_chunk', M, r))
        assert c >= 64 and c % 4 == 0
        assert int(ops.LIB.query('pb_lora_wgrad_ws_floats', M, r, 72)) == -(-M // c) * r * 72
    assert int(ops.LIB.query('pb_lora_wgrad_ws_floats', 64, 6, 72)) == 0 and int(ops.LIB.query('pb_lora_wgrad_chunk', 0, 8)) == 0


@pytest.mark.parametrize('sign', [1.0, -1.0])
def test_merge(ops, sign):
    """W += alpha B A in place on a row range of a flat buffer: within (r + 2) 2^-24 (|W| + |alpha| sum |B| |A|) of float64; integers exactly;
    the floats around the range untouched."""
    gen = torch.Generator().manual_seed(14)
    for i, (N, r, K) in enumerate(itertools.product((1, 8, 72, 320), RANKS, WIDTHS)):
        integer = bool(i & 1)
        alpha = sign * (1.0 if integer else ALPHAS[(i >> 1) & 1] / r * 16)
        alpha = float(torch.tensor(alpha, dtype=F32))
        flat = torch.full((8 + N * K + 8,), 7.0, dtype=F32, device='cuda')
        W = flat[8:8 + N * K].view(N, K)
        w0 = _small((N, K), gen, integer)
        W.copy_(w0)
        B, A = _small((N, r), gen, integer), _small((r, K), gen, integer)
        ops.lora_merge(W, B, A, alpha)
        term, mag = R.merge_term(B, A, alpha)
        ref = w0.cpu().double() + term
        if integer:
            assert torch.equal(W.cpu(), ref.to(F32)), (N, r, K)
        else:
            err = (W.cpu().double() - ref).abs()
            assert bool((err <= R.bound(r, w0.cpu().double().abs() + mag)).all()), (N, r, K)
        assert bool((flat[:8] == 7.0).all()) and bool((flat[-8:] == 7.0).all())


def test_unaligned_slices_take_the_element_path(ops):
    """A slice that starts off a 16-byte boundary, a leading dimension and a width that are no multiple of the vector: same results, nothing
    outside the slice touched."""
    gen = torch.Generator().manual_seed(15)
    for dtype in (F32, BF16):
        M, r, w, ld, off = 37, 8, 43, 101, 3
        X, x = _act(M, ld, off, w, dtype, gen, True)
        W = _small((r, w), gen, True)
        T = torch.empty(M, r, dtype=F32, device='cuda')
        ops.lora_down(X, W, T, M, w, x_off=off)
        assert torch.equal(T.cpu(), R.down(x, W, 1, False, True)[0].to(F32))
        G = torch.empty(r, w, dtype=F32, device='cuda')
        ops.lora_wgrad(T, X, G, M, w, x_off=off)
        assert torch.equal(G.cpu(), R.wgrad(T, x, 1, False, True)[0].to(F32))
        Y = torch.zeros(M + 1, ld, dtype=dtype, device='cuda')
        t1 = _ints((M, r), 1, F32, gen)
        ops.lora_up(Y, t1, W, M, w, y_off=off)
        exp = torch.zeros(M + 1, ld, dtype=torch.float64)
        exp[:M, off:off + w] = R.up_term(t1, W, 1, False, True)[0].double()
        assert torch.equal(Y.cpu(), exp.to(F32).to(dtype))


def test_zero_rows_is_a_no_op(ops):
    X = torch.randn(4, 24, device='cuda')
    T = torch.full((4, 8), 3.0, device='cuda')
    W = torch.randn(8, 24, device='cuda')
    G = torch.full((8, 24), 5.0, device='cuda')
    Y = X.clone()
    ops.lora_down(X, W, T, 0, 24)
    ops.lora_up(Y, T, W, 0, 24)
    ops.lora_wgrad(T, X, G, 0, 24)
    assert bool((T == 3.0).all()) and bool((G == 5.0).all()) and torch.equal(Y, X)


def test_wrappers_refuse_cpu_tensors_and_bad_ranks(ops):
    from pianobart_amd._lib import PBError
    x, t, w = torch.zeros(4, 8), torch.zeros(4, 4), torch.zeros(4, 8)
    for call in (lambda: ops.lora_down(x, w, t, 4, 8), lambda: ops.lora_up(x, t, w, 4, 8), lambda: ops.lora_wgrad(t, x, w.clone(), 4, 8),
                 lambda: ops.lora_merge(torch.zeros(8, 8), torch.zeros(8, 4), torch.zeros(4, 8), 1.0)):
        with pytest.raises(PBError, match='HIP device tensors'):
            call()
    xc, wc = x.cuda(), torch.zeros(6, 8, device='cuda')
    with pytest.raises(PBError, match=r'pb_lora_down.*r = 6'):
        ops.lora_down(xc, wc, torch.zeros(4, 6, device='cuda'), 4, 8)
    with pytest.raises(PBError, match='lie outside'):
        ops.lora_down(xc, w.cuda(), t.cuda(), 4, 8, x_off=4)
