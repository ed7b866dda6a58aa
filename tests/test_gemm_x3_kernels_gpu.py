"""GPU: pb_gemm with dtype PB_F32X3 (csrc/pb_gemm_x3.hip) at every pad, layout and plane edge, against the float64 model of
tests/gemm_x3_ref.py (checked without a GPU in tests/test_gemm_x3_ref_cpu.py). Everything goes through pianobart_amd.ops.gemm
(pb_split_bf16 through ops.split_bf16).

Three kinds of assertion, as in tests/test_gemm_kernels_gpu.py:
  1. exact (the bulk). Operands x = p + q 2^-11 whose planes are hi = p, lo = q, so every term of a_hi b_hi + a_hi b_lo + a_lo b_hi is a
     multiple of 2^-11 and float32 accumulation is exact in any order (gemm_x3_ref: the caps are asserted in every case). torch.equal on C,
     on colsum_out and on the sum of the split-K slabs. The dropped lo lo term is a multiple of 2^-22: a kernel that added it, lost a lo
     contribution, exchanged the roles of the planes, dropped a pad row or read a stale pad changes the result.
  2. guards. C, aux_out, colsum_out and the slabs are views inside larger allocations (gemm_ref.Guarded): sentinels in front, behind and
     in the pad columns of ldc / ldaux, the interior NaN going in. The operands sit in NaN: pad columns of lda / ldb / ldaux, in front,
     behind, between batches. test_workspace_pads_are_rewritten_after_a_poisoned_call fills the per-stream workspace with inf / NaN first:
     a pad element of A3 / B3 the split did not rewrite meets a zero of the other operand and reaches C as NaN.
  3. float64 with a per-element bound for randn operands and the GELU pair: |got - model| <= k 2^-24 S, S = |alpha| sum_k (|a_hi b_hi| +
     |a_hi b_lo| + |a_lo b_hi|) + |bias| (+ 1 for gelu'), k = 4 x the same figure of a plain float32 torch evaluation of the model
     (gemm_x3_ref.float32_evaluation), computed here. The post pass uses gelu_f / gelu_grad_f (erff), as the generic f32 kernel does:
     no allowance for the function, as on that row of the GEMM suite. How far the model is from the true product is a statement about
     the arithmetic and is asserted on the CPU (3.008 2^-16 sum |a b|).

Branches (the id of a case starts with the forms its two splits take and the product kernel, computed by the mirrors of gemm_x3_ref):
  kcV / kcS  split_kc_kernel<ROLE, VEC>: a K-contiguous operand of NT. VEC needs the base on 16 bytes, ld % 4 == 0, batch strides % 4 == 0;
             the chunk with c + 8 > K and every chunk of the scalar form go element by element. rcV / rcS: split_rc_kernel, both operands of
             TN, rows [K, Kp) and columns [rows, Rp) zero. tr: split_tr_kernel<0> (A of TT) / <1> (B of NN), 64 x 64 tiles through LDS.
  tile128    the default: pb_gemm_x3 sets PB_GEMM_TILE128 below 128 tiles of 256 x 256 (one unsplit batch). pingpong: from 128 tiles
             (8192 x 1024), or PB_GEMM_TILE256 with split-K or batches. generic: pb_gemm2_try declines N % 8, M % 8 under TN, C off 16
             bytes, ldc % 4 (and PB_GEMM_FORCE_V1).
  split-K    over the 3 Kp / 64 K tiles: cuts inside a segment, on the segment boundaries, empty slabs. Bias, batches, ldc != N are refused.
  postV / postS   x3_post_kernel (GELU pair, multiply by aux_in), vector and scalar form.

Measured on an MI355X, worst kernel / float32-torch ratio over the cases of a product kernel (in brackets the largest kernel figure, in
units of 2^-24 S); the bound is 4:
  real operands, 264 x 264 (268) x 100   tile128 NT / NN 1.87 (3.72), ping-pong TN in two batches 1.87 (3.68), generic 1.56 (3.28)
  split-K 3 slabs, 264 x 264 x 448       tile128 TN and ping-pong NT: 1.25 (1.37), the same bits
  GELU pair                              C 2.17 (3.88), gelu' 2.44 (1.40); the same figures from the vector and the scalar post pass
Every exact case holds bit for bit; nothing skips. The file takes about 5 s.
"""
import pytest
import torch

from tests import gemm_ref as G
from tests import gemm_x3_ref as X

pytestmark = pytest.mark.gpu

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
NAN, INF = float('nan'), float('inf')
WORST = {}


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from pianobart_amd import ops as o
    return o


# ---------------------------------------------------------------- helpers
_AB = {}


def _inputs(case):
    """make_inputs on the device; the operand pair of the last (shape, seed) is kept: the epilogues of one shape share it."""
    key = (case.M, case.N, case.K, case.nbatch, case.seed, case.exact)
    if key not in _AB:
        _AB.clear()
        _AB[key] = tuple(t.cuda() for t in X.make_ab(case))
    x = X.make_inputs(case, ab=_AB[key])
    return {k: (None if v is None else v.cuda()) for k, v in x.items()}


def _nan_wrapped(t, pad=64):
    buf = torch.full((t.numel() + 2 * pad,), NAN, dtype=F32, device='cuda')
    buf[pad:pad + t.numel()] = t.reshape(-1).to(F32)
    return buf[pad:pad + t.numel()]


def _run(ops, case, x, expect_error=None, **override):
    """One ops.gemm call of the case in PB_F32X3 with every output guarded -> dict of gemm_ref.Guarded. The guards are checked here."""
    M, N, K, nb = case.M, case.N, case.K, case.nbatch
    A, lda, sa = X.place_batches(x['A'].to(F32), case.a_kc, case.lda_pad, case.a_off, case.a_spad)
    B, ldb, sb = X.place_batches(x['B'].to(F32), case.b_kc, case.ldb_pad, case.b_off, case.b_spad)
    assert (sa, sb) == (X.batch_stride(case, 'a'), X.batch_stride(case, 'b'))
    assert A.data_ptr() % 16 == 0 and B.data_ptr() % 16 == 0                    # the mirrors of vec_ok count from an aligned base
    ldc = N + case.ldc_pad
    o = dict(C=G.Guarded(nb * M, N, F32, 'cuda', ld=ldc, shift=case.c_off, init=(x['c0'].reshape(nb * M, N) if case.acc else None)))
    kw = dict(M=M, N=N, K=K, dtype=ops.PB_F32X3, a_kc=case.a_kc, b_kc=case.b_kc, lda=lda, ldb=ldb, ldc=ldc, alpha=case.alpha,
              accum=case.acc, c_f32=True, a_off=case.a_off, b_off=case.b_off, c_off=o['C'].start, nb1=case.nb1, nb2=case.nb2)
    if nb > 1:
        kw.update(sA=(case.nb2 * sa, sa), sB=(case.nb2 * sb, sb), sC=(case.nb2 * M * ldc, M * ldc))
    if case.bias:
        kw['bias'] = _nan_wrapped(x['bias'])
    if case.mul:
        aux, ldaux, _ = G.place(x['aux'][None].to(F32), True, case.ldaux_pad, 64 + case.aux_off, F32)
        kw.update(gelu_grad_aux_in=aux[64 + case.aux_off:], ldaux=ldaux)
    if case.gelu:
        o['aux_out'] = G.Guarded(M, N, F32, 'cuda', ld=N + case.ldaux_pad, shift=case.aux_off)
        kw.update(gelu_aux_out=o['aux_out'].view, ldaux=N + case.ldaux_pad)
    if case.colsum:
        o['colsum'] = G.Guarded(1, N, F32, 'cuda', pad=8, init=torch.full((1, N), G.CS_PRIOR))
        ws = torch.full((int(ops.LIB.query('pb_gemm_colsum_ws_floats', M, N)),), NAN, device='cuda')
        kw.update(colsum_out=o['colsum'].view, colsum_ws=ws)
    if case.splitk > 1:
        o['slabs'] = G.Guarded(1, case.splitk * M * N, F32, 'cuda', pad=4096, guard=NAN)
        kw.update(splitk=case.splitk, slabs=o['slabs'].view)
    kw.update(case.flags)
    kw.update(override)
    if expect_error is not None:
        with pytest.raises(expect_error):
            ops.gemm(A, B, o['C'].buf, **kw)
    else:
        ops.gemm(A, B, o['C'].buf, **kw)
    torch.cuda.synchronize()
    for name, g in o.items():
        g.assert_guards('%s: %s' % (case.id, name))
    return o


def _c(case, o):
    return o['C'].view.reshape(case.nbatch, case.M, case.N)


def _check_exact(case, x, o, what=''):
    ref = X.reference(case, x)
    stored = G.store(ref['C'], F32)
    X.assert_caps(case, stored)
    tag = case.id + what
    G.assert_equal(_c(case, o), stored, tag + ': C')
    if case.colsum:
        G.assert_equal(o['colsum'].view[0], G.colsum_reference(case, stored), tag + ': colsum_out')
    if case.splitk > 1 and case.kernel != 'generic':
        slabs = o['slabs'].view.view(case.splitk, case.M, case.N)
        assert bool(torch.isfinite(slabs).all()), tag + ': a slab element was not written'
        G.assert_equal(slabs.double().sum(0), case.alpha * ref['acc'][0], tag + ': sum of the slabs')


def _bound(what, family, kernel, f32):
    ratio = kernel / f32 if f32 > 0 else (0.0 if kernel == 0 else float('inf'))
    print('RATIO %-84s kernel %10.4g   float32 torch %10.4g   ratio %6.3f' % (what, kernel, f32, ratio))
    w = WORST.setdefault(family, [0.0, 0.0])
    w[0], w[1] = max(w[0], ratio), max(w[1], kernel)
    assert kernel <= G.MARGIN * f32, '%s: kernel %.4g > %g x float32 torch %.4g' % (what, kernel, G.MARGIN, f32)


def _check_kind3(case, x, o):
    xc = {k: (None if v is None else v.cpu()) for k, v in x.items()}          # model and yardstick both on the CPU
    refc = X.reference(case, xc)
    c32, aux32 = X.float32_evaluation(case, xc)
    got = _c(case, o).cpu()
    assert bool(torch.isfinite(got).all()), case.id + ': C not finite'
    S = refc['abs']
    family = case.kernel + ('-split' if case.splitk > 1 else '') + ('-gelu' if case.gelu else '')
    _bound(case.id + ' C', family, G.kind3_figure(got, refc['C'], S, False), G.kind3_figure(c32, refc['C'], S, False))
    if case.gelu:
        ga = o['aux_out'].view.cpu()[None]
        assert bool(torch.isfinite(ga).all()), case.id + ': aux_out not finite'
        _bound(case.id + ' aux_out', family, G.kind3_figure(ga, refc['aux_out'], S + 1, False), G.kind3_figure(aux32, refc['aux_out'], S + 1, False))


def _ids(c):
    return c.id


def _exact(ops, case):
    assert case.exact
    x = _inputs(case)
    _check_exact(case, x, _run(ops, case, x))


# ---------------------------------------------------------------- the operand splits
@pytest.mark.parametrize('case', X.FAMILIES['k'], ids=_ids)
def test_every_k_in_both_forms_of_every_split(ops, case):
    _exact(ops, case)


@pytest.mark.parametrize('case', X.FAMILIES['mn'], ids=_ids)
def test_rows_around_8_64_128_256(ops, case):
    _exact(ops, case)


@pytest.mark.parametrize('case', X.FAMILIES['vec'], ids=_ids)
def test_vec_ok_one_condition_at_a_time(ops, case):
    _exact(ops, case)


@pytest.mark.parametrize('case', X.FAMILIES['unroll'], ids=_ids)
def test_four_chunk_unroll_at_the_workgroup_boundary(ops, case):
    _exact(ops, case)


@pytest.mark.parametrize('case', X.POISON, ids=_ids)
def test_workspace_pads_are_rewritten_after_a_poisoned_call(ops, case):
    """The same entry point, layout and alignment at a larger shape with operands full of inf (hi = inf, lo = NaN), then the small ragged
    case on the same stream: every K pad, pad row and pad column of A3 / B3 has to be rewritten, or 0 x inf reaches C."""
    Pm, Pn, Pk = X.POISON_SHAPE
    like = lambda cols_small, pad_small, cols_big: 4 + (cols_small + pad_small - cols_big) % 4      # the same ld % 4, so the same VEC form
    big = X.Case(Pm, Pn, Pk, a_kc=case.a_kc, b_kc=case.b_kc, a_off=case.a_off, b_off=case.b_off,
                 lda_pad=like(case.K if case.a_kc else case.M, case.lda_pad, Pk if case.a_kc else Pm),
                 ldb_pad=like(case.K if case.b_kc else case.N, case.ldb_pad, Pk if case.b_kc else Pn))
    assert X.split_forms(big) == X.split_forms(case)
    inf = dict(A=torch.full((1, Pm, Pk), INF, device='cuda'), B=torch.full((1, Pn, Pk), INF, device='cuda'), bias=None, aux=None, c0=None)
    o = _run(ops, big, inf)
    assert not bool(torch.isfinite(o['C'].view).any())                         # the poison went through the product
    _exact(ops, case)


# ---------------------------------------------------------------- product kernels, split-K, batches
@pytest.mark.parametrize('case', X.FAMILIES['product'], ids=_ids)
def test_product_kernels_and_the_declines(ops, case):
    _exact(ops, case)


@pytest.mark.parametrize('case', X.FAMILIES['splitk'], ids=_ids)
def test_split_k_across_the_three_segments(ops, case):
    _exact(ops, case)


@pytest.mark.parametrize('tile', ['default', 'tile256'])
def test_split_k_refusals_leave_c_alone(ops, tile):
    from pianobart_amd._lib import PBError
    base = dict(flags=({} if tile == 'default' else X.T256), splitk=2)
    case = X._c(264, 264, 130, X.TN, **base)
    x = _inputs(case)
    bias = torch.ones(264, device='cuda')
    for what, c, over in (('bias', case, dict(bias=bias)), ('batch', case, dict(nb1=2)), ('ldc != N', X._c(264, 264, 130, X.TN, ldc_pad=8, **base), {})):
        o = _run(ops, c, x, expect_error=PBError, **over)
        o['C'].assert_untouched('%s: split-K with %s' % (case.id, what))
    _exact(ops, case)                                                          # and the same call without the offence is served


@pytest.mark.parametrize('case', X.FAMILIES['batch'], ids=_ids)
def test_batches(ops, case):
    _exact(ops, case)


@pytest.mark.parametrize('B_,H,S,hd', X.ATTN)
def test_heads_addressed_by_stride_like_the_unfused_attention(ops, B_, H, S, hd):
    """Q K^T (NT, K = head_dim) and P V (B row-contiguous: split_tr<1> with batch strides) with the heads inside (T, 3 d) rows, C strided
    through sC and c_off, all exact."""
    d, nb = H * hd, B_ * H
    q, k, v = (X.pq((nb, S, hd), 11 + i).cuda() for i in range(3))
    rows = lambda t: t.view(B_, H, S, hd).permute(0, 2, 1, 3).reshape(B_ * S, d)
    qkv = torch.cat([rows(q), rows(k), rows(v)], 1).to(F32).contiguous()
    case = X.Case(S, S, hd, nb1=B_, nb2=H, ldc_pad=4)
    ref = X.reference(case, dict(A=q, B=k, bias=None, aux=None, c0=None))
    X.assert_caps(case)
    ldc = S + 4
    sc = G.Guarded(nb * S, S, F32, 'cuda', ld=ldc, shift=4)
    ops.gemm(qkv, qkv, sc.buf, M=S, N=S, K=hd, dtype=ops.PB_F32X3, lda=3 * d, ldb=3 * d, ldc=ldc, c_f32=True, nb1=B_, nb2=H,
             sA=(S * 3 * d, hd), sB=(S * 3 * d, hd), sC=(H * S * ldc, S * ldc), a_off=0, b_off=d, c_off=sc.start)
    torch.cuda.synchronize()
    sc.assert_guards('scores')
    G.assert_equal(sc.view.reshape(nb, S, S), G.store(ref['C'], F32), 'Q K^T %dx%dx%dx%d' % (B_, H, S, hd))
    # P V: P is its own exact operand (not the softmax, whose values are not of the p + q form)
    P = X.pq((nb, S, S), 17).cuda()
    case = X.Case(S, hd, S, b_kc=False, nb1=B_, nb2=H)
    ref = X.reference(case, dict(A=P, B=v.transpose(1, 2), bias=None, aux=None, c0=None))
    X.assert_caps(case)
    ldo = d + 8
    out = G.Guarded(B_ * S, d, F32, 'cuda', ld=ldo, shift=8)
    ops.gemm(P.to(F32).contiguous(), qkv, out.buf, M=S, N=hd, K=S, dtype=ops.PB_F32X3, b_kc=False, lda=S, ldb=3 * d, ldc=ldo, c_f32=True,
             nb1=B_, nb2=H, sA=(H * S * S, S * S), sB=(S * 3 * d, hd), sC=(S * ldo, hd), b_off=2 * d, c_off=out.start)
    torch.cuda.synchronize()
    out.assert_guards('P V')
    want = G.store(ref['C'], F32).view(B_, H, S, hd).permute(0, 2, 1, 3).reshape(B_ * S, d)
    G.assert_equal(out.view.contiguous(), want.contiguous(), 'P V %dx%dx%dx%d' % (B_, H, S, hd))


# ---------------------------------------------------------------- epilogues and the post pass
@pytest.mark.parametrize('case', X.FAMILIES['epilogue'] + X.FAMILIES['mul'], ids=_ids)
def test_epilogues(ops, case):
    _exact(ops, case)


@pytest.mark.parametrize('case', X.FAMILIES['gelu'] + X.FAMILIES['real'], ids=_ids)
def test_real_valued_and_gelu_within_four_times_float32(ops, case):
    x = _inputs(case)
    _check_kind3(case, x, _run(ops, case, x))


def test_refusals_write_nothing(ops):
    from pianobart_amd._lib import PBError
    case = X._c(72, 72, 65, X.NT, epi='gelu', ldaux_pad=4)
    x = _inputs(case)
    for what, over in (('GELU with accumulate', dict(accum=True)), ('GELU with batches', dict(nb1=2))):
        o = _run(ops, case, x, expect_error=PBError, **over)
        o['C'].assert_untouched(what + ': C')
        o['aux_out'].assert_untouched(what + ': aux_out')
    plain = X._c(72, 72, 65, X.NT)
    x = _inputs(plain)
    o = _run(ops, plain, x, expect_error=PBError, K=0)
    o['C'].assert_untouched('K = 0')
    aux = torch.ones(72, 72, device='cuda')
    rd = G.Guarded(2, 72, F32, 'cuda', ld=72 + 64)
    o = _run(ops, plain, x, expect_error=PBError, rowdot=(aux, rd.view, 72 + 64))
    o['C'].assert_untouched('ROWDOT: C')
    rd.assert_untouched('ROWDOT: the row dots')
    mul = X._c(72, 72, 65, X.NT, epi='mul', ldaux_pad=4)
    xm = _inputs(mul)
    o = _run(ops, mul, xm, expect_error=PBError, accum=True)
    o['C'].assert_untouched('multiply by aux_in with accumulate')
    cs = X._c(72, 70, 65, X.NT, epi='mulcs')                                   # column sums of an N that is no multiple of 4: refused BEFORE the product
    o = _run(ops, cs, _inputs(cs), expect_error=PBError)
    o['C'].assert_untouched('column sums with N % 4: C')
    assert bool((o['colsum'].view == G.CS_PRIOR).all()), 'column sums with N % 4: colsum_out written'
    _check_exact(plain, x, _run(ops, plain, x))                                # and the call without an offence is served


# ---------------------------------------------------------------- pb_split_bf16
def _special(n):
    g = torch.Generator(device='cuda').manual_seed(5)
    x = torch.randn(n, device='cuda', generator=g) * torch.logspace(-6, 3, 264, device='cuda').repeat(-(-n // 264))[:n]
    if n >= 8:
        x[:8] = torch.tensor([0.0, -0.0, 1.0, -1.0, 3.0e38, -3.0e38, 1e-38, 65504.0], device='cuda')
    return x


@pytest.mark.parametrize('n', [0, 8, 2040, 2048, 2056, 4096 * 256 * 8 + 2056])
@pytest.mark.parametrize('values', ['p+q', 'special'])
def test_split_bf16_planes_every_size(ops, n, values):
    """n around one workgroup's 2048 elements, and past a full stride of the 4096-workgroup grid. The planes are torch's casts."""
    x = X.pq((max(n, 8),), 23).to(F32).cuda()[:n] if values == 'p+q' else _special(n)
    xg = torch.full((n + 128,), NAN, device='cuda')
    xg[64:64 + n] = x
    hi, lo = (G.Guarded(1, n or 8, BF16, 'cuda') for _ in range(2))
    if n:
        ops.split_bf16(xg[64:64 + n], hi.view, lo.view)
    else:                                                                      # an empty tensor has no address: the C entry point, with real ones
        ops.LIB.call('pb_split_bf16', ops._p(xg[64:]), ops._p(hi.view), ops._p(lo.view), 0, ops._stream())
    torch.cuda.synchronize()
    hi.assert_guards('hi'); lo.assert_guards('lo')
    if n == 0:
        hi.assert_untouched('hi, n = 0'); lo.assert_untouched('lo, n = 0')
        return
    want_hi = x.to(BF16)
    G.assert_equal(hi.view[0], want_hi, 'hi')
    G.assert_equal(lo.view[0], (x - want_hi.float()).to(BF16), 'lo')
    if values == 'p+q':
        assert torch.equal(hi.view[0].double() + lo.view[0].double(), x.double())


def test_split_bf16_refusals(ops):
    from pianobart_amd._lib import PBError
    x = torch.ones(4096, device='cuda')
    for what, (xo, ho, lo_, n) in dict(n_not_8=(0, 0, 0, 2044), x_off=(1, 0, 0, 2048), hi_off=(0, 4, 0, 2048), lo_off=(0, 0, 4, 2048)).items():
        hi, lo = G.Guarded(1, 2048, BF16, 'cuda', shift=ho), G.Guarded(1, 2048, BF16, 'cuda', shift=lo_)
        with pytest.raises(PBError):
            ops.split_bf16(x[xo:xo + n], hi.view, lo.view)
        torch.cuda.synchronize()
        hi.assert_untouched(what + ': hi'); lo.assert_untouched(what + ': lo')


def test_zz_worst_ratios():
    """Prints (pytest -s) the worst kernel / float32-torch ratio per product kernel."""
    for family, (ratio, fig) in sorted(WORST.items()):
        print('WORST %-22s ratio %6.3f   largest kernel figure %8.3g' % (family, ratio, fig))
        assert ratio <= G.MARGIN
