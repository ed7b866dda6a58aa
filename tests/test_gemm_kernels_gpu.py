"""GPU: the GEMM kernels behind pb_gemm (csrc/pb_gemm.hip, pb_gemm2.hip) at every tile, split and epilogue edge, against the float64
references of tests/gemm_ref.py (checked without a GPU in tests/test_gemm_ref_cpu.py). Everything goes through pianobart_amd.ops.gemm.

Three kinds of assertion, the first two without a tolerance:
  1. exact (the bulk). A and B hold integers from [-2, 2], bias from [-8, 8], aux_in from [-2, 2], the old C of an accumulate from [-64, 64],
     alpha is 1, 0.5 or -2. Operands are bf16 (or f32) and accumulation is f32, so every product and partial sum is an integer below 2^24
     and the f32 result is that integer WHATEVER the summation order -- across K tiles, split-K slabs, tail-split partials, MFMA lanes and
     the column-sum / row-dot trees. The reference is a float64 matmul of the same integers and the epilogue in float64, rounded once
     (.to(float32).to(bfloat16)) for a bf16 C: torch.equal on C, on the f32 C of split-K with and without accumulate, on colsum_out (prior
     contents + column sums of the STORED values) and on the row dots (sums over each 64-column group of stored C * aux). A dropped,
     doubled, misplaced or mis-split contribution changes an integer. The caps that make this exact are conditions on the reference
     (gemm_ref.caps: 4 K + 8 < 2^24; per column sum_m |stored C| + |prior| < 2^24; per row dot 64 max|C| 2 < 2^24) and are asserted in
     every case here and for the whole table on the CPU.
  2. guards. Every output -- C (bf16 or f32), aux_out, colsum_out (N floats inside N + 16), the row dots (ld_rowdot = M + 64), the split-K
     slabs -- is a view inside a larger allocation. The interior starts as NaN; before the first and after the last element, and in the
     pad columns of ldc > N, ldaux > N and ld_rowdot > M, sits a finite sentinel (a stray store changes it and so does a stray
     read-modify-write; for the row dots this asks more than "the tail columns stay NaN"). After the call the interior equals the
     reference, so it holds no NaN, and every sentinel is untouched. The slabs and the column-sum workspace are prefilled with NaN (the
     slabs' surroundings too): a slab or partial row the kernel failed to write reaches C / colsum_out as NaN. The operands sit in NaN as
     well -- pad columns of lda / ldb / ldaux, the elements in front and behind, bias -- so a read outside a matrix poisons the sum.
  3. float64 with a per-element bound, only where the arithmetic is not exact: the GELU epilogue (C = gelu, aux_out = gelu') and one
     real-valued (randn) case per kernel, where an error that integers hide (a partial sum kept at reduced precision) would show. Inputs
     are rounded to the storage dtype first. |got - ref| <= k 2^-24 S (+ 2^-8 |ref| for bf16 storage), S = |alpha| sum_k |a_mk b_nk| + |bias|
     (+ 1 for gelu', whose own magnitude is 1). k is FOUR times the same figure of a plain float32 torch evaluation of the same formula
     on the same rounded inputs, computed in the test (the row suite's margin: it covers the other summation order); no bound was taken
     from a kernel's own error. The tiled bf16 kernels' GELU uses the Abramowitz-Stegun erf of pb_common.h (|error| <= 1.5e-7): its share,
     0.5 * 1.5e-7 |v| in gelu = v (1 + erf) / 2 and 0.5 * 1.5e-7 in gelu', is added to the float32 figure before the margin applies.
     _bound() prints both figures of every check and test_zz_worst_ratios the worst per family (pytest -s).

Branches (pb_gemm -> pb_gemm2_try; `kernel` in a case id is the row it is expected to take):
  generic    pb_gemm.hip gemm_kernel, 128 x 128, BK = 64 (bf16) / 32 (f32), scalar epilogue: PB_GEMM_FORCE_V1, every f32 case, and what
             pb_gemm2_try declines: K % 64, N % 8, M % 8 under a row-contiguous A, an operand or C off 16 bytes, an ld that is no multiple
             of 8 (C f32: 4). Column sums by the streaming pass (pb_colsum). Partial vectors of a K / row tail go element by element.
  tile128    gemm2_kernel<.,.,2,2,4,4>, 128 x 128, epilogue_regs for every tile: PB_GEMM_TILE128, and by default below M 2048 or N 512
             (test_default_dispatch: both sides of M >= 2048 && N >= 512). Column sums by the streaming pass.
  onebar256  gemm2_kernel<.,.,2,4,8,4>, 256 x 256, epilogue_regs: PB_GEMM_TILE256 with a mixed layout (NN, TT), or NT / TN with dbg 2048.
             Column sums by the streaming pass.
  pingpong   gemm3_kernel<AK,BK,4>, 256 x 256, persistent, K tiles t+1 / t+2 prefetched in four phases: PB_GEMM_TILE256 (or the default
             above the threshold) with NT or TN. Epilogue per tile: NT interior tiles -- store / bias / alpha -> epilogue_plain (row-staged);
             accumulate into bf16 C -> epilogue_pf<2> (asm, row-staged); * aux_in -> epilogue_pf<1>, with fused column sums
             epilogue_pf<1, true>; GELU pair -> epilogue_gelu; row dots -> epilogue_pf<3> (whole tiles only, the host refuses the rest);
             f32 C, with or without accumulate -> epilogue_regs. NT edge tiles and dbg 256 -> epilogue_regs. TN: interior plain f32 C
             without bias -> epilogue_f32_plain (the split-K slabs), everything else epilogue_regs. Column sums fused (cs_ws) for both.
             520 x 520 is the mixed launch: 3 x 3 tiles, 4 interior, 5 edge. 512 x 512 interior only, 264 x 264 edge only.
  split-K    nsplit > 1: f32 slabs (a.C = slabs, ldc = N), Kc = ceil(nkt / nsplit) * 64, then reduce_slabs_kernel over ALL nsplit slabs;
             (nkt, nsplit) = (5, 4) and (9, 8) leave empty splits (nk = 0: the kernels store zeros). tile128 -> gemm2_kernel, tile256 ->
             pingpong. bf16 C, a bias, batches and ldc != N are refused (PBError) and leave C alone.
  persistent several work items per workgroup of the ping-pong kernel (the hand-counted `pend` waits): ncu + 2 and 2 ncu + 4 tiles, each
             epilogue against the reference and against dbg 4096 (plain grid).
  tail / row split   PB_GEMM_TAIL_SPLIT (32768) / PB_GEMM_ROW_SPLIT (65536) only allow the split; the cost model decides from ncu
             (mirrored in gemm_ref.tail_split_factor / row_split_rows). With the flag and without, C must EQUAL the reference. Where the
             model (or the layout: NN never reaches the ping-pong kernel) does not take the split, the case is checked and then skipped.

Measured on an MI355X, worst kernel / float32-torch ratio of kind 3 over the cases of a kernel (in brackets the largest kernel figure, in
units of 2^-24 S); the bound is 4:
  f32 C, real operands (520 x 520 x 320)   tile128, pingpong NT / TN, onebar256 NT / NN, generic bf16: 1.13 (1.40), the same bits from all six
  split-K 3 x f32 slabs (264 x 264 x 448)  tile128, pingpong TN: 0.68 (0.76)
  bf16 C, real operands and the GELU pair  tiled kernels: C at most 0.004 (0.008), gelu' 0; generic bf16 (erff): C 0.06 (0.13), gelu' 0.03 (0.02);
                                           ping-pong at 33 024 / 65 800 rows: C 0.04 (0.14), gelu' 0 -- the error stays inside the bf16 ulp
  generic f32 (264 x 264 x 100)            C 1.00 (3.98), gelu 1.00 (3.77), gelu' 1.00 (1.59): the same bits as the float32 matmul of torch
Skipped there (256 CUs): the three NN tail-split cases (the layout never reaches the ping-pong kernel); every NT tail and row split is taken.
"""
import pytest
import torch

from tests import gemm_ref as G

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
NAN = float('nan')
WORST = {}


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from pianobart_amd import ops as o
    return o


def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count // 8 * 8      # pb_num_cus()


# ---------------------------------------------------------------- helpers
_AB = {}


def _inputs(case, keep_a_in_storage_dtype=False):
    """make_inputs on the device. The operand pair of the last (shape, seed) is kept: the epilogues of one shape share it."""
    key = (case.M, case.N, case.K, case.nbatch, case.seed, case.exact, case.dt, keep_a_in_storage_dtype)
    if key not in _AB:
        _AB.clear()
        A, B = G.make_ab(case)
        _AB[key] = (A.to(case.in_dtype).cuda() if keep_a_in_storage_dtype else A.cuda(), B.cuda())
    x = G.make_inputs(case, ab=_AB[key])
    return {k: (None if v is None else v.cuda()) for k, v in x.items()}


def _nan_wrapped(t, dtype, pad=64):
    buf = torch.full((t.numel() + 2 * pad,), NAN, dtype=dtype, device='cuda')
    buf[pad:pad + t.numel()] = t.reshape(-1).to(dtype)
    return buf[pad:pad + t.numel()]


def _run(ops, case, x, dbg=0, expect_error=None, **override):
    """One ops.gemm call of the case with every output guarded. -> dict of gemm_ref.Guarded (C, aux_out, colsum, rowdot, slabs).
    The guards are checked here; the contents by the caller."""
    M, N, K, nb = case.M, case.N, case.K, case.nbatch
    idt, cdt = case.in_dtype, case.c_dtype
    A, lda, sa = G.place(x['A'], case.a_kc, case.lda_pad, case.a_off, idt)
    B, ldb, sb = G.place(x['B'], case.b_kc, case.ldb_pad, case.b_off, idt)
    ldc = N + case.ldc_pad
    o = dict(C=G.Guarded(nb * M, N, cdt, 'cuda', ld=ldc, shift=case.c_off, init=(x['c0'].reshape(nb * M, N) if case.acc else None)))
    kw = dict(M=M, N=N, K=K, dtype=ops.dtype_code(idt), a_kc=case.a_kc, b_kc=case.b_kc, lda=lda, ldb=ldb, ldc=ldc, alpha=case.alpha,
              accum=case.acc, c_f32=case.c32, a_off=case.a_off, b_off=case.b_off, c_off=o['C'].start, nb1=case.nb1, nb2=case.nb2)
    if nb > 1:
        kw.update(sA=(case.nb2 * sa, sa), sB=(case.nb2 * sb, sb), sC=(case.nb2 * M * ldc, M * ldc))
    if case.bias:
        kw['bias'] = _nan_wrapped(x['bias'], F32)
    if case.mul or case.rowdot:
        aux, ldaux, _ = G.place(x['aux'][None], True, case.ldaux_pad if case.mul else case.ldc_pad, 0, idt)
        if case.mul:
            kw.update(gelu_grad_aux_in=aux, ldaux=ldaux)
        else:
            o['rowdot'] = G.Guarded(N // 64, M, F32, 'cuda', ld=M + 64)
            kw['rowdot'] = (aux, o['rowdot'].view, M + 64)
    if case.gelu:
        o['aux_out'] = G.Guarded(M, N, idt, 'cuda', ld=N + case.ldaux_pad)
        kw.update(gelu_aux_out=o['aux_out'].view, ldaux=N + case.ldaux_pad)
    if case.colsum:
        o['colsum'] = G.Guarded(1, N, F32, 'cuda', pad=8, init=torch.full((1, N), G.CS_PRIOR))
        ws = torch.full((int(ops.LIB.query('pb_gemm_colsum_ws_floats', M, N)),), NAN, device='cuda')
        kw.update(colsum_out=o['colsum'].view, colsum_ws=ws)
    if case.splitk > 1:
        o['slabs'] = G.Guarded(1, case.splitk * M * N, F32, 'cuda', pad=4096, guard=NAN)
        kw.update(splitk=case.splitk, slabs=o['slabs'].view)
    flags = dict(case.flags)
    kw['dbg'] = flags.pop('dbg', 0) | dbg
    kw.update(flags)
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
    ref = G.reference(case, x)
    stored = G.store(ref['C'], case.c_dtype)
    G.assert_caps(case, stored)
    tag = case.id + what
    G.assert_equal(_c(case, o), stored, tag + ': C')
    if case.colsum:
        G.assert_equal(o['colsum'].view[0], G.colsum_reference(case, stored), tag + ': colsum_out')
    if case.rowdot:
        G.assert_equal(o['rowdot'].view.contiguous(), G.rowdot_reference(case, stored, x['aux']), tag + ': rowdot')
    if case.splitk > 1:
        slabs = o['slabs'].view.view(case.splitk, case.M, case.N)
        assert bool(torch.isfinite(slabs).all()), tag + ': a slab element was not written'
        G.assert_equal(slabs.double().sum(0), case.alpha * ref['acc'][0], tag + ': sum of the slabs')
    return stored


def _same_bits(case, a, b, what):
    for name in a:
        if name != 'slabs':
            G.assert_equal(a[name].view.contiguous(), b[name].view.contiguous(), '%s: %s, %s' % (case.id, name, what))


def _bound(what, family, kernel, f32):
    ratio = kernel / f32 if f32 > 0 else (0.0 if kernel == 0 else float('inf'))
    print('RATIO %-72s kernel %10.4g   float32 torch %10.4g   ratio %6.3f' % (what, kernel, f32, ratio))
    w = WORST.setdefault(family, [0.0, 0.0])
    w[0], w[1] = max(w[0], ratio), max(w[1], kernel)
    assert kernel <= G.MARGIN * f32, '%s: kernel %.4g > %g x float32 torch %.4g' % (what, kernel, G.MARGIN, f32)


def _check_kind3(case, x, o):
    xc = {k: (None if v is None else v.cpu()) for k, v in x.items()}          # reference and yardstick both on the CPU
    refc = G.reference(case, xc)
    c32, aux32 = G.float32_evaluation(case, xc)
    bf = case.c_dtype == BF16
    fast_erf = case.gelu and case.dt == 'bf16' and case.kernel != 'generic'     # gelu_both_fast; the generic kernel and f32 use erff
    got = _c(case, o).cpu()
    assert bool(torch.isfinite(got).all()), case.id + ': C not finite'
    S = refc['abs']
    extra = G.MARGIN * 0.5 * G.ERF_ERR * refc['pre'].abs() if fast_erf else None
    _bound(case.id + ' C', case.kernel, G.kind3_figure(got, refc['C'], S, bf, extra), G.kind3_figure(c32, refc['C'], S, False))
    if case.gelu:
        ga = o['aux_out'].view.cpu()[None]
        assert bool(torch.isfinite(ga).all()), case.id + ': aux_out not finite'
        extra = torch.full_like(S, G.MARGIN * 0.5 * G.ERF_ERR) if fast_erf else None
        _bound(case.id + ' aux_out', case.kernel, G.kind3_figure(ga, refc['aux_out'], S + 1, case.in_dtype == BF16, extra),
               G.kind3_figure(aux32, refc['aux_out'], S + 1, False))


def _ids(c):
    return c.id


# ---------------------------------------------------------------- the tile edges of every kernel
@pytest.mark.parametrize('case', G.FAMILIES['tile128'], ids=_ids)
def test_tile128_every_edge(ops, case):
    x = _inputs(case)
    _check_exact(case, x, _run(ops, case, x))


@pytest.mark.parametrize('case', G.FAMILIES['tile256'], ids=_ids)
def test_tile256_every_edge_and_k_tile_count(ops, case):
    x = _inputs(case)
    _check_exact(case, x, _run(ops, case, x))


@pytest.mark.parametrize('case', G.FAMILIES['default'], ids=_ids)
def test_default_dispatch(ops, case):
    x = _inputs(case)
    _check_exact(case, x, _run(ops, case, x))


@pytest.mark.parametrize('case', G.FAMILIES['generic'], ids=_ids)
def test_generic_kernel_every_edge(ops, case):
    x = _inputs(case)
    _check_exact(case, x, _run(ops, case, x))


@pytest.mark.parametrize('case', G.FAMILIES['ld'], ids=_ids)
def test_leading_dimensions_offsets_batches(ops, case):
    x = _inputs(case)
    _check_exact(case, x, _run(ops, case, x))


# ---------------------------------------------------------------- epilogues
@pytest.mark.parametrize('case', G.FAMILIES['epilogue'] + G.FAMILIES['rowdot'], ids=_ids)
def test_epilogues(ops, case):
    x = _inputs(case)
    o = _run(ops, case, x)
    _check_exact(case, x, o)
    if case.kernel == 'pingpong':                                              # the register epilogue gives the same bits
        o2 = _run(ops, case, x, dbg=256)
        _check_exact(case, x, o2, ' (dbg 256)')
        _same_bits(case, o, o2, 'dbg 256 against the default')


@pytest.mark.parametrize('case', G.FAMILIES['kind3'], ids=_ids)
def test_real_valued_and_gelu_within_four_times_float32(ops, case):
    x = _inputs(case)
    o = _run(ops, case, x)
    _check_kind3(case, x, o)
    if case.kernel == 'pingpong' and case.splitk == 1:
        _same_bits(case, o, _run(ops, case, x, dbg=256), 'dbg 256 against the default')


# ---------------------------------------------------------------- split-K
@pytest.mark.parametrize('case', G.FAMILIES['splitk'], ids=_ids)
def test_split_k(ops, case):
    x = _inputs(case)
    _check_exact(case, x, _run(ops, case, x))


@pytest.mark.parametrize('tile', ['tile128', 'tile256'])
def test_split_k_refusals_leave_c_alone(ops, tile):
    from pianobart_amd._lib import PBError
    base = dict(a_kc=False, b_kc=False, flags={tile: True}, splitk=4)
    case = G.Case(264, 136, 320, **base)
    x = _inputs(case)
    bias = torch.ones(136, device='cuda')
    for what, c, over in (('bf16 C', case, dict(c_f32=False)), ('bias', case, dict(bias=bias)), ('batch', case, dict(nb1=2)),
                          ('ldc != N', G.Case(264, 136, 320, ldc_pad=8, **base), {})):
        o = _run(ops, c, x, expect_error=PBError, **over)
        o['C'].assert_untouched('%s: split-K with %s' % (case.id, what))
    _check_exact(case, x, _run(ops, case, x))                                  # and the same call without the offence is served


# ---------------------------------------------------------------- several work items per persistent workgroup
@pytest.mark.parametrize('epi', G.PERSISTENT_EPIS)
@pytest.mark.parametrize('which', [0, 1], ids=['ncu+2_tiles', '2ncu+4_tiles'])
def test_persistent_workgroups_take_several_items(ops, which, epi):
    rows = G.persistent_rows(_ncu())[which]
    cases = [c for c in G.persistent_cases(_ncu()) if c.seed == which and c.epi == epi]
    assert cases and all(-(-c.M // 256) == -(-rows // 256) for c in cases)
    for case in cases:
        assert -(-case.M // 256) * 2 > (which + 1) * _ncu()
        x = _inputs(case)
        o = _run(ops, case, x)
        if case.exact:
            _check_exact(case, x, o)
        else:
            _check_kind3(case, x, o)
        o2 = _run(ops, case, x, dbg=4096)
        _same_bits(case, o, o2, 'the plain grid (dbg 4096) against the persistent one')
        del o, o2, x


# ---------------------------------------------------------------- tail split and row split
def _check_rows_exact(case, x, o, what):
    for r0 in range(0, case.M, 4096):                                          # the float64 reference in row chunks
        r1 = min(case.M, r0 + 4096)
        stored = G.store(G.reference(case, x, r0, r1)['C'], case.c_dtype)
        G.assert_equal(o['C'].view[r0:r1].contiguous(), stored[0], '%s %s: C rows %d..%d' % (case.id, what, r0, r1))


def _split_case(ops, shape, epi, flag, taken, why_not):
    M, N, K, b_kc = shape
    case = G.Case(M, N, K, b_kc=b_kc, epi=epi, kernel='pingpong' if b_kc else 'onebar256')
    G.assert_caps(case)
    x = _inputs(case, keep_a_in_storage_dtype=True)
    for dbg in (0, flag):
        o = _run(ops, case, x, dbg=dbg)
        _check_rows_exact(case, x, o, 'dbg %d' % dbg)
        del o
    if not taken:
        pytest.skip('exact with and without the flag, but %s' % why_not)


@pytest.mark.parametrize('epi', G.SPLIT_EPIS)
@pytest.mark.parametrize('shape', G.TAIL_SHAPES, ids=lambda s: '%dx%dx%d-%s' % (s[0], s[1], s[2], 'NT' if s[3] else 'NN'))
def test_tail_split_is_exact(ops, shape, epi):
    M, N, K, b_kc = shape
    sp = G.tail_split_factor(M, N, K, _ncu()) if b_kc else 1
    _split_case(ops, shape, epi, 32768, sp > 1, 'the NN layout takes the one-barrier kernel, which has no tail split' if not b_kc else
                'the cost model of pb_gemm2_try does not take the tail split at %d CUs' % _ncu())


@pytest.mark.parametrize('epi', G.SPLIT_EPIS)
@pytest.mark.parametrize('shape', G.ROW_SHAPES, ids=lambda s: '%dx%dx%d-%s' % (s[0], s[1], s[2], 'NT' if s[3] else 'NN'))
def test_row_split_is_exact(ops, shape, epi):
    M, N, K, b_kc = shape
    main = G.row_split_rows(M, N, K, _ncu()) if b_kc else M
    _split_case(ops, shape, epi, 65536, main < M, 'the cost model of pb_gemm2_try does not take the row split at %d CUs' % _ncu())


def test_zz_worst_ratios():
    """Prints (pytest -s) the worst kernel / float32-torch ratio of kind 3 per kernel: the docstring's figures."""
    for family, (ratio, fig) in sorted(WORST.items()):
        print('WORST %-10s ratio %6.3f   largest kernel figure %8.3g' % (family, ratio, fig))
        assert ratio <= G.MARGIN
