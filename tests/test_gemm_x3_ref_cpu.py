"""CPU: the operands, model, caps and case table of tests/gemm_x3_ref.py, which tests/test_gemm_x3_kernels_gpu.py holds pb_gemm (PB_F32X3) to.

  * x = p + q 2^-11 splits into hi = p, lo = q exactly, for every operand of the table;
  * the caps hold for every exact case, and under them a float32 evaluation of the model over a random permutation of the 3 K axis and one
    accumulated in 64-wide steps both equal the float64 model bit for bit;
  * the model is within the DERIVED bound of the true product (test_model_is_within_the_derived_bound_of_the_true_product);
  * every branch of pb_gemm_x3 has a case (the branch of a case is computed by the mirrors of gemm_x3_ref, which are checked here against
    the conditions the source states);
  * the comparison rejects what the model excludes: the lo lo term added, a lo plane zeroed, the roles of one operand exchanged.
The project's kernels are never altered to show that."""
import pytest
import torch

from tests import gemm_ref as G
from tests import gemm_x3_ref as X

F32, F64 = torch.float32, torch.float64
ALL = X.all_cases()
EXACT_CASES = [c for c in ALL if c.exact]


def _rows(case, x, limit=520):
    """The first rows of a large case: rows are independent, and the CPU need not repeat 8192 of them."""
    return dict(x, A=x['A'][:, :limit], aux=None if x['aux'] is None else x['aux'][:limit], c0=None if x['c0'] is None else x['c0'][:, :limit])


def test_unique_ids_and_every_branch_has_a_case():
    for name, fam in list(X.FAMILIES.items()) + [('poison', X.POISON)]:
        ids = [c.id for c in fam]
        assert len(fam) > 0 and len(set(ids)) == len(ids), (name, sorted(i for i in ids if ids.count(i) > 1)[:4])
    main = [c for f in X.FAMILIES.values() for c in f]
    exact = [c for c in main if c.exact]
    forms = {(i, f) for c in exact for i, f in enumerate(X.split_forms(c))}
    assert forms == {(r, f) for r in (0, 1) for f in ('kcV', 'kcS', 'rcV', 'rcS', 'tr')}           # every split kernel, role and VEC form
    assert {(i, f) for c in X.POISON for i, f in enumerate(X.split_forms(c))} == forms              # ... and each after a poisoned workspace
    for lay, want in ((X.NT, ('kc', 'kc')), (X.TN, ('rc', 'rc')), (X.NN, ('kc', 'tr')), (X.TT, ('tr', 'kc'))):
        assert tuple(f[:2] for f in X.split_forms(X._c(65, 72, 65, lay))) == want
    for lay in X.LAYOUTS:
        fam = [c for c in X.FAMILIES['k'] if (c.a_kc, c.b_kc) == lay]
        for vec in ('V', 'S'):                                                 # every K in both VEC forms of every layout's kc / rc kernels
            assert {c.K for c in fam if all(f == 'tr' or f[2] == vec for f in X.split_forms(c))} == set(X.KS)
        assert {c.M for c in X.FAMILIES['mn'] if (c.a_kc, c.b_kc) == lay} >= set(X.SIZES) and {c.N for c in X.FAMILIES['mn'] if (c.a_kc, c.b_kc) == lay} >= set(X.SIZES)
    # vec_ok: each condition alone turns VEC off for that operand and leaves the other operand's form alone
    for lay in (X.NT, X.TN):
        fam = [c for c in X.FAMILIES['vec'] if (c.a_kc, c.b_kc) == lay]
        why = lambda c: (c.a_off % 4 != 0, c.b_off % 4 != 0, (c.K if c.a_kc else c.M) + c.lda_pad, (c.K if c.b_kc else c.N) + c.ldb_pad, c.a_spad, c.b_spad, c.nbatch)
        off = {(w, why(c)) for c in fam for w, f in zip('ab', X.split_forms(c)) if f[2] == 'S'}
        assert any(w == 'a' and y[0] and not y[1] and y[2] % 4 == 0 and y[6] == 1 for w, y in off)        # A's base alone
        assert any(w == 'b' and y[1] and not y[0] and y[3] % 4 == 0 and y[6] == 1 for w, y in off)        # B's base alone
        assert any(w == 'a' and not y[0] and y[2] % 4 for w, y in off) and any(w == 'b' and not y[1] and y[3] % 4 for w, y in off)   # ld alone
        assert any(w == 'a' and not y[0] and y[2] % 4 == 0 and y[4] % 4 for w, y in off)                   # A's batch stride alone
        assert any(w == 'b' and not y[1] and y[3] % 4 == 0 and y[5] % 4 for w, y in off)
        assert {c.a_off for c in fam} >= {1, 2} and {c.b_off for c in fam} >= {1, 2}
        assert any(c.nbatch > 1 and X.split_forms(c) in (('kcV', 'kcV'), ('rcV', 'rcV')) for c in fam)
    # the four-chunk unroll: a full workgroup, one just past it, and a part of one
    n = {X.chunks(c, w) for c in X.FAMILIES['unroll'] for w in 'ab'}
    assert 1024 in n and 1032 in n and any(v % 1024 and v < 1024 for v in n)
    # product kernels and the 128-tile threshold; the declines of pb_gemm2_try
    prod = X.FAMILIES['product']
    assert {c.kernel for c in prod} == {'tile128', 'pingpong', 'generic'}
    assert any(c.kernel == 'pingpong' and -(-c.M // 256) * -(-c.N // 256) == 128 and c.a_kc for c in prod)
    assert any(c.kernel == 'pingpong' and not c.a_kc and not c.b_kc for c in prod) and any(c.kernel == 'tile128' and c.M > 7000 for c in prod)
    gen = [c for c in prod if c.kernel == 'generic']
    assert any(c.N % 8 for c in gen) and any(c.M % 8 and not c.N % 8 and not c.a_kc and not c.b_kc for c in gen)
    assert any(c.c_off % 4 for c in gen) and any((c.N + c.ldc_pad) % 4 and not c.N % 8 for c in gen) and any(c.flags.get('force_v1') for c in gen)
    assert X.product_kernel(X._c(268, 264, 65, X.NT)) == 'tile128'             # M % 8 only matters under a row-contiguous A3
    # split-K: a cut inside a segment, cuts on the segment boundaries, empty slabs; both tiles, with and without accumulate
    sk = X.FAMILIES['splitk']
    assert {(c.K, c.splitk) for c in sk} == set(X.SPLITS)
    assert [X.slab_cuts(X._c(72, 72, k, X.NT, splitk=s)) for k, s in X.SPLITS] == [(1, 0, 0), (0, 2, 0), (0, 2, 1), (0, 2, 1)]
    assert {(c.kernel, c.accum) for c in sk} == {(k, a) for k in ('tile128', 'pingpong') for a in (False, True)}
    # batches, epilogues, both forms of the post pass
    assert {c.kernel for c in X.FAMILIES['batch'] if c.nbatch > 1} == {'tile128', 'pingpong', 'generic'}
    assert {c.epi for c in X.FAMILIES['epilogue']} == set(X.EPI_LIST) and {c.alpha for c in X.FAMILIES['epilogue']} == {1.0, 0.5, -2.0}
    assert {c.kernel for c in X.FAMILIES['epilogue']} == {'tile128', 'generic'}
    for epi in ('mul', 'gelu'):
        fam = X.FAMILIES[epi]
        assert all(c.epi == epi for c in fam) and {X.post_vec(c) for c in fam} == {True, False}
        scalar = [c for c in fam if not X.post_vec(c)]
        ld = lambda c: ((c.N + c.ldc_pad) % 4 != 0, (c.N + c.ldaux_pad) % 4 != 0)
        assert any(c.c_off % 4 and not c.aux_off % 4 and ld(c) == (False, False) for c in scalar)
        assert any(c.aux_off % 4 and not c.c_off % 4 and ld(c) == (False, False) for c in scalar)
        assert any(ld(c) == (True, False) and not c.c_off % 4 for c in scalar) and any(ld(c) == (False, True) for c in scalar)
        assert any(X.post_vec(c) and c.N % 4 for c in fam) and any(X.post_vec(c) and c.c_off and c.aux_off for c in fam)
    real = X.FAMILIES['real']
    assert {c.kernel for c in real if c.epi == 'real'} == {'tile128', 'pingpong', 'generic'} and {c.splitk for c in real} == {1, 3}
    assert {X.post_vec(c) for c in real if c.epi == 'gelu'} == {True, False}
    for Pm, Pn, Pk in [X.POISON_SHAPE]:                                        # the poisoning call covers the small case's whole workspace and has no pad
        assert Pk % 64 == 0 and Pm % 8 == 0 and Pn % 8 == 0
        for c in X.POISON:
            small = 3 * X.kp(c.K) * (-(-c.M // 8) * 8 + -(-c.N // 8) * 8) * 2 + 512
            assert small <= 3 * Pk * min(Pm, Pn) * 2 and c.M <= Pm and c.N <= Pn and c.K <= Pk


def test_the_operands_split_exactly_into_p_and_q():
    x = X.pq((130, 1000), 3)
    p = x.round()
    q = (x - p) * X.UNIT
    assert torch.equal(q, q.round()) and float(q.abs().max()) == 3 and float(p.abs().max()) == 2
    assert set(p.unique().tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0} and set(q.unique().tolist()) == {float(v) for v in range(-3, 4)}
    assert bool((q[p == 0] == 0).all())                                        # no hi hi product finer than 1
    assert torch.equal(x.to(F32).double(), x)                                  # float32 holds x
    hi, lo = X.planes(x)
    assert torch.equal(hi, p) and torch.equal(lo, q / X.UNIT) and torch.equal(hi + lo, x)
    assert 0.6 < float((lo != 0).double().mean()) < 0.75                       # the lo planes are exercised: 4/5 * 6/7 = 69 %
    seen = set()
    for case in EXACT_CASES:                                                   # ... and for the operands of the table (they depend on shape and seed alone)
        key = (case.M, case.N, case.K, case.nbatch, case.seed)
        if key in seen:
            continue
        seen.add(key)
        for t in X.make_ab(case):
            hi, lo = X.planes(t[:, :520])
            assert torch.equal(hi, t[:, :520].round()) and torch.equal(hi + lo, t[:, :520])


def _perm_and_stepped(case, x3):
    """Two float32 evaluations of sum_k A3 B3: over a random permutation of the 3 K axis, and accumulated in 64-wide steps."""
    A, B = x3['A'].to(F32), x3['B'].to(F32)
    perm = torch.randperm(A.shape[2], generator=torch.Generator().manual_seed(case.K))
    permuted = A[:, :, perm] @ B[:, :, perm].transpose(1, 2)
    stepped = torch.zeros_like(permuted)
    for k0 in range(0, A.shape[2], 64):
        stepped = stepped + A[:, :, k0:k0 + 64] @ B[:, :, k0:k0 + 64].transpose(1, 2)
    return permuted, stepped


def test_caps_hold_and_float32_is_exact_in_any_order_for_every_case_of_the_table():
    seen = set()
    with_colsum = 0
    for case in EXACT_CASES:
        X.assert_caps(case) if not case.colsum else None
        key = (case.M, case.N, case.K, case.nbatch, case.seed)
        if key in seen and not case.colsum:
            continue                                                           # the operands depend on the shape and the seed alone
        seen.add(key)
        x = _rows(case, X.make_inputs(case))
        ref = X.reference(case, x)
        if case.colsum:
            X.assert_caps(case, G.store(ref['C'], F32))
            with_colsum += 1
        assert torch.equal(G.store(ref['C'], F32).double(), ref['C']), case.id  # float32 holds the reference
        assert float(ref['acc'].abs().max()) <= 4 * case.K + 8
        assert torch.equal(ref['acc'] * X.UNIT, (ref['acc'] * X.UNIT).round())
        for what, got in zip(('permuted', 'stepped'), _perm_and_stepped(case, X.triple(x))):
            assert torch.equal(got.double(), ref['acc']), '%s: the %s float32 sum is not the float64 model' % (case.id, what)
    assert with_colsum >= 4
    with pytest.raises(AssertionError):                                        # and the check can fail
        X.assert_caps(X.Case(64, 64, 1024, alpha=0.5))
    X.assert_caps(X.Case(64, 64, 1000, alpha=0.5))


def test_the_issue_shape_130x72x1000():
    case = X.Case(130, 72, 1000)
    x = X.make_inputs(case)
    ref = X.reference(case, x)
    X.assert_caps(case)
    for got in _perm_and_stepped(case, X.triple(x)):
        assert torch.equal(got.double(), ref['acc'])
    assert float(ref['C'].abs().max()) * X.UNIT < 1e6 < G.EXACT


def test_the_model_is_within_the_derived_bound_of_the_true_product():
    """|model - sum_k a b| <= C_MODEL sum_k |a b| per element, C_MODEL = 2^-16 ((1 + 2^-8)^2 + 2 + 2^-16) = 3.008 2^-16 = 4.59e-5.

    bf16 keeps 8 significant bits, so round-to-nearest gives |x - hi| <= 2^-8 |x| (attained: x = 1 + 2^-8 is a tie and goes to 1; the
    2^-9 one might expect is half an ulp relative to the NEXT power of two, and is exceeded by every x just above a power of two -- asserted
    at the end). lo = bf16(x - hi) is the same rounding of the exactly formed remainder: r = x - hi - lo has |r| <= 2^-8 |x - hi| <=
    2^-16 |x|, and |lo| <= |x - hi| + |r| <= 2^-8 (1 + 2^-8) |x|. With a = a_hi + a_lo + r_a and b likewise,
        a b - (a_hi b_hi + a_hi b_lo + a_lo b_hi) = a_lo b_lo + r_a b + (a - r_a) r_b,
    whose magnitude is at most (2^-16 (1 + 2^-8)^2 + 2^-16 + 2^-16 + 2^-32) |a b|. Summing over k gives the bound; it is per element and scaled
    by the cancellation-free sum of THAT element (the earlier tests use 2e-5 of the largest |C| of the matrix, a figure without a derivation:
    as a worst case it is not true of the arithmetic, as a typical figure it is ten times what randn operands give). Values whose lo would be
    subnormal in bf16 are not in randn operands. Both sides are evaluated in float64, whose own error (1e-13 of sum |a b| at K = 1000) is
    far below the bound's slack."""
    assert X.C_MODEL == 2.0 ** -16 * ((1 + 2.0 ** -8) ** 2 + 2 + 2.0 ** -16) and 4.58e-5 < X.C_MODEL < 4.6e-5
    worst = 0.0
    for case in [c for c in X.FAMILIES['real'] if c.epi == 'real'] + [X.Case(130, 72, 1000, epi='real')]:
        x = X.make_inputs(case)
        model = X.reference(case, x)['acc']
        true = x['A'] @ x['B'].transpose(1, 2)
        S = x['A'].abs() @ x['B'].abs().transpose(1, 2)
        fig = float(((model - true).abs() / S).max())
        print('MODEL %-60s max |model - true| / sum |a b| = %.3g  (bound %.3g; 2^-16 = %.3g)' % (case.id, fig, X.C_MODEL, 2.0 ** -16))
        assert bool(((model - true).abs() <= X.C_MODEL * S).all()), (case.id, fig)
        worst = max(worst, fig)
    assert worst > 2.0 ** -24                                                  # the model does differ from the true product: the bound is not vacuous
    # element by element, for values that sit at every 20-bit significand of one binade: |lo| and the residual stay inside their bounds and come within a factor 2 / 4 of them
    v = 1 + torch.arange(1, 1 << 20, dtype=F64) / (1 << 20)
    hi, lo = X.planes(v)
    r = v.to(F32).double() - hi - lo
    assert float((lo.abs() / v).max()) <= 2.0 ** -8 * (1 + 2.0 ** -8) and float((r.abs() / v).max()) <= 2.0 ** -16
    assert float((lo.abs() / v).max()) > 2.0 ** -9 and float((r.abs() / v).max()) > 2.0 ** -18


# ---------------------------------------------------------------- the comparison rejects what the model excludes
def _tampered(case, x, what):
    ah, al = X.planes(x['A'])
    bh, bl = X.planes(x['B'])
    t = lambda m: m.transpose(1, 2)
    model = ah @ t(bh) + ah @ t(bl) + al @ t(bh)
    if what == 'model':
        return model
    if what == 'lo lo added':
        return model + al @ t(bl)
    if what == 'lo of A zero in the last K chunk':
        k0 = (case.K - 1) // 8 * 8
        return model - al[:, :, k0:] @ t(bh[:, :, k0:])
    if what == 'roles of B exchanged':                                         # B3 = [hi | hi | lo] against A3 = [hi | hi | lo]
        return ah @ t(bh) + ah @ t(bh) + al @ t(bl)
    if what == 'one pad row of the split dropped':
        return model - (ah[:, :, -1:] @ t(bh[:, :, -1:]) + ah[:, :, -1:] @ t(bl[:, :, -1:]) + al[:, :, -1:] @ t(bh[:, :, -1:]))
    raise KeyError(what)


def test_the_exact_comparison_rejects_a_wrong_triple():
    case = X.Case(65, 72, 65)
    x = X.make_inputs(case)
    ref = G.store(X.reference(case, x)['C'], F32)
    G.assert_equal(G.store(_tampered(case, x, 'model'), F32), ref, 'C')
    for what in ('lo lo added', 'lo of A zero in the last K chunk', 'roles of B exchanged', 'one pad row of the split dropped'):
        with pytest.raises(AssertionError):
            G.assert_equal(G.store(_tampered(case, x, what), F32), ref, what)
    # the per-element bound of the real-valued cases sees the zeroed lo chunk as well
    case = X.Case(264, 264, 100, epi='real')
    x = X.make_inputs(case)
    ref = X.reference(case, x)
    bad = _tampered(case, x, 'lo of A zero in the last K chunk')
    f32, _ = X.float32_evaluation(case, x)
    fig32 = G.kind3_figure(f32, ref['C'], ref['abs'], False)
    assert 0 < fig32 < 2 and G.kind3_figure(bad, ref['C'], ref['abs'], False) > 10 * G.MARGIN * fig32


def test_place_batches_lengthens_the_batch_stride():
    case = X.Case(5, 8, 16, nb1=2, nb2=3, a_spad=3)
    A = X.make_inputs(case)['A']
    for kc in (True, False):
        buf, ld, stride = X.place_batches(A, kc, 4, 2, 3)
        assert ld == (16 if kc else 5) + 4 and stride == (5 if kc else 16) * ld + 3
        for z, m, k in ((0, 0, 0), (5, 4, 15), (3, 2, 7)):
            assert float(buf[2 + z * stride + (m * ld + k if kc else k * ld + m)]) == float(A[z, m, k])
        assert int(torch.isnan(buf).sum()) == buf.numel() - A.numel()
        same = X.place_batches(A, kc, 4, 2, 0)
        ref = G.place(A, kc, 4, 2, F32)
        assert same[1:] == ref[1:] and torch.equal(torch.nan_to_num(same[0]), torch.nan_to_num(ref[0]))
    case = X.Case(65, 72, 65, a_kc=False, b_kc=False, nb1=2, nb2=3, a_spad=1, lda_pad=7)
    assert X.batch_stride(case, 'a') == 65 * 72 + 1 and X.split_forms(case)[0] == 'rcS'
