"""CPU: the references, caps and comparison helpers of tests/gemm_ref.py, which tests/test_gemm_kernels_gpu.py holds the GEMM kernels to.

  * the float64 reference of every exact operand maker equals an int64 evaluation of the same epilogue;
  * the caps that make float32 exact in any summation order hold for EVERY case of the GPU case table (imported, so the two cannot drift);
  * the comparison helpers reject a wrong answer: a copy of the reference perturbed here, in torch -- one element one bf16 ulp off, two rows
    exchanged, one K tile's contribution missing from one output tile, one split-K slab counted twice, a sentinel overwritten, a partial sum
    kept in bf16 (kind 3). The project's kernels are never altered to show that."""
import math

import pytest
import torch

from tests import gemm_ref as G

F64 = torch.float64
ALL = G.all_cases(256)
EXACT_CASES = [c for c in ALL if c.exact]


def test_the_table_has_every_family_and_unique_ids():
    for fam in list(G.FAMILIES.values()) + [G.persistent_cases(256), G.split_cases()]:
        ids = [c.id for c in fam]
        assert len(fam) > 0 and len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)[:4]
    assert {c.epi for c in ALL} == set(G.EPIS)
    # both empty-split pairs, all five K-tile counts of the 256 x 256 kernels, the mixed launch
    assert {(c.K // 64, c.splitk) for c in G.FAMILIES['splitk']} >= set(G.SPLITS)
    assert {c.K // 64 for c in G.FAMILIES['tile256'] if (c.M, c.N) == (520, 520)} == {1, 2, 3, 4, 5}


def _int_epilogue(case, x):
    """The epilogue in int64, in halves when alpha = 0.5 (everything times two)."""
    two = 2 if case.alpha == 0.5 else 1
    L = lambda t: t.round().long()
    v = int(case.alpha * two) * (L(x['A']) @ L(x['B']).transpose(1, 2))
    if x['bias'] is not None:
        v = v + two * L(x['bias'])
    if case.mul:
        v = v * L(x['aux'])
    if case.acc:
        v = v + two * L(x['c0'])
    return v, two


SMALL = [c for c in EXACT_CASES if c.M * c.N * c.K * c.nbatch <= 136 * 264 * 192 * 6]
ONE_PER_EPI = [next(c for c in EXACT_CASES if c.epi == e and (c.M, c.N) == (520, 520)) for e in G.EPI_LIST]


@pytest.mark.parametrize('case', SMALL[::3] + ONE_PER_EPI, ids=lambda c: c.id)
def test_float64_reference_equals_int64(case):
    x = G.make_inputs(case)
    for k, (lo, hi) in dict(A=(-2, 2), B=(-2, 2), bias=(-8, 8), aux=(-2, 2), c0=(-64, 64)).items():
        if x[k] is not None:
            assert torch.equal(x[k], x[k].round()) and lo <= float(x[k].min()) and float(x[k].max()) <= hi
            assert float(x[k].min()) == lo and float(x[k].max()) == hi or x[k].numel() < 64      # the whole range is drawn
    ref = G.reference(case, x)
    want, two = _int_epilogue(case, x)
    assert torch.equal(ref['C'] * two, want.double())
    assert torch.equal(G.store(ref['C'], torch.float32).double(), ref['C'])                    # float32 holds it exactly
    if case.c_dtype == torch.bfloat16:
        assert float((G.store(ref['C'], case.c_dtype).double() - ref['C']).abs().max()) <= 2.0 ** -8 * float(ref['C'].abs().max())
    # row chunks of the reference are the rows of the whole
    r0 = case.M // 3
    assert torch.equal(G.reference(case, x, r0, case.M)['C'], ref['C'][:, r0:])


def test_caps_hold_for_every_case_of_the_table():
    checked = 0
    for case in EXACT_CASES:
        if case.colsum or case.rowdot:
            x = G.make_inputs(case)
            stored = G.store(G.reference(case, x)['C'], case.c_dtype)
            G.assert_caps(case, stored)
            checked += 1
        else:
            G.assert_caps(case)
    assert checked >= 20
    with pytest.raises(AssertionError):                                        # and the check can fail: K beyond what float32 holds
        G.assert_caps(G.Case(256, 256, 64 * 70000))


def test_place_puts_the_operand_where_the_kernels_read_it():
    case = G.Case(5, 8, 16, nb1=2, nb2=3)
    A = G.make_inputs(case)['A']
    for kc in (True, False):
        buf, ld, stride = G.place(A, kc, 8, 16, torch.bfloat16)
        assert ld == (16 if kc else 5) + 8 and stride == (5 if kc else 16) * ld
        for z, m, k in ((0, 0, 0), (5, 4, 15), (3, 2, 7)):
            assert float(buf[16 + z * stride + (m * ld + k if kc else k * ld + m)]) == float(A[z, m, k])
        assert int(torch.isnan(buf).sum()) == buf.numel() - A.numel()             # front, pad columns and tail are NaN


def test_the_split_models_say_what_pb_gemm2_try_documents():
    assert G.tail_split_factor(26624, 768, 3072, 256) >= 2 and G.tail_split_factor(26624, 768, 2304, 256) >= 2
    assert G.tail_split_factor(26624, 768, 768, 256) == 1                      # "K = 768 loses"
    assert G.tail_split_factor(32768, 768, 3072, 256) == 1                     # "and so does a half-full round"
    assert G.tail_split_factor(256 * 256, 256, 3072, 256) == 1                 # whole rounds: nothing to split
    assert G.row_split_rows(26624, 768, 768, 256) == 85 * 256
    assert G.row_split_rows(26620, 768, 768, 256) == 26620                     # M no multiple of 8
    assert G.persistent_rows(256) == (33024, 66048 - 248)


# ---------------------------------------------------------------- the helpers reject a wrong answer
def _stored(case):
    x = G.make_inputs(case)
    return x, G.store(G.reference(case, x)['C'], case.c_dtype)


def _ulp_off(t, idx):
    bits = t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)
    bits[idx] += 1
    return t


@pytest.mark.parametrize('epi', ['store', 'acc32'])
def test_one_element_one_ulp_off_fails(epi):
    case = G.Case(264, 264, 128, epi=epi)
    _, ref = _stored(case)
    G.assert_equal(ref.clone(), ref, 'C')
    for idx in ((0, 0, 0), (0, 263, 263), (0, 100, 7)):
        with pytest.raises(AssertionError, match='1 of'):
            G.assert_equal(_ulp_off(ref.clone(), idx), ref, 'C')
    bad = ref.clone(); bad[0, 5, 5] = float('nan')
    with pytest.raises(AssertionError):
        G.assert_equal(bad, ref, 'C')


def test_two_rows_exchanged_fail():
    case = G.Case(264, 264, 128)
    _, ref = _stored(case)
    bad = ref.clone()
    bad[0, [255, 256]] = ref[0, [256, 255]]
    with pytest.raises(AssertionError):
        G.assert_equal(bad, ref, 'C')
    case = G.Case(512, 256, 128, epi='rowdot')                                 # ... and in the row dots, which are stored transposed
    x, ref = _stored(case)
    rd = G.rowdot_reference(case, ref, x['aux'])
    bad = rd.clone(); bad[:, [0, 1]] = rd[:, [1, 0]]
    with pytest.raises(AssertionError):
        G.assert_equal(bad, rd, 'rowdot')


@pytest.mark.parametrize('K,kt', [(64, 0), (192, 2), (320, 3)])
def test_one_k_tile_missing_from_one_tile_fails(K, kt):
    case = G.Case(520, 520, K, epi='bias')
    x, ref = _stored(case)
    short = G.reference(case, x)['C'].clone()
    rows, cols, ks = slice(256, 512), slice(0, 256), slice(64 * kt, 64 * kt + 64)
    short[0, rows, cols] -= x['A'][0, rows, ks] @ x['B'][0, cols, ks].t()
    with pytest.raises(AssertionError):
        G.assert_equal(G.store(short, case.c_dtype), ref, 'C')
    # the column sums see it too
    cs = G.colsum_reference(case, ref)
    with pytest.raises(AssertionError):
        G.assert_equal(G.colsum_reference(case, G.store(short, case.c_dtype)), cs, 'colsum')


def test_one_slab_counted_twice_or_left_out_fails():
    case = G.Case(264, 136, 320, a_kc=False, b_kc=False, splitk=4, accum=True)
    x, ref = _stored(case)
    kc = -(-5 // 4) * 64
    slabs = [x['A'][0][:, s * kc:(s + 1) * kc] @ x['B'][0][:, s * kc:(s + 1) * kc].t() for s in range(4)]
    assert slabs[3].numel() == ref[0].numel() and float(slabs[3].abs().max()) == 0     # the empty split holds zeros
    G.assert_equal(G.store(sum(slabs) + x['c0'][0], case.c_dtype), ref[0], 'C')
    for s in range(3):
        with pytest.raises(AssertionError):
            G.assert_equal(G.store(sum(slabs) + slabs[s] + x['c0'][0], case.c_dtype), ref[0], 'C')
        with pytest.raises(AssertionError):
            G.assert_equal(G.store(sum(slabs) - slabs[s] + x['c0'][0], case.c_dtype), ref[0], 'C')
    nan_slab = torch.full_like(slabs[3], float('nan'))                           # a slab nobody wrote reaches C as NaN
    with pytest.raises(AssertionError):
        G.assert_equal(G.store(sum(slabs[:3]) + nan_slab + x['c0'][0], case.c_dtype), ref[0], 'C')


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
def test_a_sentinel_overwritten_fails(dtype):
    for where in ('front', 'back', 'pad column', 'last pad column', 'read-modify-write'):
        g = G.Guarded(6, 8, dtype, 'cpu', ld=12, pad=16, shift=1)
        assert g.start == 17 and g.view.shape == (6, 8) and bool(torch.isnan(g.view).all())
        g.assert_untouched('fresh')
        g.view.copy_(torch.ones(6, 8))
        g.assert_guards('written inside only')
        i = dict(front=g.start - 1, back=g.start + 6 * 12).get(where, g.start + (8 if where != 'last pad column' else 5 * 12 + 11))
        if where == 'read-modify-write':
            g.buf[i] += 1.0
        else:
            g.buf[i] = 0.0
        with pytest.raises(AssertionError, match='guard'):
            g.assert_guards(where)
    g = G.Guarded(4, 8, torch.float32, 'cpu', pad=8, guard=float('nan'))       # an all-NaN workspace: any store shows
    g.assert_untouched('slabs')
    g.buf[3] = 0.0
    with pytest.raises(AssertionError):
        g.assert_guards('slabs')
    g = G.Guarded(4, 8, torch.float32, 'cpu')
    g.view[2, 2] = 1.0
    with pytest.raises(AssertionError):
        g.assert_untouched('a refused call')


def test_kind3_figure_rejects_a_partial_sum_kept_in_bf16():
    case = G.Case(264, 264, 320, epi='real')
    x = G.make_inputs(case)
    ref = G.reference(case, x)
    f32, _ = G.float32_evaluation(case, x)
    fig32 = G.kind3_figure(f32, ref['C'], ref['abs'], False)
    assert 0 < fig32 < 2                                                       # a float32 sum of K terms stays within a few ulp of its magnitude
    assert G.kind3_figure(ref['C'], ref['C'], ref['abs'], False) == 0
    A, B = x['A'][0].float(), x['B'][0].float()
    low = (A[:, :256] @ B[:, :256].t()).to(torch.bfloat16).float() + A[:, 256:] @ B[:, 256:].t()
    assert G.kind3_figure(low[None], ref['C'], ref['abs'], False) > 100 * G.MARGIN * fig32
    # bf16 storage forgives one bf16 ulp of the result and nothing more
    stored = G.store(ref['C'], torch.bfloat16)
    assert G.kind3_figure(stored, ref['C'], ref['abs'], True) == 0
    off = _ulp_off(_ulp_off(stored.clone(), (0, 3, 3)), (0, 3, 3))
    assert G.kind3_figure(off, ref['C'], ref['abs'], True) > G.MARGIN * fig32
    # GELU: the float64 pair is the derivative pair
    v = torch.linspace(-6, 6, 4001, dtype=F64, requires_grad=True)
    y, dy = G.gelu64(v)
    assert torch.allclose(torch.autograd.grad(y.sum(), v)[0], dy.detach(), rtol=0, atol=1e-14)
    assert torch.allclose(y.detach(), torch.nn.functional.gelu(v.detach()), rtol=0, atol=1e-14)
