"""GPU: pb_distill_fwd_bwd (csrc/pb_distill.hip) alone, against the float64 form of tests/distill_ref.py (checked against float64 autograd
in tests/test_distill_cpu.py). The devices are those of tests/test_row_kernels_gpu.py, restated here:
  * every output sits inside a larger allocation whose guard elements hold a small finite sentinel and whose inside starts as NaN (integers:
    a sentinel): after the call the guards are untouched and the written region is finite;
  * `sums` goes in non-zero: it is accumulated into;
  * the student's logits have a float64 top-2 gap >= 0.01 in every head of every row, except planted exact ties (first / last class of a
    head, classes 63 / 64 / 128, classes 1 / 64: the lowest index wins); targets at class 0 (row 0) and n - 1 (last row); head 6 has no
    loss position, so coef = inf and dlogits is NaN exactly where inf * 0 is in the reference.
Planes 2 and 3 (mask count, correct count) and the argmax of EVERY row are exact. Planes 1, 4, 5 and dlogits: the kernel's error against
float64 is at most MARGIN = 4 times the error of the float32 evaluation of the same restatement at the same inputs. Sums are taken relative
to |start| + sum_t |term_t|; for the KL plane a row's |term| is m sum_c q_c (|log q_c| + |log p_tau,c|), what the KL is the difference of, so
that cancellation in a near-zero KL is not charged to the kernel. dlogits is taken in units of 2^-24 |coef m|, with 2^-8 |ref| of rounding
allowance for bf16 storage. No bound was taken from the kernel's own error; _bound prints both figures of every check (pytest -s).

Forms: every head <= 320 classes -> register-resident ('reg', 'default'); a head above -> the general form ('generic': 330, 'wide': 1088,
the largest legal head). Rows: T 1, 3, 4, 5 = idle waves, one full workgroup, a second; T = 8197 = five rows past one sweep of the
2048 x 4 grid, and the finalize kernel's 4-way unrolled loop.

Measured on an MI355X, worst kernel / float32-torch ratio over every case of this file (in brackets the largest kernel figure); the bound is 4:
  loss sums 2.99 at 'generic' T = 1 (0, 1, 0.1) (largest 1.7e-7 of sum |term|)     hard 2.53 at 'wide' T = 8197 (largest 1.4e-7, 'reg' T = 3)
  kl 3.04 at 'default' T = 5 (0.3, 0.5, 0.1) (largest 1.1e-7, the extremes case)
  dlogits f32 2.09 at 'wide' T = 3 (1, 1, 0) (largest 4.0 units, 'generic' T = 8197, where float32 torch has 3.7), bf16 0.08 (0.24 units)
At T <= 5 a column sums one to five rows and the float32 evaluation's own error is a matter of luck (2.4e-8 .. 1.7e-7), so the ratios there say
little about the kernel; they are what the rule asks for. Two earlier forms of the soft part missed the bound: `__expf` with reciprocal products
(dlogits 4.24 at 'default' T = 1 (1, 1, 0)) and float32 KL sums (kl 6.16 at 'generic' T = 4 (0, 1, 0)); the kernel now uses a one-ulp
exponential, corrected quotients and float64 for the KL's three sums.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import distill_ref as DR

pytestmark = pytest.mark.gpu

E24, E8 = 2.0 ** -24, 2.0 ** -8
MARGIN = 4.0
F32, BF16 = torch.float32, torch.bfloat16
SENT = -31111
GUARD = 1.5 * 2.0 ** -20
LAYOUTS = {'reg': [70, 7, 8, 64, 65, 129, 9, 12],           # every head <= 320 classes: the register-resident form
           'generic': [330, 7, 8, 64, 65, 129, 9, 12],      # one head of 330 classes: the general form for the whole row
           'default': [262, 134, 135, 262, 134, 38, 260, 55],
           'wide': [1088, 7, 8, 64, 65, 129, 9, 12]}        # the largest legal head: 17 classes per lane
PARAMS = [(0.0, 1.0, 0.0), (1.0, 1.0, 0.0), (0.5, 2.0, 0.0), (0.3, 0.5, 0.1), (0.0, 1.0, 0.1)]      # (alpha, tau, eps)
SUMS0 = [0.5] * 8 + [3.0] * 8 + [2.0] * 8 + [0.25] * 8 + [0.125] * 8    # `sums` going in: it is accumulated into


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from pianobart_amd import ops as o
    return o


# ---------------------------------------------------------------- helpers
def _gen(seed):
    return torch.Generator(device='cuda').manual_seed(seed)


def _D(t):
    return t.double()


def _galloc(shape, dtype, pad=8, init=None):
    """(buffer, view, pad): a view of `shape` inside a flat buffer with `pad` guard elements on both sides. The guards hold GUARD, a small
    finite value (exact in bf16): a stray store changes it, and so does a stray read-modify-write. The view starts as NaN (integers: SENT)
    unless `init` is given."""
    n = int(np.prod(shape))
    fl = dtype.is_floating_point
    buf = torch.full((n + 2 * pad,), GUARD if fl else SENT, dtype=dtype, device='cuda')
    view = buf[pad:pad + n].view(shape)
    if init is not None:
        view.copy_(torch.as_tensor(init, dtype=dtype, device='cuda').expand(shape))
    elif fl:
        view.fill_(float('nan'))
    return buf, view, pad


def _gcheck(g, what, finite=None):
    buf, view, pad = g
    n = view.numel()
    torch.cuda.synchronize()
    guards = torch.cat([buf[:pad], buf[pad + n:]])
    assert bool((guards == (GUARD if buf.dtype.is_floating_point else SENT)).all()), '%s: guard elements written' % what
    if view.dtype.is_floating_point:
        assert bool(torch.isfinite(view if finite is None else finite).all()), '%s: not finite' % what
    else:
        assert bool((view != SENT).all()), '%s: not written' % what


def _row_err(got, ref, scale, bf16):
    """max over elements of (|got - ref| [- 2^-8 |ref|]) / (2^-24 scale)."""
    err = (got.double() - ref).abs()
    if bf16:
        err = (err - E8 * ref.abs()).clamp_min(0)
    if err.numel() == 0:
        return 0.0
    return float((err / (E24 * scale).clamp_min(1e-300)).max())


def _col_err(got, start, terms, mags=None):
    """max over columns of |got - (start + sum_t term_t)| / (|start| + sum_t |term_t|); mags: the |term_t| to use instead."""
    ref = start + terms.sum(0)
    den = (abs(start) + (terms.abs() if mags is None else mags).sum(0)).clamp_min(1e-300)
    return float(((got.double() - ref).abs() / den).max())


def _bound(what, kernel, f32):
    ratio = kernel / f32 if f32 > 0 else (0.0 if kernel == 0 else float('inf'))
    print('RATIO %-52s kernel %10.4g   float32 torch %10.4g   ratio %6.3f' % (what, kernel, f32, ratio))
    assert kernel <= MARGIN * f32, '%s: kernel %.4g > %g x float32 torch %.4g' % (what, kernel, MARGIN, f32)


def _inputs(sizes, T, seed=0, extreme=False):
    """Student and teacher logits, targets, loss mask; the planted ties of the student as {(row, head): winning class}."""
    off = [0] + [int(v) for v in np.cumsum(sizes)]
    g = _gen(T + len(sizes) + sizes[0] + seed)
    z = 2 * torch.randn(T, off[8], device='cuda', generator=g)
    u = 2 * torch.randn(T, off[8], device='cuda', generator=g)
    if extreme:                                                         # +-80 in both rows: the quotients by tau = 0.5 reach +-160
        for t in (z, u):
            hit = torch.rand(T, off[8], device='cuda', generator=g) < 0.05
            sign = torch.where(torch.rand(T, off[8], device='cuda', generator=g) < 0.5, -1.0, 1.0)
            t.copy_(torch.where(hit, 80.0 * sign, t))
            t[:, ::37] = -80.0
            t[0, off[3]] = 80.0
    for i in range(8):
        seg = z[:, off[i]:off[i + 1]]
        seg.scatter_add_(1, seg.argmax(-1, keepdim=True), torch.full((T, 1), 0.01, device='cuda'))
    target = torch.stack([torch.randint(0, n, (T,), device='cuda', generator=g) for n in sizes], dim=1)
    target[0] = 0
    target[T - 1] = torch.tensor(sizes, device='cuda') - 1
    ties = {}
    if T >= 3:
        h = [i for i in range(1, 8) if sizes[i] >= 129][0]             # a head with classes 63, 64 and 128
        top = 90.0 if extreme else 50.0
        z[1, 0] = z[1, sizes[0] - 1] = top
        z[2, off[h] + 63] = z[2, off[h] + 64] = z[2, off[h] + 128] = top
        z[2, off[0] + 1] = z[2, off[0] + 64] = top                      # lane 1's first class against lane 0's second
        ties = {(1, 0): 0, (2, h): 63, (2, 0): 1}
    m = (torch.rand(T, 8, device='cuda', generator=g) < 0.6).float()
    m[0] = 1
    m[:, 6] = 0
    return off, z, u, target, m.contiguous(), ties


def _coef(ops, m):
    ws = torch.empty(int(ops.LIB.query('pb_ce_partials_floats')), device='cuda')
    counts, coef = torch.empty(8, device='cuda'), torch.empty(8, device='cuda')
    ops.mask_count(m, counts, ws)
    ops.loss_coef(counts, torch.tensor([3.0, 1, 4, 1, 5, 9, 2, 6], device='cuda'), coef)
    torch.cuda.synchronize()
    assert torch.isinf(coef[6]) and coef[6] > 0
    return coef


def _ws(ops):
    return torch.empty(int(ops.LIB.query('pb_distill_partials_floats')), device='cuda')


def _check(ops, tag, dt, inp, coef, par, with_dl=True, with_am=True, teacher=True, lay=None):
    """One call inside guarded outputs, held to the float64 reference. Returns the outputs."""
    off, z, u, target, m, ties = inp
    alpha, tau, eps = par
    T, V = z.shape
    sizes = [off[i + 1] - off[i] for i in range(8)]
    tag = '%s %s (%g, %g, %g)' % (tag, {F32: 'f32', BF16: 'bf16', None: 'no-dl'}[dt if with_dl else None], alpha, tau, eps)
    sums = _galloc((40,), F32, 8, SUMS0)
    dl = _galloc((T, V), dt, max(8, 2 * V)) if with_dl else None
    am = _galloc((T, 8), torch.int16, 16) if with_am else None
    tch = u if teacher else None
    ops.distill_fwd_bwd(z, tch, None, target.to(torch.int16), m, sums[1], _ws(ops), coef, dl[1] if with_dl else None, am[1] if with_am else None,
                        alpha, tau, eps, layout=lay)
    _gcheck(sums, tag + ': sums')
    r64 = DR.distill_fwd_bwd(_D(z), _D(tch) if teacher else None, target, _D(m), off, _D(coef), alpha, tau, eps)
    r32 = DR.distill_fwd_bwd(z, tch, target, m, off, coef, alpha, tau, eps)
    for (row, head), want in ties.items():
        assert int(r64['argmax'][row, head]) == want
    if with_am:
        _gcheck(am, tag + ': argmax')
        assert torch.equal(am[1].long(), r64['argmax']), tag + ': argmax (every row; ties: the lowest index)'
    s0 = torch.tensor(SUMS0, device='cuda', dtype=torch.float64).reshape(5, 8)
    got = sums[1].reshape(5, 8)
    assert torch.equal(got[1:3].double(), s0[1:3] + r64['terms'][1:3].sum(1)), tag + ': mask / correct counts are not exact'
    f32sum = lambda p: s0[p].float() + r32['terms'][p].sum(0)
    _bound(tag + ' loss', _col_err(got[0], s0[0], r64['terms'][0]), _col_err(f32sum(0), s0[0], r64['terms'][0]))
    _bound(tag + ' hard', _col_err(got[3], s0[3], r64['terms'][3]), _col_err(f32sum(3), s0[3], r64['terms'][3]))
    if teacher:
        _bound(tag + ' kl', _col_err(got[4], s0[4], r64['terms'][4], r64['kl_abs']), _col_err(f32sum(4), s0[4], r64['terms'][4], r64['kl_abs']))
    else:
        assert torch.equal(got[4].double(), s0[4]), tag + ': KL plane without a teacher'
    if with_dl:
        live = [i for i in range(8) if i != 6]
        _gcheck(dl, tag + ': dlogits', finite=torch.cat([dl[1][:, :off[6]], dl[1][:, off[7]:]], 1))
        nan_ref = torch.isnan(r64['dlogits'])
        assert torch.equal(torch.isnan(dl[1]), nan_ref) and bool(nan_ref[:, off[6]:off[7]].all()) and int(nan_ref.sum()) == T * sizes[6]
        sc = torch.cat([r64['gscale'][:, i:i + 1].expand(T, sizes[i]) for i in range(8)], 1)
        cols = torch.tensor([c for i in live for c in range(off[i], off[i + 1])], device='cuda')
        on = sc[:, cols] > 0
        assert bool((dl[1][:, cols][~on] == 0).all()), tag + ': dlogits of a position without loss'
        pick = lambda t: t[:, cols][on]
        _bound(tag + ' dlogits', _row_err(pick(dl[1]), pick(r64['dlogits']), pick(sc), dt == BF16),
               _row_err(pick(r32['dlogits']), pick(r64['dlogits']), pick(sc), False))
    return dict(sums=sums[1], dl=dl[1] if with_dl else None, am=am[1] if with_am else None)


def _sweep_rows(T, per_sweep):
    rows = {0, T - 1}
    for k in range(per_sweep, T, per_sweep):
        rows.update(r for r in (k - 1, k, k + 1) if r < T)
    return sorted(rows)


def _same_bytes(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ---------------------------------------------------------------- against float64
@pytest.mark.parametrize('dt', [F32, BF16])
@pytest.mark.parametrize('kind', ['reg', 'generic', 'default', 'wide'])
@pytest.mark.parametrize('T', [1, 3, 4, 5, 8197])
def test_distill_row_loop(ops, dt, kind, T):
    """Every (alpha, tau, eps) of PARAMS on one set of inputs per (layout, T): pure CE, pure KL, the usual mixture, a temperature below 1
    with smoothing, smoothing alone. See the module docstring for what is exact and what is bounded."""
    lay = ops.Layout(LAYOUTS[kind])
    inp = _inputs(LAYOUTS[kind], T)
    coef = _coef(ops, inp[4])
    for par in PARAMS:
        _check(ops, 'distill %s T=%d' % (kind, T), dt, inp, coef, par, lay=lay)


@pytest.mark.parametrize('dt', [F32, BF16])
@pytest.mark.parametrize('kind', ['reg', 'generic'])
def test_distill_extremes(ops, dt, kind):
    """Student and teacher rows carry +-80 (and a planted 90 / 90 tie) at tau = 0.5: the quotients reach +-160 and more, every softmax
    subtracts its own maximum, so everything stays finite and inside the same bounds."""
    lay = ops.Layout(LAYOUTS[kind])
    inp = _inputs(LAYOUTS[kind], 67, extreme=True)
    assert float(inp[1].abs().max()) >= 80 and float(inp[2].abs().max()) >= 80
    out = _check(ops, 'distill extreme %s' % kind, dt, inp, _coef(ops, inp[4]), (0.3, 0.5, 0.1), lay=lay)
    assert bool(torch.isfinite(out['sums']).all())


@pytest.mark.parametrize('kind', ['reg', 'generic'])
def test_distill_without_teacher(ops, kind):
    """alpha = 0 with teacher = NULL: the KL plane is not touched, and every other output equals the call with a teacher bit for bit."""
    lay = ops.Layout(LAYOUTS[kind])
    inp = _inputs(LAYOUTS[kind], 133)
    coef = _coef(ops, inp[4])
    for par in ((0.0, 1.0, 0.0), (0.0, 1.0, 0.1)):
        a = _check(ops, 'distill no teacher %s' % kind, F32, inp, coef, par, teacher=False, lay=lay)
        b = _check(ops, 'distill %s' % kind, F32, inp, coef, par, lay=lay)
        assert torch.equal(a['am'], b['am']) and torch.equal(a['sums'][:32], b['sums'][:32])
        assert torch.equal(torch.nan_to_num(a['dl'], nan=7.0), torch.nan_to_num(b['dl'], nan=7.0))


# ---------------------------------------------------------------- bit-for-bit properties
def _call(ops, inp, coef, par, lay, dt=F32, teacher=None, t_row=None, dl=True, am=True, sums0=0.0, rows=None):
    off, z, u, target, m, _ = inp
    if rows is not None:
        z, u, target, m = z[rows].contiguous(), u[rows].contiguous(), target[rows].contiguous(), m[rows].contiguous()
    T, V = z.shape
    sums = torch.full((40,), sums0, device='cuda')
    d = torch.full((T, V), float('nan'), device='cuda', dtype=dt) if dl else None
    a = torch.full((T, 8), SENT, device='cuda', dtype=torch.int16) if am else None
    ops.distill_fwd_bwd(z, u if teacher is None else teacher, t_row, target.to(torch.int16), m, sums, _ws(ops), coef, d, a, *par, layout=lay)
    torch.cuda.synchronize()
    return sums, d, a


@pytest.mark.parametrize('kind', ['reg', 'generic'])
def test_distill_teacher_row_map(ops, kind):
    """The teacher has 2 T rows and t_row is a permutation into them; the rows nobody references are NaN. The result equals the call on
    the gathered teacher rows bit for bit, and is finite (head 6's NaN gradient columns aside)."""
    lay = ops.Layout(LAYOUTS[kind])
    inp = _inputs(LAYOUTS[kind], 261)
    off, z, u = inp[0], inp[1], inp[2]
    T = z.shape[0]
    coef = _coef(ops, inp[4])
    rows = torch.randperm(2 * T, device='cuda', generator=_gen(5))[:T]
    big = torch.full((2 * T, off[8]), float('nan'), device='cuda')
    big[rows] = u
    par = (0.5, 2.0, 0.0)
    s1, d1, a1 = _call(ops, inp, coef, par, lay, teacher=big, t_row=rows.to(torch.int32))
    s2, d2, a2 = _call(ops, inp, coef, par, lay)
    assert _same_bytes(s1, s2) and _same_bytes(d1, d2) and torch.equal(a1, a2)
    assert bool(torch.isfinite(s1).all()) and bool(torch.isfinite(torch.cat([d1[:, :off[6]], d1[:, off[7]:]], 1)).all())
    assert float(s1[32:40].abs().sum()) > 0


@pytest.mark.parametrize('dt', [F32, BF16])
@pytest.mark.parametrize('kind', ['reg', 'generic', 'default', 'wide'])
def test_distill_teacher_equals_student(ops, dt, kind):
    """Teacher == student: the KL plane is exactly 0 at every temperature and the soft gradient vanishes; at alpha = 0, eps = 0 plane 1
    equals plane 4 bit for bit."""
    lay = ops.Layout(LAYOUTS[kind])
    inp = _inputs(LAYOUTS[kind], 517)
    off, z = inp[0], inp[1]
    coef = _coef(ops, inp[4])
    for tau in (1.0, 2.0, 0.5):
        s, d, _ = _call(ops, inp, coef, (1.0, tau, 0.0), lay, dt=dt, teacher=z.clone())
        assert bool((s[32:40] == 0).all()) and bool((s[0:8] == 0).all())
        assert bool((torch.cat([d[:, :off[6]], d[:, off[7]:]], 1) == 0).all())
    s, _, _ = _call(ops, inp, coef, (0.0, 1.0, 0.0), lay, dt=dt, teacher=z.clone())
    assert _same_bytes(s[0:8], s[24:32]) and float(s[0:8].abs().sum()) > 0
    s, _, _ = _call(ops, inp, coef, (0.0, 1.0, 0.0), lay, dt=dt)              # another teacher: the hard part does not see it
    assert _same_bytes(s[0:8], s[24:32])


@pytest.mark.parametrize('dt', [F32, BF16])
@pytest.mark.parametrize('kind', ['reg', 'generic'])
def test_distill_rows_are_independent(ops, dt, kind):
    """T = 8197: dlogits and argmax of rows 0, 8191, 8192, 8193, 8196 bit-equal to a 5-row call (NaN columns of the empty head excluded)."""
    lay = ops.Layout(LAYOUTS[kind])
    inp = _inputs(LAYOUTS[kind], 8197, seed=1)
    off = inp[0]
    coef = _coef(ops, inp[4])
    rows = _sweep_rows(8197, 8192)
    assert rows == [0, 8191, 8192, 8193, 8196]
    idx = torch.tensor(rows, device='cuda')
    par = (0.3, 0.5, 0.1)
    _, d, a = _call(ops, inp, coef, par, lay, dt=dt)
    _, d5, a5 = _call(ops, inp, coef, par, lay, dt=dt, rows=idx)
    keep = torch.tensor([c for i in range(8) if i != 6 for c in range(off[i], off[i + 1])], device='cuda')
    assert torch.equal(a5, a[idx]) and _same_bytes(d5[:, keep], d[idx][:, keep])


@pytest.mark.parametrize('kind', ['reg', 'generic'])
def test_distill_optional_outputs_and_repeatability(ops, kind):
    """dlogits = NULL, argmax_out = NULL, and both: the sums and the remaining output do not change by a bit. Two identical calls give
    identical bytes (per-workgroup partials summed in a fixed order; no atomics)."""
    lay = ops.Layout(LAYOUTS[kind])
    inp = _inputs(LAYOUTS[kind], 8197, seed=2)
    coef = _coef(ops, inp[4])
    par = (0.5, 2.0, 0.1)
    s, d, a = _call(ops, inp, coef, par, lay, sums0=0.75)
    s2, d2, a2 = _call(ops, inp, coef, par, lay, sums0=0.75)
    assert _same_bytes(s, s2) and _same_bytes(d, d2) and _same_bytes(a, a2)
    sa, _, aa = _call(ops, inp, coef, par, lay, dl=False, sums0=0.75)
    sb, db, _ = _call(ops, inp, coef, par, lay, am=False, sums0=0.75)
    sc, _, _ = _call(ops, inp, coef, par, lay, dl=False, am=False, sums0=0.75)
    assert _same_bytes(sa, s) and _same_bytes(sb, s) and _same_bytes(sc, s) and _same_bytes(aa, a) and _same_bytes(db, d)


# ---------------------------------------------------------------- refusals
def test_distill_refusals(ops):
    """Every refusal names its argument, and a refused call writes nothing."""
    from pianobart_amd._lib import PBError
    lay = ops.Layout(LAYOUTS['reg'])
    off, z, u, target, m, _ = _inputs(LAYOUTS['reg'], 9)
    coef = _coef(ops, m)
    t16 = target.to(torch.int16)
    sums, dl, am = _galloc((40,), F32, 8, SUMS0), _galloc(tuple(z.shape), F32, 64), _galloc((9, 8), torch.int16, 16)
    ws = _ws(ops)

    def call(alpha=0.5, tau=2.0, eps=0.0, teacher=u, coef=coef, dlogits=dl[1]):
        ops.distill_fwd_bwd(z, teacher, None, t16, m, sums[1], ws, coef, dlogits, am[1], alpha, tau, eps, layout=lay)

    for kw, word in ((dict(alpha=-0.1), 'alpha'), (dict(alpha=1.5), 'alpha'), (dict(alpha=float('nan')), 'alpha'),
                     (dict(eps=-0.01), 'eps'), (dict(eps=1.0), 'eps'),
                     (dict(tau=0.0), 'tau'), (dict(tau=-1.0), 'tau'), (dict(tau=float('inf')), 'tau'), (dict(tau=float('nan')), 'tau'),
                     (dict(teacher=None), 'teacher'), (dict(coef=None), 'dlogits needs coef')):
        with pytest.raises(PBError, match='pb_distill_fwd_bwd: .*' + word):
            call(**kw)
    short = u[:5].contiguous()                                           # fewer teacher rows than student rows and no row map
    with pytest.raises(PBError, match='pb_distill_fwd_bwd: .*T_t'):
        call(teacher=short)
    bad = (ctypes.c_int32 * 9)(*(list(off[:8]) + [off[8] - 1]))          # offsets that stop one column short of V
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    with pytest.raises(PBError, match='pb_distill_fwd_bwd: segment offsets'):
        ops.LIB.call('pb_distill_fwd_bwd', p(z), p(u), None, p(t16), p(m), bad, p(sums[1]), p(ws), p(coef), p(dl[1]), p(am[1]), 9, 9, off[8], ops.PB_F32,
                     0.5, 2.0, 0.0, None)
    torch.cuda.synchronize()
    assert torch.equal(sums[1], torch.tensor(SUMS0, device='cuda')) and bool(torch.isnan(dl[1]).all()) and bool((am[1] == SENT).all())
    call()                                                               # and the same buffers are accepted by a legal call
    _gcheck(sums, 'sums')
    _gcheck(am, 'argmax')

