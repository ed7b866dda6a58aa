"""GPU: the row kernels (csrc/pb_norm.hip, pb_softmax.hip, pb_loss.hip, pb_optim.hip) at every row width and on both sides of every
row-loop edge, against the float64 references of tests/row_ref.py (checked against float64 autograd in tests/test_row_ref_cpu.py).

Three kinds of assertion, the first two without a tolerance:
  1. row independence, bit for bit: a call at a T that needs several sweeps of the grid-stride loop, and the same rows again in a
     small call (one sweep: the region the float64 cases cover); torch.equal on the first and last row of every sweep;
  2. exact sums: small-integer cotangents and masks make dbeta, the column sums, the mask counts and the correct counts integers that
     float32 holds exactly, so they must EQUAL the float64 sum: a dropped, doubled or misattributed row cannot pass;
  3. float64 with a per-element bound, for everything else. The inputs are rounded to the storage dtype first and the reference runs
     on the rounded values. Per-row outputs: |got - ref| <= k 2^-24 scale_row (+ 2^-8 |ref| for bf16 storage: one bf16 ulp), scale_row
     the row's natural magnitude. Sums over T rows: |got - ref| / sum_t |term_t|. In both, the figure the kernel may reach is FOUR
     times the figure of a plain float32 torch evaluation of the same formula (row_ref with float32 tensors) at the same shape and
     inputs: the factor covers the other summation order (per-wave chains, then a fixed tree). No bound here was taken from a kernel's
     own error. _bound() prints both figures of every check (pytest -s).
Every output sits inside a larger allocation whose guard elements on both sides (two rows for a (T, d) output) hold a small finite
sentinel and whose inside starts as NaN: after the call the guards must be untouched and the written region finite.

Branches (LN_WAVES = 8 rows per workgroup; forward grids <= 2048 workgroups, backward grids <= 512):
  NIT instance      d 4, 200, 256 -> 1; 260, 512 -> 2; 772 -> 4 (ceil(193 / 64)); 1024 -> 4; 1028, 1280, 2044, 2048 -> 8; d 64 -> 1
                    (NIT = 3 is d 516 .. 768: the d = 768 cases of tests/test_kernels_gpu.py, and d = 520 here)
  partial sweep     d 4, 200, 260, 520, 772, 1028, 1280, 2044 leave the last 64-lane sweep partly filled (1028 .. 2044: whole sweeps idle)
  second grid sweep backward T 4099, 8200 (4096 rows per sweep), forward T 16391 / 16400 (16384), softmax 16446 rows (16384),
                    cross-entropy T 8197 (8192), mask count T 4099 (4096), optimizer n 2 100 227 (2 097 152), batch_sum 2 098 180
  finalize_block    T <= 3072 (<= 384 partial rows): the plain loop; T 3073, 4096, 4099, 8200: the 4-way unrolled branch, then the plain
                    loop for the rest. pb_colsum has at most 128 partial rows: the plain loop only, at every T.
  scalar finalize   parameter-gradient outputs shifted by one float (finalize_partials_kernel<1>)
  scalar tail       optimizer n 1, 3, 5, 1027, 2 100 227 (n & 3 != 0)

Measured on an MI355X, worst kernel / float32-torch ratio over every case of a family (in brackets the largest kernel figure: per-row
outputs in units of 2^-24 scale_row, sums as a fraction of sum |term|); the bound is 4:
  add_ln    y 1.17 (4.1)  mean 1.21 (1.1)  rstd 1.55 (2.9)  dres 1.31 (3.3)  da 1.02 (3.4)  dgamma 1.48 (1.8e-7)  dbias_a 1.67 (1.2e-7)
  embed_ln  y 1.48 (4.6)  mean 1.43 (1.7)  rstd 1.01 (4.9)  dz 1.06 (6.1)  dP 1.06 .. 1.20 by run: atomics (6.1)  dpos 2.02 (3.5)  dgamma 1.68 (7.7e-8)
            dbias 1.74 (1.6e-7)  dbeta with dropout 1.63 (2.7e-8)
  softmax   P 1.50 (1.9)  dS 1.62 (0.63)        cross-entropy  loss sums 1.85 (1.15e-7)  dlogits 1.23 (4.0)
  optimizer sqnorm 1.00 (2.6e-8)  AdamW p 1.08 (4.1)  m 1.22 (1.7)  v 1.91 (3.8)
With bf16 storage the per-row figures of y, dres, da, dz, P, dS and dlogits are at most 0.42: the error stays inside the bf16 ulp.
"""
import numpy as np
import pytest
import torch

from tests import row_ref as R

pytestmark = pytest.mark.gpu

E24, E8 = 2.0 ** -24, 2.0 ** -8
MARGIN = 4.0
SEED, SITE = 0x1234567A5, 7
F32, BF16 = torch.float32, torch.bfloat16
WIDTHS = [4, 200, 256, 260, 512, 520, 772, 1024, 1028, 1280, 2044, 2048]
SENT = -31111
GUARD = 1.5 * 2.0 ** -20


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
    finite value (exact in bf16): a stray store changes it, and so does a stray read-modify-write (NaN guards would survive `+=`). The
    view starts as NaN (integers: SENT everywhere) unless `init` is given."""
    n = int(np.prod(shape))
    fl = dtype.is_floating_point
    buf = torch.full((n + 2 * pad,), GUARD if fl else SENT, dtype=dtype, device='cuda')
    view = buf[pad:pad + n].view(shape)
    if init is not None:
        view.copy_(torch.as_tensor(init, dtype=dtype, device='cuda').expand(shape))
    elif fl:
        view.fill_(float('nan'))
    return buf, view, pad


def _rows(T, d, dtype, init=None):
    return _galloc((T, d), dtype, max(8, 2 * d), init)


def _untouched(t):
    return torch.isnan(t) if t.dtype.is_floating_point else t == SENT


def _gcheck(g, what, written=True, finite=None):
    """guards untouched; the region between them (or the part `finite` of it) finite, or untouched as well (written=False: a refused or
    empty call)."""
    buf, view, pad = g
    n = view.numel()
    torch.cuda.synchronize()
    guards = torch.cat([buf[:pad], buf[pad + n:]])
    assert bool((guards == (GUARD if buf.dtype.is_floating_point else SENT)).all()), '%s: guard elements written' % what
    if not written:
        assert bool(_untouched(view).all()), '%s: written by a call that must not write' % what
    elif view.dtype.is_floating_point:
        assert bool(torch.isfinite(view if finite is None else finite).all()), '%s: not finite' % what


def _row_err(got, ref, scale, bf16):
    """max over elements of (|got - ref| [- 2^-8 |ref|]) / (2^-24 scale_row); scale broadcasts against ref."""
    err = (got.double() - ref).abs()
    if bf16:
        err = (err - E8 * ref.abs()).clamp_min(0)
    if err.numel() == 0:
        return 0.0
    return float((err / (E24 * scale).clamp_min(1e-300)).max())


def _col_err(got, start, terms):
    """max over columns of |got - (start + sum_t term_t)| / (|start| + sum_t |term_t|)."""
    ref = start + terms.sum(0)
    den = (abs(start) + terms.abs().sum(0)).clamp_min(1e-300)
    return float(((got.double() - ref).abs() / den).max())


def _bound(what, kernel, f32):
    print('RATIO %-44s kernel %10.4g   float32 torch %10.4g   ratio %6.3f' % (what, kernel, f32, kernel / f32 if f32 > 0 else (0.0 if kernel == 0 else float('inf'))))
    assert kernel <= MARGIN * f32, '%s: kernel %.4g > %g x float32 torch %.4g' % (what, kernel, MARGIN, f32)


def _partials(ops, d):
    return torch.empty(int(ops.LIB.query('pb_ln_partials_floats', max(d, 4))), device='cuda')


def _sweep_rows(T, per_sweep):
    """first row, last row, and the last / first / second row around every sweep boundary."""
    rows = {0, T - 1}
    for k in range(per_sweep, T, per_sweep):
        rows.update(r for r in (k - 1, k, k + 1) if r < T)
    return sorted(rows)


# ---------------------------------------------------------------- y = LN(res + drop(a)) and its backward
START = (0.25, 5.0, -0.5)          # dgamma, dbeta, dbias_a going in: the calls accumulate


def _ln_inputs(dt, T, d, seed=0):
    g = _gen(1000 * d + T + seed)
    x = dict(res=(torch.randn(T, d, device='cuda', generator=g) + 1.5).to(dt), a=torch.randn(T, d, device='cuda', generator=g).to(dt),
             w=1 + 0.2 * torch.randn(d, device='cuda', generator=g), b=0.2 * torch.randn(d, device='cuda', generator=g),
             dy=torch.randint(-3, 4, (T, d), device='cuda', generator=g).to(dt),
             dres0=torch.randint(-8, 9, (T, d), device='cuda', generator=g).float() / 4)
    return x


def _ln_run(ops, dt, x, p, row_ids=None, accum=False, dres_f32=False, da_none=False, shift=0, bwd=True):
    T, d = x['res'].shape
    o = dict(y=_rows(T, d, dt), mean=_galloc((T,), F32), rstd=_galloc((T,), F32))
    ops.add_ln_fwd(x['res'], x['a'], x['w'], x['b'], o['y'][1], o['mean'][1], o['rstd'][1], 1e-5, SEED, SITE, p, row_ids=row_ids)
    if bwd:
        ddt = F32 if dres_f32 else dt
        o['dres'] = _rows(T, d, ddt, x['dres0'].to(ddt) if accum else None)
        o['da'] = None if da_none else _rows(T, d, dt)
        for k, name in enumerate(('dgamma', 'dbeta', 'dbias')):
            o[name] = _galloc((d,), F32, 8 + shift, START[k])
        ops.add_ln_bwd(x['dy'], x['res'], x['a'], x['w'], o['mean'][1], o['rstd'][1], o['dres'][1], None if da_none else o['da'][1],
                       o['dgamma'][1], o['dbeta'][1], o['dbias'][1], _partials(ops, d), accum, SEED, SITE, p, row_ids=row_ids)
    for name, g in o.items():
        if g is not None:
            _gcheck(g, name)
    return o


def _ln_check(dt, x, o, mask, tag, accum=False, dres_f32=False, da_none=False, bwd=True):
    bf = dt == BF16
    f = lambda t: t.float()
    res, a, w, b, dy = (x[k] for k in ('res', 'a', 'w', 'b', 'dy'))
    y64, mean64, rstd64 = R.add_ln_fwd(_D(res), _D(a), _D(mask), _D(w), _D(b), 1e-5)
    y32, mean32, rstd32 = R.add_ln_fwd(f(res), f(a), mask, w, b, 1e-5)
    z = _D(res) + _D(a) * _D(mask)
    sy = (((z - mean64[:, None]) * rstd64[:, None] * _D(w)).abs().amax(-1) + _D(b).abs().max())[:, None]
    _bound(tag + ' y', _row_err(o['y'][1], y64, sy, bf), _row_err(y32, y64, sy, False))
    _bound(tag + ' mean', _row_err(o['mean'][1], mean64, z.abs().amax(-1), False), _row_err(mean32, mean64, z.abs().amax(-1), False))
    _bound(tag + ' rstd', _row_err(o['rstd'][1], rstd64, rstd64, False), _row_err(rstd32, rstd64, rstd64, False))
    if not bwd:
        return
    mean_k, rstd_k = o['mean'][1], o['rstd'][1]                       # the statistics the backward was given
    r64 = R.add_ln_bwd(_D(dy), _D(res), _D(a), _D(mask), _D(w), _D(mean_k), _D(rstd_k))
    r32 = R.add_ln_bwd(f(dy), f(res), f(a), mask, w, mean_k, rstd_k)
    d0 = x['dres0'].to(o['dres'][1].dtype)
    ref = r64['dres'] + (_D(d0) if accum else 0)
    ev32 = r32['dres'] + (f(d0) if accum else 0)
    sc = (r64['scale'] + (_D(d0).abs().amax(-1) if accum else 0))[:, None]
    _bound(tag + ' dres', _row_err(o['dres'][1], ref, sc, bf and not dres_f32), _row_err(ev32, ref, sc, False))
    if not da_none:
        sa = r64['scale'][:, None] * float(mask.max())
        _bound(tag + ' da', _row_err(o['da'][1], r64['da'], sa, bf), _row_err(r32['da'], r64['da'], sa, False))
    # exact: small-integer dy, integer starting value
    assert torch.equal(o['dbeta'][1].double(), START[1] + _D(dy).sum(0)), tag + ': dbeta is not the exact column sum of dy'
    _bound(tag + ' dgamma', _col_err(o['dgamma'][1], START[0], r64['t_dgamma']), _col_err(START[0] + r32['t_dgamma'].sum(0), START[0], r64['t_dgamma']))
    _bound(tag + ' dbias_a', _col_err(o['dbias'][1], START[2], r64['t_dbias']), _col_err(START[2] + r32['t_dbias'].sum(0), START[2], r64['t_dbias']))


def _ln_case(ops, dt, T, d, p, packed=False, bwd=True, **forms):
    x = _ln_inputs(dt, T, d)
    rid = np.arange(T) * 3 + 2 if packed else np.arange(T)              # gapped rows of a padded batch
    row_ids = torch.from_numpy(rid).int().cuda() if packed else None
    mask = R.drop_mask_rows(SEED, SITE, p, rid, d).cuda()
    o = _ln_run(ops, dt, x, p, row_ids=row_ids, bwd=bwd, **forms)
    tag = 'add_ln %s T=%d d=%d' % ('bf16' if dt == BF16 else 'f32', T, d)
    _ln_check(dt, x, o, mask, tag, bwd=bwd, **{k: v for k, v in forms.items() if k != 'shift'})
    return x, o


@pytest.mark.parametrize('dt', [F32, BF16])
@pytest.mark.parametrize('d', WIDTHS)
def test_add_ln_widths(ops, dt, d):
    """T = 67 (9 workgroups, the last with 3 live waves), dropout 0.1, every NIT instance and every partly filled last sweep; d = 2048
    is the backward at exactly 64 KiB of dynamic LDS. finalize_block: plain loop (9 partial rows).
    Measured ratios: the add_ln line of the module docstring."""
    _ln_case(ops, dt, 67, d, 0.1)


@pytest.mark.parametrize('dt', [F32, BF16])
@pytest.mark.parametrize('T', [1, 7, 8, 9, 3073, 4096, 4099, 8200])
def test_add_ln_row_loop(ops, dt, T):
    """d = 64, dropout 0.1 from the Philox reference. T 1 .. 9: one workgroup with idle waves, a full one, a second one. T = 3073 is the
    first T whose 385 partial rows enter finalize_block's 4-way unrolled branch; 4096 fills the backward grid (512 x 8 rows) exactly; 4099
    and 8200 make waves take a second and a third row with dgamma / dbeta / dbias_a carried in registers; the forward stays in one sweep.
    Measured ratios: the add_ln line of the module docstring."""
    _ln_case(ops, dt, T, 64, 0.1)


@pytest.mark.parametrize('dt', [F32, BF16])
def test_add_ln_fwd_second_sweep(ops, dt):
    """Forward only, d = 64, T = 16391: 7 rows past the 2048 x 8 rows of the forward grid; float64 on every row, and rows 0, 16383,
    16384, 16385, 16390 bit-equal to a 5-row packed call that draws the same dropout bits. Measured at this T: y 0.87, mean 1.06, rstd 0.90 (kernel figures 3.3, 0.81, 2.3
    in units of 2^-24 scale_row)."""
    T, d = 16391, 64
    x, o = _ln_case(ops, dt, T, d, 0.1, bwd=False)
    rows = _sweep_rows(T, 16384)
    assert rows == [0, 16383, 16384, 16385, 16390]
    idx = torch.tensor(rows, device='cuda')
    xs = {k: (v[idx] if v.dim() == 2 else v) for k, v in x.items()}
    s = _ln_run(ops, dt, xs, 0.1, row_ids=idx.int(), bwd=False)
    for k in ('y', 'mean', 'rstd'):
        assert torch.equal(o[k][1][idx], s[k][1]), k


@pytest.mark.parametrize('dt', [F32, BF16])
def test_add_ln_bwd_d2048_two_sweeps(ops, dt):
    """d = 2048, T = 4099: NIT = 8, a second row for three waves and 64 KiB of dynamic LDS in one launch; finalize_block's unrolled
    branch (512 partial rows). No dropout (the mask of 8.4M elements would cost seconds on the host).
    Measured: y 1.08, mean 1.00, rstd 0.93, dres 1.00, da 1.00, dgamma 0.67, dbias_a 0.84 (kernel figures: y 4.1, dres 3.0 in units of
    2^-24 scale_row; dgamma 9.1e-9, dbias_a 8.5e-9 of sum |term|)."""
    _ln_case(ops, dt, 4099, 2048, 0.0)


@pytest.mark.parametrize('dt', [F32, BF16])
@pytest.mark.parametrize('form', ['accum_dres', 'dres_f32', 'da_none', 'shifted', 'packed', 'packed_two_sweeps'])
def test_add_ln_forms(ops, dt, form):
    """Each argument form against float64 at d = 260 (NIT = 2, partial sweep), T = 67, dropout 0.1: dres accumulated into a non-zero
    dres; float32 dres beside bf16 activations (the float32 case is then the plain call); no da; dgamma / dbeta / dbias_a one float off
    16-byte alignment (the scalar finalize kernel); gapped row_ids; and gapped row_ids at T = 4099 (d = 64).
    Measured ratios: the add_ln line of the module docstring."""
    kw = dict(accum_dres=dict(accum=True), dres_f32=dict(dres_f32=dt == BF16), da_none=dict(da_none=True), shifted=dict(shift=1),
              packed=dict(packed=True), packed_two_sweeps=dict(packed=True))[form]
    T, d = (4099, 64) if form == 'packed_two_sweeps' else (67, 260)
    _ln_case(ops, dt, T, d, 0.1, **kw)


@pytest.mark.parametrize('dt', [F32, BF16])
def test_add_ln_rows_are_independent(ops, dt):
    """T = 8200, d = 64, dropout 0.1: three sweeps of the backward grid. y, mean, rstd, dres, da of rows 0, 4095, 4096, 4097, 8191, 8192,
    8193, 8199 are bit-equal to a packed 8-row call (one workgroup, one sweep) on those rows with their row numbers as row_ids."""
    T, d = 8200, 64
    x = _ln_inputs(dt, T, d, seed=5)
    o = _ln_run(ops, dt, x, 0.1)
    rows = _sweep_rows(T, 4096)
    assert rows == [0, 4095, 4096, 4097, 8191, 8192, 8193, 8199]
    idx = torch.tensor(rows, device='cuda')
    xs = {k: (v[idx] if v.dim() == 2 else v) for k, v in x.items()}
    s = _ln_run(ops, dt, xs, 0.1, row_ids=idx.int())
    for k in ('y', 'mean', 'rstd', 'dres', 'da'):
        assert torch.equal(o[k][1][idx], s[k][1]), k


def test_add_ln_refusals(ops):
    """d = 6 (no multiple of 4), d = 2052 (over the register budget) and d = 0 raise PBError and write nothing; T = 0 succeeds and
    writes nothing."""
    for T, d, ok in ((5, 6, False), (5, 2052, False), (5, 0, False), (0, 64, True)):
        dd = max(d, 4)
        mk = lambda *s: torch.ones(*s, device='cuda')
        res, a, dy, w, b = mk(T, d), mk(T, d), mk(T, d), mk(dd), mk(dd)
        o = dict(y=_galloc((T, d), F32, 2 * dd), mean=_galloc((T,), F32), rstd=_galloc((T,), F32), dres=_galloc((T, d), F32, 2 * dd),
                 da=_galloc((T, d), F32, 2 * dd), dgamma=_galloc((dd,), F32), dbeta=_galloc((dd,), F32), dbias=_galloc((dd,), F32))
        fwd = lambda: ops.add_ln_fwd(res, a, w, b, o['y'][1], o['mean'][1], o['rstd'][1], 1e-5, SEED, SITE, 0.0)
        bwd = lambda: ops.add_ln_bwd(dy, res, a, w, mk(T), mk(T), o['dres'][1], o['da'][1], o['dgamma'][1], o['dbeta'][1], o['dbias'][1],
                                     _partials(ops, dd), False, SEED, SITE, 0.0)
        for call in (fwd, bwd):
            if ok:
                call()
            else:
                with pytest.raises(ops.PBError):
                    call()
        for name, g in o.items():
            _gcheck(g, '%s (T=%d, d=%d)' % (name, T, d), written=False)


# ---------------------------------------------------------------- Octuple embedding + position + LayerNorm (+ dropout)
def _embed_inputs(ops, dt, T, S, d, seed=0):
    g = _gen(77 * d + T + seed)
    ids = torch.stack([torch.randint(0, n, (T,), device='cuda', generator=g) for n in ops.SEG_SIZES], dim=1)
    ids[0] = 0                                                          # the first and the last entry of every table
    ids[T - 1] = torch.tensor(ops.SEG_SIZES, device='cuda') - 1
    return dict(ids=ids, ids16=ops.ids_to_i16(ids), P=torch.randn(ops.VOCAB, d, device='cuda', generator=g),
                lb=torch.randn(d, device='cuda', generator=g), pos=torch.randn(S + 2, d, device='cuda', generator=g),
                w=1 + 0.2 * torch.randn(d, device='cuda', generator=g), b=0.2 * torch.randn(d, device='cuda', generator=g),
                dy=torch.randint(-3, 4, (T, d), device='cuda', generator=g).to(dt))


def _embed_run(ops, dt, x, S, p, route, row_ids=None, bwd=True):
    T, d = x['dy'].shape
    o = dict(y=_rows(T, d, dt), mean=_galloc((T,), F32), rstd=_galloc((T,), F32))
    ops.embed_ln_fwd(x['ids16'], x['P'], x['lb'], x['pos'], x['w'], x['b'], o['y'][1], o['mean'][1], o['rstd'][1], S, 1e-5, SEED, SITE, p,
                     row_ids=row_ids)
    if bwd:
        atomic = route == 'atomic'
        o['dP'] = _rows(ops.VOCAB, d, F32, 0.0 if atomic else None)
        o['dpos'] = _rows(S + 2, d, F32, 0.0 if atomic else None)
        o['dz'] = None if atomic else _rows(T, d, dt)
        for k, name in enumerate(('dgamma', 'dbeta', 'dbias')):
            o[name] = _galloc((d,), F32, 8, START[k])
        ops.embed_ln_bwd(x['dy'], x['ids16'], x['P'], x['lb'], x['pos'], x['w'], o['mean'][1], o['rstd'][1], o['dP'][1], o['dpos'][1],
                         o['dbias'][1], o['dgamma'][1], o['dbeta'][1], _partials(ops, d), S, SEED, SITE, p,
                         dz_out=None if atomic else o['dz'][1], row_ids=row_ids)
    for name, g in o.items():
        if g is not None:
            _gcheck(g, name, written=not (bwd and route == 'dz' and name in ('dP', 'dpos')))          # the dz route leaves dP / dpos alone
    return o


def _embed_check(ops, dt, x, o, S, mask, pos_idx, route, tag, bwd=True):
    bf = dt == BF16
    f = lambda t: t.float()
    off = ops.SEG_OFF
    ids, P, lb, pos, w, b, dy = (x[k] for k in ('ids', 'P', 'lb', 'pos', 'w', 'b', 'dy'))
    y64, mean64, rstd64 = R.embed_ln_fwd(ids, _D(P), off, _D(lb), _D(pos), pos_idx, _D(w), _D(b), 1e-5, _D(mask))
    y32, mean32, rstd32 = R.embed_ln_fwd(ids, P, off, lb, pos, pos_idx, w, b, 1e-5, mask)
    z = R.embed_z(ids, _D(P), off, _D(lb), _D(pos), pos_idx)
    sy = (((z - mean64[:, None]) * rstd64[:, None] * _D(w)).abs().amax(-1) + _D(b).abs().max())[:, None] * float(mask.max())
    _bound(tag + ' y', _row_err(o['y'][1], y64, sy, bf), _row_err(y32, y64, sy, False))
    _bound(tag + ' mean', _row_err(o['mean'][1], mean64, z.abs().amax(-1), False), _row_err(mean32, mean64, z.abs().amax(-1), False))
    _bound(tag + ' rstd', _row_err(o['rstd'][1], rstd64, rstd64, False), _row_err(rstd32, rstd64, rstd64, False))
    if not bwd:
        return
    mean_k, rstd_k = o['mean'][1], o['rstd'][1]
    r64 = R.embed_ln_bwd(_D(dy), ids, _D(P), off, _D(lb), _D(pos), pos_idx, _D(w), _D(mean_k), _D(rstd_k), _D(mask))
    r32 = R.embed_ln_bwd(f(dy), ids, P, off, lb, pos, pos_idx, w, mean_k, rstd_k, mask)
    if route == 'dz':
        sc = r64['scale'][:, None]
        _bound(tag + ' dz', _row_err(o['dz'][1], r64['dz'], sc, bf), _row_err(r32['dz'], r64['dz'], sc, False))
    else:
        # an element of dP / dpos is a sum of dz elements: measured in units of 2^-24 x the summed row scales of its addends
        for name, sn in (('dP', 'sP'), ('dpos', 'spos')):
            got, used = o[name][1], r64[sn] > 0
            assert bool((got[~used] == 0).all()), tag + ': %s changed where no row with a gradient points' % name
            sc = r64[sn][used][:, None]
            _bound(tag + ' ' + name, _row_err(got[used], r64[name][used], sc, False), _row_err(r32[name][used], r64[name][used], sc, False))
    if float(mask.max()) == 1.0:
        assert torch.equal(o['dbeta'][1].double(), START[1] + _D(dy).sum(0)), tag + ': dbeta is not the exact column sum of dy'
    else:
        _bound(tag + ' dbeta', _col_err(o['dbeta'][1], START[1], r64['t_dbeta']), _col_err(START[1] + r32['t_dbeta'].sum(0), START[1], r64['t_dbeta']))
    _bound(tag + ' dgamma', _col_err(o['dgamma'][1], START[0], r64['t_dgamma']), _col_err(START[0] + r32['t_dgamma'].sum(0), START[0], r64['t_dgamma']))
    _bound(tag + ' dbias', _col_err(o['dbias'][1], START[2], r64['t_dbias']), _col_err(START[2] + r32['t_dbias'].sum(0), START[2], r64['t_dbias']))


def _embed_case(ops, dt, B, S, d, p, route, packed=False, bwd=True):
    T = B * S
    rid = np.arange(T)
    if packed:                                                          # every third row of the padded batch is missing
        rid = rid[rid % 3 != 1]
        T = len(rid)
    x = _embed_inputs(ops, dt, T, S, d)
    row_ids = torch.from_numpy(rid).int().cuda() if packed else None
    mask = R.drop_mask_rows(SEED, SITE, p, rid, d).cuda()
    pos_idx = torch.from_numpy(rid % S).cuda()
    o = _embed_run(ops, dt, x, S, p, route, row_ids=row_ids, bwd=bwd)
    tag = 'embed_ln %s %s T=%d S=%d d=%d' % ('bf16' if dt == BF16 else 'f32', route, T, S, d)
    _embed_check(ops, dt, x, o, S, mask, pos_idx, route, tag, bwd=bwd)
    return x, o


@pytest.mark.parametrize('dt', [F32, BF16])
@pytest.mark.parametrize('route', ['atomic', 'dz'])
@pytest.mark.parametrize('d', WIDTHS)
def test_embed_ln_widths(ops, dt, route, d):
    """B x S = 3 x 23, no dropout (dbeta is then the exact integer column sum), both backward routes: float32 atomics into dP / dpos, and
    dz written out (dP and dpos must stay untouched). Row 0 holds id 0 of every table, the last row every table's last id.
    dP / dpos are measured in units of 2^-24 x the summed row scales of the dz rows added into the element (row_ref.embed_ln_bwd).
    Measured ratios: the embed_ln line of the module docstring."""
    _embed_case(ops, dt, 3, 23, d, 0.0, route)


@pytest.mark.parametrize('dt', [F32, BF16])
@pytest.mark.parametrize('B,S,p,route,packed', [(1, 4099, 0.0, 'atomic', False), (8, 513, 0.1, 'dz', False), (8, 513, 0.1, 'atomic', False),
                                                 (9, 700, 0.1, 'dz', True), (3, 23, 0.1, 'atomic', True)])
def test_embed_ln_row_loop(ops, dt, B, S, p, route, packed):
    """d = 64. T = 4099 as one sequence (positions never wrap); T = 4104 with S = 513 (the position index wraps 8 times, and not at a
    sweep boundary) with dropout after the LayerNorm; packed rows (two of every three rows of a 9 x 700 batch: T = 4200, a second
    sweep with gapped row_ids, and the small 3 x 23 one). finalize_block: unrolled branch for T > 3072.
    Measured ratios: the embed_ln line of the module docstring."""
    _embed_case(ops, dt, B, S, 64, p, route, packed=packed)


@pytest.mark.parametrize('dt', [F32, BF16])
def test_embed_ln_rows_are_independent(ops, dt):
    """d = 64, dropout 0.1. Forward at T = 16400 (S = 2050): rows 0, 16383, 16384, 16385, 16399 against a packed 5-row call; backward
    (dz route) at T = 4104 (S = 513): rows 0, 4095, 4096, 4097, 4103. torch.equal on y, mean, rstd and dz. The forward at T = 16400 is also
    compared with float64 on every row (ratios: the embed_ln line of the module docstring)."""
    x, o = _embed_case(ops, dt, 8, 2050, 64, 0.1, 'dz', bwd=False)
    for S, T, per, bwd in ((2050, 16400, 16384, False), (513, 4104, 4096, True)):
        if bwd:
            x = _embed_inputs(ops, dt, T, S, 64, seed=3)
            o = _embed_run(ops, dt, x, S, 0.1, 'dz')
        rows = _sweep_rows(T, per)
        idx = torch.tensor(rows, device='cuda')
        xs = {k: (v[idx] if k in ('ids', 'ids16', 'dy') else v) for k, v in x.items()}
        s = _embed_run(ops, dt, xs, S, 0.1, 'dz', row_ids=idx.int(), bwd=bwd)
        for k in ('y', 'mean', 'rstd') + (('dz',) if bwd else ()):
            assert torch.equal(o[k][1][idx], s[k][1]), (T, k)


@pytest.mark.parametrize('dt', [F32, BF16])
def test_embed_ln_zero_rows_are_skipped(ops, dt):
    """The atomic route skips a row whose dy is all zero. B x S = 2 x 24 with rows 10 .. 17 zero: dP and dpos must be bit-equal to a packed
    call without those rows. Every table entry and position is used by at most two live rows (ids = position mod table size), and a
    sum of two float32 terms does not depend on their order, so the atomics cannot blur the comparison."""
    B, S, d = 2, 24, 260
    T = B * S
    x = _embed_inputs(ops, dt, T, S, d)
    x['ids'] = torch.stack([torch.arange(T, device='cuda') % S % n for n in ops.SEG_SIZES], dim=1)
    x['ids16'] = ops.ids_to_i16(x['ids'])
    x['dy'][10:18] = 0
    o = _embed_run(ops, dt, x, S, 0.0, 'atomic')
    keep = torch.tensor([r for r in range(T) if not 10 <= r < 18], device='cuda')
    xs = {k: (v[keep] if k in ('ids', 'ids16', 'dy') else v) for k, v in x.items()}
    s = _embed_run(ops, dt, xs, S, 0.0, 'atomic', row_ids=keep.int())
    assert torch.equal(o['dP'][1], s['dP'][1]) and torch.equal(o['dpos'][1], s['dpos'][1])
    assert float(o['dP'][1].abs().max()) > 0
    _embed_check(ops, dt, x, o, S, torch.ones(T, d, device='cuda'), torch.arange(T, device='cuda') % S, 'atomic', 'embed_ln zero rows')


def test_embed_ln_refusals(ops):
    """d = 6, d = 2052 and T no multiple of S raise PBError and write nothing."""
    for T, S, d in ((6, 3, 6), (6, 3, 2052), (7, 3, 64)):
        x = _embed_inputs(ops, F32, T, S, d)
        o = dict(y=_rows(T, d, F32), mean=_galloc((T,), F32), rstd=_galloc((T,), F32))
        with pytest.raises(ops.PBError):
            ops.embed_ln_fwd(x['ids16'], x['P'], x['lb'], x['pos'], x['w'], x['b'], o['y'][1], o['mean'][1], o['rstd'][1], S, 1e-5, 0, 0, 0.0)
        for name, g in o.items():
            _gcheck(g, name, written=False)


# ---------------------------------------------------------------- column sums, batch sum
@pytest.mark.parametrize('dt', [F32, BF16])
@pytest.mark.parametrize('T', [1, 63, 64, 65, 8200])
def test_colsum_exact(ops, dt, T):
    """pb_colsum (N = 260 of a row stride of 264: a second, partly filled column block) and pb_colsum_any (N = 259, stride 261) on small
    integers with a non-zero integer start: the float32 result EQUALS the float64 column sum. T = 65 is the first T with two row
    blocks; T = 8200 gives 128 row blocks of 65 rows (the 4-rows-in-flight loop and its remainder loop) and 128 partial rows, the most
    pb_colsum's grid allows: finalize_block's unrolled branch (> 384 partial rows) cannot be reached through pb_colsum."""
    g = _gen(T)
    src = torch.randint(-3, 4, (T, 264), device='cuda', generator=g).to(dt)
    ws = torch.empty(int(ops.LIB.query('pb_colsum_partials_floats', 264)), device='cuda')
    out = _galloc((260,), F32, 8, 3.0)
    ops.colsum(src, out[1], ws, T, 260, ld=264)
    _gcheck(out, 'colsum')
    assert torch.equal(out[1].double(), 3.0 + src[:, :260].double().sum(0))
    src = src.reshape(-1)[:T * 261].reshape(T, 261)
    out = _galloc((259,), F32, 8, 3.0)
    ops.colsum_any(src, out[1], ws, T, 259, ld=261)
    _gcheck(out, 'colsum_any')
    assert torch.equal(out[1].double(), 3.0 + src[:, :259].double().sum(0))


@pytest.mark.parametrize('dt', [F32, BF16])
@pytest.mark.parametrize('Sd', [4, 1028, 2097152 + 1028])
def test_batch_sum_exact(ops, dt, Sd):
    """out[i] += sum_b x[b][i], B = 3, small integers: exact. Sd = 2 098 180 is 257 elements of 4 past one sweep of the 2048 x 256 grid."""
    x = torch.randint(-3, 4, (3, Sd), device='cuda', generator=_gen(Sd)).to(dt)
    out = _galloc((Sd,), F32, 8, 2.0)
    ops.batch_sum(x, out[1], 3, Sd)
    _gcheck(out, 'batch_sum')
    assert torch.equal(out[1].double(), 2.0 + x.double().sum(0))


# ---------------------------------------------------------------- masked softmax
def _softmax_case(ops, dt, B, H, Sq, Sk, causal, km, scores, scale, tag):
    bf = dt == BF16
    rows = B * H * Sq
    Pg = _galloc((B, H, Sq, Sk), dt, max(8, 2 * Sk))
    ops.softmax_fwd(scores, km, Pg[1], B, H, Sq, Sk, scale, causal)
    _gcheck(Pg, 'P')
    P = Pg[1]
    scale32 = float(np.float32(scale))
    ref = R.softmax_fwd(_D(scores), km, scale32, causal)
    ev32 = R.softmax_fwd(scores, km, scale32, causal)
    vis = R.softmax_visible(B, H, Sq, Sk, km, causal, 'cuda')
    assert bool((P[~vis] == 0).all()), tag + ': a masked position is not exactly 0'
    assert bool((P[~vis.any(-1)] == 0).all())
    one = torch.ones((), dtype=torch.float64, device='cuda')
    _bound(tag + ' P', _row_err(P, ref, one, bf), _row_err(ev32, ref, one, False))
    # rows sum to 1 (or 0) within the same bound, summed over the row's elements
    live = vis.any(-1)
    tot = P.double().sum(-1)
    k32 = _row_err(ev32, ref, one, False)
    assert bool(((tot - live.double()).abs() <= Sk * MARGIN * k32 * E24 + (E8 if bf else 0)).all()), tag + ': row sums'
    dP = torch.randn(B, H, Sq, Sk, device='cuda', generator=_gen(Sq + Sk))
    dSg = _galloc((B, H, Sq, Sk), dt, max(8, 2 * Sk))
    ops.softmax_bwd(dP, P, dSg[1], rows, Sk, scale)
    _gcheck(dSg, 'dS')
    rb = R.softmax_bwd(_D(dP), _D(P), scale32)
    e32 = R.softmax_bwd(dP, P.float(), scale32)
    sc = abs(scale32) * (dP.double().abs().amax(-1, keepdim=True) + (dP.double() * P.double()).abs().sum(-1, keepdim=True))
    _bound(tag + ' dS', _row_err(dSg[1], rb, sc, bf), _row_err(e32, rb, sc, False))
    return P, dSg[1], dP


@pytest.mark.parametrize('dt', [F32, BF16])
@pytest.mark.parametrize('causal', [False, True])
@pytest.mark.parametrize('Sq,Sk', [(1, 1), (5, 63), (5, 64), (5, 65), (7, 130), (130, 7), (3, 1029)])
@pytest.mark.parametrize('masked', [False, True])
def test_softmax_shapes(ops, dt, causal, Sq, Sk, masked):
    """B = 2, H = 3, scale 0.25. Sk 63 / 64 / 65 / 130 / 1029: one partly filled 64-lane sweep, one full, a second, a third, seventeen;
    Sq != Sk both ways (causal: key j visible iff j <= i, so Sq = 130 > Sk = 7 has rows that see every key and Sq < Sk rows that see a
    prefix). masked: batch 1 sees no key (zero rows), key 0 of batch 0 is masked (causal query 0 then has no candidate left), the rest
    at random; not masked: key_mask = None. Masked positions are exactly 0.
    Measured over the 56 cases: worst ratio P 1.50, dS 1.62 (largest kernel figures P 1.41, dS 0.43 in units of 2^-24 scale_row; bf16: the
    error never leaves the one-ulp allowance, figure 0)."""
    B, H = 2, 3
    g = _gen(Sq * 31 + Sk)
    scores = 3 * torch.randn(B, H, Sq, Sk, device='cuda', generator=g)
    km = None
    if masked:
        km = (torch.rand(B, Sk, device='cuda', generator=g) > 0.3).float()
        km[1] = 0
        km[0, 0] = 0
    _softmax_case(ops, dt, B, H, Sq, Sk, causal, km, scores, 0.25, 'softmax %s Sq=%d Sk=%d c=%d m=%d' % ('bf16' if dt == BF16 else 'f32', Sq, Sk, causal, masked))


@pytest.mark.parametrize('dt', [F32, BF16])
def test_softmax_extreme_scores(ops, dt):
    """Scores of +-80 at scale 1 (exp(80) overflows nothing only with the maximum subtracted; exp(-160) underflows to 0): no inf or NaN,
    and the rows sum to 1 within the bound. Measured: P 1.00, dS 1.00 (kernel figures 0.029, 0.019: the float32
    kernel gives torch's bits here)."""
    B, H, Sq, Sk = 1, 2, 6, 70
    g = _gen(80)
    scores = torch.where(torch.rand(B, H, Sq, Sk, device='cuda', generator=g) < 0.5, 80.0, -80.0)
    scores[0, 0, 0] = -80.0                                             # a row of equal minima
    scores[0, 0, 1] = 80.0
    scores[0, 0, 2, 1:] = -80.0; scores[0, 0, 2, 0] = 80.0                # one maximum
    P, dS, _ = _softmax_case(ops, dt, B, H, Sq, Sk, False, None, scores, 1.0, 'softmax %s +-80' % ('bf16' if dt == BF16 else 'f32'))
    assert bool(torch.isfinite(P).all()) and bool(torch.isfinite(dS).all())
    assert float(P[0, 0, 2, 0]) == 1.0 and float(P[0, 0, 2, 1:].abs().max()) == 0.0


@pytest.mark.parametrize('dt', [F32, BF16])
def test_softmax_second_sweep(ops, dt):
    """B = 2, H = 3, Sq = 2741, Sk = 8: 16446 rows, 62 past one sweep of the 4096 x 4 grid. Causal and not against float64 on every row;
    then rows 0, 16383, 16384, 16385, 16445 of the non-causal P and dS bit-equal to a call on those five rows alone (B = 5, H = Sq = 1,
    each with the key mask of its batch). Measured: P 1.08, dS 1.00 (kernel figures 1.92, 0.63), causal and not."""
    B, H, Sq, Sk = 2, 3, 2741, 8
    g = _gen(2741)
    scores = 3 * torch.randn(B, H, Sq, Sk, device='cuda', generator=g)
    km = (torch.rand(B, Sk, device='cuda', generator=g) > 0.3).float()
    km[:, 0] = 1
    name = 'bf16' if dt == BF16 else 'f32'
    _softmax_case(ops, dt, B, H, Sq, Sk, True, km, scores, 0.25, 'softmax %s 16446 rows causal' % name)
    P, dS, dP = _softmax_case(ops, dt, B, H, Sq, Sk, False, km, scores, 0.25, 'softmax %s 16446 rows' % name)
    rows = _sweep_rows(B * H * Sq, 16384)
    assert rows == [0, 16383, 16384, 16385, 16445]
    idx = torch.tensor(rows, device='cuda')
    sm = scores.reshape(-1, Sk)[idx].reshape(5, 1, 1, Sk).contiguous()
    kms = km[idx // (H * Sq)].contiguous()
    Ps = torch.empty(5, 1, 1, Sk, device='cuda', dtype=dt)
    ops.softmax_fwd(sm, kms, Ps, 5, 1, 1, Sk, 0.25, False)
    assert torch.equal(Ps.reshape(5, Sk), P.reshape(-1, Sk)[idx])
    dSs = torch.empty_like(Ps)
    ops.softmax_bwd(dP.reshape(-1, Sk)[idx].contiguous(), Ps, dSs, 5, Sk, 0.25)
    assert torch.equal(dSs.reshape(5, Sk), dS.reshape(-1, Sk)[idx])


# ---------------------------------------------------------------- cross-entropy, mask count, loss coefficients
LAYOUTS = {'reg': [70, 7, 8, 64, 65, 129, 9, 12],          # every head <= 320 classes: the register-resident kernel
           'generic': [330, 7, 8, 64, 65, 129, 9, 12]}     # one head of 330 classes: the generic kernel for the whole row
SUMS0 = [0.5] * 8 + [3.0] * 8 + [2.0] * 8                  # `sums` going in: it is accumulated into


def _ce_inputs(sizes, T, seed=0):
    """logits whose float64 top-2 gap is >= 0.01 in every head of every row (the maximum is raised), except the planted exact ties;
    targets at class 0 (row 0) and at the last class (last row); head 6 without any loss position."""
    off = [0] + [int(v) for v in np.cumsum(sizes)]
    g = _gen(T + len(sizes) + sizes[0] + seed)
    logits = 2 * torch.randn(T, off[8], device='cuda', generator=g)
    for i in range(8):
        seg = logits[:, off[i]:off[i + 1]]
        seg.scatter_add_(1, seg.argmax(-1, keepdim=True), torch.full((T, 1), 0.01, device='cuda'))
    target = torch.stack([torch.randint(0, n, (T,), device='cuda', generator=g) for n in sizes], dim=1)
    target[0] = 0
    target[T - 1] = torch.tensor(sizes, device='cuda') - 1
    ties = {}
    if T >= 3:                                                          # row 1: first and last class of head 0; row 2: classes 63 / 64 / 128 of head 5
        logits[1, 0] = logits[1, sizes[0] - 1] = 50.0
        logits[2, off[5] + 63] = logits[2, off[5] + 64] = logits[2, off[5] + 128] = 50.0
        logits[2, off[0] + 1] = logits[2, off[0] + 64] = 50.0           # lane 1's first class against lane 0's second
        ties = {(1, 0): 0, (2, 5): 63, (2, 0): 1}
    m = (torch.rand(T, 8, device='cuda', generator=g) < 0.6).float()
    m[0] = 1
    m[:, 6] = 0
    return off, logits, target, m.contiguous(), ties


def _ce_case(ops, dt, kind, T, with_dl=True, with_am=True, seed=0):
    sizes = LAYOUTS[kind]
    lay = ops.Layout(sizes)
    off, logits, target, m, ties = _ce_inputs(sizes, T, seed)
    V = off[8]
    tag = 'ce %s %s T=%d' % (kind, {F32: 'f32', BF16: 'bf16', None: 'no dlogits'}[dt if with_dl else None], T)
    ws = torch.empty(int(ops.LIB.query('pb_ce_partials_floats')), device='cuda')
    counts, coef = _galloc((8,), F32), _galloc((8,), F32)
    ops.mask_count(m, counts[1], ws)
    w = torch.tensor([3.0, 1, 4, 1, 5, 9, 2, 6], device='cuda')
    ops.loss_coef(counts[1], w, coef[1])
    torch.cuda.synchronize()
    _gcheck(counts, 'counts')
    _gcheck(coef, 'coef', finite=coef[1][:6])
    assert torch.equal(counts[1].double(), m.double().sum(0)), tag + ': mask count'
    cref = R.loss_coef(counts[1].double(), w.double())
    assert torch.isinf(coef[1][6]) and coef[1][6] > 0
    live = [i for i in range(8) if i != 6]
    # w >= 0: the sum of 8 (7 roundings), the product, the multiplication by scale and the division: 10 roundings of 2^-24 at the most
    assert float(((coef[1].double() - cref).abs() / cref)[live].max()) <= 10 * E24, tag + ': loss_coef'
    sums = _galloc((24,), F32, 8, SUMS0)
    dl = _rows(T, V, dt) if with_dl else None
    am = _galloc((T, 8), torch.int16, 16) if with_am else None
    ops.ce_fwd_bwd(logits, target.to(torch.int16), m, sums[1], ws, coef[1], dl[1] if with_dl else None, am[1] if with_am else None, layout=lay)
    _gcheck(sums, 'sums')
    r64 = R.ce_fwd_bwd(_D(logits), target, _D(m), off, _D(coef[1]))
    r32 = R.ce_fwd_bwd(logits, target, m, off, coef[1])
    for (row, head), want in ties.items():
        assert int(r64['argmax'][row, head]) == want
    if with_am:
        _gcheck(am, 'argmax')
        assert torch.equal(am[1].long(), r64['argmax']), tag + ': argmax (every row; ties: the lowest index)'
    s0 = torch.tensor(SUMS0, device='cuda', dtype=torch.float64).reshape(3, 8)
    got = sums[1].reshape(3, 8)
    assert torch.equal(got[1:].double(), s0[1:] + r64['terms'][1:].sum(1)), tag + ': mask / correct counts are not exact'
    _bound(tag + ' loss sums', _col_err(got[0], s0[0], r64['terms'][0]), _col_err(s0[0].float() + r32['terms'][0].sum(0), s0[0], r64['terms'][0]))
    if with_dl:
        _gcheck(dl, 'dlogits', finite=torch.cat([dl[1][:, :off[6]], dl[1][:, off[7]:]], 1))
        nan_ref = torch.isnan(r64['dlogits'])
        assert torch.equal(torch.isnan(dl[1]), nan_ref) and bool(nan_ref[:, off[6]:off[7]].all()) and int(nan_ref.sum()) == T * sizes[6]
        sc = torch.cat([r64['gscale'][:, i:i + 1].expand(T, sizes[i]) for i in range(8)], 1)
        cols = torch.tensor([c for i in live for c in range(off[i], off[i + 1])], device='cuda')
        on = sc[:, cols] > 0
        assert bool((dl[1][:, cols][~on] == 0).all()), tag + ': dlogits of a position without loss'
        pick = lambda t: t[:, cols][on]
        _bound(tag + ' dlogits', _row_err(pick(dl[1]), pick(r64['dlogits']), pick(sc), dt == BF16), _row_err(pick(r32['dlogits']), pick(r64['dlogits']), pick(sc), False))
    return dict(logits=logits, target=target, m=m, coef=coef[1], dl=dl[1] if with_dl else None, am=am[1] if with_am else None, lay=lay, off=off)


@pytest.mark.parametrize('dt', [F32, BF16])
@pytest.mark.parametrize('kind', ['reg', 'generic'])
@pytest.mark.parametrize('T', [1, 3, 4, 5, 8197])
def test_ce_row_loop(ops, dt, kind, T):
    """Small dictionaries (V = 364 / 624) through both kernels. T 1, 3, 4, 5: idle waves, one full workgroup, a second; T = 8197 is five
    rows past one sweep of the 2048 x 4 grid, and ce_finalize's 8-way unrolled loop (2048 partial rows). sums start non-zero; planes 1
    and 2 (mask count, correct count) are exact; argmax is compared on EVERY row (top-2 gap >= 0.01, except the planted ties: first /
    last class of a head, classes 63 / 64 / 128, classes 1 / 64: the lowest index wins); targets at class 0 and n - 1; head 6 has no loss
    position, so coef = inf and dlogits is NaN exactly where inf * 0 is in the reference.
    Measured over all cross-entropy cases of this file: worst ratio loss sums 1.85 (kernel 7.9e-8 of sum |term| at T = 8197, generic kernel;
    largest kernel figure 1.15e-7 at T = 1), dlogits 1.23 (largest kernel figure 3.96 in units of 2^-24 |coef m|; bf16: 0)."""
    _ce_case(ops, dt, kind, T)


@pytest.mark.parametrize('kind', ['reg', 'generic'])
def test_ce_optional_outputs(ops, kind):
    """dlogits = None, argmax_out = None, and both: the sums and the remaining output do not change by a bit."""
    full = _ce_case(ops, F32, kind, 333)
    a = _ce_case(ops, F32, kind, 333, with_dl=False)
    b = _ce_case(ops, F32, kind, 333, with_am=False)
    _ce_case(ops, F32, kind, 333, with_dl=False, with_am=False)
    assert torch.equal(a['am'], full['am'])
    assert torch.equal(b['dl'][:, :full['off'][6]], full['dl'][:, :full['off'][6]])


@pytest.mark.parametrize('dt', [F32, BF16])
@pytest.mark.parametrize('kind', ['reg', 'generic'])
def test_ce_rows_are_independent(ops, dt, kind):
    """T = 8197: dlogits and argmax of rows 0, 8191, 8192, 8193, 8196 bit-equal to a 5-row call (NaN columns of the empty head excluded)."""
    c = _ce_case(ops, dt, kind, 8197, seed=1)
    rows = _sweep_rows(8197, 8192)
    assert rows == [0, 8191, 8192, 8193, 8196]
    idx = torch.tensor(rows, device='cuda')
    V = c['off'][8]
    dl = torch.empty(5, V, device='cuda', dtype=dt); am = torch.empty(5, 8, device='cuda', dtype=torch.int16)
    ws = torch.empty(int(ops.LIB.query('pb_ce_partials_floats')), device='cuda')
    ops.ce_fwd_bwd(c['logits'][idx].contiguous(), c['target'][idx].to(torch.int16).contiguous(), c['m'][idx].contiguous(), torch.zeros(24, device='cuda'),
                   ws, c['coef'], dl, am, layout=c['lay'])
    keep = torch.tensor([col for i in range(8) if i != 6 for col in range(c['off'][i], c['off'][i + 1])], device='cuda')
    assert torch.equal(am, c['am'][idx]) and torch.equal(dl[:, keep], c['dl'][idx][:, keep])


@pytest.mark.parametrize('T', [0, 1, 31, 32, 33, 4099])
def test_mask_count_exact(ops, T):
    """counts = column sums of a 0 / 1 mask: exact. 32 rows per workgroup, 128 workgroups: T = 4099 is three rows into a second sweep.
    T = 0 writes zeros."""
    m = (torch.rand(T, 8, device='cuda', generator=_gen(T + 1)) < 0.5).float()
    counts = _galloc((8,), F32)
    ws = torch.empty(int(ops.LIB.query('pb_ce_partials_floats')), device='cuda')
    ops.mask_count(m, counts[1], ws)
    _gcheck(counts, 'counts')
    assert torch.equal(counts[1].double(), m.double().sum(0))


# ---------------------------------------------------------------- optimizer, casts, fill
SIZES = [1, 3, 4, 5, 1027, 2097152 + 3 * 1024 + 3]


@pytest.mark.parametrize('n', SIZES)
def test_sqnorm_and_clip(ops, n):
    """sum g^2 against float64, error relative to the sum (all terms positive) and bounded by four times that of torch's float32
    (g * g).sum(); the finalize adds the <= 2048 block sums in double. clip_coef: sqrt, product, sum, quotient, min, product: 6 roundings.
    Measured: ratio 1.00 at n = 1, 3, 4, 1027 and 2 100 227 (kernel 2.6e-8, 1.5e-8, 1.3e-8, 1.2e-8, 1.3e-8: torch's bits), 0.01 at n = 5."""
    g = torch.randn(n + 8, device='cuda', generator=_gen(n))[:n] * 0.1
    ws = torch.empty(int(ops.LIB.query('pb_norm_partials_floats')), device='cuda')
    sq, coef = _galloc((1,), F32), _galloc((1,), F32)
    ops.grad_sqnorm(g, ws, sq[1])
    _gcheck(sq, 'sq')
    ref = (g.double() ** 2).sum()
    _bound('sqnorm n=%d' % n, abs(float(sq[1].double() - ref)) / float(ref), abs(float((g * g).sum().double() - ref)) / float(ref))
    for max_norm, gscale in ((3.0, 1.0), (1e-3, 0.5)):
        ops.clip_coef(sq[1], max_norm, gscale, coef[1])
        _gcheck(coef, 'coef')
        cref = R.clip_coef(sq[1].double(), float(np.float32(max_norm)), gscale)
        assert abs(float(coef[1].double() - cref)) <= 6 * E24 * float(cref)


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('wd,clip,shadow', [(0.01, True, True), (0.0, False, False), (0.01, False, True), (0.0, True, False)])
def test_adamw_steps(ops, n, wd, clip, shadow):
    """Three steps, each against the float64 transcription of the formula in the header of pb_optim.hip applied to the state the kernel
    was given (hyper-parameters rounded to float32 as the ABI takes them). Per element: p within k 2^-24 (|p| + |update|), m within
    k 2^-24 (b1 |m| + (1 - b1) |g|), v likewise, k = 4 x the float32 torch evaluation's. The shadow is p.to(bfloat16) bit for bit;
    n = 2 100 227 takes a second sweep of the 2048 x 256 x 4 grid and a 3-element scalar tail.
    Measured over the 24 cases x 3 steps: worst ratio p 1.08, m 1.22, v 1.91 (n = 5: 1.28 against 0.67); largest kernel figures p 4.07,
    m 1.71, v 3.79 (units of 2^-24 scale), all three equal to torch's at n = 2 100 227."""
    g = _gen(n)
    f32r = lambda v: float(np.float32(v))
    lr, b1, b2, eps = f32r(1e-3), f32r(0.9), f32r(0.999), f32r(1e-6)
    wdr = f32r(wd)
    st = {k: _galloc((n,), F32, 8, torch.randn(n, device='cuda', generator=g) * s) for k, s in (('p', 1.0), ('m', 0.0), ('v', 0.0))}
    gr = torch.randn(n + 8, device='cuda', generator=g)[:n] * 0.1
    sh = _galloc((n,), BF16, 8) if shadow else None
    cl = torch.tensor([0.37], device='cuda') if clip else None
    for step in (1, 2, 3):
        before = {k: v[1].clone() for k, v in st.items()}
        ops.adamw_step(st['p'][1], gr, st['m'][1], st['v'][1], sh[1] if shadow else None, cl, lr, b1, b2, eps, wdr, step)
        for k, v in st.items():
            _gcheck(v, k)
        # lr * weight_decay is one float32 product on the host side of the kernel
        wd_eff = f32r(np.float32(lr) * np.float32(wdr)) / lr
        r64 = R.adamw_step(_D(before['p']), _D(gr), _D(before['m']), _D(before['v']), _D(cl) if clip else None, lr, b1, b2, eps, wd_eff, step)
        r32 = R.adamw_step(before['p'], gr, before['m'], before['v'], cl if clip else None, lr, b1, b2, eps, wd_eff, step)
        gc = _D(gr) * (_D(cl) if clip else 1.0)
        upd = (r64[0] - _D(before['p'])).abs()
        scales = (_D(before['p']).abs() + upd, b1 * _D(before['m']).abs() + (1 - b1) * gc.abs(), b2 * _D(before['v']) + (1 - b2) * gc * gc)
        for k, ref, ev, sc in zip('pmv', r64, r32, scales):
            _bound('adamw n=%d wd=%g clip=%d step %d %s' % (n, wd, clip, step, k), _row_err(st[k][1], ref, sc, False), _row_err(ev, ref, sc, False))
        if shadow:
            _gcheck(sh, 'shadow')
            assert torch.equal(sh[1], st['p'][1].to(BF16))


@pytest.mark.parametrize('n', [5, 1027])
def test_adamw_tail_follows_the_body(ops, n):
    """Equal elements in, equal bits out: the n & 3 tail elements (scalar code) must round as the float4 body does."""
    st = [torch.full((n,), v, device='cuda') for v in (0.7310585975646973, 0.0123456, 0.0003217, 3.1e-5)]
    p, gr, m, v = st
    sh = torch.empty(n, device='cuda', dtype=BF16)
    for step in (1, 2, 3):
        ops.adamw_step(p, gr, m, v, sh, torch.tensor([0.37], device='cuda'), 1e-3, 0.9, 0.999, 1e-6, 0.01, step)
        for t in (p, m, v, sh):
            assert bool((t == t[0]).all()), step


@pytest.mark.parametrize('n', SIZES)
def test_casts_and_fill(ops, n):
    """float32 -> bf16 (round to nearest even, as torch), bf16 -> float32 and fill: bit-exact, guard elements untouched at every n."""
    x = torch.randn(n + 8, device='cuda', generator=_gen(n))[:n]
    xb = _galloc((n,), BF16)
    ops.cast_f32_to_bf16(x, xb[1])
    _gcheck(xb, 'bf16')
    assert torch.equal(xb[1], x.to(BF16))
    xf = _galloc((n,), F32)
    ops.cast_bf16_to_f32(xb[1], xf[1])
    _gcheck(xf, 'f32')
    assert torch.equal(xf[1], xb[1].float())
    fl = _galloc((n,), F32)
    ops.fill_f32(fl[1], -2.5)
    _gcheck(fl, 'fill')
    assert bool((fl[1] == -2.5).all())
