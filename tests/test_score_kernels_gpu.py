"""GPU: the scoring kernels (csrc/pb_score.hip: pb_token_scores in its register and its wide form, pb_seq_scores) at every head-width and
target edge, against the float64 reference of tests/score_ref.py (checked in tests/test_score_ref_cpu.py), and Engine.score on the
small model of tests/test_score_gpu.py. The C ABI is driven through ops.LIB.call with the test's own int32[9] offsets: ops.Layout wants
at least 7 classes per head, the kernel takes 1 .. 1088.

Without a tolerance: rank against float64 on every live (row, head), targets outside the head included; rank == 0 exactly where
pb_ce_fwd_bwd's argmax is the target (targets inside the head: a target < 0 on a row without a positive logit has rank 0 and is no
argmax); masked rows 0 / 0 / -1; a head of one class 0 / 0 / 0; the four calls (all outputs, logp alone, logp + entropy, logp + rank)
bit-equal in what they share; rows independent of T and of their place in the grid-stride loop, bit for bit; heads 1 .. 7 of the
'switch' layout (wide form) bit-equal to the same heads of 'narrow_edges' (register form); pb_seq_scores equal to the float64 sums on
small integers with weights 0 / 1 / 2 / 0.5, unmoved by NaN / inf under a zero of the mask, and equal bytes from two launches; Engine.score
bit-equal wherever two (start, length) windows overlap. Every output sits between guard elements (a finite sentinel; the inside starts as
NaN / SENT): the guards are untouched, everything written is finite, and logits, target and mask keep their bits. T = 0 and every
refused call write nothing.

With a bound: logp and entropy, per live element with a positive scale, |got - float64| / (2^-24 S) with S = S_logp / S_entropy of
score_ref. The kernel's worst figure over a (layout, output, row family) may reach MARGIN = 4 times the worst figure of the float32
model (score_ref.token_scores on float32 tensors, no option) on the same rows, a model figure below 1 unit counting as 1 (the floor of
tests/test_attention_kernels_gpu.py: a uniform head of 1088 classes leaves the model exact to 0.008). pb_seq_scores on random floats: per
plane |got - sum| / sum |term| against 4 times the float32 model's, floor 2^-24; that model adds in the order the header documents
(score_ref.seq_sums, option `chain`, with the reason: against torch.sum's tree the kernel's two chains of 32 same-sign terms measured
4.67 x 2^-24 at B = 1, S = 64 and 4.36 at B = 3, S = 1000, the tree 0.9 and 0.75). No number here was taken from a kernel; _bound() prints
both figures of every check (pytest -s) and the last test prints the worst ratio per (form, output, family).

Measured on an MI355X: worst kernel / model ratio over every case of a (form, output, family), in brackets the largest kernel figure
in units of 2^-24 S; the bound is 4:
  register  logp     random 1.17 (2.28)  uniform 1.24 (1.24)  plateau 0.19 (0.19)  zero_tie 2.17 (2.17)  spike 0 (0)  offset 0.99 (0.99)
                     ladder 0.66 (0.66)  outside 0.82 (0.82)
            entropy  random 1.24 (2.53)  uniform 1.24 (1.24)  plateau 0.19 (0.19)  zero_tie 1.85 (2.30)  spike 0 (2.8e-58)  offset 1.82 (2.02)
                     ladder 0.48 (0.48)  outside 1.67 (1.67)
  wide      logp     random 1.14 (2.43)  uniform 1.24 (1.24)  plateau 0.19 (0.19)  zero_tie 2.27 (2.27)  spike 0 (0)  offset 1.14 (1.14)
                     ladder 0.66 (0.66)  outside 1.28 (1.28)
            entropy  random 1.11 (2.58)  uniform 1.24 (1.24)  plateau 0.19 (0.19)  zero_tie 2.14 (2.48)  spike 0 (9.5e-58)  offset 1.02 (1.97)
                     ladder 0.48 (0.48)  outside 1.58 (1.81)
  seq_scores (fraction of sum |term|)  plane 0 1.43 (3.7e-7)  plane 1 1.32 (3.2e-7)  plane 2 1.00 (3.2e-7)  plane 3 1.00 (2.5e-7)
No row family needed one of score_ref.OPTIONS (exp2, log2): the plain float32 model holds every case.
Narrow against wide: heads 1 .. 7 of 'switch' and of 'narrow_edges' are bit-equal in logp, entropy and rank on every row: the header's
"same arithmetic and summation order" holds on the device.

Scratch builds of csrc/pb_score.hip with one token changed (never committed), failing tests of the 43 of this file:
  * the register form's tie rule `c < tgt` made `c <= tgt`: 8 -- test_token_scores_layout and test_rank_zero_is_the_argmax_of_the_loss_kernel
    on narrow_edges, narrow_b and default, test_wide_form_gives_the_register_form_bits, the second-sweep test on narrow_b.
  * the select chain's `tk == k` made `tk == k + 1`: the same 8.
  * the dispatch `> 64 * SC_K` made `>= 64 * SC_K`: 0, and none can fail: the change sends a row whose largest head has exactly 320 classes
    to the wide form, which holds 320 classes as well and gives the register form's bits (test_wide_form_gives_the_register_form_bits): it
    picks between two kernels with equal results. The other direction, `> 64 * SC_K + 1` (a head of 321 classes in the register form,
    which drops class 320): 5 -- both layout tests on switch and sweep_wide, the second-sweep test on sweep_wide.
  * the wide form's `x[o + tgt]` made `x[o + (tgt & 63)]`: 8 -- both layout tests on switch, wide_edges and sweep_wide,
    test_wide_form_gives_the_register_form_bits, the second-sweep test on sweep_wide.
  * seq_scores' `s += 32` made `s += 64`: 13 -- test_seq_scores at S = 33, 64, 65, 1000 for B = 1, 3, 70 (S <= 32 is one trip either way)
    and test_engine_score_windows_overlap_bit_for_bit (count is no longer length - start).
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import score_ref as R

pytestmark = pytest.mark.gpu

E24 = 2.0 ** -24
MARGIN = 4.0
SENT = -31111
GUARD = 1.5 * 2.0 ** -20
F32, I16 = torch.float32, torch.int16
WHICH = {'all': (True, True), 'lp': (False, False), 'lp_en': (True, False), 'lp_rk': (False, True)}
RATIOS = {}                                                             # (form, output, family) -> [worst ratio, largest kernel figure]
_CASES = {}
_DUMMY = []


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from pianobart_amd import ops as o
    return o


# ---------------------------------------------------------------- helpers
def _galloc(shape, dtype, pad=16, init=None):
    """(buffer, view, pad): a view of `shape` inside a flat buffer with `pad` guard elements on both sides (the idiom of
    tests/test_row_kernels_gpu.py): the guards hold GUARD / SENT, the view starts as NaN (integers: SENT) unless `init` is given."""
    n = int(np.prod(shape))
    fl = dtype.is_floating_point
    buf = torch.full((n + 2 * pad,), GUARD if fl else SENT, dtype=dtype, device='cuda')
    view = buf[pad:pad + n].view(shape)
    if init is not None:
        view.fill_(init)
    elif fl:
        view.fill_(float('nan'))
    return buf, view, pad


def _gcheck(g, what, written=True):
    buf, view, pad = g
    n = view.numel()
    torch.cuda.synchronize()
    guards = torch.cat([buf[:pad], buf[pad + n:]])
    assert bool((guards == (GUARD if buf.dtype.is_floating_point else SENT)).all()), '%s: guard elements written' % what
    if not written:
        assert bool((torch.isnan(view) if view.dtype.is_floating_point else view == SENT).all()), '%s: written by a call that must not write' % what
    elif view.dtype.is_floating_point:
        assert bool(torch.isfinite(view).all()), '%s: not finite' % what
    else:
        assert bool((view != SENT).all()), '%s: not written' % what


def _gptr(g):
    """the address of the guarded view (a view of no elements has no data pointer of its own)."""
    return None if g is None else ctypes.c_void_p(g[0].data_ptr() + g[2] * g[0].element_size())


def _dp(t):
    """the address of an input tensor; a tensor of no elements gets a valid address that nothing may touch."""
    if t is None:
        return None
    if t.numel() == 0:
        if not _DUMMY:
            _DUMMY.append(torch.zeros(64, device='cuda'))
        t = _DUMMY[0]
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.view(torch.int32) if t.dtype == F32 else t


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _bound(what, kernel, model, floor=1.0, note=''):
    ref = max(model, floor)
    print('RATIO %-58s kernel %10.4g   float32 model %10.4g   ratio %6.3f %s' % (what, kernel, model, kernel / ref, note))
    assert kernel <= MARGIN * ref, '%s: kernel %.4g > %g x float32 model %.4g' % (what, kernel, MARGIN, ref)
    return kernel / ref


def _outs(T, which='all'):
    en, rk = WHICH[which]
    return dict(logp=_galloc((T, 8), F32), entropy=_galloc((T, 8), F32) if en else None, rank=_galloc((T, 8), I16) if rk else None)


def _launch(ops, x, tgt, mask, off, g, T=None, V=None, logp_null=False):
    ops.LIB.call('pb_token_scores', _dp(x), _dp(tgt), _dp(mask), ops.seg_array(off), None if logp_null else _gptr(g['logp']), _gptr(g['entropy']),
                 _gptr(g['rank']), x.shape[0] if T is None else T, x.shape[1] if V is None else V, _stream())


def _token(ops, x, tgt, mask, off, which='all'):
    """One call on device tensors: guarded outputs, the guards, the written region and the inputs checked. Returns {name: view}."""
    keep = [t.clone() for t in (x, tgt, mask)]
    g = _outs(x.shape[0], which)
    _launch(ops, x, tgt, mask, off, g)
    for name, v in g.items():
        if v is not None:
            _gcheck(v, '%s (%s)' % (name, which))
    for name, a, b in zip(('logits', 'target', 'mask'), keep, (x, tgt, mask)):
        assert _same(a, b), '%s changed by pb_token_scores' % name
    return {k: v[1] for k, v in g.items() if v is not None}


def _form(sizes):
    return 'wide' if max(sizes) > 320 else 'register'


def _case(name):
    """The rows of a layout (score_ref.make_case), their float64 reference and float32 model on the host, and device copies; once."""
    if name not in _CASES:
        c = R.make_case(R.LAYOUTS[name])
        c['ref'] = R.token_scores(c['x'].double(), c['target'], c['mask'], c['off'])
        c['model'] = R.token_scores(c['x'], c['target'], c['mask'], c['off'])
        c['model_dev'] = R.token_scores(c['x'], c['target'], c['mask'], c['off'], exp2=True, log2=True)      # printed only
        c['dev'] = (c['x'].cuda(), c['target'].cuda(), c['mask'].cuda())
        _CASES[name] = c
    return _CASES[name]


def _measure(tag, form, case, got, ref, model, model_dev=None):
    """the bound of the module docstring per (output, family) of a case; fills RATIOS."""
    k, m = R.worst_by_family(case, got, ref), R.worst_by_family(case, model, ref)
    d = R.worst_by_family(case, model_dev, ref) if model_dev is not None else {}
    assert set(k) == set(m)
    for key in sorted(k):
        r = _bound('%s %s %s' % (tag, key[0], key[1]), k[key], m[key], note='(model with exp2, log2: %.4g)' % d[key] if key in d else '')
        w = RATIOS.setdefault((form,) + key, [0.0, 0.0])
        w[0], w[1] = max(w[0], r), max(w[1], k[key])


# ---------------------------------------------------------------- pb_token_scores: every layout, every row family
@pytest.mark.parametrize('name', list(R.LAYOUTS))
def test_token_scores_layout(ops, name):
    """Every family block of score_ref.make_case on one layout, in one call per output set. Measured ratios: the module docstring."""
    c = _case(name)
    x, tgt, mask = c['dev']
    if name == 'default':
        assert c['sizes'] == list(ops.SEG_SIZES)
    runs = {w: _token(ops, x, tgt, mask, c['off'], w) for w in WHICH}
    full = runs['all']
    for w, out in runs.items():                                         # the four calls: equal bits in every output they share
        for k, v in out.items():
            assert _same(v, full[k]), '%s of the %s call differs from the call with all three outputs' % (k, w)
    got = {k: v.cpu() for k, v in full.items()}
    ref = c['ref']
    assert torch.equal(got['rank'].long(), ref['rank']), 'rank differs from float64 at (row, head) %s' % (got['rank'].long() != ref['rank']).nonzero()[:8].tolist()
    dead = c['mask'] == 0
    assert int(dead.sum()) == 3
    assert bool((got['logp'][dead] == 0).all()) and bool((got['entropy'][dead] == 0).all()) and bool((got['rank'][dead] == -1).all())
    live = ~dead[:, None].expand(-1, 8)
    z_en, z_lp = live & (ref['s_entropy'] == 0), live & (ref['s_logp'] == 0)
    assert int(z_lp.sum()) > 0 if 1 in c['sizes'] else int(z_en.sum()) == 0
    assert bool((got['entropy'][z_en] == 0).all()) and bool((got['logp'][z_lp] == 0).all())
    t = c['target'].long()
    inside = (t >= 0) & (t < torch.tensor(c['sizes'])[None])            # a zero of a one-class head at column 0 beats a target >= 1: rank 1
    assert bool((got['rank'][z_lp & inside] == 0).all())
    _measure(name, _form(c['sizes']), c, got, ref, c['model'], c['model_dev'])


@pytest.mark.parametrize('name', list(R.LAYOUTS))
def test_rank_zero_is_the_argmax_of_the_loss_kernel(ops, name):
    """rank == 0 exactly where pb_ce_fwd_bwd's argmax_out on the same logits is the target, on every live (row, head) whose target lies
    inside its head (the masked rows' NaN logits are zeroed for the loss kernel, which reads every row)."""
    c = _case(name)
    x, tgt, mask = c['dev']
    T, V = x.shape
    rank = _token(ops, x, tgt, mask, c['off'], 'lp_rk')['rank']
    sizes = torch.tensor(c['sizes'], device='cuda')[None]
    inside = (tgt >= 0) & (tgt < sizes) & (mask != 0)[:, None]
    am = _galloc((T, 8), I16)
    xs, ts, ms = torch.nan_to_num(x), torch.where(inside, tgt, torch.zeros_like(tgt)), torch.ones(T, 8, device='cuda')
    sums, ws = torch.zeros(24, device='cuda'), torch.empty(int(ops.LIB.query('pb_ce_partials_floats')), device='cuda')
    ops.LIB.call('pb_ce_fwd_bwd', _dp(xs), _dp(ts), _dp(ms), ops.seg_array(c['off']), _dp(sums), _dp(ws), None, None, _gptr(am), T, V, ops.PB_F32,
                 _stream())
    _gcheck(am, 'argmax')
    assert torch.equal((rank == 0)[inside], (am[1] == tgt)[inside])
    assert int((rank == 0)[inside].sum()) > 8 and int((rank != 0)[inside].sum()) > 8


def test_wide_form_gives_the_register_form_bits(ops):
    """'switch' (head 0 of 321 classes: the wide form for the whole row) against 'narrow_edges' (320: the register form) with the same
    logits and targets in heads 1 .. 7 and the same first 320 columns in head 0: heads 1 .. 7 are bit-equal in all three outputs -- the
    header's "same arithmetic and summation order"."""
    c = _case('switch')
    x, tgt, mask = c['dev']
    wide = _token(ops, x, tgt, mask, c['off'], 'all')
    xn = torch.cat([x[:, :320], x[:, 321:]], 1).contiguous()
    narrow = _token(ops, xn, tgt, mask, R.offsets(R.LAYOUTS['narrow_edges']), 'all')
    for k in ('logp', 'entropy', 'rank'):
        a, b = wide[k][:, 1:], narrow[k][:, 1:]
        diff = _bits(a.contiguous()) != _bits(b.contiguous())
        assert not bool(diff.any()), '%s: %d of %d elements of heads 1 .. 7 differ between the forms, first at %s' % (k, int(diff.sum()), diff.numel(), diff.nonzero()[:4].tolist())


@pytest.mark.parametrize('name', ['narrow_b', 'sweep_wide'])
def test_rows_are_independent_and_the_second_sweep(ops, name):
    """T = 4 x 4096 + 9: nine rows into the grid's second sweep. Rank against float64 and the bound of the module docstring on every row;
    rows 0, 16383, 16384, 16385, T - 1 again as a 5-row call, and the first 1, 3, 4, 5 rows as calls of their own (idle waves, a full
    workgroup, a second one): equal bits."""
    sizes = R.LAYOUTS[name]
    off = R.offsets(sizes)
    T = 4 * 4096 + 9
    g = torch.Generator(device='cuda').manual_seed(len(name))
    x = 2.0 * torch.randn(T, off[8], generator=g, device='cuda')
    tgt = torch.stack([torch.randint(0, n, (T,), generator=g, device='cuda') for n in sizes], 1)
    far = torch.rand(T, 8, generator=g, device='cuda') < 0.02           # some targets outside their head
    tgt = torch.where(far, torch.tensor([-1, 1088, 32767, -32768], device='cuda')[torch.randint(0, 4, (T, 8), generator=g, device='cuda')], tgt).to(I16)
    mask = (torch.rand(T, generator=g, device='cuda') < 0.9).float()
    rows = [0, 16383, 16384, 16385, T - 1]
    idx = torch.tensor(rows, device='cuda')
    mask[idx] = 1
    mask[5:7] = 0
    big = _token(ops, x, tgt, mask, off, 'all')
    case = dict(fam=['random'] * T)
    ref = R.token_scores(x.double(), tgt, mask, off)
    assert torch.equal(big['rank'].long(), ref['rank'])
    dead = mask == 0
    assert bool((big['logp'][dead] == 0).all()) and bool((big['entropy'][dead] == 0).all()) and bool((big['rank'][dead] == -1).all())
    _measure('%s T=%d' % (name, T), _form(sizes), case, big, ref, R.token_scores(x, tgt, mask, off))
    small = _token(ops, x[idx].contiguous(), tgt[idx].contiguous(), mask[idx].contiguous(), off, 'all')
    for k in ('logp', 'entropy', 'rank'):
        assert _same(small[k], big[k][idx].contiguous()), '%s of rows %s depends on T' % (k, rows)
    for t in (1, 3, 4, 5):
        part = _token(ops, x[:t].contiguous(), tgt[:t].contiguous(), mask[:t].contiguous(), off, 'all')
        for k in ('logp', 'entropy', 'rank'):
            assert _same(part[k], big[k][:t].contiguous()), '%s at T = %d' % (k, t)


def test_token_scores_empty_and_refused_calls(ops):
    """T = 0 succeeds and writes nothing. seg_off[8] != V, seg_off[0] != 0, a head of 0 classes, a head of 1089 and logp = NULL raise
    PBError naming pb_token_scores and write nothing."""
    good = R.offsets([1032] + [8] * 7)                                  # V = 1088
    V = good[8]
    T = 3
    tgt, mask = torch.zeros(T, 8, dtype=I16, device='cuda'), torch.ones(T, device='cuda')
    xw = torch.zeros(T, V + 57, device='cuda')                          # wide enough for every V below
    g = _outs(T)
    _launch(ops, xw[:0], tgt[:0], mask[:0], good, g, T=0, V=V)
    for name, v in g.items():
        _gcheck(v, name + ' (T = 0)', written=False)
    refused = {'seg_off[8] != V': dict(off=good, V=V + 1), 'seg_off[0] != 0': dict(off=[1] + good[1:], V=V),
               'a head of 0 classes': dict(off=good[:3] + [good[2]] + good[4:], V=V),
               'a head of 1089 classes': dict(off=[0] + [o + 57 for o in good[1:]], V=V + 57), 'logp NULL': dict(off=good, V=V, logp_null=True)}
    assert refused['a head of 1089 classes']['off'][1] == 1089 and refused['a head of 0 classes']['off'][2] == refused['a head of 0 classes']['off'][3]
    for what, kw in refused.items():
        g = _outs(T)
        with pytest.raises(ops.PBError, match='pb_token_scores'):
            _launch(ops, xw, tgt, mask, kw['off'], g, T=T, V=kw['V'], logp_null=kw.get('logp_null', False))
        for name, v in g.items():
            _gcheck(v, '%s (%s)' % (name, what), written=False)
    g = _outs(T)                                                        # and the accepted layout next to them runs
    _launch(ops, xw[:, :V].contiguous(), tgt, mask, good, g, T=T, V=V)
    for name, v in g.items():
        _gcheck(v, name)


# ---------------------------------------------------------------- pb_seq_scores
def _seq(ops, lp, en, rk, m, B, S):
    out = _galloc((B, 4, 8), F32)
    ops.LIB.call('pb_seq_scores', _dp(lp), _dp(en), _dp(rk), _dp(m), _gptr(out), B, S, _stream())
    _gcheck(out, 'out', written=B > 0)
    return out[1]


def _plane_err(out, want, absum):
    """per plane, max over (sequence, head) of |out - want| / sum |term|; 0 where there is no term."""
    err = (out.double() - want).abs() / absum.clamp_min(1e-300)
    return [float(err[:, p].max()) if err.numel() else 0.0 for p in range(4)]


@pytest.mark.parametrize('B', [1, 3, 70])
@pytest.mark.parametrize('S', [0, 1, 31, 32, 33, 64, 65, 1000])
def test_seq_scores(ops, B, S):
    """One workgroup per sequence, 32 positions per trip of its loop: S on both sides of one and two trips, none at all, and 1000.
    exact    logp and entropy small integers (|v| <= 8), rank in {0, 1, 5}, weights in {0, 1, 2, 0.5}: every partial sum is exact in
             float32 and all four planes EQUAL the float64 sums; NaN / inf and another rank under the zeros of the mask change no bit;
             entropy = rank = NULL leave planes 1 and 2 exactly 0 in an `out` prefilled with NaN, planes 0 and 3 as before.
    random   float inputs, weights in (0, 2]: the bound of the module docstring per plane; two launches give equal bytes."""
    g = torch.Generator(device='cuda').manual_seed(1000 * B + S)
    ri = lambda lo, hi, *s: torch.randint(lo, hi, s, generator=g, device='cuda')
    lp, en = ri(-8, 9, B * S, 8).float(), ri(-8, 9, B * S, 8).float()
    rk = torch.tensor([0, 1, 5], device='cuda')[ri(0, 3, B * S, 8)].to(I16)
    m = torch.tensor([0.0, 1.0, 2.0, 0.5], device='cuda')[ri(0, 4, B, S)]
    want, _ = R.seq_sums(lp.double(), en.double(), rk, m.double())
    out = _seq(ops, lp, en, rk, m, B, S)
    assert torch.equal(out.double(), want), 'planes %s differ from the exact sums' % sorted(set((out.double() != want).nonzero()[:, 1].tolist()))
    off = (m.view(-1) == 0)[:, None].expand(-1, 8)
    alt = (torch.arange(B * S * 8, device='cuda').view(B * S, 8) % 3)
    bad = torch.tensor([float('nan'), float('inf'), -float('inf')], device='cuda')[alt]
    out2 = _seq(ops, torch.where(off, bad, lp), torch.where(off, bad.roll(1, 0), en), torch.where(off, (alt % 2 * 7).to(I16), rk), m, B, S)
    assert _same(out2, out), 'a masked position changed the sums'
    nul = _seq(ops, lp, None, None, m, B, S)
    assert bool((nul[:, 1:3] == 0).all()) and _same(nul[:, 0].contiguous(), out[:, 0].contiguous()) and _same(nul[:, 3].contiguous(), out[:, 3].contiguous())
    # random floats
    lp, en = -3.0 * torch.randn(B * S, 8, generator=g, device='cuda').abs(), 2.0 * torch.randn(B * S, 8, generator=g, device='cuda').abs()
    rk = ri(0, 3, B * S, 8).to(I16)
    m = 2.0 * (1.0 - torch.rand(B, S, generator=g, device='cuda'))
    assert S == 0 or (float(m.min()) > 0 and float(m.max()) <= 2)
    want, absum = R.seq_sums(lp.double(), en.double(), rk, m.double())
    model, _ = R.seq_sums(lp, en, rk, m, chain=True)                    # the header's order of summation: score_ref.seq_sums says why
    tree = _plane_err(R.seq_sums(lp, en, rk, m)[0], want, absum)        # printed only
    out = _seq(ops, lp, en, rk, m, B, S)
    assert _same(out, _seq(ops, lp, en, rk, m, B, S)), 'two launches differ'
    for p, (k, f) in enumerate(zip(_plane_err(out, want, absum), _plane_err(model, want, absum))):
        r = _bound('seq_scores B=%d S=%d plane %d' % (B, S, p), k, f, floor=E24, note='(torch.sum: %.4g)' % tree[p])
        w = RATIOS.setdefault(('seq_scores', 'plane %d' % p, 'random'), [0.0, 0.0])
        w[0], w[1] = max(w[0], r), max(w[1], k)
    if S == 0:
        assert bool((out == 0).all())


def test_seq_scores_without_sequences_writes_nothing(ops):
    z = torch.zeros(8, 8, device='cuda')
    _seq(ops, z, z, z.to(I16), torch.ones(1, 8, device='cuda'), 0, 8)


# ---------------------------------------------------------------- Engine.score
def test_engine_score_windows_overlap_bit_for_bit(ops):
    """The three pieces of tests/test_score_gpu.py's small bf16 model scored with (start, length) = (0, L), (5, L), (L - 1, L), (L, L)
    per row: the runs share `length`, so the decoder mask and the logits, and every position scored in two runs is bit-equal in both;
    an unscored position is exactly 0 / 0 / -1, count is length - start, a row with start == length has four sums of exactly 0. And the
    same with row 0 at (0, 0)."""
    from pianobart_amd.scoring import default_length
    from tests.test_score_gpu import _small
    c = _small('bf16')
    m, enc, emask, piece = c['m'], c['enc'], c['emask'], c['piece']
    B, S = piece.shape[:2]
    L = default_length(piece, 256)
    assert all(5 < n <= S for n in L)
    pos = torch.arange(S, device='cuda')[None]
    runs = {}
    for tag, start, length in (('0', [0] * B, L), ('5', [5] * B, L), ('L-1', [n - 1 for n in L], L), ('L', list(L), L), ('row 0 empty', [0] * B, [0] + L[1:])):
        r = m.score(enc, piece, emask, start=start, length=length, device_num=0)
        st, ln = torch.tensor(start, device='cuda')[:, None], torch.tensor(length, device='cuda')[:, None]
        on = (pos >= st) & (pos < ln)
        assert bool((r.logp[~on] == 0).all()) and bool((r.entropy[~on] == 0).all()) and bool((r.rank[~on] == -1).all()), tag
        assert bool((r.rank[on] >= 0).all()) and bool(torch.isfinite(r.logp).all()) and bool(torch.isfinite(r.entropy).all()), tag
        assert r.count.tolist() == [float(n - s) for s, n in zip(start, length)], tag
        for b in range(B):
            if start[b] == length[b]:
                for k in ('sum_logp', 'sum_entropy', 'hits'):
                    assert bool((getattr(r, k)[b] == 0).all()), (tag, k)
                assert float(r.count[b]) == 0
        runs[tag] = (r, on, length)
    tags = list(runs)
    for i, a in enumerate(tags):
        for b in tags[i + 1:]:
            (ra, ona, la), (rb, onb, lb) = runs[a], runs[b]
            both = ona & onb & torch.tensor([x == y for x, y in zip(la, lb)], device='cuda')[:, None]       # rows whose length the two runs share
            if a != 'row 0 empty' and b != 'row 0 empty':
                assert int(both.sum()) == int(onb.sum())                # the later window lies inside the earlier one
            for k in ('logp', 'entropy', 'rank'):
                assert _same(getattr(ra, k)[both], getattr(rb, k)[both]), '%s differs between the runs %s and %s' % (k, a, b)


# ---------------------------------------------------------------- the figures of the module docstring
def test_zz_print_the_worst_ratios():
    """Prints the worst kernel / model ratio (and the largest kernel figure) per (form, output, family) over the tests above."""
    for key in sorted(RATIOS):
        print('WORST %-10s %-8s %-9s ratio %6.3f   largest kernel figure %.4g' % (key + tuple(RATIOS[key])))
    assert all(v[0] <= MARGIN for v in RATIOS.values())
