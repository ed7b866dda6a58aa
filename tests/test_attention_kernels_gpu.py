"""GPU: the attention kernels behind pb_attn_fwd / pb_attn_bwd (csrc/pb_flash.hip, pb_flash64.hip, pb_flash1.hip, pb_flash_x3.hip) at every
tile and mask edge, against the float64 reference of tests/attn_ref.py (checked against float64 autograd in tests/test_attn_ref_cpu.py).

The measure, the same for a kernel and for the storage model (attn_ref.figure), per element and over ALL elements of an output:
    (|got - truth| - ulp) / (2^-9 S),   ulp = 2^-8 |truth| for a bf16-stored result, 0 for f32
with S the cancellation-free sum of the term magnitudes of the element's contraction (attn_ref.scales: o: p @ |v|, dv: p^T @ |dO|,
dq: scale a @ |k|, dk: scale a^T @ |q| with a = p (|dP| + sum |dO O|), delta: sum |dO O|, lse: the largest scale |q|.|k| of a visible key,
dbias_*: the column sums of these). An element with S == 0 must be exactly 0, one whose truth is +inf exactly +inf. A kernel's figure may
reach MARGIN = 4 times the figure of the storage model of its family (attn_ref.MODELS, float32 arithmetic with the roundings the ABI and
the kernels' header comments state) at the same shape and inputs, computed in the test: the factor of tests/test_row_kernels_gpu.py, for
the same reason -- another summation order (tile-wise online softmax, per-wave chains) over the same roundings. No figure here was taken
from a kernel's own error. One floor: a model figure below one float32 ulp of S (2^-24 S = 2^-15 in these units) counts as that ulp
(_bound). It acts only where no bf16 rounding does -- one query per (batch, head) or a single visible key, where the model's p is 1 and its
dP - delta cancels to a few float32 bits or to none, so that its figure is 0 or the luck of its summation order; the kernels reach 1.3 ulp
there. _bound() prints both figures of every check and test_zz_worst_ratios the worst per family (pytest -s).

Without a tolerance, in every case: every output (o, lse, delta, dq, dk, dv, dbias_*, the dbias workspace) is a view inside a larger
allocation whose guard rows / elements on both sides hold a small finite sentinel and whose inside starts as NaN; q / k / v / dO and the
gradients sit beside neighbour columns (the qkv layout where Sq == Sk, else q beside a neighbour and K, V as one layer of a stacked K | V
projection). After the calls the guards and neighbour columns are untouched, the input buffers unchanged, everything written is finite
(lse: finite or +inf). Rows without a visible key (a whole batch row with kmax == 0 among them): o == 0, lse == +inf, dq == 0; keys no
query sees: dk == dv == 0. Batch and head independence: one (batch, head) pair of the B = 3, H = 3 call equals, torch.equal, the same data
run as B = 1, H = 1, in o, lse, dq, dk, dv -- for every family, the one-pass backward included: none had to be held to the bound instead.

Cases (B = 3, H = 3):
  test_every_tile_edge   the 13 (Sq, Sk) of SHAPES x causal x every family and head_dim of FAMILIES, keys masked at random plus a masked tail
  test_every_mask_edge   Sq 129, Sk 193: no mask, holes, first key tile wholly masked, only key Sk - 1 (alone in a partial tile) / only key 0
                         visible, tails cut at 0 (one batch row), 1, 63, 64, 65, a fully masked batch row; with and without kmax, causal or not
  test_lazy_reference_maximum   the pipelined forward's lazy maximum (LAZY_THR = 8 log2 units): scores rising / falling 9.5 log2 units per
                         key tile, stepping by 7.6 / 8.4, randn * 4, all about -100; nine key tiles; every backward behind it
  test_packed_rows       SHAPES x causal for the pipelined, one-pass and split-bf16 families: three batches of different q_len, k_len, k_vis
The head_dim 64 pipelined cases run the one-pass backward behind the same forward; the pipelined and one-pass cases accumulate dbias_q / k / v
onto 0.25. Not run, because the header refuses them: PB_ATTN_GENERIC with head_dim 96 or packed rows; dbias_* and the one-pass backward
outside the pipelined head dims; packed rows at head_dim 32 in bf16. The generic kernels do not read kmax: their mask cases run without.

Measured on an MI355X, worst kernel / model ratio over every case of a family (in brackets the largest kernel figure); the bound is 4:
  generic (32, 64g, 128g)  o 1.02 (1.4)  lse 1.74 (6.5e-5)  delta 1.63 (1.7)  dq 1.27 (0.78)  dk 1.61 (1.3)  dv 1.00 (1.8)
  pipelined (64, 96, 128)  o 1.28 (5.5)  lse 1.15 (0.57)  delta 1.48 (2.5)  dq 1.45 (1.7)  dk 1.67 (4.6)  dv 1.21 (9.1)
                           dbias_q 1.31 (0.35)  dbias_k 1.28 (0.49)  dbias_v 1.18 (6.0)
      lazy-maximum inputs  o 1.04 (50)  lse 1.16 (0.62)  delta 1.12 (8.7)  dq 1.20 (17)  dk 1.19 (53)  dv 1.05 (104)  dbias_q/k/v 1.39 / 1.13 / 1.35
      packed rows          o 1.37 (6.2)  lse 1.12 (0.65)  delta 1.70 (2.5)  dq 1.33 (1.9)  dk 1.30 (4.2)  dv 1.34 (10)  dbias_q/k/v 1.21 / 1.43 / 1.21
  one-pass backward (64)   delta 1.30 (2.5)  dq 1.45 (2.6)  dk 1.67 (3.7)  dv 1.21 (9.1)  dbias_q/k/v 1.52 / 1.26 / 1.18
      lazy-maximum inputs  delta 1.01 (7.3)  dq 1.00 (33)  dk 1.07 (53)  dv 1.00 (104)  dbias_q/k/v 1.08 / 1.10 / 1.10
      packed rows          delta 1.09 (2.5)  dq 1.61 (3.9)  dk 1.19 (4.1)  dv 1.34 (9.0)  dbias_q/k/v 1.19 / 1.02 / 1.16
  PB_F32X3 (32, 64, 128)   o 1.28 (0.023)  lse 1.09 (0.0032)  delta 1.29 (0.017)  dq 1.36 (0.0090)  dk 1.38 (0.018)  dv 1.29 (0.026)
      packed rows          o 1.38 (0.021)  lse 1.08 (0.0027)  delta 1.24 (0.0098)  dq 1.54 (0.0095)  dk 1.46 (0.018)  dv 1.13 (0.035)
  checks whose model figure is below one float32 ulp of S: kernel at most 1.29 ulp (generic), 1.22 (pipelined), 0.90 (one-pass), 0 (PB_F32X3)
The large dk / dv figures of the pipelined family (and its figures with one visible key, where the first model, with p = 1, had 0) are the
dK / dV kernels' documented K prescale: their p = exp2(q . bf16(c k) - lse) meets an lse made from bf16(c q) . k, so p is off by
2^-9 |score| and not normalised; attn_ref's `kv_prescale` states it, and the model then has the same figures (ratios 1.0 - 1.2).
A scratch build whose pipelined forward runs its key loop one tile short (nt - 1) fails 69 of the 78 pipelined test_every_tile_edge cases,
one whose causal compare there is >= for > fails 36 of their 39 causal cases and no other.
"""
import pytest
import torch

from tests import attn_ref as A

pytestmark = pytest.mark.gpu

MARGIN = 4.0
GUARD = 1.5 * 2.0 ** -20                       # small, finite, exact in bf16: a stray store changes it and so does a stray read-modify-write
F32_ULP = 2.0 ** -15                           # one float32 ulp (2^-24 S) in units of the figure (2^-9 S)
PAD = 2                                        # guard rows on both sides of every (rows, width) buffer
B3, H3 = 3, 3
F32, BF16 = torch.float32, torch.bfloat16

# (Sq, Sk): 1, 2, NS, NS + 1 and more 64-key tiles for both ring depths (NS = 3 at head_dim 64, 2 at 96 / 128), both sides of the one-pass
# 256-key block and of the 64- / 128-key dK / dV blocks, both sides of the 64-row chunk and the 128-query block, Sq != Sk in most
SHAPES = [(1, 1), (1, 257), (63, 65), (64, 64), (65, 63), (127, 129), (128, 128), (129, 193), (257, 1), (130, 513), (200, 255), (200, 256), (65, 257)]
# family, head_dim. 'generic' at 64 / 128 runs with PB_ATTN_GENERIC; 'pipe' at 64 also runs the one-pass backward behind the same forward
FAMILIES = [('generic', 32), ('generic', 64), ('generic', 128), ('pipe', 64), ('pipe', 96), ('pipe', 128), ('x3', 32), ('x3', 64), ('x3', 128)]
MODEL = {'generic': 'bf16', 'pipe': 'prescale', 'x3': 'x3'}
MASKS = ['none', 'holes', 'first_tile', 'last_only', 'first_only', 'tail0', 'tail1', 'tail63', 'tail64', 'tail65', 'row_masked']
WORST = {}                                     # (family, output) -> [worst kernel / model ratio, largest kernel figure]


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from pianobart_amd import ops as o
    return o


# ---------------------------------------------------------------- helpers
def _gen(seed):
    return torch.Generator(device='cuda').manual_seed(seed)


def _galloc(shape, dtype, pad=8, init=None):
    """(buffer, view, pad): a view of `shape` inside a flat buffer with `pad` guard elements on both sides (test_row_kernels_gpu._galloc):
    the guards hold GUARD, the view starts as NaN unless `init` is given."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * pad,), GUARD, dtype=dtype, device='cuda')
    view = buf[pad:pad + n].view(shape)
    view.fill_(float('nan') if init is None else init)
    return buf, view, pad


def _gcheck(g, what, finite=None):
    """guards untouched; the view (or the part `finite` of it; False: not looked at) finite."""
    buf, view, pad = g
    n = view.numel()
    assert bool((torch.cat([buf[:pad], buf[pad + n:]]) == GUARD).all()), '%s: guard elements written' % what
    if finite is not False:
        assert bool(torch.isfinite(view if finite is None else finite).all()), '%s: not finite' % what


class Wide:
    """A (PAD + rows + PAD, width) buffer: `rows` rows of `width` columns between two blocks of guard rows. As an output it holds GUARD
    everywhere except the named column spans of the inside rows, which start as NaN; as an input it holds random data everywhere."""

    def __init__(self, rows, width, dtype, spans, gen=None, amp=1.0):
        self.rows, self.width, self.spans = rows, width, spans           # spans: name -> (first column, columns)
        if gen is None:
            self.buf = torch.full((rows + 2 * PAD, width), GUARD, dtype=dtype, device='cuda')
            for c0, n in spans.values():
                self.buf[PAD:PAD + rows, c0:c0 + n] = float('nan')
        else:
            self.buf = (torch.randn(rows + 2 * PAD, width, device='cuda', generator=gen) * amp).to(dtype)
        self.before = None

    def loc(self, name, S=None):
        """(tensor, element offset, row stride[, batch stride]) of a span, as pianobart_amd.ops takes operands."""
        t = (self.buf, PAD * self.width + self.spans[name][0], self.width)
        return t if S is None else t + (S * self.width,)

    def span(self, name):
        c0, n = self.spans[name]
        return self.buf[PAD:PAD + self.rows, c0:c0 + n]

    def put(self, name, rows2d):
        self.span(name).copy_(rows2d)

    def freeze(self):
        self.before = self.buf.clone()

    def check_input(self, what):
        assert torch.equal(self.buf, self.before), '%s: an input buffer was written' % what

    def check_output(self, what):
        """guard rows and neighbour columns untouched; the spans finite."""
        g = self.buf.clone()
        for name, (c0, n) in self.spans.items():
            inside = g[PAD:PAD + self.rows, c0:c0 + n]
            assert bool(torch.isfinite(inside).all()), '%s %s: not finite' % (what, name)
            inside.fill_(GUARD)
        assert bool((g == GUARD).all()), '%s: guard rows or neighbour columns written' % what


def _rows2d(x4):
    """(B, H, S, hd) -> (B * S, H * hd), the projection layout."""
    Bn, Hn, S, hd = x4.shape
    return x4.permute(0, 2, 1, 3).reshape(Bn * S, Hn * hd)


def _x4(rows2d, Bn, Hn, S, hd):
    return rows2d.reshape(Bn, S, Hn, hd).permute(0, 2, 1, 3)


def _key_mask(kind, Bn, Sk, gen):
    """(Bn, Sk) float key mask, or None."""
    if kind == 'none':
        return None
    km = torch.ones(Bn, Sk, device='cuda')
    if kind in ('holes', 'row_masked'):
        km = (torch.rand(Bn, Sk, device='cuda', generator=gen) > 0.25).float()
        km[0, 0] = 0                                                     # causal: query 0 of batch 0 sees nothing
        km[1 % Bn, Sk // 2:] = 0                                         # a masked tail
        if kind == 'row_masked':
            km[Bn - 1] = 0                                               # one batch row without a visible key
    elif kind == 'first_tile':
        km[:, :64] = 0                                                   # every row meets its first visible key in a later tile
    elif kind == 'last_only':
        km[:] = 0
        km[:, Sk - 1] = 1
    elif kind == 'first_only':
        km[:] = 0
        km[:, 0] = 1
    elif kind == 'tail0':
        km[1 % Bn] = 0                                                   # kmax == 0 for one batch row
    else:
        km[:, int(kind[4:]):] = 0                                        # tail1, tail63, tail64, tail65
    return km


def _bound(over, what, fam, name, kernel, model):
    """Prints both figures and notes in `over` a kernel figure above MARGIN x the model's (the case asserts once, so that -s shows every
    output of a failing case). A model figure below F32_ULP -- one float32 ulp of S, 2^-24 S, in units of the figure -- counts as F32_ULP:
    where no bf16 rounding acts (rows with a single visible key: p = 1, and dP - delta cancels to a few float32 bits or to none) the
    model's figure is 0 or the luck of its own summation order, and no float32 accumulation can be held below the format's resolution.
    That is the precision of the number format (0.003 % of the bf16 figures), not a number taken from any kernel; such checks are kept out
    of the worst ratios."""
    ratio = kernel / model if model > 0 else (0.0 if kernel == 0 else float('inf'))
    print('RATIO %-60s %-16s %-8s kernel %10.4g   model %10.4g   ratio %6.3f' % (what, fam, name, kernel, model, ratio))
    if model >= F32_ULP:
        w = WORST.setdefault((fam, name), [0.0, 0.0])
        w[0], w[1] = max(w[0], ratio), max(w[1], kernel)
    else:
        w = WORST.setdefault((fam, 'below one float32 ulp'), [0.0, 0.0])
        w[0], w[1] = max(w[0], kernel / F32_ULP), max(w[1], kernel)
    if not kernel <= MARGIN * max(model, F32_ULP):
        over.append('%s: kernel %.4g > %g x model %.4g' % (name, kernel, MARGIN, model))


# ---------------------------------------------------------------- one call of a family, every output inside guards
def _run(ops, fam, q4, k4, v4, do4, scale, causal, km=None, use_kmax=False, one_pass=False, dbias=False, packed=None, tag=''):
    """Forward and backward of `fam` on (Bn, Hn, S, hd) operands in the storage dtype. Dense: q / k / v in one qkv buffer where Sq == Sk, else
    q beside a neighbour and k, v as layer 1 of three stacked K | V projections; the gradients in buffers of the same layouts; o and dO
    beside a neighbour. packed = (q_len, k_len, k_vis) lists: the operands are padded to the maxima and only batch b's first q_len[b] /
    k_len[b] rows exist in the buffers, back to back. Returns the outputs as (Bn, Hn, S, hd) / (Bn, Hn, Sq) tensors (packed: rows of no
    batch are 0, their lse +inf) after checking every guard, neighbour column, input buffer and that all that is written is finite."""
    from pianobart_amd._lib import LIB
    Bn, Hn, Sq, hd = q4.shape
    Sk = k4.shape[2]
    d, dt = Hn * hd, q4.dtype
    x3 = fam == 'x3'
    g = _gen(17)
    if packed is None:
        Tq, Tk = Bn * Sq, Bn * Sk
        vq = vk = None
    else:
        q_len, k_len, k_vis = packed
        Tq, Tk = sum(q_len), sum(k_len)
        vq = (torch.arange(Sq, device='cuda')[None, :] < torch.tensor(q_len, device='cuda')[:, None]).reshape(-1)     # rows of the padded (Bn * Sq) that exist
        vk = (torch.arange(Sk, device='cuda')[None, :] < torch.tensor(k_len, device='cuda')[:, None]).reshape(-1)
    pick = lambda x2, valid: x2 if valid is None else x2[valid]
    if Sq == Sk and packed is None:
        inq = ink = Wide(Tq, 3 * d, dt, dict(q=(0, d), k=(d, d), v=(2 * d, d)), g, 1.5)
        gq = gk = Wide(Tq, 3 * d, dt, dict(dq=(0, d), dk=(d, d), dv=(2 * d, d)))
    else:
        inq = Wide(Tq, 2 * d, dt, dict(q=(d, d)), g, 1.5)
        ink = Wide(Tk, 6 * d, dt, dict(k=(2 * d, d), v=(3 * d, d)), g, 1.5)
        gq = Wide(Tq, 2 * d, dt, dict(dq=(d, d)))
        gk = Wide(Tk, 6 * d, dt, dict(dk=(2 * d, d), dv=(3 * d, d)))
    ino = Wide(Tq, 2 * d, dt, dict(dout=(d, d)), g, 1.0)
    out = Wide(Tq, 2 * d, dt, dict(o=(d, d)))
    inq.put('q', pick(_rows2d(q4), vq))
    ink.put('k', pick(_rows2d(k4), vk))
    ink.put('v', pick(_rows2d(v4), vk))
    ino.put('dout', pick(_rows2d(do4), vq))
    for w in (inq, ink, ino):
        w.freeze()
    lse = _galloc((Bn, Hn, Sq), F32)
    kmax = None
    if use_kmax:
        kmax = torch.full((Bn,), Sk, dtype=torch.int32, device='cuda')
        if km is not None:
            ops.key_extent(km, kmax)
            assert kmax.tolist() == [int(km[b].nonzero().max()) + 1 if bool(km[b].any()) else 0 for b in range(Bn)]
    S_ = (lambda s: s) if packed is None else (lambda s: None)
    ql, kl, vl, ol = inq.loc('q', S_(Sq)), ink.loc('k', S_(Sk)), ink.loc('v', S_(Sk)), out.loc('o', S_(Sq))
    rows = None
    if packed is not None:
        i32 = lambda x: torch.tensor(x, dtype=torch.int32, device='cuda')
        off = lambda ln: [sum(ln[:b]) for b in range(Bn)]
        rows = ops.PackedRows(i32(off(q_len)), i32(q_len), i32(off(k_len)), i32(k_len), i32(k_vis), Sq, Sk, 'dec' if causal else 'enc')
        if x3:
            ops.flash_fwd_x3_packed(ql, kl, vl, ol, lse[1], rows, Bn, Hn, hd, scale, causal)
        else:
            ops.flash_fwd_packed(ql, kl, vl, ol, lse[1], rows, Bn, Hn, hd, scale, causal)
    elif x3:
        ops.flash_fwd_x3(ql, kl, vl, ol, lse[1], km, Bn, Hn, Sq, Sk, hd, scale, causal, kmax=kmax)
    else:
        ops.flash_fwd(ql, kl, vl, ol, lse[1], km, Bn, Hn, Sq, Sk, hd, scale, causal, force_generic=fam == 'generic' and hd != 32, kmax=kmax)
    torch.cuda.synchronize()
    out.check_output(tag + ' forward')
    vq3 = None if vq is None else vq.reshape(Bn, 1, Sq).expand(Bn, Hn, Sq)
    _gcheck(lse, tag + ' lse', finite=False)                            # the guards; lse itself: finite or +inf, never NaN or -inf
    lw = lse[1] if vq3 is None else lse[1][vq3]
    assert not bool(torch.isnan(lw).any()) and not bool((lw == float('-inf')).any()), tag + ' lse: NaN or -inf'
    out.freeze()                                                         # o is an input of the backward

    def unpad(w, name, valid, S):
        x = w.span(name)
        if valid is not None:
            full = torch.zeros(Bn * S, d, dtype=dt, device='cuda')
            full[valid] = x
            x = full
        return _x4(x, Bn, Hn, S, hd).clone()

    def lse_like(gl):
        return (gl[1] if vq3 is None else torch.where(vq3, gl[1], torch.full_like(gl[1], float('inf')))).clone()

    def delta_like(gl):
        return (gl[1] if vq3 is None else torch.where(vq3, gl[1], torch.zeros_like(gl[1]))).clone()

    res = dict(o=unpad(out, 'o', vq, Sq), lse=lse_like(lse))
    dol = ino.span('dout')                                               # a view: dO has o's strides, its pointer is the view's first element
    for one in ((False, True) if one_pass else (False,)):
        if one:
            assert LIB.query('pb_flash_bwd1_supported', Sq, Sk, hd, Tq, Hn) == 1
            if gq is gk:
                gq = gk = Wide(Tq, 3 * d, dt, dict(dq=(0, d), dk=(d, d), dv=(2 * d, d)))
            else:
                gq = Wide(Tq, 2 * d, dt, dict(dq=(d, d)))
                gk = Wide(Tk, 6 * d, dt, dict(dk=(2 * d, d), dv=(3 * d, d)))
        delta = _galloc((Bn, Hn, Sq), F32)
        db = dbws = None
        if dbias:
            db = [_galloc((d,), F32, init=0.25) for _ in range(3)]
            dbws = _galloc((int(LIB.query('pb_flash_bias_ws_floats', Bn, Hn, Sq, Sk, hd)),), F32)
        kw = dict(dbias=[x[1] for x in db], dbias_ws=dbws[1]) if dbias else {}
        dql, dkl, dvl = gq.loc('dq', S_(Sq)), gk.loc('dk', S_(Sk)), gk.loc('dv', S_(Sk))
        if packed is not None:
            args = (ql, kl, vl, ol, dol, lse[1], dql, dkl, dvl, delta[1], rows, Bn, Hn, hd, scale, causal)
            if x3:
                ops.flash_bwd_x3_packed(*args)
            elif one:
                ops.flash_bwd1_packed(*args, Tq, **kw)
            else:
                ops.flash_bwd_packed(*args, **kw)
        else:
            args = (ql, kl, vl, ol, dol, lse[1], km, dql, dkl, dvl, delta[1], Bn, Hn, Sq, Sk, hd, scale, causal)
            if x3:
                ops.flash_bwd_x3(*args, kmax=kmax)
            elif one:
                ops.flash_bwd1(*args, kmax=kmax, **kw)
            else:
                ops.flash_bwd(*args, force_generic=fam == 'generic' and hd != 32, kmax=kmax, **kw)
        torch.cuda.synchronize()
        t = tag + (' one-pass backward' if one else ' backward')
        gq.check_output(t)
        if gk is not gq:
            gk.check_output(t)
        _gcheck(delta, t + ' delta', finite=None if vq3 is None else delta[1][vq3])
        sfx = '1' if one else ''
        res.update({'dq' + sfx: unpad(gq, 'dq', vq, Sq), 'dk' + sfx: unpad(gk, 'dk', vk, Sk), 'dv' + sfx: unpad(gk, 'dv', vk, Sk), 'delta' + sfx: delta_like(delta)})
        if dbias:
            for x, n in zip(db, 'qkv'):
                _gcheck(x, t + ' dbias_' + n)
                res['dbias_' + n + sfx] = x[1] - 0.25
            assert bool((torch.cat([dbws[0][:dbws[2]], dbws[0][dbws[2] + dbws[1].numel():]]) == GUARD).all()), t + ': dbias_ws guard elements written'
    for w, n in ((inq, 'q'), (ink, 'k / v'), (ino, 'dO'), (out, 'o')):
        w.check_input(tag + ' ' + n)
    return res


def _case(ops, fam, hd, Sq, Sk, causal, mask, use_kmax, seed, qk=None, packed=None, tag=''):
    """One case: run the family at B = 3, H = 3, hold every output to MARGIN x the model's figure against the float64 truth, assert the
    exact zeros, and (dense) run one (batch, head) pair again as B = 1, H = 1: bit-identical."""
    Bn, Hn = B3, H3
    dt = F32 if fam == 'x3' else BF16
    scale = hd ** -0.5
    g = _gen(seed)
    if qk is None:
        q4 = (torch.randn(Bn, Hn, Sq, hd, device='cuda', generator=g) * 1.5).to(dt)
        k4 = (torch.randn(Bn, Hn, Sk, hd, device='cuda', generator=g) * 1.5).to(dt)
    else:
        q4, k4 = (x.to(dt) for x in A.lazy_inputs(qk, Bn, Hn, Sq, Sk, hd, scale, g, 'cuda'))
    v4 = (torch.randn(Bn, Hn, Sk, hd, device='cuda', generator=g) * 1.5).to(dt)
    do4 = torch.randn(Bn, Hn, Sq, hd, device='cuda', generator=g).to(dt)
    km = _key_mask(mask, Bn, Sk, g)
    pipe64 = fam == 'pipe' and hd == 64
    if packed is None:
        vis = A.visible(Bn, Sq, Sk, 'cuda', km, causal)
    else:
        q_len, k_len, k_vis = packed
        vis = A.visible(Bn, Sq, Sk, 'cuda', None, causal, kmax=k_vis) & (torch.arange(Sq, device='cuda')[None, :] < torch.tensor(q_len, device='cuda')[:, None])[:, None, :, None]
        for x4, ln in ((q4, q_len), (do4, q_len), (k4, k_len), (v4, k_len)):
            for b in range(Bn):
                x4[b, :, ln[b]:] = 0                                     # rows of no batch: nothing there, nothing from there
    tag = tag or '%s hd %d Sq %d Sk %d causal %d mask %s kmax %d' % (fam, hd, Sq, Sk, causal, mask, use_kmax)
    got = _run(ops, fam, q4, k4, v4, do4, scale, causal, km, use_kmax, one_pass=pipe64, dbias=fam == 'pipe', packed=packed, tag=tag)
    D = lambda x: x.double()
    truth = A.attn(D(q4), D(k4), D(v4), D(do4), vis, scale)
    S = A.scales(truth, D(q4), D(k4), D(v4), D(do4), vis, scale)
    narrow = fam != 'x3'
    # the exact zeros, by name (figure() asserts them again through S == 0)
    dead_q = ~vis.any(-1).expand(Bn, Hn, Sq)
    dead_k = ~vis.any(-2).expand(Bn, Hn, Sk)
    for sfx in ('', '1') if pipe64 else ('',):
        assert bool((got['dq' + sfx][dead_q] == 0).all()), tag + ': dq of a row without a visible key'
        assert bool((got['dk' + sfx][dead_k] == 0).all()) and bool((got['dv' + sfx][dead_k] == 0).all()), tag + ': dk / dv of a key no query sees'
    assert bool((got['o'][dead_q] == 0).all()) and bool((got['lse'][dead_q] == float('inf')).all()), tag + ': o / lse of a row without a visible key'
    assert bool(torch.isfinite(got['lse'][~dead_q]).all()), tag + ': lse of a row with a visible key'
    over = []
    for model, fam_name, sfx, names in ((MODEL[fam], fam, '', ('o', 'lse', 'delta', 'dq', 'dk', 'dv')),) + ((('one_pass', 'one_pass', '1', ('delta', 'dq', 'dk', 'dv')),) if pipe64 else ()):
        m = A.attn(q4.float(), k4.float(), v4.float(), do4.float(), vis, scale, **A.MODELS[model])
        fn = fam_name + (' packed' if packed is not None else '') + (' lazy' if qk is not None else '')
        for n in names:
            st = narrow and n not in ('lse', 'delta')
            _bound(over, tag, fn, n, A.figure(got[n + sfx], truth[n], S[n], st), A.figure(m[n], truth[n], S[n], st))
        if fam == 'pipe':
            for n in 'qkv':
                cs = A.colsum(S['d' + n])
                _bound(over, tag, fn, 'dbias_' + n, A.figure(got['dbias_' + n + sfx], A.colsum(truth['d' + n]), cs, False), A.figure(A.colsum(m['d' + n]), A.colsum(truth['d' + n]), cs, False))
    same = []
    if packed is None:
        b, h = (Sq + Sk + hd) % Bn, (Sq + 2 * Sk + causal) % Hn
        one = lambda x4: x4[b:b + 1, h:h + 1].contiguous()
        alone = _run(ops, fam, one(q4), one(k4), one(v4), one(do4), scale, causal, None if km is None else km[b:b + 1].contiguous(), use_kmax,
                     one_pass=pipe64, dbias=False, tag=tag + ' alone')
        for n in ('o', 'lse', 'dq', 'dk', 'dv') + (('dq1', 'dk1', 'dv1') if pipe64 else ()):
            if not torch.equal(alone[n][0, 0], got[n][b, h]):
                same.append('%s of pair (%d, %d) differs from the same data run as B = 1, H = 1' % (n, b, h))
    assert not over and not same, tag + ': ' + '; '.join(over + same)


# ---------------------------------------------------------------- the cases
@pytest.mark.parametrize('causal', [False, True])
@pytest.mark.parametrize('Sq,Sk', SHAPES)
@pytest.mark.parametrize('fam,hd', FAMILIES)
def test_every_tile_edge(ops, fam, hd, Sq, Sk, causal):
    """Every (Sq, Sk) of SHAPES, causal and not, under a key mask with holes and a masked tail (kmax from pb_key_extent where the family reads
    it); at Sq == Sk in the qkv layout, else q alone and K, V in the stacked-projection layout."""
    _case(ops, fam, hd, Sq, Sk, causal, 'holes', fam != 'generic', 1000 * hd + 7 * Sq + Sk)


@pytest.mark.parametrize('causal', [False, True])
@pytest.mark.parametrize('mask', MASKS)
@pytest.mark.parametrize('fam,hd,use_kmax', [(f, h, u) for f, h in FAMILIES for u in (False, True) if not (u and f == 'generic')])
def test_every_mask_edge(ops, fam, hd, use_kmax, mask, causal):
    """Every mask of MASKS at Sq 129, Sk 193 (three whole key tiles and one key of a fourth: 'last_only' leaves only the last key of a partial
    tile visible), with and without kmax. The generic kernels do not read kmax: their cases run without."""
    _case(ops, fam, hd, 129, 193, causal, mask, use_kmax, 31 * hd + len(mask))


@pytest.mark.parametrize('causal', [False, True])
@pytest.mark.parametrize('kind', A.LAZY_KINDS)
@pytest.mark.parametrize('hd', [64, 96, 128])
def test_lazy_reference_maximum(ops, hd, kind, causal):
    """The pipelined forward keeps a row's reference maximum until a tile holds a score more than 8 log2 units above it: scores that rise or
    fall by 9.5 log2 units per 64-key tile, step by just under and just over 8, are randn * 4, or sit near -100; nine key tiles. Forward and
    every backward behind it (head_dim 64: the one-pass kernel too)."""
    _case(ops, 'pipe', hd, 130, 513, causal, 'none', False, hd + len(kind), qk=kind)


@pytest.mark.parametrize('causal', [False, True])
@pytest.mark.parametrize('Sq,Sk', SHAPES)
@pytest.mark.parametrize('fam,hd', [f for f in FAMILIES if f[0] != 'generic'])
def test_packed_rows(ops, fam, hd, Sq, Sk, causal):
    """Packed rows: three batches of different lengths back to back, the longest Sq / Sk rows, against the visibility the dense call would see
    (key j < k_vis[b], causal j <= i). The generic kernels refuse packed rows."""
    q_len = [max(1, Sq // 2), Sq, max(1, Sq - 1)]
    k_len = [Sk, max(1, Sk - 1), max(1, Sk // 3)]
    k_vis = [max(1, Sk - 2), k_len[1], max(1, k_len[2] // 2)]
    _case(ops, fam, hd, Sq, Sk, causal, 'none', False, 13 * hd + Sq + 3 * Sk, packed=(q_len, k_len, k_vis),
          tag='%s packed hd %d Sq %d Sk %d causal %d' % (fam, hd, Sq, Sk, causal))


def test_zz_worst_ratios():
    """Prints the worst kernel / model ratio and the largest kernel figure per family and output over the cases that ran before (pytest -s)."""
    for (fam, name), (ratio, fig) in sorted(WORST.items()):
        print('WORST %-16s %-8s ratio %6.3f   largest kernel figure %10.4g' % (fam, name, ratio, fig))
