"""Operand makers, the float64 model, the caps and the case table of tests/test_gemm_x3_kernels_gpu.py: pb_gemm with dtype PB_F32X3
(csrc/pb_gemm_x3.hip). Checked without a GPU by tests/test_gemm_x3_ref_cpu.py. Case, place, Guarded, assert_equal, kind3_figure and MARGIN
are those of tests/gemm_ref.py; nothing here touches the library.

The kernel cuts every f32 operand value x into hi = bf16(x), lo = bf16(x - hi) and runs ONE bf16 GEMM over a K axis three times as long,
A3 = [hi | hi | lo], B3 = [hi | lo | hi]: C = alpha sum_k (a_hi b_hi + a_hi b_lo + a_lo b_hi) (+ the epilogue of gemm_ref). That is the MODEL;
triple() builds A3 and B3 with torch casts (test_split_bf16_planes pins the kernel's split1 to them) and the model is gemm_ref.reference()
on them, in float64.

Exact operands: x = p + q, p uniform on {-2 .. 2}, q uniform on {-3 .. 3} 2^-11, q = 0 wherever p = 0. Then hi = p and lo = q exactly
(|q| < half a bf16 ulp of 1, and q itself is a bf16 number), 69 % of the elements have a nonzero lo, every term of the model is a multiple of
2^-11 (hi hi is an integer, hi lo and lo hi multiples of 2^-11; lo lo, a multiple of 2^-22, is NOT part of the model), and every partial sum
is at most (4 K + 8) in magnitude: |a_hi b_hi| + |a_hi b_lo| + |a_lo b_hi| <= 4 + 12 2^-11 per k. So while (4 K + 8) 2^11 < 2^24 float32
holds every partial sum exactly whatever the order -- K tiles, the three segments, split-K slabs, MFMA lanes -- and torch.equal applies.
A kernel that added lo lo, lost a lo contribution, mixed up the roles or read a pad changes a multiple of 2^-11 (or of 2^-22).
"""
import math

import torch

from tests import gemm_ref as G

F32, BF16, F64 = G.F32, G.BF16, G.F64
UNIT = 2 ** 11                                      # the model's terms are multiples of 1 / UNIT
EPIS = ('store', 'bias', 'alpha', 'acc', 'acc32', 'mul', 'mulcs', 'gelu', 'real')
KIND3 = ('gelu', 'real')
# |model - true| <= C_MODEL sum_k |a b| per element (test_gemm_x3_ref_cpu.py: the derivation and the assertion)
C_MODEL = 2.0 ** -16 * ((1 + 2.0 ** -8) ** 2 + 2 + 2.0 ** -16)


class Case(G.Case):
    """gemm_ref.Case for PB_F32X3: f32 operands, f32 C. More knobs: a_spad / b_spad lengthen the batch stride of an operand (so that it
    is no multiple of 4), aux_off moves aux_in / aux_out off 16 bytes. `kernel` and the split forms in the id are COMPUTED by the mirrors
    below (product_kernel, split_forms), not written by hand."""

    def __init__(self, M, N, K, **kw):
        self.a_spad, self.b_spad, self.aux_off = kw.pop('a_spad', 0), kw.pop('b_spad', 0), kw.pop('aux_off', 0)
        alpha = kw.get('alpha')
        assert 'dt' not in kw and 'kernel' not in kw
        G.Case.__init__(self, M, N, K, dt='f32', **kw)
        assert self.epi in EPIS
        if alpha is not None:
            self.alpha = alpha
        self.kernel = product_kernel(self)

    exact = property(lambda s: s.epi not in KIND3)
    c32 = property(lambda s: True)

    @property
    def id(self):
        extra = ''
        if self.a_spad or self.b_spad:
            extra += '-spad%d.%d' % (self.a_spad, self.b_spad)
        if self.epi in ('mul', 'mulcs', 'gelu'):
            extra += '-aux%d.%d-%s' % (self.aux_off, self.ldaux_pad, 'postV' if post_vec(self) else 'postS')
        if self.alpha != 1.0:
            extra += '-alpha%g' % self.alpha
        return '%s+%s-' % split_forms(self) + G.Case.id.fget(self).replace('-f32-', '-x3-') + extra


# ---------------------------------------------------------------- mirrors of pb_gemm_x3 / pb_gemm2_try: which branch a case takes
def _ld(case, which):
    kc, cols_kc, cols_rc, pad = ((case.a_kc, case.K, case.M, case.lda_pad) if which == 'a' else (case.b_kc, case.K, case.N, case.ldb_pad))
    return (cols_kc if kc else cols_rc) + pad


def batch_stride(case, which):
    """Elements between two batches of an operand as place_batches() lays them out."""
    kc, rows_kc, spad = (case.a_kc, case.M, case.a_spad) if which == 'a' else (case.b_kc, case.N, case.b_spad)
    return (rows_kc if kc else case.K) * _ld(case, which) + spad


def _vec_ok(case, which):
    """vec_ok(): base on 16 bytes, ld and both batch strides multiples of 4 (one batch: the strides passed are 0)."""
    off = case.a_off if which == 'a' else case.b_off
    s = batch_stride(case, which)
    return off % 4 == 0 and _ld(case, which) % 4 == 0 and (case.nbatch == 1 or (s % 4 == 0 and case.nb2 * s % 4 == 0))


def split_forms(case):
    """(form of A, form of B): kcV / kcS split_kc_kernel<ROLE, VEC>, rcV / rcS split_rc_kernel, tr split_tr_kernel; ROLE 0 is A, 1 is B."""
    nt = case.a_kc or case.b_kc                                                # a mixed layout is made NT by the transposing split
    out = []
    for which, kc in (('a', case.a_kc), ('b', case.b_kc)):
        form = 'kc' if kc else 'tr' if nt else 'rc'
        out.append(form if form == 'tr' else form + ('V' if _vec_ok(case, which) else 'S'))
    return tuple(out)


def product_kernel(case):
    """The kernel the bf16 product over 3 Kp runs on: 'generic' (pb_gemm2_try declines: N % 8, M % 8 with a row-contiguous A3, C off 16 bytes,
    ldc % 4; or PB_GEMM_FORCE_V1), else 'pingpong' (256 x 256) or 'tile128'. pb_gemm_x3 sets PB_GEMM_TILE128 for one unsplit batch below 128
    tiles of 256 x 256; A3 / B3 themselves always satisfy pb_gemm2_try (K = 3 Kp, ld = 3 Kp or Mp / Np, 256-byte bases)."""
    M, N = case.M, case.N
    tn = not (case.a_kc or case.b_kc)
    if case.flags.get('force_v1') or N % 8 or (tn and M % 8) or case.c_off % 4 or (N + case.ldc_pad) % 4:
        return 'generic'
    t128 = case.flags.get('tile128') or (case.splitk <= 1 and case.nbatch == 1 and -(-M // 256) * -(-N // 256) < 128)
    big = not t128 and M >= 256 and N >= 256 and (case.flags.get('tile256') or (case.splitk <= 1 and M >= 2048 and N >= 512))
    return 'pingpong' if big else 'tile128'


def post_vec(case):
    """`vec` of x3_post_kernel: C and aux on 16 bytes, ldc and ldaux multiples of 4 (and then n + 4 <= N per group of four)."""
    return case.c_off % 4 == 0 and case.aux_off % 4 == 0 and (case.N + case.ldc_pad) % 4 == 0 and (case.N + case.ldaux_pad) % 4 == 0


def kp(K):
    return -(-K // 64) * 64


def slab_cuts(case):
    """Split-K over the 3 Kp / 64 K tiles of the triple product: (cuts that fall INSIDE a segment, cuts ON a segment boundary, empty slabs)."""
    seg, nkt = kp(case.K) // 64, 3 * kp(case.K) // 64
    per = -(-nkt // case.splitk)
    cuts = [per * i for i in range(1, case.splitk) if per * i < nkt]
    return (sum(1 for c in cuts if c % seg), sum(1 for c in cuts if c % seg == 0), sum(1 for i in range(case.splitk) if per * i >= nkt))


def chunks(case, which):
    """Work items (8-element chunks) of the kc / rc split of an operand: the four-chunk unroll hands out 1024 per workgroup."""
    kc, rows = (case.a_kc, case.M) if which == 'a' else (case.b_kc, case.N)
    return rows * (kp(case.K) // 8) if kc else kp(case.K) * (-(-rows // 8))


# ---------------------------------------------------------------- operands
def pq(shape, seed):
    """float64 x = p + q 2^-11 (module docstring)."""
    p = G.ints(shape, -2, 2, seed)
    q = G.ints(shape, -3, 3, seed + 500009)
    return p.to(F64) + torch.where(p == 0, torch.zeros_like(q), q).to(F64) / UNIT


def make_ab(case):
    if not case.exact:
        return G.make_ab(case)                                                 # randn, rounded to f32
    s = G._seed(case)
    return pq((case.nbatch, case.M, case.K), s), pq((case.nbatch, case.N, case.K), s + 1)


def make_inputs(case, ab=None):
    """gemm_ref.make_inputs with the operands of this module: bias, aux and the old C stay the integers of the bf16 suite."""
    return G.make_inputs(case, ab=ab if ab is not None else make_ab(case))


def planes(x):
    """hi, lo of an operand as float64, by torch casts."""
    x = x.to(F32)
    hi = x.to(BF16)
    lo = (x - hi.to(F32)).to(BF16)
    return hi.to(F64), lo.to(F64)


def triple(x):
    """The inputs with A and B replaced by A3 = [hi | hi | lo], B3 = [hi | lo | hi] along K (float64)."""
    ah, al = planes(x['A'])
    bh, bl = planes(x['B'])
    return dict(x, A=torch.cat([ah, ah, al], 2), B=torch.cat([bh, bl, bh], 2))


def reference(case, x, r0=0, r1=None):
    """The model in float64: gemm_ref.reference on the triple operands. 'abs' (real-valued cases) is then
    S = |alpha| sum_k (|a_hi b_hi| + |a_hi b_lo| + |a_lo b_hi|) + |bias|."""
    return G.reference(case, triple(x), r0, r1)


def float32_evaluation(case, x):
    """The model in plain float32 torch on the same planes, term by term as it is written -- a_hi b_hi + a_hi b_lo + a_lo b_hi, three
    matmuls -- and the epilogue of gemm_ref.float32_evaluation: the yardstick of the real-valued cases."""
    (ah, al), (bh, bl) = planes(x['A']), planes(x['B'])
    ah, al, bh, bl = (t.to(F32) for t in (ah, al, bh.transpose(1, 2), bl.transpose(1, 2)))
    v = torch.tensor(case.alpha, dtype=F32) * (ah @ bh + ah @ bl + al @ bh)
    if x['bias'] is not None:
        v = v + x['bias'].to(F32)
    if not case.gelu:
        return v, None
    cdf = 0.5 * (1 + torch.erf(v * (1.0 / math.sqrt(2.0))))
    return v * cdf, cdf + v * torch.exp(-0.5 * v * v) * (1.0 / math.sqrt(2 * math.pi))


def place_batches(mat, kc, ld_pad, off, spad):
    """gemm_ref.place, and with spad > 0 the same layout with `spad` more NaN elements between two batches.
    -> (flat f32 tensor, ld, stride of a batch)."""
    if not spad:
        return G.place(mat, kc, ld_pad, off, F32)
    nb, R, K = mat.shape
    rows, cols = (R, K) if kc else (K, R)
    ld = cols + ld_pad
    stride = rows * ld + spad
    buf = torch.full((off + nb * stride + 8,), float('nan'), dtype=F32, device=mat.device)
    buf[off:].as_strided((nb, rows, cols), (stride, ld, 1)).copy_(mat if kc else mat.transpose(1, 2))
    return buf, ld, stride


# ---------------------------------------------------------------- caps
def caps(case, stored=None):
    """[(what, value, limit)], value < limit required, in units of 2^-11 (2^-12 when alpha = 0.5): gemm_ref.caps for the p + q operands."""
    half = 2 if case.alpha == 0.5 else 1
    K = case.K
    top = (abs(case.alpha) * (4 * K + 8) + (8 if case.bias else 0)) * (2 if case.mul else 1) + (64 if case.acc else 0)
    out = [('K: the bound 4 K + 8 on a partial sum needs 12 K 2^-11 <= 8', K, 1366),
           ('(4 K + 8) 2^11', half * (4 * K + 8) * UNIT, G.EXACT),
           ('largest epilogue value ((|alpha| (4 K + 8) + 8 [bias]) 2 [aux_in] + 64 [old C]) 2^11', half * top * UNIT, G.EXACT)]
    if case.colsum:
        out.append(('column sums: (sum_m |stored C| + |prior|) 2^11', half * float((stored[0].double().abs().sum(0) + G.CS_PRIOR).max()) * UNIT, G.EXACT))
    return out


def assert_caps(case, stored=None):
    for what, value, limit in caps(case, stored):
        assert value < limit, '%s: the reference is not exact: %s = %g >= %g' % (case.id, what, value, limit)


# ---------------------------------------------------------------- the case table
NT, NN, TT, TN = (True, True), (True, False), (False, True), (False, False)     # (a_kc, b_kc)
LAYOUTS = [NT, NN, TT, TN]
KS = [1, 7, 8, 9, 63, 64, 65, 72, 130]
SIZES = [1, 7, 8, 9, 63, 64, 65, 129, 264]
T256 = dict(tile256=True)


def _pad(cols, vec):
    """A pad of 4 .. 8 NaN columns that makes ld a multiple of 4 (the VEC form) or not."""
    return (-cols) % 4 + (4 if vec else 5)


def _c(M, N, K, lay, vec=True, **kw):
    a_kc, b_kc = lay
    kw.setdefault('lda_pad', _pad(K if a_kc else M, vec))
    kw.setdefault('ldb_pad', _pad(K if b_kc else N, vec))
    return Case(M, N, K, a_kc=a_kc, b_kc=b_kc, **kw)


def _k_cases():
    """Every K around the 8-element chunk, the 64-wide segment pad and a ragged second K tile, each split kernel in both VEC forms."""
    return [_c(65, 72, k, lay, vec, epi='bias' if k % 2 else 'store') for lay in LAYOUTS for vec in (True, False) for k in KS]


def _mn_cases():
    """Rows around 8 (Mp / Np pad columns of the rc form), 64 (ragged tiles of split_tr, K = 65 ragged as well), 128 and 256."""
    out = []
    for lay in LAYOUTS:
        for vec in (True, False):
            out += [_c(m, 72, 65, lay, vec) for m in SIZES if m != 65] + [_c(65, n, 65, lay, vec) for n in SIZES]
    return out


def _vec_cases():
    """vec_ok, one condition at a time (the rest satisfied): base off 16 bytes by 1 and by 2 elements, ld % 4, batch strides off 4 -- and all satisfied."""
    out = []
    for lay in LAYOUTS:
        base = dict(lda_pad=_pad(65 if lay[0] else 72, True), ldb_pad=_pad(65 if lay[1] else 72, True))
        for kw in (dict(a_off=1), dict(a_off=2), dict(b_off=1), dict(b_off=2), dict(a_off=4, b_off=8),
                   dict(lda_pad=base['lda_pad'] + 1), dict(ldb_pad=base['ldb_pad'] + 2)):
            out.append(Case(72, 72, 65, a_kc=lay[0], b_kc=lay[1], **dict(base, **kw)))
        for kw in (dict(), dict(a_spad=1), dict(b_spad=2), dict(a_spad=4, b_spad=8), dict(a_off=1, b_off=1)):
            out.append(Case(72, 72, 65, a_kc=lay[0], b_kc=lay[1], nb1=2, nb2=3, epi='acc', ldc_pad=4, **dict(base, **kw)))
    return out


def _unroll_cases():
    """idx >= n in the four-chunk unroll: 1024 chunks (one full workgroup), 1032 / 1088 (a second one with 8 / 64 chunks), 520 (half of one)."""
    return [_c(m, n, 64, lay, vec) for lay in (NT, TN) for vec in (True, False) for m, n in ((128, 128), (129, 136), (65, 72))]


EPI_LIST = ['store', 'bias', 'alpha', 'acc', 'acc32', 'mul', 'mulcs']


def _epilogue_cases():
    out = []
    for lay in (NT, TN):
        for n in (72, 70):                                                     # tile128 and the generic fallback
            out += [_c(72, n, 65, lay, epi=e) for e in EPI_LIST if n % 4 == 0 or e != 'mulcs']      # column sums need N % 4 == 0: test_refusals_write_nothing
            out += [_c(72, n, 65, lay, epi='bias', alpha=a) for a in (0.5, -2.0)]
    out += [_c(264, 264, 130, lay, epi=e) for lay in (NT, NN) for e in ('acc', 'mulcs')]    # more than one tile
    return out


def _post_cases(epi):
    """x3_post_kernel, vector and scalar form: C off 16 bytes, aux off 16 bytes, ldc % 4, ldaux % 4 one at a time; N % 4 under the vector form."""
    var = [dict(ldaux_pad=4), dict(ldaux_pad=4, c_off=1), dict(ldaux_pad=4, aux_off=1), dict(ldaux_pad=4, ldc_pad=1), dict(ldaux_pad=5),
           dict(ldaux_pad=4, ldc_pad=4), dict(ldaux_pad=4, c_off=4, aux_off=4)]
    out = [_c(65, 72, 65, NT, epi=epi, **kw) for kw in var]
    out += [_c(65, 70, 65, NT, epi=epi, ldc_pad=2, ldaux_pad=2), _c(65, 67, 65, NT, epi=epi, ldc_pad=1, ldaux_pad=5),
            _c(65, 70, 65, NT, epi=epi, ldc_pad=3, ldaux_pad=2), _c(264, 264, 65, TN, epi=epi, ldaux_pad=8)]
    return out


def _product_cases():
    """The 128-tile threshold of pb_gemm_x3 on both sides, NT and TN; the declines of pb_gemm2_try."""
    out = [_c(8192, 1024, 64, lay, epi=e) for lay, e in ((NT, 'bias'), (TN, 'store'))]     # 32 x 4 = 128 tiles: ping-pong
    out += [_c(8192 - 256, 1024, 64, NT, epi='acc')]                                           # 124 tiles: tile128
    out += [_c(264, 268, 65, lay) for lay in LAYOUTS] + [_c(268, 264, 65, TN), _c(268, 264, 65, NT)]
    out += [_c(264, 264, 65, NT, c_off=1), _c(264, 264, 65, NT, ldc_pad=2), _c(264, 264, 65, NT, flags=dict(force_v1=True), epi='bias')]
    return out


SPLITS = [(130, 2), (128, 3), (130, 4), (65, 4)]       # (K, splits): 9 K tiles cut at 5 (inside the middle segment); 6 at 2, 4 (the segment boundaries);
#                                                        9 at 3, 6 (boundaries) + an empty slab; 6 at 2, 4 + an empty slab


def _splitk_cases():
    out = []
    for k, ns in SPLITS:
        for lay in (NT, TN, NN):
            for (m, n), fl in (((72, 72), {}), ((264, 264), T256)):
                out += [_c(m, n, k, lay, flags=fl, splitk=ns, accum=acc) for acc in (False, True)]
    return out


def _batch_cases():
    out = [_c(65, 72, 65, lay, nb1=2, nb2=3, epi=e, ldc_pad=4) for lay in LAYOUTS for e in ('store', 'acc')]
    out += [_c(264, 264, 64, lay, nb1=1, nb2=2, flags=T256) for lay in (NT, TN)]            # batches keep PB_GEMM_TILE256: ping-pong
    return out


def _real_cases():
    """One randn case per product kernel, and the GELU pair on the tiled and the generic product, both forms of the post pass."""
    out = [_c(264, 264, 100, NT, epi='real'), _c(264, 264, 100, NN, epi='real'),                       # tile128
           _c(264, 264, 100, TN, epi='real', nb2=2, flags=T256),                                        # ping-pong
           _c(264, 268, 100, NT, epi='real'),                                                           # generic
           _c(264, 264, 448, TN, epi='real', splitk=3), _c(264, 264, 448, NT, epi='real', splitk=3, flags=T256)]
    out += [_c(264, 264, 100, NT, epi='gelu', ldaux_pad=8), _c(264, 262, 100, NT, epi='gelu', ldaux_pad=3)]
    return out


FAMILIES = dict(k=_k_cases(), mn=_mn_cases(), vec=_vec_cases(), unroll=_unroll_cases(), epilogue=_epilogue_cases(), mul=_post_cases('mul'),
                gelu=_post_cases('gelu'), product=_product_cases(), splitk=_splitk_cases(), batch=_batch_cases(), real=_real_cases())

# Workspace reuse: (the small ragged case, the poisoning call's shape); one per split kernel form. The poisoning shape has no pad of its own
# (K a multiple of 64, rows a multiple of 8), so every element of its A3 / B3 is inf or NaN, and its A3 alone is larger than the small case's A3 + B3.
POISON_SHAPE = (264, 264, 256)
POISON = [_c(65, 72, 65, NT), _c(65, 72, 65, NT, vec=False), _c(72, 72, 65, TN), _c(72, 72, 65, TN, vec=False), _c(65, 72, 65, NN), _c(65, 72, 65, TT),
          _c(65, 70, 7, TN), _c(7, 72, 130, NT)]

# The unfused attention: heads addressed by stride inside (T, 3 d) rows. (batches, heads, tokens, head_dim)
ATTN = [(2, 3, 72, 32), (2, 2, 67, 32)]


def all_cases():
    return [c for f in FAMILIES.values() for c in f] + POISON
