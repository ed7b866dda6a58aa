"""Operand makers, float64 references, guarded allocations and the case table of tests/test_gemm_kernels_gpu.py (checked without a GPU
by tests/test_gemm_ref_cpu.py). Nothing here touches the library: every function works on CPU and on device tensors alike.

The GEMM is  C[m][n] (+)= epi(alpha * sum_k A(m,k) B(n,k))  with, in this order,  v = alpha acc + bias;  GELU: aux_out = gelu'(v), v = gelu(v);
v *= aux_in;  v += old C;  store. With small-integer operands every product, partial sum and epilogue value is an integer (or a half-integer,
alpha = 0.5) far below 2^24, so float32 holds it exactly whatever the summation order, and a bf16 store is ONE round-to-nearest-even of an
exactly known number: reference() in float64, then .to(float32).to(bfloat16). caps() states the conditions on the REFERENCE that make this
exact; they are asserted in every GPU case and, for the whole table, on the CPU.
"""
import math

import torch

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
EXACT = 2 ** 24
E24, E8 = 2.0 ** -24, 2.0 ** -8
MARGIN = 4.0
ERF_ERR = 1.5e-7                      # |error| of the Abramowitz-Stegun 7.1.26 erf that pb_common.h states for its bf16 GELU
GUARD = 1.5 * 2.0 ** -20              # finite, exact in bf16: a stray store changes it, and so does a stray read-modify-write
CS_PRIOR = 3.0                        # what colsum_out holds going in (the call accumulates)
ALPHAS = (1.0, 0.5, -2.0)
EPIS = ('store', 'bias', 'alpha', 'acc', 'acc32', 'c32', 'mul', 'mulcs', 'rowdot', 'rowdotb', 'gelu', 'real', 'real32')
KIND3 = ('gelu', 'real', 'real32')             # float64 with a per-element bound; every other epilogue is exact


class Case(object):
    """One call of ops.gemm. `kernel` names the branch the dispatcher is expected to take (documentation and test ids only)."""
    _defaults = dict(a_kc=True, b_kc=True, dt='bf16', epi='store', alpha=1.0, flags=None, lda_pad=0, ldb_pad=0, ldc_pad=0, ldaux_pad=0,
                     a_off=0, b_off=0, c_off=0, nb1=1, nb2=1, splitk=1, accum=False, kernel='', seed=0)

    def __init__(self, M, N, K, **kw):
        self.M, self.N, self.K = M, N, K
        for k, v in self._defaults.items():
            setattr(self, k, kw.pop(k, v))
        assert not kw, kw
        assert self.epi in EPIS and self.dt in ('bf16', 'f32')
        self.flags = dict(self.flags or {})
        if self.epi == 'alpha':
            self.alpha = ALPHAS[1 + (M + N + K) // 8 % 2]
        if self.epi == 'acc32':
            self.alpha = -2.0
        if self.epi in ('mul', 'mulcs', 'gelu') and not self.ldaux_pad:
            self.ldaux_pad = 16

    # what the epilogue does
    bias = property(lambda s: s.epi in ('bias', 'rowdotb', 'gelu', 'acc', 'mulcs'))
    c32 = property(lambda s: s.epi in ('acc32', 'c32', 'real32') or s.splitk > 1)
    acc = property(lambda s: s.epi in ('acc', 'acc32') or s.accum)
    mul = property(lambda s: s.epi in ('mul', 'mulcs'))
    colsum = property(lambda s: s.epi == 'mulcs')
    rowdot = property(lambda s: s.epi in ('rowdot', 'rowdotb'))
    gelu = property(lambda s: s.epi == 'gelu')
    exact = property(lambda s: s.epi not in KIND3)
    in_dtype = property(lambda s: BF16 if s.dt == 'bf16' else F32)
    c_dtype = property(lambda s: F32 if (s.c32 or s.dt == 'f32') else BF16)
    nbatch = property(lambda s: s.nb1 * s.nb2)

    @property
    def id(self):
        lay = ('N' if self.a_kc else 'T') + ('T' if self.b_kc else 'N')
        fl = ''.join('-%s%s' % (k, '' if v is True else v) for k, v in sorted(self.flags.items()))
        extra = ''
        if self.lda_pad or self.ldb_pad or self.ldc_pad:
            extra += '-ld%d.%d.%d' % (self.lda_pad, self.ldb_pad, self.ldc_pad)
        if self.a_off or self.b_off or self.c_off:
            extra += '-off%d.%d.%d' % (self.a_off, self.b_off, self.c_off)
        if self.nbatch > 1:
            extra += '-b%dx%d' % (self.nb1, self.nb2)
        if self.splitk > 1:
            extra += '-split%d%s' % (self.splitk, 'acc' if self.accum else '')
        return '%s-%s-%dx%dx%d-%s-%s%s%s' % (self.kernel or 'auto', lay, self.M, self.N, self.K, self.dt, self.epi, fl, extra)


# ---------------------------------------------------------------- operands
def ints(shape, lo, hi, seed):
    """int64, uniform on [lo, hi], from a CPU generator: the same numbers on every machine."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, tuple(shape), generator=g)


def make_ab(case):
    """The two operands alone, on the CPU, as float64: A (nbatch, M, K), B (nbatch, N, K). They depend on the shape and the seed, not on the epilogue."""
    M, N, K, nb = case.M, case.N, case.K, case.nbatch
    s = _seed(case)
    if case.exact:
        return ints((nb, M, K), -2, 2, s).to(F64), ints((nb, N, K), -2, 2, s + 1).to(F64)
    g = torch.Generator().manual_seed(s)
    A = torch.randn(nb, M, K, generator=g, dtype=F64).to(case.in_dtype)            # rounded to the storage dtype first: the reference runs on the rounded values
    B = (torch.randn(nb, N, K, generator=g, dtype=F64) / math.sqrt(K) + 0.1 * torch.arange(N, dtype=F64)[None, :, None] / N).to(case.in_dtype)   # asymmetric
    return A.to(F64), B.to(F64)


def _seed(case):
    return 1000003 * case.seed + 7919 * case.M + 104729 * case.N + 31 * case.K + 17 * case.nbatch


def make_inputs(case, ab=None):
    """The logical operands of a case on the CPU as float64 (integers for an exact case): A, B (make_ab, or the pair given), bias (N), aux (M, N),
    c0 (nbatch, M, N) -- whatever the case does not use is None."""
    M, N, nb, s = case.M, case.N, case.nbatch, _seed(case)
    x = dict(bias=None, aux=None, c0=None)
    x['A'], x['B'] = ab if ab is not None else make_ab(case)
    if case.exact:
        if case.bias:
            x['bias'] = ints((N,), -8, 8, s + 2).to(F64)
        if case.mul or case.rowdot:
            x['aux'] = ints((M, N), -2, 2, s + 3).to(F64)
        if case.acc:
            x['c0'] = ints((nb, M, N), -64, 64, s + 4).to(F64)
    elif case.bias:
        x['bias'] = torch.randn(N, generator=torch.Generator().manual_seed(s + 2), dtype=F32).to(F64)
    return x


def place(mat, kc, ld_pad, off, dtype, tail=8):
    """A (nbatch, R, K) operand as the kernels read it. kc: memory [R][ld = K + ld_pad], else [K][ld = R + ld_pad]; the batches are stacked; `off` elements
    in front. Pad columns, the front and `tail` elements behind hold NaN: an operand element read from outside the matrix poisons C.
    -> (flat tensor, ld, (stride of a batch))."""
    nb, R, K = mat.shape
    rows, cols = (R, K) if kc else (K, R)
    ld = cols + ld_pad
    buf = torch.full((off + nb * rows * ld + tail,), float('nan'), dtype=dtype, device=mat.device)
    view = buf[off:off + nb * rows * ld].view(nb, rows, ld)[:, :, :cols]
    view.copy_(mat if kc else mat.transpose(1, 2))
    return buf, ld, rows * ld


# ---------------------------------------------------------------- references
def gelu64(v):
    cdf = 0.5 * (1 + torch.erf(v / math.sqrt(2.0)))
    return v * cdf, cdf + v * torch.exp(-0.5 * v * v) / math.sqrt(2 * math.pi)


def store(v, dtype):
    """float64 -> what the kernel leaves in memory: one rounding of the exactly known number."""
    return v.to(F32) if dtype == F32 else v.to(F32).to(BF16)


def reference(case, x, r0=0, r1=None):
    """float64 reference of rows r0 .. r1 - 1 (all batches): dict with 'acc' = sum_k a b, 'pre' = alpha acc + bias, 'C' (before the store rounding),
    'aux_out' (GELU), 'abs' = sum_k |a b| (+ |bias|) for the bounds of kind 3. Exact for integer operands."""
    r1 = case.M if r1 is None else r1
    A, B = x['A'][:, r0:r1].double(), x['B'].double()                          # (a large A may be kept in its storage dtype)
    acc = A @ B.transpose(1, 2)
    v = case.alpha * acc
    if x['bias'] is not None:
        v = v + x['bias']
    out = dict(acc=acc, pre=v, aux_out=None)
    if not case.exact:
        out['abs'] = abs(case.alpha) * (A.abs() @ B.abs().transpose(1, 2)) + (x['bias'].abs() if x['bias'] is not None else 0)
    if case.gelu:
        v, out['aux_out'] = gelu64(v)
    if case.mul:
        v = v * x['aux'][r0:r1]
    if case.acc:
        v = v + x['c0'][:, r0:r1]
    out['C'] = v
    return out


def colsum_reference(case, stored):
    """colsum_out after the call: the prior contents plus the column sums of the STORED values (one batch)."""
    return (CS_PRIOR + stored[0].double().sum(0)).to(F32)


def rowdot_reference(case, stored, aux):
    """(N / 64, M): sums over each 64-column group of stored C * aux."""
    M, N = case.M, case.N
    return (stored[0].double() * aux).reshape(M, N // 64, 64).sum(-1).t().contiguous().to(F32)


def float32_evaluation(case, x):
    """The same formula in plain float32 torch on the same rounded inputs: the yardstick of kind 3."""
    A, B = x['A'].to(F32), x['B'].to(F32)
    v = torch.tensor(case.alpha, dtype=F32) * (A @ B.transpose(1, 2))
    if x['bias'] is not None:
        v = v + x['bias'].to(F32)
    if not case.gelu:
        return v, None
    cdf = 0.5 * (1 + torch.erf(v * (1.0 / math.sqrt(2.0))))
    return v * cdf, cdf + v * torch.exp(-0.5 * v * v) * (1.0 / math.sqrt(2 * math.pi))


def caps(case, stored=None):
    """[(what, value, limit)], value < limit required: the conditions on the reference under which every float32 sum is exact in any order.
    `stored` (the reference C as stored) is needed by a case with column sums or row dots; the others have a-priori caps only."""
    half = 2 if case.alpha == 0.5 else 1                                       # half-integers: one more bit
    out = [('4 K + 8', 4 * case.K + 8, EXACT),
           ('largest epilogue value: 2 (2 * 4 K + 8) + 64, in halves when alpha = 0.5', half * (2 * (2 * 4 * case.K + 8) + 64), EXACT)]
    if case.colsum:
        out.append(('column sums: sum_m |stored C| + |prior|', half * float((stored[0].double().abs().sum(0) + CS_PRIOR).max()), EXACT))
    if case.rowdot:
        out.append(('row dots: 64 max|C| * 2', half * 64 * float(stored.double().abs().max()) * 2, EXACT))
    return out


def assert_caps(case, stored=None):
    for what, value, limit in caps(case, stored):
        assert value < limit, '%s: the reference is not exact: %s = %g >= %g' % (case.id, what, value, limit)


# ---------------------------------------------------------------- comparisons
def assert_equal(got, ref, what):
    """torch.equal with a message that says where. NaN never equals: an interior the kernel left unwritten fails here."""
    assert got.shape == ref.shape and got.dtype == ref.dtype, '%s: %s %s against %s %s' % (what, got.dtype, tuple(got.shape), ref.dtype, tuple(ref.shape))
    if torch.equal(got, ref):
        return
    bad = (got != ref) | torch.isnan(got)
    idx = torch.nonzero(bad)[0].tolist()
    raise AssertionError('%s: %d of %d elements differ, first at %s: got %r, reference %r'
                         % (what, int(bad.sum()), got.numel(), idx, float(got[tuple(idx)]), float(ref[tuple(idx)])))


class Guarded(object):
    """A (rows, cols) output with row stride ld inside a flat buffer: `pad` elements in front (pad + shift when the view is to start off the
    buffer's alignment) and behind, and the ld - cols pad columns of every row, hold GUARD; the interior starts as NaN or as `init`.
    guard=nan: the whole buffer is NaN (slab workspaces, which are only ever stored to)."""

    def __init__(self, rows, cols, dtype, device, ld=None, pad=64, shift=0, init=None, guard=GUARD):
        self.rows, self.cols, self.ld, self.guard = rows, cols, ld or cols, guard
        n, s = rows * self.ld, pad + shift
        self.start = s                                                         # element offset of the view in the buffer
        self.buf = torch.full((n + s + pad,), guard, dtype=dtype, device=device)
        self.inside = torch.zeros(n + s + pad, dtype=torch.bool, device=device)
        self.inside[s:s + n].view(rows, self.ld)[:, :cols] = True
        self.view = self.buf[s:s + n].view(rows, self.ld)[:, :cols]
        if init is None:
            self.view.fill_(float('nan'))
        else:
            self.view.copy_(init)

    def assert_guards(self, what):
        g = self.buf[~self.inside]
        ok = torch.isnan(g) if math.isnan(self.guard) else g == self.guard
        assert bool(ok.all()), '%s: %d guard elements written' % (what, int((~ok).sum()))

    def assert_untouched(self, what):
        self.assert_guards(what)
        assert bool(torch.isnan(self.view).all()), '%s: written by a call that must not write' % what


def kind3_figure(got, ref, scale, bf16, extra=None):
    """max over elements of (|got - ref| [- extra] [- 2^-8 |ref|]) / (2^-24 scale): the error in units of one float32 ulp of the element's
    cancellation-free sum. `extra`: an absolute allowance per element taken off first (the erf approximation)."""
    err = (got.double() - ref).abs()
    if extra is not None:
        err = err - extra
    if bf16:
        err = err - E8 * ref.abs()
    return float((err.clamp_min(0) / (E24 * scale).clamp_min(1e-300)).max())


# ---------------------------------------------------------------- the cost models of the two splits (pb_gemm2_try), mirrored
def tail_split_factor(M, N, K, ncu):
    """K ranges PB_GEMM_TAIL_SPLIT cuts the last round's tiles into on a chip of ncu CUs (1: the model turns the split down)."""
    ntile, nkt = -(-M // 256) * -(-N // 256), K // 64
    rem = ntile % ncu
    if rem == 0:
        return 1
    best, best_net = 1, 0.0
    for sp in range(2, min(ncu // rem, nkt // 3, 8) + 1):
        per = -(-nkt // sp)
        net = (nkt - per) - 1.3 * (5.0 + 0.105 * rem * sp) / 1.6
        if net > best_net:
            best, best_net = sp, net
    if best < 2:
        return 1
    per = -(-nkt // best)
    return -(-nkt // per)


def row_split_rows(M, N, K, ncu):
    """Rows PB_GEMM_ROW_SPLIT leaves with the 256 x 256 kernel (M: no split)."""
    tiles_n = -(-N // 256)
    ntile, nkt = -(-M // 256) * tiles_n, K // 64
    rounds, rem = ntile // ncu, ntile % ncu
    if M % 8 or rounds < 1 or rem == 0:
        return M
    m_main = (rounds * ncu // tiles_n) * 256
    m_rest = M - m_main
    t2 = -(-m_rest // 128) * -(-N // 128)
    r256 = 1.53 * nkt + 6.5
    r128 = (0.75 if t2 <= ncu else 1.0) * nkt + 4.0
    now = (rounds + 1) * r256
    then = rounds * r256 + -(-t2 // (2 * ncu)) * r128 + 2.0
    return m_main if (m_main >= 256 and m_rest > 0 and then < 0.92 * now) else M


# ---------------------------------------------------------------- the case table
LAYOUTS = [(True, True), (True, False), (False, True), (False, False)]          # NT, NN, TT, TN in (a_kc, b_kc)
T128 = dict(tile128=True)
T256 = dict(tile256=True)


def _k256(a_kc, b_kc, one_barrier=False):
    if a_kc == b_kc and not one_barrier:
        return 'pingpong', dict(T256)
    return 'onebar256', (dict(T256, dbg=2048) if a_kc == b_kc else dict(T256))


def _tile128_cases():
    out = []
    for a_kc, b_kc in LAYOUTS:
        sizes = [8, 120, 128, 136, 264]
        shapes = [(136, n, 128) for n in sizes] + [(m, 136, 128) for m in sizes if m != 136] + [(136, 136, 64), (136, 136, 192)]
        if a_kc:
            shapes += [(m, 136, 128) for m in (1, 5, 127, 129)]
        out += [Case(m, n, k, a_kc=a_kc, b_kc=b_kc, flags=T128, kernel='tile128') for m, n, k in shapes]
    return out


def _tile256_cases():
    out = []
    for a_kc, b_kc in LAYOUTS:
        for one_barrier in ((False, True) if a_kc == b_kc else (False,)):
            kernel, flags = _k256(a_kc, b_kc, one_barrier)
            sizes = [256, 264, 504, 512, 520]
            shapes = [(520, 520, 64 * t) for t in (1, 2, 3, 4, 5)] + [(264, n, 128) for n in sizes] + [(m, 264, 128) for m in sizes if m != 264]
            if a_kc:
                shapes += [(257, 264, 128), (511, 264, 128)]
            out += [Case(m, n, k, a_kc=a_kc, b_kc=b_kc, flags=flags, kernel=kernel) for m, n, k in shapes]
    return out


def _default_cases():
    return [Case(m, n, 128, a_kc=a_kc, b_kc=b_kc, kernel=('tile128' if (m < 2048 or n < 512) else 'pingpong' if a_kc == b_kc else 'onebar256'))
            for a_kc, b_kc in LAYOUTS for m in (2040, 2048) for n in (504, 512)]


EPI_SHAPES = [(512, 512), (264, 264), (520, 520)]                              # interior tiles only, edge tiles only, 4 interior + 5 edge
EPI_KERNELS = [('tile128', True, True, T128), ('pingpong', True, True, T256), ('pingpong', False, False, T256),
               ('onebar256', True, True, dict(T256, dbg=2048)), ('onebar256', True, False, T256), ('generic', True, True, dict(force_v1=True))]
EPI_LIST = ['store', 'bias', 'alpha', 'acc', 'acc32', 'c32', 'mul', 'mulcs']


def _epilogue_cases():
    out = []
    for kernel, a_kc, b_kc, flags in EPI_KERNELS:
        for m, n in EPI_SHAPES:
            out += [Case(m, n, 128, a_kc=a_kc, b_kc=b_kc, flags=flags, kernel=kernel, epi=e) for e in EPI_LIST]
    out += [Case(m, n, 96, dt='f32', epi=e, kernel='generic') for m, n in EPI_SHAPES[1:] for e in EPI_LIST]   # the f32 dtype, once: always the generic kernel
    return out


def _rowdot_cases():
    return [Case(m, n, 128, epi=e, kernel='pingpong') for m, n in ((512, 512), (768, 256)) for e in ('rowdot', 'rowdotb')]


def _kind3_cases():
    out = []
    for kernel, a_kc, b_kc, flags in EPI_KERNELS:
        out += [Case(520, 520, 320, a_kc=a_kc, b_kc=b_kc, flags=flags, kernel=kernel, epi=e) for e in ('real', 'real32')]   # bf16 C; f32 C, where nothing hides behind the bf16 ulp
        out += [Case(m, n, 128, a_kc=a_kc, b_kc=b_kc, flags=flags, kernel=kernel, epi='gelu') for m, n in EPI_SHAPES]
    out += [Case(264, 264, 100, dt='f32', epi=e, kernel='generic') for e in ('real', 'gelu')]
    out += [Case(264, 264, 448, a_kc=False, b_kc=False, flags=fl, kernel=k, splitk=3, epi='real') for k, fl in (('tile128', T128), ('pingpong', T256))]
    return out


SPLITS = [(4, 4), (7, 3), (5, 4), (9, 8), (8, 8)]                              # (K tiles, splits); (5, 4) -> 2, 2, 1, 0 and (9, 8) -> 2, 2, 2, 2, 1, 0, 0, 0 K tiles


def _splitk_cases():
    out = []
    for nkt, ns in SPLITS:
        for kernel, flags in (('tile128', T128), ('pingpong', T256)):
            for m, n in ((264, 136), (520, 264)):
                for accum in (False, True):                                    # (N = 136 < 256: PB_GEMM_TILE256 still gets the 128 x 128 kernel)
                    out.append(Case(m, n, 64 * nkt, a_kc=False, b_kc=False, flags=flags, kernel=kernel if n >= 256 else 'tile128', splitk=ns, accum=accum))
    out += [Case(520, 264, 64 * 5, flags=fl, kernel=k, splitk=4, accum=True) for k, fl in (('tile128', T128), ('pingpong', T256))]   # NT
    return out


def _ld_cases():
    out = []
    for (m, n), kflags in (((136, 136), [('tile128', T128)]), ((264, 264), [('256', T256)])):
        for a_kc, b_kc in LAYOUTS:
            for kernel, flags in kflags:
                if kernel == '256':
                    kernel, flags = _k256(a_kc, b_kc)
                kw = dict(a_kc=a_kc, b_kc=b_kc, flags=flags, kernel=kernel)
                out.append(Case(m, n, 128, lda_pad=8, ldb_pad=8, ldc_pad=8, epi='bias', **kw))
                out.append(Case(m, n, 128, lda_pad=8, ldb_pad=8, ldc_pad=8, a_off=8, b_off=16, c_off=8, epi='mul', ldaux_pad=24, **kw))
                out.append(Case(m, n, 128, lda_pad=8, ldb_pad=8, ldc_pad=8, c_off=16, epi='c32', **kw))
                out.append(Case(m, n, 128, nb1=2, nb2=3, lda_pad=8, ldc_pad=8, a_off=8, epi='acc', **kw))
                # one element off 16-byte alignment / an ld that is no multiple of 8: the tiled kernels decline, the generic kernel serves
                out.append(Case(m, n, 128, a_off=1, epi='bias', **dict(kw, kernel='generic')))
                out.append(Case(m, n, 128, b_off=1, **dict(kw, kernel='generic')))
                out.append(Case(m, n, 128, c_off=1, epi='acc', **dict(kw, kernel='generic')))
                out.append(Case(m, n, 128, lda_pad=4, epi='alpha', **dict(kw, kernel='generic')))
                out.append(Case(m, n, 128, ldb_pad=12, ldc_pad=3, **dict(kw, kernel='generic')))
    return out


def _generic_cases():
    out = []
    sizes = [1, 5, 127, 128, 129, 136]
    for dt, ks in (('bf16', [8, 56, 64, 72, 104]), ('f32', [4, 28, 32, 36, 100])):
        fl = dict(force_v1=True) if dt == 'bf16' else {}
        for a_kc, b_kc in LAYOUTS:
            shapes = [(129, 136, k) for k in ks] + [(m, 136, ks[3]) for m in sizes if m != 129] + [(129, n, ks[3]) for n in sizes if n != 136]
            out += [Case(m, n, k, a_kc=a_kc, b_kc=b_kc, dt=dt, flags=fl, kernel='generic', epi=('bias' if (m + n + k) % 2 else 'store')) for m, n, k in shapes]
            if dt == 'bf16':                                                   # the decline paths: K no multiple of 64, N no multiple of 8, M no multiple of 8 under a row-contiguous A
                out += [Case(136, 136, 72, a_kc=a_kc, b_kc=b_kc, kernel='generic'), Case(136, 132, 64, a_kc=a_kc, b_kc=b_kc, kernel='generic', epi='bias')]
                if not a_kc:
                    out.append(Case(132, 136, 64, a_kc=a_kc, b_kc=b_kc, kernel='generic'))
    return out


FAMILIES = dict(tile128=_tile128_cases(), tile256=_tile256_cases(), default=_default_cases(), epilogue=_epilogue_cases(), rowdot=_rowdot_cases(),
                kind3=_kind3_cases(), splitk=_splitk_cases(), ld=_ld_cases(), generic=_generic_cases())

# Several work items per persistent workgroup, and the two splits: the shapes depend on the chip (ncu), so the table holds makers.
PERSISTENT_EPIS = ['store', 'bias', 'alpha', 'acc', 'acc32', 'c32', 'mul', 'mulcs', 'rowdot', 'rowdotb', 'gelu']


def persistent_rows(ncu):
    """M (N = 512: two tile columns) for ncu + 2 tiles, whole, and for 2 ncu + 3 tiles -- rounded up to the 2 ncu + 4 that two tile columns allow -- with a
    ragged last tile row (the row dots take whole tiles only: they get it whole)."""
    return (ncu + 2) // 2 * 256, (2 * ncu + 4) // 2 * 256 - 248


def persistent_cases(ncu):
    out = []
    for i, m in enumerate(persistent_rows(ncu)):
        for e in PERSISTENT_EPIS:
            mm = -(-m // 256) * 256 if e.startswith('rowdot') else m
            for a_kc in ((True, False) if e in ('store', 'acc32', 'c32', 'mulcs') else (True,)):
                out.append(Case(mm, 512, 128, a_kc=a_kc, b_kc=a_kc, epi=e, kernel='pingpong', seed=i))
    return out


TAIL_SHAPES = [(26624, 768, 3072, True), (26880, 768, 2304, False)]            # (M, N, K, b_kc): NT and NN, the first two of test_gemm_tail_split_matches_whole_tiles
ROW_SHAPES = [(26624, 768, 768, True), (26880, 768, 2304, True)]               # the first two of test_gemm_row_split_matches_one_launch
SPLIT_EPIS = ['bias', 'acc', 'c32']


def split_cases():
    return [Case(m, n, k, b_kc=b_kc, epi=e, kernel='pingpong' if b_kc else 'onebar256') for m, n, k, b_kc in TAIL_SHAPES + ROW_SHAPES for e in SPLIT_EPIS]


def all_cases(ncu=256):
    return [c for f in FAMILIES.values() for c in f] + persistent_cases(ncu) + split_cases()
