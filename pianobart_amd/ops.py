"""Tensor-level wrappers over the C ABI (include/pianobart_hip.h). PyTorch is used only to own
device memory and the HIP stream; every op below launches a hand-written gfx950 kernel from
libpianobart_hip.so on torch's current stream. There is no fallback path."""
import ctypes
import math
import os

import torch

from ._lib import (LIB, PB_BF16, PB_F32, PB_F32X3, AttnDesc, GemmDesc, PBError, GEMM_ACCUM, GEMM_C_F32, GEMM_GELU,
                   GEMM_MUL_GELU_GRAD, GEMM_ROWDOT, ATTN_CAUSAL, ATTN_GENERIC, ATTN_ONE_PASS, FisherDesc, MergeDesc, MERGE_MAX_MODELS, MERGE_AVERAGE,
                   MERGE_DELTA, MERGE_MASK_NONE)

CLASS_NAMES = ('Bar', 'Position', 'Instrument', 'Pitch', 'Duration', 'Velocity', 'TimeSig', 'Tempo')   # PianoBart.classes order
SPECIAL_TAGS = ('PAD', 'MASK', 'SOS', 'EOS', 'CLS', 'SEP')  # the six special ids of a head: its last six, in this order
HEAD_MIN, HEAD_MAX = 7, 64 * 17                             # six specials and one class .. the wide sampler / score kernels' 17 classes per lane


class Layout:
    """The vocabulary layout of one Octuple dictionary: a property of the model, handed to the kernels at run time (they take segment
    offsets, sizes and pad ids as arguments). sizes: the 8 head sizes in CLASS_NAMES order; specials: per head the six special ids
    (SPECIAL_TAGS order), None = the last six of the head. Immutable. A head outside HEAD_MIN .. HEAD_MAX classes, or specials that
    are not the head's last six ids with PAD first, raise PBError here: on the host, before any device work.
      seg_off[9]   start of every head in a logits row (seg_off[8] = vocab, the row's width and stride)
      tab_rows     rows of one slot of the projected Octuple table: the largest head rounded up to a multiple of 8, so the per-stream
                   table GEMMs are ONE batched launch with uniform strides; tab_off[9] / tab_total = 8 such slots
      pad8         the first special id of every head (an id >= pad8[h] ends a generated piece)
      seg9 / tab9  seg_off / tab_off as ctypes int32[9]"""
    _FIELDS = ('sizes', 'specials', 'seg_off', 'vocab', 'tab_rows', 'tab_off', 'tab_total', 'pad8', 'seg9', 'tab9')
    __slots__ = _FIELDS + ('_hash',)

    def __init__(self, sizes, specials=None):
        try:
            sizes = tuple(int(n) for n in sizes)
        except (TypeError, ValueError):
            raise PBError('Layout: sizes must be 8 integers (got %r)' % (sizes,))
        if len(sizes) != 8:
            raise PBError('Layout: %d heads; the Octuple layout has 8 (%s)' % (len(sizes), ', '.join(CLASS_NAMES)))
        for h, n in enumerate(sizes):
            if not HEAD_MIN <= n <= HEAD_MAX:
                raise PBError('Layout: head %d (%s) has %d classes; a head needs %d .. %d (its six special ids and at least one class; '
                              'the kernels hold at most 64 x 17 classes of a head)' % (h, CLASS_NAMES[h], n, HEAD_MIN, HEAD_MAX))
        if specials is None:
            specials = [range(n - 6, n) for n in sizes]
        specials = tuple(tuple(int(v) for v in sp) for sp in specials)
        if len(specials) != 8:
            raise PBError('Layout: special ids of %d heads for 8' % len(specials))
        for h, (n, sp) in enumerate(zip(sizes, specials)):
            if sp != tuple(range(n - 6, n)):
                raise PBError('Layout: head %d (%s): the special ids <%s> = %s must be the last six ids of the head, %d .. %d in this order '
                              '(the stop rule is "an id >= <PAD>")' % (h, CLASS_NAMES[h], '> <'.join(SPECIAL_TAGS), list(sp), n - 6, n - 1))
        seg_off = [0]
        for n in sizes:
            seg_off.append(seg_off[-1] + n)
        tab_rows = (max(sizes) + 7) // 8 * 8
        tab_off = tuple(tab_rows * i for i in range(9))
        for k, v in zip(self._FIELDS, (sizes, specials, tuple(seg_off), seg_off[-1], tab_rows, tab_off, tab_off[8], tuple(sp[0] for sp in specials),
                                       (ctypes.c_int32 * 9)(*seg_off), (ctypes.c_int32 * 9)(*tab_off))):
            object.__setattr__(self, k, v)
        object.__setattr__(self, '_hash', hash((sizes, specials)))      # a layout keys per-thread scratch on the sampling path

    @classmethod
    def from_dict(cls, e2w):
        """The layout of a dictionary's event -> word half (the reference's e2w): 8 classes under the reference's names, each with its six
        special words '<class> <TAG>'. PBError names the class and the rule that a dictionary breaks."""
        try:
            keys = list(e2w.keys())
        except AttributeError:
            raise PBError('Layout: the dictionary must map class names to {word: id} tables (got %s)' % type(e2w).__name__)
        if len(keys) != 8 or set(keys) != set(CLASS_NAMES):
            raise PBError('Layout: the dictionary has the classes %s; the Octuple layout needs exactly %s' % (keys, list(CLASS_NAMES)))
        sizes, specials = [], []
        for h, name in enumerate(CLASS_NAMES):
            tab = e2w[name]
            sizes.append(len(tab))
            sp = []
            for tag in SPECIAL_TAGS:
                word = '%s <%s>' % (name, tag)
                if word not in tab:
                    raise PBError('Layout: head %d (%s) has no special word %r (every head needs <%s>)' % (h, name, word, '> <'.join(SPECIAL_TAGS)))
                sp.append(int(tab[word]))
            specials.append(sp)
        return cls(sizes, specials)

    def __setattr__(self, k, v):
        raise AttributeError('Layout is immutable')

    __delattr__ = __setattr__

    def __reduce__(self):                # copy / pickle rebuild it (the ctypes arrays do not pickle)
        return (Layout, (self.sizes, self.specials))

    def __eq__(self, other):
        return isinstance(other, Layout) and self.sizes == other.sizes and self.specials == other.specials

    def __hash__(self):
        return self._hash

    def __repr__(self):
        return 'Layout(sizes=%s)' % list(self.sizes)


# Today's dictionary (data/octuple_vocab.json). The module globals below are its fields under their earlier names: the `layout=None` of
# every wrapper means this one.
DEFAULT_LAYOUT = Layout([262, 134, 135, 262, 134, 38, 260, 55])
SEG_SIZES = list(DEFAULT_LAYOUT.sizes)                      # PianoBart.classes order
SEG_OFF = list(DEFAULT_LAYOUT.seg_off)
VOCAB = DEFAULT_LAYOUT.vocab                                # 1280
_SEG9 = DEFAULT_LAYOUT.seg9
# the projected Octuple table keeps every stream in a fixed 264-row slot (max vocabulary 262, padded to a multiple of 8) so the
# per-stream table GEMMs are ONE batched launch with uniform strides
TAB_ROWS = DEFAULT_LAYOUT.tab_rows                          # 264
TAB_OFF = list(DEFAULT_LAYOUT.tab_off)
TAB_TOTAL = DEFAULT_LAYOUT.tab_total                        # 2112
_TAB9 = DEFAULT_LAYOUT.tab9


def _off9(layout, padded):
    layout = layout or DEFAULT_LAYOUT
    return layout.tab9 if padded else layout.seg9


def seg_array(offsets):
    return (ctypes.c_int32 * len(offsets))(*offsets)


def dtype_code(t):
    if t == torch.float32:
        return PB_F32
    if t == torch.bfloat16:
        return PB_BF16
    raise PBError('unsupported storage dtype %s' % t)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise PBError('pianobart_amd ops need HIP device tensors (got %s); there is no CPU path' % t.device)
    return ctypes.c_void_p(t.data_ptr())


def _adr(t):
    """_p(t) as a plain address for a descriptor field (None stays None): a tensor that is not on the device is refused alike."""
    p = _p(t)
    return None if p is None else p.value


# developer aid for same-box A/B runs (tools/ab_step.sh): extra flag bits for every GEMM, e.g. PB_GEMM_FLAGS=4096 = ordinary grids
_ENV_GEMM_FLAGS = int(os.environ.get('PB_GEMM_FLAGS', '0'))


def gemm(A, B, C, *, M, N, K, dtype, a_kc=True, b_kc=True, lda=None, ldb=None, ldc=None, bias=None, alpha=1.0,
         accum=False, c_f32=False, gelu_aux_out=None, gelu_grad_aux_in=None, ldaux=0, nb1=1, nb2=1,
         sA=(0, 0), sB=(0, 0), sC=(0, 0), a_off=0, b_off=0, c_off=0, splitk=1, slabs=None, force_v1=False, tile128=False, tile256=False, dbg=0,
         colsum_out=None, colsum_ws=None, rowdot=None):
    """C[m,n] (+)= epi(alpha * sum_k A(m,k) B(n,k)). a_off/b_off/c_off are element offsets into the tensors.
    rowdot = (aux (M, N) storage dtype, out (N / 64, ld) f32, ld): PB_GEMM_ROWDOT, out[n / 64][m] = sum over the 64-column group of C * aux."""
    d = GemmDesc()
    esz = 2 if dtype == PB_BF16 else 4
    d.A = A.data_ptr() + a_off * esz
    d.B = B.data_ptr() + b_off * esz
    d.C = C.data_ptr() + c_off * (4 if c_f32 else esz)
    d.bias = bias.data_ptr() if bias is not None else None
    d.aux_in = gelu_grad_aux_in.data_ptr() if gelu_grad_aux_in is not None else None
    d.aux_out = gelu_aux_out.data_ptr() if gelu_aux_out is not None else None
    d.dtype, d.a_kcontig, d.b_kcontig = dtype, int(a_kc), int(b_kc)
    d.flags = (GEMM_ACCUM if accum else 0) | (GEMM_C_F32 if c_f32 else 0) | \
              (GEMM_GELU if gelu_aux_out is not None else 0) | (GEMM_MUL_GELU_GRAD if gelu_grad_aux_in is not None else 0) | \
              (16 if force_v1 else 0) | (32 if tile128 else 0) | (64 if tile256 else 0) | dbg | _ENV_GEMM_FLAGS
    d.splitk = splitk if (splitk > 1 and slabs is not None) else 1
    d.slabs = slabs.data_ptr() if (splitk > 1 and slabs is not None) else None
    d.colsum_out = colsum_out.data_ptr() if colsum_out is not None else None
    d.colsum_ws = colsum_ws.data_ptr() if colsum_ws is not None else None
    if rowdot is not None:
        d.aux_in, d.rowdot_out, d.ld_rowdot = rowdot[0].data_ptr(), rowdot[1].data_ptr(), rowdot[2]
        d.flags |= GEMM_ROWDOT
    d.M, d.N, d.K, d.nb1, d.nb2 = M, N, K, nb1, nb2
    d.lda = lda if lda is not None else (K if a_kc else M)
    d.ldb = ldb if ldb is not None else (K if b_kc else N)
    d.ldc = ldc if ldc is not None else N
    d.ldaux = ldaux or d.ldc
    d.sA1, d.sA2 = sA
    d.sB1, d.sB2 = sB
    d.sC1, d.sC2 = sC
    d.alpha = alpha
    if not (A.is_cuda and B.is_cuda and C.is_cuda):
        raise PBError('gemm needs HIP device tensors; there is no CPU path')
    LIB.call('pb_gemm', ctypes.byref(d), _stream())


def linear_fwd(x, w, bias, out, dtype, **kw):
    """out (T,N) = x (T,K) @ w(N,K)^T + bias."""
    T, K = x.shape
    N = w.shape[0]
    gemm(x, w, out, M=T, N=N, K=K, dtype=dtype, bias=bias, **kw)


def ids_to_i16(ids):
    out = torch.empty(ids.shape, dtype=torch.int16, device=ids.device)
    ids = ids.contiguous()
    if ids.dtype != torch.int64:
        ids = ids.long()
    LIB.call('pb_ids_to_i16', _p(ids), _p(out), ids.numel(), _stream())
    return out


def ids_check(ids16, limits, flag):
    """flag (device int32[1]) |= 1 if any of the (..., 8) int16 ids lies outside [0, limits[column])."""
    LIB.call('pb_ids_check', _p(ids16), ids16.numel(), _p(limits), _p(flag), _stream())


def embed_ln_fwd(ids16, P, lin_bias, pos, ln_w, ln_b, y, mean, rstd, S, eps, seed, site, p_drop, padded=False, row_ids=None, layout=None):
    T, d = y.shape
    if row_ids is not None:
        LIB.call('pb_embed_ln_fwd_packed', _p(ids16), _p(row_ids), _p(P), _off9(layout, padded), _p(lin_bias), _p(pos), _p(ln_w), _p(ln_b),
                 _p(y), _p(mean), _p(rstd), T, S, d, dtype_code(y.dtype), eps, seed, site, p_drop, _stream())
        return
    LIB.call('pb_embed_ln_fwd', _p(ids16), _p(P), _off9(layout, padded), _p(lin_bias), _p(pos), _p(ln_w), _p(ln_b), _p(y), _p(mean),
             _p(rstd), T, S, d, dtype_code(y.dtype), eps, seed, site, p_drop, _stream())


def embed_ln_bwd(dy, ids16, P, lin_bias, pos, ln_w, mean, rstd, dP, dpos, dbias, dgamma, dbeta, partials, S, seed, site, p_drop,
                 dz_out=None, padded=False, row_ids=None, layout=None):
    T, d = dy.shape
    if row_ids is not None:
        LIB.call('pb_embed_ln_bwd_packed', _p(dy), _p(ids16), _p(row_ids), _p(P), _off9(layout, padded), _p(lin_bias), _p(pos), _p(ln_w),
                 _p(mean), _p(rstd), _p(dP), _p(dpos), _p(dbias), _p(dgamma), _p(dbeta), _p(partials), _p(dz_out), T, S, d,
                 dtype_code(dy.dtype), seed, site, p_drop, _stream())
        return
    LIB.call('pb_embed_ln_bwd', _p(dy), _p(ids16), _p(P), _off9(layout, padded), _p(lin_bias), _p(pos), _p(ln_w), _p(mean), _p(rstd),
             _p(dP), _p(dpos), _p(dbias), _p(dgamma), _p(dbeta), _p(partials), _p(dz_out), T, S, d, dtype_code(dy.dtype), seed, site,
             p_drop, _stream())


def split_bf16(x, hi, lo):
    """x (f32) -> hi = bf16(x), lo = bf16(x - hi) (pb_split_bf16)."""
    LIB.call('pb_split_bf16', _p(x), _p(hi), _p(lo), x.numel(), _stream())


def onehot_build(ids16, out, padded=False, layout=None):
    layout = layout or DEFAULT_LAYOUT
    LIB.call('pb_onehot_build', _p(ids16), _off9(layout, padded), _p(out), ids16.numel() // 8, layout.tab_total if padded else layout.vocab, _stream())


def batch_sum(x, out, B, Sd):
    LIB.call('pb_batch_sum', _p(x), _p(out), B, Sd, dtype_code(x.dtype), _stream())


def add_ln_fwd(res, a, ln_w, ln_b, y, mean, rstd, eps, seed, site, p_drop, row_ids=None):
    T, d = y.shape
    if row_ids is not None:
        LIB.call('pb_add_ln_fwd_packed', _p(res), _p(a), _p(ln_w), _p(ln_b), _p(y), _p(mean), _p(rstd), _p(row_ids), T, d, dtype_code(y.dtype),
                 eps, seed, site, p_drop, _stream())
        return
    LIB.call('pb_add_ln_fwd', _p(res), _p(a), _p(ln_w), _p(ln_b), _p(y), _p(mean), _p(rstd), T, d, dtype_code(y.dtype),
             eps, seed, site, p_drop, _stream())


def add_ln_bwd(dy, res, a, ln_w, mean, rstd, dres, da, dgamma, dbeta, dbias_a, partials, accum_dres, seed, site, p_drop, row_ids=None):
    T, d = dy.shape
    if row_ids is not None:
        LIB.call('pb_add_ln_bwd_packed', _p(dy), _p(res), _p(a), _p(ln_w), _p(mean), _p(rstd), _p(dres), _p(da), _p(dgamma), _p(dbeta),
                 _p(dbias_a), _p(partials), _p(row_ids), T, d, dtype_code(dy.dtype), int(dres.dtype == torch.float32 and dy.dtype != torch.float32),
                 int(accum_dres), seed, site, p_drop, _stream())
        return
    LIB.call('pb_add_ln_bwd', _p(dy), _p(res), _p(a), _p(ln_w), _p(mean), _p(rstd), _p(dres), _p(da), _p(dgamma), _p(dbeta),
             _p(dbias_a), _p(partials), T, d, dtype_code(dy.dtype), int(dres.dtype == torch.float32 and dy.dtype != torch.float32),
             int(accum_dres), seed, site, p_drop, _stream())


def colsum(dy, out, partials, T, N, ld=None):
    LIB.call('pb_colsum', _p(dy), ld if ld is not None else N, _p(out), _p(partials), T, N,
             PB_F32 if dy.dtype == torch.float32 else PB_BF16, int(dy.dtype == torch.float32), _stream())


def colsum_any(dy, out, partials, T, N, ld=None):
    """colsum for any N and ld (pb_colsum_any: one column per thread); pb_colsum needs multiples of 4."""
    LIB.call('pb_colsum_any', _p(dy), ld if ld is not None else N, _p(out), _p(partials), T, N,
             PB_F32 if dy.dtype == torch.float32 else PB_BF16, int(dy.dtype == torch.float32), _stream())


def softmax_fwd(scores, key_mask, P, B, H, Sq, Sk, scale, causal):
    LIB.call('pb_softmax_fwd', _p(scores), _p(key_mask), _p(P), B, H, Sq, Sk, scale, int(causal), dtype_code(P.dtype), _stream())


def softmax_bwd(dP, P, dS, rows, Sk, scale):
    LIB.call('pb_softmax_bwd', _p(dP), _p(P), _p(dS), rows, Sk, scale, dtype_code(P.dtype), _stream())


def ce_fwd_bwd(logits, target16, loss_mask, sums, partials, coef, dlogits, argmax_out, layout=None):
    T, V = logits.shape
    LIB.call('pb_ce_fwd_bwd', _p(logits), _p(target16), _p(loss_mask), _off9(layout, False), _p(sums), _p(partials), _p(coef), _p(dlogits),
             _p(argmax_out), T, V, dtype_code(dlogits.dtype) if dlogits is not None else PB_F32, _stream())


def distill_fwd_bwd(logits, teacher, t_row, target16, loss_mask, sums, partials, coef, dlogits, argmax_out, alpha, tau, eps, layout=None):
    """pb_distill_fwd_bwd: ce_fwd_bwd with soft targets. teacher (T_t, V) f32 or None; t_row (T,) int32 (the teacher row of every student
    row) or None; sums (40,) f32 = (5, 8) {loss, m, correct, hard CE, KL}, accumulated into; partials >= pb_distill_partials_floats()."""
    T, V = logits.shape
    if teacher is not None and (teacher.dim() != 2 or teacher.shape[1] != V or teacher.dtype != torch.float32 or not teacher.is_contiguous()):
        raise PBError('distill_fwd_bwd: teacher logits must be a contiguous (T_t, %d) float32 tensor (got %s %s)' % (V, tuple(teacher.shape), teacher.dtype))
    if t_row is not None and (t_row.dtype != torch.int32 or t_row.numel() < T):
        raise PBError('distill_fwd_bwd: t_row must hold %d int32 row numbers (got %d of %s)' % (T, t_row.numel(), t_row.dtype))
    LIB.call('pb_distill_fwd_bwd', _p(logits), _p(teacher), _p(t_row), _p(target16), _p(loss_mask), _off9(layout, False), _p(sums), _p(partials),
             _p(coef), _p(dlogits), _p(argmax_out), T, teacher.shape[0] if teacher is not None else 0, V,
             dtype_code(dlogits.dtype) if dlogits is not None else PB_F32, float(alpha), float(tau), float(eps), _stream())


def token_scores(logits, target16, mask, logp, entropy=None, rank=None, layout=None):
    """pb_token_scores: logits (T, V) f32, target16 (T, 8) int16, mask (T,) f32 of 0 / 1 -> logp / entropy (T, 8) f32, rank (T, 8) int16
    (entropy and rank may be None)."""
    T, V = logits.shape
    LIB.call('pb_token_scores', _p(logits), _p(target16), _p(mask), _off9(layout, False), _p(logp), _p(entropy), _p(rank), T, V, _stream())


def seq_scores(logp, entropy, rank, mask, out):
    """pb_seq_scores: the (B * S, 8) outputs of token_scores and mask (B, S) -> out (B, 4, 8) f32 = per sequence and head
    {sum mask * logp, sum mask * entropy, sum mask * [rank == 0], sum mask}."""
    B, S = mask.shape
    LIB.call('pb_seq_scores', _p(logp), _p(entropy), _p(rank), _p(mask), _p(out), B, S, _stream())


def mask_count(loss_mask, counts, partials):
    LIB.call('pb_mask_count', _p(loss_mask), _p(counts), _p(partials), loss_mask.numel() // 8, _stream())


def loss_coef(counts, w, coef, scale=1.0):
    LIB.call('pb_loss_coef', _p(counts), _p(w), _p(coef), scale, _stream())


def grad_sqnorm(g, partials, out_sq):
    LIB.call('pb_grad_sqnorm', _p(g), g.numel(), _p(partials), _p(out_sq), _stream())


def clip_coef(sq, max_norm, gscale, coef):
    LIB.call('pb_clip_coef', _p(sq), max_norm, gscale, _p(coef), _stream())


def adamw_step(p, g, m, v, shadow, clip, lr, beta1, beta2, eps, weight_decay, step):
    LIB.call('pb_adamw_step', _p(p), _p(g), _p(m), _p(v), _p(shadow), p.numel(), _p(clip), lr, beta1, beta2, eps,
             weight_decay, step, _stream())


def cast_f32_to_bf16(src, dst):
    LIB.call('pb_cast_f32_to_bf16', _p(src), _p(dst), src.numel(), _stream())


def cast_bf16_to_f32(src, dst):
    LIB.call('pb_cast_bf16_to_f32', _p(src), _p(dst), src.numel(), _stream())


def sum_rows_bf16(src, dst, rows):
    LIB.call('pb_sum_rows_bf16', _p(src), _p(dst), rows, dst.numel(), _stream())


def accum_f32(dst, src, add=True):
    """pb_accum_f32 over two contiguous f32 tensors of one size (views into flat buffers included): dst += src, or dst = src with add=False."""
    if dst.dtype != torch.float32 or src.dtype != torch.float32 or dst.numel() != src.numel() or not (dst.is_contiguous() and src.is_contiguous()):
        raise PBError('accum_f32 needs two contiguous f32 tensors of the same size')
    LIB.call('pb_accum_f32', _p(dst), _p(src), dst.numel(), int(bool(add)), _stream())


def _flat_f32(t, what):
    if t.dtype != torch.float32 or t.dim() != 1 or not t.is_contiguous():
        raise PBError('%s must be a contiguous 1-D f32 tensor' % what)
    return _p(t).value


def merge_kth_ws(device):
    """The state of one pb_merge_kth_abs call (reusable by the next call on the same stream)."""
    return torch.empty((LIB.query('pb_merge_kth_ws_bytes') + 7) // 8, dtype=torch.int64, device=device)


def merge_kth_abs(x, base, k, kth_out, flags, ws):
    """kth_out[0] = the exact k-th smallest of |x - base| (base None: |x|), 1 <= k <= x.numel(); x / base are flat f32 tensors or views into
    them. flags (int32[1], zeroed by the caller) gets bit 0 when a magnitude is inf or NaN. Nothing comes back to the host."""
    if base is not None and base.numel() != x.numel():
        raise PBError('merge_kth_abs: x and base differ in size')
    if kth_out.dtype != torch.float32 or flags.dtype != torch.int32:
        raise PBError('merge_kth_abs: kth_out is f32, flags int32')
    LIB.call('pb_merge_kth_abs', _flat_f32(x, 'x'), None if base is None else _flat_f32(base, 'base'), x.numel(), int(k), _p(kth_out), _p(flags), _p(ws), _stream())


def merge_desc(pre, models, out=None, *, method=MERGE_AVERAGE, fmt=MERGE_DELTA, lam=1.0, kinds=None, thresh=None, drop_thresh=None,
               rescale=None, tally=None, seed=0, g0=0, model_base=0):
    """A pb_merge_desc over flat f32 tensors (or equal views of them: a segment that starts at element g0 of the whole vector). kinds /
    thresh (one-element f32 device tensors or None) / drop_thresh (ints) / rescale (the divisor float32(1 - rate); 1 = none) are per model;
    model_base = the index of models[0] in the whole merge (its random mask stream)."""
    N = len(models)
    if N > MERGE_MAX_MODELS:
        raise PBError('merging takes at most %d models at a time (got %d)' % (MERGE_MAX_MODELS, N))
    d = MergeDesc()
    d.pre, d.n = _flat_f32(pre, 'pre'), pre.numel()
    if out is not None:
        if out.numel() != pre.numel():
            raise PBError('merge: out and pre differ in size')
        d.out = _flat_f32(out, 'out')
    for m, f in enumerate(models):
        if f.numel() != pre.numel():
            raise PBError('merge: model %d and pre differ in size' % m)
        d.model[m] = _flat_f32(f, 'model %d' % m)
        d.mask_kind[m] = kinds[m] if kinds else MERGE_MASK_NONE
        d.thresh[m] = _adr(thresh[m]) if thresh and thresh[m] is not None else None
        d.drop_thresh[m] = int(drop_thresh[m]) if drop_thresh else 0
        d.rescale[m] = float(rescale[m]) if rescale else 1.0
    d.tally = _adr(tally)
    d.g0, d.seed = int(g0), int(seed) & 0xFFFFFFFFFFFFFFFF
    d.n_models, d.method, d.format, d.lam, d.model_base = N, method, fmt, float(lam), int(model_base)
    return d


def merge_sign_tally(desc):
    """TIES pass 1: desc.tally (int64[2], zeroed by the caller) += the counts of positive and negative summed signs."""
    LIB.call('pb_merge_sign_tally', ctypes.byref(desc), _stream())


def merge_apply(desc):
    LIB.call('pb_merge_apply', ctypes.byref(desc), _stream())


def fisher_rows(logits, weight, e_out, dlogits):
    """pb_fisher_rows over logits (rows, C) f32: e_out[row] = sum_c sqrt(p_c) log p_c; dlogits (None: not wanted) = weight[row] * dE/dlogits
    with sqrt(p) held constant (weight None = 1)."""
    rows, C = logits.shape
    for t, what in ((logits, 'logits'), (weight, 'weight'), (e_out, 'e_out'), (dlogits, 'dlogits')):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise PBError('fisher_rows: %s must be a contiguous f32 tensor' % what)
    if e_out.numel() != rows or (weight is not None and weight.numel() != rows) or (dlogits is not None and dlogits.shape != logits.shape):
        raise PBError('fisher_rows: e_out / weight hold one value per row, dlogits has the shape of logits')
    LIB.call('pb_fisher_rows', _p(logits), _p(weight), _p(e_out), _p(dlogits), rows, C, _stream())


def fisher_accum(F, g):
    """F += g * g (two roundings) over two flat f32 tensors of one size, or equal views of them."""
    if F.numel() != g.numel():
        raise PBError('fisher_accum: F and g differ in size')
    LIB.call('pb_fisher_accum', _flat_f32(F, 'F'), _flat_f32(g, 'g'), F.numel(), _stream())


def fisher_finish(F, divisor, flags):
    """F /= float32(divisor); flags (int32[1], zeroed by the caller) gets bit 0 where a result is not finite."""
    if flags.dtype != torch.int32:
        raise PBError('fisher_finish: flags is int32')
    LIB.call('pb_fisher_finish', _flat_f32(F, 'F'), F.numel(), int(divisor), _p(flags), _stream())


def fisher_norm_ws(device):
    return torch.empty((LIB.query('pb_fisher_norm_ws_bytes') + 7) // 8, dtype=torch.float64, device=device)


def fisher_norm(F, ws, norm_out):
    """norm_out[0] = float32(sqrt(float64 sum of F^2)), in an order that depends on F.numel() alone."""
    if norm_out.dtype != torch.float32 or ws.dtype != torch.float64:
        raise PBError('fisher_norm: norm_out is f32, ws the float64 tensor of fisher_norm_ws')
    LIB.call('pb_fisher_norm', _flat_f32(F, 'F'), F.numel(), _p(ws), _p(norm_out), _stream())


def fisher_desc(models, fishers, out, coef, minimal):
    """A pb_fisher_desc over flat f32 tensors (or equal views of them); coef: one float32 per model, minimal: float32."""
    N = len(models)
    if N > MERGE_MAX_MODELS:
        raise PBError('merging takes at most %d models at a time (got %d)' % (MERGE_MAX_MODELS, N))
    if len(fishers) != N or len(coef) != N:
        raise PBError('fisher merge: %d models, %d Fisher vectors, %d coefficients' % (N, len(fishers), len(coef)))
    d = FisherDesc()
    d.out, d.n = _flat_f32(out, 'out'), out.numel()
    for m in range(N):
        if models[m].numel() != out.numel() or fishers[m].numel() != out.numel():
            raise PBError('fisher merge: model %d or its Fisher vector and out differ in size' % m)
        d.model[m], d.fisher[m], d.coef[m] = _flat_f32(models[m], 'model %d' % m), _flat_f32(fishers[m], 'fisher %d' % m), float(coef[m])
    d.minimal, d.n_models = float(minimal), N
    return d


def fisher_merge(desc):
    LIB.call('pb_fisher_merge', ctypes.byref(desc), _stream())


def _mat_f32(t, rows, cols, what):
    """(address, leading dimension) of a 2-D f32 device tensor of `rows` x `cols` whose rows are contiguous (a column slice of a wider buffer is one)."""
    if t.dtype != torch.float32 or t.dim() != 2 or tuple(t.shape) != (rows, cols) or t.stride(1) != 1 or (rows > 1 and t.stride(0) < cols):
        raise PBError('%s must be a (%d, %d) f32 tensor with contiguous rows (got %s %s, strides %s)' % (what, rows, cols, tuple(t.shape), t.dtype, t.stride()))
    return _p(t), (t.stride(0) if rows > 1 else cols)


def gram_ws(T, K, device):
    """The workspace of one gram_accum call over (T, K) activations (reusable by the next call of that size on the same stream)."""
    return torch.empty(max(1, LIB.query('pb_gram_ws_bytes', int(T), int(K)) // 4), dtype=torch.float32, device=device)


def gram_accum(G, X, ws=None):
    """G (K, K) f32 += X^T X for X (T, K) bf16 or f32 with contiguous rows; G comes out symmetric bit for bit. ws: gram_ws(T, K, device)."""
    if X.dim() != 2 or X.stride(1) != 1 or (X.shape[0] > 1 and X.stride(0) < X.shape[1]):
        raise PBError('gram_accum: X must be a (T, K) tensor with contiguous rows')
    T, K = X.shape
    g, ldg = _mat_f32(G, K, K, 'gram_accum: G')
    if ws is None:
        ws = gram_ws(T, K, X.device)
    if ws.dtype != torch.float32 or ws.numel() * 4 < LIB.query('pb_gram_ws_bytes', T, K):
        raise PBError('gram_accum: ws is smaller than pb_gram_ws_bytes(%d, %d)' % (T, K))
    LIB.call('pb_gram_accum', _p(X), X.stride(0) if T > 1 else K, dtype_code(X.dtype), T, K, g, ldg, _p(ws), _stream())


def regmean_scale(G, out, off, diag):
    """out = G * (diag on the diagonal, off elsewhere); out may be G."""
    K = G.shape[0]
    g, ldg = _mat_f32(G, K, K, 'regmean_scale: G')
    o, ldo = _mat_f32(out, K, K, 'regmean_scale: out')
    LIB.call('pb_regmean_scale', g, ldg, o, ldo, K, float(off), float(diag), _stream())


def chol_factor(A, info):
    """A (K, K) f32 -> its lower Cholesky factor in place (strict upper triangle 0). info (int32[1], zeroed by the caller) becomes 1 + j
    for the first pivot j that is <= 0 or not finite if it still holds 0."""
    K = A.shape[0]
    a, ld = _mat_f32(A, K, K, 'chol_factor: A')
    if info.dtype != torch.int32 or info.numel() != 1:
        raise PBError('chol_factor: info is one int32')
    LIB.call('pb_chol_factor', a, ld, K, _p(info), _stream())


def chol_solve(L, R):
    """R (K, nrhs) f32 -> Z with L L^T Z = R, in place."""
    K = L.shape[0]
    l, ldl = _mat_f32(L, K, K, 'chol_solve: L')
    if R.dim() != 2:
        raise PBError('chol_solve: R must be (K, nrhs)')
    r, ldr = _mat_f32(R, K, R.shape[1], 'chol_solve: R')
    LIB.call('pb_chol_solve', l, ldl, K, r, ldr, R.shape[1], _stream())


def transpose_f32(src, dst):
    """dst (cols, rows) = src (rows, cols)^T, a copy on the device."""
    if src.dim() != 2:
        raise PBError('transpose_f32: src must be 2-D')
    rows, cols = src.shape
    s, lds = _mat_f32(src, rows, cols, 'transpose_f32: src')
    d, ldd = _mat_f32(dst, cols, rows, 'transpose_f32: dst')
    LIB.call('pb_transpose_f32', s, lds, d, ldd, rows, cols, _stream())


FEATURE_COLS = 288                                          # the row of pb_piece_features


def _dense(t, dtype, dim, what):
    if t.dtype != dtype or t.dim() != dim or not t.is_contiguous():
        raise PBError('%s must be a contiguous %d-D %s tensor (got %s %s)' % (what, dim, str(dtype).replace('torch.', ''), tuple(t.shape), t.dtype))
    return _p(t)


def _pieces(who, max_S, ids16, pitch_of, start, layout):
    """The arguments the five piece_* wrappers share, checked: (ids16, start, pad8, pitch_of) as the entries take them, then N and S.
    who: the wrapper's name; max_S: its largest S (None: no limit of its own)."""
    layout = layout or DEFAULT_LAYOUT
    p_ids = _dense(ids16, torch.int16, 3, who + ': ids16')
    N, S = ids16.shape[0], ids16.shape[1]
    if ids16.shape[2] != 8 or S < 1 or (max_S is not None and S > max_S):
        raise PBError('%s: ids16 must be (N, S, 8) with %s (got %s)' % (who, 'S >= 1' if max_S is None else '1 <= S <= %d' % max_S, tuple(ids16.shape)))
    p_pitch = _dense(pitch_of, torch.int16, 1, who + ': pitch_of')
    if pitch_of.numel() != layout.pad8[3]:
        raise PBError('%s: pitch_of holds %d entries, the layout has %d pitch ids' % (who, pitch_of.numel(), layout.pad8[3]))
    p_start = None
    if start is not None:
        p_start = _dense(start, torch.int32, 1, who + ': start')
        if start.numel() != N:
            raise PBError('%s: start holds %d entries for %d pieces' % (who, start.numel(), N))
    return (p_ids, p_start, seg_array(layout.pad8), p_pitch), N, S


def piece_features(ids16, pitch_of, dur_pos, start=None, layout=None):
    """pb_piece_features: the (N, 288) int32 feature rows of ids16 (N, S, 8) int16. pitch_of (int16, layout.pad8[3] entries: the MIDI number
    of a pitch id, -1 = percussion) and dur_pos (int32, layout.pad8[4] entries) are device tables; start (N) int32 or None = 0."""
    shared, N, S = _pieces('piece_features', None, ids16, pitch_of, start, layout)
    p_dur = _dense(dur_pos, torch.int32, 1, 'piece_features: dur_pos')
    n_dur = (layout or DEFAULT_LAYOUT).pad8[4]
    if dur_pos.numel() != n_dur:
        raise PBError('piece_features: dur_pos holds %d entries, the layout has %d duration ids' % (dur_pos.numel(), n_dur))
    feat = torch.empty((N, FEATURE_COLS), dtype=torch.int32, device=ids16.device)
    LIB.call('pb_piece_features', *shared, p_dur, _p(feat), N, S, _stream())
    return feat


def pairwise_l2(A, B, out=None):
    """pb_pairwise_l2: D (N, M) f32 with D[i, j] = |A[i] - B[j]| for A (N, F), B (M, F) f32, 1 <= F <= 144."""
    pa, pb = _dense(A, torch.float32, 2, 'pairwise_l2: A'), _dense(B, torch.float32, 2, 'pairwise_l2: B')
    if A.shape[1] != B.shape[1]:
        raise PBError('pairwise_l2: A has %d features, B %d' % (A.shape[1], B.shape[1]))
    D = torch.empty((A.shape[0], B.shape[0]), dtype=torch.float32, device=A.device) if out is None else out
    if tuple(D.shape) != (A.shape[0], B.shape[0]):
        raise PBError('pairwise_l2: out is %s for %d x %d rows' % (tuple(D.shape), A.shape[0], B.shape[0]))
    LIB.call('pb_pairwise_l2', pa, pb, _dense(D, torch.float32, 2, 'pairwise_l2: out'), A.shape[0], B.shape[0], A.shape[1], _stream())
    return D


def metrics_ws(N, M, G, device):
    """The partial rows of sample_moments / kde_eval over an (N, M) matrix and G grid points (reusable by the next call on the same stream)."""
    return torch.empty(max(1, (LIB.query('pb_metrics_ws_bytes', int(N), int(M), int(G)) + 7) // 8), dtype=torch.float64, device=device)


def _samples_ws(D, G, ws, who):
    N, M = D.shape
    need = LIB.query('pb_metrics_ws_bytes', N, M, G)
    if ws is None:
        ws = metrics_ws(N, M, G, D.device)
    if ws.dtype != torch.float64 or not ws.is_contiguous() or ws.numel() * 8 < need:
        raise PBError('%s: ws must be a contiguous f64 tensor of at least %d bytes (metrics_ws)' % (who, need))
    return ws


def sample_moments(D, upper=False, ws=None):
    """pb_sample_moments: a device f64[6] = n, sum, sum of squares, 0, min, max of D (N, M) f32, or of its strict upper triangle (upper)."""
    pd = _dense(D, torch.float32, 2, 'sample_moments: D')
    ws = _samples_ws(D, 1, ws, 'sample_moments')
    out = torch.empty(6, dtype=torch.float64, device=D.device)
    LIB.call('pb_sample_moments', pd, D.shape[0], D.shape[1], int(bool(upper)), _p(out), _p(ws), _stream())
    return out


def kde_eval(D, grid, h, upper=False, ws=None):
    """pb_kde_eval: the Gaussian kernel density (bandwidth h) of the samples of D (as sample_moments) at the f32 grid points, a device f64 (G)."""
    pd, pg = _dense(D, torch.float32, 2, 'kde_eval: D'), _dense(grid, torch.float32, 1, 'kde_eval: grid')
    ws = _samples_ws(D, grid.numel(), ws, 'kde_eval')
    dens = torch.empty(grid.numel(), dtype=torch.float64, device=D.device)
    LIB.call('pb_kde_eval', pd, D.shape[0], D.shape[1], int(bool(upper)), pg, grid.numel(), float(h), _p(dens), _p(ws), _stream())
    return dens


SQDIST_MAX_D = 4096                                         # the widest row of pb_sqdist and pb_embed_moments
KNN_MAX_K = 64                                              # the largest k of pb_knn_radius


def _rows_f32(t, what, cols=None):
    """(address, rows, cols, leading dimension) of a 2-D f32 tensor whose rows are contiguous (a column or row slice of a wider buffer is one).
    Checked on the host: a tensor that is not on the device is refused last, by _p."""
    if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1 or t.stride(1) != 1 \
            or (t.shape[0] > 1 and t.stride(0) < t.shape[1]) or (cols is not None and t.shape[1] != cols):
        raise PBError('%s must be a 2-D f32 tensor%s with contiguous rows (got %s)'
                      % (what, '' if cols is None else ' of %d columns' % cols, (tuple(t.shape), t.dtype, t.stride()) if torch.is_tensor(t) else type(t)))
    return _p(t), t.shape[0], t.shape[1], (t.stride(0) if t.shape[0] > 1 else t.shape[1])


def _vec(t, dtype, n, what):
    if not torch.is_tensor(t) or t.dtype != dtype or t.dim() != 1 or t.numel() != n or not t.is_contiguous():
        raise PBError('%s must be a contiguous %s tensor of %d entries' % (what, str(dtype).replace('torch.', ''), n))
    return _p(t)


def pool_rows(H, mask=None, out=None):
    """pb_pool_rows: (out (B, d) f32, count (B) int32) with out[b] = the mean of the rows H[b, s] whose mask[b, s] != 0 (mask (B, S) f32 or
    None = all rows) and count[b] their number. H (B, S, d) bf16 or f32 with contiguous (b, s) rows at one leading dimension (a column slice
    of a (B, S, D) buffer is one). The sum runs in f64 in a fixed order; a row without a visible position is a zero vector."""
    if not torch.is_tensor(H) or H.dim() != 3 or H.dtype not in (torch.float32, torch.bfloat16) or min(H.shape) < 1:
        raise PBError('pool_rows: H must be a (B, S, d) bf16 or f32 tensor (got %s)' % ((tuple(H.shape), H.dtype) if torch.is_tensor(H) else type(H),))
    B, S, d = H.shape
    ldh = H.stride(1) if S > 1 else (H.stride(0) if B > 1 else d)
    if H.stride(2) != 1 or ldh < d or (B > 1 and H.stride(0) != S * ldh):
        raise PBError('pool_rows: the rows of H must be contiguous and evenly spaced (strides %s)' % (H.stride(),))
    if S > 65536 or B > 65535:
        raise PBError('pool_rows: B = %d, S = %d out of range (B <= 65535, S <= 65536)' % (B, S))
    pm = None
    if mask is not None:
        if not torch.is_tensor(mask) or mask.dtype != torch.float32 or tuple(mask.shape) != (B, S) or not mask.is_contiguous():
            raise PBError('pool_rows: mask must be a contiguous (%d, %d) f32 tensor' % (B, S))
        pm = _p(mask)
    ph = _p(H)
    if out is None:
        out = torch.empty((B, d), dtype=torch.float32, device=H.device)
    po, _, _, ldo = _rows_f32(out, 'pool_rows: out', d)
    if out.shape[0] != B:
        raise PBError('pool_rows: out holds %d rows for %d pieces' % (out.shape[0], B))
    count = torch.empty(B, dtype=torch.int32, device=H.device)
    LIB.call('pb_pool_rows', ph, ldh, dtype_code(H.dtype), pm, po, ldo, _p(count), B, S, d, _stream())
    return out, count


def embed_ws(N, d, device):
    """The workspace of one embed_moments call over an (N, d) set (reusable by the next call of that size on the same stream)."""
    return torch.empty(max(1, LIB.query('pb_embed_ws_bytes', int(N), int(d)) // 8), dtype=torch.float64, device=device)


def embed_moments(X, ws=None):
    """pb_embed_moments: (mean (d) f64, C (d, d) f64) of X (N, d) f32, N >= 2: C = sum_n (x_n - mean)(x_n - mean)^T, symmetric bit for bit;
    the caller divides by N - 1."""
    if not torch.is_tensor(X) or X.dim() != 2:
        raise PBError('embed_moments: X must be an (N, d) f32 tensor')
    N, d = X.shape
    if N < 2:
        raise PBError('embed_moments: N = %d; a covariance needs at least 2 rows' % N)
    if not 1 <= d <= SQDIST_MAX_D:
        raise PBError('embed_moments: d = %d out of range (1 .. %d)' % (d, SQDIST_MAX_D))
    px, _, _, ldx = _rows_f32(X, 'embed_moments: X')
    need = LIB.query('pb_embed_ws_bytes', N, d)
    if ws is None:
        ws = embed_ws(N, d, X.device)
    if ws.dtype != torch.float64 or not ws.is_contiguous() or ws.numel() * 8 < need:
        raise PBError('embed_moments: ws must be a contiguous f64 tensor of at least %d bytes (embed_ws)' % need)
    mean = torch.empty(d, dtype=torch.float64, device=X.device)
    C = torch.empty((d, d), dtype=torch.float64, device=X.device)
    LIB.call('pb_embed_moments', px, ldx, N, d, _p(mean), _p(C), d, _p(ws), _stream())
    return mean, C


def sqdist(A, B, out=None):
    """pb_sqdist: D2 (N, M) f32 with D2[i, j] = |A[i] - B[j]|^2 for A (N, d), B (M, d) f32 with contiguous rows, 1 <= d <= 4096; one f32
    chain of squared differences per element: equal rows give exactly 0. out: an (N, M) f32 tensor with contiguous rows."""
    if not torch.is_tensor(A) or not torch.is_tensor(B) or A.dim() != 2 or B.dim() != 2 or A.shape[1] != B.shape[1]:
        raise PBError('sqdist: A (N, d) and B (M, d) must have the same width (got %s and %s)'
                      % (tuple(A.shape) if torch.is_tensor(A) else type(A), tuple(B.shape) if torch.is_tensor(B) else type(B)))
    d = A.shape[1]
    if not 1 <= d <= SQDIST_MAX_D:
        raise PBError('sqdist: d = %d out of range (1 .. %d)' % (d, SQDIST_MAX_D))
    pa, N, _, lda = _rows_f32(A, 'sqdist: A')
    pb, M, _, ldb = _rows_f32(B, 'sqdist: B')
    if out is None:
        out = torch.empty((N, M), dtype=torch.float32, device=A.device)
    po, n_out, _, ldd = _rows_f32(out, 'sqdist: out', M)
    if n_out != N:
        raise PBError('sqdist: out is %s for %d x %d rows' % (tuple(out.shape), N, M))
    LIB.call('pb_sqdist', pa, lda, pb, ldb, po, ldd, N, M, d, _stream())
    return out


def knn_radius(D2, k, r0=0):
    """pb_knn_radius: rad (n) f32, rad[i] = the k-th smallest of D2[i, j] over j != r0 + i, for the (n, N) block D2 = the rows r0 .. r0 + n - 1
    of a set's own (N, N) squared distances. 1 <= k <= min(N - 1, 64)."""
    if not torch.is_tensor(D2) or D2.dim() != 2:
        raise PBError('knn_radius: D2 must be an (n, N) f32 tensor')
    n, N = D2.shape
    k, r0 = int(k), int(r0)
    if N < 2 or r0 < 0 or r0 + n > N:
        raise PBError('knn_radius: rows r0 = %d .. %d of an (N, N) matrix with N = %d' % (r0, r0 + n, N))
    if not 1 <= k <= min(N - 1, KNN_MAX_K):
        raise PBError('knn_radius: k = %d out of range (1 .. min(N - 1, %d) = %d)' % (k, KNN_MAX_K, min(N - 1, KNN_MAX_K)))
    pd, _, _, ldd = _rows_f32(D2, 'knn_radius: D2')
    rad = torch.empty(n, dtype=torch.float32, device=D2.device)
    LIB.call('pb_knn_radius', pd, ldd, n, N, r0, k, _p(rad), _stream())
    return rad


def ball_counts(D2, rad_ref, rad_gen, row_hits, col_hits, col_hits_gen):
    """pb_ball_counts: over the block D2 (n, M) of generated rows against reference columns add into the int32 counters (zeroed by the caller)
    row_hits (n) and col_hits (M) the entries with D2[i, j] < rad_ref[j], and into col_hits_gen (M) those with D2[i, j] < rad_gen[i]."""
    pd, n, M, ldd = _rows_f32(D2, 'ball_counts: D2')
    args = (_vec(rad_ref, torch.float32, M, 'ball_counts: rad_ref'), _vec(rad_gen, torch.float32, n, 'ball_counts: rad_gen'),
            _vec(row_hits, torch.int32, n, 'ball_counts: row_hits'), _vec(col_hits, torch.int32, M, 'ball_counts: col_hits'),
            _vec(col_hits_gen, torch.int32, M, 'ball_counts: col_hits_gen'))
    LIB.call('pb_ball_counts', pd, ldd, n, M, *args, _stream())


RUNS_TILE = 32                                              # corpus pieces per workgroup of pb_shared_runs (pb_runs_tile)
RUNS_MAX_S = 4096                                           # rows of a piece / keys of a row that pb_piece_keys and pb_shared_runs take
NO_KEY = 0xFFFFFFFF
assert HEAD_MAX == 1088                                     # the key's interval field: 1088 + difference, 2304 + id, both below 4096


def piece_keys(ids16, pitch_of, start=None, layout=None, mode=0):
    """pb_piece_keys: (keys (N, S) int32 holding the uint32 keys, klen (N) int32) of ids16 (N, S, 8) int16, S <= 4096. mode 0 = exact pitch,
    1 = interval to the note before. pitch_of and start as in piece_features. Key rows behind klen hold NO_KEY (-1 as int32)."""
    shared, N, S = _pieces('piece_keys', RUNS_MAX_S, ids16, pitch_of, start, layout)
    if mode not in (0, 1):
        raise PBError('piece_keys: mode = %r (0 = exact, 1 = interval)' % (mode,))
    keys = torch.empty((N, S), dtype=torch.int32, device=ids16.device)
    klen = torch.empty((N,), dtype=torch.int32, device=ids16.device)
    LIB.call('pb_piece_keys', *shared, _p(keys), _p(klen), N, S, int(mode), _stream())
    return keys, klen


def shared_runs(A, alen, B, blen, min_run=8, exclude_self=False, j_base=0, want_matrix=True, run_end=None, best=None):
    """pb_shared_runs: (R, run_end, best) for key rows A (N, Sa) / B (M, Sb) int32 with lengths alen (N) / blen (M) int32. R (N, M) int32 is
    None without want_matrix. Given run_end (N, Sa) int32 and best (N) int64 are maxed into (a corpus fed in chunks, j_base = the
    chunk's first piece); otherwise they are new tensors."""
    pa, pb = _dense(A, torch.int32, 2, 'shared_runs: A'), _dense(B, torch.int32, 2, 'shared_runs: B')
    pal, pbl = _dense(alen, torch.int32, 1, 'shared_runs: alen'), _dense(blen, torch.int32, 1, 'shared_runs: blen')
    (N, Sa), (M, Sb) = A.shape, B.shape
    if alen.numel() != N or blen.numel() != M:
        raise PBError('shared_runs: alen / blen hold %d / %d entries for %d / %d rows' % (alen.numel(), blen.numel(), N, M))
    if not (1 <= Sa <= RUNS_MAX_S and 1 <= Sb <= RUNS_MAX_S):
        raise PBError('shared_runs: rows of %d and %d keys; 1 .. %d' % (Sa, Sb, RUNS_MAX_S))
    if (run_end is None) != (best is None):
        raise PBError('shared_runs: run_end and best are given together (accumulate) or not at all')
    accumulate = run_end is not None
    if accumulate:
        if tuple(run_end.shape) != (N, Sa) or tuple(best.shape) != (N,):
            raise PBError('shared_runs: run_end %s / best %s for %d rows of %d keys' % (tuple(run_end.shape), tuple(best.shape), N, Sa))
    else:
        run_end = torch.empty((N, Sa), dtype=torch.int32, device=A.device)
        best = torch.empty((N,), dtype=torch.int64, device=A.device)
    p_re, p_best = _dense(run_end, torch.int32, 2, 'shared_runs: run_end'), _dense(best, torch.int64, 1, 'shared_runs: best')
    R = torch.empty((N, M), dtype=torch.int32, device=A.device) if want_matrix else None
    LIB.call('pb_shared_runs', pa, pal, N, Sa, pb, pbl, M, Sb, int(min_run), int(bool(exclude_self)), int(j_base), _p(R), p_re, p_best,
             int(accumulate), _stream())
    return R, run_end, best


ALIGN_BLOCK = 256                                           # B columns one sweep of a wave of pb_local_align covers (pb_align_block)
ALIGN_TILE = RUNS_TILE                                      # corpus pieces per workgroup of pb_local_align: the tile of pb_shared_runs
ALIGN_RANGES = (('match', 1, 8), ('mismatch', 1, 16), ('gap', 1, 16))


def align_params(match=1, mismatch=2, gap=2, min_score=8, who='local_align'):
    """The four integers of pb_local_align, checked against their ranges (match 1 .. 8, mismatch and gap 1 .. 16, min_score >= 1)."""
    vals = {'match': match, 'mismatch': mismatch, 'gap': gap, 'min_score': min_score}
    for name, v in vals.items():
        if isinstance(v, bool) or int(v) != v:
            raise PBError('%s: %s = %r is not an integer' % (who, name, v))
    for name, lo, hi in ALIGN_RANGES:
        if not lo <= int(vals[name]) <= hi:
            raise PBError('%s: %s = %d out of range (%d .. %d)' % (who, name, int(vals[name]), lo, hi))
    if not 1 <= int(min_score) < 2 ** 31:
        raise PBError('%s: min_score = %d must be >= 1' % (who, int(min_score)))
    return int(match), int(mismatch), int(gap), int(min_score)


def local_align(A, alen, B, blen, match=1, mismatch=2, gap=2, min_score=8, exclude_self=False, j_base=0, want_matrix=True, align_end=None,
                best=None):
    """pb_local_align: (score, align_end, best) for key rows A (N, Sa) / B (M, Sb) int32 with lengths alen (N) / blen (M) int32. score
    (N, M) int32 is None without want_matrix. Given align_end (N, Sa) int32 and best (N) int64 are maxed into (a corpus fed in chunks,
    j_base = the chunk's first piece); otherwise they are new tensors."""
    match, mismatch, gap, min_score = align_params(match, mismatch, gap, min_score)
    pa, pb = _dense(A, torch.int32, 2, 'local_align: A'), _dense(B, torch.int32, 2, 'local_align: B')
    pal, pbl = _dense(alen, torch.int32, 1, 'local_align: alen'), _dense(blen, torch.int32, 1, 'local_align: blen')
    assert LIB.query('pb_align_block') == ALIGN_BLOCK, 'ops.ALIGN_BLOCK and the library disagree'
    (N, Sa), (M, Sb) = A.shape, B.shape
    if alen.numel() != N or blen.numel() != M:
        raise PBError('local_align: alen / blen hold %d / %d entries for %d / %d rows' % (alen.numel(), blen.numel(), N, M))
    if not (1 <= Sa <= RUNS_MAX_S and 1 <= Sb <= RUNS_MAX_S):
        raise PBError('local_align: rows of %d and %d keys; 1 .. %d' % (Sa, Sb, RUNS_MAX_S))
    if (align_end is None) != (best is None):
        raise PBError('local_align: align_end and best are given together (accumulate) or not at all')
    accumulate = align_end is not None
    if accumulate:
        if tuple(align_end.shape) != (N, Sa) or tuple(best.shape) != (N,):
            raise PBError('local_align: align_end %s / best %s for %d rows of %d keys' % (tuple(align_end.shape), tuple(best.shape), N, Sa))
    else:
        align_end = torch.empty((N, Sa), dtype=torch.int32, device=A.device)
        best = torch.empty((N,), dtype=torch.int64, device=A.device)
    p_ae, p_best = _dense(align_end, torch.int32, 2, 'local_align: align_end'), _dense(best, torch.int64, 1, 'local_align: best')
    score = torch.empty((N, M), dtype=torch.int32, device=A.device) if want_matrix else None
    LIB.call('pb_local_align', pa, pal, N, Sa, pb, pbl, M, Sb, match, mismatch, gap, min_score, int(bool(exclude_self)), int(j_base), _p(score),
             p_ae, p_best, int(accumulate), _stream())
    return score, align_end, best


STRUCTURE_LAGS = 64                                         # the lags of pb_piece_structure (pb_structure_lags)
STRUCTURE_COLS = 8 + 4 * STRUCTURE_LAGS                     # its row: 8 scalar columns, then I_O, T_O, I_N, T_N (pb_structure_cols)


def piece_structure(ids16, pitch_of, start=None, layout=None, mode=0):
    """pb_piece_structure: the (N, 264) int32 lag sums of ids16 (N, S, 8) int16, S <= 4096. mode 0 = exact pitch, 1 = pitch class.
    pitch_of and start as in piece_features."""
    shared, N, S = _pieces('piece_structure', RUNS_MAX_S, ids16, pitch_of, start, layout)
    if mode not in (0, 1):
        raise PBError('piece_structure: mode = %r (0 = exact pitch, 1 = pitch class)' % (mode,))
    assert LIB.query('pb_structure_lags') == STRUCTURE_LAGS and LIB.query('pb_structure_cols') == STRUCTURE_COLS, \
        'ops.STRUCTURE_LAGS / STRUCTURE_COLS and the library disagree'
    out = torch.empty((N, STRUCTURE_COLS), dtype=torch.int32, device=ids16.device)
    LIB.call('pb_piece_structure', *shared, _p(out), N, S, int(mode), _stream())
    return out


HARMONY_LAGS = 64                                           # the lags of pb_piece_harmony (pb_harmony_lags)
HARMONY_COLS = 36 + 3 * HARMONY_LAGS                        # its row: 36 scalar and window columns, then I_H, T_H, I_X (pb_harmony_cols)
HARMONY_SHIFT = 20                                          # the entropy sums are bits times 2^20
_HARMONY_TABLES = {}


def harmony_table(device=None):
    """The int64 table of pb_piece_harmony: TL[k] = round(k log2(k) 2^20) for k = 0 .. 4096, TL[0] = TL[1] = 0, from the plain float64
    expression (no entry lies closer than 1.47e-4 to a rounding tie, so every correct evaluation gives these integers;
    tests/test_harmony_cpu.py compares them with a 60-digit evaluation). device=None: the host tensor; else that device's cached copy."""
    if 'host' not in _HARMONY_TABLES:
        t = [0, 0] + [int(round(k * math.log2(k) * float(1 << HARMONY_SHIFT))) for k in range(2, RUNS_MAX_S + 1)]
        _HARMONY_TABLES['host'] = torch.tensor(t, dtype=torch.int64)
    if device is None:
        return _HARMONY_TABLES['host']
    dev = torch.device(device)
    if dev not in _HARMONY_TABLES:
        _HARMONY_TABLES[dev] = _HARMONY_TABLES['host'].to(dev)
    return _HARMONY_TABLES[dev]


def piece_harmony(ids16, pitch_of, start=None, layout=None, table=None):
    """pb_piece_harmony: the (N, 228) int64 harmony columns of ids16 (N, S, 8) int16, S <= 4096. pitch_of and start as in piece_features.
    table: harmony_table() on the device of ids16 (the default: that device's cached copy)."""
    shared, N, S = _pieces('piece_harmony', RUNS_MAX_S, ids16, pitch_of, start, layout)
    assert LIB.query('pb_harmony_lags') == HARMONY_LAGS and LIB.query('pb_harmony_cols') == HARMONY_COLS, \
        'ops.HARMONY_LAGS / HARMONY_COLS and the library disagree'
    if table is None:
        table = harmony_table(ids16.device)
    p_table = _dense(table, torch.int64, 1, 'piece_harmony: table')
    if table.numel() != RUNS_MAX_S + 1:
        raise PBError('piece_harmony: table holds %d entries; harmony_table() has %d' % (table.numel(), RUNS_MAX_S + 1))
    out = torch.empty((N, HARMONY_COLS), dtype=torch.int64, device=ids16.device)
    LIB.call('pb_piece_harmony', *shared, p_table, _p(out), N, S, _stream())
    return out


TEXTURE_COLS = 64                                           # the row of pb_piece_texture (pb_texture_cols)


def piece_texture(ids16, pitch_of, dur_pos, bar_pos, start=None, layout=None):
    """pb_piece_texture: the (N, 64) int32 texture columns of ids16 (N, S, 8) int16, S <= 4096. pitch_of, dur_pos and start as in
    piece_features; bar_pos (int32, layout.pad8[6] entries: the positions of a bar of a time-signature id) is a device table."""
    shared, N, S = _pieces('piece_texture', RUNS_MAX_S, ids16, pitch_of, start, layout)
    assert LIB.query('pb_texture_cols') == TEXTURE_COLS, 'ops.TEXTURE_COLS and the library disagree'
    p_dur, p_bar = _dense(dur_pos, torch.int32, 1, 'piece_texture: dur_pos'), _dense(bar_pos, torch.int32, 1, 'piece_texture: bar_pos')
    pad8 = (layout or DEFAULT_LAYOUT).pad8
    if dur_pos.numel() != pad8[4]:
        raise PBError('piece_texture: dur_pos holds %d entries, the layout has %d duration ids' % (dur_pos.numel(), pad8[4]))
    if bar_pos.numel() != pad8[6]:
        raise PBError('piece_texture: bar_pos holds %d entries, the layout has %d time-signature ids' % (bar_pos.numel(), pad8[6]))
    out = torch.empty((N, TEXTURE_COLS), dtype=torch.int32, device=ids16.device)
    LIB.call('pb_piece_texture', *shared, p_dur, p_bar, _p(out), N, S, _stream())
    return out


def transpose_batch_bf16(src, dst, table, n_tiles):
    LIB.call('pb_transpose_batch_bf16', _p(src), _p(dst), _p(table), table.shape[0], n_tiles, _stream())


def fill_f32(dst, value):
    LIB.call('pb_fill_f32', _p(dst), value, dst.numel(), _stream())


def shift_right(ids16, sos_row16, out, B, S):
    LIB.call('pb_shift_right', _p(ids16), _p(sos_row16), _p(out), B, S, _stream())


class PackedRows:
    """Row descriptors of one packed attention call (include/pianobart_hip.h, pb_attn_desc): device int32 (B) tensors plus
    the two maxima."""

    def __init__(self, q_off, q_len, k_off, k_len, k_vis, Sq_max, Sk_max, kind='', order=None):
        self.q_off, self.q_len, self.k_off, self.k_len, self.k_vis, self.Sq_max, self.Sk_max = q_off, q_len, k_off, k_len, k_vis, Sq_max, Sk_max
        self.kind = kind                    # a label for profiles ('enc', 'dec', 'cross')
        self.order = order                  # device int32 (B * H): dispatch order of the (batch, head) pairs, longest first (or None)


_fa1_ws = {}


def _flash1_ws(nbytes, device):
    """The dQ slab workspace of the one-pass backward (one per device, grown on demand)."""
    ws = _fa1_ws.get(device)
    if ws is None or ws.numel() < nbytes:
        ws = _fa1_ws[device] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return ws


def _attn(entry, dtype, q, k, v, o, lse, B, H, hd, scale, causal, *, Sq=0, Sk=0, key_mask=None, kmax=None, rows=None, generic=False,
          dout=None, grads=None, delta=None, dbias=None, dbias_ws=None, one_pass=False, q_rows=None, delta_rows=None):
    """One pb_attn_desc, one call (entry = 'pb_attn_fwd' / 'pb_attn_bwd'). q, k, v, o and grads = (dq, dk, dv) are (tensor, element
    offset, row stride[, batch stride]); dout is a tensor with o's strides. rows (a PackedRows) replaces Sq / Sk / key_mask / kmax
    (its dispatch order is for the bf16 kernels only). one_pass: the one-pass backward with its slab workspace (q_rows: rows of the q side)."""
    d = AttnDesc()
    esz = 2 if dtype == PB_BF16 else 4
    for name, (t, off, ss, *sb) in zip(('q', 'k', 'v', 'o', 'dq', 'dk', 'dv'), (q, k, v, o) + tuple(grads or ())):
        setattr(d, name, _adr(t) + esz * off)
        setattr(d, name + '_ss', ss)
        setattr(d, name + '_sb', sb[0] if sb else 0)
    d.dout, d.lse, d.delta, d.key_mask, d.kmax, d.delta_rows = _adr(dout), _adr(lse), _adr(delta), _adr(key_mask), _adr(kmax), _adr(delta_rows)
    if rows is not None:
        Sq, Sk = rows.Sq_max, rows.Sk_max
        d.q_off, d.q_len, d.k_off, d.k_len, d.k_vis = _adr(rows.q_off), _adr(rows.q_len), _adr(rows.k_off), _adr(rows.k_len), _adr(rows.k_vis)
        d.bh_order = _adr(rows.order) if dtype == PB_BF16 else None
    if dbias:
        d.dbias_q, d.dbias_k, d.dbias_v, d.dbias_ws = _adr(dbias[0]), _adr(dbias[1]), _adr(dbias[2]), _adr(dbias_ws)
    if one_pass:
        d.q_rows = q_rows if q_rows is not None else B * Sq
        d.dq_ws = _adr(_flash1_ws(int(LIB.query('pb_flash_bwd1_ws_bytes', d.q_rows, H, hd, Sk)), q[0].device))
    d.dtype, d.B, d.H, d.Sq, d.Sk, d.hd, d.scale = dtype, B, H, Sq, Sk, hd, scale
    d.flags = (ATTN_CAUSAL if causal else 0) | (ATTN_GENERIC if generic else 0) | (ATTN_ONE_PASS if one_pass else 0)
    LIB.call(entry, ctypes.byref(d), _stream())


def flash_fwd(q, k, v, o, lse, key_mask, B, H, Sq, Sk, hd, scale, causal, force_generic=False, kmax=None):
    """q,k,v,o: (tensor, element offset, row stride, batch stride) bf16."""
    _attn('pb_attn_fwd', PB_BF16, q, k, v, o, lse, B, H, hd, scale, causal, Sq=Sq, Sk=Sk, key_mask=key_mask, kmax=kmax, generic=force_generic)


def flash_bwd(q, k, v, o, dout, lse, key_mask, dq, dk, dv, delta, B, H, Sq, Sk, hd, scale, causal, force_generic=False, kmax=None, dbias=None, dbias_ws=None):
    """dbias = (gq, gk, gv): f32 vectors of H*hd that receive += the column sums of dq / dk / dv (bias gradients), with dbias_ws."""
    _attn('pb_attn_bwd', PB_BF16, q, k, v, o, lse, B, H, hd, scale, causal, Sq=Sq, Sk=Sk, key_mask=key_mask, kmax=kmax, generic=force_generic,
          dout=dout, grads=(dq, dk, dv), delta=delta, dbias=dbias, dbias_ws=dbias_ws)


def flash_bwd1(q, k, v, o, dout, lse, key_mask, dq, dk, dv, delta, B, H, Sq, Sk, hd, scale, causal, kmax=None, dbias=None, dbias_ws=None, delta_rows=None):
    """flash_bwd's arguments and results, one pass over the (key block, query tile) pairs (head_dim 64)."""
    _attn('pb_attn_bwd', PB_BF16, q, k, v, o, lse, B, H, hd, scale, causal, Sq=Sq, Sk=Sk, key_mask=key_mask, kmax=kmax, dout=dout, grads=(dq, dk, dv),
          delta=delta, dbias=dbias, dbias_ws=dbias_ws, one_pass=True, delta_rows=delta_rows)


def flash_fwd_packed(q, k, v, o, lse, rows, B, H, hd, scale, causal):
    """q,k,v,o: (tensor, element offset, row stride) bf16 over packed rows."""
    _attn('pb_attn_fwd', PB_BF16, q, k, v, o, lse, B, H, hd, scale, causal, rows=rows)


def flash_bwd_packed(q, k, v, o, dout, lse, dq, dk, dv, delta, rows, B, H, hd, scale, causal, dbias=None, dbias_ws=None):
    _attn('pb_attn_bwd', PB_BF16, q, k, v, o, lse, B, H, hd, scale, causal, rows=rows, dout=dout, grads=(dq, dk, dv), delta=delta,
          dbias=dbias, dbias_ws=dbias_ws)


def flash_bwd1_packed(q, k, v, o, dout, lse, dq, dk, dv, delta, rows, B, H, hd, scale, causal, q_rows, dbias=None, dbias_ws=None, delta_rows=None):
    """flash_bwd_packed's arguments and results in one pass; q_rows = rows of the q-side tensors."""
    _attn('pb_attn_bwd', PB_BF16, q, k, v, o, lse, B, H, hd, scale, causal, rows=rows, dout=dout, grads=(dq, dk, dv), delta=delta,
          dbias=dbias, dbias_ws=dbias_ws, one_pass=True, q_rows=q_rows, delta_rows=delta_rows)


def flash_fwd_x3(q, k, v, o, lse, key_mask, B, H, Sq, Sk, hd, scale, causal, kmax=None):
    """Fused attention of the bf16x3 instantiation. q,k,v,o: (tensor, element offset, row stride, batch stride) f32."""
    _attn('pb_attn_fwd', PB_F32X3, q, k, v, o, lse, B, H, hd, scale, causal, Sq=Sq, Sk=Sk, key_mask=key_mask, kmax=kmax)


def flash_bwd_x3(q, k, v, o, dout, lse, key_mask, dq, dk, dv, delta, B, H, Sq, Sk, hd, scale, causal, kmax=None):
    _attn('pb_attn_bwd', PB_F32X3, q, k, v, o, lse, B, H, hd, scale, causal, Sq=Sq, Sk=Sk, key_mask=key_mask, kmax=kmax,
          dout=dout, grads=(dq, dk, dv), delta=delta)


def flash_fwd_x3_packed(q, k, v, o, lse, rows, B, H, hd, scale, causal):
    """q,k,v,o: (tensor, element offset, row stride) f32 over packed rows (bf16x3 instantiation)."""
    _attn('pb_attn_fwd', PB_F32X3, q, k, v, o, lse, B, H, hd, scale, causal, rows=rows)


def flash_bwd_x3_packed(q, k, v, o, dout, lse, dq, dk, dv, delta, rows, B, H, hd, scale, causal):
    _attn('pb_attn_bwd', PB_F32X3, q, k, v, o, lse, B, H, hd, scale, causal, rows=rows, dout=dout, grads=(dq, dk, dv), delta=delta)


def rowmap_count(emask, dmask, loss_mask, counts):
    B, S = emask.shape
    LIB.call('pb_rowmap_count', _p(emask), _p(dmask), _p(loss_mask), _p(counts), B, S, _stream())


def rowmap_build(mask, loss_mask, off, length, row_src, row_pos, inv):
    B, S = mask.shape
    LIB.call('pb_rowmap_build', _p(mask), _p(loss_mask), _p(off), _p(length), _p(row_src), _p(row_pos), _p(inv), B, S, _stream())


def rowmap_build_sub(loss_mask, present, off, length, row_src, row_idx):
    B, S = loss_mask.shape[:2]
    LIB.call('pb_rowmap_build_sub', _p(loss_mask), _p(present), _p(off), _p(length), _p(row_src), _p(row_idx), B, S, _stream())


def scatter_rows16(src, row_dst, dst, n_rows, row_bytes):
    LIB.call('pb_scatter_rows16', _p(src), _p(row_dst), _p(dst), n_rows, row_bytes, _stream())


def gather_rows16(src, row_src, dst, n_rows, row_bytes):
    LIB.call('pb_gather_rows16', _p(src), _p(row_src), _p(dst), n_rows, row_bytes, _stream())


def pos_grad_packed(x, inv, out, B, S):
    LIB.call('pb_pos_grad_packed', _p(x), _p(inv), _p(out), B, S, x.shape[1], dtype_code(x.dtype), _stream())


def corrupt(ids16, out16, loss_mask, choice, choice_out, mask_percent, seed, pad_row, mask_row, n_tokens):
    """ids16/out16 (B,S,8) int16 device; loss_mask (B,S,8) f32; choice/choice_out (B,) int32 device or None."""
    B, S = ids16.shape[:2]
    pr = (ctypes.c_int16 * 8)(*[int(x) for x in pad_row])
    mr = (ctypes.c_int16 * 8)(*[int(x) for x in mask_row])
    nt = (ctypes.c_int32 * 8)(*[int(x) for x in n_tokens])
    LIB.call('pb_corrupt', _p(ids16), _p(out16), _p(loss_mask), _p(choice), _p(choice_out), B, S, float(mask_percent), seed, pr, mr, nt, _stream())


def corrupt_replay(ids16, out16, loss_mask, choice, mask_percent, decisions, rand_rows, pad_row, mask_row):
    """pb_corrupt with caller-supplied random decisions (layout: include/pianobart_hip.h). decisions (B, stride) int32 device,
    rand_rows (B,S,8) int16 device or None."""
    B, S = ids16.shape[:2]
    pr = (ctypes.c_int16 * 8)(*[int(x) for x in pad_row])
    mr = (ctypes.c_int16 * 8)(*[int(x) for x in mask_row])
    LIB.call('pb_corrupt_replay', _p(ids16), _p(out16), _p(loss_mask), _p(choice), B, S, float(mask_percent), _p(decisions),
             decisions.shape[1], _p(rand_rows), pr, mr, _stream())


def augment(ids16, out16, shifts, coord, id_at, plan18, seed):
    """pb_augment (include/pianobart_hip.h): ids16 / out16 (B,S,8) int16 device (out16 may be ids16), shifts (B,3) int32 device, coord / id_at
    (3, HEAD_MAX) int16 device, plan18 a HOST ctypes int32[18] (augment.AugmentPlan builds the three). Refusals raise PBError."""
    B, S = ids16.shape[:2]
    LIB.call('pb_augment', _p(ids16), _p(out16), _p(shifts), B, S, _p(coord), _p(id_at), plan18, ctypes.c_uint64(seed), _stream())


def key_extent(key_mask, kmax):
    B, Sk = key_mask.shape
    LIB.call('pb_key_extent', _p(key_mask), _p(kmax), B, Sk, _stream())


# ---- K14: fine-tune heads (f32) ------------------------------------------------------------------------------------
def eltwise_fwd(op, x, x2, y, seed, site, p):
    LIB.call('pb_eltwise_fwd', op, _p(x), _p(x2), _p(y), x.numel(), seed, site, p, _stream())


def eltwise_bwd(op, y, x2, dy, dx, dx2, seed, site, p):
    LIB.call('pb_eltwise_bwd', op, _p(y), _p(x2), _p(dy), _p(dx), _p(dx2), dy.numel(), seed, site, p, _stream())


def softmax_dim1_fwd(x, y):
    B, S, R = x.shape
    LIB.call('pb_softmax_dim1_fwd', _p(x), _p(y), B, S, R, _stream())


def softmax_dim1_bwd(y, dy, dx):
    B, S, R = y.shape
    LIB.call('pb_softmax_dim1_bwd', _p(y), _p(dy), _p(dx), B, S, R, _stream())


def ce_rows(logits, target32, weight, coef, loss, dlogits, argmax):
    rows, C = logits.shape
    LIB.call('pb_ce_rows', _p(logits), _p(target32), _p(weight), _p(coef), _p(loss), _p(dlogits), _p(argmax), rows, C, _stream())


def gather_rows(table, ids32, bias, out):
    LIB.call('pb_gather_rows', _p(table), _p(ids32), _p(bias), _p(out), ids32.numel(), table.shape[1], table.shape[0], _stream())


def gather_rows_bwd(dout, ids32, dtable):
    LIB.call('pb_gather_rows_bwd', _p(dout), _p(ids32), _p(dtable), ids32.numel(), dtable.shape[1], dtable.shape[0], _stream())


def dropout(x, y, seed, site, p):
    LIB.call('pb_dropout', _p(x), _p(y), x.numel(), dtype_code(x.dtype), seed, site, p, _stream())


def defer_begin(arena, table):
    """Open a deferred-reduction window (K15): bias / LayerNorm-parameter partial sums collect in `arena` until defer_flush."""
    LIB.call('pb_defer_begin', _p(arena), arena.numel(), _p(table), table.numel() // int(LIB.query('pb_defer_desc_bytes')))


def defer_flush():
    LIB.call('pb_defer_flush', _stream())


def l2_penalty(p, g, weight, scratch, loss_acc):
    """finetune.py:241-243 for one parameter tensor: loss_acc += weight * ||p||, g += weight * p / ||p|| (g may be None)."""
    LIB.call('pb_l2_penalty', _p(p), _p(g), p.numel(), float(weight), _p(scratch), _p(loss_acc), _stream())


# ---- K27: LoRA (pb_lora.hip) -------------------------------------------------------------------------------------------------------------
def _lora_rows(t, M, width, off, what):
    """(address, leading dimension) of the (M, width) slice at column `off` of the row-major activation buffer `t` (bf16 or f32)."""
    if t.dim() != 2 or t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        raise PBError('%s must be a 2-D tensor with contiguous rows (got %s, strides %s)' % (what, tuple(t.shape), t.stride()))
    if M > t.shape[0] or off < 0 or off + width > t.shape[1]:
        raise PBError('%s: rows 0 .. %d, columns %d .. %d lie outside the %s tensor' % (what, M - 1, off, off + width - 1, tuple(t.shape)))
    return _p(t), (t.stride(0) if t.shape[0] > 1 else t.shape[1])


def _lora_small(t, shape, what):
    if t.dtype != torch.float32 or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise PBError('%s must be a contiguous f32 tensor of shape %s (got %s %s)' % (what, tuple(shape), tuple(t.shape), t.dtype))
    return _p(t)


def lora_down(X, W, T, M, K, alpha=1.0, x_off=0, w_kr=False):
    """T (M, r) f32 = alpha * X[:M, x_off : x_off + K] @ W^T. W is (r, K), or (K, r) with w_kr. X: bf16 or f32 rows of any leading dimension."""
    r = T.shape[1]
    x, ldx = _lora_rows(X, M, K, x_off, 'lora_down: X')
    w = _lora_small(W, (K, r) if w_kr else (r, K), 'lora_down: W')
    if T.dtype != torch.float32 or T.dim() != 2 or not T.is_contiguous() or T.shape[0] < M:
        raise PBError('lora_down: T must be a contiguous (>= M, r) f32 tensor')
    LIB.call('pb_lora_down', x, ldx, x_off, dtype_code(X.dtype), w, int(w_kr), _p(T), M, K, r, float(alpha), _stream())


def lora_up(Y, T, W, M, N, alpha=1.0, y_off=0, w_nr=False):
    """Y[:M, y_off : y_off + N] += alpha * T[:M] @ W in Y's dtype. W is (r, N), or (N, r) with w_nr."""
    r = T.shape[1]
    y, ldy = _lora_rows(Y, M, N, y_off, 'lora_up: Y')
    w = _lora_small(W, (N, r) if w_nr else (r, N), 'lora_up: W')
    if T.dtype != torch.float32 or T.dim() != 2 or not T.is_contiguous() or T.shape[0] < M:
        raise PBError('lora_up: T must be a contiguous (>= M, r) f32 tensor')
    LIB.call('pb_lora_up', y, ldy, y_off, dtype_code(Y.dtype), _p(T), w, int(w_nr), M, N, r, float(alpha), _stream())


def lora_wgrad_ws(M, r, C, device):
    """The workspace of one lora_wgrad call (reusable by the next call of that size on the same stream)."""
    return torch.empty(max(4, int(LIB.query('pb_lora_wgrad_ws_floats', int(M), int(r), int(C)))), dtype=torch.float32, device=device)


def lora_wgrad(T, X, G, M, C, alpha=1.0, x_off=0, g_cr=False, ws=None):
    """G = alpha * T[:M]^T @ X[:M, x_off : x_off + C], overwritten. G is (r, C), or (C, r) with g_cr. Bitwise reproducible."""
    r = T.shape[1]
    x, ldx = _lora_rows(X, M, C, x_off, 'lora_wgrad: X')
    g = _lora_small(G, (C, r) if g_cr else (r, C), 'lora_wgrad: G')
    if T.dtype != torch.float32 or T.dim() != 2 or not T.is_contiguous() or T.shape[0] < M:
        raise PBError('lora_wgrad: T must be a contiguous (>= M, r) f32 tensor')
    if ws is None:
        ws = lora_wgrad_ws(M, r, C, X.device)
    if ws.dtype != torch.float32 or ws.numel() < LIB.query('pb_lora_wgrad_ws_floats', M, r, C):
        raise PBError('lora_wgrad: ws is smaller than pb_lora_wgrad_ws_floats(%d, %d, %d)' % (M, r, C))
    LIB.call('pb_lora_wgrad', _p(T), x, ldx, x_off, dtype_code(X.dtype), g, int(g_cr), M, C, r, float(alpha), _p(ws), _stream())


def lora_merge(W, B, A, alpha):
    """W (N, K) f32 += alpha * B (N, r) @ A (r, K), in place (W may be a row range of a flat-buffer slot)."""
    N, K = W.shape
    r = A.shape[0]
    w = _lora_small(W, (N, K), 'lora_merge: W')
    LIB.call('pb_lora_merge', w, _lora_small(B, (N, r), 'lora_merge: B'), _lora_small(A, (r, K), 'lora_merge: A'), N, K, r, float(alpha), _stream())
