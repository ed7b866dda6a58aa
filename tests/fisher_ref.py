"""Host restatement (float32 numpy) of the Fisher merge of csrc/pb_fisher.hip / pianobart_amd/merge.py.

Every operation is float32, rounded once, in the order the reference's CPU tensors take it (model_merging_methods/merging_methods.py:131-177,
254-259); tests/test_fisher_cpu.py holds it to the reference's recorded outputs (tests/golden/g16_fisher.npz) bit for bit, the GPU tests
hold the kernels to it bit for bit."""
import numpy as np

F32 = np.float32


def _f(x):
    a = np.asarray(x)
    assert a.dtype == np.float32, a.dtype
    return a


def small_sum(x):
    """tensor.sum() of a float32 row of at most 8 values on the CPU: 8 values are one vector, added lane by lane from +0; fewer go through
    four interleaved partial sums (left to right below 4 values)."""
    x = _f(x)
    assert x.ndim == 1 and x.size <= 8
    if x.size == 8:
        s = F32(0.0)
        for v in x:
            s = F32(s + v)
        return s
    q = x.size // 4
    p = [F32(0.0)] * 4
    for i in range(q):
        for k in range(4):
            p[k] = F32(p[k] + x[4 * i + k])
    for v in x[4 * q:]:
        p[0] = F32(p[0] + v)
    for k in range(1, 4):
        p[0] = F32(p[0] + p[k])
    return p[0]


def norm64(F):
    """float32(sqrt(float64 sum of squares)): what pb_fisher_norm computes."""
    return F32(np.sqrt((_f(F).astype(np.float64) ** 2).sum()))


def coefficients(n, fisher_scaling_coefficients=None, normalize_fisher_weight=True, minimal_fisher_weight=1e-6, norms=None):
    c = np.ones(n, dtype=F32) / F32(n) if fisher_scaling_coefficients is None else np.asarray(fisher_scaling_coefficients, dtype=np.float64).astype(F32)
    if normalize_fisher_weight:
        r = F32(1.0) / (_f(np.asarray(norms, dtype=F32)) + F32(minimal_fisher_weight))
        c = c * (r / small_sum(r))
    assert c.dtype == np.float32
    return c


def accumulate(F, g):
    """pb_fisher_accum: F + g * g, the product and the sum each rounded."""
    return _f(F) + _f(g) * _f(g)


def finish(F, divisor):
    return _f(F) / F32(divisor)


def merge(ws, fs, fisher_scaling_coefficients=None, normalize_fisher_weight=True, minimal_fisher_weight=1e-6, norms=None, own_norm=False):
    """The merged flat vector of the flat models `ws` and their Fisher vectors `fs`. norms: one per model (the reference's, or a device's);
    own_norm: use norm64 of each Fisher vector instead."""
    ws, fs = [_f(w) for w in ws], [_f(f) for f in fs]
    if normalize_fisher_weight and own_norm:
        norms = np.array([norm64(f) for f in fs], dtype=F32)
    c = coefficients(len(ws), fisher_scaling_coefficients, normalize_fisher_weight, minimal_fisher_weight, norms)
    num, den = np.zeros_like(ws[0]), np.zeros_like(ws[0])
    for m in range(len(ws)):
        k = c[m] * (fs[m] + F32(minimal_fisher_weight))
        num = num + k * ws[m]
        den = den + k
    out = num / den
    assert out.dtype == np.float32
    return out
