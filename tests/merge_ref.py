"""Host restatement (float32 numpy) of the merge arithmetic of csrc/pb_merge.hip / pianobart_amd/merge.py.

Every operation is float32, rounded once, in the order the reference's CPU tensors take it (model_merging_methods/merging_methods.py,
mask_weights_utils.py); tests/test_merge_cpu.py holds it to the reference's recorded outputs (tests/golden/g15_merge.npz) bit for bit,
the GPU tests hold the kernels to it bit for bit. Masks multiply by 0 or 1 as the reference does (x * 0 keeps x's sign).
Flat vectors are laid out by a segment table [(name, offset, numel, shape)] in sorted-name order."""
import numpy as np

from tests.philox_ref import philox4x32

F32 = np.float32
MERGE_STREAM = 0x4D455247          # third counter word of the mask stream (dropout uses 0x5EED)


def _f(x):
    a = np.asarray(x)
    assert a.dtype == np.float32, a.dtype
    return a


def lsum(xs):
    """Left-to-right float32 sum of a list of arrays: (x0 + x1) + x2 ..."""
    s = _f(xs[0])
    for x in xs[1:]:
        s = s + _f(x)
    return s


def kth_abs(x, k):
    """The k-th smallest (1-based) magnitude."""
    return np.sort(np.abs(_f(x)).reshape(-1))[k - 1]


def zsum(xs):
    """torch's sum over the model axis: the accumulator starts at +0, so a sum of nothing but -0.0 is +0.0 (0 + x is x otherwise)."""
    return lsum([np.zeros_like(_f(xs[0]))] + list(xs))


def average(ws):
    return zsum(ws) / F32(len(ws))


def task_arithmetic(p, ws, lam):
    return p + F32(lam) * lsum([w - p for w in ws])


def ties_parts(p, ws, rate):
    """(T, sign, majority): the trimmed task vectors, the elected sign with zeros still 0, and the exact integer majority."""
    n = p.size
    k = int(n * rate)
    ts = []
    for w in ws:
        d = w - p
        ts.append(d * (np.abs(d) >= kth_abs(d, k)).astype(F32) if k >= 1 else d)
    sign = np.sign(zsum(ts))
    majority = int(np.sign(int((sign > 0).sum()) - int((sign < 0).sum())))
    return ts, sign, majority


def ties(p, ws, rate, lam):
    ts, sign, majority = ties_parts(p, ws, rate)
    sign = np.where(sign == 0, F32(majority), sign)
    kept = [t * (((sign > 0) & (t > 0)) | ((sign < 0) & (t < 0))).astype(F32) for t in ts]
    count = sum((kv != 0).astype(np.int64) for kv in kept)
    merged = zsum(kept) / np.maximum(count, 1).astype(F32)
    return p + F32(lam) * merged


def mask_words(seed, model, g):
    """uint32 mask word of every flat element index in g for model `model`: word g & 3 of philox4x32-7(g >> 2, model, MERGE_STREAM, 0)
    under the key (low, high half of seed)."""
    g = np.asarray(g, dtype=np.uint64)
    seed = int(seed)
    w = philox4x32(g >> np.uint64(2), np.uint64(model), np.uint64(MERGE_STREAM), np.uint64(0), np.uint64(seed & 0xFFFFFFFF),
                   np.uint64((seed >> 32) & 0xFFFFFFFF), 7)
    w = np.stack([np.broadcast_to(x, g.shape) for x in w], axis=-1)
    return np.take_along_axis(w, (g & np.uint64(3)).astype(np.int64)[..., None], axis=-1)[..., 0].astype(np.uint32)


def drop_threshold(rate):
    return int(F32(rate) * F32(4294967296.0))


def masked_model(p, f, segs, rate, strategy, weight_format, use_rescale, seed=0, model=0):
    """W_m of mask_merging: the fine-tuned vector f after its mask (magnitude: per parameter tensor)."""
    x = f - p if weight_format == 'delta_weight' else f.copy()
    if strategy == 'random':
        keep = (mask_words(seed, model, np.arange(x.size, dtype=np.uint64)).astype(np.uint64) >= np.uint64(drop_threshold(rate))).astype(F32)
        x = x * keep
    else:
        assert strategy == 'magnitude'
        x = x.copy()
        for s in segs:
            k = int(s[2] * rate)
            if k >= 1:                                  # k == 0 masks nothing (the reference raises there)
                seg = x[s[1]:s[1] + s[2]]
                x[s[1]:s[1] + s[2]] = seg * (~(np.abs(seg) <= kth_abs(seg, k))).astype(F32)
    if use_rescale and float(rate) != 1.0:
        x = x / F32(1.0 - float(rate))
    return p + x if weight_format == 'delta_weight' else x


def merge(p, fs, segs, method='mask_merging', mask_apply_method='average_merging', mask_strategy='random', use_weight_rescale=True,
          weight_format='delta_weight', weight_mask_rate=0.8, weight_mask_rates=None, scaling_coefficient=1.0, param_value_mask_rate=0.8, seed=0):
    """The merged flat vector: the arguments and defaults of pianobart_amd.merge.MergePlan."""
    p, fs = _f(p), [_f(f) for f in fs]
    apply = method
    if method == 'mask_merging':
        rates = [weight_mask_rate] * len(fs) if weight_mask_rates is None else list(weight_mask_rates)
        fs = [masked_model(p, f, segs, rates[m], mask_strategy, weight_format, use_weight_rescale, seed, m) for m, f in enumerate(fs)]
        apply = mask_apply_method
    if apply == 'average_merging':
        return average(fs)
    if apply == 'task_arithmetic':
        return task_arithmetic(p, fs, scaling_coefficient)
    assert apply == 'ties_merging', apply
    return ties(p, fs, param_value_mask_rate, scaling_coefficient)
