"""Merge fine-tuned PianoBart backbones into one model on the device: average merging, task arithmetic, TIES, and random (DARE) or
magnitude masking of the task vectors (the reference's model_merge.py, model_merging_methods/merging_methods.py and
mask_weights_utils.py).

Every model is packed into ONE flat f32 device vector in the order of the sorted parameter names (the order the reference's TIES uses);
the host keeps the segment table. PyTorch allocates and copies; all arithmetic on parameters runs in pb_merge.hip, float32,
each operation rounded once in the reference's order, so a merge equals the reference's CPU result bit for bit wherever the reference
is deterministic (everything but its torch.bernoulli masks, which are replaced by a counter-based stream of our own).
fisher_merging takes Fisher weights that fisher_weights() (python -m pianobart_amd.fisher) computes on the device from a fine-tuned model and its
own training data (pb_fisher.hip); without them it is refused by name. regmean_merging takes the Gram matrices of every linear layer's inputs that
regmean_weights() (python -m pianobart_amd.regmean) accumulates from the engine's workspace, and solves W^T = (sum G_m)^-1 sum G_m W_m^T per layer by
a Cholesky factorisation on the device (pb_regmean.hip); without them it is refused by name too."""
import contextlib
import re
from collections import OrderedDict, namedtuple

import numpy as np
import torch

from . import ops
from ._lib import (PBError, MERGE_AVERAGE, MERGE_DELTA, MERGE_FINETUNED, MERGE_MASK_MAGNITUDE, MERGE_MASK_NONE, MERGE_MASK_RANDOM, MERGE_MASKED,
                   MERGE_MAX_MODELS, MERGE_TASK, MERGE_TIES)

METHODS = ('mask_merging', 'average_merging', 'task_arithmetic', 'ties_merging')
FISHER = 'fisher_merging'                                  # a method of its own inputs: one Fisher vector per model (fisher_weights)
REGMEAN = 'regmean_merging'                                # and another: one {weight name: Gram matrix} dict per model (regmean_weights)
NEEDS_TRAINERS = (FISHER, REGMEAN)
_APPLY = {'average_merging': MERGE_AVERAGE, 'task_arithmetic': MERGE_TASK, 'ties_merging': MERGE_TIES}

Segment = namedtuple('Segment', 'name offset numel shape')


def _check_method(name, what, fisher=False, regmean=False):
    if name == REGMEAN and what == 'method':
        if regmean:
            return
        raise PBError("method 'regmean_merging' needs the Gram matrices of every linear layer's inputs, one set per fine-tuned model: compute each "
                      "with merge.regmean_weights(model, batches, ..) or `python -m pianobart_amd.regmean --ckpt ft.ckpt --task .. --dataset .. --output "
                      "ft.regmean.pt` on the model's own training data, then pass regmean_weights=[..] (model_merge: --regmean a.regmean.pt,b.regmean.pt)")
    if name == FISHER and what == 'method':
        if fisher:
            return
        raise PBError("method 'fisher_merging' needs one set of Fisher weights per fine-tuned model: compute each with merge.fisher_weights(model, "
                      "batches, ..) or `python -m pianobart_amd.fisher --ckpt ft.ckpt --task .. --dataset .. --output ft.fisher.pt` on the model's own "
                      "training data, then pass fisher_weights=[..] (model_merge: --fisher a.fisher.pt,b.fisher.pt)")
    if name in NEEDS_TRAINERS:
        raise PBError('%s %r needs the fine-tune trainers and their data (per-example gradients / layer inputs): not part of checkpoint merging '
                      'here. Choose one of %s' % (what, name, ', '.join(METHODS if what == 'method' else sorted(_APPLY))))
    if name not in (METHODS if what == 'method' else _APPLY):
        raise PBError('unknown %s %r (one of %s)' % (what, name, ', '.join(METHODS if what == 'method' else sorted(_APPLY))))


def drop_threshold(rate):
    """An element is dropped where its 32-bit mask word is below uint32(float32(rate) * 2^32); kept as 64 bits so that rate 1 drops all."""
    return int(np.float32(rate) * np.float32(4294967296.0))


def rescale_divisor(rate, use_rescale):
    """The reference divides the masked tensor by the Python float 1 - rate (formed in double, rounded to float32 by the division)."""
    return float(np.float32(1.0 - float(rate))) if use_rescale and float(rate) != 1.0 else 1.0


class MergePlan:
    """What a merge does, checked before any device work. The names and defaults are the reference's (MergingMethod.get_merged_model)."""

    def __init__(self, n_models, method='mask_merging', mask_apply_method='average_merging', mask_strategy='random', use_weight_rescale=True,
                 weight_format='delta_weight', weight_mask_rate=0.8, weight_mask_rates=None, scaling_coefficient=1.0, param_value_mask_rate=0.8,
                 seed=0, exclude=(), fisher_weights=None, fisher_scaling_coefficients=None, normalize_fisher_weight=True, minimal_fisher_weight=1e-6,
                 fisher_norms=None, regmean_weights=None, reduce_non_diagonal_ratio=1.0):
        _check_method(method, 'method', fisher=fisher_weights is not None, regmean=regmean_weights is not None)
        if method == 'mask_merging':
            _check_method(mask_apply_method, 'mask_apply_method')
            if mask_strategy not in ('random', 'magnitude'):
                raise PBError("mask_strategy %r: 'random' or 'magnitude'" % (mask_strategy,))
            if weight_format not in ('delta_weight', 'finetuned_weight'):
                raise PBError("weight_format %r: 'delta_weight' or 'finetuned_weight'" % (weight_format,))
        if n_models < 2:
            raise PBError('merging needs at least two fine-tuned models (got %d)' % n_models)
        if n_models > MERGE_MAX_MODELS:
            raise PBError('merging takes at most %d models at a time (got %d)' % (MERGE_MAX_MODELS, n_models))
        rates = [float(weight_mask_rate)] * n_models if weight_mask_rates is None else [float(r) for r in weight_mask_rates]
        if len(rates) != n_models:
            raise PBError('weight_mask_rates names %d rates for %d models' % (len(rates), n_models))
        for r in rates + [float(param_value_mask_rate)]:
            if not 0.0 <= r <= 1.0:
                raise PBError('a mask rate must lie in [0, 1] (got %r)' % (r,))
        self.n_models, self.method = n_models, method
        self.apply = mask_apply_method if method == 'mask_merging' else method
        self.masked = method == 'mask_merging'
        self.strategy, self.rescale, self.format = mask_strategy, bool(use_weight_rescale), weight_format
        self.rates, self.lam, self.ties_rate = rates, float(scaling_coefficient), float(param_value_mask_rate)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.exclude = [exclude] if isinstance(exclude, str) else list(exclude or ())
        self.regmean = method == REGMEAN
        if self.regmean:
            self.regmean_weights = list(regmean_weights)
            if len(self.regmean_weights) != n_models:
                raise PBError('regmean_weights holds %d sets of Gram matrices for %d models' % (len(self.regmean_weights), n_models))
            self.ratio = float(reduce_non_diagonal_ratio)
            if not 0.0 <= self.ratio <= 1.0:                                   # NaN fails both comparisons
                raise PBError('reduce_non_diagonal_ratio must lie in [0, 1] (got %r)' % (reduce_non_diagonal_ratio,))
        self.fisher = method == FISHER
        if self.fisher:
            self.fisher_weights = list(fisher_weights)
            if len(self.fisher_weights) != n_models:
                raise PBError('fisher_weights holds %d sets of Fisher weights for %d models' % (len(self.fisher_weights), n_models))
            self.minimal = float(minimal_fisher_weight)
            if not (self.minimal > 0.0 and np.isfinite(np.float32(self.minimal)) and np.float32(self.minimal) > 0):
                raise PBError('minimal_fisher_weight must be positive and finite in float32 (got %r): it keeps every denominator above 0' % (minimal_fisher_weight,))
            self.coefficients = None if fisher_scaling_coefficients is None else [float(c) for c in fisher_scaling_coefficients]
            if self.coefficients is not None:
                if len(self.coefficients) != n_models:
                    raise PBError('fisher_scaling_coefficients names %d coefficients for %d models' % (len(self.coefficients), n_models))
                if not all(c > 0.0 and np.isfinite(c) for c in self.coefficients):
                    raise PBError('fisher_scaling_coefficients must be positive and finite (got %r)' % (self.coefficients,))
            self.normalize = bool(normalize_fisher_weight)
            self.norms = None if fisher_norms is None else [float(v) for v in fisher_norms]
            if self.norms is not None and (len(self.norms) != n_models or not all(v >= 0.0 and np.isfinite(v) for v in self.norms)):
                raise PBError('fisher_norms must hold one finite norm >= 0 per model (got %r for %d models)' % (self.norms, n_models))


def torch_sum_f32(x):
    """The float32 sum of at most 8 values as the reference's `tensor.sum()` takes it on the CPU (ATen's cascade sum, 8 float lanes): a row
    of 8 is added lane by lane from +0, left to right; a shorter row goes through four interleaved partial sums p_k = x_k + x_(k+4) + ..,
    then the elements behind the last whole group of 4 onto p_0, then (p_0 + p_1) + p_2 + p_3. Below 4 values that is left to right."""
    x = np.asarray(x, dtype=np.float32)
    assert x.ndim == 1 and x.size <= 8
    if x.size == 8:
        s = np.float32(0.0)
        for v in x:
            s = np.float32(s + v)
        return s
    q = x.size // 4
    p = [np.float32(0.0)] * 4
    for i in range(q):
        for k in range(4):
            p[k] = np.float32(p[k] + x[4 * i + k])
    for v in x[4 * q:]:
        p[0] = np.float32(p[0] + v)
    for k in range(1, 4):
        p[0] = np.float32(p[0] + p[k])
    return p[0]


def fisher_coefficients(n_models, coefficients=None, normalize=True, minimal=1e-6, norms=None):
    """The N float32 coefficients c_m of a Fisher merge, formed as the reference forms them (merging_methods.py:160-167, 254-259):
    ones(N) / N or the given list; with `normalize` times r_m / sum(r), r_m = 1 / (norm_m + minimal)."""
    f32 = np.float32
    c = np.ones(n_models, dtype=f32) / f32(n_models) if coefficients is None else np.asarray(coefficients, dtype=f32)
    if normalize:
        r = f32(1.0) / (np.asarray(norms, dtype=f32) + f32(minimal))
        c = c * (r / torch_sum_f32(r))
    return c.astype(f32)


def segment_table(shapes):
    """[(name, offset, numel, shape)] of the canonical flat vector: names sorted, tensors back to back. shapes: {name: shape}."""
    segs, off = [], 0
    for name in sorted(shapes):
        numel = int(np.prod(shapes[name], dtype=np.int64)) if len(shapes[name]) else 1
        segs.append(Segment(name, off, numel, tuple(shapes[name])))
        off += numel
    return segs


def regmean_factors(ratio):
    """(off, diag): the float32 factors of reduce_non_diagonal_elements as the reference's float32 tensors evaluate them
    (merging_methods.py:309-313): off = float32(ratio), diag = (1 - ratio) + ratio with every operation in float32, which is not always 1."""
    off = torch.zeros(1, dtype=torch.float32).fill_(float(ratio))
    diag = (torch.ones(1, dtype=torch.float32) - float(ratio)) + off
    return float(off.item()), float(diag.item())


def regmean_groups(regmean, segs):
    """[[Segment, ..]]: the segments with Gram matrices, those whose matrices are ONE tensor in every model's dict (q / k / v of an attention
    block; every decoder layer's cross-attention k / v) together: they share a factorisation and go as one stacked right-hand side."""
    groups = OrderedDict()
    for s in segs:
        if s.name in regmean[0]:
            groups.setdefault(tuple(r[s.name].data_ptr() for r in regmean), []).append(s)
    return list(groups.values())


def _regmean_flat(plan, pre, models, segs, regmean, out):
    """out = the plain mean of the fine-tuned vectors (the MERGE_AVERAGE pass), then per group of weights with Gram matrices
    S = sum_m G'_m, R (K, outs) = sum_m G'_m W_m^T, S = L L^T, L L^T Z = R, W = Z^T written over the mean. G'_m = scale(G_m)."""
    from ._lib import PB_F32
    N, dev = len(models), pre.device
    ops.merge_apply(ops.merge_desc(pre, models, out, method=MERGE_AVERAGE, lam=plan.lam))
    off, diag = regmean_factors(plan.ratio)
    groups = regmean_groups(regmean, segs)
    info = torch.zeros(max(1, len(groups)), dtype=torch.int32, device=dev)     # one word per factorisation, read once at the end
    for gi, members in enumerate(groups):
        K, outs = members[0].shape[1], [s.shape[0] for s in members]
        nout = sum(outs)
        S, R, Gs = (torch.zeros(K, K, dtype=torch.float32, device=dev), torch.zeros(K, nout, dtype=torch.float32, device=dev),
                    torch.empty(K, K, dtype=torch.float32, device=dev))
        for m in range(N):
            ops.regmean_scale(regmean[m][members[0].name], Gs, off, diag)
            ops.accum_f32(S, Gs)
            o = 0
            for s, n_out in zip(members, outs):                                 # R[:, o : o + out] += G' W^T: NT form, W is (out, K)
                ops.gemm(Gs, models[m][s.offset:s.offset + s.numel], R, M=K, N=n_out, K=K, dtype=PB_F32, ldc=nout, c_off=o, accum=True)
                o += n_out
        ops.chol_factor(S, info[gi:gi + 1])
        ops.chol_solve(S, R)
        o = 0
        for s, n_out in zip(members, outs):
            ops.transpose_f32(R[:, o:o + n_out], out[s.offset:s.offset + s.numel].view(n_out, K))
            o += n_out
    for gi, col in enumerate(info.cpu().tolist()):
        if col and groups:
            raise PBError('%s: the summed Gram matrix is not positive definite (pivot of column %d of %d is <= 0 or not finite): too few rows for '
                          'its %d inputs, or an input that is identically 0' % (', '.join(s.name for s in groups[gi]), col - 1, groups[gi][0].shape[1],
                                                                                groups[gi][0].shape[1]))
    return out


def merge_flat(plan, pre, models, segs, fishers=None, regmean=None):
    """The merged flat vector (a new device tensor) of the flat f32 device vectors `pre` and `models` laid out by `segs`. A Fisher plan
    also takes `fishers`: one flat Fisher vector per model in the same layout (`pre` then only gives the size); a RegMean plan `regmean`:
    per model {segment name: (K, K) f32 device tensor} (regmean_groups tells which weights share one)."""
    N, n, dev = len(models), pre.numel(), pre.device
    if N != plan.n_models:
        raise PBError('the plan was made for %d models, got %d' % (plan.n_models, N))
    if n != sum(s.numel for s in segs):
        raise PBError('the segment table covers %d elements, the vectors hold %d' % (sum(s.numel for s in segs), n))
    out = torch.empty_like(pre)
    if plan.regmean:
        if regmean is None or len(regmean) != N:
            raise PBError('a regmean_merging plan takes one {segment name: (K, K) device tensor} dict per model')
        return _regmean_flat(plan, pre, models, segs, regmean, out)
    if plan.fisher:
        if fishers is None or len(fishers) != N:
            raise PBError('a fisher_merging plan takes one flat Fisher vector per model')
        norms = plan.norms
        if plan.normalize and norms is None:                                    # L2 norm of each model's whole Fisher vector, on the device
            ws, dn = ops.fisher_norm_ws(dev), torch.empty(N, dtype=torch.float32, device=dev)
            for m in range(N):
                ops.fisher_norm(fishers[m], ws, dn[m:m + 1])
            norms = dn.cpu().numpy()
            if not np.isfinite(norms).all():
                raise PBError('the norm of a Fisher vector is not finite: refusing to merge')
        coef = fisher_coefficients(N, plan.coefficients, plan.normalize, plan.minimal, norms)
        if not (np.isfinite(coef).all() and (coef > 0).all()):
            raise PBError('the Fisher coefficients %r are not positive and finite (norms %r)' % (coef.tolist(), None if norms is None else list(norms)))
        ops.fisher_merge(ops.fisher_desc(models, fishers, out, coef, np.float32(plan.minimal)))
        return out
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = ops.merge_kth_ws(dev)
    fmt = MERGE_FINETUNED if plan.masked and plan.format == 'finetuned_weight' else MERGE_DELTA
    method = _APPLY[plan.apply]

    def ties(ms, dst):
        thr = torch.zeros(N, dtype=torch.float32, device=dev)                  # bit pattern 0: nothing trimmed when int(n * rate) == 0
        k = int(n * plan.ties_rate)
        if k >= 1:
            for m in range(N):
                ops.merge_kth_abs(ms[m], pre, k, thr[m:m + 1], flags, ws)
        tally = torch.zeros(2, dtype=torch.int64, device=dev)
        d = ops.merge_desc(pre, ms, dst, method=MERGE_TIES, lam=plan.lam, thresh=[thr[m:m + 1] for m in range(N)], tally=tally)
        ops.merge_sign_tally(d)
        ops.merge_apply(d)

    if not plan.masked:
        if method == MERGE_TIES:
            ties(models, out)
        else:
            ops.merge_apply(ops.merge_desc(pre, models, out, method=method, lam=plan.lam))
    else:
        magnitude = plan.strategy == 'magnitude'
        kinds = [MERGE_MASK_MAGNITUDE if magnitude else MERGE_MASK_RANDOM] * N
        common = dict(fmt=fmt, lam=plan.lam, seed=plan.seed, drop_thresh=[drop_threshold(r) for r in plan.rates],
                      rescale=[rescale_divisor(r, plan.rescale) for r in plan.rates])
        pieces = segs if magnitude else [Segment('', 0, n, (n,))]               # magnitude thresholds are per parameter tensor
        thr = torch.zeros(len(pieces) * N, dtype=torch.float32, device=dev) if magnitude else None
        if magnitude:
            for i, s in enumerate(pieces):
                for m in range(N):
                    k = int(s.numel * plan.rates[m])                            # k == 0 masks nothing (the reference raises): the threshold stays 0
                    if k >= 1:
                        sl = slice(s.offset, s.offset + s.numel)
                        ops.merge_kth_abs(models[m][sl], pre[sl] if fmt == MERGE_DELTA else None, k, thr[i * N + m:i * N + m + 1], flags, ws)
        masked = [torch.empty_like(pre) for _ in range(N)] if method == MERGE_TIES else None
        for i, s in enumerate(pieces):
            if s.numel == 0:
                continue
            sl = slice(s.offset, s.offset + s.numel)
            th = [thr[i * N + m:i * N + m + 1] for m in range(N)] if magnitude else None
            if masked is None:
                ops.merge_apply(ops.merge_desc(pre[sl], [f[sl] for f in models], out[sl], method=method, kinds=kinds, thresh=th, g0=s.offset, **common))
            else:                                                               # TIES trims over the whole vector of each MASKED model: write those first
                for m in range(N):                                              # model_base = m: model m keeps its own mask stream
                    ops.merge_apply(ops.merge_desc(pre[sl], [models[m][sl]], masked[m][sl], method=MERGE_MASKED, kinds=[kinds[m]], thresh=[th[m]] if th else None,
                                                   g0=s.offset, model_base=m, **{k: ([v[m]] if isinstance(v, list) else v) for k, v in common.items()}))
        if masked is not None:
            ties(masked, out)
    if int(flags.item()):
        raise PBError('a parameter (or its difference from the pre-trained one) is inf or NaN: refusing to merge')
    return out


def backbone_state_dict(sd, own, label=''):
    """The backbone tensors of a checkpoint as this project's trainers write it: {'state_dict': ...} or a bare dict; a `module.` prefix
    (nn.DataParallel) is stripped through checkpoint_state_dict and a `pianobart.` prefix (the fine-tune wrappers) too; keys outside
    `own` (classification heads, LM heads) are dropped with a message. A file with no backbone key is refused: the reference's
    strict=False would merge random weights without a word."""
    from .model import checkpoint_state_dict
    if isinstance(sd, dict) and 'state_dict' in sd and isinstance(sd['state_dict'], dict):
        sd = sd['state_dict']
    sd = checkpoint_state_dict(sd)
    out, dropped = OrderedDict(), []
    for k, v in sd.items():
        k2 = k[len('pianobart.'):] if k.startswith('pianobart.') else k
        if k2 in own:
            out[k2] = v
        else:
            dropped.append(k)
    print('   [merge] %s: %d of %d backbone keys matched' % (label or 'checkpoint', len(out), len(own)))
    if dropped:
        print('   [merge] %s: dropped %d keys that are not backbone parameters (first: %r)' % (label or 'checkpoint', len(dropped), dropped[0]))
    if not out:
        raise PBError('%s: none of its %d keys names a backbone parameter (first key: %r): refusing to merge an unloaded model'
                      % (label or 'checkpoint', len(sd), next(iter(sd), None)))
    return out


def state_dict_layout(pretrained_sd, exclude=()):
    """(segment table, {representative name: [every name of that parameter]}) of the tensors of `pretrained_sd` that a merge covers:
    float32, no `exclude` regex matching (re.match, as the reference), names that share storage (tied tables) counted once."""
    groups, shapes = OrderedDict(), {}
    for name in sorted(pretrained_sd):
        t = pretrained_sd[name]
        if not torch.is_tensor(t) or not t.is_floating_point() or any(re.match(p, name) for p in exclude):
            continue
        if t.dtype != torch.float32:
            raise PBError('%s is %s: only float32 checkpoints are merged' % (name, t.dtype))
        key = (t.data_ptr(), tuple(t.shape)) if t.numel() else ('empty', name)
        if key in groups:
            groups[key].append(name)
            continue
        groups[key] = [name]
        shapes[name] = tuple(t.shape)
    if not shapes:
        raise PBError('nothing to merge: no float32 parameter is left after the exclusions')
    return segment_table(shapes), {names[0]: names for names in groups.values()}


def merge_state_dicts(pretrained_sd, finetuned_sds, method='mask_merging', device=None, **kw):
    """Merged backbone state dict (CPU tensors, the keys of `pretrained_sd`: what PianoBart.state_dict() holds).

    Merged: every float32 tensor of `pretrained_sd` whose name no `exclude` regex matches (re.match, as the reference). Names that share
    storage in `pretrained_sd` (tied tables) are one parameter, as in the reference's named_parameters(). Excluded and non-float entries
    come back as the pre-trained ones. Keyword arguments: see MergePlan.

    method='fisher_merging' takes fisher_weights=[{name: f32 tensor}, ..], one dict per model as fisher_weights() returns it, and
    fisher_scaling_coefficients / normalize_fisher_weight / minimal_fisher_weight with the reference's meaning; fisher_norms=[..]
    overrides the device's norms of the Fisher vectors. A merged parameter that no Fisher dict names (BART's never-read `shared`
    table: its gradient is identically 0) has Fisher weight 0 and comes out as the coefficient-weighted mean.

    method='regmean_merging' takes regmean_weights=[{weight name: (K, K) f32 Gram matrix}, ..], one dict per model as regmean_weights()
    returns it, and reduce_non_diagonal_ratio (default 1.0: the matrices as they are) with the reference's meaning. Every 2-D `.weight` with
    an entry becomes (sum_m G'_m)^-1 sum_m G'_m W_m^T, transposed back; every other merged parameter is the plain mean of the fine-tuned
    values (what method='average_merging' gives). The pre-trained model supplies names, shapes, exclusions and tied-table aliases only.
    A summed Gram matrix that is not positive definite is a PBError that names the weight."""
    finetuned_sds = list(finetuned_sds)
    plan = MergePlan(len(finetuned_sds), method=method, **kw)
    segs, alias = state_dict_layout(pretrained_sd, plan.exclude)
    if plan.fisher:
        check_fisher_dicts(plan.fisher_weights, pretrained_sd, segs, alias)
    if plan.regmean:
        check_regmean_dicts(plan.regmean_weights, segs, alias)
    for s in segs:
        for i, sd in enumerate(finetuned_sds):
            if s.name not in sd:
                raise PBError('fine-tuned model %d has no parameter %s' % (i, s.name))
            if tuple(sd[s.name].shape) != s.shape or sd[s.name].dtype != torch.float32:
                raise PBError('%s: fine-tuned model %d holds %s %s, the pre-trained model %s float32' % (s.name, i, tuple(sd[s.name].shape), sd[s.name].dtype, s.shape))
    n = segs[-1].offset + segs[-1].numel

    def pack(sd, who):
        flat = np.empty(n, dtype=np.float32)
        for s in segs:
            a = sd[s.name].detach().cpu().contiguous().numpy().reshape(-1)
            if not np.isfinite(a).all():
                raise PBError('%s: %s holds a non-finite value: refusing to merge' % (who, s.name))
            flat[s.offset:s.offset + s.numel] = a
        return flat

    host = [pack(pretrained_sd, 'the pre-trained model')] + [pack(sd, 'fine-tuned model %d' % i) for i, sd in enumerate(finetuned_sds)]
    fhost = [pack_fisher(fw, segs, alias, n, i) for i, fw in enumerate(plan.fisher_weights)] if plan.fisher else None
    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    flats = [torch.from_numpy(h).to(dev) for h in host]
    fishers = [torch.from_numpy(h).to(dev) for h in fhost] if plan.fisher else None
    regmean = None
    if plan.regmean:                                                            # a tensor that several names share goes to the device once and stays shared
        on_dev, regmean = {}, []
        for rw in plan.regmean_weights:
            by_seg = {}
            for s in segs:
                t = _fisher_entry(rw, alias[s.name])
                if t is not None:
                    key = (t.device, t.data_ptr())
                    if key not in on_dev:
                        on_dev[key] = (t, t.detach().to(dev).contiguous())      # (the source is kept alive: its address is the key)
                    by_seg[s.name] = on_dev[key][1]
            regmean.append(by_seg)
    merged = merge_flat(plan, flats[0], flats[1:], segs, fishers, regmean).cpu()
    out = OrderedDict((k, v.detach().cpu().clone() if torch.is_tensor(v) else v) for k, v in pretrained_sd.items())
    for s in segs:
        t = merged[s.offset:s.offset + s.numel].reshape(s.shape).clone()
        for name in alias[s.name]:
            out[name] = t
    return out


def _fisher_entry(fw, names):
    for name in names:
        if name in fw:
            return fw[name]
    return None


def check_fisher_dicts(fisher_weights, pretrained_sd, segs, alias):
    """Refuses, before any device work: a Fisher dict that is empty or names something the model does not hold, dicts that name different
    parameters, and a shape or dtype that is not the parameter's."""
    first = None
    for i, fw in enumerate(fisher_weights):
        if not isinstance(fw, dict) or not fw:
            raise PBError('Fisher weights of model %d: expected a non-empty {name: tensor} dict' % i)
        unknown = [k for k in fw if k not in pretrained_sd]
        if unknown:
            raise PBError('Fisher weights of model %d name %d parameters the model does not hold (first: %s)' % (i, len(unknown), unknown[0]))
        covered = {s.name for s in segs if _fisher_entry(fw, alias[s.name]) is not None}     # by parameter: a tied table may come under any of its names
        if first is None:
            first = covered
        elif covered != first:
            raise PBError('Fisher weights of model %d and of model 0 name different parameters (first: %s)' % (i, sorted(covered ^ first)[0]))
        for s in segs:
            t = _fisher_entry(fw, alias[s.name])
            if t is None:
                continue
            if not torch.is_tensor(t) or tuple(t.shape) != s.shape or t.dtype != torch.float32:
                raise PBError('Fisher weights of model %d: %s is %s %s, the parameter %s float32' % (
                    i, s.name, tuple(t.shape) if torch.is_tensor(t) else type(t).__name__, getattr(t, 'dtype', ''), s.shape))


def pack_fisher(fw, segs, alias, n, i):
    """One model's Fisher dict as a flat host vector in the layout of `segs` (a parameter without an entry: 0); a negative or non-finite
    value is refused."""
    flat = np.zeros(n, dtype=np.float32)
    for s in segs:
        t = _fisher_entry(fw, alias[s.name])
        if t is None:
            continue
        a = t.detach().cpu().contiguous().numpy().reshape(-1)
        if not (np.isfinite(a).all() and (a >= 0).all()):
            raise PBError('Fisher weights of model %d: %s holds a negative or non-finite value: refusing to merge' % (i, s.name))
        flat[s.offset:s.offset + s.numel] = a
    return flat


@contextlib.contextmanager
def _training_without_dropout(model, eng):
    """The state both data passes run in: training mode (the engine then keeps every activation of the forward in its workspace) with
    every dropout probability 0. Module modes, probabilities and the engine's p_drop come back as found, and no .grad stays set."""
    modes = [(m, m.training) for m in model.modules()]
    drops = [(m, m.p) for m in model.modules() if isinstance(m, torch.nn.Dropout)]
    p_drop = eng.p_drop
    try:
        model.train()
        eng.p_drop = 0.0
        for m, _ in drops:
            m.p = 0.0
        yield
    finally:
        model.zero_grad()
        eng.p_drop = p_drop
        for m, p in drops:
            m.p = p
        for m, t in modes:
            m.training = t


def check_regmean_dicts(regmean_weights, segs, alias):
    """Refuses, before any device work: a dict that is empty or names something that is not a merged 2-D `.weight`, dicts that name different
    parameters, an entry that is not a float32 (K, K) matrix with K the weight's in_features, and one that is not finite or not symmetric
    to 1e-6 of its largest diagonal element."""
    seg_of = {name: s for s in segs for name in alias[s.name]}
    first, seen = None, {}
    for i, rw in enumerate(regmean_weights):
        if not isinstance(rw, dict) or not rw:
            raise PBError('RegMean weights of model %d: expected a non-empty {weight name: (K, K) tensor} dict' % i)
        unknown = [k for k in rw if k not in seg_of]
        if unknown:
            raise PBError('RegMean weights of model %d name %d entries that are no merged parameter (first: %s)' % (i, len(unknown), unknown[0]))
        covered = {seg_of[k].name for k in rw}
        if first is None:
            first = covered
        elif covered != first:
            raise PBError('RegMean weights of model %d and of model 0 name different parameters (first: %s)' % (i, sorted(covered ^ first)[0]))
        for k, t in rw.items():
            s = seg_of[k]
            if not k.endswith('.weight') or len(s.shape) != 2:
                raise PBError('RegMean weights of model %d: %s is not the 2-D weight of a linear layer (shape %s)' % (i, k, s.shape))
            K = s.shape[1]
            if not torch.is_tensor(t) or tuple(t.shape) != (K, K) or t.dtype != torch.float32:
                raise PBError('RegMean weights of model %d: %s is %s %s, expected a float32 (%d, %d) Gram matrix of the in_features of the %s weight'
                              % (i, k, tuple(t.shape) if torch.is_tensor(t) else type(t).__name__, getattr(t, 'dtype', ''), K, K, s.shape))
            key = (t.device, t.data_ptr())
            if key in seen:                                                     # a matrix several names share is looked at once
                continue
            seen[key] = t
            c = t.detach().cpu()
            if not bool(torch.isfinite(c).all()):
                raise PBError('RegMean weights of model %d: %s holds a non-finite value: refusing to merge' % (i, k))
            if float((c - c.t()).abs().max()) > 1e-6 * float(c.diagonal().max()):
                raise PBError('RegMean weights of model %d: %s is not symmetric to 1e-6 of its largest diagonal element: not a Gram matrix' % (i, k))


def regmean_weights(model, batches, num_examples, seq, device=None):
    """{name of a backbone Linear weight: (K, K) f32 Gram matrix of its inputs (on `device`)}: G = X^T X / rows over the model's own training
    data, as the reference's regmean_merging collects it with forward hooks (merging_methods.py:330-388).

    model: a SequenceClassification (seq=True) or TokenClassification (seq=False) over a PianoBart of any precision; batches yields (x, y) as
    the fine-tune loaders do; inputs are prepared by finetune.prepare_inputs. Per batch ONE dense forward, then one pb_gram_accum per entry of
    Engine.linear_inputs(): the workspace already holds every layer's input. All B * S rows of the padded batch count, PAD positions
    included (the reference's hook sees x.reshape(-1, K)). The loop ends before a batch once the examples counted (+= the batch's actual
    size) reach num_examples; every sum is divided ONCE by the rows counted (the reference keeps a running mean of per-batch means: the
    same number in exact arithmetic, here with one rounding instead of one per batch). Names that read the same input (q / k / v; every
    decoder layer's cross-attention k / v) hold the SAME tensor. encoder_linear.weight has no entry (its input is never materialised)
    and is therefore averaged by the merge, as the reference averages a weight without RegMean weights; heads are never merged. Dropout,
    module modes and parameters are left as found."""
    return regmean_pass(model, batches, num_examples, seq, device)[0]


def regmean_pass(model, batches, num_examples, seq, device=None):
    """(regmean_weights' result, the rows counted: the divisor, the examples counted)."""
    from .finetune import prepare_inputs
    num_examples = int(num_examples)
    if num_examples < 1:
        raise PBError('regmean_weights: num_examples = %d must be positive' % num_examples)
    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    if dev.type != 'cuda':
        raise PBError('pianobart_amd has no CPU execution path')
    pb = model.pianobart
    model.to(dev)
    eng = pb._get_engine()
    eng.bind(dev)
    class_num = model.classifier[3].out_features - (0 if seq else 1)
    grams, shared, ws = OrderedDict(), {}, {}
    num_rows = num_counted = 0
    with _training_without_dropout(model, eng), torch.no_grad():
        for x, y in batches:
            if num_counted >= num_examples:
                break
            x, y, attn, inputs = prepare_inputs(x, y, dev, pb.bar_pad_word, class_num, seq)
            model(**inputs)
            for key, X, names in eng.linear_inputs():
                T, K = X.shape
                if key not in grams:
                    grams[key] = torch.zeros(K, K, dtype=torch.float32, device=dev)
                    shared[key] = names
                if (T, K) not in ws:
                    ws[(T, K)] = ops.gram_ws(T, K, dev)
                ops.gram_accum(grams[key], X, ws[(T, K)])
            num_rows += x.shape[0] * x.shape[1]
            num_counted += x.shape[0]
    if num_counted == 0:
        raise PBError('regmean_weights: the loader gave no batch')
    if num_rows > 1 << 24:
        raise PBError('regmean_weights: %d rows counted; the divisor must stay exact in float32 (at most 2^24 rows)' % num_rows)
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    for G in grams.values():
        ops.fisher_finish(G.view(-1), num_rows, flags)                          # G /= float32(rows); flags where a result is not finite
    if int(flags.item()):
        raise PBError('a Gram matrix holds inf or NaN (an activation overflowed or the model holds a non-finite value)')
    out = OrderedDict()
    for key, G in grams.items():
        for name in shared[key]:
            out[name] = G
    print('   [regmean] encoder_linear.weight has no Gram matrix (its input, eight concatenated embedding rows, is never materialised): '
          'a merge averages it')
    return out, num_rows, num_counted


def fisher_weights(model, batches, num_examples, batch_size, seq, device=None):
    """{backbone parameter name: f32 tensor (on `device`)}: the diagonal of the empirical Fisher information of a fine-tuned classifier on its
    own training data, as the reference's fisher_merging computes it (merging_methods.py:189-250).

    model: a SequenceClassification (seq=True) or TokenClassification (seq=False) over a PianoBart of any precision; batches yields (x, y)
    as the fine-tune loaders do; inputs are prepared as FinetuneTrainer.iteration prepares them (finetune.prepare_inputs). Per batch the
    objective E = sum over rows and classes of sqrt(p).detach() * log_softmax(logits) is differentiated through the engine's backward into
    its flat f32 gradient buffer, and F += grad^2 is ONE pb_fisher_accum launch over that buffer: the square of the gradient summed over the
    batch, as in the reference. The loop ends before a batch once num_computed >= num_examples; num_computed grows by batch_size per batch
    (a short last batch too), and F / num_computed is the result. Token tasks (an extension of ours: the reference handles (B, C) logits)
    sum over the non-pad positions. The pass runs without dropout (every probability is 0 for its duration), takes no optimizer step and
    leaves the weights as they were. Only parameters the engine holds get Fisher weights -- under every name the backbone's state dict
    gives them (tied tables are one parameter) --, never a head's."""
    return fisher_pass(model, batches, num_examples, batch_size, seq, device)[0]


def fisher_pass(model, batches, num_examples, batch_size, seq, device=None):
    """(fisher_weights' result, num_computed: the divisor it used)."""
    from . import heads
    from .finetune import prepare_inputs
    num_examples, batch_size = int(num_examples), int(batch_size)
    if num_examples < 1 or batch_size < 1:
        raise PBError('fisher_weights: num_examples = %d and batch_size = %d must be positive' % (num_examples, batch_size))
    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    if dev.type != 'cuda':
        raise PBError('pianobart_amd has no CPU execution path')
    pb = model.pianobart
    model.to(dev)
    eng = pb._get_engine()
    eng.bind(dev)
    class_num = model.classifier[3].out_features - (0 if seq else 1)           # the trainer's class_num: token heads hold one more (the pad label)
    F = torch.zeros_like(eng.G32)
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    num_computed = 0
    with _training_without_dropout(model, eng), torch.enable_grad():
        for x, y in batches:
            if num_computed >= num_examples:
                break
            x, y, attn, inputs = prepare_inputs(x, y, dev, pb.bar_pad_word, class_num, seq)
            logits = model(**inputs)
            e = heads.fisher_expectation_rows(logits, None if seq else attn)
            model.zero_grad()                                               # .grad = None: the backward then writes the engine's primary buffer
            e.sum().backward()
            ops.fisher_accum(F, eng.G32)
            num_computed += batch_size
    if num_computed == 0:
        raise PBError('fisher_weights: the loader gave no batch')
    ops.fisher_finish(F, num_computed, flags)
    if int(flags.item()):
        raise PBError('a Fisher weight is inf or NaN (a gradient overflowed or the model holds a non-finite value)')
    slot = {id(p): i for i, p in enumerate(eng.params)}
    views = eng.grad_views_of(F)
    out = OrderedDict()
    for name, p in pb.state_dict(keep_vars=True).items():
        if id(p) in slot:
            out[name] = views[slot[id(p)]]
    return out, num_computed
