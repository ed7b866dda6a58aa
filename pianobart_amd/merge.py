"""Merge fine-tuned PianoBart backbones into one model on the device: average merging, task arithmetic, TIES, and random (DARE) or
magnitude masking of the task vectors (the reference's model_merge.py, model_merging_methods/merging_methods.py and
mask_weights_utils.py).

Every model is packed into ONE flat f32 device vector in the order of the sorted parameter names (the order the reference's TIES uses);
the host keeps the segment table. PyTorch allocates and copies; all arithmetic on parameters runs in pb_merge.hip, float32,
each operation rounded once in the reference's order, so a merge equals the reference's CPU result bit for bit wherever the reference
is deterministic (everything but its torch.bernoulli masks, which are replaced by a counter-based stream of our own).
fisher_merging and regmean_merging need trainers and data and are refused by name."""
import re
from collections import OrderedDict, namedtuple

import numpy as np
import torch

from . import ops
from ._lib import (PBError, MERGE_AVERAGE, MERGE_DELTA, MERGE_FINETUNED, MERGE_MASK_MAGNITUDE, MERGE_MASK_NONE, MERGE_MASK_RANDOM, MERGE_MASKED,
                   MERGE_MAX_MODELS, MERGE_TASK, MERGE_TIES)

METHODS = ('mask_merging', 'average_merging', 'task_arithmetic', 'ties_merging')
NEEDS_TRAINERS = ('fisher_merging', 'regmean_merging')
_APPLY = {'average_merging': MERGE_AVERAGE, 'task_arithmetic': MERGE_TASK, 'ties_merging': MERGE_TIES}

Segment = namedtuple('Segment', 'name offset numel shape')


def _check_method(name, what):
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
                 seed=0, exclude=()):
        _check_method(method, 'method')
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


def segment_table(shapes):
    """[(name, offset, numel, shape)] of the canonical flat vector: names sorted, tensors back to back. shapes: {name: shape}."""
    segs, off = [], 0
    for name in sorted(shapes):
        numel = int(np.prod(shapes[name], dtype=np.int64)) if len(shapes[name]) else 1
        segs.append(Segment(name, off, numel, tuple(shapes[name])))
        off += numel
    return segs


def merge_flat(plan, pre, models, segs):
    """The merged flat vector (a new device tensor) of the flat f32 device vectors `pre` and `models` laid out by `segs`."""
    N, n, dev = len(models), pre.numel(), pre.device
    if N != plan.n_models:
        raise PBError('the plan was made for %d models, got %d' % (plan.n_models, N))
    if n != sum(s.numel for s in segs):
        raise PBError('the segment table covers %d elements, the vectors hold %d' % (sum(s.numel for s in segs), n))
    out = torch.empty_like(pre)
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
    come back as the pre-trained ones. Keyword arguments: see MergePlan."""
    finetuned_sds = list(finetuned_sds)
    plan = MergePlan(len(finetuned_sds), method=method, **kw)
    segs, alias = state_dict_layout(pretrained_sd, plan.exclude)
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
    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    flats = [torch.from_numpy(h).to(dev) for h in host]
    merged = merge_flat(plan, flats[0], flats[1:], segs).cpu()
    out = OrderedDict((k, v.detach().cpu().clone() if torch.is_tensor(v) else v) for k, v in pretrained_sd.items())
    for s in segs:
        t = merged[s.offset:s.offset + s.numel].reshape(s.shape).clone()
        for name in alias[s.name]:
            out[name] = t
    return out
