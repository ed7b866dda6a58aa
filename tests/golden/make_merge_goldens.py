"""Writes tests/golden/g15_merge.npz: the reference's own merge results on a toy module (run once, on the CPU).

    python tests/golden/make_merge_goldens.py --reference <directory that holds the reference's model_merging_methods/ and utils/>

The reference's MergingMethod is imported at generation time only; no test reads the reference. The file holds arrays only, every
model as ONE flat float32 vector in the order of the sorted parameter names (the canonical layout of pianobart_amd/merge.py):
    names (str), shapes (len(names), 3) int64, unused dimensions 0      the segment table
    pre (n), ft (3, n)                                                  the pre-trained toy module and its 3 perturbed copies
    out/<case> (n)                                                      MergingMethod.merging_models(...) of the case
Cases: average, task (task_arithmetic, 0.7), ties (ties_merging, rate 0.8, 1.0), and mask_merging with magnitude masks at rates
0.8 / 0.5 / 0.9 as mag/<apply>/<format>/<rescale|plain> for the three apply methods, both weight formats, with and without rescale
(task arithmetic and TIES under a mask use the scaling coefficient 0.7). Random masks are not recorded: torch.bernoulli's stream is
not part of the contract."""
import argparse
import copy
import os
import sys

import numpy as np
import torch
import torch.nn as nn

RATES = [0.8, 0.5, 0.9]
LAMBDA = 0.7
TIES_RATE = 0.8


class Toy(nn.Module):
    """1 258 parameters: rank 1 (biases, LayerNorm), rank 2 (embedding, linears), rank 3 (a 1-D convolution)."""

    def __init__(self):
        super().__init__()
        self.emb = nn.Embedding(11, 16)
        self.proj = nn.Linear(16, 24)
        self.conv = nn.Conv1d(4, 6, 5)
        self.norm = nn.LayerNorm(24)
        self.head = nn.Linear(24, 20)


def make_models(seed=15):
    g = torch.Generator().manual_seed(seed)
    pre = Toy()
    with torch.no_grad():
        for p in pre.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    fts = []
    for i in range(3):
        m = copy.deepcopy(pre)
        with torch.no_grad():
            for p in m.parameters():
                step = torch.randn(p.shape, generator=g) * (0.01 * (i + 1))
                step[torch.rand(p.shape, generator=g) < 0.05] = 0.0           # untouched elements: ties in the magnitude order, zero task-vector entries
                p.add_(step)
        fts.append(m)
    return pre, fts


def cases():
    yield 'average', dict(method='average_merging')
    yield 'task', dict(method='task_arithmetic', scaling_coefficient=LAMBDA)
    yield 'ties', dict(method='ties_merging', param_value_mask_rate=TIES_RATE, scaling_coefficient=1.0)
    for apply in ('average_merging', 'task_arithmetic', 'ties_merging'):
        for fmt in ('delta_weight', 'finetuned_weight'):
            for rescale in (True, False):
                yield 'mag/%s/%s/%s' % (apply, fmt, 'rescale' if rescale else 'plain'), dict(
                    method='mask_merging', mask_apply_method=apply, mask_strategy='magnitude', weight_format=fmt, use_weight_rescale=rescale,
                    weight_mask_rates=RATES, scaling_coefficient=LAMBDA, param_value_mask_rate=TIES_RATE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), 'g15_merge.npz'))
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    from model_merging_methods.merging_methods import MergingMethod

    pre, fts = make_models()
    names = sorted(n for n, _ in pre.named_parameters())
    shapes = {n: tuple(p.shape) for n, p in pre.named_parameters()}

    def flat(params):
        params = dict(params)
        return np.concatenate([params[n].detach().numpy().astype(np.float32).reshape(-1) for n in names])

    arrays = {'names': np.array(names), 'shapes': np.array([list(shapes[n]) + [0] * (3 - len(shapes[n])) for n in names], dtype=np.int64),
              'pre': flat(pre.named_parameters()), 'ft': np.stack([flat(f.named_parameters()) for f in fts])}
    for case, kw in cases():
        kw = dict(kw)
        method = kw.pop('method')
        merged = MergingMethod(merging_method_name=method).merging_models(
            merged_model=copy.deepcopy(pre), models_to_merge=copy.deepcopy(fts), exclude_param_names_regex=[], models_use_deepcopy=True, **kw)
        arrays['out/' + case] = flat(merged)
    np.savez_compressed(args.out, **arrays)
    print('wrote %s: %d arrays, %d bytes' % (args.out, len(arrays), os.path.getsize(args.out)))


if __name__ == '__main__':
    main()
