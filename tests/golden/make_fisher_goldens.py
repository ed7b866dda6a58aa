"""Writes tests/golden/g16_fisher.npz: the reference's own fisher_merging results on a toy classifier (run once, on the CPU).

    python tests/golden/make_fisher_goldens.py --reference <directory that holds the reference's model_merging_methods/ and utils/>

The reference's MergingMethod is imported at generation time only; no test reads the reference. The file holds arrays only, every
model as ONE flat float32 vector in the order of the sorted parameter names (the canonical layout of pianobart_amd/merge.py):
    names (str), shapes (len(names), 3) int64, unused dimensions 0      the segment table
    ft3 (3, n), ft8 (8, n)                                              the perturbed copies of the toy classifier
    F3 (3, n), F8 (8, n)                                                each model's Fisher weights: THIS script's torch restatement of the reference's
                                                                        loop on the same data (10 examples in batches of 4, num_fisher_examples 10: /12)
    norm3 (3), norm8 (8)                                                the reference's norms: torch.norm of the per-tensor torch.norms, float32
    coef (8)                                                            the coefficients of the `coef` cases (their first N)
    out/<case>/<N> (n)                                                  MergingMethod('fisher_merging').fisher_merging(...) of the case
Cases: default, plain (normalize_fisher_weight=False), coef (fisher_scaling_coefficients given), minimal (minimal_fisher_weight=1e-3).

The toy. Every tensor's size is a multiple of 64, because torch's CPU sum over the model axis is left to right only for the columns it
takes four vectors at a time; the columns behind the last whole group of 4 x 8 (or 4 x 16) go through four interleaved partial sums when
N >= 4, so their result would depend on the element's place in its tensor and on the build's vector width. Model m's data never holds
token m % 6 and no model's holds token 7: row 7 of the embedding has F = 0 in every model, row m % 6 in model m alone.
The script checks what the tests rely on: its F reproduces every recorded output bit for bit through tests/fisher_ref.py, and the
reference's norms are within 8 * 2^-24 (relative) of float32(sqrt(float64 sum))."""
import argparse
import copy
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

COEF = [0.3, 1.7, 0.9, 0.4, 1.1, 0.6, 2.0, 0.8]
N_EXAMPLES, BATCH, T = 10, 4, 6


class Toy(nn.Module):
    """1 280 parameters: rank 1 (a bias, LayerNorm), rank 2 (embedding, linears), rank 3 (a 1-D convolution); 4 classes."""

    def __init__(self):
        super().__init__()
        self.emb = nn.Embedding(8, 8)
        self.conv = nn.Conv1d(8, 8, 4, bias=False)
        self.proj = nn.Linear(8, 64)
        self.norm = nn.LayerNorm(64)
        self.head = nn.Linear(64, 4, bias=False)

    def forward(self, ids):
        h = torch.relu(self.conv(self.emb(ids).transpose(1, 2))).mean(dim=2)
        return SimpleNamespace(logits=self.head(self.norm(torch.tanh(self.proj(h)))))


def make_models(n_models, seed=16):
    g = torch.Generator().manual_seed(seed)
    base = Toy()
    with torch.no_grad():
        for p in base.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.3)
    fts = []
    for i in range(n_models):
        m = copy.deepcopy(base)
        with torch.no_grad():
            for p in m.parameters():
                p.add_(torch.randn(p.shape, generator=g) * (0.02 * (i + 1)))
        fts.append(m)
    return fts


def make_data(m, seed=160):
    """(10, T) token ids of model m's own training set: no token m % 6, no token 7."""
    g = torch.Generator().manual_seed(seed + m)
    allowed = torch.tensor([t for t in range(7) if t != m % 6])
    return allowed[torch.randint(0, len(allowed), (N_EXAMPLES, T), generator=g)]


class StubTrainer:
    """What the reference's fisher_merging asks of a trainer."""

    def __init__(self, ids):
        self.ids = ids
        self._train_batch_size = BATCH

    def get_train_dataloader(self):
        return [{'ids': self.ids[i:i + BATCH]} for i in range(0, len(self.ids), BATCH)]

    def _prepare_inputs(self, inputs):
        return inputs


def own_fisher(model, trainer, num_examples):
    """The reference's loop (merging_methods.py:201-249) in this script's words: per batch the square of the summed gradient."""
    total, computed = None, 0
    for inputs in trainer.get_train_dataloader():
        if computed >= num_examples:
            break
        logits = model(**trainer._prepare_inputs(inputs)).logits
        e = (torch.sqrt(torch.softmax(logits, dim=-1).detach()) * torch.log_softmax(logits, dim=-1)).sum(dim=-1).sum(dim=0)
        model.zero_grad()
        e.backward()
        sq = {k: p.grad.detach() ** 2 for k, p in model.named_parameters()}
        if total is None:
            total = sq
        else:
            for k in sq:
                total[k] += sq[k]
        computed += trainer._train_batch_size
    for k in total:
        total[k] /= computed
    return total, computed


def cases(n):
    yield 'default', {}
    yield 'plain', dict(normalize_fisher_weight=False)
    yield 'coef', dict(fisher_scaling_coefficients=COEF[:n])
    yield 'minimal', dict(minimal_fisher_weight=1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), 'g16_fisher.npz'))
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from model_merging_methods.merging_methods import MergingMethod
    from tests import fisher_ref as R

    torch.set_num_threads(1)
    # The reference takes torch.norm(stacked, dim=[1, .., rank]) per tensor. For the rank-3 tensor that is three dimensions, which this
    # torch's torch.norm hands to linalg.matrix_norm and refuses (the reference's own models stop at rank 2). The L2 norm over those
    # dimensions is what it means and what earlier builds computed: for more than two dimensions, and only while this script runs,
    # torch.norm goes to linalg.vector_norm. One and two dimensions take torch's own route.
    torch_norm = torch.norm

    def norm(input, p='fro', dim=None, *a, **kw):
        if p == 'fro' and isinstance(dim, (list, tuple)) and len(dim) > 2 and not a and not kw:
            return torch.linalg.vector_norm(input, 2, list(dim))
        return torch_norm(input, p, dim, *a, **kw)

    torch.norm = norm
    probe = Toy()
    names = sorted(n for n, _ in probe.named_parameters())
    shapes = {n: tuple(p.shape) for n, p in probe.named_parameters()}
    assert all(int(np.prod(s)) % 64 == 0 for s in shapes.values()), shapes
    assert {len(s) for s in shapes.values()} == {1, 2, 3}

    def flat(params):
        params = dict(params)
        return np.concatenate([params[n].detach().numpy().astype(np.float32).reshape(-1) for n in names])

    arrays = {'names': np.array(names), 'shapes': np.array([list(shapes[n]) + [0] * (3 - len(shapes[n])) for n in names], dtype=np.int64),
              'coef': np.array(COEF, dtype=np.float32)}
    eps_c = 0.0
    for N in (3, 8):
        fts = make_models(N)
        trainers = [StubTrainer(make_data(m)) for m in range(N)]
        Fs = []
        for m in range(N):
            F, computed = own_fisher(copy.deepcopy(fts[m]), trainers[m], N_EXAMPLES)
            assert computed == 12
            Fs.append(F)
        # the reference's norm (get_models_fisher_norm): per tensor over the stacked models, then over the tensors in named_parameters() order
        order = [n for n, _ in fts[0].named_parameters()]
        per = [torch.norm(torch.stack([F[k] for F in Fs], dim=0), dim=list(range(1, Fs[0][k].dim() + 1))) for k in order]
        norms = torch.norm(torch.stack(per, dim=1), dim=1).numpy().astype(np.float32)
        W, FF = np.stack([flat(f.named_parameters()) for f in fts]), np.stack([flat(F) for F in Fs])
        arrays['ft%d' % N], arrays['F%d' % N], arrays['norm%d' % N] = W, FF, norms
        own = np.sqrt((FF.astype(np.float64) ** 2).sum(axis=1)).astype(np.float32)
        eps_c = max(eps_c, float(np.max(np.abs(norms.astype(np.float64) - own) / own)))
        everywhere = (FF == 0).all(axis=0).sum()
        one = ((FF == 0).sum(axis=0) == 1).sum()
        assert everywhere >= 8 and one >= 8, (everywhere, one)
        for case, kw in cases(N):
            merged = MergingMethod(merging_method_name='fisher_merging').fisher_merging(
                models_to_merge=copy.deepcopy(fts), trainers=trainers, exclude_param_names_regex=[], nums_fisher_examples=[N_EXAMPLES] * N, **kw)
            want = flat(merged)
            arrays['out/%s/%d' % (case, N)] = want
            got = R.merge(list(W), list(FF), norms=norms, **kw)
            bad = int((got.view(np.uint32) != want.view(np.uint32)).sum())
            assert bad == 0, (case, N, bad)
            print('%-8s N=%d: the restatement equals the reference on all %d elements' % (case, N, want.size))
    assert eps_c <= 8 * 2.0 ** -24, eps_c
    print('eps_c = %.3g (= %.2f * 2^-24)' % (eps_c, eps_c * 2 ** 24))
    np.savez_compressed(args.out, **arrays)
    print('wrote %s: %d arrays, %d bytes' % (args.out, len(arrays), os.path.getsize(args.out)))


if __name__ == '__main__':
    main()
