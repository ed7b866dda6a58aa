"""Writes tests/golden/g17_regmean.npz: the reference's own regmean_merging results on a toy classifier (run once, on the CPU).

    python tests/golden/make_regmean_goldens.py --reference <directory that holds the reference's model_merging_methods/ and utils/>

The reference's MergingMethod is imported at generation time only; no test reads the reference. The file holds arrays only, every
model as ONE flat float32 vector in the order of the sorted parameter names (the canonical layout of pianobart_amd/merge.py):
    names (str), shapes (len(names), 2) int64, unused dimensions 0      the segment table
    pre (n), ft (3, n)                                                  the base and its three perturbed copies; the N = 2 cases take the first two
    modules (str), gram_of (str)                                        the Linear modules, and the module whose matrix each one's is (k reads q's
                                                                        input: the two matrices came out equal bit for bit and are stored once)
    G/<m>/<module> (K, K)                                               model m's Gram matrix of the module's inputs: THIS script's forward hooks, the
                                                                        reference's running-average expression in the reference's order
    symmetric (len(modules)) bool                                       whether the module's matrix is exactly symmetric in every model
    rows (3, len(modules)), examples (3)                                the rows each hook counted, the examples each model used
    num_examples (3), batch, T                                          nums_regmean_examples, the loader's batch size, the sequence length
    ids/<m> (examples available, T)                                     model m's token data: more than it uses where the stop rule bites
    ratios (4), ratio_names (str), exclude (str)                        the ratios of the cases in the order of ratio_names; the exclude pattern
    act_model, act3_module, act2_module, act_batches                    which model and modules the activations are of; the sizes of its batches
    act3 (rows, K), act2 (examples, K)                                  what the two hooks saw, batch after batch (act3: x.reshape(-1, K))
    out/<case>/<N> (n, or fewer with the exclusion)                     MergingMethod('regmean_merging').regmean_merging(...) of the case, flat over
                                                                        the names it returned, sorted
Cases: r1 (reduce_non_diagonal_ratio 1.0), r09 (0.9), r03 (0.3: float32(0.3) is not the double 0.3, see below), r0 (0.0: a diagonal
system), r09x (0.9 with exclude_param_names_regex = ['q\\..*']: q.weight and q.bias are absent from the output, k -- same input -- stays solved).

A ratio whose float32 (1 - r) + r is not 1 was looked for and does not exist in [0, 1]: for r >= 0.5 the difference 1 - r is exact, so the
sum is exactly 1; for r < 0.5 the difference lies in [0.5, 1], where float32 numbers are 2^-24 apart, so it is off by at most 2^-25, the exact
sum is within 2^-25 of 1, and both neighbours of 1 are further away or lose the tie to 1 (even). The script checks 10^5 + 10^5 ratios and
asserts that it finds none; the diagonal factor is 1 in every case and the off-diagonal one is float32(r).

The toy: an embedding (16, 12); q (12 -> 64) and k (12 -> 64, no bias) both read the embedded tokens (B, T, 12): K = 12 is no multiple of 8;
a LayerNorm(64); mid (64 -> 16, no bias) reads (B, T, 64): K = 64, one 64-column block of pb_chol_factor; wide (80 -> 8, no bias) reads
(B, T, 80): K = 80, a whole block and a part of one; head (16 -> 64) reads the mean over T, (B, 16): its hook counts one row per example.
Every tensor's size is a multiple of 64, for the reason make_fisher_goldens.py gives: torch's CPU mean over the model axis is order-dependent
elsewhere, and the averaged parameters are compared bit for bit. Batches of 8; the models hold 70 / 86 / 78 examples and are asked for
67 / 67 / 75: model 0 takes eight batches (64 < 67) and one more, the short one of 6 (70); model 1 stops after nine (72) and leaves 14
unread; model 2 takes nine (72 < 75) and the short one (78). A running average therefore mixes batches of 8 T and 6 T rows.

CONDITIONS on the toy, asserted here (they are what makes the tests' yardstick meaningful, not measurements):
  * for every solved layer, case and N the 2-norm condition number of the summed, scaled Gram matrix in float64 is at most 1e4 (head, the
    2-D-input layer with K = 16, gets 70 or more rows per model: over 4 K), so the reference's float32 inverse is a sound one and its
    error the rounding of float32, not the garbage an (almost) singular sum gives;
  * every summed Gram matrix is positive definite in float64 (a float64 Cholesky factorisation succeeds);
  * the file stays below 512 KiB.
The script also asserts that its restatement (these Gram matrices through tests/regmean_ref.merge32_recipe, torch's mean over the stacked
models for everything else) equals the reference's returned dict bit for bit for every case and parameter, that an excluded name is
absent from it, and it reports whether the Gram matrices are exactly symmetric. Two runs write the same bytes."""
import argparse
import copy
import io
import os
import sys
import zipfile
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

BATCH, T, VOCAB = 8, 5, 16
AVAILABLE, ASKED = (70, 86, 78), (67, 67, 75)
EXCLUDE = r'q\..*'
ACT_MODEL, ACT3, ACT2 = 0, 'mid', 'head'
COND_MAX = 1e4


class Toy(nn.Module):
    """4 672 parameters; Linear inputs of rank 3 (q, k, mid, wide) and rank 2 (head)."""

    def __init__(self):
        super().__init__()
        self.emb = nn.Embedding(VOCAB, 12)
        self.q = nn.Linear(12, 64)
        self.k = nn.Linear(12, 64, bias=False)
        self.norm = nn.LayerNorm(64)
        self.mid = nn.Linear(64, 16, bias=False)
        self.wide = nn.Linear(80, 8, bias=False)
        self.head = nn.Linear(16, 64)

    def forward(self, ids):
        e = self.emb(ids)
        h = self.norm(torch.sin(4.0 * (self.q(e) + self.k(e).cumsum(dim=1))))
        c = self.mid(h)
        g = self.wide(torch.cat([h, torch.cos(2.0 * c)], dim=-1))
        p = torch.cat([torch.tanh(c[..., :8]) * g, c[..., 8:] + g], dim=-1).mean(dim=1)
        return SimpleNamespace(logits=self.head(p))


def make_models(seed=17):
    g = torch.Generator().manual_seed(seed)
    base = Toy()
    with torch.no_grad():
        for name, p in base.named_parameters():
            p.copy_(torch.randn(p.shape, generator=g) * {'emb': 1.0, 'norm': 0.1}.get(name.split('.')[0], 0.3) + (1.0 if name == 'norm.weight' else 0.0))
    fts = []
    for i in range(3):
        m = copy.deepcopy(base)
        with torch.no_grad():
            for p in m.parameters():
                p.add_(torch.randn(p.shape, generator=g) * (0.02 * (i + 1)))
        fts.append(m)
    return base, fts


def make_data(m, seed=170):
    g = torch.Generator().manual_seed(seed + m)
    return torch.randint(0, VOCAB, (AVAILABLE[m], T), generator=g)


class StubTrainer:
    """What the reference's regmean_merging asks of a trainer."""

    def __init__(self, ids):
        self.ids = ids
        self._train_batch_size = BATCH

    def get_train_dataloader(self):
        return [{'ids': self.ids[i:i + BATCH]} for i in range(0, len(self.ids), BATCH)]

    def _prepare_inputs(self, inputs):
        return inputs


def own_grams(model, trainer, num_examples, keep=()):
    """The reference's pass (merging_methods.py:276-299, 383-411) in this script's words: a forward hook on every nn.Linear keeps the running
    average (G n + X^T X) / (n + rows) over x.reshape(-1, K); the loop ends before a batch once the examples the FIRST hook counted reach
    num_examples. ({module: G}, {module: rows}, examples, {module in keep: [x of every batch]})."""
    G, rows, examples, seen, handles = {}, {}, {}, {k: [] for k in keep}, []

    def hook(name):
        def fn(module, inputs, output):
            x = inputs[0].detach()
            b = x.shape[0]
            x = x.reshape(-1, x.shape[-1])
            if name in seen:
                seen[name].append(x.clone())
            xtx = torch.matmul(x.transpose(0, 1), x)
            if name not in G:
                G[name] = xtx / x.shape[0]
                rows[name] = x.shape[0]
                examples[name] = b
            else:
                G[name] = (G[name] * rows[name] + xtx) / (rows[name] + x.shape[0])
                rows[name] += x.shape[0]
                examples[name] += b
        return fn

    for name, mod in model.named_modules():
        if isinstance(mod, nn.Linear):
            handles.append(mod.register_forward_hook(hook(name)))
    with torch.no_grad():
        for inputs in trainer.get_train_dataloader():
            if examples and list(examples.values())[0] >= num_examples:
                break
            model(**trainer._prepare_inputs(inputs))
    for h in handles:
        h.remove()
    assert len(set(examples.values())) == 1
    return G, rows, list(examples.values())[0], seen


def write_npz(path, arrays):
    """np.savez_compressed with a fixed timestamp on every member: two runs give the same bytes."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), 'g17_regmean.npz'))
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from model_merging_methods.merging_methods import MergingMethod
    from tests import regmean_ref as R

    torch.set_num_threads(1)
    base, fts = make_models()
    names = sorted(n for n, _ in base.named_parameters())
    shapes = {n: tuple(p.shape) for n, p in base.named_parameters()}
    assert all(int(np.prod(s)) % 64 == 0 for s in shapes.values()), shapes
    modules = sorted(n for n, m in base.named_modules() if isinstance(m, nn.Linear))
    K_of = {n: dict(base.named_modules())[n].in_features for n in modules}
    assert sorted(set(K_of.values())) == [12, 16, 64, 80]

    def flat(params, keys):
        params = dict(params)
        return np.concatenate([params[n].detach().contiguous().numpy().astype(np.float32).reshape(-1) for n in keys])

    tried = np.concatenate([np.arange(100001, dtype=np.float64) / 1e5, np.random.RandomState(17).rand(100000) ** 4]).astype(np.float32)
    odd = tried[(np.float32(1.0) - tried) + tried != np.float32(1.0)]
    assert tried.dtype == np.float32 and odd.size == 0, odd[:4]
    print('no ratio among %d has a float32 (1 - r) + r other than 1' % tried.size)
    ratio_of = {'r1': 1.0, 'r09': 0.9, 'r03': 0.3, 'r0': 0.0}
    assert all(R.factors(r)[1] == np.float32(1.0) for r in ratio_of.values())
    trainers = [StubTrainer(make_data(m)) for m in range(3)]
    Gs, rows, examples = [], [], []
    for m in range(3):
        G, r, ex, seen = own_grams(copy.deepcopy(fts[m]), trainers[m], ASKED[m], (ACT3, ACT2) if m == ACT_MODEL else ())
        stop = next(t for t in [min(i + BATCH, AVAILABLE[m]) for i in range(0, AVAILABLE[m], BATCH)] if t >= ASKED[m])
        assert ex == stop and ASKED[m] % BATCH != 0, (m, ex, stop)
        assert all(r[n] == ex * (1 if n == 'head' else T) for n in modules), r
        assert r['head'] >= 4 * K_of['head']
        assert torch.equal(G['q'], G['k'])
        Gs.append(G), rows.append(r), examples.append(ex)
        if m == ACT_MODEL:
            acts = seen
    assert examples == [70, 72, 78] and [e % BATCH for e in examples] == [6, 0, 6], examples
    sym = {n: all(torch.equal(G[n], G[n].t()) for G in Gs) for n in modules}
    print('Gram matrices exactly symmetric: %s' % ', '.join('%s %s' % (n, 'yes' if s else 'NO') for n, s in sym.items()))
    gram_of = ['q' if n == 'k' else n for n in modules]
    arrays = {'names': np.array(names), 'shapes': np.array([list(shapes[n]) + [0] * (2 - len(shapes[n])) for n in names], dtype=np.int64),
              'pre': flat(base.named_parameters(), names), 'ft': np.stack([flat(f.named_parameters(), names) for f in fts]),
              'modules': np.array(modules), 'gram_of': np.array(gram_of), 'rows': np.array([[r[n] for n in modules] for r in rows], dtype=np.int64),
              'examples': np.array(examples, dtype=np.int64), 'num_examples': np.array(ASKED, dtype=np.int64), 'batch': np.array(BATCH, dtype=np.int64),
              'T': np.array(T, dtype=np.int64), 'ratios': np.array([ratio_of[c] for c in ('r1', 'r09', 'r03', 'r0')], dtype=np.float64),
              'ratio_names': np.array(['r1', 'r09', 'r03', 'r0']), 'exclude': np.array(EXCLUDE), 'act_model': np.array(ACT_MODEL, dtype=np.int64),
              'act3_module': np.array(ACT3), 'act2_module': np.array(ACT2),
              'act_batches': np.array([x.shape[0] for x in acts[ACT2]], dtype=np.int64),
              'act3': torch.cat(acts[ACT3]).numpy(), 'act2': torch.cat(acts[ACT2]).numpy()}
    assert arrays['act3'].shape == (examples[ACT_MODEL] * T, K_of[ACT3]) and arrays['act2'].shape == (examples[ACT_MODEL], K_of[ACT2])
    for m in range(3):
        arrays['ids/%d' % m] = trainers[m].ids.numpy().astype(np.int64)
        for n in modules:
            if n != 'k':
                arrays['G/%d/%s' % (m, n)] = Gs[m][n].numpy()
    worst_cond, conds = 0.0, {}
    for N in (2, 3):
        for case, ratio, exclude in [(c, r, []) for c, r in ratio_of.items()] + [('r09x', 0.9, [EXCLUDE])]:
            merged = MergingMethod(merging_method_name='regmean_merging').regmean_merging(
                models_to_merge=copy.deepcopy(fts[:N]), trainers=trainers[:N], exclude_param_names_regex=exclude, nums_regmean_examples=list(ASKED[:N]),
                reduce_non_diagonal_ratio=ratio)
            kept = [n for n in names if not (exclude and n.startswith('q.'))]
            assert sorted(merged) == kept, (sorted(merged), kept)
            if exclude:
                assert 'q.weight' not in merged and 'q.bias' not in merged and 'k.weight' in merged
            own = {}
            for n in kept:
                Ws = [dict(f.named_parameters())[n].detach() for f in fts[:N]]
                mod = n[:-len('.weight')] if n.endswith('.weight') else None
                if mod in modules:
                    G_list = [G[mod] for G in Gs[:N]]
                    own[n] = R.merge32_recipe(Ws, G_list, ratio)
                    S = sum(R.scale64(G, ratio) for G in G_list)
                    cond = float(torch.linalg.cond(S, 2))
                    torch.linalg.cholesky(S)                                    # raises unless positive definite
                    worst_cond = max(worst_cond, cond)
                    assert cond <= COND_MAX, (case, N, n, cond)
                    conds[K_of[mod]] = max(conds.get(K_of[mod], 0.0), cond)
                else:
                    own[n] = torch.stack(Ws, dim=0).mean(dim=0)
            want, got = flat(merged, kept), flat(own, kept)
            bad = int((got.view(np.uint32) != want.view(np.uint32)).sum())
            assert bad == 0 and np.isfinite(want).all(), (case, N, bad)
            arrays['out/%s/%d' % (case, N)] = want
            print('%-5s N=%d: the restatement equals the reference on all %d elements' % (case, N, want.size))
    print('largest condition number of a summed, scaled Gram matrix: %.4g (at most %g); per K: %s' % (worst_cond, COND_MAX, ', '.join('%d: %.4g' % kv for kv in sorted(conds.items()))))
    arrays['symmetric'] = np.array([sym[n] for n in modules])
    write_npz(args.out, arrays)
    size = os.path.getsize(args.out)
    assert size < 512 * 1024, size
    print('wrote %s: %d arrays, %d bytes' % (args.out, len(arrays), size))


if __name__ == '__main__':
    main()
