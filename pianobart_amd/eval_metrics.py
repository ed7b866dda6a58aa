"""python -m pianobart_amd.eval_metrics: compare a generated set of pieces with a reference set (pianobart_amd.metrics).

  --generated g.npy   what eval_generation wrote: (N, S, 8), or (N, n, S, 8) with --samples n (the samples are flattened to N * n pieces)
  --reference r.npy   the data to compare with, e.g. the test split the prompts came from: (N, S, 8)
  --skip K            the first K rows of every piece do not count (a prime of K rows that both sets share)
  --max_pieces N      the first N pieces of each file only
  --grid G            points of the density grid (2 .. 4096)
  --output m.json     the result of metrics.compare_sets as JSON (nan is written as null)

One line per feature group is printed: the feature's mean in both sets, the mean intra-set and inter-set distances, the KL divergence of
the intra-reference from the inter-set distances and their overlapped area (1 = the sets are told apart by nothing this feature sees).
The reference's "FAD" lines of finetune_generation stay n/a: they need the third-party `shapesimilarity`, and this is another measure."""
import argparse
import json
import math
import os

import numpy as np

from . import metrics
from ._lib import PBError

_HERE = os.path.dirname(os.path.abspath(__file__))
_VOCAB = os.path.join(_HERE, 'data', 'octuple_vocab.json')


def get_args(argv=None):
    ap = argparse.ArgumentParser(description='')
    ap.add_argument('--generated', type=str, required=True)
    ap.add_argument('--reference', type=str, required=True)
    ap.add_argument('--dict_file', type=str, default=_VOCAB)
    ap.add_argument('--grid', type=int, default=1024)
    ap.add_argument('--skip', type=int, default=0, metavar='K')
    ap.add_argument('--max_pieces', type=int, default=None, metavar='N')
    ap.add_argument('--output', type=str, default='./metrics.json')
    ap.add_argument('--cpu', action='store_true')
    return ap.parse_args(argv)


def load_pieces(path, what, max_pieces=None):
    """An (N, S, 8) array from a .npy file of (N, S, 8) or (N, n, S, 8); PBError for a missing file or another shape."""
    if not os.path.isfile(path):
        raise PBError('%s: no file %r' % (what, path))
    a = np.load(path, allow_pickle=False)
    if a.ndim not in (3, 4) or a.shape[-1] != 8 or a.shape[-2] < 1:
        raise PBError('%s %r holds an array of shape %s; pieces are (N, S, 8) or (N, n, S, 8): rows of 8 ids' % (what, path, a.shape))
    a = a.reshape(-1, a.shape[-2], 8)
    return a if max_pieces is None else a[:max_pieces]


def _json_safe(v):
    if isinstance(v, dict):
        return {k: _json_safe(x) for k, x in v.items()}
    if isinstance(v, float) and not math.isfinite(v):
        return None
    return v


def main(argv=None):
    args = get_args(argv)
    if args.cpu:
        raise PBError('--cpu: the set metrics run in HIP kernels (pb_metrics.hip); there is no CPU path')
    if args.skip < 0 or (args.max_pieces is not None and args.max_pieces < 1):
        raise PBError('--skip takes a number of rows >= 0 and --max_pieces a number of pieces >= 1')
    if not 2 <= args.grid <= 4096:
        raise PBError('--grid takes 2 .. 4096 points (got %d)' % args.grid)
    gen = load_pieces(args.generated, '--generated', args.max_pieces)
    ref = load_pieces(args.reference, '--reference', args.max_pieces)
    from .pretrain import _load_vocab
    if not os.path.isfile(args.dict_file):
        raise PBError('--dict_file: no file %r' % args.dict_file)
    tab = metrics.tables(_load_vocab(args.dict_file)[0])
    for what, a in (('--generated', gen), ('--reference', ref)):
        n = int((metrics.piece_lengths(a, tab.layout, args.skip) > 0).sum())
        if n < 2:
            raise PBError('%s holds %d pieces with a note behind row %d; a set needs at least 2 (its intra-set distances)' % (what, n, args.skip))
    res = metrics.compare_sets(gen, ref, tab, grid=args.grid, start=args.skip)
    with open(args.output, 'w') as f:
        json.dump(_json_safe(res), f, indent=1)
    print('   [metrics] %d generated (%d empty), %d reference (%d empty) pieces; %.2f ms on the device'
          % (res['n_gen'], res['empty_gen'], res['n_ref'], res['empty_ref'], res['device_ms']['total']))
    for name, g in res['groups'].items():
        print('   [metrics] %-17s gen %10.4f  ref %10.4f | dist gen %9.4f ref %9.4f inter %9.4f | KL %8.4f  OA %6.4f'
              % (name, g['mean_gen'], g['mean_ref'], g['dist_gen'], g['dist_ref'], g['dist_inter'], g['kl'], g['oa']))
    print('   [metrics] -> %s' % args.output)
    return res


if __name__ == '__main__':
    main()
