"""python -m pianobart_amd.eval_metrics: compare a generated set of pieces with a reference set (pianobart_amd.metrics).

  --generated g.npy   what eval_generation wrote: (N, S, 8), or (N, n, S, 8) with --samples n (the samples are flattened to N * n pieces)
  --reference r.npy   the data to compare with, e.g. the test split the prompts came from: (N, S, 8)
  --skip K            the first K rows of every piece do not count (a prime of K rows that both sets share)
  --max_pieces N      the first N pieces of each file only
  --grid G            points of the density grid (2 .. 4096)
  --output m.json     the result of metrics.compare_sets as JSON (nan is written as null)

One line per feature group is printed: the feature's mean in both sets, the mean intra-set and inter-set distances, the KL divergence of
the intra-reference from the inter-set distances and their overlapped area (1 = the sets are told apart by nothing this feature sees).
The reference's "FAD" lines of finetune_generation stay n/a: they need the third-party `shapesimilarity`, and this is another measure.

This module also holds what the five eval_* tools (metrics, novelty, structure, harmony, texture) share: their common arguments and refusals, the
loading of pieces, the checks on a loaded set, the line of a compared group and the JSON writer."""
import argparse
import json
import math
import os

import numpy as np

from . import metrics, ops, pieces
from ._lib import PBError


# ---- shared by the eval_* tools -----------------------------------------------------------------------------------------------------------
def parser(output, reference=None, lags=False):
    """The arguments every eval_* tool takes. reference: None (the tool compares no sets), else whether --reference is required; with it
    comes --grid. lags: add --lags."""
    ap = argparse.ArgumentParser(description='')
    ap.add_argument('--generated', type=str, required=True)
    ap.add_argument('--dict_file', type=str, default=pieces.VOCAB)
    ap.add_argument('--skip', type=int, default=0, metavar='K')
    ap.add_argument('--max_pieces', type=int, default=None, metavar='N')
    ap.add_argument('--output', type=str, default=output)
    ap.add_argument('--cpu', action='store_true')
    if reference is not None:
        ap.add_argument('--reference', type=str, required=reference, default=None)
        ap.add_argument('--grid', type=int, default=1024)
    if lags:
        ap.add_argument('--lags', type=int, default=16)
    return ap


def refuse_common(args, what_runs, max_lags=None):
    """The refusals of the common arguments: --cpu first (what_runs: '<what> run in HIP kernels (<file>)'), then the ranges."""
    if args.cpu:
        raise PBError('--cpu: %s; there is no CPU path' % what_runs)
    if args.skip < 0 or (args.max_pieces is not None and args.max_pieces < 1):
        raise PBError('--skip takes a number of rows >= 0 and --max_pieces a number of pieces >= 1')
    if max_lags is not None and not 1 <= args.lags <= max_lags:
        raise PBError('--lags takes 1 .. %d (got %d)' % (max_lags, args.lags))
    if hasattr(args, 'grid') and not 2 <= args.grid <= 4096:
        raise PBError('--grid takes 2 .. 4096 points (got %d)' % args.grid)


def load_pieces(path, what, max_pieces=None):
    """An (N, S, 8) array from a .npy file of (N, S, 8) or (N, n, S, 8); PBError for a missing file or another shape."""
    if not os.path.isfile(path):
        raise PBError('%s: no file %r' % (what, path))
    a = np.load(path, allow_pickle=False)
    if a.ndim not in (3, 4) or a.shape[-1] != 8 or a.shape[-2] < 1:
        raise PBError('%s %r holds an array of shape %s; pieces are (N, S, 8) or (N, n, S, 8): rows of 8 ids' % (what, path, a.shape))
    a = a.reshape(-1, a.shape[-2], 8)
    return a if max_pieces is None else a[:max_pieces]


def load_sets(args, second='reference'):
    """[(flag, pieces)] of --generated and, when given, of the tool's second file (--reference or --corpus)."""
    sets = [('--generated', load_pieces(args.generated, '--generated', args.max_pieces))]
    if getattr(args, second) is not None:
        sets.append(('--' + second, load_pieces(getattr(args, second), '--' + second, args.max_pieces)))
    return sets


def load_tables(dict_file):
    """pieces.tables of the --dict_file; PBError for a missing one."""
    from .pretrain import _load_vocab
    if not os.path.isfile(dict_file):
        raise PBError('--dict_file: no file %r' % dict_file)
    return pieces.tables(_load_vocab(dict_file)[0])


def refuse_long(sets, what):
    """The kernels that keep a piece in LDS take ops.RUNS_MAX_S rows; what: who takes them, for the message."""
    for flag, a in sets:
        if a.shape[1] > ops.RUNS_MAX_S:
            raise PBError('%s holds pieces of %d rows; %s takes at most %d' % (flag, a.shape[1], what, ops.RUNS_MAX_S))


def need_two(sets, count, phrase, skip):
    """A compared set needs two pieces that count, for its intra-set distances. count(pieces) -> how many do; phrase: which those are."""
    for flag, a in sets:
        n = int(count(a))
        if n < 2:
            raise PBError('%s holds %d pieces %s behind row %d; a set needs at least 2 (its intra-set distances)' % (flag, n, phrase, skip))


def print_groups(tag, groups):
    for name, g in groups.items():
        print('   [%s] %-17s gen %10.4f  ref %10.4f | dist gen %9.4f ref %9.4f inter %9.4f | KL %8.4f  OA %6.4f'
              % (tag, name, g['mean_gen'], g['mean_ref'], g['dist_gen'], g['dist_ref'], g['dist_inter'], g['kl'], g['oa']))


def json_safe(v):
    """v as json.dump takes it: arrays as lists, tuples as lists, a float that is not finite as None (null)."""
    if isinstance(v, dict):
        return {k: json_safe(x) for k, x in v.items()}
    if isinstance(v, np.ndarray):
        return json_safe(v.tolist())
    if isinstance(v, (list, tuple)):
        return [json_safe(x) for x in v]
    if isinstance(v, float) and not math.isfinite(v):
        return None
    return v


def write_json(res, path):
    with open(path, 'w') as f:
        json.dump(json_safe(res), f, indent=1)


def lag_family_main(args, tag, family, compare, print_set, what_runs, what_takes, count, phrase, **kw):
    """main() of eval_structure and eval_harmony behind get_args: one set alone (family.describe_set) or against --reference (compare).
    print_set(name, n, short, profile, means) prints a set; count(pieces, tables, skip) and phrase: see need_two; kw: the family's own
    arguments of both calls."""
    refuse_common(args, what_runs, family.LAGS)
    sets = load_sets(args)
    refuse_long(sets, what_takes)
    tab = load_tables(args.dict_file)
    kw.update(lags=args.lags, start=args.skip)
    if args.reference is None:
        res = family.describe_set(sets[0][1], tab, **kw)
        print_set('generated', res['n'], res['short'], res['profile'], res['means'])
    else:
        need_two(sets, lambda a: count(a, tab, args.skip), phrase, args.skip)
        res = compare(sets[0][1], sets[1][1], tab, grid=args.grid, **kw)
        for t, name in (('gen', 'generated'), ('ref', 'reference')):
            means = {k: res['groups'][k]['mean_' + t] for k in family.SCALAR_GROUPS}
            print_set(name, res['n_' + t], res['short_' + t], res['profile_' + t], means)
        print_groups(tag, res['groups'])
    write_json(res, args.output)
    print('   [%s] %.2f ms on the device -> %s' % (tag, res['device_ms']['total'], args.output))
    return res


# ---- the tool ---------------------------------------------------------------------------------------------------------------------------
def get_args(argv=None):
    return parser('./metrics.json', reference=True).parse_args(argv)


def main(argv=None):
    args = get_args(argv)
    refuse_common(args, 'the set metrics run in HIP kernels (pb_metrics.hip)')
    sets = load_sets(args)
    tab = load_tables(args.dict_file)
    need_two(sets, lambda a: (metrics.piece_lengths(a, tab.layout, args.skip) > 0).sum(), 'with a note', args.skip)
    res = metrics.compare_sets(sets[0][1], sets[1][1], tab, grid=args.grid, start=args.skip)
    write_json(res, args.output)
    print('   [metrics] %d generated (%d empty), %d reference (%d empty) pieces; %.2f ms on the device'
          % (res['n_gen'], res['empty_gen'], res['n_ref'], res['empty_ref'], res['device_ms']['total']))
    print_groups('metrics', res['groups'])
    print('   [metrics] -> %s' % args.output)
    return res


if __name__ == '__main__':
    main()
