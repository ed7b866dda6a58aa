"""python -m pianobart_amd.eval_harmony: the harmony of a generated set of pieces, alone or against a reference set
(pianobart_amd.harmony).

  --generated g.npy   what eval_generation wrote: (N, S, 8), or (N, n, S, 8) with --samples n (the samples are flattened to N * n pieces)
  --reference r.npy   optional: the data to compare with, (N, S, 8)
  --skip K            the first K rows of every piece do not count (a prime of K rows)
  --max_pieces N      the first N pieces of each file only
  --lags L            the lags 1 .. L that the per-piece groups cover (1 .. 64)
  --grid G            points of the density grid (2 .. 4096)
  --output h.json     the result as JSON (nan is written as null)

Printed for each set: the pooled harmonic repetition (D_H) and sequence (D_X, up to transposition) similarity of bars 1, 2, 4, 8 and 16
apart, and the means of the scalar groups (entropies, scale consistency, key stability, ..) over the pieces of at least two bars that hold
a pitched note. With a reference one line per group follows, as eval_metrics prints them: the group's mean in both sets, the intra-set and
inter-set distances, KL and overlapped area."""
import argparse
import json
import os

from . import harmony, metrics, ops
from ._lib import PBError
from .eval_metrics import _json_safe, load_pieces

_HERE = os.path.dirname(os.path.abspath(__file__))
_VOCAB = os.path.join(_HERE, 'data', 'octuple_vocab.json')
PRINT_LAGS = (1, 2, 4, 8, 16)


def get_args(argv=None):
    ap = argparse.ArgumentParser(description='')
    ap.add_argument('--generated', type=str, required=True)
    ap.add_argument('--reference', type=str, default=None)
    ap.add_argument('--dict_file', type=str, default=_VOCAB)
    ap.add_argument('--lags', type=int, default=16)
    ap.add_argument('--grid', type=int, default=1024)
    ap.add_argument('--skip', type=int, default=0, metavar='K')
    ap.add_argument('--max_pieces', type=int, default=None, metavar='N')
    ap.add_argument('--output', type=str, default='./harmony.json')
    ap.add_argument('--cpu', action='store_true')
    return ap.parse_args(argv)


def _safe(v):
    """_json_safe, through lists too (the pooled profiles)."""
    if isinstance(v, dict):
        return {k: _safe(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_safe(x) for x in v]
    return _json_safe(v)


def _print_set(tag, n, short, profile, means):
    print('   [harmony] %s: %d pieces of two bars or more with a pitched note (%d left out)' % (tag, n, short))
    for name in ('harmony', 'sequence'):
        print('   [harmony] %s %-8s  ' % (tag, name) + '  '.join('lag %2d %6.4f' % (l, profile[name][l - 1]) for l in PRINT_LAGS))
    items = list(means.items())
    for part in (items[:5], items[5:]):
        print('   [harmony] %s means   ' % tag + '  '.join('%s %.4f' % kv for kv in part))


def main(argv=None):
    args = get_args(argv)
    if args.cpu:
        raise PBError('--cpu: the harmony columns come from a HIP kernel (pb_harmony.hip); there is no CPU path')
    if args.skip < 0 or (args.max_pieces is not None and args.max_pieces < 1):
        raise PBError('--skip takes a number of rows >= 0 and --max_pieces a number of pieces >= 1')
    if not 1 <= args.lags <= harmony.LAGS:
        raise PBError('--lags takes 1 .. %d (got %d)' % (harmony.LAGS, args.lags))
    if not 2 <= args.grid <= 4096:
        raise PBError('--grid takes 2 .. 4096 points (got %d)' % args.grid)
    sets = [('--generated', load_pieces(args.generated, '--generated', args.max_pieces))]
    if args.reference is not None:
        sets.append(('--reference', load_pieces(args.reference, '--reference', args.max_pieces)))
    for what, a in sets:
        if a.shape[1] > ops.RUNS_MAX_S:
            raise PBError('%s holds pieces of %d rows; the harmony kernel takes at most %d' % (what, a.shape[1], ops.RUNS_MAX_S))
    from .pretrain import _load_vocab
    if not os.path.isfile(args.dict_file):
        raise PBError('--dict_file: no file %r' % args.dict_file)
    tab = metrics.tables(_load_vocab(args.dict_file)[0])
    if args.reference is not None:
        for what, a in sets:
            n = int(harmony.kept_pieces(metrics._host_ids(a, tab.layout), tab, args.skip).sum())
            if n < 2:
                raise PBError('%s holds %d pieces of two bars or more with a pitched note behind row %d; a set needs at least 2 (its intra-set '
                              'distances)' % (what, n, args.skip))
    kw = dict(lags=args.lags, start=args.skip)
    if args.reference is None:
        res = harmony.describe_set(sets[0][1], tab, **kw)
        _print_set('generated', res['n'], res['short'], res['profile'], res['means'])
    else:
        res = harmony.compare_harmony(sets[0][1], sets[1][1], tab, grid=args.grid, **kw)
        for tag in ('gen', 'ref'):
            means = {k: res['groups'][k]['mean_' + tag] for k in harmony.SCALAR_GROUPS}
            _print_set('generated' if tag == 'gen' else 'reference', res['n_' + tag], res['short_' + tag], res['profile_' + tag], means)
        for name, g in res['groups'].items():
            print('   [harmony] %-17s gen %10.4f  ref %10.4f | dist gen %9.4f ref %9.4f inter %9.4f | KL %8.4f  OA %6.4f'
                  % (name, g['mean_gen'], g['mean_ref'], g['dist_gen'], g['dist_ref'], g['dist_inter'], g['kl'], g['oa']))
    with open(args.output, 'w') as f:
        json.dump(_safe(res), f, indent=1)
    print('   [harmony] %.2f ms on the device -> %s' % (res['device_ms']['total'], args.output))
    return res


if __name__ == '__main__':
    main()
