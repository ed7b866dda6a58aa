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
from . import eval_metrics as cli
from . import harmony, pieces

PRINT_LAGS = (1, 2, 4, 8, 16)


def get_args(argv=None):
    return cli.parser('./harmony.json', reference=False, lags=True).parse_args(argv)


def _print_set(tag, n, short, profile, means):
    print('   [harmony] %s: %d pieces of two bars or more with a pitched note (%d left out)' % (tag, n, short))
    for name in ('harmony', 'sequence'):
        print('   [harmony] %s %-8s  ' % (tag, name) + '  '.join('lag %2d %6.4f' % (l, profile[name][l - 1]) for l in PRINT_LAGS))
    items = list(means.items())
    for part in (items[:5], items[5:]):
        print('   [harmony] %s means   ' % tag + '  '.join('%s %.4f' % kv for kv in part))


def main(argv=None):
    args = get_args(argv)
    return cli.lag_family_main(args, 'harmony', harmony, harmony.compare_harmony, _print_set,
                               'the harmony columns come from a HIP kernel (pb_harmony.hip)', 'the harmony kernel',
                               lambda a, tab, skip: harmony.kept_pieces(pieces.host_ids(a, tab.layout), tab, skip).sum(),
                               'of two bars or more with a pitched note')


if __name__ == '__main__':
    main()
