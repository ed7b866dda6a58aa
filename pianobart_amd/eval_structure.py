"""python -m pianobart_amd.eval_structure: the repetition structure of a generated set of pieces, alone or against a reference set
(pianobart_amd.structure).

  --generated g.npy   what eval_generation wrote: (N, S, 8), or (N, n, S, 8) with --samples n (the samples are flattened to N * n pieces)
  --reference r.npy   optional: the data to compare with, (N, S, 8)
  --skip K            the first K rows of every piece do not count (a prime of K rows)
  --max_pieces N      the first N pieces of each file only
  --lags L            the lags 1 .. L that the per-piece groups cover (1 .. 64)
  --pitch_class       a note is (position, pitch class) instead of (position, pitch); percussion stays itself
  --grid G            points of the density grid (2 .. 4096)
  --output s.json     the result as JSON (nan is written as null)

Printed for each set: the pooled groove (onsets) and repetition (onsets and pitches) similarity of bars 1, 2, 4, 8 and 16 apart, and the
means of groove_mean, repeat_mean and repeat_period over the pieces of at least two bars. With a reference one line per group follows, as
eval_metrics prints them: the group's mean in both sets, the intra-set and inter-set distances, KL and overlapped area."""
from . import eval_metrics as cli
from . import structure

PRINT_LAGS = (1, 2, 4, 8, 16)


def get_args(argv=None):
    ap = cli.parser('./structure.json', reference=False, lags=True)
    ap.add_argument('--pitch_class', action='store_true')
    return ap.parse_args(argv)


def _print_set(tag, n, short, profile, means=None):
    print('   [structure] %s: %d pieces of two bars or more (%d shorter)' % (tag, n, short))
    for name in ('groove', 'repeat'):
        print('   [structure] %s %-6s  ' % (tag, name) + '  '.join('lag %2d %6.4f' % (l, profile[name][l - 1]) for l in PRINT_LAGS))
    if means is not None:
        print('   [structure] %s means   ' % tag + '  '.join('%s %.4f' % kv for kv in means.items()))


def main(argv=None):
    args = get_args(argv)
    return cli.lag_family_main(args, 'structure', structure, structure.compare_structure, _print_set,
                               'the lag sums run in a HIP kernel (pb_structure.hip)', 'the structure kernel',
                               lambda a, tab, skip: (structure.bar_spans(a, tab.layout, skip) >= 2).sum(), 'of two bars or more',
                               pitch_class=args.pitch_class)


if __name__ == '__main__':
    main()
