"""python -m pianobart_amd.eval_texture: the texture of a generated set of pieces, alone or against a reference set
(pianobart_amd.texture).

  --generated g.npy   what eval_generation wrote: (N, S, 8), or (N, n, S, 8) with --samples n (the samples are flattened to N * n pieces)
  --reference r.npy   optional: the data to compare with, (N, S, 8)
  --skip K            the first K rows of every piece do not count (a prime of K rows)
  --max_pieces N      the first N pieces of each file only
  --grid G            points of the density grid (2 .. 4096)
  --output t.json     the result as JSON (nan is written as null)

Printed for each set: the pooled polyphony profile (the share of the steps between the first onset and the last end at which 0, 1, 2, ..
pitches sound), and the means of the scalar groups (silence, mean and largest polyphony, overlaps, collisions, duplicates, ties, ..) over
the pieces that hold a pitched note. With a reference one line per group follows, as eval_metrics prints them: the group's mean in both
sets, the intra-set and inter-set distances, KL and overlapped area."""
from . import eval_metrics as cli
from . import pieces, texture

PRINT_LEVELS = 9                                  # the profile columns printed: 0 .. 7 pitches, and all above


def get_args(argv=None):
    return cli.parser('./texture.json', reference=False).parse_args(argv)


def _print_set(tag, n, unpitched, profile, means):
    print('   [texture] %s: %d pieces with a pitched note (%d left out)' % (tag, n, unpitched))
    poly = [float('nan') if v is None else v for v in profile['polyphony']]
    shown = poly[:PRINT_LEVELS - 1] + [sum(poly[PRINT_LEVELS - 1:])]
    print('   [texture] %s polyphony  ' % tag + '  '.join('%s %6.4f' % ('%d' % c if c < PRINT_LEVELS - 1 else '>=%d' % c, v) for c, v in enumerate(shown)))
    items = list(means.items())
    for part in (items[:5], items[5:]):
        print('   [texture] %s means   ' % tag + '  '.join('%s %.4f' % kv for kv in part))


def main(argv=None):
    args = get_args(argv)
    cli.refuse_common(args, 'the texture columns come from a HIP kernel (pb_texture.hip)')
    sets = cli.load_sets(args)
    cli.refuse_long(sets, 'the texture kernel')
    tab = cli.load_tables(args.dict_file)
    if args.reference is None:
        res = texture.describe_set(sets[0][1], tab, start=args.skip)
        _print_set('generated', res['n'], res['unpitched'], res['profile'], res['means'])
    else:
        cli.need_two(sets, lambda a: texture.kept_pieces(pieces.host_ids(a, tab.layout), tab, args.skip).sum(), 'with a pitched note', args.skip)
        res = texture.compare_texture(sets[0][1], sets[1][1], tab, grid=args.grid, start=args.skip)
        for t, name in (('gen', 'generated'), ('ref', 'reference')):
            means = {k: res['groups'][k]['mean_' + t] for k in texture.SCALAR_GROUPS}
            _print_set(name, res['n_' + t], res['unpitched_' + t], res['profile_' + t], means)
        cli.print_groups('texture', res['groups'])
    cli.write_json(res, args.output)
    print('   [texture] %.2f ms on the device -> %s' % (res['device_ms']['total'], args.output))
    return res


if __name__ == '__main__':
    main()
