"""python -m pianobart_amd.eval_novelty: did the generator copy its training data? (pianobart_amd.novelty)

  --generated g.npy   what eval_generation wrote: (N, S, 8), or (N, n, S, 8) with --samples n (the samples are flattened to N * n pieces)
  --corpus train.npy  the pieces to look the generated ones up in, e.g. the training split: (M, S', 8), whole pieces
  --self              no corpus: compare --generated with itself, a piece never with itself (the diversity of one set; duplicates in a corpus)
  --skip K            the first K rows of every GENERATED piece do not count (a prime of K rows taken from the data is a copy by construction)
  --min_run R         a shared run counts towards coverage from R keys on (R + 1 notes; default 8)
  --transpose         interval keys: a copy moved to another key is still found
  --align             also align the keys locally (Smith-Waterman, linear gaps): a copy with edits is found whole
  --align_scores M,X,G  the reward of a match and the penalties of a mismatch and of a gap, positive numbers (default 1,2,2; M 1 .. 8,
                      X and G 1 .. 16); implies --align
  --min_score H       an aligned region counts towards align_coverage from score H on (default 8); implies --align
  --max_pieces N      the first N pieces of each file only
  --output n.json     the result of novelty.compare_to_corpus as JSON (nan is written as null)

A key holds a note's pitch (or interval), its position in the bar and the bar step from the note before: the identity tested is "the
same pitches at the same places in the bar". Instrument, duration, velocity, time signature and tempo are not compared."""
import numpy as np

from . import eval_metrics as cli
from . import novelty, ops
from ._lib import PBError


def get_args(argv=None):
    ap = cli.parser('./novelty.json')
    ap.add_argument('--corpus', type=str, default=None)
    ap.add_argument('--self', dest='self_', action='store_true')
    ap.add_argument('--min_run', type=int, default=8, metavar='R')
    ap.add_argument('--transpose', action='store_true')
    ap.add_argument('--align', action='store_true')
    ap.add_argument('--align_scores', type=str, default=None, metavar='M,X,G')
    ap.add_argument('--min_score', type=int, default=None, metavar='H')
    return ap.parse_args(argv)


def _align_arg(args):
    """None without the alignment flags, else the dict compare_to_corpus takes; values out of range are refused here."""
    if not (args.align or args.align_scores is not None or args.min_score is not None):
        return None
    par = dict(novelty.ALIGN_DEFAULTS)
    if args.align_scores is not None:
        try:
            vals = [int(v) for v in args.align_scores.split(',')]
        except ValueError:
            vals = []
        if len(vals) != 3:
            raise PBError('--align_scores takes three integers M,X,G (got %r)' % args.align_scores)
        par.update(zip(('match', 'mismatch', 'gap'), vals))
    if args.min_score is not None:
        par['min_score'] = args.min_score
    ops.align_params(who='--align_scores M,X,G / --min_score H', **par)
    return par


def main(argv=None):
    args = get_args(argv)
    cli.refuse_common(args, 'copy detection runs in HIP kernels (pb_runs.hip)')
    if args.min_run < 1:
        raise PBError('--min_run takes a number of keys >= 1 (got %d)' % args.min_run)
    if args.self_ and args.corpus is not None:
        raise PBError('--self compares --generated with itself; it takes no --corpus')
    if not args.self_ and args.corpus is None:
        raise PBError('--corpus (or --self) is required')
    align = _align_arg(args)
    sets = cli.load_sets(args, 'corpus')
    cli.refuse_long(sets, 'copy detection')
    tab = cli.load_tables(args.dict_file)
    gen, cor = sets[0][1], sets[-1][1]                 # --self: the corpus is the generated set
    kw = {} if align is None else {'align': align}
    res = novelty.compare_to_corpus(gen, cor, tab, start=(args.skip, 0), min_run=args.min_run, transpose=args.transpose, exclude_self=args.self_, **kw)
    cli.write_json(res, args.output)
    tag = '   [novelty]'
    print('%s %d generated pieces against %s, %s keys, runs from %d keys on; %.2f ms on the device'
          % (tag, res['n_gen'], 'themselves' if args.self_ else '%d corpus pieces' % res['n_corpus'], 'interval' if args.transpose else 'exact',
             args.min_run, res['device_ms']['total']))
    print('%s longest shared run: mean %.2f  median %.1f  max %d keys' % (tag, res['longest_mean'], res['longest_median'], res['longest_max']))
    print('%s coverage: mean %.4f | pieces at least half covered %.4f | pieces with a run >= %d keys %.4f'
          % (tag, res['coverage_mean'], res['share_half_covered'], args.min_run, res['share_with_run']))
    if res['n_gen'] and res['longest_max'] > 0:
        i = int(np.argmax(res['longest']))
        print('%s most copied: generated piece %d shares %d keys with piece %d' % (tag, i, res['longest'][i], res['nearest'][i]))
    if align is not None:
        print('%s local alignment (match %d, mismatch %d, gap %d): best score mean %.2f  median %.1f  max %d; %.2f ms on the device'
              % (tag, align['match'], align['mismatch'], align['gap'], res['align_score_mean'], res['align_score_median'], res['align_score_max'],
                 res['device_ms']['align']))
        print('%s aligned coverage: mean %.4f | pieces at least half aligned %.4f | pieces with an alignment >= %d %.4f'
              % (tag, res['align_coverage_mean'], res['share_half_aligned'], align['min_score'], res['share_with_alignment']))
    print('%s -> %s' % (tag, args.output))
    return res


if __name__ == '__main__':
    main()
