"""python -m pianobart_amd.eval_embedding: compare a generated set of pieces with a reference set in the embedding space of a trained
PianoBART encoder (pianobart_amd.embedding): a Frechet distance and precision / recall / density / coverage.

  --generated g.npy   what eval_generation wrote: (N, S, 8), or (N, n, S, 8) with --samples n (the samples are flattened to N * n pieces)
  --reference r.npy   the data to compare with, e.g. the test split the prompts came from: (N, S, 8)
  --ckpt pre.ckpt     the encoder, with eval_generation's model flags (--hs --layers --ffn_dims --heads --max_seq_len --precision
                      --dict_file --nopretrain --cuda_devices)
  --k K               the neighbour whose distance is a ball's radius (default 5; below the smaller set's size, at most 64)
  --skip K            the first K rows of every piece do not count (a prime of K rows that both sets share); bar ids are not rebased
  --max_pieces N      the first N pieces of each file only
  --batch_size B      pieces per encoder pass
  --output e.json     the result of embedding.compare_embeddings as JSON
  --save_embeddings PREFIX   also write PREFIX_generated.npy and PREFIX_reference.npy, the (n, d) float32 vectors of the non-empty pieces
  --embeddings_generated a.npy --embeddings_reference b.npy   compare two saved embedding files; no model, no pieces

This is not the reference's "FAD" of finetune_generation (it needs the third-party `shapesimilarity`); those lines stay n/a."""
import argparse
import os

import numpy as np
import torch

from . import embedding
from ._lib import PBError
from .eval_metrics import load_pieces, write_json
from .pieces import VOCAB


def get_args(argv=None):
    ap = argparse.ArgumentParser(description='')
    ap.add_argument('--generated', type=str, default=None)
    ap.add_argument('--reference', type=str, default=None)
    ap.add_argument('--embeddings_generated', type=str, default=None)
    ap.add_argument('--embeddings_reference', type=str, default=None)
    ap.add_argument('--save_embeddings', type=str, default=None, metavar='PREFIX')
    ap.add_argument('--k', type=int, default=5)
    ap.add_argument('--skip', type=int, default=0, metavar='K')
    ap.add_argument('--max_pieces', type=int, default=None, metavar='N')
    ap.add_argument('--batch_size', type=int, default=16)
    ap.add_argument('--output', type=str, default='./embedding.json')
    # the model, as eval_generation builds it
    ap.add_argument('--dict_file', type=str, default=VOCAB)
    ap.add_argument('--ckpt', type=str, default='result/pretrain/pianobart/model_best.ckpt')
    ap.add_argument('--max_seq_len', type=int, default=1024)
    ap.add_argument('--hs', type=int, default=1024)
    ap.add_argument('--layers', type=int, default=8)
    ap.add_argument('--ffn_dims', type=int, default=2048)
    ap.add_argument('--heads', type=int, default=8)
    ap.add_argument('--nopretrain', action='store_true', default=False)
    ap.add_argument('--cpu', action='store_true')
    ap.add_argument('--cuda_devices', type=int, nargs='+', default=[0], help='HIP device id (one)')
    ap.add_argument('--precision', default='bf16', choices=['bf16', 'fp32', 'bf16x3'])
    return ap.parse_args(argv)


def load_embeddings(path, what):
    """An (n, d) float array from a .npy file; PBError for a missing file or another shape."""
    if not os.path.isfile(path):
        raise PBError('%s: no file %r' % (what, path))
    a = np.load(path, allow_pickle=False)
    if a.ndim != 2 or a.dtype.kind != 'f' or a.shape[1] < 1:
        raise PBError('%s %r holds %s of shape %s; embeddings are (n, d) floats' % (what, path, a.dtype, a.shape))
    return a


def check_args(args):
    """The refusals that need no file and no device."""
    if args.cpu:
        raise PBError('--cpu: the encoder and the set kernels run in HIP kernels (pb_embed.hip); there is no CPU path')
    if args.skip < 0 or (args.max_pieces is not None and args.max_pieces < 1) or args.batch_size < 1:
        raise PBError('--skip takes a number of rows >= 0, --max_pieces a number of pieces >= 1 and --batch_size a number >= 1')
    if args.k < 1:
        raise PBError('--k takes a neighbour 1 .. 64 (got %d)' % args.k)
    saved = (args.embeddings_generated is not None, args.embeddings_reference is not None)
    if saved[0] != saved[1]:
        raise PBError('--embeddings_generated and --embeddings_reference come together')
    if all(saved) and (args.generated is not None or args.reference is not None or args.save_embeddings is not None):
        raise PBError('--embeddings_* compare saved embeddings: not with --generated, --reference or --save_embeddings')
    if not any(saved) and (args.generated is None or args.reference is None):
        raise PBError('give --generated and --reference (pieces), or --embeddings_generated and --embeddings_reference (saved embeddings)')
    return all(saved)


def main(argv=None):
    args = get_args(argv)
    if check_args(args):
        g = load_embeddings(args.embeddings_generated, '--embeddings_generated')
        r = load_embeddings(args.embeddings_reference, '--embeddings_reference')
        embedding.check_sets(g, r, args.k)
        res = embedding.compare_embedded(g, r, args.k)
    else:
        gen = load_pieces(args.generated, '--generated', args.max_pieces)
        ref = load_pieces(args.reference, '--reference', args.max_pieces)
        for flag, path in (('--dict_file', args.dict_file),) + ((('--ckpt', args.ckpt),) if not args.nopretrain else ()):
            if not os.path.isfile(path):
                raise PBError('%s: no file %r' % (flag, path))
        from .eval_generation import build_model
        from .pretrain import _load_vocab
        e2w, w2e = _load_vocab(args.dict_file)
        model = build_model(args, e2w, w2e)
        pb = model.pianobart
        rows_g, _, empty_g = embedding.arrange(gen, pb.layout, pb.pad_word_np, args.skip)
        rows_r, _, empty_r = embedding.arrange(ref, pb.layout, pb.pad_word_np, args.skip)
        embedding.check_counts(rows_g.shape[0], rows_r.shape[0], args.k)
        if not torch.cuda.is_available():
            raise PBError('pianobart_amd has no CPU execution path: eval_embedding needs an MI355X')
        model = model.to(torch.device('cuda', args.cuda_devices[0] if args.cuda_devices else 0)).eval()
        timer = embedding.pieces.Timer(embedding.STAGES)
        g = embedding._embed_rows(pb, rows_g, args.batch_size, timer)
        r = embedding._embed_rows(pb, rows_r, args.batch_size, timer)
        if args.save_embeddings is not None:
            np.save(args.save_embeddings + '_generated.npy', g.cpu().numpy())
            np.save(args.save_embeddings + '_reference.npy', r.cpu().numpy())
        res = embedding.compare_embedded(g, r, args.k, empty_g, empty_r, pb.precision, timer)
    write_json(res, args.output)
    print('   [embedding] %d generated (%d empty), %d reference (%d empty) pieces, d = %d, k = %d; %.2f ms on the device'
          % (res['n_gen'], res['empty_gen'], res['n_ref'], res['empty_ref'], res['d'], res['k'], res['device_ms']['total']))
    print('   [embedding] Frechet distance %.6f = mean %.6f + trace %.6f%s'
          % (res['fmd'], res['mean_term'], res['trace_term'], '  (rank deficient: fewer pieces than dimensions)' if res['rank_deficient'] else ''))
    print('   [embedding] precision %.4f  recall %.4f  density %.4f  coverage %.4f' % (res['precision'], res['recall'], res['density'], res['coverage']))
    print('   [embedding] -> %s' % args.output)
    return res


if __name__ == '__main__':
    main()
