"""pb_token_scores beside pb_ce_fwd_bwd (no dlogits) on the same (T, 1280) f32 logits, in one process, for a kernel trace:

  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/score_kernel_prof.py [--rows 16384] [--launches 50]
  python tools/rocpd_stats.py <dir>/*/*.db

Both kernels read the row's 5 KB once (one wave per row, register-resident); the score kernel writes 48 B per row (logp, entropy, rank)
against the ce kernel's 16 B argmax row. The two are launched alternately, every position live (mask of ones), after warm-up launches of
each; the trace's token_scores_kernel<true> and ce_rows_reg_kernel<float> rows are the comparison (profiles/score_kernel_stats.txt).
--sizes N x 8: another dictionary's logits rows (profiles/vocab_layout_kernel_stats.txt: the wide score kernel beside the general ce kernel)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pianobart_amd import ops  # noqa: E402
from pianobart_amd._lib import LIB  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=16384)
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--sizes', type=int, nargs=8, default=None, metavar='N', help='the 8 head sizes of another dictionary, e.g. 1030 134 135 518 300 38 260 55: '
                    'a head over 320 classes selects token_scores_wide_kernel and the general ce_kernel')
    a = ap.parse_args()
    lay = ops.Layout(a.sizes) if a.sizes else ops.DEFAULT_LAYOUT
    if not torch.cuda.is_available():
        raise SystemExit('score_kernel_prof needs an MI355X: there is no CPU path')
    T = a.rows
    g = torch.Generator(device='cuda').manual_seed(0)
    logits = 2.0 * torch.randn(T, lay.vocab, generator=g, device='cuda')
    tgt = torch.stack([torch.randint(0, n, (T,), generator=g, device='cuda') for n in lay.sizes], 1).to(torch.int16)
    mask = torch.ones(T, device='cuda')
    loss_mask = torch.ones(T, 8, device='cuda')
    logp, ent = torch.empty(T, 8, device='cuda'), torch.empty(T, 8, device='cuda')
    rank = torch.empty(T, 8, dtype=torch.int16, device='cuda')
    argmax = torch.empty(T, 8, dtype=torch.int16, device='cuda')
    sums = torch.zeros(24, device='cuda')
    partials = torch.empty(int(LIB.query('pb_ce_partials_floats')), device='cuda')
    for _ in range(a.warmup + a.launches):
        ops.ce_fwd_bwd(logits, tgt, loss_mask, sums, partials, None, None, argmax, layout=lay)
        ops.token_scores(logits, tgt, mask, logp, ent, rank, layout=lay)
    torch.cuda.synchronize()
    hits = int((rank == 0).sum())
    assert hits == int((argmax == tgt).sum())                 # the two kernels agree on what a hit is
    print('rows %d, launches %d + %d warm-up of each kernel, hits %d' % (T, a.launches, a.warmup, hits))


if __name__ == '__main__':
    main()
