"""Copy detection (pianobart_amd.novelty, csrc/pb_runs.hip) at two shapes: 2 048 generated against 2 048 corpus pieces of 256 rows, and
256 against 256 pieces of 1 024 rows. Synthetic pieces over a small alphabet (4 pitches, 4 positions), every piece filling its window,
with a few planted copies whose lengths the tool checks in the result.

    python tools/novelty_bench.py [--numpy 64] [--out profiles/novelty_kernel_stats.txt]
    python tools/novelty_bench.py --align --numpy 0 [--out profiles/align_kernel_stats.txt]

Each stage (pb_piece_keys over both sets; pb_shared_runs, no matrix) runs three times between device events on data already on the
device; the third run is reported, with rows/s for the keys and cells/s (K_a x K_b summed over all pairs) for the runs. --numpy P times
the numpy restatement (tests/novelty_ref.py) on P x P pieces of the first shape on this host and scales it by the cell count; 0 skips it.
--align also times pb_local_align (csrc/pb_align.hip, default scoring 1 / 2 / 2, min_score 8, no matrix) on the same keys in the same
process, the same way, and checks that the planted copies score at least their length; with --numpy it times the numpy restatement
(tests/align_ref.py) on ONE pair of the first shape and scales it by the pair count.
Nothing is asserted but the planted copies."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(2048, 2048, 256), (256, 256, 1024)]
PLANTED = [(3, 5, 40), (17, 200, 100), (40, 41, None)]              # (generated piece, corpus piece, notes copied; None = the whole piece)


def synth(N, S, seed):
    rng = np.random.default_rng(seed)
    ids = np.zeros((N, S, 8), dtype=np.int16)
    ids[:, :, 0] = np.minimum(np.cumsum(rng.random((N, S)) < 0.125, axis=1), 255)
    ids[:, :, 1] = rng.choice([0, 4, 8, 12], size=(N, S))
    ids[:, :, 3] = rng.choice([60, 62, 64, 67], size=(N, S))
    for h, n in ((2, 4), (4, 32), (5, 32), (6, 4), (7, 40)):
        ids[:, :, h] = rng.integers(0, n, size=(N, S))
    return ids


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--numpy', type=int, default=64)
    ap.add_argument('--align', action='store_true')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    from pianobart_amd import metrics, novelty, ops
    if not torch.cuda.is_available():
        raise SystemExit('novelty_bench needs a GPU: nothing is measured without one')
    dev = torch.device('cuda', 0)
    tab = metrics.tables()
    pitch_of = torch.from_numpy(tab.pitch_of).to(dev)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def third(fn):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return out, e0.elapsed_time(e1)

    say('copy detection, %s, %d corpus pieces per workgroup, min_run = 8, exact keys' % (torch.cuda.get_device_name(0), ops.RUNS_TILE))
    for N, M, S in SHAPES:
        gen, cor = synth(N, S, 1), synth(M, S, 2)
        for i, j, n in PLANTED:
            n = n or S
            gen[i, S - n:, :4] = cor[j, S - n:, :4]
        g, c = torch.from_numpy(gen).to(dev), torch.from_numpy(cor).to(dev)
        ((ka, la), (kb, lb)), ms_keys = third(lambda: (ops.piece_keys(g, pitch_of), ops.piece_keys(c, pitch_of)))
        (_, run_end, best), ms_runs = third(lambda: ops.shared_runs(ka, la, kb, lb, min_run=8, want_matrix=False))
        cells = float(la.sum().item()) * float(lb.sum().item())
        longest, nearest = novelty.split_best(best)
        for i, j, n in PLANTED:
            n = n or S
            assert longest[i] >= n - 1 and (nearest[i] == j or longest[i] > n - 1), (i, j, n, longest[i], nearest[i])
        cov = novelty.coverage(run_end, la)
        say('%d x %d pieces of %d rows: %.4g cells' % (N, M, S, cells))
        say('  pb_piece_keys  (both sets)   %9.3f ms   %10.4g rows/s' % (ms_keys, (N + M) * S / ms_keys * 1e3))
        say('  pb_shared_runs (no matrix)   %9.3f ms   %10.4g cells/s' % (ms_runs, cells / ms_runs * 1e3))
        say('  longest shared run: median %d, max %d keys; mean coverage %.4f' % (np.median(longest), longest.max(), np.nanmean(cov)))
        if args.align:
            (_, align_end, abest), ms_align = third(lambda: ops.local_align(ka, la, kb, lb, want_matrix=False))
            ascore, anearest = novelty.split_best(abest)
            for i, j, n in PLANTED:
                n = n or S
                assert ascore[i] >= n - 1 and (anearest[i] == j or ascore[i] > n - 1), (i, j, n, ascore[i], anearest[i])
            acov = novelty.align_coverage(align_end, la)
            say('  pb_local_align (no matrix)   %9.3f ms   %10.4g cells/s   (%.1f x pb_shared_runs)' % (ms_align, cells / ms_align * 1e3, ms_align / ms_runs))
            say('  best alignment score: median %d, max %d; mean aligned coverage %.4f' % (np.median(ascore), ascore.max(), np.nanmean(acov)))
            if args.numpy > 0 and S == SHAPES[0][2]:
                from tests import align_ref
                a, b = ka[0].cpu().numpy().view(np.uint32)[:int(la[0])], kb[0].cpu().numpy().view(np.uint32)[:int(lb[0])]
                t0 = time.perf_counter()
                align_ref.pair_fast(a, b)
                sec = time.perf_counter() - t0
                say('  numpy restatement of the alignment, one pair on this host: %.4f s = %.4g cells/s; SCALED by the pair count to %d x %d: %.0f s'
                    % (sec, len(a) * len(b) / sec, N, M, sec * N * M))
        if args.numpy > 0 and S == SHAPES[0][2]:
            from tests import novelty_ref as R
            P = args.numpy
            pad8 = list(tab.layout.pad8)
            t0 = time.perf_counter()
            a, al = R.keys_ref(gen[:P].astype(np.int64), pad8, tab.pitch_of)
            b, bl = R.keys_ref(cor[:P].astype(np.int64), pad8, tab.pitch_of)
            R.outputs_ref(a, al, b, bl, min_run=8)
            sec = time.perf_counter() - t0
            small = float(al.sum()) * float(bl.sum())
            say('  numpy restatement, %d x %d pieces on this host: %.2f s = %.4g cells/s; SCALED by the cell count to %d x %d: %.0f s'
                % (P, P, sec, small / sec, N, M, sec * cells / small))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
