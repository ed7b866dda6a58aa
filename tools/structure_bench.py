"""Repetition structure (pianobart_amd.structure, csrc/pb_structure.hip) at two shapes: 2 048 pieces of 256 rows and 256 pieces of 1 024
rows, the seeded motif pieces of the tests (tests/structure_ref.py: one-, two- and four-bar motifs, edit rate 0.2), every piece filling
its window; and the first shape once more with unrelated notes (positions and pitches drawn afresh for every note), where next to no pair
counts: the difference is what the matches cost.

    python tools/structure_bench.py [--numpy 64] [--out profiles/structure_kernel_stats.txt]

pb_piece_structure runs three times between device events on data already on the device; the third run is reported, with note pairs per
second: a piece of n notes is n^2 pairs, the pairs one all-pairs pass looks at (the kernel makes one and a half such passes). The result
is checked against the restatement on the first 8 pieces of each shape. The last line printed is one JSON line with the milliseconds and
the pairs per second of both shapes. --numpy P times the restatement on P pieces of the first shape on this host and scales it by the
pair count (labelled "scaled, not run"); 0 skips it."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(2048, 256), (256, 1024)]


def unrelated(sizes, N, S, seed):
    """(N, S, 8) pieces in time order, 2 to 5 notes per bar, whose positions (0 .. 127) and pitches (0 .. 127) are drawn afresh for every note:
    the same pair counts as the motif pieces with next to nothing that returns."""
    rng = np.random.default_rng(seed)
    pad = np.asarray(sizes) - 6
    ids = np.stack([rng.integers(0, pad[h], size=(N, S)) for h in range(8)], axis=2).astype(np.int64)
    ids[:, :, 0] = np.minimum(np.cumsum(rng.random((N, S)) < 1 / 3.5, axis=1), pad[0] - 1)
    ids[:, :, 1] = rng.integers(0, 128, size=(N, S))
    ids[:, :, 3] = rng.integers(0, 128, size=(N, S))
    return ids


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--numpy', type=int, default=64)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    from pianobart_amd import metrics, ops
    from tests import structure_ref as R
    if not torch.cuda.is_available():
        raise SystemExit('structure_bench needs a GPU: nothing is measured without one')
    dev = torch.device('cuda', 0)
    tab = metrics.tables()
    pad8 = list(tab.layout.pad8)
    pitch_of = torch.from_numpy(tab.pitch_of).to(dev)
    lines, result = [], {}

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

    say('repetition structure, %s, %d lags, exact pitch' % (torch.cuda.get_device_name(0), ops.STRUCTURE_LAGS))
    for N, S, kind in [(N, S, 'motif') for N, S in SHAPES] + [SHAPES[0] + ('unrelated',)]:
        sizes = list(tab.layout.sizes)
        ids = R.motif_pieces(sizes, N, S, seed=7 + S, mb=(1, 2, 4), edit=0.2) if kind == 'motif' else unrelated(sizes, N, S, 9)
        d = torch.from_numpy(ids.astype(np.int16)).to(dev)
        cols, ms = third(lambda: ops.piece_structure(d, pitch_of))
        cols = cols.cpu().numpy()
        assert np.array_equal(cols[:8], R.structure(ids[:8], pad8, tab.pitch_of)), 'the kernel and the restatement disagree'
        pairs = float((cols[:, 0].astype(np.float64) ** 2).sum())
        rep = 2.0 * cols[:, 136:152].sum() / max(1, cols[:, 200:216].sum())
        say('%d %s pieces of %d rows: %.4g note pairs' % (N, kind, S, pairs))
        say('  pb_piece_structure   %9.3f ms   %10.4g pairs/s   (pooled D_N over lags 1 .. 16: %.4f)' % (ms, pairs / ms * 1e3, rep))
        result['%dx%d%s' % (N, S, '' if kind == 'motif' else '_' + kind)] = {'ms': round(ms, 4), 'pairs_per_s': pairs / ms * 1e3}
        if args.numpy > 0 and S == SHAPES[0][1] and kind == 'motif':
            P = args.numpy
            t0 = time.perf_counter()
            small = R.structure(ids[:P], pad8, tab.pitch_of)
            sec = time.perf_counter() - t0
            small_pairs = float((small[:, 0].astype(np.float64) ** 2).sum())
            scaled = sec * pairs / small_pairs
            say('  Python-set restatement, %d pieces on this host: %.3f s = %.4g pairs/s; scaled, not run, by the pair count to %d pieces: %.1f s'
                % (P, sec, small_pairs / sec, N, scaled))
            result['restatement_%dx%d_scaled_not_run_s' % (N, S)] = round(scaled, 2)
    say(json.dumps(result))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
