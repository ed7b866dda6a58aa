"""Harmony columns (pianobart_amd.harmony, csrc/pb_harmony.hip) at the two shapes of tools/structure_bench.py: 2 048 pieces of 256 rows and
256 pieces of 1 024 rows, the seeded motif pieces of the tests (tests/structure_ref.py: one-, two- and four-bar motifs, edit rate 0.2), every
piece filling its window.

    python tools/harmony_bench.py [--out profiles/harmony_kernel_stats.txt]

pb_piece_harmony runs three times between device events on data already on the device; the third run is reported, with bar pairs per
second: a piece of W bars has sum over l = 1 .. 64 of max(W - l, 0) bar pairs, each of them 12 transpositions of 12 classes. Next to it
the share of the integer-VALU ceiling: VALU_PER_PAIR vector instructions per bar pair (a lane holds one pair), counted in the compiled pair loop (hipcc -S of
pb_harmony.hip for gfx950: the block between the loads of a partner bar's words and the two accumulator adds), against 256 CUs x 4
SIMDs x 32 lanes x 2.4 GHz lane-instructions per second. pb_piece_structure runs on the same pieces in the same process as the yardstick.
The result is checked against the restatement on the first 4 pieces of each shape. The last line printed is one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(2048, 256), (256, 1024)]
VALU_PER_PAIR = 95                  # the compiled pair block: 72 v_sad_u16, 6 v_perm_b32, 5 v_min3_u32, 1 v_min_u32, 5 adds, 2 subs, 2 shifts, 2 compares
LANE_RATE = 256 * 4 * 32 * 2.4e9    # a SIMD issues a wave64 vector instruction over 2 cycles of 32 lanes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    from pianobart_amd import metrics, ops
    from tests import harmony_ref as R
    from tests import structure_ref as SR
    if not torch.cuda.is_available():
        raise SystemExit('harmony_bench needs a GPU: nothing is measured without one')
    dev = torch.device('cuda', 0)
    tab = metrics.tables()
    pad8 = list(tab.layout.pad8)
    pitch_of = torch.from_numpy(tab.pitch_of).to(dev)
    ops.harmony_table(dev)
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

    say('harmony columns, %s, %d lags, windows of 1 and 4 bars' % (torch.cuda.get_device_name(0), ops.HARMONY_LAGS))
    for N, S in SHAPES:
        ids = SR.motif_pieces(list(tab.layout.sizes), N, S, seed=7 + S, mb=(1, 2, 4), edit=0.2)
        d = torch.from_numpy(ids.astype(np.int16)).to(dev)
        cols, ms = third(lambda: ops.piece_harmony(d, pitch_of))
        _, ms_st = third(lambda: ops.piece_structure(d, pitch_of))
        cols = cols.cpu().numpy()
        assert np.array_equal(cols[:4], R.harmony(ids[:4], pad8, tab.pitch_of)), 'the kernel and the restatement disagree'
        W = cols[:, 1].astype(np.int64)
        pairs = float(sum(np.maximum(W - l, 0).sum() for l in range(1, ops.HARMONY_LAGS + 1)))
        dh = 2.0 * cols[:, 36:52].sum() / max(1, cols[:, 100:116].sum())
        dx = 2.0 * cols[:, 164:180].sum() / max(1, cols[:, 100:116].sum())
        share = pairs * VALU_PER_PAIR / (ms * 1e-3) / LANE_RATE            # a lane works on one bar pair at a time
        say('%d motif pieces of %d rows: %.4g bar pairs (mean W %.1f)' % (N, S, pairs, W.mean()))
        say('  pb_piece_harmony     %9.3f ms   %10.4g bar pairs/s   %.3f of the integer-VALU ceiling at %d vector instructions per pair'
            % (ms, pairs / ms * 1e3, share, VALU_PER_PAIR))
        say('  pb_piece_structure   %9.3f ms   (the same pieces, the same process)' % ms_st)
        say('  pooled over lags 1 .. 16: D_H %.4f  D_X %.4f' % (dh, dx))
        result['%dx%d' % (N, S)] = {'ms': round(ms, 4), 'bar_pairs_per_s': pairs / ms * 1e3, 'valu_share': round(share, 4), 'structure_ms': round(ms_st, 4)}
    say(json.dumps(result))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
