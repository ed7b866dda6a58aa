"""Texture columns (pianobart_amd.texture, csrc/pb_texture.hip) at the two shapes of tools/structure_bench.py and tools/harmony_bench.py:
2 048 pieces of 256 rows and 256 pieces of 1 024 rows, the seeded piano-like pieces of the tests (tests/texture_ref.py: chords, overlaps,
one row in ten percussion), every piece filling its window.

    python tools/texture_bench.py [--out profiles/texture_kernel_stats.txt]

pb_piece_texture runs three times between device events on data already on the device; the third run is reported, with the
compare-exchanges of its three bitonic sorts per second: a sort of n keys (n a power of two) takes n / 2 * log2(n) * (log2(n) + 1) / 2 of
them, and a piece sorts its P pitched notes twice (32-bit and 64-bit keys) and its E interval events once, each padded to a power of two.
Next to it the share of a ceiling: INSTR_PER_EXCHANGE instructions per compare-exchange (a lane holds one exchange), counted in the
compiled loops (hipcc -S of pb_texture.hip for gfx950), against 256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz lane-instructions per second.
pb_piece_structure and pb_piece_harmony run on the same pieces in the same process as yardsticks. The result is checked against the
restatement on the first 4 pieces of each shape. The last line printed is one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(2048, 256), (256, 1024)]
INSTR_PER_EXCHANGE = 27             # the compiled exchange loop: 16 up to the compare (2 ds_read among them), 5 in the swap (2 ds_write), 6 in the loop's tail
LANE_RATE = 256 * 4 * 32 * 2.4e9    # a SIMD issues a wave64 vector instruction over 2 cycles of 32 lanes


def exchanges(n):
    """Compare-exchanges of a bitonic sort of n keys padded to a power of two."""
    p = 1
    while p < n:
        p *= 2
    k = p.bit_length() - 1
    return p // 2 * k * (k + 1) // 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    from pianobart_amd import ops, pieces
    from tests import texture_ref as R
    if not torch.cuda.is_available():
        raise SystemExit('texture_bench needs a GPU: nothing is measured without one')
    dev = torch.device('cuda', 0)
    tab = pieces.tables()
    pad8 = list(tab.layout.pad8)
    up = lambda x: torch.from_numpy(x).to(dev)
    pitch_of, dur_pos, bar_pos = up(tab.pitch_of), up(tab.dur_pos), up(tab.bar_pos)
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

    say('texture columns, %s' % torch.cuda.get_device_name(0))
    for N, S in SHAPES:
        ids = np.stack([R.from_notes(R.piano_notes(S, 7000 + S + n), S, np.asarray(pad8)) for n in range(N)])
        d = up(ids.astype(np.int16))
        cols, ms = third(lambda: ops.piece_texture(d, pitch_of, dur_pos, bar_pos))
        _, ms_st = third(lambda: ops.piece_structure(d, pitch_of))
        _, ms_hm = third(lambda: ops.piece_harmony(d, pitch_of))
        cols = cols.cpu().numpy().astype(np.int64)
        assert np.array_equal(cols[:4], R.texture(ids[:4], pad8, tab.pitch_of, tab.dur_pos, tab.bar_pos)), 'the kernel and the restatement disagree'
        P, events = cols[:, 1], 2 * (cols[:, 14] - cols[:, 9])
        cx = float(sum(2 * exchanges(int(p)) + exchanges(int(e)) for p, e in zip(P, events)))
        share = cx * INSTR_PER_EXCHANGE / (ms * 1e-3) / LANE_RATE
        say('%d piano-like pieces of %d rows: mean P %.1f, mean events %.1f, %.4g compare-exchanges' % (N, S, P.mean(), events.mean(), cx))
        say('  pb_piece_texture     %9.3f ms   %10.4g compare-exchanges/s   %.4f of the ceiling at %d instructions per exchange'
            % (ms, cx / ms * 1e3, share, INSTR_PER_EXCHANGE))
        say('  pb_piece_structure   %9.3f ms   (the same pieces, the same process)' % ms_st)
        say('  pb_piece_harmony     %9.3f ms   (the same pieces, the same process)' % ms_hm)
        say('  pooled: silence %.4f  mean polyphony %.4f  collisions %d  duplicates %d'
            % (cols[:, 16].sum() / cols[:, 3].sum(), cols[:, 6].sum() / cols[:, 4].sum(), cols[:, 9].sum(), cols[:, 10].sum()))
        result['%dx%d' % (N, S)] = {'ms': round(ms, 4), 'exchanges_per_s': cx / ms * 1e3, 'ceiling_share': round(share, 5),
                                    'structure_ms': round(ms_st, 4), 'harmony_ms': round(ms_hm, 4)}
    say(json.dumps(result))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
