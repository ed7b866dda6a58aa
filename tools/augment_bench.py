"""Time pb_augment beside the two kernels it joins in Pretrainer.prepare_batch, pb_corrupt and pb_shift_right, in one process:
    python tools/augment_bench.py [--out profiles/augment_kernel_stats.txt] [--calls 200]

Shapes: (32, 1024, 8), the pre-train batch, for all three; (8, 2048, 8) for pb_augment alone (the longest piece pb_corrupt takes). Each
kernel is warmed up, then timed three times with device events around `--calls` back-to-back launches; the THIRD run is the figure (the
first two are listed beside it: their spread is the noise). The bytes are what the algorithm needs: pb_augment reads and writes the rows
once (the second read of pass 2 is served by L2) plus 13 KB of tables per workgroup. Needs an MI355X: there is no CPU path."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pianobart_amd import augment, ops                                   # noqa: E402
from tests.golden_util import synth_octuple_batch                        # noqa: E402


def timed(fn, calls):
    """ms per call of three runs of `calls` launches each, after a warm-up."""
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    runs = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        runs.append(a.elapsed_time(b) / calls)
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'augment_kernel_stats.txt'))
    ap.add_argument('--calls', type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('augment_bench: needs an MI355X (not measured)')
    dev = torch.device('cuda', 0)
    plan = augment.AugmentPlan(None, pitch=(-6, 5), velocity=(-2, 2), tempo=(-2, 2), pitch_bounds=(21, 108))
    lay = ops.DEFAULT_LAYOUT
    pad_row, mask_row = list(lay.pad8), [p + 1 for p in lay.pad8]
    sos = torch.tensor([p + 2 for p in lay.pad8], dtype=torch.int16, device=dev)
    lines, res = [], {}

    def row(name, shape, runs, nbytes):
        ms = runs[2]
        lines.append('  %-16s %-14s %8.2f us   (runs %s us)   %7.1f GB/s of %.2f MB' % (
            name, '(%d, %d, 8)' % shape, ms * 1e3, ', '.join('%.2f' % (r * 1e3) for r in runs), nbytes / ms / 1e6, nbytes / 1e6))
        res['%s_%dx%d_us' % (name, *shape)] = round(ms * 1e3, 3)

    for B, S in ((32, 1024), (8, 2048)):
        ids = ops.ids_to_i16(synth_octuple_batch(B, S, seed=1)[5].to(dev))
        out = torch.empty_like(ids)
        shifts = torch.empty(B, 3, dtype=torch.int32, device=dev)
        coord, id_at = plan.tables(dev)
        rows_bytes = B * S * 16
        row('pb_augment', (B, S), timed(lambda: ops.augment(ids, out, shifts, coord, id_at, plan._plan18, 7), args.calls), 2 * rows_bytes + B * 13056)
        if (B, S) != (32, 1024):
            continue
        lm = torch.empty(B, S, 8, dtype=torch.float32, device=dev)
        choice = torch.tensor([1 + b % 5 for b in range(B)], dtype=torch.int32, device=dev)      # the five corruptions in equal parts
        row('pb_corrupt', (B, S), timed(lambda: ops.corrupt(ids, out, lm, choice, None, 0.15, 7, pad_row, mask_row, lay.sizes), args.calls),
            2 * rows_bytes + B * S * 32)
        row('pb_shift_right', (B, S), timed(lambda: ops.shift_right(ids, sos, out, B, S), args.calls), 2 * rows_bytes)
    a, c = res['pb_augment_32x1024_us'], res['pb_corrupt_32x1024_us']
    head = 'Octuple augmentation, %s: device events around %d back-to-back launches, third run of three (after a warm-up of 10)' % (
        torch.cuda.get_device_name(0), args.calls)
    tail = '  pb_augment takes %.2f of pb_corrupt\'s time on the pre-train batch' % (a / c)
    text = '\n'.join([head] + lines + [tail, json.dumps(res)]) + '\n'
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
