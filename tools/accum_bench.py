"""Cost of gradient accumulation (Engine.loss_and_grads(micro=(i, K))) on the BASELINE configs[1] model in bf16: one optimizer step over
the SURVEY 8(d) batch of 32 sequences, taken as one batch of 32, as 2 x 16 and as 4 x 8, and the accumulate launches alone.

    python tools/accum_bench.py [--steps 10] [--warmup 3] [--out profiles/grad_accum_b32.json]

Prints one JSON line. Expectation (derived, DESIGN.md 5 "Gradient accumulation"): the separate pass moves 12 bytes per parameter per
micro-batch at the streaming rate of the row kernels, about 1 % of a step; the rest of the difference between the legs is what smaller
batches cost the kernels themselves (fewer rows per GEMM, one packing plan per micro-batch)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--seq', type=int, default=1024)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    from pianobart_amd import ops
    from pianobart_amd.model import BartConfig, PianoBart, PianoBartLM
    from tests.golden_util import load_vocab, synth_octuple_batch
    dev = torch.device('cuda', 0)
    e2w, w2e = load_vocab()
    torch.manual_seed(1)
    cfg = dict(max_position_embeddings=args.seq, d_model=768, encoder_layers=12, decoder_layers=12, encoder_ffn_dim=3072, decoder_ffn_dim=3072,
               encoder_attention_heads=12, decoder_attention_heads=12)
    model = PianoBartLM(PianoBart(BartConfig(**cfg), e2w, w2e, precision='bf16')).train().to(dev)
    eng = model._get_engine()
    eng.bind(dev)
    eng.pipeline_updates = True
    enc, dec, loss_mask, emask, dmask, target = [x.to(dev) for x in synth_octuple_batch(args.batch, args.seq, 1234)]
    whole = (ops.ids_to_i16(enc), ops.ids_to_i16(dec), ops.ids_to_i16(target), loss_mask.contiguous(), emask, dmask)

    def leg(K):
        """ms per optimizer step over the batch cut into K micro-batches of batch / K sequences."""
        per = args.batch // K
        parts = [tuple(t[i * per:(i + 1) * per].contiguous() for t in whole) for i in range(K)]
        total = eng.mask_counts(parts[0][3])
        for p in parts[1:]:
            ops.accum_f32(total, eng.mask_counts(p[3]), add=True)
        hook = (lambda c: c.copy_(total)) if K > 1 else None
        eng._pack_prefetch.clear()
        eng.prefetch_pack(*parts[0][3:6])

        def step():
            for i, p in enumerate(parts):
                eng.prefetch_pack(*parts[(i + 1) % K][3:6])          # one micro-batch ahead, as the Pretrainer
                eng.loss_and_grads(*p, train=True, ids_checked=True, count_hook=hook, micro=(i, K) if K > 1 else None)
            eng.optimizer_step(lr=2e-5)

        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    res = {'one_batch_ms': leg(1), 'accum_2x%d_ms' % (args.batch // 2): leg(2), 'accum_4x%d_ms' % (args.batch // 4): leg(4)}
    eng.finish_updates()
    # the accumulate launches alone: one pass over the whole flat buffer in add mode (12 bytes per parameter), device-timed
    n = eng.n_total
    for _ in range(3):
        ops.accum_f32(eng.G_acc, eng.G32, add=True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 20
    e0.record()
    for _ in range(reps):
        ops.accum_f32(eng.G_acc, eng.G32, add=True)
    e1.record()
    torch.cuda.synchronize()
    pass_ms = e0.elapsed_time(e1) / reps
    res.update(accum_pass_ms=pass_ms, accum_pass_GBps=12.0 * n / pass_ms / 1e6, parameters=n,
               accum_passes_per_step={'2x': 2, '4x': 4},
               accum_share_of_step_2x=2 * pass_ms / res['accum_2x%d_ms' % (args.batch // 2)],
               accum_share_of_step_4x=4 * pass_ms / res['accum_4x%d_ms' % (args.batch // 4)],
               config='BASELINE configs[1]: 12L/768d/ffn3072/12h S=%d B=%d bf16, dropout on, packed rows, %d timed steps after %d' %
                      (args.seq, args.batch, args.steps, args.warmup),
               device=torch.cuda.get_device_name(0))
    res = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
