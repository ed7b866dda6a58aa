"""Embedding-space set metrics (pianobart_amd.embedding, csrc/pb_embed.hip) at the size of a real evaluation: 2 048 generated against 2 048
reference pieces of 1 024 rows (the seeded pieces of tests/metrics_ref.py, two styles), the encoder of BASELINE.json configs[1] (12 layers,
d = 768, ffn 3 072, 12 heads, bf16) with seeded random weights.

    python tools/embedding_bench.py [--out profiles/embedding_kernel_stats.txt] [--pieces 2048] [--rows 1024]

embedding.compare_embeddings runs three times; the device milliseconds per stage of the third run are reported (pieces.Timer: pairs of
device events). Then, in the same process, on the embeddings of that run and by device events on the third of three calls:
  pb_sqdist against ops.gemm in f32 on the same (N, M, K): the GEMM's matrix cores do none of the 2 vector operations per term that the
  difference form needs, so pb_sqdist is expected to be slower; how much is what this file is for;
  pb_embed_moments against pb_gram_accum f32 on the same X (one f32-input MFMA pass against two f64 fma passes).
The PRDC numbers are checked against the restatement of tests/embedding_ref.py on the device's own distances. The last line printed is
one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    ap.add_argument('--pieces', type=int, default=2048)
    ap.add_argument('--rows', type=int, default=1024)
    ap.add_argument('--batch_size', type=int, default=32)
    ap.add_argument('--k', type=int, default=5)
    args = ap.parse_args()
    from pianobart_amd import embedding, ops
    from pianobart_amd._lib import PB_F32
    from pianobart_amd.model import BartConfig, PianoBart
    from tests import embedding_ref as R
    from tests.golden_util import load_vocab, randomize_params
    from tests.metrics_ref import synth_pieces
    from tests.vocab_layout_util import D_DEFAULT
    if not torch.cuda.is_available():
        raise SystemExit('embedding_bench needs a GPU: nothing is measured without one')
    dev = torch.device('cuda', 0)
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

    N, S, d = args.pieces, args.rows, 768
    e2w, w2e = load_vocab()
    cfg = BartConfig(max_position_embeddings=S, d_model=d, encoder_layers=12, decoder_layers=12, encoder_ffn_dim=3072, decoder_ffn_dim=3072,
                     encoder_attention_heads=12, decoder_attention_heads=12)
    model = PianoBart(cfg, e2w, w2e, precision='bf16')
    randomize_params(model, 3)
    model = model.to(dev).eval()
    gen, ref = synth_pieces(D_DEFAULT, N, S, seed=21, style=1), synth_pieces(D_DEFAULT, N, S, seed=22)
    say('embedding-space set metrics, %s: %d generated x %d reference pieces of %d rows, encoder 12 x d = %d (bf16), k = %d'
        % (torch.cuda.get_device_name(0), N, N, S, d, args.k))
    for _ in range(3):
        res = embedding.compare_embeddings(model, gen, ref, k=args.k, batch_size=args.batch_size)
    ms = res['device_ms']
    for stage in embedding.STAGES:
        say('  %-10s %10.3f ms   %5.1f %% of the device time' % (stage, ms[stage], 100.0 * ms[stage] / ms['total']))
    say('  %-10s %10.3f ms   fmd %.4f (mean %.4f + trace %.4f)  precision %.4f  recall %.4f  density %.4f  coverage %.4f'
        % ('total', ms['total'], res['fmd'], res['mean_term'], res['trace_term'], res['precision'], res['recall'], res['density'], res['coverage']))

    g, _ = embedding.embed_set(model, gen, batch_size=args.batch_size)
    r, _ = embedding.embed_set(model, ref, batch_size=args.batch_size)
    n, m = g.shape[0], r.shape[0]
    d2 = {name: ops.sqdist(a, b).cpu().numpy() for name, (a, b) in dict(gg=(g, g), rr=(r, r), gr=(g, r)).items()}
    want = R.prdc_from_d2(d2['gg'], d2['rr'], d2['gr'], args.k)
    assert all(res[name] == v for name, v in want.items()), 'the kernels and the restatement disagree: %s' % want

    out = torch.empty((n, m), dtype=torch.float32, device=dev)
    _, ms_sq = third(lambda: ops.sqdist(g, r, out))
    C = torch.empty((n, m), dtype=torch.float32, device=dev)
    _, ms_gemm = third(lambda: ops.gemm(g, r, C, M=n, N=m, K=d, dtype=PB_F32))
    terms = float(n) * m * d
    say('pb_sqdist   (%d, %d, %d): %8.3f ms   %.4g terms/s   (3 flops a term: %.2f Tflop/s)' % (n, m, d, ms_sq, terms / ms_sq * 1e3, 3 * terms / ms_sq * 1e-9))
    say('ops.gemm f32 on the same shape: %8.3f ms   %.4g terms/s   pb_sqdist takes %.2f times as long' % (ms_gemm, terms / ms_gemm * 1e3, ms_sq / ms_gemm))
    ws = ops.embed_ws(n, d, dev)
    _, ms_mom = third(lambda: ops.embed_moments(g, ws))
    G = torch.zeros((d, d), dtype=torch.float32, device=dev)
    gws = ops.gram_ws(n, d, dev)
    _, ms_gram = third(lambda: ops.gram_accum(G, g, gws))
    say('pb_embed_moments (%d, %d): %8.3f ms   pb_gram_accum f32 on the same X: %8.3f ms   (%.2f times as long; f64 fma against f32-input MFMA)'
        % (n, d, ms_mom, ms_gram, ms_mom / ms_gram))
    result = {'stages_ms': {k: round(v, 4) for k, v in ms.items()}, 'sqdist_ms': round(ms_sq, 4), 'gemm_f32_ms': round(ms_gemm, 4),
              'moments_ms': round(ms_mom, 4), 'gram_f32_ms': round(ms_gram, 4), 'n_gen': n, 'n_ref': m, 'd': d,
              'fmd': res['fmd'], 'precision': res['precision'], 'recall': res['recall'], 'density': res['density'], 'coverage': res['coverage']}
    say(json.dumps(result))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
