"""pb_distill_fwd_bwd beside pb_ce_fwd_bwd on the same (T, 1280) f32 logits, in one process, and the distilled step beside the plain one.

  python tools/distill_bench.py [--rows 16384] [--launches 50]                  call times by device events, after a warm-up
  python tools/distill_bench.py --step [--batch 32] [--seq 1024] [--steps 10]   + plain step / distilled step / teacher forward, alternating
  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/distill_bench.py --kernels-only
  python tools/rocpd_stats.py <dir>/*/*.db                                       kernel times (profiles/distill_kernel_stats.txt)

Both kernels write the same bf16 dlogits (T x 2560 B) and int16 argmax rows; the distillation kernel reads the teacher's logits row beside
the student's: (2 x 5120 + 2560) / (5120 + 2560) = 1.67 times K9's traffic per row, which is the ratio to expect of a kernel that streams.
The calls alternate, so both see the same clocks; the figures are printed, nothing is gated. --step: a 6-layer student of the benchmark
model's width (768 / ffn 3072 / 12 heads) under the 12-layer benchmark model as teacher, bf16, on the benchmark's synthetic batch."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pianobart_amd import ops  # noqa: E402
from pianobart_amd._lib import LIB  # noqa: E402


def _timed(fn, n):
    """mean milliseconds of n calls of fn, by device events around each call."""
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) for a, b in evs)
    return sum(t) / n, t[n // 2], t[0]


def kernels(a):
    lay = ops.DEFAULT_LAYOUT
    T, V = a.rows, lay.vocab
    g = torch.Generator(device='cuda').manual_seed(0)
    z = 2.0 * torch.randn(T, V, generator=g, device='cuda')
    u = 2.0 * torch.randn(T, V, generator=g, device='cuda')
    tgt = torch.stack([torch.randint(0, n, (T,), generator=g, device='cuda') for n in lay.sizes], 1).to(torch.int16)
    lm = torch.ones(T, 8, device='cuda')
    coef = torch.full((8,), 1.0 / T, device='cuda')
    dl = torch.empty(T, V, device='cuda', dtype=torch.bfloat16)
    am = torch.empty(T, 8, dtype=torch.int16, device='cuda')
    s24, s40 = torch.zeros(24, device='cuda'), torch.zeros(40, device='cuda')
    p_ce = torch.empty(int(LIB.query('pb_ce_partials_floats')), device='cuda')
    p_d = torch.empty(int(LIB.query('pb_distill_partials_floats')), device='cuda')
    ce = lambda: ops.ce_fwd_bwd(z, tgt, lm, s24, p_ce, coef, dl, am, layout=lay)
    kd = lambda: ops.distill_fwd_bwd(z, u, None, tgt, lm, s40, p_d, coef, dl, am, 0.5, 2.0, 0.0, layout=lay)
    ls = lambda: ops.distill_fwd_bwd(z, None, None, tgt, lm, s40, p_d, coef, dl, am, 0.0, 1.0, 0.1, layout=lay)
    for _ in range(a.warmup):
        ce(); kd(); ls()
    torch.cuda.synchronize()
    if a.kernels_only:
        for _ in range(a.launches):
            ce(); kd(); ls()
        torch.cuda.synchronize()
        print('rows %d, launches %d + %d warm-up of ce / distill / smoothing-only' % (T, a.launches, a.warmup))
        return
    res = {'ce': [], 'distill': [], 'smooth': []}
    for _ in range(a.launches):                                   # alternating, one call per event pair
        res['ce'].append(_timed(ce, 1)[0]); res['distill'].append(_timed(kd, 1)[0]); res['smooth'].append(_timed(ls, 1)[0])
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    rd, wr = T * V * 4, T * V * 2 + T * 16
    out = {'rows': T, 'launches': a.launches,
           'ce_call_ms_median': med['ce'], 'distill_call_ms_median': med['distill'], 'smooth_only_call_ms_median': med['smooth'],
           'ce_call_ms_min': min(res['ce']), 'distill_call_ms_min': min(res['distill']),
           'ratio_distill_over_ce': med['distill'] / med['ce'], 'traffic_ratio': (2 * rd + wr) / (rd + wr),
           'ce_TBps': (rd + wr) / med['ce'] / 1e9, 'distill_TBps': (2 * rd + wr) / med['distill'] / 1e9,
           'note': 'call times by device events: two launches each (row kernel + finalize) and the launch gap; kernel times come from a kernel trace'}
    print(json.dumps(out))


def step(a):
    from pianobart_amd.model import BartConfig, PianoBart, PianoBartLM
    from tests.golden_util import load_vocab, synth_octuple_batch
    e2w, w2e = load_vocab()
    B, S = a.batch, a.seq

    def lm(layers):
        cfg = BartConfig(max_position_embeddings=S, d_model=768, encoder_layers=layers, decoder_layers=layers, encoder_ffn_dim=3072,
                         decoder_ffn_dim=3072, encoder_attention_heads=12, decoder_attention_heads=12)
        m = PianoBartLM(PianoBart(cfg, e2w, w2e, precision='bf16')).cuda()
        eng = m._get_engine()
        eng.bind(torch.device('cuda', 0))
        return m, eng

    (ms, student), (mt, teacher) = lm(6), lm(12)
    mt.eval()
    enc, dec, loss_mask, emask, dmask, target = [t.cuda() for t in synth_octuple_batch(B, S, seed=1234)]
    args = (ops.ids_to_i16(enc), ops.ids_to_i16(dec), ops.ids_to_i16(target), loss_mask.contiguous(), emask, dmask)

    class Plan:
        alpha, tau = 0.5, 2.0
    Plan.teacher = teacher

    def plain():
        student.loss_and_grads(*args, train=True, ids_checked=True)
        student.optimizer_step()

    def distilled():
        student.loss_and_grads(*args, train=True, ids_checked=True, distill=Plan)
        student.optimizer_step()

    fwd = lambda: teacher.teacher_logits(args[0], args[1], emask, dmask)
    for _ in range(a.warmup):
        plain(); distilled(); fwd()
    torch.cuda.synchronize()
    res = {'plain': [], 'distilled': [], 'teacher_forward': []}
    for _ in range(a.steps):
        res['plain'].append(_timed(plain, 1)[0]); res['distilled'].append(_timed(distilled, 1)[0]); res['teacher_forward'].append(_timed(fwd, 1)[0])
    student.finish_updates()
    med = {k + '_ms_median': sorted(v)[len(v) // 2] for k, v in res.items()}
    med.update(batch=B, seq=S, steps=a.steps, rows=student.last_rows,
               note='6-layer student (768 / 3072 / 12 heads) under the 12-layer benchmark model, bf16, packed rows; the teacher forward is dense (all B * S rows)')
    print(json.dumps(med))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=16384)
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--kernels-only', action='store_true', help='launch the kernels only (for a kernel trace): no event timing, no step')
    ap.add_argument('--step', action='store_true', help='also time the plain step, the distilled step and the teacher forward')
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--seq', type=int, default=1024)
    ap.add_argument('--steps', type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('distill_bench needs an MI355X: there is no CPU path')
    kernels(a)
    if a.step and not a.kernels_only:
        step(a)


if __name__ == '__main__':
    main()
