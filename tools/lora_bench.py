"""The LoRA kernels beside their yardsticks, and the adapter step beside the full step, in one process.

  python tools/lora_bench.py [--rows 32768] [--width 768] [--reps 20] [--step] [--out profiles/lora_kernel_stats.txt]

Kernels: pb_lora_down / pb_lora_up / pb_lora_wgrad at (rows, width, r = 16) and (rows, width, r = 64), bf16 and f32 activations, each
alternating with (a) pb_accum_f32 (dst = src) over a buffer of the bytes the kernel has to move -- the streaming yardstick: its rate in the
same process is the rate a bandwidth-bound kernel should reach -- and (b) ops.gemm on the same skinny shape in the storage dtype, which is
what one would use without these kernels (bf16 operands where the storage is bf16: a different precision, f32 accumulation). Times are call
times by device events after a warm-up; the median of --reps alternating repetitions is printed. Nothing is gated.
--step: the benchmark model (12 + 12 layers, d 768, ffn 3072, 12 heads) at B = 32, S = 1024, bf16, dropout on: the adapter step (default
targets, r = 16, heads training) against the full step of the same engine code, and torch.cuda.max_memory_allocated of each."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pianobart_amd import ops  # noqa: E402
from pianobart_amd._lib import PB_BF16, PB_F32  # noqa: E402


def _ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def _median(v):
    return sorted(v)[len(v) // 2]


def kernels(a, say):
    M, K = a.rows, a.width
    g = torch.Generator(device='cuda').manual_seed(0)
    for dt in (torch.bfloat16, torch.float32):
        esz = 2 if dt == torch.bfloat16 else 4
        code = PB_BF16 if dt == torch.bfloat16 else PB_F32
        X = torch.randn(M, K, generator=g, device='cuda').to(dt)
        Y = torch.zeros(M, K, device='cuda', dtype=dt)
        for r in (16, 64):
            A = torch.randn(r, K, generator=g, device='cuda') / K ** 0.5
            Bm = torch.randn(K, r, generator=g, device='cuda') * 0.01
            T = torch.empty(M, r, device='cuda')
            Gr = torch.empty(r, K, device='cuda')
            ws = ops.lora_wgrad_ws(M, r, K, 'cuda')
            Ad, Td, Cd = A.to(dt), torch.randn(M, r, generator=g, device='cuda').to(dt), torch.empty(M, r, device='cuda', dtype=dt)
            Gd = torch.empty(r, K, device='cuda')
            calls = {
                'down': (lambda: ops.lora_down(X, A, T, M, K), M * K * esz + M * r * 4,
                         lambda: ops.gemm(X, Ad, Cd, M=M, N=r, K=K, dtype=code)),
                'up': (lambda: ops.lora_up(Y, T, Bm, M, K, alpha=0.0, w_nr=True), 2 * M * K * esz + M * r * 4,
                       lambda: ops.gemm(Td, Bm.to(dt), Y, M=M, N=K, K=r, dtype=code, accum=True, alpha=0.0)),
                'wgrad': (lambda: ops.lora_wgrad(T, X, Gr, M, K, ws=ws), M * K * esz + M * r * 4 + 2 * ws.numel() * 4,
                          lambda: ops.gemm(Td, X, Gd, M=r, N=K, K=M, dtype=code, a_kc=False, b_kc=False, lda=r, ldb=K, ldc=K, c_f32=True)),
            }
            ops.lora_down(X, A, T, M, K)
            for name, (fn, nbytes, gemm) in calls.items():
                n = nbytes // 8 // 4 * 4                                  # accum (dst = src) reads n floats and writes n floats: 8 n bytes
                src, dst = torch.empty(n, device='cuda'), torch.empty(n, device='cuda')
                yard = lambda: ops.accum_f32(dst, src, add=False)
                try:
                    gemm()
                    gemm_ok = True
                except Exception as e:                                    # a shape the GEMM entry refuses: reported, not hidden
                    gemm_ok, why = False, str(e)[:80]
                for _ in range(3):
                    fn(); yard()
                torch.cuda.synchronize()
                t = {'k': [], 'y': [], 'g': []}
                for _ in range(a.reps):
                    t['k'].append(_ms(fn)); t['y'].append(_ms(yard))
                    if gemm_ok:
                        t['g'].append(_ms(gemm))
                k, y = _median(t['k']), _median(t['y'])
                say('%-6s %s r=%-2d (%d, %d): %8.1f us  %5.2f TB/s of %6.1f MB | pb_accum_f32 same bytes %8.1f us  %5.2f TB/s | ratio %.2f | ops.gemm %s'
                    % (name, str(dt)[6:], r, M, K, k * 1e3, nbytes / k / 1e9, nbytes / 1e6, y * 1e3, 8 * n / y / 1e9, k / y,
                       ('%8.1f us' % (_median(t['g']) * 1e3)) if gemm_ok else 'refused: ' + why))
                del src, dst


def step(a, say):
    from pianobart_amd.lora import LoraConfig
    from pianobart_amd.model import BartConfig, PianoBart, PianoBartLM
    from tests.golden_util import load_vocab, synth_octuple_batch
    e2w, w2e = load_vocab()
    B, S = a.batch, a.seq
    enc, dec, loss_mask, emask, dmask, target = [t.cuda() for t in synth_octuple_batch(B, S, seed=1234)]
    args = (ops.ids_to_i16(enc), ops.ids_to_i16(dec), ops.ids_to_i16(target), loss_mask.contiguous(), emask, dmask)
    out = {}
    for mode in ('full', 'lora'):
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        cfg = BartConfig(max_position_embeddings=S, d_model=768, encoder_layers=12, decoder_layers=12, encoder_ffn_dim=3072, decoder_ffn_dim=3072,
                         encoder_attention_heads=12, decoder_attention_heads=12)
        m = PianoBartLM(PianoBart(cfg, e2w, w2e, precision='bf16')).cuda().train()
        eng = m._get_engine()
        eng.bind(torch.device('cuda', 0))
        if mode == 'lora':
            eng.attach_lora(LoraConfig(rank=16, alpha=32), seed=0)

        def one():
            eng.loss_and_grads(*args, train=True, ids_checked=True)
            eng.optimizer_step()
        for _ in range(a.warmup):
            one()
        torch.cuda.synchronize()
        t = [_ms(one) for _ in range(a.steps)]
        out[mode] = (_median(t), min(t), torch.cuda.max_memory_allocated() / 2 ** 30)
        del m, eng
    for mode, (med, lo, gib) in out.items():
        say('%-4s step B=%d S=%d bf16 dropout on: median %7.2f ms  min %7.2f ms  max_memory_allocated %6.2f GiB' % (mode, B, S, med, lo, gib))
    say('adapter step / full step: %.3f' % (out['lora'][0] / out['full'][0]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=32768)
    ap.add_argument('--width', type=int, default=768)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--step', action='store_true')
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--seq', type=int, default=1024)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', type=str, default=None, help='also write the lines to this file (profiles/lora_kernel_stats.txt)')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('lora_bench needs an MI355X: there is no CPU path')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say('tools/lora_bench.py %s on %s' % (json.dumps(vars(a), sort_keys=True), torch.cuda.get_device_name(0)))
    kernels(a, say)
    if a.step:
        step(a, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
