"""Checkpoint merging at the size of the BASELINE configs[1] backbone (12L / 768d / ffn 3072 / 12 heads, S = 1024) with N = 4 models:
ms per kernel family, GB/s on the bytes each family moves, the whole merge_flat call of each method, and pb_accum_f32 on the same n in
the same process as the yardstick of a streaming kernel on the machine.

    python tools/merge_bench.py [--models 4] [--out profiles/merge_kernel_stats.txt]
    python tools/merge_bench.py --fisher [--models 4] [--out profiles/fisher_kernel_stats.txt]     the Fisher merging passes instead
    python tools/merge_bench.py --regmean [--models 4] [--out profiles/regmean_kernel_stats.txt]   the RegMean kernels and merge instead

Each timed call runs once after one warm-up call of the same shape, between device events. Bytes are counted from the shapes:
accum 12 n; one k-th call 4 passes x 8 n (x and base); tally (N + 1) 4 n; apply (N + 1) 4 n + 4 n. Nothing is asserted."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def backbone_segments(seq):
    """The segment table of the configs[1] backbone, from a model built without storage."""
    from pianobart_amd.merge import segment_table
    from pianobart_amd.model import BartConfig, PianoBart
    from tests.golden_util import load_vocab
    e2w, w2e = load_vocab()
    cfg = BartConfig(max_position_embeddings=seq, d_model=768, encoder_layers=12, decoder_layers=12, encoder_ffn_dim=3072, decoder_ffn_dim=3072,
                     encoder_attention_heads=12, decoder_attention_heads=12)
    m = PianoBart(cfg, e2w, w2e)
    return segment_table({n: tuple(p.shape) for n, p in m.named_parameters()})


def regmean_groups_of(segs):
    """{key: [names]} of the backbone's Linear weights as the Gram pass shares their inputs: q / k / v of a self-attention block, every
    decoder layer's cross-attention k / v; encoder_linear has none."""
    groups = {}
    for s in segs:
        if not s.name.endswith('.weight') or len(s.shape) != 2 or '.layers.' not in s.name or 'layer_norm' in s.name:
            continue
        block, leaf = s.name.rsplit('.', 2)[:2]
        key = block + '.qkv' if leaf in ('q_proj', 'k_proj', 'v_proj') and block.endswith('self_attn') else 'cross.kv' if leaf in ('k_proj', 'v_proj') else s.name
        groups.setdefault(key, []).append(s.name)
    return groups


def regmean_mode(args, dev, segs, pre, models, say, row, timed):
    """pb_gram_accum beside the TN ops.gemm on the same X, factor + solve, and one whole merge_flat."""
    from pianobart_amd import ops, _lib
    from pianobart_amd.merge import MergePlan, merge_flat
    g = torch.Generator(device=dev).manual_seed(4321)
    T = 8192
    for K in (768, 3072):
        for dt, code in ((torch.bfloat16, _lib.PB_BF16), (torch.float32, _lib.PB_F32)):
            X = (torch.randn(T, K, device=dev, generator=g) + 0.5).to(dt)
            G, C, ws = torch.zeros(K, K, device=dev), torch.zeros(K, K, device=dev), ops.gram_ws(T, K, dev)
            flop = 2.0 * T * K * K
            ms = timed(lambda: ops.gram_accum(G, X, ws))
            say('%-46s %9.3f ms   %8.1f TFLOP/s of the %.1f GFLOP of the full product' % ('pb_gram_accum (%d, %d) %s' % (T, K, str(dt)[6:]), ms, flop / ms / 1e9, flop / 1e9))
            ms = timed(lambda: ops.gemm(X, X, C, M=K, N=K, K=T, dtype=code, a_kc=False, b_kc=False, c_f32=True, accum=True))
            say('%-46s %9.3f ms   %8.1f TFLOP/s' % ('ops.gemm TN, same X, both triangles', ms, flop / ms / 1e9))
    info = torch.zeros(1, dtype=torch.int32, device=dev)
    for K, nrhs in ((768, 2304), (3072, 768)):
        X = torch.randn(2 * K, K, device=dev, generator=g) + 0.5
        S0 = torch.zeros(K, K, device=dev)
        ops.gram_accum(S0, X)
        S0 /= 2 * K
        R0 = torch.randn(K, nrhs, device=dev, generator=g)
        S, R = S0.clone(), R0.clone()

        def factor():
            S.copy_(S0)
            ops.chol_factor(S, info)

        row('pb_chol_factor K = %d (with the copy of S)' % K, timed(factor))
        row('pb_chol_solve K = %d, nrhs = %d' % (K, nrhs), timed(lambda: ops.chol_solve(S, R)))
    assert int(info.item()) == 0
    groups, N = regmean_groups_of(segs), len(models)
    shape = {s.name: s.shape for s in segs}
    base = {}
    for K in (768, 3072):                                  # one Gram matrix per K and model, copied per group (a shared tensor would be ONE group)
        for m in range(N):
            X = (torch.randn(2 * K, K, device=dev, generator=g) + 0.5).bfloat16()
            base[(K, m)] = torch.zeros(K, K, device=dev)
            ops.gram_accum(base[(K, m)], X)
            base[(K, m)] /= 2 * K
    regmean = [dict() for _ in range(N)]
    for names in groups.values():
        for m in range(N):
            G = base[(shape[names[0]][1], m)].clone()
            for name in names:
                regmean[m][name] = G
    plan = MergePlan(N, method='regmean_merging', regmean_weights=[{}] * N)
    say('%d weights in %d groups (one factorisation each)' % (sum(len(v) for v in groups.values()), len(groups)))
    row('merge_flat: regmean_merging', timed(lambda: merge_flat(plan, pre, models, segs, regmean=regmean)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--models', type=int, default=4)
    ap.add_argument('--seq', type=int, default=1024)
    ap.add_argument('--out', default='')
    ap.add_argument('--fisher', action='store_true', help='time the Fisher merging passes (pb_fisher.hip) against the yardstick instead')
    ap.add_argument('--regmean', action='store_true', help='time the RegMean kernels (pb_regmean.hip) and a whole regmean merge_flat instead')
    args = ap.parse_args()
    from pianobart_amd import ops, _lib
    from pianobart_amd.merge import MergePlan, drop_threshold, merge_flat, rescale_divisor
    if not torch.cuda.is_available():
        raise SystemExit('merge_bench needs a GPU: nothing is measured without one')
    dev = torch.device('cuda', 0)
    segs = backbone_segments(args.seq)
    n, N = segs[-1].offset + segs[-1].numel, args.models
    g = torch.Generator(device=dev).manual_seed(1234)
    pre = torch.randn(n, device=dev, generator=g) * 0.02
    models = [pre + torch.randn(n, device=dev, generator=g) * 0.002 * (m + 1) for m in range(N)]
    out = torch.empty_like(pre)
    flags0 = torch.zeros(1, dtype=torch.int32, device=dev)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def timed(fn):
        fn()                                                   # warm-up of the same shape
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def row(name, ms, nbytes=None):
        say('%-46s %9.3f ms%s' % (name, ms, '' if nbytes is None else '   %8.1f GB/s over %6.2f GB' % (nbytes / ms / 1e6, nbytes / 1e9)))

    say('checkpoint merging, %s, n = %d parameters (%d tensors), N = %d models' % (torch.cuda.get_device_name(0), n, len(segs), N))
    row('pb_accum_f32 add (yardstick)', timed(lambda: ops.accum_f32(out, pre, add=True)), 12.0 * n)
    if args.regmean:
        regmean_mode(args, dev, segs, pre, models, say, row, timed)
        if args.out:
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')
        return
    if args.fisher:
        # the four Fisher passes on the same n: accumulate 12 n bytes (F read and written, g read), finish 8 n, norm 4 n, the fused pass
        # (2 N + 1) 4 n (N weight vectors and N Fisher vectors read, one written)
        fishers = [(torch.randn(n, device=dev, generator=g) * 1e-3) ** 2 * (m + 1) for m in range(N)]
        F = torch.zeros_like(pre)
        row('pb_fisher_accum', timed(lambda: ops.fisher_accum(F, models[0])), 12.0 * n)
        row('pb_fisher_finish', timed(lambda: ops.fisher_finish(F, 256, flags0)), 8.0 * n)
        nws, norm = ops.fisher_norm_ws(dev), torch.zeros(1, device=dev)
        row('pb_fisher_norm', timed(lambda: ops.fisher_norm(fishers[0], nws, norm)), 4.0 * n)
        desc = ops.fisher_desc(models, fishers, out, [1.0 / N] * N, 1e-6)
        row('pb_fisher_merge', timed(lambda: ops.fisher_merge(desc)), (2 * N + 1) * 4.0 * n)
        plan = MergePlan(N, method='fisher_merging', fisher_weights=[{}] * N)
        row('merge_flat: fisher_merging (N norms + fused pass)', timed(lambda: merge_flat(plan, pre, models, segs, fishers)))
        if args.out:
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')
        return
    ws, flags, thr = ops.merge_kth_ws(dev), torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(N, device=dev)
    k = int(n * 0.8)
    row('pb_merge_kth_abs, whole vector, k = 0.8 n', timed(lambda: ops.merge_kth_abs(models[0], pre, k, thr[0:1], flags, ws)), 4 * 8.0 * n)
    for m in range(1, N):
        ops.merge_kth_abs(models[m], pre, k, thr[m:m + 1], flags, ws)
    tally = torch.zeros(2, dtype=torch.int64, device=dev)
    th = [thr[m:m + 1] for m in range(N)]
    d = ops.merge_desc(pre, models, out, method=_lib.MERGE_TIES, lam=1.0, thresh=th, tally=tally)
    row('pb_merge_sign_tally', timed(lambda: ops.merge_sign_tally(d)), (N + 1) * 4.0 * n)
    rates = [0.8] * N
    common = dict(drop_thresh=[drop_threshold(r) for r in rates], rescale=[rescale_divisor(r, True) for r in rates], seed=7)
    for name, desc in (('average', ops.merge_desc(pre, models, out, method=_lib.MERGE_AVERAGE)),
                       ('task arithmetic', ops.merge_desc(pre, models, out, method=_lib.MERGE_TASK, lam=0.7)),
                       ('ties', d),
                       ('average, random masks', ops.merge_desc(pre, models, out, method=_lib.MERGE_AVERAGE, kinds=[_lib.MERGE_MASK_RANDOM] * N, **common)),
                       ('average, magnitude masks', ops.merge_desc(pre, models, out, method=_lib.MERGE_AVERAGE, kinds=[_lib.MERGE_MASK_MAGNITUDE] * N, thresh=th, **common))):
        row('pb_merge_apply: ' + name, timed(lambda: ops.merge_apply(desc)), (N + 2) * 4.0 * n)
    for name, kw in (('average_merging', dict(method='average_merging')), ('task_arithmetic', dict(method='task_arithmetic', scaling_coefficient=0.7)),
                     ('ties_merging', dict(method='ties_merging')), ('mask_merging random / average', dict(method='mask_merging')),
                     ('mask_merging magnitude / average (per tensor)', dict(method='mask_merging', mask_strategy='magnitude')),
                     ('mask_merging random / ties', dict(method='mask_merging', mask_apply_method='ties_merging'))):
        plan = MergePlan(N, **kw)
        row('merge_flat: ' + name, timed(lambda: merge_flat(plan, pre, models, segs)))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
