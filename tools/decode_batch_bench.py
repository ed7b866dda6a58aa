"""Batched KV-cached generation throughput (Engine.generate_batch) at BASELINE configs[3]'s model: 12 layers, d 768, 12 heads, ffn 3072,
S = 1024, prompts with ~S/2 visible encoder rows, special ids made unsamplable as in bench.py's decode_bench (every row generates --steps
positions). Prints ONE JSON line: per B in --batches, aggregate tokens/s, ms per batched step, launches per step, rewinds, host
verification ms per step and an HBM-bytes estimate per step (decoder + LM-head weights once, plus each row's cross K/V over its visible
encoder rows and its self K/V cache at the mean position); plus the batch-1 Engine.generate rate measured in the same process.

    python tools/decode_batch_bench.py [--steps 256] [--batches 1 4 8 16] [--prime K] [--keep ATTR[,ATTR...]] [--bars N] [--ordered]
                                        [--key TONIC:MODE] [--pitch_range LO:HI] [--chords ROOT:QUALITY[,...]] [--accompany skyline|bass]

--keep pitch,velocity: forced tokens -- the named attributes of synthetic pieces are given at every position (generation.keep_mask) and the
model samples the others, at the largest B of --batches: ms per step and rewinds per row, beside the unforced run of the same process.

--ordered: time-ordered sampling -- the same prompts and seeds with and without the constraint (order = 0 for every row) at the largest B of
--batches, in this process: ms per step and rewinds per row for both, and at how many positions per row the unordered run goes back in
time (where a device sampler that did not know the constraint would be rewound).

--key C:major / --pitch_range 48:84: allowed classes -- every row of the plain --batches runs (and of the batch-1 run) carries the one allow
mask generation.allow_mask builds from the dictionary, so the step is timed with masked rows; the line then names the mask ("allow").
Compare with a run of the same command without the flags.

--chords C:maj,G:maj,A:min,F:maj [--bars_per_chord N] [--chord_start B]: a bar schedule -- every row of the plain --batches runs (and of the
batch-1 run) follows the chord progression bar by bar (generation.chord_schedule), so the step is timed with scheduled rows; the line then
names the schedule ("chords") and the rewinds per row. Compare with a run of the same command without the flags.

--accompany skyline|bass: anchored generation -- every row of the plain --batches runs (and of the batch-1 run) keeps that line of a
synthetic piece of its own (generation.anchor_rows, at most --steps / 2 anchors a row) and writes the notes around it, so the step is timed
with anchored rows; the line then names the anchors ("accompany"), the anchors placed and the rewinds per row. Compare with a run of the
same command without the flag.

--samples n: n samples of ONE prompt instead. Three runs alternate in this process, --reps times: "grouped" (samples=n: one encoder pass,
one (1, S, 2d) cross cache per layer, the grouped cross-attention kernel), "indirect" (the same with PB_DECODE_CROSS_GROUPED=0: the per-row
kernel reading the shared slice) and "repeated" (the prompt repeated n times through generate_batch without samples: the yardstick). Per
run: setup ms (encoder passes, cross K/V projections, prefill -- host time up to the decoder's start), ms per step, aggregate tokens/s over
the decode loop and over the whole call, cross_cache_bytes. One JSON line; with --prime K the runs are primed with K rows.

--refill [N]: refilled against chunked generation of --prompts (64) prompts whose lengths are fixed by a seeded table of given EOS rows,
uniform in --len_min .. --len_max (16 .. 256) positions, every other head free. "refill" (generate_batch(refill=N or True): one decoder, a
finished row's slot going to the next prompt) and "chunked" (refill=False: chunks of 16, each lasting until its longest row) alternate in
this process, --reps times. Per run: tokens/s of the whole call with the set-up included, steps, occupancy (row_steps / (steps * slots)),
setup_ms (summed over the chunks) and rewinds. One JSON line per run and a summary line, printed and appended to profiles/refill_b16.jsonl.

--bars N: what the stop at a bar buys. --prompts (64) synthetic pieces, each primed with its first S/4 .. S/2 rows, the bar attribute of the
rows behind the prime given (generation.keep_mask: a piece's own bars, a new one every ~17 rows) and the other heads sampled; row r stops at
generation.stop_after_bars(prime, N). Four runs alternate in this process, --reps times: "refill" and "chunked" with the stop, and
"nostop_refill" / "nostop_chunked" -- the same prompts decoded to the window's end without it and cut afterwards, which is what a caller had
to do before and the yardstick here. Per run: tokens/s of KEPT tokens over the whole call (kept = the positions of the stopped rows, the
same in all four runs), steps and occupancy. One JSON line per run and a summary line, printed and appended to profiles/bar_stop_b16.jsonl.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--seq', type=int, default=1024)
    ap.add_argument('--layers', type=int, default=12)
    ap.add_argument('--hs', type=int, default=768)
    ap.add_argument('--ffn', type=int, default=3072)
    ap.add_argument('--heads', type=int, default=12)
    ap.add_argument('--steps', type=int, default=256, help='generated positions per row')
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 4, 8, 16])
    ap.add_argument('--prime', type=int, default=0, help='also time primed generation: K decoder rows given per prompt, --steps sampled after them')
    ap.add_argument('--keep', type=str, default=None, help='also time forced generation at the largest batch: these attributes of synthetic pieces given, the others sampled')
    ap.add_argument('--samples', type=int, default=0, help='time n samples of one prompt: grouped / indirect / repeated-prompt runs, alternating')
    ap.add_argument('--reps', type=int, default=3, help='--samples: repetitions of the alternating runs')
    ap.add_argument('--kinds', nargs='+', default=['grouped', 'indirect', 'repeated'], choices=['grouped', 'indirect', 'repeated'],
                    help='--samples: the runs to alternate (one kind alone for a kernel trace)')
    ap.add_argument('--refill', type=int, nargs='?', const=0, default=None, metavar='N', help='time refilled against chunked generation (N slots; no N: 16)')
    ap.add_argument('--prompts', type=int, default=64, help='--refill: prompts of the call')
    ap.add_argument('--len_min', type=int, default=16, help='--refill: shortest row')
    ap.add_argument('--len_max', type=int, default=256, help='--refill: longest row')
    ap.add_argument('--log', type=str, default=os.path.join(ROOT, 'profiles', 'refill_b16.jsonl'), help='--refill: the file the lines are appended to')
    ap.add_argument('--bars', type=int, default=None, metavar='N', help='time bar-bounded generation (N new bars per primed row), refilled and chunked, '
                    'against the same prompts decoded without the stop and cut afterwards')
    ap.add_argument('--ordered', action='store_true', help='also time time-ordered generation at the largest batch, beside the unordered run of the same '
                    'prompts and seeds')
    ap.add_argument('--key', type=str, default=None, metavar='TONIC:MODE', help='the plain --batches runs with an allow mask on every row: melodic pitches of this key')
    ap.add_argument('--pitch_range', type=str, default=None, metavar='LO:HI', help='... melodic pitches LO <= k < HI')
    from pianobart_amd.generation import add_schedule_flags
    add_schedule_flags(ap)                      # --chords / --bars_per_chord / --chord_start: the plain --batches runs with a bar schedule on every row
    ap.add_argument('--accompany', type=str, default=None, choices=('skyline', 'bass'), help='the plain --batches runs with anchors on every row: that line of '
                    'a synthetic piece per row, at most --steps / 2 anchors')
    ap.add_argument('--sizes', type=int, nargs=8, default=None, metavar='N', help='the 8 head sizes of another dictionary (PianoBart.classes order), e.g. '
                    '1030 134 135 518 300 38 260 55: a head over 272 classes selects the wide device sampler. Plain --batches runs only')
    ap.add_argument('--bars_log', type=str, default=os.path.join(ROOT, 'profiles', 'bar_stop_b16.jsonl'), help='--bars: the file the lines are appended to')
    args = ap.parse_args(argv)

    import numpy as np
    import torch
    from pianobart_amd.model import BartConfig, PianoBart, PianoBartLM
    from tests.golden_util import load_vocab, synth_octuple_batch
    dev = torch.device('cuda', 0)
    e2w, w2e = load_vocab()
    sizes = [262, 134, 135, 262, 134, 38, 260, 55]
    if args.sizes is not None:
        if args.refill is not None or args.bars is not None or args.samples or args.prime or args.keep or args.ordered:
            raise SystemExit('--sizes times the plain --batches runs only')
        from tests.vocab_layout_util import make_dict, synth_batch
        sizes = list(args.sizes)
        e2w, w2e = make_dict(sizes)
    pads = [n - 6 for n in sizes]
    S, d, L, f = args.seq, args.hs, args.layers, args.ffn
    cfg = BartConfig(max_position_embeddings=S, d_model=d, encoder_layers=L, decoder_layers=L, encoder_ffn_dim=f, decoder_ffn_dim=f,
                     encoder_attention_heads=args.heads, decoder_attention_heads=args.heads, dropout=0.0)
    torch.manual_seed(0)
    model = PianoBartLM(PianoBart(cfg, e2w, w2e, precision='bf16')).to(dev).eval()
    with torch.no_grad():
        for i, p0 in enumerate(pads):
            model.mask_lm.proj[i].bias[p0:] = -30.0
    eng = model._get_engine()
    eng.bind(dev)
    sampler = dict(T=model.SAMPLE_T, P=model.SAMPLE_P)
    Bmax = max(args.batches) if args.refill is None and args.bars is None else args.prompts
    enc = (synth_octuple_batch(Bmax, S, seed=7, min_len=S // 2) if args.sizes is None else synth_batch(sizes, Bmax, S, seed=7, min_len=S // 2))[5].to(dev)     # S/2 .. S visible rows, as bench.py's decode prompt
    emask = (enc[:, :, 0] != pads[0]).float()
    steps = min(args.steps, S)
    vis = [int(v) for v in emask.sum(1).tolist()]

    # weight bytes a step streams once (bf16): per layer q|k|v, out, q_c, out_c, fc1, fc2; the LM head
    w_layer = (3 * d * d + d * d + d * d + d * d + 2 * d * f) * 2
    w_bytes = L * w_layer + sum(sizes) * d * 2

    def kv_bytes(rows):                                     # cross K/V over the visible rows + self K/V at the mean position
        return sum(L * (vis[b] + steps / 2) * 2 * d * 2 for b in range(rows))

    if args.bars is not None:
        from pianobart_amd.generation import keep_mask, stop_after_bars
        R, slots = args.prompts, args.refill or eng.BATCH_MAX
        piece = synth_octuple_batch(R, S + 1, seed=9, min_len=S + 1)[5][:, :S]       # ordinary rows all the way, bars non-decreasing
        ks = [int(v) for v in np.random.RandomState(17).randint(S // 4, S // 2 + 1, size=R)]
        forced = keep_mask(piece, 'bar', ks)                 # the bar of every position behind the prime is the piece's own
        stops = [stop_after_bars(piece[r, :ks[r]], args.bars, 256) for r in range(R)]
        penc = piece.clone().to(dev)
        for r in range(R):                                   # the encoder sees the prime only (Ablation.py:132-139)
            penc[r, ks[r]:] = torch.tensor(model.pianobart.pad_word_np, device=dev)
        pmask = (penc[:, :, 0] != 256).float()
        chunks = []
        chunk_fn = eng._generate_batch_chunk

        def counted(*a, **k):                               # last_decode holds the last chunk only: keep every chunk's
            y = chunk_fn(*a, **k)
            chunks.append(dict(eng.last_decode))
            return y
        eng._generate_batch_chunk = counted

        def cut(y):                                         # what a caller did before: decode on, then drop everything from the stop bar on
            y = y.clone()
            for r in range(len(y)):
                hit = (y[r, ks[r]:, 0] >= stops[r]).nonzero()
                if len(hit):
                    y[r, ks[r] + int(hit[0, 0]):] = torch.tensor(model.pianobart.pad_word_np)
            return y

        def run(kind, rows):
            rngs = [np.random.RandomState(b) for b in range(rows)]
            del chunks[:]
            refill = (args.refill or True) if kind.endswith('refill') else False
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            y = eng.generate_batch(penc[:rows], pmask[:rows], model.sample_row, rngs, sampler=sampler, prefix=piece[:rows], prefix_len=ks[:rows],
                                   forced=forced[:rows], refill=refill, stop=None if kind.startswith('nostop') else stops[:rows]).cpu()
            if kind.startswith('nostop'):
                y = cut(y)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            infos = list(chunks) if chunks else [dict(eng.last_decode)]
            kept = int(sum(int((y[r, ks[r]:, 0] != 256).sum()) for r in range(rows)))
            nsteps = sum(i['steps'] for i in infos)
            row_steps = sum(i.get('row_steps', sum(i['tokens'])) for i in infos)
            width = sum(i['steps'] * i['batch'] for i in infos)
            return y, dict(kind=kind, prompts=rows, bars=args.bars, slots=slots if refill else eng.BATCH_MAX, kept_tokens=kept, wall_ms=dt * 1e3,
                           kept_tokens_per_s=kept / dt, decoded_tokens=sum(sum(i['tokens']) for i in infos), steps=nsteps,
                           occupancy=row_steps / max(1, width), setup_ms=sum(i['setup_ms'] for i in infos), loop_ms=sum(i['loop_ms'] for i in infos),
                           rewinds=sum(sum(i['rewinds']) for i in infos), decoders=len(infos), admissions=infos[0].get('admissions', 0),
                           launches_per_step=infos[0]['launches_per_token'], graph=infos[0]['graph'])
        kinds = ('refill', 'chunked', 'nostop_refill', 'nostop_chunked')
        for kind in kinds[:2]:
            run(kind, min(R, 2 * slots))                    # warm-up (capture, pinned logs, allocator)
        lines, same = [], True
        for _ in range(args.reps):
            ys = {}
            for kind in kinds:
                ys[kind], r = run(kind, R)
                lines.append(r)
            same = same and all(bool(torch.equal(ys[k], ys['refill'])) for k in kinds)
        med = lambda kind, key: float(np.median([r[key] for r in lines if r['kind'] == kind]))
        summ = {kind: {key: med(kind, key) for key in ('kept_tokens_per_s', 'kept_tokens', 'decoded_tokens', 'steps', 'occupancy', 'wall_ms', 'rewinds')}
                for kind in kinds}
        lines.append(dict(kind='summary', metric='stop at a bar vs decode-and-cut (%dL/%dd, S=%d, %d prompts primed with S/4 .. S/2 rows, %d new bars)'
                          % (L, d, S, R, args.bars), same_tokens_in_all_runs=same, medians=summ,
                          speedup_refill=summ['refill']['kept_tokens_per_s'] / summ['nostop_refill']['kept_tokens_per_s'],
                          speedup_chunked=summ['chunked']['kept_tokens_per_s'] / summ['nostop_chunked']['kept_tokens_per_s']))
        eng._generate_batch_chunk = chunk_fn
        with open(args.bars_log, 'a') as fh:
            for ln in lines:
                print(json.dumps(ln), flush=True)
                fh.write(json.dumps(ln) + '\n')
        return

    if args.refill is not None:
        R, slots = args.prompts, args.refill or eng.BATCH_MAX
        eos = [p0 + 3 for p0 in (256, 128, 129, 256, 128, 32, 254, 49)]
        lens = np.random.RandomState(17).randint(args.len_min, min(args.len_max, S - 1) + 1, size=R)
        forced = np.full((R, S, 8), -1, dtype=np.int64)
        for r in range(R):
            forced[r, lens[r]] = eos                        # specials are unsamplable: row r decodes lens[r] positions and its EOS row
        chunks = []
        chunk_fn = eng._generate_batch_chunk

        def counted(*a, **k):                               # last_decode holds the last chunk only: keep every chunk's
            y = chunk_fn(*a, **k)
            chunks.append(dict(eng.last_decode))
            return y
        eng._generate_batch_chunk = counted

        def run(kind, rows):
            rngs = [np.random.RandomState(b) for b in range(rows)]
            del chunks[:]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            y = eng.generate_batch(enc[:rows], emask[:rows], model.sample_row, rngs, sampler=sampler, forced=forced[:rows],
                                   refill=(args.refill or True) if kind == 'refill' else False)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            infos = [dict(eng.last_decode)] if kind == 'refill' else list(chunks)
            ntok = sum(sum(i['tokens']) for i in infos)
            nsteps = sum(i['steps'] for i in infos)
            row_steps = sum(i.get('row_steps', sum(i['tokens'])) for i in infos)      # chunked: verified positions (equal without rewinds)
            width = sum(i['steps'] * i['batch'] for i in infos)
            return y.cpu(), dict(kind=kind, prompts=rows, slots=slots if kind == 'refill' else eng.BATCH_MAX, tokens=ntok, wall_ms=dt * 1e3,
                                 tokens_per_s=ntok / dt, steps=nsteps, occupancy=row_steps / max(1, width), setup_ms=sum(i['setup_ms'] for i in infos),
                                 loop_ms=sum(i['loop_ms'] for i in infos), rewinds=sum(sum(i['rewinds']) for i in infos),
                                 encoder_passes=sum(i['encoder_passes'] for i in infos), decoders=len(infos),
                                 admissions=infos[0].get('admissions', 0), launches_per_step=infos[0]['launches_per_token'], graph=infos[0]['graph'])
        for kind in ('refill', 'chunked'):
            run(kind, min(R, 2 * slots))                    # warm-up (capture, pinned logs, allocator)
        lines, same = [], True
        for _ in range(args.reps):
            ya, ra = run('refill', R)
            yb, rb = run('chunked', R)
            same = same and bool(torch.equal(ya, yb))
            lines += [ra, rb]
        med = lambda kind, key: float(np.median([r[key] for r in lines if r['kind'] == kind]))
        summ = {kind: {key: med(kind, key) for key in ('tokens_per_s', 'steps', 'occupancy', 'setup_ms', 'wall_ms', 'rewinds')} for kind in ('refill', 'chunked')}
        lines.append(dict(kind='summary', metric='refill vs chunked generate_batch (%dL/%dd, S=%d, %d prompts, rows of %d .. %d positions)'
                          % (L, d, S, R, args.len_min, args.len_max), same_tokens_in_all_runs=same, medians=summ,
                          speedup_tokens_per_s=summ['refill']['tokens_per_s'] / summ['chunked']['tokens_per_s']))
        eng._generate_batch_chunk = chunk_fn
        with open(args.log, 'a') as fh:
            for ln in lines:
                print(json.dumps(ln), flush=True)
                fh.write(json.dumps(ln) + '\n')
        return

    if args.samples:
        n = args.samples
        K = min(args.prime, S - steps) if args.prime else 0
        penc, pmask, piece = enc[:1], emask[:1], None
        if K:                                               # primed as below: the encoder sees the K given rows only
            piece = synth_octuple_batch(1, S + 1, seed=9, min_len=S + 1)[5][:, :K]
            penc = enc[:1].clone()
            penc[:, :K] = piece.to(dev)
            penc[:, K:] = torch.tensor(model.pianobart.pad_word_np, device=dev)
            pmask = (penc[:, :, 0] != 256).float()

        def run(kind, max_new):
            rngs = [np.random.RandomState(b) for b in range(n)]
            os.environ['PB_DECODE_CROSS_GROUPED'] = '0' if kind == 'indirect' else '1'
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if kind == 'repeated':
                y = eng.generate_batch(penc.repeat(n, 1, 1), pmask.repeat(n, 1), model.sample_row, rngs, max_new=max_new, sampler=sampler,
                                       prefix=piece.repeat(n, 1, 1) if K else None)
            else:
                y = eng.generate_batch(penc, pmask, model.sample_row, rngs, max_new=max_new, sampler=sampler, prefix=piece, samples=n)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            info = eng.last_decode
            ntok = sum(info['tokens'])
            return y.cpu(), dict(setup_ms=info['setup_ms'], prefill_ms=info['prefill_ms'], ms_per_step=info['loop_ms'] / max(1, info['steps']),
                                 loop_tokens_per_s=ntok / (info['loop_ms'] * 1e-3), tokens_per_s=ntok / dt, wall_ms=dt * 1e3, tokens=ntok,
                                 steps=info['steps'], rewinds=sum(info['rewinds']), cross_cache_bytes=info['cross_cache_bytes'],
                                 encoder_passes=info['encoder_passes'], prefill_passes=info['prefill_passes'],
                                 launches_per_step=info['launches_per_token'], graph=info['graph'], batch=info['batch'])
        kinds = tuple(args.kinds)
        for kind in kinds:
            run(kind, 16)                                   # warm-up (capture, pinned logs, allocator)
        reps = {k: [] for k in kinds}
        same = True
        for _ in range(args.reps):
            ys = {}
            for kind in kinds:
                ys[kind], r = run(kind, steps)
                reps[kind].append(r)
            same = same and all(torch.equal(ys[k], ys[kinds[-1]]) for k in kinds)
        summ = {}
        for kind in kinds:
            tps = [r['loop_tokens_per_s'] for r in reps[kind]]
            summ[kind] = dict(loop_tokens_per_s_median=float(np.median(tps)), loop_tokens_per_s_min=min(tps), loop_tokens_per_s_max=max(tps),
                              ms_per_step_median=float(np.median([r['ms_per_step'] for r in reps[kind]])),
                              setup_ms_median=float(np.median([r['setup_ms'] for r in reps[kind]])),
                              tokens_per_s_median=float(np.median([r['tokens_per_s'] for r in reps[kind]])),
                              cross_cache_bytes=reps[kind][0]['cross_cache_bytes'])
        print(json.dumps({"metric": "n samples of one prompt (%dL/%dd, S=%d, %d positions per row, %d prefix rows)" % (L, d, S, steps, K),
                          "samples": n, "prefix_rows": K, "same_tokens_in_all_runs": bool(same), "summary": summ, "runs": reps,
                          "group_tile": os.environ.get('PB_DECODE_GROUP_TILE', 'default')}), flush=True)
        return

    from pianobart_amd.generation import allow_from_args
    amask = allow_from_args(args, e2w)          # --key / --pitch_range: one allow mask for every row of the plain runs (None: free rows)
    allow_of = lambda B: [amask] * B if amask is not None else None
    from pianobart_amd.generation import schedule_from_args
    bar = schedule_from_args(args, e2w)         # --chords: one bar schedule for every row of the plain runs (None: no schedule)
    lines = None                                # --accompany: one anchor list per row of the plain runs (None: no anchors)
    if args.accompany is not None:
        from pianobart_amd.generation import anchor_rows
        pieces = (synth_octuple_batch(Bmax, S, seed=13, min_len=S) if args.sizes is None else synth_batch(sizes, Bmax, S, seed=13, min_len=S))[5].numpy()
        lines = [anchor_rows(p, args.accompany, e2w)[:max(1, steps // 2)] for p in pieces]
    bar_of = lambda B, n=steps: dict(**(dict(bar_allow=[bar] * B) if bar is not None else {}),
                                     **(dict(anchors=[a[:max(1, n // 2)] for a in lines[:B]]) if lines is not None else {}))
    # batch 1 through Engine.generate (the device-sampled batch-1 decoder), same process
    np.random.seed(0)
    eng.generate(enc[:1], emask[:1], model.sample_row, max_new=16, sampler=sampler, allow=amask, **bar_of(1, 16))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.generate(enc[:1], emask[:1], model.sample_row, max_new=steps, sampler=sampler, allow=amask, **bar_of(1))
    torch.cuda.synchronize()
    b1 = steps / (time.perf_counter() - t0)
    b1_info = dict(eng.last_decode)

    res = {}
    for B in args.batches:
        rngs = [np.random.RandomState(b) for b in range(B)]
        eng.generate_batch(enc[:B], emask[:B], model.sample_row, rngs, max_new=16, sampler=sampler, allow=allow_of(B), **bar_of(B, 16))     # warm-up (capture, pinned logs)
        torch.cuda.synchronize()
        rngs = [np.random.RandomState(b) for b in range(B)]
        t0 = time.perf_counter()
        eng.generate_batch(enc[:B], emask[:B], model.sample_row, rngs, max_new=steps, sampler=sampler, allow=allow_of(B), **bar_of(B))
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        info = eng.last_decode
        ntok = sum(info['tokens'])
        res[str(B)] = dict(tokens_per_s=ntok / dt, ms_per_step=info['loop_ms'] / max(1, info['steps']), wall_ms=dt * 1e3,
                           loop_ms=info['loop_ms'], launches_per_step=info['launches_per_token'], graph=info['graph'],
                           rewinds=sum(info['rewinds']), host_ms_per_step=info['host_ms'] / max(1, info['steps']), steps=info['steps'],
                           tokens=ntok, hbm_bytes_per_step=w_bytes + kv_bytes(B))
        if bar is not None or lines is not None:
            res[str(B)]['rewinds_per_row'] = [int(v) for v in info['rewinds']]
        if lines is not None:
            res[str(B)]['anchors_placed'] = [int(v) for v in info['anchors_placed']]
    best = max(res.values(), key=lambda r: r['tokens_per_s'])['tokens_per_s']
    out = {"metric": "batched generate tokens/s (KV-cached decode, %dL/%dd, S=%d, %d positions per row)" % (L, d, S, steps),
           "batch1_generate_tokens_per_s": b1, "batch1_info": b1_info, "by_batch": res,
           "speedup_best_vs_batch1": best / b1, "visible_encoder_rows": vis[:Bmax]}
    if amask is not None:
        out['allow'] = dict(key=args.key, pitch_range=args.pitch_range, allowed_columns=int(amask.sum()), vocab=int(amask.size))
    if bar is not None:
        out['chords'] = dict(chords=args.chords, bars_per_chord=args.bars_per_chord, chord_start=args.chord_start, scheduled=bool(b1_info.get('scheduled')))
    if lines is not None:
        out['accompany'] = dict(which=args.accompany, anchors_per_row=[len(a[:max(1, steps // 2)]) for a in lines[:max(args.batches)]])
    if args.prime:
        # primed generation: the first K rows of each prompt's own piece given to the decoder, the encoder sees those rows only
        # (Ablation.py:132-139); --steps positions sampled after them. prefill_ms = the teacher-forced decoder pass that fills the
        # self-attention caches, per prompt (device time)
        K = min(args.prime, S - steps)
        piece = synth_octuple_batch(Bmax, S + 1, seed=9, min_len=S + 1)[5][:, :K]
        penc = enc.clone()
        penc[:, :K] = piece.to(dev)
        penc[:, K:] = torch.tensor(model.pianobart.pad_word_np, device=dev)
        pmask = (penc[:, :, 0] != 256).float()
        primed = {}
        for B in sorted(set([1] + [b for b in args.batches if b in (1, 16)])):
            rngs = [np.random.RandomState(b) for b in range(B)]
            eng.generate_batch(penc[:B], pmask[:B], model.sample_row, rngs, max_new=16, sampler=sampler, prefix=piece[:B])   # warm-up
            torch.cuda.synchronize()
            rngs = [np.random.RandomState(b) for b in range(B)]
            t0 = time.perf_counter()
            eng.generate_batch(penc[:B], pmask[:B], model.sample_row, rngs, max_new=steps, sampler=sampler, prefix=piece[:B])
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            info = eng.last_decode
            ntok = sum(info['tokens'])
            primed[str(B)] = dict(prefill_ms_per_prompt=info['prefill_ms'] / B, continuation_tokens_per_s=ntok / (info['loop_ms'] * 1e-3),
                                  tokens_per_s_incl_encoder_and_prefill=ntok / dt, wall_ms=dt * 1e3, loop_ms=info['loop_ms'], tokens=ntok,
                                  rewinds=sum(info['rewinds']))
            if str(B) in res:
                primed[str(B)]['unprimed_loop_tokens_per_s'] = res[str(B)]['tokens'] / (res[str(B)]['loop_ms'] * 1e-3)
        out['primed'] = dict(prefix_rows=K, by_batch=primed)
    if args.keep:
        # forced tokens: the kept attributes of each row's synthetic piece (ordinary events only) are given at every position, the other
        # heads are sampled; same launches per step, and a given head cannot disagree with the host
        from pianobart_amd.generation import keep_mask
        B = Bmax
        forced = keep_mask(synth_octuple_batch(B, S + 1, seed=11, min_len=S + 1)[5][:, :S], args.keep)
        by = {}
        for tag, tab in (('unforced', None), ('forced', forced)):
            rngs = [np.random.RandomState(b) for b in range(B)]
            eng.generate_batch(enc[:B], emask[:B], model.sample_row, rngs, max_new=16, sampler=sampler, forced=tab)     # warm-up (capture)
            torch.cuda.synchronize()
            rngs = [np.random.RandomState(b) for b in range(B)]
            eng.generate_batch(enc[:B], emask[:B], model.sample_row, rngs, max_new=steps, sampler=sampler, forced=tab)
            torch.cuda.synchronize()
            info = eng.last_decode
            by[tag] = dict(ms_per_step=info['loop_ms'] / max(1, info['steps']), rewinds_per_row=sum(info['rewinds']) / B, steps=info['steps'],
                           tokens=sum(info['tokens']), launches_per_step=info['launches_per_token'], graph=info['graph'],
                           host_ms_per_step=info['host_ms'] / max(1, info['steps']))
        out['forced'] = dict(keep=args.keep, batch=B, **by)
    if args.ordered:
        # time-ordered sampling: every row with floor 0; same launches per step, the sampler masks heads 0 and 1 on the device
        from pianobart_amd.generation import is_time_ordered
        B = Bmax
        by, ys = {}, {}
        for tag, order in (('unordered', None), ('ordered', [0] * B)):
            rngs = [np.random.RandomState(b) for b in range(B)]
            eng.generate_batch(enc[:B], emask[:B], model.sample_row, rngs, max_new=16, sampler=sampler, order=order)     # warm-up (capture)
            torch.cuda.synchronize()
            rngs = [np.random.RandomState(b) for b in range(B)]
            ys[tag] = eng.generate_batch(enc[:B], emask[:B], model.sample_row, rngs, max_new=steps, sampler=sampler, order=order).cpu().numpy()
            torch.cuda.synchronize()
            info = eng.last_decode
            by[tag] = dict(ms_per_step=info['loop_ms'] / max(1, info['steps']), rewinds_per_row=sum(info['rewinds']) / B, steps=info['steps'],
                           tokens=sum(info['tokens']), launches_per_step=info['launches_per_token'], graph=info['graph'],
                           host_ms_per_step=info['host_ms'] / max(1, info['steps']),
                           rows_in_time_order=sum(bool(is_time_ordered(ys[tag][b])) for b in range(B)))
        t = ys['unordered'][:, :steps, 0].astype(np.int64) * 1024 + ys['unordered'][:, :steps, 1].astype(np.int64)
        out['ordered'] = dict(batch=B, positions_going_back_per_row_unordered=float((np.diff(t, axis=1) < 0).sum() / B), **by)
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
