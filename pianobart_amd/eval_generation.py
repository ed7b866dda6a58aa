"""Generate a whole test set into one .npy: the reference's eval_generation.py on the HIP path (python -m pianobart_amd.eval_generation).

Same flags as the reference (--dict_file --ckpt --dataset_path --dataset_name --output --num_workers --batch_size --max_seq_len --hs
--layers --ffn_dims --heads --nopretrain --cpu --cuda_devices) plus --precision and --seed, and the same order of work as demo.py:
vocabulary, model from the flags, checkpoint through checkpoint_state_dict with strict=False, encoder mask = bar column != PAD,
generation, one device. The output is float32 (N, max_seq_len, 8), one row per prompt, PAD after each prompt's stop.

RNG rules:
  * without --seed: --batch_size 1 is the reference's loop, every prompt drawing from the one global np.random stream in turn
    (PianoBartLM.forward(generate=True)); --batch_size > 1 is refused (the reference's model exits with ERROR for B != 1).
  * with --seed s: prompt i draws from its own RandomState(s + i) (PianoBartLM.generate_batch: up to 16 prompts per batched decode
    step), so the file is identical for every --batch_size.
  * --samples n (default 1) asks for n continuations of every prompt. n = 1 writes the (N, max_seq_len, 8) file above, byte for byte.
    n > 1 needs --seed and writes (N, n, max_seq_len, 8): sample j of prompt i draws from RandomState(seed + j N + i) (sample_seed), so
    [:, 0] is the --samples 1 file. --batch_size then counts output rows; the samples of a prompt inside one batch share its encoder
    pass and cross-attention K/V (PianoBartLM.generate_batch's samples_per_prompt), and the file does not depend on --batch_size.
  * --refill [N] (needs --seed, not with --samples > 1): all prompts go to ONE generate_batch call with refill = N (no N: 16 slots): one
    decoder whose rows are handed to the next prompt as they stop. --batch_size then only sets the score batches. The generation file
    is byte-identical to the run without the flag.
The prompts are sliced from the loaded array in order; --num_workers is accepted for the reference's command lines and not needed.

Kept attributes (--keep ATTR[,ATTR...], needs --prime): the named attributes (bar, position, instrument, pitch, duration, velocity, timesig,
tempo) of the dataset piece's own rows behind the prime, up to and including its EOS row, are given to the generation and the model samples
the other attributes (generation.keep_mask with start = k_b -> PianoBartLM.generate_batch's decoder_forced). The generation file has the
shape and dtype it has without the flag, and without the flag it is byte-identical. --score still scores all 8 heads of a position.

Bar-bounded generation (--bars N): every row also stops at a bar -- generation.stop_after_bars of its prime (q = the bar of the prime's last
row, -1 without --prime; the stop bar is min(q + 1 + N, the bar PAD id), 256 in the default dictionary), so the row finishes the bar it is in and writes N whole new bars
(PianoBartLM.generate_batch's decoder_stop). Works with and without --prime and with --keep, --samples, --refill, --score and --pick.

Infilling (--infill LO:HI [--infill_mode rows|span], needs --seed): bars LO .. HI-1 of every piece are rewritten and the rest is left alone.
Per piece generation.infill_plan gives the prime (the rows with bar < LO), the stop bar HI, the encoder input (rows: every row of the region
replaced by the MASK row, TokenMask's convention; span: the region replaced by one MASK row, TokenInfilling's) and the suffix (the rows with
bar >= HI and the EOS row); the generated row is spliced with the suffix (generation.infill_splice) and the output file holds the spliced
pieces, cut at max_seq_len (the number of truncated pieces is printed). The flag sets the prime, the kept attributes and the stop itself, so
it excludes --prime, --keep, --bars and --score_dataset; it combines with --samples, --refill, --score and --pick. --score scores the
generated row before the splice, with start = the prime length, as a primed row is scored.

Time-ordered sampling (--ordered): no sampled (bar, position) goes back in time (PianoBartLM.generate_batch's decoder_order; DESIGN.md
section 1, "Time-ordered sampling"). The bar floor is 0 with --prime, --bars or neither, and LO with --infill LO:HI, so no new row of an
infilled region sounds in front of it; the tool then checks generation.is_time_ordered on every spliced piece from its prime on and raises
PBError where it fails. Combines with --samples, --refill, --keep (a kept bar or position is given, never reordered), --score and --pick; not
with --score_dataset. Without the flag the output files are byte-identical to a run of a version without it.

Allowed classes (--key C:major, --pitch_range LO:HI, --instruments 0,1, --tempo LO:HI, --max_duration N, --velocity LO:HI): what a free head
may sample is restricted to the named classes (PianoBartLM.generate_batch's decoder_allow; DESIGN.md section 1, "Allowed classes"). One
mask, built by generation.allow_mask from the model's own dictionary, is used for every row; the flags of one head intersect. The tool
checks generation.is_allowed on every output row behind its prime (kept attributes are given, not tested) and raises PBError where it
fails. Combines with --prime, --keep, --bars, --infill, --ordered, --samples, --refill, --score and --pick; not with --score_dataset. Without
the flags the output files are byte-identical to a run of a version without them.

Bar schedules (--chords C:maj,G:maj,A:min,F:maj [--bars_per_chord N] [--chord_start B]): the pitches a free head may sample change with the
bar -- bar B takes the tones of the first chord, bar B + N those of the second, .., the progression repeated to the end of the piece
(PianoBartLM.generate_batch's decoder_bar_allow; generation.chord_schedule; DESIGN.md section 1, "Bar schedules"). B defaults to 0, and
with --prime to the bar after the one each piece's prime ends in, so every piece gets its own schedule. The tool checks
generation.follows_schedule on every output row behind its prime and raises PBError where it fails. Combines with the allow flags (the
masks intersect) and everything they combine with; not with --score_dataset. Without the flags the output files are byte-identical to a
run of a version without them.

Anchored generation (--prime N|half --accompany skyline|bass): of each piece's own rows behind the prime, the highest (skyline) or lowest
(bass) melodic note of every (bar, position) is kept where it falls in time and the model writes the notes around them
(generation.anchor_rows -> PianoBartLM.generate_batch's decoder_anchors; DESIGN.md section 1, "Anchored notes"). --ordered is implied; the
row stops at the bar after its last anchor unless --bars is given. The tool checks generation.follows_anchors on every output row behind
its prime and raises PBError where it fails. Combines with --bars, the allow flags, --chords, --samples, --refill, --score and --pick; not
with --keep, --infill or --score_dataset. Without the flag the output files are byte-identical to a run of a version without it.

Scoring (PianoBartLM.score: one teacher-forced pass per generate call, after it; the generation file is byte-identical with and without):
  * --score writes a second float32 file, (N, 9) or (N, n, 9) with --samples n: per output row the 8 per-head sums of the log-probability
    of its sampled events (start = the prime length under --prime, so forced rows are not scored) and the number of scored positions.
    The encoder input and mask are the ones the generation saw. Path: --score_output, default --output with .npy -> _score.npy.
  * --pick best (needs --score): of each prompt's n samples only the one with the largest sum_heads(sum_logp) / count is written,
    (N, max_seq_len, 8); rows without a scored position rank last, ties go to the lower sample index (scoring.pick_best). The score
    file keeps all n samples.
  * --score_dataset (needs --prime, no --samples): no generation -- the dataset rows themselves are the targets, the encoder sees the primed
    split (prime_inputs), start = k_b, length = the rows before the first bar PAD. Writes the score file only and prints the per-head mean
    log-probability and top-1 hit rate over the scored positions.
"""
import argparse
import os

import numpy as np
import torch

from ._lib import PBError
from .generation import add_anchor_flags, anchors_from_args, check_anchor_flags, follows_anchors, add_allow_flags, add_schedule_flags, follows_schedule, schedule_from_args, allow_flags_given, allow_from_args, check_refill, infill_plan, is_allowed, infill_splice, is_time_ordered, keep_mask, parse_keep, sample_seed, stop_after_bars
from .scoring import pick_best
from .model import BartConfig, PianoBart, PianoBartLM, checkpoint_state_dict

_HERE = os.path.dirname(os.path.abspath(__file__))
_VOCAB = os.path.join(_HERE, 'data', 'octuple_vocab.json')


def get_args(argv=None):
    ap = argparse.ArgumentParser(description='')
    ap.add_argument('--dict_file', type=str, default=_VOCAB)
    ap.add_argument('--ckpt', type=str, default='result/pretrain/pianobart/model_best.ckpt')
    ap.add_argument('--dataset_path', type=str, default='./Data/output_generate/GiantMIDI1k/gen_method')
    ap.add_argument('--dataset_name', type=str, default='GiantMIDI1k_test.npy')
    ap.add_argument('--output', type=str, default='./output.npy')
    ap.add_argument('--num_workers', type=int, default=5)
    ap.add_argument('--batch_size', type=int, default=1)
    ap.add_argument('--max_seq_len', type=int, default=1024, help='all sequences are padded to `max_seq_len`')
    ap.add_argument('--hs', type=int, default=1024)
    ap.add_argument('--layers', type=int, default=8)
    ap.add_argument('--ffn_dims', type=int, default=2048)
    ap.add_argument('--heads', type=int, default=8)
    ap.add_argument('--nopretrain', action='store_true', default=False)
    ap.add_argument('--cpu', action='store_true')
    ap.add_argument('--cuda_devices', type=int, nargs='+', default=[0], help='HIP device id (one)')
    ap.add_argument('--precision', default='bf16', choices=['bf16', 'fp32', 'bf16x3'])
    ap.add_argument('--seed', type=int, default=None, help='prompt i samples from RandomState(seed + i): the output is the same for every --batch_size')
    ap.add_argument('--prime', type=str, default=None, help='N or "half": continue each piece from its first k = min(N, L) (half: L // 2) rows, '
                    'L = rows whose bar id is not PAD (Ablation.py:134); the encoder sees rows < k only')
    ap.add_argument('--samples', type=int, default=1, help='continuations per prompt; n > 1 needs --seed and writes (N, n, max_seq_len, 8), '
                    'sample j of prompt i drawing from RandomState(seed + j * N + i)')
    ap.add_argument('--keep', type=str, default=None, help='ATTR[,ATTR...] of bar, position, instrument, pitch, duration, velocity, timesig, tempo (needs '
                    '--prime): these attributes of the piece\'s own rows behind the prime are kept and the model samples the others')
    ap.add_argument('--refill', type=int, nargs='?', const=0, default=None, metavar='N', help='one batched decoder of N slots (no N: 16) for the whole '
                    'test set, a finished row\'s slot going to the next prompt; needs --seed, not with --samples > 1; same output file')
    ap.add_argument('--score', action='store_true', help='also write the teacher-forced scores of the generated rows: float32 (N, 9) or (N, n, 9) = the 8 '
                    'per-head sums of log-probability and the number of scored positions (all 8 heads of a position, kept by --keep or sampled)')
    ap.add_argument('--score_output', type=str, default=None, help='path of the score file (default: --output with .npy replaced by _score.npy)')
    ap.add_argument('--pick', type=str, default=None, choices=['best'], help='best: write only the sample of each prompt with the largest mean '
                    'log-probability per scored position, (N, max_seq_len, 8); needs --score')
    ap.add_argument('--score_dataset', action='store_true', help='no generation: score the dataset rows themselves behind their prime (needs --prime); '
                    'writes only the score file')
    ap.add_argument('--bars', type=int, default=None, metavar='N', help='every row finishes the bar its prime ends in and writes N whole new bars, then '
                    'stops (with and without --prime)')
    ap.add_argument('--infill', type=str, default=None, metavar='LO:HI', help='rewrite bars LO .. HI-1 of every piece and leave the rest alone: the rows '
                    'in front prime the decoder, the region is a MASK for the encoder, the rows behind are spliced back; needs --seed')
    ap.add_argument('--infill_mode', type=str, default='rows', choices=['rows', 'span'], help='the encoder sees a MASK row per row of the region (rows) '
                    'or one MASK row for the whole region (span)')
    ap.add_argument('--ordered', action='store_true', help='time-ordered sampling: no sampled (bar, position) goes back; the bar floor is LO under '
                    '--infill LO:HI and 0 otherwise')
    ap.add_argument('--lora', type=str, default=None, metavar='PATH', help='an adapter file (finetune_generation --lora_rank): loaded on top of --ckpt '
                    'and merged into the weights before anything runs')
    add_allow_flags(ap)
    add_schedule_flags(ap)
    add_anchor_flags(ap)
    return ap.parse_args(argv)


def score_path(args):
    """--score_output, or --output with .npy replaced by _score.npy."""
    if getattr(args, 'score_output', None):
        return args.score_output
    out = args.output
    return (out[:-4] if out.endswith('.npy') else out) + '_score.npy'


def parse_prime(value):
    """--prime -> None, 'half' or an int N >= 0; PBError otherwise."""
    if value is None or value == 'half':
        return value
    try:
        n = int(value)
    except ValueError:
        n = -1
    if n < 0:
        raise PBError('--prime takes a number of rows >= 0 or "half" (got %r)' % value)
    return n


def parse_infill(value, bar_pad=256):
    """--infill -> None or (lo, hi) with 0 <= lo < hi <= bar_pad; PBError otherwise. bar_pad: the bar head's PAD id of the dictionary in use
    (model.pianobart.bar_pad_word; 256 = the default dictionary's); None = no upper bound (check_args, before the dictionary is read)."""
    if value is None:
        return None
    parts = str(value).split(':')
    try:
        lo, hi = (int(v) for v in parts) if len(parts) == 2 else (-1, -1)
    except ValueError:
        lo, hi = -1, -1
    if not 0 <= lo < hi or (bar_pad is not None and hi > bar_pad):
        raise PBError('--infill takes LO:HI, two bar ids with 0 <= LO < HI <= %s (got %r)' % ('the bar PAD id' if bar_pad is None else '%d' % bar_pad, value))
    return lo, hi


def prime_lengths(x, prime, bar_pad, pad_word):
    """The prime length of every prompt of x (B, S, 8): k_b = min(N, L_b), or L_b // 2 for 'half', with L_b = the rows whose bar id is not
    PAD (Ablation.py:134), capped at the number of leading rows that are ordinary events (every id < PAD of its head: a prefix row may hold
    no special id, e.g. the EOS row)."""
    x = np.asarray(x)
    L = (x[:, :, 0] != bar_pad).sum(1)
    k = L // 2 if prime == 'half' else np.minimum(int(prime), L)
    ordinary = ((x >= 0) & (x < np.asarray(pad_word))).all(-1)
    lead = np.where(ordinary.all(1), x.shape[1], np.argmin(ordinary, axis=1))
    return [int(v) for v in np.minimum(k, lead)]


def prime_inputs(x, ks, pad_word):
    """Ablation.py:138: the encoder input with rows >= k_b of prompt b set to PAD, and the (B, max k, 8) decoder prefix (the same rows)."""
    enc = torch.as_tensor(np.asarray(x)).long().clone()
    prefix = enc[:, :max(ks, default=0)].clone()
    for b, k in enumerate(ks):
        enc[b, k:] = torch.as_tensor(np.asarray(pad_word))
    return enc, prefix


def check_args(args):
    """The argument rules that need no device; raises PBError."""
    parse_prime(getattr(args, 'prime', None))
    if args.batch_size < 1:
        raise PBError('--batch_size must be >= 1 (got %d)' % args.batch_size)
    if getattr(args, 'bars', None) is not None and args.bars < 0:
        raise PBError('--bars must be >= 0 (got %d)' % args.bars)
    if getattr(args, 'bars', None) is not None and getattr(args, 'score_dataset', False):
        raise PBError('--score_dataset generates nothing: it takes no --bars')
    if getattr(args, 'infill', None) is not None:
        parse_infill(args.infill, None)                  # the form; run() checks the bars against the dictionary's bar PAD id
        if args.seed is None:
            raise PBError('--infill needs --seed: the pieces are generated side by side, each from its own RandomState(seed + i)')
        for flag in ('prime', 'keep', 'bars'):
            if getattr(args, flag, None) is not None:
                raise PBError('--infill does not combine with --%s: it sets the prime, the kept attributes and the stop bar itself' % flag)
        if getattr(args, 'score_dataset', False):
            raise PBError('--score_dataset generates nothing: it takes no --infill')
    elif getattr(args, 'infill_mode', 'rows') != 'rows':
        raise PBError('--infill_mode %s needs --infill' % args.infill_mode)
    if getattr(args, 'ordered', False) and getattr(args, 'score_dataset', False):
        raise PBError('--score_dataset generates nothing: it takes no --ordered')
    if allow_flags_given(args) and getattr(args, 'score_dataset', False):
        raise PBError('--score_dataset generates nothing: it takes no --%s' % allow_flags_given(args)[0])
    if getattr(args, 'chords', None) is not None and getattr(args, 'score_dataset', False):
        raise PBError('--score_dataset generates nothing: it takes no --chords')
    check_anchor_flags(args)                                 # --accompany: needs --prime, not with --keep / --infill
    if getattr(args, 'accompany', None) is not None and getattr(args, 'score_dataset', False):
        raise PBError('--score_dataset generates nothing: it takes no --accompany')
    if getattr(args, 'keep', None) is not None:
        parse_keep(args.keep)
        if getattr(args, 'prime', None) is None:
            raise PBError('--keep needs --prime: the kept attributes come from the piece\'s own rows behind the prime')
        if getattr(args, 'score_dataset', False):
            raise PBError('--score_dataset generates nothing: it takes no --keep')
    samples = getattr(args, 'samples', 1)
    if samples < 1:
        raise PBError('--samples must be >= 1 (got %d)' % samples)
    if samples > 1 and args.seed is None:
        raise PBError('--samples %d needs --seed: sample j of prompt i draws from its own RandomState(seed + j * N + i); the one global RNG '
                      'stream of a run without --seed gives one continuation per prompt' % samples)
    if getattr(args, 'refill', None) is not None:
        check_refill(args.refill or True)
        if args.seed is None:
            raise PBError('--refill needs --seed: the prompts of a refilled decoder run side by side, each from its own RandomState(seed + i)')
        if samples > 1:
            raise PBError('--refill does not combine with --samples %d: the samples of a prompt share one cache slice' % samples)
        if getattr(args, 'score_dataset', False):
            raise PBError('--score_dataset generates nothing: it takes no --refill')
    if args.seed is None and args.batch_size > 1:
        raise PBError('--batch_size %d needs --seed: without it every prompt draws from the one global RNG stream in turn, which only the '
                      'batch-1 loop reproduces (the reference exits with ERROR for batches); with --seed s prompt i uses RandomState(s + i) '
                      'and the output does not depend on --batch_size' % args.batch_size)
    if getattr(args, 'pick', None) is not None and not getattr(args, 'score', False):
        raise PBError('--pick %s needs --score: the pick is made from the scores of the samples' % args.pick)
    if getattr(args, 'score_dataset', False):
        if getattr(args, 'prime', None) is None:
            raise PBError('--score_dataset needs --prime: the encoder sees the first k rows of a piece and the rows behind them are scored')
        if samples > 1:
            raise PBError('--score_dataset scores the dataset rows themselves: it takes no --samples (got %d)' % samples)
    if args.cuda_devices is not None and len(args.cuda_devices) > 1:
        raise PBError('eval_generation runs on ONE device: give one id to --cuda_devices')
    if args.cpu:
        raise PBError('pianobart_amd has no CPU execution path: eval_generation needs an MI355X')


def build_model(args, e2w, w2e):
    """demo.py's model from the flags (+ the checkpoint unless --nopretrain)."""
    shape = dict(max_position_embeddings=args.max_seq_len, d_model=args.hs)
    for side in ('encoder', 'decoder'):
        shape.update({side + '_layers': args.layers, side + '_ffn_dim': args.ffn_dims, side + '_attention_heads': args.heads})
    pianobart = PianoBart(bartConfig=BartConfig(**shape), e2w=e2w, w2e=w2e, precision=args.precision)
    model = PianoBartLM(pianobart)
    if not args.nopretrain:
        print("   Loading pre-trained model from", args.ckpt.split('/')[-1])
        sd = torch.load(args.ckpt, map_location='cpu', weights_only=False)['state_dict']
        model.load_state_dict(checkpoint_state_dict(sd, model), strict=False)
    return model


def load_data(dataset_path, dataset_name):
    return np.load(os.path.join(dataset_path, dataset_name), allow_pickle=True)


def eval_generation(args=None):
    """Returns the float32 array it saved to args.output: (N, max_seq_len, 8), or (N, n, max_seq_len, 8) with --samples n > 1 and no --pick;
    under --score_dataset the (N, 9) score array it saved instead."""
    if args is None:
        args = get_args()
    check_args(args)
    if not torch.cuda.is_available():
        raise PBError('pianobart_amd has no CPU execution path: eval_generation needs an MI355X')
    from .pretrain import _load_vocab
    print("Loading Dictionary")
    e2w, w2e = _load_vocab(args.dict_file)
    print("\nBuilding BART model")
    model = build_model(args, e2w, w2e)
    print("\nLoading Dataset", args.dataset_name)
    data = load_data(args.dataset_path, args.dataset_name)
    N = len(data)
    print("   len of dataset", N)
    if N and tuple(np.shape(data[0])) != (args.max_seq_len, 8):
        raise PBError('prompts of shape %s: expected (%d, 8) (--max_seq_len)' % (tuple(np.shape(data[0])), args.max_seq_len))
    device_num = args.cuda_devices[0] if args.cuda_devices else 0
    device = torch.device('cuda', device_num)
    print("Use GPU", device)
    model = model.to(device).eval()
    if getattr(args, 'lora', None):
        from . import lora as _lora
        print("   Merging adapters from", args.lora.split('/')[-1])
        _lora.load(args.lora, model, with_optimizer=False)
        model._get_engine().merge_lora()
    bar_pad = model.pianobart.bar_pad_word
    prime = parse_prime(getattr(args, 'prime', None))
    samples = getattr(args, 'samples', 1)
    keep = parse_keep(args.keep) if getattr(args, 'keep', None) is not None else None
    bars, infill, truncated = getattr(args, 'bars', None), parse_infill(getattr(args, 'infill', None), bar_pad), 0
    pad_word = model.pianobart.pad_word_np
    accompany = getattr(args, 'accompany', None)
    floor = (infill[0] if infill is not None else 0) if getattr(args, 'ordered', False) or accompany is not None else None       # --ordered (implied by --accompany): every row's bar floor
    amask = allow_from_args(args, e2w)                   # --key / --pitch_range / ..: the one allow mask of every row (None: no flag)

    def allowed(y, ks, forced, own):
        """The allow flags: every output row of y (row r belongs to piece own[r] of the call) stays inside the mask behind its prime."""
        for r, p in enumerate(own if amask is not None else []):
            k = ks[p] if ks is not None else 0
            if not is_allowed(y[r], amask, start=k, forced=forced[p] if forced is not None else None, layout=model.pianobart.layout):
                raise PBError('--%s: output row %d leaves the allowed classes behind its prime of %d rows' % (allow_flags_given(args)[0], r, k))

    schedule_from_args(args, e2w)                        # --chords: the flags' own refusals, before any device work

    def scheduled(y, ks, forced, own, bar):
        """--chords: every output row of y (row r belongs to piece own[r] of the call) follows its piece's schedule behind its prime."""
        for r, p in enumerate(own if bar is not None else []):
            k = ks[p] if ks is not None else 0
            if not follows_schedule(y[r], bar[p], start=k, forced=forced[p] if forced is not None else None, layout=model.pianobart.layout):
                raise PBError('--chords: output row %d leaves its bar schedule behind its prime of %d rows' % (r, k))

    def anchored(y, ks, own, anc):
        """--accompany: every output row of y (row r belongs to piece own[r] of the call) holds its piece's anchors, in time order."""
        for r, p in enumerate(own if anc is not None else []):
            ok, placed = follows_anchors(y[r], anc[p], start=ks[p], layout=model.pianobart.layout)
            if not ok:
                raise PBError('--accompany: output row %d holds %d of its %d anchors in time order behind its prime of %d rows' % (r, placed, len(anc[p]), ks[p]))

    def inputs(x):
        """What one generate call gets for the pieces x (B, S, 8): the encoder input, decoder prefix, prefix lengths, forced table, stop bars,
        (--infill) the plans, (--ordered) the bar floors, (the allow flags) the masks, (--chords) the bar schedules and (--accompany) the
        anchors."""
        prefix = ks = forced = stops = plans = anc = None
        order = [floor] * len(x) if floor is not None else None
        allow = [amask] * len(x) if amask is not None else None
        if infill is not None:
            plans = [infill_plan(p, infill[0], infill[1], model.pianobart.mask_word_np, pad_word, getattr(args, 'infill_mode', 'rows')) for p in x.numpy()]
            ks, stops = [pl['k'] for pl in plans], [pl['stop'] for pl in plans]
            prefix = torch.as_tensor(np.asarray(pad_word)).long().repeat(len(plans), max(ks, default=0), 1)
            for b, pl in enumerate(plans):
                prefix[b, :ks[b]] = torch.as_tensor(pl['prefix'])
            x = torch.as_tensor(np.stack([pl['enc'] for pl in plans])).long() if plans else x
        elif prime is not None:                       # the Ablation.py:132-139 split: first k_b rows primed, the encoder sees them only
            ks = prime_lengths(x.numpy(), prime, bar_pad, pad_word)
            forced = keep_mask(x, keep, ks, bar_pad) if keep is not None else None     # from the piece's rows, before prime_inputs pads them
            if accompany is not None:                 # likewise: each piece's skyline / bass line behind its prime
                anc = [anchors_from_args(args, x[b], ks[b], e2w) for b in range(len(x))]
            x, prefix = prime_inputs(x, ks, pad_word)
        if bars is not None:
            stops = [stop_after_bars(prefix[b, :ks[b]] if ks is not None else None, bars, bar_pad) for b in range(len(x))]
        elif anc is not None:                         # --accompany without --bars: the row stops at the bar after its last anchor
            stops = [min(int(a[-1, 0]) + 1, int(bar_pad)) if len(a) else int(bar_pad) for a in anc]
        bar = None
        if getattr(args, 'chords', None) is not None:        # one schedule per piece: its first chord sits behind the piece's own prime
            bar = [schedule_from_args(args, e2w, prefix[b, :ks[b]] if ks is not None and ks[b] else None) for b in range(len(x))]
        return x, prefix, ks, forced, stops, plans, order, allow, bar, anc

    def splice(y, plans, own):
        """--infill: row r of y (numpy) spliced with the suffix of its piece own[r]; counts the truncated ones."""
        nonlocal truncated
        for r, p in enumerate(own):
            y[r], cut = infill_splice(y[r], plans[p]['suffix'], args.max_seq_len, bar_pad)
            truncated += int(cut)
            if floor is not None and not is_time_ordered(y[r], start=plans[p]['k'], floor=floor):
                raise PBError('--ordered --infill: output row %d is not in time order behind its prime of %d rows' % (r, plans[p]['k']))
        return y
    output = np.zeros((N, args.max_seq_len, 8) if samples == 1 else (N, samples, args.max_seq_len, 8), dtype=np.float32)
    do_score = getattr(args, 'score', False)
    scores = np.zeros((N, 9) if samples == 1 else (N, samples, 9), dtype=np.float32)

    def score_rows(x, y, start):
        """(R, 9) scores of the rows y of one generate call: encoder input x and its mask as the generation saw them, one row of x per row of y."""
        r = model.score(x, y.to(device), (x[:, :, 0] != bar_pad).float(), start=start, device_num=-1)
        return torch.cat([r.sum_logp, r.count[:, None]], 1).numpy(), r.hits.double().sum(0).numpy()

    print("\nEval Start")
    if getattr(args, 'score_dataset', False):
        hits = np.zeros(8)
        for c0 in range(0, N, args.batch_size):
            c1 = min(N, c0 + args.batch_size)
            piece = torch.as_tensor(np.asarray(data[c0:c1])).long()
            ks = prime_lengths(piece.numpy(), prime, bar_pad, model.pianobart.pad_word_np)
            x, _ = prime_inputs(piece, ks, model.pianobart.pad_word_np)
            scores[c0:c1], h = score_rows(x.to(device), piece, ks)
            hits += h
        np.save(score_path(args), scores)
        print("Saved", scores.shape, "to", score_path(args))
        count = max(float(scores[:, 8].astype(np.float64).sum()), 1.0)
        logp, hit = scores[:, :8].astype(np.float64).sum(0) / count, hits / count
        print('LogP: {:06f} | logp: {:03f}, {:03f}, {:03f}, {:03f}, {:03f}, {:03f}, {:03f}, {:03f}'.format(np.average(logp), *logp))
        print('Hit: {:06f} | hit: {:03f}, {:03f}, {:03f}, {:03f}, {:03f}, {:03f}, {:03f}, {:03f}'.format(np.average(hit), *hit))
        return scores
    with torch.no_grad():
        rows = [(i, j) for i in range(N) for j in range(samples)] if samples > 1 else []      # prompt-major output rows
        for r0 in range(0, len(rows), args.batch_size):     # --samples n > 1: --batch_size rows per call, the samples of a prompt grouped
            chunk = rows[r0:r0 + args.batch_size]
            c0, c1 = chunk[0][0], chunk[-1][0] + 1
            x, prefix, ks, forced, stops, plans, order, allow, bar, anc = inputs(torch.as_tensor(np.asarray(data[c0:c1])).long())
            x = x.to(device)
            y = model.generate_batch(x, (x[:, :, 0] != bar_pad).float(), seeds=[sample_seed(args.seed, j, i, N) for i, j in chunk],
                                     device_num=device_num, decoder_prefix=prefix, prefix_len=ks, decoder_forced=forced, decoder_stop=stops,
                                     decoder_order=order, decoder_allow=allow, **(dict(decoder_bar_allow=bar) if bar is not None else {}),
                                     **(dict(decoder_anchors=anc) if anc is not None else {}),
                                     samples_per_prompt=[sum(1 for i, _ in chunk if i == p) for p in range(c0, c1)])
            own = [i - c0 for i, _ in chunk]
            allowed(y, ks, forced, own)
            scheduled(y, ks, forced, own, bar)
            anchored(y, ks, own, anc)
            if do_score:
                sc, _ = score_rows(x[torch.as_tensor(own, device=device)], y, [ks[p] for p in own] if ks is not None else None)
            y = y.float().cpu().numpy()
            if plans is not None:
                y = splice(y, plans, own)
            for r, (i, j) in enumerate(chunk):
                output[i, j] = y[r]
                if do_score:
                    scores[i, j] = sc[r]
        refill = getattr(args, 'refill', None)
        gen_rows = max(N, 1) if refill is not None else args.batch_size          # --refill: every prompt in one call, scored in --batch_size batches
        for c0 in range(0, N if samples == 1 else 0, gen_rows):
            c1 = min(N, c0 + gen_rows)
            x, prefix, ks, forced, stops, plans, order, allow, bar, anc = inputs(torch.as_tensor(np.asarray(data[c0:c1])).long())
            x = x.to(device)
            attn_encoder = (x[:, :, 0] != bar_pad).float()
            if args.seed is None:
                y = model(input_ids_encoder=x, encoder_attention_mask=attn_encoder, generate=True, device_num=device_num, decoder_prefix=prefix,
                          decoder_forced=forced, decoder_stop=stops, decoder_order=order, decoder_allow=allow,
                          **(dict(decoder_bar_allow=bar) if bar is not None else {}), **(dict(decoder_anchors=anc) if anc is not None else {}))
            else:
                y = model.generate_batch(x, attn_encoder, seeds=[args.seed + i for i in range(c0, c1)], device_num=device_num,
                                         decoder_prefix=prefix, prefix_len=ks, decoder_forced=forced, decoder_stop=stops, decoder_order=order,
                                         decoder_allow=allow, refill=(refill or True) if refill is not None else False,
                                         **(dict(decoder_bar_allow=bar) if bar is not None else {}), **(dict(decoder_anchors=anc) if anc is not None else {}))
            allowed(y, ks, forced, list(range(c1 - c0)))
            scheduled(y, ks, forced, list(range(c1 - c0)), bar)
            anchored(y, ks, list(range(c1 - c0)), anc)
            output[c0:c1] = y.float().cpu().numpy() if plans is None else splice(y.float().cpu().numpy(), plans, list(range(c1 - c0)))
            for s0 in range(0, c1 - c0 if do_score else 0, args.batch_size):
                s1 = min(c1 - c0, s0 + args.batch_size)
                scores[c0 + s0:c0 + s1], _ = score_rows(x[s0:s1], y[s0:s1], ks[s0:s1] if ks is not None else None)
    if do_score:
        np.save(score_path(args), scores)
        print("Saved", scores.shape, "to", score_path(args))
        if getattr(args, 'pick', None) == 'best' and samples > 1:
            output = output[np.arange(N), pick_best(scores)]
    if infill is not None:
        print("Truncated pieces:", truncated)
    np.save(args.output, output)
    print("Saved", output.shape, "to", args.output)
    return output


if __name__ == '__main__':
    eval_generation()
