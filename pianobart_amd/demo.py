"""MIDI in -> PianoBART continuation -> MIDI out: the reference's demo.py:105-170 on the HIP path.

Same `Args` fields and command-line flags as the reference (demo.py:12-29, 33-58), same order of work: vocabulary, model from the
flags, checkpoint with `load_state_dict(strict=False)` (demo.py:128-129), `Midi2Octuple` (demo.py:61-68), encoder mask = bar
column != PAD, `model(generate=True)` (demo.py:157; here one decoder token per step against the K/V caches instead of a full
encoder + decoder pass per position: same tokens), `Octuple2Midi` (demo.py:72-102). No CPU path (`--cpu` raises).
"""
import argparse
import os

import numpy as np
import torch

from ._lib import PBError
from .model import BartConfig, PianoBart, PianoBartLM, checkpoint_state_dict
from .octuple_midi import Midi2Octuple, Octuple2Midi

_HERE = os.path.dirname(os.path.abspath(__file__))
_VOCAB = os.path.join(_HERE, 'data', 'octuple_vocab.json')


class Args:
    """demo.py:12-29: what gui/backend/app.py builds instead of a command line."""

    def __init__(self, dict_file=_VOCAB, ckpt='./PianoBART_Giant.ckpt', input='./Data/POP909/POP909/001/001.mid', output='./output.mid',
                 num_workers=5, max_seq_len=1024, hs=1024, layers=8, ffn_dims=2048, heads=8, nopretrain=False, cpu=False, cuda_devices=[0],
                 precision='bf16', prime=None, samples=1, seed=None, keep=None, bars=None, infill=None, infill_mode='rows', ordered=False,
                 key=None, pitch_range=None, instruments=None, tempo=None, max_duration=None, velocity=None, chords=None, bars_per_chord=1,
                 chord_start=None, lora=None, accompany=None):
        self.dict_file, self.ckpt, self.input, self.output, self.num_workers = dict_file, ckpt, input, output, num_workers
        self.max_seq_len, self.hs, self.layers, self.ffn_dims, self.heads = max_seq_len, hs, layers, ffn_dims, heads
        self.nopretrain, self.cpu, self.cuda_devices, self.precision = nopretrain, cpu, cuda_devices, precision
        self.prime = prime                  # None, N or 'half': continue the piece from its first rows (eval_generation's --prime rule)
        self.keep = keep                    # None or 'ATTR[,ATTR...]': attributes of the piece's own rows behind the prime that are kept (needs prime)
        self.bars = bars                    # None or N: finish the bar the prime ends in, write N whole new bars, stop (eval_generation --bars)
        self.infill, self.infill_mode = infill, infill_mode     # None or 'LO:HI': rewrite bars LO .. HI-1 of the piece (eval_generation --infill; needs a seed)
        self.ordered = ordered              # time-ordered sampling: no sampled (bar, position) goes back (eval_generation --ordered)
        # allowed classes (eval_generation --key / --pitch_range / --instruments / --tempo / --max_duration / --velocity): one mask for the piece
        self.key, self.pitch_range, self.instruments, self.tempo, self.max_duration, self.velocity = key, pitch_range, instruments, tempo, max_duration, velocity
        # a bar schedule (eval_generation --chords / --bars_per_chord / --chord_start): the pitches follow a chord progression bar by bar
        self.chords, self.bars_per_chord, self.chord_start = chords, bars_per_chord, chord_start
        self.accompany = accompany          # None, 'skyline' or 'bass': keep that line of the piece behind the prime, write the notes around it (needs prime)
        self.lora = lora                    # None or the path of an adapter file: merged into the checkpoint's weights before generation (eval_generation --lora)
        self.samples, self.seed = samples, seed     # n continuations of the piece (n > 1 needs a seed): sample j from RandomState(seed + j)


def get_args(argv=None):
    ap = argparse.ArgumentParser(description='')
    ap.add_argument('--dict_file', type=str, default=_VOCAB)
    ap.add_argument('--ckpt', default='result/pretrain/pianobart/model_best.ckpt')
    ap.add_argument('--input', default='./Data/POP909/POP909/001/001.mid')
    ap.add_argument('--output', default='./output.mid')
    ap.add_argument('--num_workers', type=int, default=5)
    ap.add_argument('--max_seq_len', type=int, default=1024, help='all sequences are padded to `max_seq_len`')
    ap.add_argument('--hs', type=int, default=1024)
    ap.add_argument('--layers', type=int, default=8)
    ap.add_argument('--ffn_dims', type=int, default=2048)
    ap.add_argument('--heads', type=int, default=8)
    ap.add_argument('--nopretrain', action='store_true', default=False)
    ap.add_argument('--cpu', action='store_true')
    ap.add_argument('--cuda_devices', type=int, nargs='+', default=[0], help='HIP device ids (one: generate is batch-1 sequential)')
    ap.add_argument('--precision', default='bf16', choices=['bf16', 'fp32', 'bf16x3'])
    ap.add_argument('--prime', type=str, default=None, help='N or "half": keep the first k = min(N, L) (half: L // 2) rows of the piece and '
                    'continue from there (eval_generation --prime)')
    ap.add_argument('--keep', type=str, default=None, help='ATTR[,ATTR...] of bar, position, instrument, pitch, duration, velocity, timesig, tempo (needs '
                    '--prime): these attributes of the input piece behind the prime are kept and the model writes the others')
    ap.add_argument('--samples', type=int, default=1, help='continuations of the piece: n MIDI files, --output for the first, the others with '
                    'the sample index in front of the extension (out.mid, out.1.mid, ..); n > 1 needs --seed')
    ap.add_argument('--seed', type=int, default=None, help='with --samples: sample j draws from RandomState(seed + j)')
    ap.add_argument('--bars', type=int, default=None, metavar='N', help='finish the bar the prime ends in, write N whole new bars, then stop')
    ap.add_argument('--infill', type=str, default=None, metavar='LO:HI', help='rewrite bars LO .. HI-1 of the piece and leave the rest alone (needs --seed; '
                    'not with --prime, --keep or --bars)')
    ap.add_argument('--infill_mode', type=str, default='rows', choices=['rows', 'span'], help='the encoder sees a MASK row per row of the region (rows) '
                    'or one MASK row for the whole region (span)')
    ap.add_argument('--ordered', action='store_true', help='time-ordered sampling: no sampled (bar, position) goes back; the bar floor is LO under '
                    '--infill LO:HI and 0 otherwise')
    ap.add_argument('--lora', type=str, default=None, metavar='PATH', help='an adapter file (finetune_generation --lora_rank): loaded on top of --ckpt '
                    'and merged into the weights before generation')
    from .generation import add_allow_flags
    add_allow_flags(ap)
    from .generation import add_schedule_flags
    add_schedule_flags(ap)
    from .generation import add_anchor_flags
    add_anchor_flags(ap)
    return ap.parse_args(argv)


def sample_paths(output, n):
    """The n files of --samples n: the name as given, then the sample index in front of the extension."""
    root, ext = os.path.splitext(output)
    return [output] + ['%s.%d%s' % (root, j, ext) for j in range(1, n)]


def check_samples_args(samples, seed):
    """The --samples rules; raises PBError."""
    if samples < 1:
        raise PBError('--samples must be >= 1 (got %d)' % samples)
    if samples > 1 and seed is None:
        raise PBError('--samples %d needs --seed: sample j draws from its own RandomState(seed + j)' % samples)


def check_keep_args(keep, prime):
    """The --keep rules; raises PBError. Returns the kept head indices, or None."""
    if keep is None:
        return None
    from .generation import parse_keep
    heads = parse_keep(keep)
    if prime is None:
        raise PBError('--keep needs --prime: the kept attributes come from the piece\'s own rows behind the prime')
    return heads


def check_dictionary(e2w):
    """demo() converts MIDI <-> Octuple with octuple_midi, which is the DEFAULT dictionary's codec: its PAD_ROW / EOS_ROW are that
    dictionary's ids. The model itself takes any legal dictionary (ops.Layout); a piece encoded under another one would be read and
    written with the wrong ids here, so the demo refuses it. Raises PBError naming the first head that differs."""
    from . import octuple_midi as OM
    from .ops import CLASS_NAMES, Layout
    lay = Layout.from_dict(e2w)
    for h, name in enumerate(CLASS_NAMES):
        if lay.sizes[h] != OM.PAD_ROW[h] + 6 or lay.pad8[h] != OM.PAD_ROW[h] or lay.specials[h][3] != OM.EOS_ROW[h]:
            raise PBError('demo: the dictionary\'s head %d (%s) has %d ids with <PAD> = %d; the MIDI codec (octuple_midi) is written for %d ids with '
                          '<PAD> = %d. MIDI conversion exists for the default dictionary only: generate with eval_generation on encoded data'
                          % (h, name, lay.sizes[h], lay.pad8[h], OM.PAD_ROW[h] + 6, OM.PAD_ROW[h]))
    return lay


def check_bar_args(bars, infill, prime, keep, seed):
    """The --bars and --infill rules (eval_generation's); raises PBError. Returns (lo, hi) or None."""
    from .eval_generation import parse_infill
    if bars is not None and bars < 0:
        raise PBError('--bars must be >= 0 (got %d)' % bars)
    region = parse_infill(infill)
    if region is not None:
        if seed is None:
            raise PBError('--infill needs --seed: the piece is generated from its own RandomState(seed)')
        for flag, v in (('prime', prime), ('keep', keep), ('bars', bars)):
            if v is not None:
                raise PBError('--infill does not combine with --%s: it sets the prime, the kept attributes and the stop bar itself' % flag)
    return region


def demo(args=None):
    if not args:
        args = get_args()
    keep = check_keep_args(getattr(args, 'keep', None), getattr(args, 'prime', None))
    bars = getattr(args, 'bars', None)
    region = check_bar_args(bars, getattr(args, 'infill', None), getattr(args, 'prime', None), getattr(args, 'keep', None), getattr(args, 'seed', None))
    from .generation import check_anchor_flags
    check_anchor_flags(args)                 # --accompany: needs --prime, not with --keep / --infill
    if args.cpu or not torch.cuda.is_available():
        raise PBError('pianobart_amd has no CPU execution path: demo() needs an MI355X')
    if args.cuda_devices is not None and len(args.cuda_devices) > 1:
        raise PBError('generate is batch-1 sequential: give ONE device (the reference itself is single-device here, README.md:154)')
    from .eval_generation import parse_prime, prime_inputs, prime_lengths
    samples, seed = getattr(args, 'samples', 1), getattr(args, 'seed', None)
    check_samples_args(samples, seed)
    prime = parse_prime(getattr(args, 'prime', None))
    from .pretrain import _load_vocab
    print("Loading Dictionary")
    e2w, w2e = _load_vocab(args.dict_file)
    check_dictionary(e2w)
    print("\nBuilding BART model")
    shape = dict(max_position_embeddings=args.max_seq_len, d_model=args.hs)
    for side in ('encoder', 'decoder'):
        shape.update({side + '_layers': args.layers, side + '_ffn_dim': args.ffn_dims, side + '_attention_heads': args.heads})
    pianobart = PianoBart(bartConfig=BartConfig(**shape), e2w=e2w, w2e=w2e, precision=getattr(args, 'precision', 'bf16'))
    model = PianoBartLM(pianobart)
    if not args.nopretrain:
        print("   Loading pre-trained model from", args.ckpt.split('/')[-1])
        sd = torch.load(args.ckpt, map_location='cpu', weights_only=False)['state_dict']
        model.load_state_dict(checkpoint_state_dict(sd, model), strict=False)       # 'module.'-prefixed multi-GPU files load too
    octuple = Midi2Octuple(args.input, window=args.max_seq_len)
    device_num = args.cuda_devices[0] if args.cuda_devices else 0
    device = torch.device('cuda', device_num)
    print("Use GPU", device)
    model = model.to(device).eval()
    if getattr(args, 'lora', None):
        from . import lora as _lora
        print("   Merging adapters from", args.lora.split('/')[-1])
        _lora.load(args.lora, model, with_optimizer=False)
        model._get_engine().merge_lora()
    octuple, prefix, ks, forced, stops, plan, anc = octuple.long(), None, None, None, None, None, None
    if region is not None:                   # the rows in front of the region prime the decoder, the encoder sees the region as MASK
        from .generation import infill_plan
        plan = infill_plan(octuple[0], region[0], region[1], pianobart.mask_word_np, pianobart.pad_word_np, getattr(args, 'infill_mode', 'rows'))
        ks, stops = [plan['k']], [plan['stop']]
        prefix = torch.as_tensor(plan['prefix']).long()[None]
        octuple = torch.as_tensor(plan['enc']).long()[None]
    elif prime is not None:                    # the piece's first k rows primed, the encoder sees them only
        ks = prime_lengths(octuple.numpy(), prime, pianobart.bar_pad_word, pianobart.pad_word_np)
        if keep is not None:                 # the kept attributes of the piece's rows behind the prime are given, the others sampled
            from .generation import keep_mask
            forced = keep_mask(octuple, keep, ks, pianobart.bar_pad_word)
        from .generation import anchors_from_args
        anc = anchors_from_args(args, octuple[0], ks[0], e2w)     # --accompany: the piece's skyline / bass line behind the prime (None: no flag)
        octuple, prefix = prime_inputs(octuple, ks, pianobart.pad_word_np)
    if bars is not None:                     # the row finishes the bar its prime ends in and writes `bars` whole new bars
        from .generation import stop_after_bars
        stops = [stop_after_bars(prefix[0, :ks[0]] if ks is not None else None, bars, pianobart.bar_pad_word)]
    elif anc is not None and len(anc):       # --accompany without --bars: the row stops at the bar after its last anchor
        stops = [min(int(anc[-1, 0]) + 1, int(pianobart.bar_pad_word))]
    order = [region[0] if region is not None else 0] if getattr(args, 'ordered', False) or anc is not None else None      # the bar floor: the region's first bar, else 0
    from .generation import allow_from_args
    amask = allow_from_args(args, e2w)       # --key / --pitch_range / ..: what the free heads may sample (None: no flag)
    allow = [amask] if amask is not None else None
    from .generation import schedule_from_args
    bar = schedule_from_args(args, e2w, prefix[0, :ks[0]] if ks is not None and ks[0] else None)     # --chords: the first chord behind the prime
    bar = dict(decoder_bar_allow=[bar]) if bar is not None else {}
    if anc is not None:
        bar['decoder_anchors'] = [anc]
    octuple = octuple.to(device)
    attn_encoder = (octuple[:, :, 0] != pianobart.bar_pad_word).float()
    with torch.no_grad():
        if samples > 1 or region is not None:        # n continuations from one encoder pass: sample j of the one piece under RandomState(seed + j)
            from .generation import sample_seed
            y = model.generate_batch(octuple, attn_encoder, seeds=[sample_seed(seed, j, 0, 1) for j in range(samples)], device_num=device_num,
                                     decoder_prefix=prefix, prefix_len=ks, samples_per_prompt=samples,
                                     decoder_forced=forced, decoder_stop=stops, decoder_order=order, decoder_allow=allow, **bar)
        else:
            y = model(input_ids_encoder=octuple, encoder_attention_mask=attn_encoder, generate=True, device_num=device_num, decoder_prefix=prefix,
                      decoder_forced=forced, decoder_stop=stops, decoder_order=order, decoder_allow=allow, **bar)
    if plan is not None:                     # the rows behind the region go back behind the new ones
        from .generation import infill_splice
        spliced = [infill_splice(row, plan['suffix'], args.max_seq_len, pianobart.bar_pad_word) for row in y.cpu()]
        y = torch.as_tensor(np.stack([r for r, _ in spliced])).to(y.dtype)
        print("Truncated pieces:", sum(int(c) for _, c in spliced))
        if order is not None:
            from .generation import is_time_ordered
            for j, row in enumerate(y):
                if not is_time_ordered(row, start=plan['k'], floor=order[0]):
                    raise PBError('--ordered --infill: sample %d is not in time order behind its prime of %d rows' % (j, plan['k']))
    if anc is not None:
        from .generation import follows_anchors
        for j, row in enumerate(y.cpu()):
            ok, placed = follows_anchors(row, anc, start=ks[0])
            if not ok:
                raise PBError('--accompany: sample %d holds %d of its %d anchors in time order behind its prime of %d rows' % (j, placed, len(anc), ks[0]))
    for j, path in enumerate(sample_paths(args.output, samples)):
        if Octuple2Midi(y[j:j + 1], path):
            print(f"Saved to {path}")
    print(octuple.shape, y.shape)
    return octuple, y


if __name__ == '__main__':
    demo()
