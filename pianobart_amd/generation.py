"""Generation on the engine: the KV-cached autoregressive decode of one prompt (`generate`), of a batch of prompts and of several samples
per prompt (`generate_batch`) through the fused decoder of csrc/pb_decode.hip, and the two reference paths that cross-check them.

GenerationMixin is the generation half of pianobart_amd.engine.Engine: its methods use the engine's flat parameter views (self.w / self.wf),
forward schedule (forward_hidden, heads_forward, _linear, _attn_fwd) and id checks (bind, note_ids, check_ids), and nothing here imports engine.py.

Reference semantics followed (file:line into the reference project): model.py:28-66 (the decode loop), model.py:68-107 (nucleus sampling).
"""
import contextlib
import os
import time
from types import SimpleNamespace

import numpy as np
import torch

from . import ops
from ._lib import LIB, PB_BF16, PBError

_DECODE_SPEC = int(os.environ.get('PB_DECODE_SPEC', '1'))                       # 1 = device-side sampling ahead of the host where the caller names the sampler (Engine._decode_device_sampled), 0 = one host round trip per token
_DECODE_GRAPH = int(os.environ.get('PB_DECODE_GRAPH', '1'))                     # 1 = one hipGraph replay per token (6 launches per layer), 0 = the same launches issued directly, -1 = the round-2 per-launch loop (the persistent-kernel forms of round 4, measured slower, left the library in round 5: profiles/r04_decode_persistent.txt)

LN_EPS = 1e-5                      # LayerNorm epsilon of every layer (the engine's schedules take it from here)


def check_prefix(prefix, prefix_len, B, S, pad):
    """The argument rules of primed generation, on the host before any device work. prefix: (B, P, 8) Octuple ids (tensor on any device, or
    array) whose rows 0 .. k_b - 1 prime prompt b; prefix_len: B lengths (None: P for every row). Every id of a prefix row must be an ordinary
    event, 0 <= id < pad[head] -- the range check of a decoder input (note_ids), without the special ids a decoder input may otherwise hold.
    Returns (k, rows): k = [k_b], rows = int64 CPU (B, max k_b, 8), or None when no row is primed. Raises PBError."""
    if prefix is None:
        if prefix_len is not None and any(int(v) for v in (prefix_len.tolist() if hasattr(prefix_len, 'tolist') else prefix_len)):
            raise PBError('prefix_len given without a prefix')
        return [0] * B, None
    p = torch.as_tensor(prefix)
    if p.dim() != 3 or int(p.shape[0]) != B or int(p.shape[2]) != 8:
        raise PBError('prefix of shape %s: expected (%d, P, 8) for %d prompt(s)' % (tuple(p.shape), B, B))
    if p.dtype.is_floating_point or p.dtype.is_complex or p.dtype == torch.bool:
        raise PBError('prefix ids must be integers (got %s)' % p.dtype)
    P = int(p.shape[1])
    if prefix_len is None:
        k = [P] * B
    else:
        k = [int(v) for v in (prefix_len.tolist() if hasattr(prefix_len, 'tolist') else prefix_len)]
        if len(k) != B:
            raise PBError('prefix_len has %d entries for %d prompt(s)' % (len(k), B))
    for b, kb in enumerate(k):
        if not 0 <= kb <= min(S, P):
            raise PBError('prefix_len[%d] = %d outside 0 .. %d (window S = %d, prefix rows P = %d)' % (b, kb, min(S, P), S, P))
    if max(k, default=0) == 0:
        return k, None
    rows = p[:, :max(k)].detach().to('cpu', torch.int64)
    lim = torch.as_tensor(np.asarray(pad), dtype=torch.int64)
    for b, kb in enumerate(k):
        bad = ((rows[b, :kb] < 0) | (rows[b, :kb] >= lim)).nonzero()
        if len(bad):
            i, h = int(bad[0, 0]), int(bad[0, 1])
            raise PBError('prefix of prompt %d, row %d, head %d: id %d is not an ordinary event (0 <= id < %d)' % (b, i, h, int(rows[b, i, h]), int(lim[h])))
    return k, rows


def check_samples(samples, P, n_rngs):
    """The argument rules of samples-per-prompt generation, on the host before any device work. samples: an int n >= 1 (n samples of every
    prompt) or P ints >= 1 (n_p samples of prompt p); n_rngs: the generators the caller holds, one per output row. Returns the row-to-prompt
    map of the R = sum(n_p) output rows in prompt-major order: [0] * n_0 + [1] * n_1 + ... Raises PBError."""
    if isinstance(samples, (int, np.integer)) and not isinstance(samples, bool):
        counts = [int(samples)] * P
    else:
        try:
            counts = [v for v in (samples.tolist() if hasattr(samples, 'tolist') else list(samples))]
        except TypeError:
            raise PBError('samples_per_prompt must be an int or a sequence of ints (got %r)' % (samples,))
        if len(counts) != P:
            raise PBError('samples_per_prompt has %d entries for %d prompt(s)' % (len(counts), P))
    for p, n in enumerate(counts):
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)):
            raise PBError('samples_per_prompt[%d] = %r is not an integer' % (p, n))
        if n < 1:
            raise PBError('samples_per_prompt[%d] = %d: every prompt needs at least one sample' % (p, n))
    owner = [p for p, n in enumerate(counts) for _ in range(int(n))]
    if n_rngs != len(owner):
        raise PBError('generate_batch: %d generators for %d output rows (samples_per_prompt sums to %d over %d prompts)'
                      % (n_rngs, len(owner), len(owner), P))
    return owner


def check_refill(refill, samples=None, batch_max=16):
    """The argument rules of refilled batched generation, on the host before any device work. refill: False / None (off), True (batch_max
    slots) or an int n, 2 <= n <= batch_max (n slots). It does not combine with samples-per-prompt generation: the samples of a prompt
    share a cache slice, which would have to change owners. Returns the slot count, 0 for off. Raises PBError."""
    if refill is None or refill is False:
        return 0
    if refill is True:
        n = int(batch_max)
    elif isinstance(refill, (int, np.integer)):
        n = int(refill)
        if not 2 <= n <= batch_max:
            raise PBError('refill = %d: the slot count must be 2 .. %d (True = %d)' % (n, batch_max, batch_max))
    else:
        raise PBError('refill must be False, True or an int 2 .. %d (got %r)' % (batch_max, refill))
    if samples is not None:
        raise PBError('refill does not combine with samples: the samples of a prompt share one cache slice')
    return n


def check_stop(stop, P, pad0, owner=None):
    """The argument rules of bar-bounded generation, on the host before any device work. stop: P bar ids (list, array or tensor on any
    device), one per prompt: row p also ends at its first token, from its prefix length on, whose bar id (head 0) is >= stop[p];
    0 <= stop[p] <= pad0, pad0 (the bar head's first special id) = no stop. owner (row -> prompt, check_samples): the list is expanded to
    one entry per output row. Returns a list of ints, P or R long; None for stop=None or a list that is pad0 everywhere (no stop: the
    caller runs what it ran before). Raises PBError for a wrong length, a non-integer or a value outside 0 .. pad0."""
    if stop is None:
        return None
    try:
        vals = stop.tolist() if hasattr(stop, 'tolist') else list(stop)
    except TypeError:
        raise PBError('stop must be a sequence of %d bar ids, one per prompt (got %r)' % (P, stop))
    if not isinstance(vals, list) or len(vals) != P:
        raise PBError('stop has %d entries for %d prompt(s)' % (len(vals) if isinstance(vals, list) else 1, P))
    for p, v in enumerate(vals):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise PBError('stop[%d] = %r is not an integer' % (p, v))
        if not 0 <= v <= pad0:
            raise PBError('stop[%d] = %d outside 0 .. %d (a bar id; %d = no stop)' % (p, v, pad0, pad0))
    if all(int(v) == pad0 for v in vals):
        return None
    vals = [int(v) for v in vals]
    return vals if owner is None else [vals[p] for p in owner]


def check_order(order, P, owner=None, order_max=None):
    """The argument rules of time-ordered generation, on the host before any device work. order: P ints (list, array or tensor on any
    device), one per prompt: -1 = row p is sampled as ever, 0 .. order_max = row p is time-ordered with that bar floor (0: ordered, no
    extra floor). order_max = the dictionary's last bar id, pad[0] - 1 (None: ORDER_MAX, the default dictionary's). owner (row -> prompt,
    check_samples): the list is expanded to one entry per output row. Returns a list of ints, P or R long; None for order=None or a list
    that is -1 everywhere (no order: the caller runs what it ran before). Raises PBError for a wrong length, a non-integer or a value
    outside -1 .. order_max."""
    if order is None:
        return None
    order_max = ORDER_MAX if order_max is None else int(order_max)
    try:
        vals = order.tolist() if hasattr(order, 'tolist') else list(order)
    except TypeError:
        raise PBError('order must be a sequence of %d bar floors, one per prompt (got %r)' % (P, order))
    if not isinstance(vals, list) or len(vals) != P:
        raise PBError('order has %d entries for %d prompt(s)' % (len(vals) if isinstance(vals, list) else 1, P))
    for p, v in enumerate(vals):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise PBError('order[%d] = %r is not an integer' % (p, v))
        if not -1 <= v <= order_max:
            raise PBError('order[%d] = %d outside -1 .. %d (a bar floor; -1 = not ordered)' % (p, v, order_max))
    if all(int(v) == -1 for v in vals):
        return None
    vals = [int(v) for v in vals]
    return vals if owner is None else [vals[p] for p in owner]


ORDER_MAX = 255                    # the default dictionary's last bar id: for heads 0 and 1 the ids ARE the values (Bar k = k, Position k/64 = k in octuple_vocab.json)


def ordered_token(frow, sample, floor, prev, pad):
    """The token of ONE position under the time-ordered contract, for every decode path: the reference's `current_output = self.sample(x,
    i)` (model.py:46) becomes the ordered sample, followed by forced_token's overwrite of the given heads. floor: the row's bar floor (None
    or -1: the row is not ordered -- forced_token(frow, sample), nothing else); prev: the 8 ids of the decoder's input row at this position
    (the SOS row, the prime's last row, else the previous position's token after forcing); pad: the first special id per head.
    sample(order=(low, prev0, low1, given0)) is the path's own sampling of the position with the mask described by the tuple
    (PianoBartLM.sample_row): head 0's classes below low = max(floor, prev[0] if ordinary) are impossible; head 1's classes below low1 =
    prev[1] are impossible if the token's bar after forcing (given0 where forced gives one, else the sample) equals prev0 -- low1 is 0 (no
    mask) unless prev[0] and prev[1] are both ordinary. Given heads are never masked or changed, and the draws are forced_token's."""
    if floor is None or int(floor) < 0:
        return forced_token(frow, sample)
    p0, p1 = int(prev[0]), int(prev[1])
    bar = p0 < int(pad[0])
    low = max(int(floor), p0 if bar else 0)
    low1 = p1 if bar and p1 < int(pad[1]) else 0
    given0 = int(frow[0]) if frow is not None else -1
    return forced_token(frow, lambda: sample(order=(low, p0, low1, given0)))


def is_time_ordered(rows, start=0, floor=0):
    """Whether the emitted rows of a piece are in time order from `start` on (host, numpy). rows (S, 8) Octuple ids; the emitted rows are
    those in front of the first row whose bar id is special (>= 256: EOS or PAD). True iff the pairs (bar, position) of rows start - 1,
    start, .. (from row `start` itself for start = 0) are non-decreasing in lexicographic order and every bar of the rows from `start` on
    is >= floor."""
    x = rows.detach().cpu().numpy() if isinstance(rows, torch.Tensor) else np.asarray(rows)
    x = x.astype(np.int64)
    special = np.flatnonzero(x[:, 0] > ORDER_MAX)
    e = int(special[0]) if len(special) else len(x)
    if start >= e:
        return True
    if (x[start:e, 0] < floor).any():
        return False
    t = x[max(start - 1, 0):e, 0] * 1024 + x[max(start - 1, 0):e, 1]      # position ids stay below 1024
    return not (np.diff(t) < 0).any()


def _as_numpy(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _layout_of(layout_or_e2w):
    if layout_or_e2w is None:
        return ops.DEFAULT_LAYOUT, None
    if isinstance(layout_or_e2w, ops.Layout):
        return layout_or_e2w, None
    return ops.Layout.from_dict(layout_or_e2w), layout_or_e2w


def check_allow(allow, P, layout=None, owner=None):
    """The argument rules of allowed-class generation, on the host before any device work. allow: one mask per prompt -- a bool array or
    tensor (P, V), a list of P entries each a (V,) bool mask or None (= the row is free), or, for P = 1, one (V,) mask; V = layout.vocab,
    columns in model order (ops.Layout offsets), True = the class may be sampled. The six special ids of every head are set here (a row
    can always end); a head left without an ordinary class raises PBError naming it. owner (row -> prompt, check_samples): the indices are
    expanded to one per output row. Returns None for allow=None or masks that are True everywhere (the caller runs what it ran before),
    else (masks, index): the distinct masks packed to uint32 words, (n, ceil(V / 32)), bit c & 31 of word c >> 5 = column c, and one int per
    row, the row's mask or -1 = free. Equal masks share an entry."""
    if allow is None:
        return None
    lay = layout if layout is not None else ops.DEFAULT_LAYOUT
    V = int(lay.vocab)
    if isinstance(allow, (list, tuple)):
        entries = list(allow)
    else:
        a = _as_numpy(allow)
        if a.ndim == 1 and P == 1:
            entries = [a]
        elif a.ndim == 2:
            entries = list(a)
        else:
            raise PBError('allow of shape %s: expected (%d, %d) bools for %d prompt(s)%s' % (tuple(a.shape), P, V, P, ', or (%d,)' % V if P == 1 else ''))
    if len(entries) != P:
        raise PBError('allow has %d entries for %d prompt(s)' % (len(entries), P))
    keys, masks, index = {}, [], []
    for p, m in enumerate(entries):
        if m is None:
            index.append(-1)
            continue
        try:
            m = _as_numpy(m)
        except Exception:
            raise PBError('allow[%d] = %r is neither None nor a bool mask' % (p, m))
        if m.dtype != np.bool_:
            raise PBError('allow[%d] must be a bool mask (got %s)' % (p, m.dtype))
        if m.shape != (V,):
            raise PBError('allow[%d] of shape %s: expected (%d,), one bool per vocabulary column' % (p, tuple(m.shape), V))
        m = m.copy()
        for h in range(8):
            o, n, pad = lay.seg_off[h], lay.sizes[h], lay.pad8[h]
            if not m[o:o + pad].any():
                raise PBError('allow[%d] leaves head %d (%s) without an ordinary class' % (p, h, ops.CLASS_NAMES[h]))
            m[o + pad:o + n] = True
        if m.all():
            index.append(-1)
            continue
        key = m.tobytes()
        if key not in keys:
            keys[key] = len(masks)
            masks.append(m)
        index.append(keys[key])
    if not masks:
        return None
    words = (V + 31) // 32
    bits = np.zeros((len(masks), words * 32), dtype=np.uint8)
    bits[:, :V] = np.stack(masks)
    packed = np.ascontiguousarray(np.packbits(bits, axis=1, bitorder='little')).view('<u4').astype(np.uint32).reshape(len(masks), words)
    return packed, (index if owner is None else [index[p] for p in owner])


def unpack_allow(allow, vocab):
    """The masks of check_allow's result as bool tensors: one (vocab,) torch.bool per ROW (True = allowed), None for a free row."""
    if allow is None:
        return None
    packed, index = allow
    bits = np.unpackbits(np.ascontiguousarray(packed).astype('<u4').view(np.uint8), axis=1, bitorder='little')[:, :vocab].astype(bool)
    ms = [torch.from_numpy(np.ascontiguousarray(b)) for b in bits]
    return [ms[i] if i >= 0 else None for i in index]


def _slice_allow(allow, a, b):
    """check_allow's result for the rows a .. b - 1 (the table stays whole); None where they are all free."""
    if allow is None or all(i < 0 for i in allow[1][a:b]):
        return None
    return allow[0], list(allow[1][a:b])


_SCALES = dict(major=(0, 2, 4, 5, 7, 9, 11), minor=(0, 2, 3, 5, 7, 8, 10))
_TONICS = {'C': 0, 'C#': 1, 'Db': 1, 'D': 2, 'D#': 3, 'Eb': 3, 'E': 4, 'F': 5, 'F#': 6, 'Gb': 6, 'G': 7, 'G#': 8, 'Ab': 8, 'A': 9, 'A#': 10, 'Bb': 10, 'B': 11}


def _range2(name, r):
    try:
        lo, hi = r
        lo, hi = float(lo), float(hi)
    except (TypeError, ValueError):
        raise PBError('allow_mask: %s must be a pair (lo, hi) of numbers (got %r)' % (name, r))
    if not lo < hi:
        raise PBError('allow_mask: %s = %r is an empty range (lo <= value < hi)' % (name, r))
    return lo, hi


def allow_mask(layout_or_e2w=None, key=None, pitch_range=None, instruments=None, velocity=None, tempo=None, max_duration=None, timesig=None,
               heads=None):
    """One (V,) bool allow mask (check_allow's input) built from a dictionary's NAMES (host, numpy). layout_or_e2w: the dictionary's event ->
    word half (the reference's e2w: {class: {word: id}}; PianoBart.e2w), so any legal dictionary works; an ops.Layout (or None: the default
    one) serves the raw form `heads` only, since a layout has no names. A head without a rule stays free; several rules on one head
    intersect; the special ids of every head are always set.
      key='C:major'        tonic C, C#, Db, D, .. B and mode major or minor (natural minor): the melodic 'Pitch k' with k % 12 in the scale
      pitch_range=(lo, hi) the melodic 'Pitch k' with lo <= k < hi. key and pitch_range both remove the 'Pitch percussion k' classes
      instruments={..}     a set of 'Instrument <x>' words given by <x> (0, '0', 'percussion') or in full
      timesig={..}         a set of 'TimeSig <x>' words given by <x> ('4/4') or in full; an int is the id itself
      velocity=(lo, hi)    the 'Velocity v' with lo <= v < hi;  tempo=(lo, hi): the 'Tempo t' with lo <= t < hi (beats per minute)
      max_duration=N       the duration ids 0 .. N
      heads={h: ids}       the raw form: head h admits exactly these ordinary ids
    PBError: an unknown tonic, mode, word or head, an id outside its head, an empty range, or a head left without an ordinary class."""
    lay, e2w = _layout_of(layout_or_e2w)
    ok = [np.ones(lay.pad8[h], dtype=bool) for h in range(8)]

    def names(h):
        if e2w is None:
            raise PBError('allow_mask: the rule on %s needs the dictionary\'s names: pass e2w (PianoBart.e2w), not a Layout' % ops.CLASS_NAMES[h])
        cls = ops.CLASS_NAMES[h]
        return [(w[len(cls) + 1:], int(i)) for w, i in e2w[cls].items() if int(i) < lay.pad8[h]]

    def numbered(h):
        out = []
        for rest, i in names(h):
            try:
                out.append((float(rest), i))
            except ValueError:
                pass
        return out

    def keep(h, ids, what):
        m = np.zeros(lay.pad8[h], dtype=bool)
        m[list(ids)] = True
        ok[h] &= m
        if not ok[h].any():
            raise PBError('allow_mask: %s leaves head %d (%s) without an ordinary class' % (what, h, ops.CLASS_NAMES[h]))

    def named_set(h, items, what):
        tab = dict(names(h))
        cls = ops.CLASS_NAMES[h]
        try:
            items = list(items) if not isinstance(items, (str, int, np.integer)) else [items]
        except TypeError:
            raise PBError('allow_mask: %s must be a set of names or numbers (got %r)' % (what, items))
        if not items:
            raise PBError('allow_mask: %s is empty' % what)
        ids = []
        for it in items:
            if h == 6 and isinstance(it, (int, np.integer)) and not isinstance(it, bool):
                if not 0 <= int(it) < lay.pad8[h]:
                    raise PBError('allow_mask: %s: id %d outside 0 .. %d' % (what, int(it), lay.pad8[h] - 1))
                ids.append(int(it))
                continue
            w = str(it)
            w = w[len(cls) + 1:] if w.startswith(cls + ' ') else w
            if w not in tab:
                raise PBError('allow_mask: %s: the dictionary has no word %r' % (what, '%s %s' % (cls, w)))
            ids.append(tab[w])
        keep(h, ids, what)

    if key is not None:
        try:
            tonic, mode = str(key).split(':')
        except ValueError:
            raise PBError('allow_mask: key %r is not TONIC:MODE (C:major, A:minor, ..)' % (key,))
        if tonic not in _TONICS:
            raise PBError('allow_mask: unknown tonic %r (%s)' % (tonic, ', '.join(_TONICS)))
        if mode not in _SCALES:
            raise PBError('allow_mask: unknown mode %r (major, minor)' % mode)
        pcs = {(_TONICS[tonic] + d) % 12 for d in _SCALES[mode]}
        keep(3, [i for rest, i in names(3) if rest.isdigit() and int(rest) % 12 in pcs], 'key %s' % key)
    if pitch_range is not None:
        lo, hi = _range2('pitch_range', pitch_range)
        keep(3, [i for rest, i in names(3) if rest.isdigit() and lo <= int(rest) < hi], 'pitch_range %r' % (pitch_range,))
    if instruments is not None:
        named_set(2, instruments, 'instruments')
    if timesig is not None:
        named_set(6, timesig, 'timesig')
    if velocity is not None:
        lo, hi = _range2('velocity', velocity)
        keep(5, [i for v, i in numbered(5) if lo <= v < hi], 'velocity %r' % (velocity,))
    if tempo is not None:
        lo, hi = _range2('tempo', tempo)
        keep(7, [i for v, i in numbered(7) if lo <= v < hi], 'tempo %r' % (tempo,))
    if max_duration is not None:
        if isinstance(max_duration, bool) or not isinstance(max_duration, (int, np.integer)) or max_duration < 0:
            raise PBError('allow_mask: max_duration must be a duration id >= 0 (got %r)' % (max_duration,))
        keep(4, range(min(int(max_duration) + 1, lay.pad8[4])), 'max_duration %d' % max_duration)
    if heads is not None:
        for h, ids in dict(heads).items():
            if isinstance(h, bool) or not isinstance(h, (int, np.integer)) or not 0 <= h < 8:
                raise PBError('allow_mask: heads: %r is not a head 0 .. 7' % (h,))
            ids = [int(v) for v in _as_numpy(ids).reshape(-1)]
            if any(not 0 <= v < lay.pad8[h] for v in ids):
                raise PBError('allow_mask: heads[%d]: an id outside the ordinary ids 0 .. %d of %s' % (h, lay.pad8[h] - 1, ops.CLASS_NAMES[h]))
            if not ids:
                raise PBError('allow_mask: heads[%d] is empty: it leaves head %d (%s) without an ordinary class' % (h, h, ops.CLASS_NAMES[h]))
            keep(int(h), ids, 'heads[%d]' % h)
    mask = np.ones(lay.vocab, dtype=bool)
    for h in range(8):
        mask[lay.seg_off[h]:lay.seg_off[h] + lay.pad8[h]] = ok[h]
    return mask


def add_allow_flags(ap):
    """The command-line form of allow_mask, shared by eval_generation, demo and tools/decode_batch_bench.py: one mask for every row."""
    ap.add_argument('--key', type=str, default=None, metavar='TONIC:MODE', help='allowed classes: melodic pitches of this key only (C:major, A:minor, ..)')
    ap.add_argument('--pitch_range', type=str, default=None, metavar='LO:HI', help='allowed classes: melodic pitches LO <= k < HI only')
    ap.add_argument('--instruments', type=str, default=None, metavar='I[,I...]', help='allowed classes: these instruments only (numbers or "percussion")')
    ap.add_argument('--tempo', type=str, default=None, metavar='LO:HI', help='allowed classes: tempo classes with LO <= beats per minute < HI only')
    ap.add_argument('--max_duration', type=int, default=None, metavar='N', help='allowed classes: duration ids 0 .. N only')
    ap.add_argument('--velocity', type=str, default=None, metavar='LO:HI', help='allowed classes: velocity classes with LO <= velocity < HI only')


ALLOW_FLAGS = ('key', 'pitch_range', 'instruments', 'tempo', 'max_duration', 'velocity')


def allow_flags_given(args):
    """The allow flags (add_allow_flags) the arguments set, by name."""
    return [f for f in ALLOW_FLAGS if getattr(args, f, None) is not None]


def allow_from_args(args, e2w):
    """The one (V,) allow mask the flags of add_allow_flags describe, built from the dictionary e2w; None where no flag is given. PBError
    for a flag that is not of its form, and allow_mask's."""
    if not allow_flags_given(args):
        return None

    def pair(flag):
        v = getattr(args, flag, None)
        if v is None:
            return None
        try:
            lo, hi = (float(t) for t in str(v).split(':'))
        except ValueError:
            raise PBError('--%s takes LO:HI, two numbers (got %r)' % (flag, v))
        return lo, hi
    inst = getattr(args, 'instruments', None)
    return allow_mask(e2w, key=getattr(args, 'key', None), pitch_range=pair('pitch_range'), tempo=pair('tempo'), velocity=pair('velocity'),
                      instruments=[t.strip() for t in str(inst).split(',') if t.strip()] if inst is not None else None,
                      max_duration=getattr(args, 'max_duration', None))


def allowed_token(frow, sample, allow, floor, prev, pad):
    """The token of ONE position under the allowed-class contract, for every decode path: ordered_token (and through it forced_token) with
    the path's sample() given the row's mask. allow: the row's (V,) bool mask, True = the class may be sampled (None: the row is free --
    ordered_token(frow, sample, floor, prev, pad), nothing else). sample(allow=mask[, order=...]) is the path's own sampling of the position
    with the masked columns at -inf in front of the softmax (PianoBartLM.sample_row). Given heads are written as given, inside the mask or
    not; a position whose 8 heads are given draws nothing; the draws are forced_token's."""
    if allow is None:
        return ordered_token(frow, sample, floor, prev, pad)
    return ordered_token(frow, lambda **kw: sample(allow=allow, **kw), floor, prev, pad)


def is_allowed(rows, mask, start=0, forced=None, layout=None):
    """Whether every emitted, non-given head of the rows from `start` on is inside the mask (host, numpy). rows (S, 8) Octuple ids; the
    emitted rows are those in front of the first row whose bar id is special. mask (V,) bools in model column order (special ids count as
    allowed, as check_allow sets them); forced (S, 8) or None: the row's forced table -- a given head (>= 0) is not tested."""
    lay = layout if layout is not None else ops.DEFAULT_LAYOUT
    x = _as_numpy(rows).astype(np.int64)
    m = _as_numpy(mask).astype(bool)
    special = np.flatnonzero(x[:, 0] >= lay.pad8[0])
    e = int(special[0]) if len(special) else len(x)
    if start >= e:
        return True
    x = x[start:e]
    off, pad = np.asarray(lay.seg_off[:8], dtype=np.int64), np.asarray(lay.pad8, dtype=np.int64)
    ok = m[np.clip(x, 0, np.asarray(lay.sizes) - 1) + off] | (x >= pad)
    if forced is not None:
        ok |= _as_numpy(forced)[start:e] >= 0
    return bool(ok.all())


def _unpack_bits(packed, vocab):
    """(n, V) bool rows of a table packed as check_allow packs it."""
    return np.unpackbits(np.ascontiguousarray(packed).astype('<u4').view(np.uint8), axis=1, bitorder='little')[:, :vocab].astype(bool)


def _pack_bits(masks, V):
    words = (V + 31) // 32
    bits = np.zeros((len(masks), words * 32), dtype=np.uint8)
    bits[:, :V] = np.stack(masks)
    return np.ascontiguousarray(np.packbits(bits, axis=1, bitorder='little')).view('<u4').astype(np.uint32).reshape(len(masks), words)


def _schedule_entries(sched, nbar, who):
    """One bar schedule in either argument form -> {bar: mask or None}, the bars checked."""
    if isinstance(sched, dict):
        items = list(sched.items())
    else:
        try:
            items = list(enumerate(sched))
        except TypeError:
            raise PBError('%s = %r is neither None, a dict {bar: mask} nor a sequence of masks' % (who, sched))
        if len(items) > nbar:
            raise PBError('%s has %d entries: a schedule holds at most one per ordinary bar id 0 .. %d' % (who, len(items), nbar - 1))
    out = {}
    for k, m in items:
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= int(k) < nbar:
            raise PBError('%s: bar %r is not an ordinary bar id 0 .. %d' % (who, k, nbar - 1))
        out[int(k)] = m
    return out


def check_bar_allow(bar_allow, allow, P, layout=None, owner=None):
    """The argument rules of bar schedules, on the host before any device work. bar_allow: one schedule per prompt -- a list of P entries,
    each None (no schedule), a dict {bar id: (V,) bool mask} or a sequence of at most pad[0] masks / None indexed by bar id; for P = 1 one
    schedule by itself will do. allow: the call's `allow` argument as check_allow takes it (the rows' own masks). Every bar mask is
    intersected with its prompt's row mask and gets the special ids of every head set; a (row mask, bar mask) pair that leaves a head
    without an ordinary class raises PBError naming the prompt, the bar and the head. An entry that removes nothing beyond the row mask
    is no entry. owner (row -> prompt, check_samples): the indices are expanded to one per output row.
    Returns None where no schedule is in force (bar_allow None, or no entry that removes a class: the caller runs what it ran before,
    check_allow included), else (masks, index, table, sched): masks = the distinct masks of rows AND bars packed as check_allow packs
    them, (n, ceil(V / 32)) uint32; index = one int per row, the row's own mask or -1 = free; table = the distinct schedules, (n_sched,
    pad[0]) int32, entry k = the mask in force for heads 1 .. 7 of a token of bar k or -1 = the row's own; sched = one int per row, the
    row's schedule or -1 = none. (masks, index) is check_allow's result for the call, with the bars' masks appended to the table."""
    if bar_allow is None:
        return None
    lay = layout if layout is not None else ops.DEFAULT_LAYOUT
    V, nbar = int(lay.vocab), int(lay.pad8[0])
    is_mask = lambda m: isinstance(m, (np.ndarray, torch.Tensor)) and m.ndim == 1
    if isinstance(bar_allow, dict) or (P == 1 and isinstance(bar_allow, (list, tuple)) and any(is_mask(m) for m in bar_allow)):
        bar_allow = [bar_allow]
    if not isinstance(bar_allow, (list, tuple)):
        raise PBError('bar_allow must be a list of %d schedules, one per prompt (got %r)' % (P, type(bar_allow).__name__))
    if len(bar_allow) != P:
        raise PBError('bar_allow has %d entries for %d prompt(s)' % (len(bar_allow), P))
    base = check_allow(allow, P, lay)                        # the rows' own masks: the argument rules and refusals of the call without a schedule
    rows = list(_unpack_bits(base[0], V)) if base is not None else []
    index = list(base[1]) if base is not None else [-1] * P
    keys = {m.tobytes(): i for i, m in enumerate(rows)}
    masks = list(rows)
    skeys, table, sched = {}, [], []
    for p, sc in enumerate(bar_allow):
        if sc is None:
            sched.append(-1)
            continue
        own = rows[index[p]] if index[p] >= 0 else np.ones(V, dtype=bool)
        line = np.full(nbar, -1, dtype=np.int32)
        for k, m in sorted(_schedule_entries(sc, nbar, 'bar_allow[%d]' % p).items()):
            if m is None:
                continue
            try:
                m = _as_numpy(m)
            except Exception:
                raise PBError('bar_allow[%d], bar %d: %r is neither None nor a bool mask' % (p, k, m))
            if m.dtype != np.bool_:
                raise PBError('bar_allow[%d], bar %d: the mask must be bool (got %s)' % (p, k, m.dtype))
            if m.shape != (V,):
                raise PBError('bar_allow[%d], bar %d: mask of shape %s, expected (%d,), one bool per vocabulary column' % (p, k, tuple(m.shape), V))
            m = m & own
            for h in range(8):
                o, n, pad = lay.seg_off[h], lay.sizes[h], lay.pad8[h]
                if h and not m[o:o + pad].any():                 # head 0 never sees the schedule
                    raise PBError('bar_allow[%d]: the row mask and the mask of bar %d leave head %d (%s) without an ordinary class'
                                  % (p, k, h, ops.CLASS_NAMES[h]))
                m[o + pad:o + n] = True
            m[lay.seg_off[0]:lay.seg_off[1]] = own[lay.seg_off[0]:lay.seg_off[1]]     # ... so its columns stay the row's: one canonical form per effect
            if (m == own).all():
                continue
            key = m.tobytes()
            if key not in keys:
                keys[key] = len(masks)
                masks.append(m)
            line[k] = keys[key]
        if (line < 0).all():
            sched.append(-1)
            continue
        key = line.tobytes()
        if key not in skeys:
            skeys[key] = len(table)
            table.append(line)
        sched.append(skeys[key])
    if not table:
        return None
    if owner is not None:
        index, sched = [index[p] for p in owner], [sched[p] for p in owner]
    return _pack_bits(masks, V), index, np.ascontiguousarray(np.stack(table), dtype=np.int32), sched


def unpack_schedule(plan, vocab):
    """The schedules of check_bar_allow's result as the host's decode loops take them: per ROW None, or a list of pad[0] entries, entry k
    = the (vocab,) torch.bool mask in force for heads 1 .. 7 of a token of bar k, None = the row's own mask."""
    if plan is None:
        return None
    ms = [torch.from_numpy(np.ascontiguousarray(b)) for b in _unpack_bits(plan[0], vocab)]
    lines = [[ms[e] if e >= 0 else None for e in line] for line in plan[2]]
    return [lines[i] if i >= 0 else None for i in plan[3]]


def _slice_schedule(plan, a, b):
    """check_bar_allow's result for the rows a .. b - 1 (both tables stay whole); None where none of them has a schedule."""
    if plan is None or all(i < 0 for i in plan[3][a:b]):
        return None
    return plan[0], list(plan[1][a:b]), plan[2], list(plan[3][a:b])


def scheduled_token(frow, sample, allow, sched, floor, prev, pad):
    """The token of ONE position under the bar-schedule contract, for every decode path: allowed_token (and through it ordered_token and
    forced_token) with the path's sample() told the row's schedule and head 0's given id. sched: the row's entry of unpack_schedule (None:
    no schedule -- allowed_token(frow, sample, allow, floor, prev, pad), nothing else). sample(sched=(masks_by_bar, given0)[, allow=..,
    order=..]) is the path's own sampling of the position: head 0 as ever, heads 1 .. 7 from the mask of bar b0 = given0 if >= 0 else the
    sampled bar (PianoBartLM.sample_row). Given heads are written as given; the draws are forced_token's."""
    if sched is None:
        return allowed_token(frow, sample, allow, floor, prev, pad)
    given0 = int(frow[0]) if frow is not None else -1
    return allowed_token(frow, lambda **kw: sample(sched=(sched, given0), **kw), allow, floor, prev, pad)


def follows_schedule(rows, schedule, start=0, forced=None, layout=None):
    """Whether every emitted, non-given head 1 .. 7 of the rows from `start` on is inside the mask its row's bar has in `schedule` (host,
    numpy). rows (S, 8) Octuple ids; the emitted rows are those in front of the first row whose bar id is special. schedule: a dict {bar:
    (V,) bools} or a sequence of masks / None by bar id (check_bar_allow's forms, the masks as given: is_allowed tests the row's own);
    a bar without an entry tests nothing, special ids count as allowed. forced (S, 8) or None: a given head (>= 0) is not tested."""
    lay = layout if layout is not None else ops.DEFAULT_LAYOUT
    x = _as_numpy(rows).astype(np.int64)
    special = np.flatnonzero(x[:, 0] >= lay.pad8[0])
    e = int(special[0]) if len(special) else len(x)
    ent = {k: _as_numpy(m).astype(bool) for k, m in _schedule_entries(schedule, int(lay.pad8[0]), 'schedule').items() if m is not None}
    off, pad, top = np.asarray(lay.seg_off[:8], dtype=np.int64), np.asarray(lay.pad8, dtype=np.int64), np.asarray(lay.sizes) - 1
    fr = _as_numpy(forced) if forced is not None else None
    for i in range(start, e):
        m = ent.get(int(x[i, 0]))
        if m is None:
            continue
        ok = m[np.clip(x[i], 0, top) + off] | (x[i] >= pad)
        if fr is not None:
            ok |= fr[i] >= 0
        if not ok[1:].all():
            return False
    return True


_CHORDS = {'maj': (0, 4, 7), 'min': (0, 3, 7), 'dim': (0, 3, 6), 'aug': (0, 4, 8), '7': (0, 4, 7, 10), 'maj7': (0, 4, 7, 11), 'min7': (0, 3, 7, 10),
           'sus2': (0, 2, 7), 'sus4': (0, 5, 7)}


def chord_mask(e2w, chord):
    """One (V,) bool mask (a bar's entry of a schedule, or an allow mask) that keeps the melodic 'Pitch k' whose pitch class is a tone of the
    chord and removes the 'Pitch percussion k' classes; every other head stays free. chord = 'ROOT:QUALITY': roots C, C#, Db, D, .. B
    (allow_mask's tonics), qualities maj, min, dim, aug, 7, maj7, min7, sus2, sus4. e2w: the dictionary's event -> word half (PianoBart.e2w).
    PBError: a string of another form, an unknown root or quality (the known ones listed), or a dictionary without such a pitch."""
    try:
        root, quality = str(chord).split(':')
    except ValueError:
        raise PBError('chord_mask: %r is not ROOT:QUALITY (C:maj, A:min7, ..)' % (chord,))
    if root not in _TONICS:
        raise PBError('chord_mask: unknown root %r (%s)' % (root, ', '.join(_TONICS)))
    if quality not in _CHORDS:
        raise PBError('chord_mask: unknown quality %r (%s)' % (quality, ', '.join(_CHORDS)))
    lay, cls = ops.Layout.from_dict(e2w), ops.CLASS_NAMES[3]
    pcs = {(_TONICS[root] + d) % 12 for d in _CHORDS[quality]}
    ids = [int(i) for w, i in e2w[cls].items() if int(i) < lay.pad8[3] and w[len(cls) + 1:].isdigit() and int(w[len(cls) + 1:]) % 12 in pcs]
    if not ids:
        raise PBError('chord_mask: the dictionary has no melodic pitch on a tone of %s' % chord)
    return allow_mask(e2w, heads={3: ids})


def chord_schedule(e2w, chords, bars_per_chord=1, start_bar=0, repeat=True, n_bars=None):
    """A bar schedule (check_bar_allow's sequence form: pad[0] entries, a chord_mask or None) from a chord progression: bar start_bar +
    j takes chord (j // bars_per_chord) of `chords`, for j = 0 .. n_bars - 1 (None: up to the dictionary's last bar id). repeat: the
    progression starts over when it ends; otherwise the bars behind it have no entry. Bars in front of start_bar have none."""
    chords = [chords] if isinstance(chords, str) else list(chords)
    if not chords:
        raise PBError('chord_schedule: no chord named')
    for name, v, lo in (('bars_per_chord', bars_per_chord, 1), ('start_bar', start_bar, 0)) + ((('n_bars', n_bars, 0),) if n_bars is not None else ()):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo:
            raise PBError('chord_schedule: %s must be an integer >= %d (got %r)' % (name, lo, v))
    nbar = int(ops.Layout.from_dict(e2w).pad8[0])
    ms = {}
    out = [None] * nbar
    for k in range(int(start_bar), nbar if n_bars is None else min(nbar, int(start_bar) + int(n_bars))):
        c = (k - int(start_bar)) // int(bars_per_chord)
        if c >= len(chords) and not repeat:
            break
        name = chords[c % len(chords)]
        if name not in ms:
            ms[name] = chord_mask(e2w, name)
        out[k] = ms[name]
    return out


def add_schedule_flags(ap):
    """The command-line form of chord_schedule, shared by eval_generation, demo and tools/decode_batch_bench.py."""
    ap.add_argument('--chords', type=str, default=None, metavar='ROOT:QUALITY[,...]', help='bar schedule: the pitches of bar after bar follow this chord '
                    'progression (C:maj,G:maj,A:min,F:maj), repeated to the end of the piece')
    ap.add_argument('--bars_per_chord', type=int, default=1, metavar='N', help='--chords: every chord holds for N bars')
    ap.add_argument('--chord_start', type=int, default=None, metavar='B', help='--chords: the bar of the first chord (default: 0, or with --prime the bar '
                    'after the one each piece\'s prime ends in)')


def schedule_from_args(args, e2w, prime=None):
    """The bar schedule the flags of add_schedule_flags describe for ONE piece, built from the dictionary e2w; None where --chords is not
    given. prime: the piece's prime rows (k, 8) or None -- without --chord_start the first chord sits in the bar after the one the prime
    ends in (bar 0 for an unprimed piece). PBError for flags that are not of their form, and chord_schedule's."""
    chords = getattr(args, 'chords', None)
    if chords is None:
        if getattr(args, 'chord_start', None) is not None or getattr(args, 'bars_per_chord', 1) != 1:
            raise PBError('--chord_start and --bars_per_chord need --chords')
        return None
    names = [t.strip() for t in str(chords).split(',') if t.strip()]
    start = getattr(args, 'chord_start', None)
    if start is None:
        start = int(_as_numpy(prime)[-1, 0]) + 1 if prime is not None and len(prime) else 0
    return chord_schedule(e2w, names, bars_per_chord=getattr(args, 'bars_per_chord', 1), start_bar=int(start))


def stop_vector(pad_cpu, s):
    """The 8 thresholds of ONE row's stop test, for every decode path: the reference's `(current_output >= pad).any()` (model.py:47)
    becomes `(current_output >= stop_vector(pad, s)).any()` -- pad with its head 0 lowered to the row's stop bar s, so the one comparison
    covers the special ids and the bar. s None (or pad[0]): pad itself."""
    if s is None or int(s) == int(pad_cpu[0]):
        return pad_cpu
    v = pad_cpu.clone()
    v[0] = int(s)
    return v


def end_reason(tok, pad_cpu):
    """Why a token that tripped a row's stop test ended the row: 'special' (a special id in any head) or 'bar' (its bar reached the stop)."""
    return 'special' if bool((tok >= pad_cpu).any()) else 'bar'


def stop_after_bars(prefix_rows, n, pad0):
    """The stop bar of "write n more bars": with q the bar of the prime's last row (-1 for an unprimed row: prefix_rows None or empty),
    min(q + 1 + n, pad0) -- the row finishes the bar it is in and writes n whole new bars. prefix_rows (k, 8) Octuple ids; n >= 0."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 0:
        raise PBError('bars: the number of new bars must be an integer >= 0 (got %r)' % (n,))
    rows = None if prefix_rows is None else (prefix_rows.detach().cpu().numpy() if isinstance(prefix_rows, torch.Tensor) else np.asarray(prefix_rows))
    q = int(rows[-1, 0]) if rows is not None and len(rows) else -1
    return min(q + 1 + int(n), int(pad0))


def _anchor_list(a, who):
    """One anchor list in any argument form -> (n, 8) int64 numpy (n may be 0)."""
    try:
        x = _as_numpy(a)
    except Exception:
        raise PBError('%s = %r is neither None nor an (n, 8) array of Octuple ids' % (who, a))
    if x.size == 0:
        return np.zeros((0, 8), dtype=np.int64)
    if x.ndim != 2 or x.shape[1] != 8:
        raise PBError('%s of shape %s: expected (n, 8), complete Octuple rows' % (who, tuple(x.shape)))
    if x.dtype == np.bool_ or not np.issubdtype(x.dtype, np.integer):
        raise PBError('%s: anchor ids must be integers (got %s)' % (who, x.dtype))
    return x.astype(np.int64)


def check_anchors(anchors, P, S, pad, ks=None, rows=None, stop=None, order=None, forced=None, max_new=None, owner=None):
    """The argument rules of anchored generation, on the host before any device work ("Anchored notes"). anchors: one
    anchor list per prompt -- a list of P entries, each None / empty (a free prompt) or (n, 8) complete Octuple rows of ordinary ids,
    non-decreasing in (bar, position); for P = 1 one (n, 8) array by itself will do. pad: the first special id per head. ks / rows: the
    prefix lengths and rows of check_prefix; stop / order: check_stop's / check_order's results, one entry per ROW (owner: row -> prompt,
    check_samples) or None; forced: check_forced's result; max_new: the call's. Raises PBError naming the prompt and the rule for: an id
    that is negative or >= pad[h]; anchors out of (bar, position) order; a bar below the row's floor max(order, 0) or >= its stop bar; an
    anchor in front of the last row of the prefix; more anchors than positions left in the window; anchors together with forced tokens.
    Returns None where no prompt has an anchor (the caller runs what it ran before), else (lists, order): lists = one entry per ROW, an
    (n, 8) int64 tensor or None; order = one bar floor per ROW with every anchored row at max(order, 0) -- anchors imply time order."""
    if anchors is None:
        return None
    pad = np.asarray(pad, dtype=np.int64).reshape(8)
    if P == 1 and not (isinstance(anchors, (list, tuple)) and len(anchors) == 1 and (anchors[0] is None or np.ndim(_as_numpy(anchors[0])) == 2)):
        anchors = [anchors]
    if not isinstance(anchors, (list, tuple)):
        raise PBError('anchors must be a list of %d anchor lists, one per prompt (got %r)' % (P, type(anchors).__name__))
    if len(anchors) != P:
        raise PBError('anchors has %d entries for %d prompt(s)' % (len(anchors), P))
    lists = [None if a is None else _anchor_list(a, 'anchors[%d]' % p) for p, a in enumerate(anchors)]
    lists = [a if a is not None and len(a) else None for a in lists]
    if all(a is None for a in lists):
        return None
    if forced is not None:
        raise PBError('anchors do not combine with forced tokens in one call: position-indexed and time-indexed givens do not combine')
    owner = list(range(P)) if owner is None else list(owner)
    first = {p: r for r, p in reversed(list(enumerate(owner)))}           # a prompt's rows share its stop and floor
    for p, a in enumerate(lists):
        if a is None:
            continue
        bad = np.argwhere((a < 0) | (a >= pad))
        if len(bad):
            i, h = int(bad[0, 0]), int(bad[0, 1])
            raise PBError('anchors of prompt %d, anchor %d, head %d: id %d is not an ordinary event (0 <= id < %d)' % (p, i, h, int(a[i, h]), int(pad[h])))
        t = a[:, 0] * (int(pad[1]) + 1) + a[:, 1]
        if (np.diff(t) < 0).any():
            i = int(np.flatnonzero(np.diff(t) < 0)[0]) + 1
            raise PBError('anchors of prompt %d: anchor %d at (bar %d, position %d) lies in front of anchor %d at (%d, %d): anchors come in (bar, position) order'
                          % (p, i, int(a[i, 0]), int(a[i, 1]), i - 1, int(a[i - 1, 0]), int(a[i - 1, 1])))
        r = first.get(p)
        floor = max(int(order[r]), 0) if order is not None and r is not None else 0
        sb = int(stop[r]) if stop is not None and r is not None else int(pad[0])
        out = np.flatnonzero((a[:, 0] < floor) | (a[:, 0] >= sb))
        if len(out):
            i = int(out[0])
            raise PBError('anchors of prompt %d: anchor %d sits in bar %d, outside the bars %d .. %d the row may write (its floor and its stop bar)'
                          % (p, i, int(a[i, 0]), floor, sb - 1))
        k = int(ks[p]) if ks is not None else 0
        if k:
            q = _as_numpy(rows[p][k - 1]).astype(np.int64)
            if (int(a[0, 0]), int(a[0, 1])) < (int(q[0]), int(q[1])):
                raise PBError('anchors of prompt %d: anchor 0 at (bar %d, position %d) lies in front of the last row of the prefix at (%d, %d)'
                              % (p, int(a[0, 0]), int(a[0, 1]), int(q[0]), int(q[1])))
        left = (S if max_new is None else max(0, min(S, k + int(max_new)))) - k
        if len(a) > left:
            raise PBError('anchors of prompt %d: %d anchors for the %d positions left in the window (S = %d, prefix %d%s)'
                          % (p, len(a), left, S, k, '' if max_new is None else ', max_new %d' % int(max_new)))
    out = [torch.from_numpy(lists[p]) if lists[p] is not None else None for p in owner]
    floors = [int(v) for v in order] if order is not None else [-1] * len(owner)
    return out, [max(f, 0) if a is not None else f for f, a in zip(floors, out)]


def anchored_token(sample, anchors, k, stop_vector, pad):
    """The token of ONE position under the anchored-notes contract, for every decode path -- the single definition of the rule. sample: the
    candidate, the 8 ids the position sampled as it would without anchors (scheduled_token's result); anchors: the row's (n, 8) int64
    tensor or None; k: the anchors written so far; stop_vector: the row's 8 stop thresholds (stop_vector()); pad: the first special id per
    head. Returns (token, k'): while k < n, a candidate that ends the row (any head >= its threshold) or whose (bar, position) has reached
    A[k]'s gives way to A[k], all 8 heads, and k' = k + 1 -- the candidate is discarded, its draws stay consumed, and the caller's stop
    test cannot trip on an anchor (its ids are ordinary and its bar is below the stop bar: check_anchors). Otherwise (sample, k)."""
    if anchors is None or k >= len(anchors):
        return sample, k
    a = anchors[k]
    ends = bool((sample >= stop_vector).any()) or bool((sample >= pad).any())
    if ends or (int(sample[0]), int(sample[1])) >= (int(a[0]), int(a[1])):
        return a.clone(), k + 1
    return sample, k


def follows_anchors(rows, anchors, start=0, layout=None):
    """Whether a generated row kept its anchors (host, numpy). rows (S, 8) Octuple ids; the emitted rows are those in front of the first row
    whose bar id is special. anchors (n, 8). Returns (ok, placed): placed = how many anchors, in order, occur as whole rows among the
    emitted rows from `start` on (a subsequence match, each anchor at the first row that equals it behind its predecessor); ok = all n
    do and the (bar, position) pairs of rows start - 1, start, .. are non-decreasing (is_time_ordered's test)."""
    lay = layout if layout is not None else ops.DEFAULT_LAYOUT
    x = _as_numpy(rows).astype(np.int64)
    a = _anchor_list(anchors, 'anchors') if anchors is not None else np.zeros((0, 8), dtype=np.int64)
    special = np.flatnonzero(x[:, 0] >= lay.pad8[0])
    e = int(special[0]) if len(special) else len(x)
    placed = 0
    for i in range(start, e):
        if placed < len(a) and np.array_equal(x[i], a[placed]):
            placed += 1
    lo = max(start - 1, 0)
    t = x[lo:e, 0] * (int(lay.pad8[1]) + 1) + x[lo:e, 1]
    ordered = start >= e or not (np.diff(t) < 0).any()
    return bool(placed == len(a) and ordered), placed


def anchor_rows(piece, which, e2w=None):
    """The rows of a piece to keep as anchors (host, numpy). piece (n, 8) Octuple ids (the rows in front of the first special bar id count);
    which: 'skyline' = of every (bar, position) the melodic note of highest pitch, 'bass' = the lowest -- percussion notes never -- or a
    boolean selector over the piece's rows. e2w: the dictionary's event -> word half (PianoBart.e2w): a pitch word 'Pitch k' is melodic
    with value k, 'Pitch percussion k' is not; None: the default dictionary, where ids 0 .. 127 are the melodic pitches. Returns the
    selected rows (m, 8) int64 in (bar, position) order (a stable sort: rows of one time keep the piece's order)."""
    x = _as_numpy(piece)
    if x.ndim != 2 or x.shape[1] != 8:
        raise PBError('anchor_rows: piece of shape %s, expected (n, 8)' % (tuple(x.shape),))
    x = x.astype(np.int64)
    lay = ops.Layout.from_dict(e2w) if e2w is not None else ops.DEFAULT_LAYOUT
    special = np.flatnonzero((x >= np.asarray(lay.pad8, dtype=np.int64)).any(1))
    x = x[:int(special[0])] if len(special) else x
    if not isinstance(which, str):
        sel = _as_numpy(which)
        if sel.dtype != np.bool_ or sel.ndim != 1 or len(sel) < len(x):
            raise PBError('anchor_rows: a row selector must be a bool vector over the piece\'s rows (got %s of shape %s)' % (sel.dtype, tuple(sel.shape)))
        keep = x[sel[:len(x)]]
    else:
        if which not in ('skyline', 'bass'):
            raise PBError('anchor_rows: %r is neither "skyline", "bass" nor a bool row selector' % (which,))
        if e2w is None:
            value = {i: i for i in range(128)}
        else:
            cls = ops.CLASS_NAMES[3]
            value = {int(i): int(w[len(cls) + 1:]) for w, i in e2w[cls].items() if w[len(cls) + 1:].isdigit()}
        best = {}
        for i, r in enumerate(x):
            v = value.get(int(r[3]))
            if v is None:
                continue
            key = (int(r[0]), int(r[1]))
            if key not in best or (v > best[key][0] if which == 'skyline' else v < best[key][0]):
                best[key] = (v, i)
        keep = x[sorted(i for _, i in best.values())]
    return keep[np.argsort(keep[:, 0] * (int(lay.pad8[1]) + 1) + keep[:, 1], kind='stable')] if len(keep) else keep.reshape(0, 8)


def add_anchor_flags(ap):
    """The command-line form of anchor_rows, shared by eval_generation, demo and tools/decode_batch_bench.py."""
    ap.add_argument('--accompany', type=str, default=None, choices=('skyline', 'bass'), help='anchored generation (needs --prime): keep the highest '
                    '(skyline) or lowest (bass) melodic note of every (bar, position) of each piece behind its prime where it falls in time and let '
                    'the model write the notes around them; implies --ordered; not with --keep or --infill')


def check_anchor_flags(args):
    """The flag rules of --accompany: PBError where it comes without --prime or together with --keep / --infill."""
    if getattr(args, 'accompany', None) is None:
        return
    if getattr(args, 'prime', None) is None:
        raise PBError('--accompany needs --prime N|half: the anchors are the piece\'s own rows behind the prime')
    for other in ('keep', 'infill'):
        if getattr(args, other, None):
            raise PBError('--accompany does not combine with --%s: position-indexed and time-indexed givens do not combine' % other)


def anchors_from_args(args, piece, k, e2w=None):
    """The anchors of ONE piece under --accompany: anchor_rows of its rows behind the prime of k rows; None without the flag."""
    which = getattr(args, 'accompany', None)
    if which is None:
        return None
    return anchor_rows(_as_numpy(piece)[int(k):], which, e2w)


def _anchor_table(lists):
    """The device form of check_anchors' lists: (table (n, 8) int16 of every row's anchors, base, cnt), the last two int32, one per row."""
    base, cnt, parts = [], [], []
    for a in lists:
        base.append(sum(cnt))
        cnt.append(0 if a is None else len(a))
        if a is not None:
            parts.append(a.numpy().astype(np.int16))
    return np.ascontiguousarray(np.concatenate(parts)), np.asarray(base, dtype=np.int32), np.asarray(cnt, dtype=np.int32)


def _slice_anchors(lists, a, b):
    """check_anchors' lists for the rows a .. b - 1; None where none of them has an anchor."""
    if lists is None or all(v is None for v in lists[a:b]):
        return None
    return list(lists[a:b])


def infill_plan(piece, lo, hi, mask_word, pad_word, mode='rows'):
    """The plan of "rewrite bars lo .. hi-1 of this piece and leave the rest alone", host only. piece (S, 8) Octuple ids: ordinary rows with
    non-decreasing bar ids (ValueError otherwise: the piece has no region), then usually an EOS row, then PAD; 0 <= lo < hi <= pad_word[0].
    Returns a dict: k = the leading rows with bar < lo; prefix = those rows (the decoder prime); stop = hi (the row's stop bar); suffix = the
    rows with bar >= hi up to and including the piece's first row with a special bar id unless that row is PAD (the EOS row travels with
    the suffix); enc = the (S, 8) encoder input. mode 'rows' (TokenMask's convention): every row of the region is replaced by mask_word,
    the length is preserved. mode 'span' (TokenInfilling's): the region is replaced by ONE mask_word row, the rest moves up and pad_word
    fills the tail (cut at S). An empty region is legal: 'rows' masks nothing, 'span' inserts the one row."""
    x = piece.detach().cpu().numpy() if isinstance(piece, torch.Tensor) else np.asarray(piece)
    if x.ndim != 2 or x.shape[1] != 8:
        raise PBError('infill_plan: piece of shape %s, expected (S, 8)' % (tuple(x.shape),))
    x = x.astype(np.int64)
    mask_word, pad_word = np.asarray(mask_word, dtype=np.int64).reshape(8), np.asarray(pad_word, dtype=np.int64).reshape(8)
    S, pad0 = x.shape[0], int(pad_word[0])
    if isinstance(lo, bool) or isinstance(hi, bool) or not isinstance(lo, (int, np.integer)) or not isinstance(hi, (int, np.integer)) or not 0 <= lo < hi <= pad0:
        raise PBError('infill_plan: bars %r:%r: expected integers 0 <= lo < hi <= %d' % (lo, hi, pad0))
    if mode not in ('rows', 'span'):
        raise PBError('infill_plan: mode %r is neither "rows" nor "span"' % (mode,))
    special = np.flatnonzero(x[:, 0] >= pad0)
    e = int(special[0]) if len(special) else S                             # the ordinary rows are x[:e]
    bars = x[:e, 0]
    if (np.diff(bars) < 0).any():
        i = int(np.flatnonzero(np.diff(bars) < 0)[0]) + 1
        raise ValueError('infill_plan: the bar ids of the piece decrease at row %d (%d after %d): it has no region of bars %d .. %d'
                         % (i, int(bars[i]), int(bars[i - 1]), lo, hi - 1))
    k, m = int((bars < lo).sum()), int((bars < hi).sum())                  # the region is x[k:m]
    tail = e + 1 if e < S and int(x[e, 0]) != pad0 else e
    if mode == 'rows':
        enc = x.copy()
        enc[k:m] = mask_word
    else:
        enc = np.concatenate([x[:k], mask_word[None], x[m:], np.tile(pad_word, (max(0, m - k - 1), 1))])[:S]
    return dict(k=k, prefix=x[:k].copy(), stop=int(hi), suffix=x[m:tail].copy(), enc=enc)


def infill_splice(out_row, suffix, S, bar_pad):
    """The piece after infilling: the emitted rows of out_row (a generated (S, 8) row: the prime, the new region, PAD behind its stop --
    the rows in front of its first bar PAD), followed by suffix (infill_plan), with PAD behind. Returns (row (S, 8), truncated): a piece
    longer than S is cut at S and truncated is True."""
    y = out_row.detach().cpu().numpy() if isinstance(out_row, torch.Tensor) else np.asarray(out_row)
    pad_rows = np.flatnonzero(y[:, 0] == bar_pad)
    n = int(pad_rows[0]) if len(pad_rows) else y.shape[0]
    row = np.concatenate([y[:n], np.asarray(suffix, dtype=y.dtype).reshape(-1, 8)])
    truncated = len(row) > S
    if len(row) < S:
        row = np.concatenate([row, np.tile(y[n], (S - len(row), 1))])      # len(row) < S <= len(y) + len(suffix): y[n] is a PAD row
    return row[:S], truncated


KEEP_NAMES = ('bar', 'position', 'instrument', 'pitch', 'duration', 'velocity', 'timesig', 'tempo')       # the 8 heads, model column order


def check_forced(forced, P, S, sizes, ks, owner=None):
    """The argument rules of forced tokens, on the host before any device work. forced: (P, S, 8) integers in model column order (tensor on
    any device, or array): -1 = the head is free, v >= 0 = head h of position i of prompt p is v. sizes: the 8 table sizes (a given id may be
    any id of its head's table, specials included); ks: the prefix lengths of check_prefix -- positions below k_p belong to the prefix and
    must be all -1. owner (row -> prompt, check_samples): the table is expanded to one row per output row. Returns an int16 array
    (P, S, 8), or (R, S, 8) with owner; None for forced=None or a table that is -1 everywhere (no forcing: the caller runs what it ran
    before). Raises PBError for a bad shape, dtype or a conflict with a prefix, IndexError for an id outside its table."""
    if forced is None:
        return None
    f = forced.detach().cpu().numpy() if isinstance(forced, torch.Tensor) else np.asarray(forced)
    if f.ndim != 3 or f.shape != (P, S, 8):
        raise PBError('forced of shape %s: expected (%d, %d, 8) for %d prompt(s) and a window of %d' % (tuple(f.shape), P, S, P, S))
    if f.dtype == np.bool_ or not np.issubdtype(f.dtype, np.integer):
        raise PBError('forced ids must be integers (got %s)' % f.dtype)
    if not (f != -1).any():
        return None
    bad = np.argwhere((f < -1) | (f >= np.asarray(sizes, dtype=np.int64)))
    if len(bad):
        b, i, h = (int(v) for v in bad[0])
        raise IndexError('index out of range in self: forced id %d of prompt %d, position %d, head %d is neither -1 nor inside its table (sizes %s)'
                         % (int(f[b, i, h]), b, i, h, list(sizes)))
    for b, kb in enumerate(ks):
        if (f[b, :kb] != -1).any():
            raise PBError('forced: prompt %d gives a head at position %d, inside its prefix of %d rows (the prefix already gives those positions)'
                          % (b, int(np.argwhere((f[b, :kb] != -1).any(1))[0, 0]), kb))
    f = f.astype(np.int16)
    return np.ascontiguousarray(f if owner is None else f[np.asarray(owner, dtype=np.int64)])


def forced_token(frow, sample):
    """The token of ONE position under the forced-token contract, for every decode path: the reference's `current_output = self.sample(x, i)`
    (model.py:46) followed by the overwrite of the given heads. frow: the position's 8 entries (-1 = free) or None; sample(): the path's own
    sampling of the position, 8 ids. A position with a free head samples (one random_sample(8): the draws of its given heads are consumed and
    unused); a position whose 8 heads are given does not call sample() at all, so it draws nothing."""
    if frow is None:
        return sample()
    given = frow >= 0
    if given.all():
        return torch.from_numpy(frow.astype(np.int64))
    tok = sample()
    if given.any():
        tok = tok.clone()
        tok[torch.from_numpy(given)] = torch.from_numpy(frow[given].astype(np.int64))
    return tok


def forced_draws(rng, frow, start, S):
    """The (S, 8) uniform draws of one row made ahead of its decode: one block of 8 from `rng` for every position >= start that has a free
    head, in position order -- the stream forced_token's sample() calls consume. Positions below start and positions whose 8 heads are
    given keep 0. frow: the row's (S, 8) forced table or None (every position free)."""
    U = np.zeros((S, 8), dtype=np.float64)
    free = np.ones(S, dtype=bool) if frow is None else (np.asarray(frow) < 0).any(1)
    free[:start] = False
    U[free] = rng.random_sample(int(free.sum()) * 8).reshape(-1, 8)
    return U


def parse_keep(keep):
    """The head indices of a list of attribute names (KEEP_NAMES, case-insensitive) and / or indices 0 .. 7, or of one comma-separated
    string of them (the --keep flag), sorted, each once. Raises PBError for an unknown name or an empty list."""
    if isinstance(keep, str):
        keep = [v for v in (w.strip() for w in keep.split(',')) if v]
    heads = set()
    for v in keep:
        if isinstance(v, (int, np.integer)) and not isinstance(v, bool):
            h = int(v)
        elif isinstance(v, str) and v.lower() in KEEP_NAMES:
            h = KEEP_NAMES.index(v.lower())
        elif isinstance(v, str) and v.isdigit():
            h = int(v)
        else:
            h = -1
        if not 0 <= h < 8:
            raise PBError('keep: %r is no Octuple attribute (%s, or a head index 0 .. 7)' % (v, ', '.join(KEEP_NAMES)))
        heads.add(h)
    if not heads:
        raise PBError('keep: no attribute named (%s)' % ', '.join(KEEP_NAMES))
    return sorted(heads)


def keep_mask(piece, keep, start=None, bar_pad=256):
    """The `forced` table that keeps some attributes of a piece and leaves the rest to the model. piece (B, S, 8) Octuple ids; keep: attribute
    names / head indices (parse_keep); start: B positions (None = 0). For row b the kept heads of positions start_b .. e_b are copied, e_b =
    the piece's first row whose bar id is special (>= bar_pad: the EOS row, so the generated row ends where the piece ends; the last row if
    there is none). Every other head and position, the PAD tail included, is -1. Returns int16 (B, S, 8)."""
    heads = parse_keep(keep)
    x = piece.detach().cpu().numpy() if isinstance(piece, torch.Tensor) else np.asarray(piece)
    if x.ndim != 3 or x.shape[2] != 8:
        raise PBError('keep_mask: piece of shape %s, expected (B, S, 8)' % (tuple(x.shape),))
    B, S = x.shape[:2]
    start = [0] * B if start is None else [int(v) for v in (start.tolist() if hasattr(start, 'tolist') else start)]
    if len(start) != B:
        raise PBError('keep_mask: %d start positions for %d pieces' % (len(start), B))
    forced = np.full((B, S, 8), -1, dtype=np.int16)
    for b in range(B):
        special = np.flatnonzero(x[b, :, 0] >= bar_pad)
        e = int(special[0]) if len(special) else S - 1
        s = max(0, start[b])
        if s <= e:
            forced[b, s:e + 1, heads] = x[b, s:e + 1][:, heads].T
    return forced


def sample_seed(seed, j, i, N):
    """The seed of sample j of prompt i among N prompts (eval_generation --samples, demo --samples): seed + j N + i. Sample 0 keeps the
    seed + i of a run without samples, and no two (prompt, sample) pairs of a run share a generator."""
    return int(seed) + int(j) * int(N) + int(i)


def sampler_form_for(sizes, p):
    """The rule of pb_batch_decoder_sampler_init, stated on the host: which device sampler a decoder with these 8 head sizes and nucleus
    thresholds gets. 'narrow' while every head has <= 272 classes (its LDS rows) AND the heads with p < 1 hold at most 512 classes together
    (it ranks them with one thread each), else 'wide' (heads up to 1088 classes, the rank counting in rounds of 512 threads). Every legal
    dictionary (ops.Layout) gets one of the two: none is refused at generation time."""
    ranked = sum(int(n) for n, q in zip(sizes, p) if float(q) < 1.0)
    return 'wide' if max(int(n) for n in sizes) > 272 or ranked > 512 else 'narrow'


def _refuse_unmerged_lora(eng, what):
    """The fused decoder reads the backbone's weights alone: with LoRA adapters attached (Engine.attach_lora) it would generate from the base
    model. Fold them in first. Reads the instance's own `lora` entry only, so it comes in front of every argument check without touching the engine."""
    if vars(eng).get('lora') is not None:
        raise PBError('%s: LoRA adapters are attached and not merged; call merge_lora() first (the decode kernels read the backbone weights only)' % what)


class GenerationMixin:
    last_sampler_form = None            # 'narrow' / 'wide': the device sampler of the last device-sampled decode (None: there was none yet)

    def _note_sampler_form(self, dec):
        """Which device sampler the decoder's steps ended with: 'narrow' (the default dictionary) or 'wide' (sampler_form_for's rule). Kept
        in `last_sampler_form`; `last_decode` names it only when it is the wide one, so the default dictionary's record keeps its keys."""
        self.last_sampler_form = 'wide' if int(LIB.query('pb_batch_decoder_sampler_form', dec)) else 'narrow'
        return dict(sampler_form='wide') if self.last_sampler_form == 'wide' else {}

    # ------------------------------------------------------------------ generate (model.py:28-66)
    def generate(self, enc_ids, emask, sample_row, use_cache=True, max_new=None, sampler=None, prefix=None, forced=None, stop=None, order=None, allow=None,
                 bar_allow=None, anchors=None):
        """Autoregressive decode with the reference's control flow (SOS start, host-side nucleus sampling, early stop on
        any special token). The reference re-runs encoder AND decoder over all S positions for every generated position
        (model.py:42-45); here the encoder runs once, the cross-attention K/V of every decoder layer are projected once,
        and each step feeds ONE decoder token through the layers against a self-attention K/V cache. Position-i logits
        only depend on decoder inputs <= i (causal), so the tokens are identical (tests/test_model_gpu.py).
        max_new: stop after that many positions (None = the window). sampler = dict(T=[8 temperatures], P=[8 thresholds]): the caller
        states that `sample_row` IS model.py:68-107 with these constants, drawing np.random.random_sample(8) per position; the decoder may
        then sample on the device ahead of the host (`_decode_device_sampled`) -- `sample_row` still decides every token.
        prefix (1, k, 8): primed generation -- the reference loop with decoder inputs 1 .. k and their mask set to the prefix, the loop
        starting at position k and result[:, :k] = prefix. The forced positions draw nothing; max_new counts sampled positions
        (the row stops at min(S, k + max_new)). The cache rows of the prefix come from one teacher-forced decoder pass (_prefill).
        forced (1, S, 8), -1 = free (check_forced): forced tokens -- the reference loop with the given heads of `current_output` overwritten
        by forced[0, i] right after `self.sample(x, i)` (forced_token). The stop rule sees the token after forcing; a position with a free
        head draws its 8 uniforms as ever, a position with all 8 heads given draws nothing; positions below k must be free; max_new counts
        positions from k on, given or sampled. Leading given positions are stepped through, not prefilled. None, or -1 everywhere: exactly
        the launches and bytes of a call without the argument.
        stop (an int, or a sequence of one; check_stop): stop at a bar -- the reference loop with the stop test `(current_output >=
        pad).any()` replaced by `(current_output >= pad).any() or current_output[0] >= stop` (stop_vector). The test sees the token after
        forcing; the token that trips it is not written (result[0, i:] stays PAD) and its draws are consumed; positions below k are not
        tested; max_new and the window still apply. pad[0] (256), or None: no stop, the call without the argument. A call that
        passes `stop` (256 included) finds last_decode['ended']: what ended the row, 'special', 'bar' or 'limit'; a call without the
        argument leaves the record it always left.
        order (an int, or a sequence of one; check_order): time-ordered sampling -- the reference loop with `current_output =
        self.sample(x, i)` replaced by the ordered sample (ordered_token; DESIGN.md section 1, "Time-ordered sampling"): with prev = the
        decoder's input row at position i, bars below max(order, prev's bar) and, inside prev's bar, positions below prev's position get
        probability 0. Forcing, the stop test, the draws and what is written are unchanged. `sample_row` must then take the keyword
        `order` (PianoBartLM.sample_row does). -1, or None: not ordered, the call without the argument.
        allow ((V,) bools, or a sequence of one; check_allow): allowed classes -- the reference loop with sampling(logit, p, t) seeing -inf
        in place of every logit whose bit is 0 (allowed_token; DESIGN.md section 1, "Allowed classes"). The mask is constant over the
        positions; the special ids stay reachable; forcing, the stop test, the draws and what is written are unchanged; an ordered row
        loses the classes either rule removes. `sample_row` must then take the keyword `allow`. None, or True everywhere: the call
        without the argument.
        bar_allow (one bar schedule, or a sequence of one; check_bar_allow): allowed classes that change with the bar -- head 0 as without
        it; heads 1 .. 7 of a token whose bar after forcing is b0 are sampled from `allow AND bar_allow[b0]` where b0 is ordinary and
        has an entry (scheduled_token; DESIGN.md section 1, "Bar schedules"). `sample_row` must then take the keyword `sched`. None, or
        no entry that removes a class: the call without the argument; last_decode gains `scheduled` only when a schedule is in force.
        anchors ((n, 8) complete Octuple rows in (bar, position) order, or a sequence of one; check_anchors): anchored notes -- every
        position is sampled as without them and anchored_token decides what is written: while anchors remain, a candidate that would end
        the row or whose (bar, position) has reached the next anchor's gives way to that anchor ("Anchored notes").
        The row is time-ordered with floor max(order, 0). Not with `forced`. None, or an empty list: the call without the argument;
        last_decode gains `anchors_placed` only when anchors were given."""
        _refuse_unmerged_lora(self, 'generate')
        S = int(enc_ids.shape[1])
        with_ended = stop is not None
        ks, rows = check_prefix(prefix, None, 1, S, self.pb.pad_word_np)
        forced = check_forced(forced, 1, S, list(self.lay.sizes) if forced is not None else None, ks)
        stop = check_stop([stop] if isinstance(stop, (int, np.integer)) and not isinstance(stop, bool) else stop, 1, int(self.pb.pad_word_np[0]))
        sb = stop[0] if stop is not None else None
        order = check_order([order] if isinstance(order, (int, np.integer)) and not isinstance(order, bool) else order, 1, order_max=int(self.pb.pad_word_np[0]) - 1)
        ob = order[0] if order is not None else None
        plan = check_bar_allow(bar_allow, allow, 1, self.lay)
        allow = plan[:2] if plan is not None else check_allow(allow, 1, self.lay if allow is not None else None)
        ab = unpack_allow(allow, self.lay.vocab)[0] if allow is not None else None
        sc = unpack_schedule(plan, self.lay.vocab)[0] if plan is not None else None
        fr = forced[0] if forced is not None else None
        k = ks[0]
        pre = rows[0, :k] if k else None
        anc = check_anchors(anchors, 1, S, self.pb.pad_word_np, ks, rows, stop, order, forced, max_new)
        if anc is not None:                                  # anchors imply time order
            order = anc[1]
            ob = order[0]
        an = anc[0][0] if anc is not None else None
        self._await_updates(2)
        if not use_cache:
            return self._generate_nocache(enc_ids, emask, sample_row, k, pre, fr, sb, ob, ab, sc, an)
        if self.hd not in (32, 64, 96, 128):                 # pb_attn_decode's row-chunk layouts; other head sizes use the training kernels
            return self._generate_pyloop(enc_ids, emask, sample_row, k, pre, fr, sb, ob, ab, sc, an)
        # One hipGraph replay per token where the fused decoder covers the shape (pb_batch_decoder_create's rule) at B = 1: it keeps the
        # position in device memory; PB_DECODE_GRAPH=0 issues the same launches directly, PB_DECODE_GRAPH=-1 keeps the round-2 loop below (A/B)
        with torch.no_grad(), self._decoder_run(enc_ids, emask, ks, rows, round2=True) as run:
            self.last_decode = None
            res_cpu, pad_cpu = run.res_cpu, run.pad_cpu
            if run.dec is not None:
                if sampler is not None and _DECODE_SPEC:
                    fault = int(getattr(self, 'decode_fault_period', 0) or 0)    # tests: the device's choice is corrupted at every fault-th position
                    info = self._decode_device_sampled(run.dec, 1, S, lambda b, row, **kw: sample_row(row, **kw), [np.random.get_state()], sampler,
                                                       res_cpu, pad_cpu, max_new, (0, fault), inline_verify=True, starts=[k], forced=forced, stop=stop,
                                                       order=order, allow=allow, sched=plan, anchors=anc[0] if anc is not None else None)
                    info.update(tokens=info['tokens'][0], rewinds=info['rewinds'][0], ended=info['ended'][0])
                else:
                    info = self._decode_host_sampled(run.dec, S, sample_row, res_cpu, pad_cpu, max_new, k, fr, sb, ob, ab, sc, an)
                self.last_decode = dict(info, s_enc=run.s_enc[0], prefix=k, prefill_ms=float(run.prefill_ms()), **(dict(scheduled=True) if sc is not None else {}))
                if not with_ended:
                    del self.last_decode['ended']
            else:
                import ctypes
                pref, stream = ctypes.byref(run.bp.plan), ops._stream()
                tok16 = run.bufs['tok16']
                if k:
                    tok16.copy_(pre[k - 1].to(torch.int16))                     # the input of position k: the prefix's last row
                tok_pin = torch.empty(8, dtype=torch.int16).pin_memory()         # one small H2D per position; the result goes up once at the end
                logit_pin = torch.empty(self.lay.vocab, dtype=torch.float32).pin_memory()
                sv = stop_vector(pad_cpu, sb)
                prev = pre[k - 1] if k else torch.from_numpy(self.pb.sos_word_np)
                ak = 0                                                          # anchors written (anchored_token)
                for i in range(k, S):
                    LIB.call('pb_decode_step', pref, i, stream)
                    logit_pin.copy_(run.bufs['logits'][0])                      # D2H on the current stream, returns when the row has landed
                    tok = scheduled_token(fr[i] if fr is not None else None, lambda **kw: sample_row(logit_pin, **kw), ab, sc, ob, prev, pad_cpu)
                    tok, ak = anchored_token(tok, an, ak, sv, pad_cpu)
                    if (tok >= sv).any():
                        break
                    res_cpu[0, i] = prev = tok
                    tok_pin.copy_(tok)
                    tok16.copy_(tok_pin, non_blocking=True)                     # stream-ordered before the next step's kernels
        return res_cpu.to(enc_ids.device)

    def _prompt_inputs(self, enc_ids, emask):
        """What every generation path does with its prompt(s) first: the engine bound to their device, the mask as contiguous f32, the ids as
        int16 and range-checked (note_ids; a rank may generate by itself, so the verdict is local). Returns (em, enc16)."""
        self.bind(enc_ids.device)
        em = emask.to(torch.float32).contiguous() if emask is not None else None
        enc16 = ops.ids_to_i16(enc_ids)
        self.note_ids(enc16); self.check_ids(collective=False)
        return em, enc16

    @contextlib.contextmanager
    def _decoder_run(self, enc_ids, emask, ks, rows, groups=None, round2=False):
        """The set-up of ONE decode run of G prompts as B <= BATCH_MAX rows, and its tear-down: `generate` (one prompt, one row) and
        _generate_batch_chunk enter it and run their loop on what it yields. ks / rows: the prefix lengths and rows of check_prefix.
        groups None: one row per prompt, (B, S, 2d) cross caches. groups = [prompt of row b] (samples of a prompt, rows prompt-major):
        enc_ids / emask / ks / rows describe the G distinct prompts; their encoder passes, projections and prefills run once each into
        (G, S, 2d) cross caches that the rows read through pb_batch_decoder_share_cross, and a primed prompt's k prefix rows of every
        layer's self cache are copied to its other samples' rows (a device copy, no arithmetic). The self caches, masks, positions,
        limits, draws, verification and rewinds stay per row.
        In order: the inputs (_prompt_inputs), each prompt's key extent, the plan and its buffers (_decode_plan), the fused decoder
        (_decoder_create: allocations only, nothing enqueued), then per prompt the batch-1 encoder pass, cross K|V projections and prefill,
        exactly as a lone `generate` of that prompt runs them, into the prompt's cache slice and first row; the decoder's reset behind all
        of that, and one synchronize (the prompts' passes are not part of the loop's per-token time). The decoder is destroyed on the way out.
        round2: the caller has the pb_decode_step loop for a run without a fused decoder -- the set-up then goes on where create declines
        the shape, and creates none at PB_DECODE_GRAPH=-1. Otherwise a declined shape is yielded at once, before any encoder work, with
        run.dec None (the caller's fallback). Yields the run: dec, bp, bufs, B, S, G, groups, s_enc / starts (per row), pad_cpu, res_cpu
        ((B, S, 8) PAD with the prefixes in place), prefill_ms() and setup_ms."""
        _refuse_unmerged_lora(self, 'the fused decoder')
        G, S, dev = int(enc_ids.shape[0]), int(enc_ids.shape[1]), enc_ids.device
        shared = groups is not None
        groups = list(groups) if shared else list(range(G))
        B = len(groups)
        first = [groups.index(g) for g in range(G)]                        # the row that receives prompt g's prefill
        pad_cpu = torch.from_numpy(self.pb.pad_word_np)
        em, enc16 = self._prompt_inputs(enc_ids, emask)
        t_setup = time.perf_counter()
        s_enc_g = [self._key_extent(em[g:g + 1] if em is not None else None, S) for g in range(G)]
        em_rows = em[torch.as_tensor(groups, device=dev)].contiguous() if shared and em is not None else em      # the decoder's masks stay per row
        bp, bufs = self._decode_plan(B, S, [s_enc_g[g] for g in groups], em_rows, dev, G=G if shared else None)
        dec = None if round2 and _DECODE_GRAPH < 0 else self._decoder_create(bp)
        timers = []
        run = SimpleNamespace(dec=dec, bp=bp, bufs=bufs, B=B, S=S, G=G, groups=groups, s_enc=[s_enc_g[g] for g in groups], starts=[ks[g] for g in groups],
                              pad_cpu=pad_cpu, res_cpu=pad_cpu.repeat(B, S, 1), prefill_ms=lambda: sum(t() for t in timers), setup_ms=None)
        if dec is None and not round2:                                     # not covered: the caller's per-prompt loop
            yield run
            return
        try:
            if shared:
                kv_row = np.asarray(groups, dtype=np.int32)
                LIB.call('pb_batch_decoder_share_cross', dec, G, kv_row.ctypes.data)
            for g in range(G):                                             # the batch-1 encoder pass (and prefill) of each prompt, into its cache slice
                emb = em[g:g + 1] if em is not None else None
                _, enc_out = self.forward_hidden(enc16[g:g + 1], None, emb, None, False, 0)
                for l in range(self.ND):
                    self._linear(enc_out, 'dec.%d.wkv_c' % l, 'dec.%d.bkv_c' % l, bufs['kvc'][l][g], S, 2 * self.d, self.d)
                if ks[g]:
                    b1 = first[g]
                    timers.append(self._prefill(enc16[g:g + 1], emb, rows[g], ks[g], [t[b1] for t in bufs['kvs']]))
                    for b in range(B):
                        if groups[b] != g:
                            continue
                        run.res_cpu[b, :ks[g]] = rows[g, :ks[g]]
                        if b != b1 and ks[g] < S:                          # the prefix rows of the prompt's other samples: copies of the prefilled ones
                            for t in bufs['kvs']:
                                t[b, :ks[g]].copy_(t[b1, :ks[g]])
            if dec is not None:
                LIB.call('pb_batch_decoder_reset', dec, ops._stream(), _DECODE_GRAPH)
                torch.cuda.current_stream().synchronize()
            run.setup_ms = (time.perf_counter() - t_setup) * 1e3
            yield run
        finally:
            if dec is not None:
                LIB.call('pb_batch_decoder_destroy', dec)

    def _prefill_inputs(self, pre, k, S, dev):
        """The device inputs of _prefill for a prefix of k rows (0 < k < S): the decoder ids SOS, pre[0] .. pre[k-2], their mask, and the
        gather index of the k cache rows. Host-to-device copies only, so a caller may make them ahead of the pass."""
        dec = torch.from_numpy(self.pb.pad_word_np).repeat(1, S, 1)
        dec[0, 0] = torch.from_numpy(self.pb.sos_word_np)
        dec[0, 1:k] = pre[:k - 1]
        dmask = torch.zeros(1, S, dtype=torch.float32)
        dmask[0, :k] = 1
        rows = torch.arange(k, dtype=torch.int32)
        idx = torch.stack([3 * rows + 1, 3 * rows + 2], 1).reshape(-1).to(dev)
        return ops.ids_to_i16(dec.to(dev)), dmask.to(dev), idx

    def _prefill(self, enc16, em, pre, k, kvs, inputs=None):
        """Primed generation: rows 0 .. k-1 of the self-attention caches kvs[l] ((S, 2d) each, row j = K | V of decoder position j, the layout
        pb_decode_step and the fused decoder's new-token workgroup write) get the K|V of the decoder inputs SOS, pre[0] .. pre[k-2]. ONE
        teacher-forced decoder pass over them on the training kernels, against the encoder pass just run (reuse_encoder), then a row gather
        (pb_gather_rows16: 16-byte copies, no arithmetic) out of each layer's q|k|v workspace: in d-wide blocks, cache blocks 2j, 2j + 1 <-
        workspace blocks 3j + 1, 3j + 2. Per prompt, like the encoder pass, so that a row of generate_batch stays the batch-1 generate of its
        prompt bit for bit. No-op unless 0 < k < S (k = S samples nothing). inputs: what _prefill_inputs returned for (pre, k), made ahead.
        Returns a callable giving the pass's device milliseconds."""
        if not 0 < k < int(enc16.shape[1]):
            return lambda: 0.0
        S, dev = int(enc16.shape[1]), enc16.device
        dec16, dmask, idx = inputs if inputs is not None else self._prefill_inputs(pre, k, S, dev)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        self.forward_hidden(enc16, dec16, em, dmask, False, 0, reuse_encoder=True)
        esz = 2 if self.xdt == torch.bfloat16 else 4
        for l in range(self.ND):
            ops.gather_rows16(self._cur_ws['dec'][l]['qkv'], idx, kvs[l], 2 * k, self.d * esz)
        t1.record()
        return lambda: t0.elapsed_time(t1)

    def _key_extent(self, em, S):
        """Encoder positions a decoder query can see: keys behind the last visible one are masked for every query, so the decode stops there."""
        if em is None:
            return S
        km = torch.empty(1, dtype=torch.int32, device=em.device)
        ops.key_extent(em, km)
        return max(1, min(S, int(km.item())))

    def _decode_plan(self, B, S, s_enc, em, dev, G=None):
        """The pb_decode_batch of B prompts (pb_decode_step reads its plan at B = 1) and the buffers it points into: per decoder layer the
        (B, S, 2d) cross K|V cache (filled by the caller from each prompt's encoder pass) and self K|V cache, the (B, d) / (B, ffn)
        scratch rows, (B, vocab) logits and the split records. G: the cross cache holds G <= B slices, one per distinct prompt
        (pb_batch_decoder_share_cross maps the rows onto them)."""
        from ._lib import DecodeBatch
        _refuse_unmerged_lora(self, 'the fused decoder')
        d, X, ff, wf = self.d, self.xdt, self.fd, self.wf
        e = lambda *shape, dt=X: torch.empty(*shape, dtype=dt, device=dev)
        bufs = dict(kvc=[e(B if G is None else G, S, 2 * d) for _ in range(self.ND)], kvs=[torch.zeros(B, S, 2 * d, dtype=X, device=dev) for _ in range(self.ND)],
                    rows={n: e(B, d) for n in ('x', 'y1', 'yc', 'y2', 'q', 'ctx', 'a')}, g=e(B, ff), stat=e(8, dt=torch.float32),
                    logits=e(B, self.lay.vocab, dt=torch.float32), tok16=torch.tensor(self.pb.sos_word_np, dtype=torch.int16, device=dev),
                    attn_part=e(B * self.H * 16 * (self.hd + 4), dt=torch.float32))      # PB_DECODE_MAX_SPLITS records per (row, head)
        bp = DecodeBatch()
        plan = bp.plan
        plan.dtype, plan.d, plan.H, plan.ffn, plan.S, plan.S_enc, plan.n_layers, plan.vocab = self.code, d, self.H, ff, S, max(s_enc), self.ND, self.lay.vocab
        for k in range(9):
            plan.tab_off[k] = self.lay.tab_off[k]
        P = lambda t: t.data_ptr()
        plan.tok16, plan.ptab, plan.lin_b, plan.pos = P(bufs['tok16']), P(self.ptab), P(wf['lin.b']), P(wf['dec.pos'])
        plan.lne_w, plan.lne_b, plan.enc_mask = P(wf['dec.lne.w']), P(wf['dec.lne.b']), (P(em) if em is not None else None)
        for n, t in bufs['rows'].items():
            setattr(plan, n, P(t))
        plan.g, plan.stat, plan.logits, plan.head_w, plan.head_b = P(bufs['g']), P(bufs['stat']), P(bufs['logits']), P(self.w['head.w']), P(wf['head.b'])
        # the split records are merged in the out-projection GEMV's prologue, which holds K = d in one chunk per thread (256 threads x
        # 16 bytes): wider models keep the one-workgroup-per-head attention
        epv = 8 if self.code == PB_BF16 else 4
        plan.attn_part = P(bufs['attn_part']) if d <= 256 * epv else None
        for l in range(self.ND):
            pf, L = 'dec.%d.' % l, plan.layers[l]
            L.wqkv, L.bqkv, L.wo, L.bo = P(self.w[pf + 'wqkv']), P(wf[pf + 'bqkv']), P(self.w[pf + 'wo']), P(wf[pf + 'bo'])
            L.ln1_w, L.ln1_b = P(wf[pf + 'ln1.w']), P(wf[pf + 'ln1.b'])
            L.wq_c, L.bq_c, L.wo_c, L.bo_c = P(self.w[pf + 'wq_c']), P(wf[pf + 'bq_c']), P(self.w[pf + 'wo_c']), P(wf[pf + 'bo_c'])
            L.lnc_w, L.lnc_b = P(wf[pf + 'lnc.w']), P(wf[pf + 'lnc.b'])
            L.w1, L.b1, L.w2, L.b2 = P(self.w[pf + 'w1']), P(wf[pf + 'b1']), P(self.w[pf + 'w2']), P(wf[pf + 'b2'])
            L.ln2_w, L.ln2_b = P(wf[pf + 'ln2.w']), P(wf[pf + 'ln2.b'])
            L.kv_self, L.kv_cross = P(bufs['kvs'][l]), P(bufs['kvc'][l])
        bp.B = B
        for b in range(B):
            bp.s_enc[b] = s_enc[b]
        return bp, bufs

    @staticmethod
    def _decoder_create(bp):
        """The fused decoder of `bp`, or None where it does not cover the shape (pb_batch_decoder_create holds the one rule)."""
        import ctypes
        dec = ctypes.c_void_p()
        rc = int(LIB.query('pb_batch_decoder_create', ctypes.byref(bp), ctypes.byref(dec)))
        if rc < 0:
            raise PBError('pb_batch_decoder_create failed (%d): %s' % (rc, LIB.load().pb_last_error().decode()))
        return dec if rc == 0 else None

    def _decode_host_sampled(self, dec, S, sample_row, res_cpu, pad_cpu, max_new, k=0, fr=None, stop=None, order=None, allow=None, sched=None, anchors=None):
        """One host round trip per token through the B = 1 decoder (pb_batch_decoder_step): tokens in, logits rows out, sample_row between.
        k > 0 (primed): the decoder starts behind the prefix (pb_batch_decoder_start), fed its last row, which res_cpu[0, k - 1] holds.
        fr (S, 8): the row's forced table (forced_token). stop: the row's stop bar or None (stop_vector). order: the row's bar floor or None
        (ordered_token; prev is tok_np, the decoder's input). allow: the row's (V,) bool mask or None (allowed_token). sched: the row's
        schedule (unpack_schedule) or None (scheduled_token). anchors: the row's (n, 8) anchors or None (anchored_token)."""
        import ctypes
        sv, ended = stop_vector(pad_cpu, stop), 'limit'
        tok_np = np.ascontiguousarray((res_cpu[0, k - 1].numpy() if k else np.asarray(self.pb.sos_word_np)).astype(np.int16))
        if k:
            last = np.asarray([k - 1], dtype=np.int32)
            LIB.call('pb_batch_decoder_start', dec, last.ctypes.data, tok_np.ctypes.data, None)
        logit_cpu = torch.empty(self.lay.vocab, dtype=torch.float32)
        tok_p, log_p = ctypes.c_void_p(tok_np.ctypes.data), ctypes.c_void_p(logit_cpu.data_ptr())
        n = ak = 0
        t_loop = time.perf_counter()
        for i in range(k, S if max_new is None else min(S, k + max_new)):
            LIB.call('pb_batch_decoder_step', dec, tok_p, log_p)
            n += 1
            tok = scheduled_token(fr[i] if fr is not None else None, lambda **kw: sample_row(logit_cpu, **kw), allow, sched, order, tok_np, pad_cpu)
            tok, ak = anchored_token(tok, anchors, ak, sv, pad_cpu)
            if (tok >= sv).any():
                ended = end_reason(tok, pad_cpu)
                break
            res_cpu[0, i] = tok
            tok_np[:] = tok.numpy()
        return dict(launches_per_token=int(LIB.query('pb_batch_decoder_launches', dec)), graph=bool(LIB.query('pb_batch_decoder_graph', dec)),
                    tokens=n, loop_ms=(time.perf_counter() - t_loop) * 1e3, ended=ended, **(dict(anchors_placed=[ak]) if anchors is not None else {}))

    # ---- batched generation ----------------------------------------------------------------------------------------------------
    BATCH_MAX = 16                         # rows per batched decoder (PB_DECODE_BATCH_MAX); larger batches go in chunks

    def generate_batch(self, enc_ids, emask, sample_row, rngs, max_new=None, sampler=None, prefix=None, prefix_len=None, samples=None, forced=None,
                       refill=False, stop=None, order=None, allow=None, bar_allow=None, anchors=None):
        """B prompts at once, each with its own numpy RandomState. For every prompt b the result row equals the batch-1 `generate` of that
        prompt run with the global RNG set to rngs[b]'s state, token for token, and rngs[b] ends where the global RNG would end (the
        contract of tests/test_generate_batch_gpu.py). sample_row(row_logits, rng) is model.py:68-107 drawing its 8 uniforms from `rng`
        (None = the global stream); it is called for different rows from a small thread pool, one generator per row. enc_ids (B, S, 8),
        emask (B, S) or None; returns (B, S, 8) with PAD after each prompt's stop.
        Where the fused decode kernels cover the shape (bf16, head_dim 64 / 128, d a multiple of 256 up to 1024) and `sampler` names
        the constants, up to BATCH_MAX prompts share one batched device-sampled decoder (pb_batch_decoder_*); every other case runs
        the per-prompt loop over `generate` (_generate_batch_loop).
        prefix (B, P, 8) with prefix_len (B lengths, None = P each): row b is primed with prefix[b, :prefix_len[b]] as in `generate`; rows with
        length 0 are today's unprimed rows, so one batch may mix both (check_prefix holds the argument rules).
        samples (an int n or P ints, check_samples): enc_ids / emask / prefix / prefix_len describe P prompts and prompt p is sampled n_p
        times: rngs holds R = sum(n_p) generators and the result R rows, prompt-major, every row under the contract above. The R rows go
        through the fused decoder in chunks of BATCH_MAX; inside a chunk the encoder pass, the cross K|V projections and the prefill run
        once per distinct prompt (a prompt whose samples straddle a chunk boundary is encoded once per chunk). Shapes the fused decoder
        declines run the per-prompt loop over the repeated prompts. samples=None is one row per prompt with a cache slice of its own; an
        explicit samples=1 gives the same rows through the shared-cache form.
        forced (B, S, 8), -1 = free (check_forced): forced tokens, row b under `generate`'s contract with forced[b]; rows that are -1
        everywhere are today's rows, so one batch may mix both. With samples it describes the P prompts, like the prefix. The fused decoder
        reads the table on the device (pb_batch_decoder_force) and the host's verification applies it to its own tokens.
        refill (False, True = BATCH_MAX slots, or an int 2 .. BATCH_MAX; check_refill): ONE decoder of that many rows ("slots") for the
        whole call instead of one per chunk of BATCH_MAX: when a row stops, its slot goes to the next waiting prompt while the other rows
        decode on (_generate_batch_refill), so a short row does not wait for the longest row of its chunk and the set-up is paid once.
        Every row stays under the contract above; the result and the final generator states are those of refill=False. With no more rows
        than slots, or where the fused decoder does not cover the shape, the call runs as with refill=False. Not with `samples`.
        stop (B bar ids, check_stop): stop at a bar, row b under `generate`'s contract with stop[b]; pad[0] (256) = no stop, so one batch
        may mix both. With samples it describes the P prompts, like the prefix. The fused decoder's device sampler makes the same test
        (pb_batch_decoder_stop; a refilled slot gets its row's value with the hand-over, pb_batch_decoder_admit_stop), so a stopped row
        frees its place at once; the host's verification decides, as for every token. None, or pad[0] everywhere: the call without the
        argument. A call that passes `stop` finds last_decode['ended'][b]: 'special', 'bar' or 'limit', for every row of the call; a call
        without the argument leaves the record it always left.
        order (B ints, check_order): time-ordered sampling, row b under `generate`'s contract with order[b]; -1 = not ordered, so one
        batch may mix both. With samples it describes the P prompts, like the prefix. The fused decoder's device sampler applies the same
        mask (pb_batch_decoder_order; a refilled slot gets its row's floor with the hand-over, pb_batch_decoder_admit_order), so its
        prediction holds where the constraint bites; the host's verification decides, as for every token. None, or -1 everywhere: the
        call without the argument.
        allow ((B, V) bools, or a list of B masks / None; check_allow): allowed classes, row b under `generate`'s contract with allow[b];
        None = a free row, so one batch may mix both. With samples it describes the P prompts, like the prefix. The fused decoder's device
        sampler tests the same bits (pb_batch_decoder_allow uploads the distinct masks once; a refilled slot gets its row's mask index
        with the hand-over, pb_batch_decoder_admit_allow). None, or True everywhere: the call without the argument.
        bar_allow (a list of B bar schedules / None; check_bar_allow): row b under `generate`'s contract with bar_allow[b]; None = no
        schedule, so one batch may mix scheduled, masked and free rows. With samples it describes the P prompts. The device sampler
        picks the mask of heads 1 .. 7 by the bar it sampled (pb_batch_decoder_schedule uploads the distinct schedules once, their
        masks travel in pb_batch_decoder_allow's table; a refilled slot gets its row's index with the hand-over,
        pb_batch_decoder_admit_schedule). None, or no entry that removes a class: the call without the argument.
        anchors (a list of B anchor lists / None; check_anchors): anchored notes, row b under `generate`'s contract with anchors[b]; None
        or empty = a free prompt, so one batch may mix both. With samples it describes the P prompts. The device sampler applies the rule
        and keeps each row's counter (pb_batch_decoder_anchor uploads all anchors once; a refilled slot gets its row's slice with the
        hand-over, pb_batch_decoder_admit_anchor; a rewind restores the counter, pb_batch_decoder_seek_anchor). Not with `forced`. None,
        or no anchor in any list: the call without the argument; last_decode gains `anchors_placed`, one count per row, otherwise."""
        def done(out, with_ended=stop is not None):      # every path below records `ended`; a call without `stop` keeps the record it had
            if not with_ended and self.last_decode is not None:
                self.last_decode.pop('ended', None)
            return out
        _refuse_unmerged_lora(self, 'generate_batch')
        P = int(enc_ids.shape[0])
        slots = check_refill(refill, samples, self.BATCH_MAX)
        owner = check_samples(samples, P, len(rngs)) if samples is not None else list(range(P))        # row -> prompt
        ks, rows = check_prefix(prefix, prefix_len, P, int(enc_ids.shape[1]), self.pb.pad_word_np)
        forced = check_forced(forced, P, int(enc_ids.shape[1]), list(self.lay.sizes) if forced is not None else None, ks)
        pad0 = int(self.pb.pad_word_np[0])
        stop = check_stop(stop, P, pad0, owner if samples is not None else None)         # one entry per output row
        order = check_order(order, P, owner if samples is not None else None, order_max=pad0 - 1)            # ... and here
        plan = check_bar_allow(bar_allow, allow, P, self.lay, owner if samples is not None else None)    # ... and here: None, or both tables and both indices per row
        allow = plan[:2] if plan is not None else check_allow(allow, P, self.lay if allow is not None else None, owner if samples is not None else None)   # (distinct masks, one index per row)
        if len(rngs) != len(owner):
            raise PBError('generate_batch: %d generators for %d prompts' % (len(rngs), P))
        anc = check_anchors(anchors, P, int(enc_ids.shape[1]), self.pb.pad_word_np, ks, rows, stop, order, forced, max_new, owner if samples is not None else None)
        if anc is not None:                              # one list per output row; anchors imply time order
            anc, order = anc
        self._await_updates(2)
        R = len(owner)
        if R == 0:
            return torch.from_numpy(self.pb.pad_word_np).to(enc_ids.device).repeat(0, enc_ids.shape[1], 1)
        if not self._batch_decoder_covers(sampler):
            if samples is None:
                return done(self._generate_batch_loop(enc_ids, emask, sample_row, rngs, max_new, sampler, ks, rows, forced, stop, order, allow, plan, anc))
            return done(self._generate_batch_expanded(enc_ids, emask, sample_row, rngs, max_new, sampler, ks, rows, owner, forced, stop, order, allow, plan, anc))
        if slots and R > slots:
            out = self._generate_batch_refill(enc_ids, emask, sample_row, rngs, max_new, sampler, ks, rows, forced, slots, stop, order, allow, plan, anc)
            if out is not None:                          # None: the fused decoder declines the shape -- the chunks' per-prompt loops, as ever
                return done(out)
        outs, ended, got = [], [], []
        for c0 in range(0, R, self.BATCH_MAX):
            own = owner[c0:c0 + self.BATCH_MAX]
            st = stop[c0:c0 + len(own)] if stop is not None else None
            st = st if st is not None and any(v != pad0 for v in st) else None     # a chunk without a real stop is today's chunk
            od = order[c0:c0 + len(own)] if order is not None else None
            od = od if od is not None and any(v != -1 for v in od) else None       # ... and one without an ordered row
            al = _slice_allow(allow, c0, c0 + len(own))                           # ... and one without a masked row
            pl = _slice_schedule(plan, c0, c0 + len(own))                         # ... and one without a scheduled row
            al = pl[:2] if pl is not None else al                                 # (a scheduled chunk uploads the table even if its rows' own masks are free)
            p0, p1 = own[0], own[-1] + 1                 # prompt-major rows: the chunk's prompts are a range
            outs.append(self._generate_batch_chunk(enc_ids[p0:p1], emask[p0:p1] if emask is not None else None, sample_row,
                                                   rngs[c0:c0 + len(own)], max_new, sampler, ks[p0:p1], rows[p0:p1] if rows is not None else None,
                                                   groups=[p - p0 for p in own] if samples is not None else None,
                                                   forced=forced[p0:p1] if forced is not None and (forced[p0:p1] != -1).any() else None, stop=st, order=od,
                                                   allow=al, sched=pl, anchors=_slice_anchors(anc, c0, c0 + len(own))))
            ended += (self.last_decode or {}).get('ended') or [None] * len(own)
            got += (self.last_decode or {}).get('anchors_placed') or [0] * len(own)
        if len(outs) > 1 and self.last_decode is not None:                # last_decode describes the last chunk; `ended` covers every row
            self.last_decode['ended'] = ended
        if anc is not None and self.last_decode is not None:              # ... and so does `anchors_placed`, where anchors were given
            self.last_decode['anchors_placed'] = got
        return done(torch.cat(outs, 0))

    def _generate_batch_expanded(self, enc_ids, emask, sample_row, rngs, max_new, sampler, ks, rows, owner, forced=None, stop=None, order=None,
                                 allow=None, sched=None, anchors=None):
        """The per-prompt loop over the rows of `owner` (row -> prompt): every row runs the batch-1 `generate` of its prompt. stop: one
        entry per ROW (check_stop expands it), or None; order likewise (check_order), and allow's indices (check_allow) and sched's
        (check_bar_allow) and anchors' lists (check_anchors)."""
        idx = torch.as_tensor(owner, dtype=torch.long)
        return self._generate_batch_loop(enc_ids[idx.to(enc_ids.device)], emask[idx.to(emask.device)] if emask is not None else None, sample_row, rngs,
                                         max_new, sampler, [ks[p] for p in owner], rows[idx] if rows is not None else None,
                                         forced[idx.numpy()] if forced is not None else None, stop, order, allow, sched, anchors)

    def _batch_decoder_covers(self, sampler):
        """The switches under which generate_batch tries the fused decoder; whether it covers the shape is pb_batch_decoder_create's rule."""
        return sampler is not None and _DECODE_SPEC and _DECODE_GRAPH >= 0

    def _generate_batch_loop(self, enc_ids, emask, sample_row, rngs, max_new, sampler, ks=None, rows=None, forced=None, stop=None, order=None,
                             allow=None, sched=None, anchors=None):
        """The per-prompt loop: each row's generator state is swapped into the global RNG for its batch-1 `generate` and copied back; the
        caller's global state is restored afterwards. ks / rows: the prefix lengths and rows of check_prefix (None: unprimed); forced: one
        checked table per row (check_forced) or None; stop: one stop bar per row (check_stop) or None; order: one bar floor per row
        (check_order) or None; allow: check_allow's result with one index per row, or None; sched: check_bar_allow's result likewise, or None;
        anchors: check_anchors' lists, one entry per row, or None."""
        saved = np.random.get_state()
        outs, ended, pad0 = [], [], int(self.pb.pad_word_np[0])
        got = []
        masks = unpack_allow(allow, self.lay.vocab)
        scheds = unpack_schedule(sched, self.lay.vocab)
        try:
            for b in range(int(enc_ids.shape[0])):
                np.random.set_state(rngs[b].get_state())
                pre = rows[b:b + 1, :ks[b]] if rows is not None and ks[b] else None
                outs.append(self.generate(enc_ids[b:b + 1], emask[b:b + 1] if emask is not None else None, lambda r, **kw: sample_row(r, None, **kw),
                                          max_new=max_new, sampler=sampler, prefix=pre, forced=forced[b:b + 1] if forced is not None else None,
                                          stop=stop[b] if stop is not None else pad0,         # 256: no stop, and the row's `ended`
                                          order=order[b] if order is not None else None,
                                          allow=masks[b].numpy() if masks is not None and masks[b] is not None else None,
                                          bar_allow=[scheds[b]] if scheds is not None and scheds[b] is not None else None,
                                          anchors=[anchors[b]] if anchors is not None and anchors[b] is not None else None))
                ended.append((self.last_decode or {}).get('ended'))
                got += (self.last_decode or {}).get('anchors_placed') or [0]
                rngs[b].set_state(np.random.get_state())
        finally:
            np.random.set_state(saved)
        self.last_decode = dict(batched=False, batch=int(enc_ids.shape[0]), ended=ended, **(dict(scheduled=True) if sched is not None else {}),
                                **(dict(anchors_placed=got) if anchors is not None else {}))
        return torch.cat(outs, 0)

    def _generate_batch_chunk(self, enc_ids, emask, sample_row, rngs, max_new, sampler, ks, rows, groups=None, forced=None, stop=None, order=None,
                              allow=None, sched=None, anchors=None):
        """<= BATCH_MAX rows through one fused decoder: the set-up of _decoder_run (groups as there), then the device-ahead / host-behind
        loop with per-row draws, per-row verification and per-row rewinds (_decode_device_sampled). stop: one stop bar per ROW, or None;
        order: one bar floor per ROW, or None; allow: check_allow's result with one index per ROW, or None; sched: check_bar_allow's
        result likewise, or None; anchors: check_anchors' lists, one entry per ROW, or None."""
        with torch.no_grad(), self._decoder_run(enc_ids, emask, ks, rows, groups) as run:
            if run.dec is None:                                            # not covered: the per-prompt loop
                return self._generate_batch_expanded(enc_ids, emask, sample_row, rngs, max_new, sampler, ks, rows, run.groups, forced, stop, order, allow, sched,
                                                     anchors)
            fault = getattr(self, 'decode_fault_row', None) or (-1, 0)     # tests: the device's choice of one row corrupted
            info = self._decode_device_sampled(run.dec, run.B, run.S, lambda b, row, **kw: sample_row(row, rngs[b], **kw), [r.get_state() for r in rngs],
                                               sampler, run.res_cpu, run.pad_cpu, max_new, fault, inline_verify=False, starts=run.starts,
                                               forced=np.ascontiguousarray(forced[np.asarray(run.groups)]) if forced is not None else None, stop=stop,
                                               order=order, allow=allow, sched=sched, anchors=anchors)
        self.last_decode = dict(info, s_enc=run.s_enc, batched=True, batch=run.B, prefix=run.starts, prefill_ms=run.prefill_ms(), groups=run.groups,
                                encoder_passes=run.G, prefill_passes=sum(1 for k in ks if 0 < k < run.S), setup_ms=run.setup_ms,
                                cross_cache_bytes=sum(t.numel() * t.element_size() for t in run.bufs['kvc']))
        return run.res_cpu.to(enc_ids.device)

    def _generate_batch_refill(self, enc_ids, emask, sample_row, rngs, max_new, sampler, ks, rows, forced, n, stop=None, order=None, allow=None, sched=None,
                               anchors=None):
        """R > n rows through ONE fused decoder of n slots (pb_batch_decoder_dynamic): a slot whose row has stopped is handed to the next
        waiting prompt (pb_batch_decoder_admit) while the other slots decode on. refill.RefillSchedule keeps the books: rows are admitted
        in row order into the lowest free slot, and the cross K|V caches hold n + E slices so that the next prompts' batch-1 encoder
        passes, projections and prefills run AHEAD on the caller's stream while the decoder is busy; a hand-over is then a slice index plus
        the row's draws, forced entries and mask (and, for a primed row, a device copy of its prefilled cache rows into the slot).
        The set-up is _decoder_run's, once; the loop is _decode_device_sampled's with slots for rows: the first n rows start as a chunk
        starts (sampler_init, force, start), the device samples ahead, the host verifies one run behind from the pinned logs (indexed by
        SLOT: an occupant's log rows are read before the next one is admitted) and rewinds a row alone. Each row's draws are made at its
        admission from a copy of rngs[r] (forced_draws). stop (R stop bars or None): the first n rows' values go up as a chunk's do
        (pb_batch_decoder_stop), a later row's is staged in front of its admission (pb_batch_decoder_admit_stop); a row without a stop
        stages nothing and its slot gets pad[0], never the previous occupant's value. order (R bar floors or None) travels the same way
        (pb_batch_decoder_order, pb_batch_decoder_admit_order; a free row stages nothing and its slot gets -1), and so does allow (check_allow's
        result for the R rows: the table of ALL rows' masks goes up at the start, pb_batch_decoder_allow, and a later row's index is staged,
        pb_batch_decoder_admit_allow), and sched (check_bar_allow's result: pb_batch_decoder_schedule, pb_batch_decoder_admit_schedule; a
        successor without a schedule stages nothing and its slot gets -1), and anchors (check_anchors' R lists: the table of ALL rows'
        anchors goes up at the start, pb_batch_decoder_anchor, a later row's slice is staged, pb_batch_decoder_admit_anchor, and the
        host's counter of a rewound row goes back with pb_batch_decoder_seek_anchor). Returns the (R, S, 8) result, or None -- before any encoder work -- where
        pb_batch_decoder_create declines the shape."""
        R, S, dev = int(enc_ids.shape[0]), int(enc_ids.shape[1]), enc_ids.device
        pad_cpu = torch.from_numpy(self.pb.pad_word_np)
        with torch.no_grad():
            em, enc16 = self._prompt_inputs(enc_ids, emask)
            t_setup = time.perf_counter()
            s_enc = [self._key_extent(em[r:r + 1] if em is not None else None, S) for r in range(R)]
            NS = n + min(n, R - n)                                         # slices: one per slot plus the prompts prepared ahead
            em_slots = em[:n].clone() if em is not None else None          # the decoder's mask rows belong to the slots
            bp, bufs = self._decode_plan(n, S, s_enc[:n], em_slots, dev, G=NS)
            dec = self._decoder_create(bp)
            if dec is None:
                return None
            try:
                return self._refill_run(dec, bufs, enc16, em, s_enc, sample_row, rngs, max_new, sampler, ks, rows, forced, n, NS, t_setup,
                                        pad_cpu, stop, order, allow, sched, anchors).to(dev)
            finally:
                LIB.call('pb_batch_decoder_destroy', dec)

    def _refill_run(self, dec, bufs, enc16, em, s_enc, sample_row, rngs, max_new, sampler, ks, rows, forced, n, NS, t_setup, pad_cpu, stop=None, order=None,
                    allow=None, bars=None, anchors=None):
        """The body of _generate_batch_refill on a created decoder (destroyed by the caller). Returns res_cpu."""
        import ctypes
        from collections import deque
        from concurrent.futures import ThreadPoolExecutor
        from .refill import RefillSchedule
        R, S, dev = int(enc16.shape[0]), int(enc16.shape[1]), enc16.device
        K, vocab = 8, self.lay.vocab
        LIB.call('pb_batch_decoder_dynamic', dec, NS)
        sched = RefillSchedule(R, n, NS)
        res_cpu = pad_cpu.repeat(R, S, 1)
        lim = [S if max_new is None else max(0, min(S, k + int(max_new))) for k in ks]
        primed = [0 < ks[r] < S for r in range(R)]
        # everything a later prepare needs from the host goes up now: behind a fence the caller's stream waits for the decoder, and a
        # pageable copy enqueued there would make the host wait with it
        pre_in = {r: self._prefill_inputs(rows[r], ks[r], S, dev) for r in range(R) if primed[r]}
        stage = [torch.zeros(NS, S, 2 * self.d, dtype=self.xdt, device=dev) for _ in range(self.ND)] if any(primed[n:]) else None
        em_host = np.ascontiguousarray(em.cpu().numpy(), dtype=np.float32) if em is not None else None
        timers, counts = [], dict(encoder_passes=0, admissions=0)
        stream = ops._stream
        used = set()                               # slices that have had a reader

        def prepare(r, c, kvs_rows, ahead=False):
            """Row r's batch-1 encoder pass, cross K|V projections into slice c and prefill into kvs_rows, as a lone `generate` runs them.
            ahead: the decoder is running -- the projected embedding table it reads was built by the first rows' passes from the same
            weights and is not rebuilt under it."""
            emb = em[r:r + 1] if em is not None else None
            if ahead:
                self._tables_ready = True
            _, enc_out = self.forward_hidden(enc16[r:r + 1], None, emb, None, False, 0)
            for l in range(self.ND):
                self._linear(enc_out, 'dec.%d.wkv_c' % l, 'dec.%d.bkv_c' % l, bufs['kvc'][l][c], S, 2 * self.d, self.d)
            if ks[r]:
                if ahead and primed[r]:
                    self._tables_ready = True
                timers.append(self._prefill(enc16[r:r + 1], emb, rows[r], ks[r], kvs_rows, inputs=pre_in.get(r)))
                res_cpu[r, :ks[r]] = rows[r, :ks[r]]
            used.add(c)
            counts['encoder_passes'] += 1

        for b in range(n):                                                 # the first n rows: slot b, slice b, as a chunk sets them up
            r, c = sched.prepare()
            prepare(r, c, [t[b] for t in bufs['kvs']])
            assert sched.admit() == (b, b, b)
        LIB.call('pb_batch_decoder_reset', dec, stream(), _DECODE_GRAPH)
        torch.cuda.current_stream().synchronize()
        setup_ms = (time.perf_counter() - t_setup) * 1e3

        def draws(r):
            ahead = np.random.RandomState()
            ahead.set_state(rngs[r].get_state())
            return forced_draws(ahead, forced[r] if forced is not None else None, ks[r], S).reshape(-1)

        def first_tok(r):
            return np.ascontiguousarray((res_cpu[r, ks[r] - 1].numpy() if ks[r] else np.asarray(self.pb.sos_word_np)).astype(np.int16))

        fault = getattr(self, 'decode_fault_row', None) or (-1, 0)         # tests: the device's choice of one SLOT corrupted
        n8 = np.asarray(self.lay.sizes, dtype=np.int32)
        off8 = np.asarray(self.lay.seg_off[:8], dtype=np.int32)
        pad8 = np.asarray(self.pb.pad_word_np, dtype=np.int32)
        t8, p8 = np.asarray(sampler['T'], dtype=np.float32), np.asarray(sampler['P'], dtype=np.float32)
        U = np.ascontiguousarray(np.stack([draws(r) for r in range(n)]))
        LIB.call('pb_batch_decoder_sampler_init', dec, t8.ctypes.data, p8.ctypes.data, n8.ctypes.data, off8.ctypes.data, pad8.ctypes.data,
                 U.ctypes.data, n * S * 8, max(lim), int(fault[0]), int(fault[1]))
        if forced is not None:                                             # the graphs end in the forced sampler for the whole run
            LIB.call('pb_batch_decoder_force', dec, np.ascontiguousarray(forced[:n]).ctypes.data)
        pad0 = int(pad_cpu[0])
        svs = [stop_vector(pad_cpu, stop[r] if stop is not None else None) for r in range(R)]
        ended = ['limit'] * R
        if stop is not None and any(v != pad0 for v in stop[:n]):
            LIB.call('pb_batch_decoder_stop', dec, np.asarray(stop[:n], dtype=np.int32).ctypes.data)
        if order is not None and any(v != -1 for v in order[:n]):
            LIB.call('pb_batch_decoder_order', dec, np.asarray(order[:n], dtype=np.int32).ctypes.data)
        if allow is not None:                                              # the masks of ALL rows: a later row's index points into this table
            LIB.call('pb_batch_decoder_allow', dec, allow[0].ctypes.data, allow[0].shape[0], allow[0].shape[1],
                     np.asarray(allow[1][:n], dtype=np.int32).ctypes.data)
        if bars is not None:                                              # ... and the schedules of ALL rows, behind the masks they point to
            rs = np.asarray(bars[3][:n], dtype=np.int32)                   # held until the call returns
            LIB.call('pb_batch_decoder_schedule', dec, bars[2].ctypes.data, bars[2].shape[0], bars[2].shape[1], rs.ctypes.data)
        if anchors is not None:                                            # ... and the anchors of ALL rows; the first n rows' slices with them
            atab, abase, acnt = _anchor_table(anchors)
            LIB.call('pb_batch_decoder_anchor', dec, atab.ctypes.data, atab.shape[0], np.ascontiguousarray(abase[:n]).ctypes.data,
                     np.ascontiguousarray(acnt[:n]).ctypes.data)
        placed = [0] * R                           # anchors the HOST has written, per row
        masks = unpack_allow(allow, vocab)
        scheds = unpack_schedule(bars, vocab)
        sos = torch.from_numpy(self.pb.sos_word_np)
        lp, tp = ctypes.c_void_p(), ctypes.c_void_p()
        LIB.call('pb_batch_decoder_logs', dec, ctypes.byref(lp), ctypes.byref(tp))
        log_logits = torch.from_numpy(np.ctypeslib.as_array((ctypes.c_float * (n * S * vocab)).from_address(lp.value)).reshape(n, S, vocab))
        log_tok = np.ctypeslib.as_array((ctypes.c_int16 * (n * S * 8)).from_address(tp.value)).reshape(n, S, 8)
        first = np.ascontiguousarray(np.stack([first_tok(r) for r in range(n)]))
        last_pos, lim32 = np.asarray([ks[r] - 1 for r in range(n)], dtype=np.int32), np.asarray(lim[:n], dtype=np.int32)
        LIB.call('pb_batch_decoder_start', dec, last_pos.ctypes.data, first.ctypes.data, lim32.ctypes.data)
        slot_row = list(range(n))                  # the row in each slot (None: empty)
        nxt = [ks[r] for r in range(n)]            # next position the enqueued work decodes, per slot
        tokens, rewinds = [0] * R, [0] * R
        row_slot = list(range(n)) + [-1] * (R - n)                         # the slot each row sat in (-1: it had nothing to decode)
        runs = deque()
        stat = dict(steps=0, row_steps=0, host_s=0.0)

        def top_up():
            """Prepare waiting rows ahead into free slices. A slice is reused only behind its last reader's last enqueued step."""
            while True:
                got = sched.prepare()
                if got is None:
                    return
                r, c = got
                if c in used:
                    LIB.call('pb_batch_decoder_fence', dec, stream())
                prepare(r, c, [t[c] for t in stage] if stage is not None else None, ahead=True)

        def hand_over(s):
            """The free slot s goes to the next row (prepared ahead where a slice was free in time). Rows with nothing to decode pass through."""
            while True:
                got = sched.admit()
                if got is None:
                    top_up()
                    got = sched.admit()
                    if got is None:                                        # no row waits: the slot stays empty
                        slot_row[s] = None
                        return
                r, s2, c = got
                assert s2 == s
                if lim[r] <= ks[r]:
                    sched.finish(s)
                    continue
                if primed[r]:                                              # its prefilled cache rows, behind the previous occupant's last step
                    LIB.call('pb_batch_decoder_fence', dec, stream())
                    for l in range(self.ND):
                        bufs['kvs'][l][s, :ks[r]].copy_(stage[l][c, :ks[r]])
                u, tok = draws(r), first_tok(r)
                fr = np.ascontiguousarray(forced[r]) if forced is not None and (forced[r] != -1).any() else None
                if stop is not None and stop[r] != pad0:                   # stored by the admit's kernel, with the row's position and done = 0
                    LIB.call('pb_batch_decoder_admit_stop', dec, s, stop[r])
                if order is not None and order[r] != -1:                   # likewise; a free successor of an ordered row gets -1
                    LIB.call('pb_batch_decoder_admit_order', dec, s, order[r])
                if allow is not None and allow[1][r] != -1:                # likewise; a free successor of a masked row gets -1
                    LIB.call('pb_batch_decoder_admit_allow', dec, s, allow[1][r])
                if bars is not None and bars[3][r] != -1:                # likewise; a successor without a schedule gets -1
                    LIB.call('pb_batch_decoder_admit_schedule', dec, s, bars[3][r])
                if anchors is not None and anchors[r] is not None:         # likewise, behind its stop bar and floor; a free successor gets none
                    LIB.call('pb_batch_decoder_admit_anchor', dec, s, int(abase[r]), int(acnt[r]))
                LIB.call('pb_batch_decoder_admit', dec, s, c, s_enc[r], ks[r] - 1, tok.ctypes.data, lim[r], u.ctypes.data,
                         fr.ctypes.data if fr is not None else None, em_host[r].ctypes.data if em_host is not None else None, stream())
                counts['admissions'] += 1
                slot_row[s], nxt[s], row_slot[r] = r, ks[r], s
                return

        def finish(s, i):
            LIB.call('pb_batch_decoder_seek', dec, s, i, None)
            sched.finish(s)
            hand_over(s)

        def launch():
            livs = [s for s in range(n) if slot_row[s] is not None]
            cnt = min(K, max(lim[slot_row[s]] - nxt[s] for s in livs))
            tk = int(LIB.query('pb_batch_decoder_launch', dec, cnt, None))
            if tk < 0:
                raise PBError('pb_batch_decoder_launch failed (%d): %s' % (tk, LIB.load().pb_last_error().decode()))
            spans = [None] * n
            for s in livs:
                e = min(lim[slot_row[s]], nxt[s] + cnt)
                spans[s] = [slot_row[s], nxt[s], e]
                stat['row_steps'] += e - nxt[s]
                nxt[s] = e
            runs.append((tk, spans))
            stat['steps'] += cnt

        def verify(s, r, a, e):                    # positions a .. e-1 of row r in slot s, in order: None, ('stop', i) or ('seek', i, ids)
            for i in range(a, e):
                tok = scheduled_token(forced[r, i] if forced is not None else None, lambda **kw: sample_row(log_logits[s, i], rngs[r], **kw),
                                    masks[r] if masks is not None else None, scheds[r] if scheds is not None else None, order[r] if order is not None else None,
                                    res_cpu[r, i - 1] if i else sos, pad_cpu)
                if anchors is not None:
                    tok, placed[r] = anchored_token(tok, anchors[r], placed[r], svs[r], pad_cpu)
                tokens[r] += 1
                if (tok >= svs[r]).any():
                    ended[r] = end_reason(tok, pad_cpu)
                    return ('stop', i)
                res_cpu[r, i] = tok
                t16 = tok.numpy().astype(np.int16)
                if not np.array_equal(t16, log_tok[s, i]):
                    return ('seek', i, t16)
            return None

        pending = lambda: any(slot_row[s] is not None and nxt[s] < lim[slot_row[s]] for s in range(n))
        t_loop = time.perf_counter()
        for s in range(n):                                                 # rows with nothing to decode leave before the first step
            if lim[s] <= ks[s]:
                finish(s, 0)
        with ThreadPoolExecutor(max_workers=min(n, 8)) as pool:
            while runs or pending():
                while len(runs) < 2 and pending():
                    launch()
                top_up()                                                   # the next prompts' passes run while the decoder is busy
                tk, spans = runs.popleft()
                LIB.call('pb_batch_decoder_wait', dec, tk)
                t_h = time.perf_counter()
                todo = [s for s in range(n) if spans[s] is not None and spans[s][0] == slot_row[s] and spans[s][2] > spans[s][1]]
                outcome = dict(zip(todo, pool.map(lambda s: verify(s, *spans[s]), todo)))
                stat['host_s'] += time.perf_counter() - t_h
                for s in todo:
                    out, (r, _, e) = outcome[s], spans[s]
                    if out is None:
                        if e >= lim[r]:                                    # the row's last position is verified
                            finish(s, e - 1)
                    elif out[0] == 'stop':
                        finish(s, out[1])
                    else:                                                  # drain, move slot s back; its spans in the queued runs are void
                        i = out[1]
                        rewinds[r] += 1
                        LIB.call('pb_batch_decoder_seek', dec, s, i, out[2].ctypes.data)
                        if anchors is not None and anchors[r] is not None:  # the device's counter ran ahead with the discarded positions
                            LIB.call('pb_batch_decoder_seek_anchor', dec, s, placed[r])
                        nxt[s] = i + 1
                        for _, sp in runs:
                            if sp[s] is not None and sp[s][0] == r:
                                sp[s][1] = sp[s][2] = i + 1
                        if i + 1 >= lim[r]:                                # rewound at its last position: nothing left to decode
                            finish(s, i)
        assert sched.done(), (sched.finished, R)
        self.last_decode = dict(launches_per_token=int(LIB.query('pb_batch_decoder_launches', dec)), graph=bool(LIB.query('pb_batch_decoder_graph', dec)),
                                tokens=tokens, rewinds=rewinds, steps=stat['steps'], row_steps=stat['row_steps'], loop_ms=(time.perf_counter() - t_loop) * 1e3,
                                host_ms=stat['host_s'] * 1e3, device_sampler=True, **self._note_sampler_form(dec), tokens_per_graph_replay=K, refill=n, slices=NS, **(dict(scheduled=True) if bars is not None else {}),
                                **(dict(anchors_placed=placed) if anchors is not None else {}),
                                admissions=counts['admissions'], row_slot=row_slot, encoder_passes=counts['encoder_passes'], s_enc=s_enc, batched=True, batch=n,
                                prefix=list(ks), prefill_ms=sum(t() for t in timers), prefill_passes=sum(primed), setup_ms=setup_ms, ended=ended,
                                cross_cache_bytes=sum(t.numel() * t.element_size() for t in bufs['kvc']))
        return res_cpu

    def _decode_device_sampled(self, dec, B, S, sample, states, sampler, res_cpu, pad_cpu, max_new, fault, inline_verify, starts=None, forced=None, stop=None,
                               order=None, allow=None, sched=None, anchors=None):
        """The decode loop without a host round trip per token (round 6), for B rows. The 8 uniform draws of a position do not depend on its
        logits (np.random.choice inside nucleus(), model.py:97), so each row's S x 8 are drawn AHEAD from a copy of its generator state
        (`states`: the global RNG's for `generate`, rngs[b]'s for `generate_batch`) and uploaded; the device then samples every position
        itself (pb_batch_decoder_sampler_init: model.py:68-107 in pb_nucleus_rows' arithmetic order) and runs on, K steps per hipGraph
        replay, two runs in flight. The host follows one run behind: for every row position it calls sample(b, logged row) -- the
        reference code path, consuming that row's generator exactly as the per-token loop does, so its state ends where the reference's
        does -- and compares with the ids the device chose. They differ only where the device's softmax rounding (1 ulp against torch's CPU
        softmax) crosses a threshold or a tie; then that row alone is rewound to the position with the host's token (pb_batch_decoder_seek
        drains, then moves that row only) and everything it decoded behind it is discarded. A row whose host token is special stops there.
        The result is the host's, token for token. inline_verify: the rows are replayed in this thread (B = 1) instead of a small pool.
        starts[b] = k_b (primed rows): row b's positions 0 .. k_b - 1 are its prefix (in res_cpu, their K|V in the cache), so it starts at
        k_b with input res_cpu[b, k_b - 1], its draws start at position k_b and it stops before min(S, k_b + max_new)
        (pb_batch_decoder_start: per-row positions, inputs and limits in one upload).
        forced (B, S, 8) int16, -1 = free (check_forced), or None: the table goes to the device sampler (pb_batch_decoder_force, between
        sampler_init and start), the draws made ahead follow it (forced_draws: a fully given position draws nothing) and the host applies
        it to its own tokens (forced_token: sample() is called only at positions with a free head, the stop test sees the token after
        forcing), so a given head cannot disagree and the result stays the host's.
        stop (B stop bars, check_stop) or None: the values go to the device sampler behind sampler_init and force (pb_batch_decoder_stop: its
        done test of head 0 then compares against the row's bar) and the host's stop test uses the row's stop_vector. The device's done
        flag stays a prediction: where it stopped a row the host does not stop, or the other way round, the tokens differ and the rewind
        below handles it. Returns `ended` per row: 'special', 'bar' or 'limit', as the host decided.
        order (B bar floors, check_order) or None: the values go to the device sampler too (pb_batch_decoder_order: it masks heads 0 and 1
        against the row's decoder input on the device) and the host samples every position through ordered_token, with prev = the row's
        previous result row (the prefix's last row at k_b, the SOS row at 0). A device that ignored the mask would be rewound wherever it
        bites; one that applies it differs from the host as rarely as the unordered sampler does.
        allow (check_allow's result with B indices) or None: the distinct masks and the rows' indices go to the device sampler
        (pb_batch_decoder_allow: it tests the class's bit where it forms the quotient) and the host samples every position through
        allowed_token with the row's mask; the logged logits rows are the raw ones.
        sched (check_bar_allow's result with B indices; allow is then its first two members) or None: the distinct schedules and the rows'
        indices go to the device sampler behind the masks (pb_batch_decoder_schedule: it picks the mask of heads 1 .. 7 by the bar of the
        token it samples) and the host samples every position through scheduled_token with the row's schedule.
        anchors (check_anchors' lists, B entries; order then holds a floor >= 0 for every anchored row) or None: the table of all anchors
        and each row's slice go to the device sampler last (pb_batch_decoder_anchor: its last stage applies the rule and advances the
        row's counter on the device) and the host passes every candidate through anchored_token with a counter of its own per row. The
        counter is state the device moved while running ahead, so a rewind restores it from the host's (pb_batch_decoder_seek_anchor
        behind pb_batch_decoder_seek). Returns `anchors_placed` per row then."""
        import contextlib
        import ctypes
        from collections import deque
        from concurrent.futures import ThreadPoolExecutor
        K, vocab = 8, self.lay.vocab
        starts = list(starts) if starts is not None else [0] * B
        lim = [S if max_new is None else max(0, min(S, k + int(max_new))) for k in starts]
        limit = max(lim)
        U = np.zeros((B, S * 8), dtype=np.float64)
        for b in range(B):
            ahead = np.random.RandomState()
            ahead.set_state(states[b])
            U[b] = forced_draws(ahead, forced[b] if forced is not None else None, starts[b], S).reshape(-1)
        n8 = np.asarray(self.lay.sizes, dtype=np.int32)
        off8 = np.asarray(self.lay.seg_off[:8], dtype=np.int32)
        pad8 = np.asarray(self.pb.pad_word_np, dtype=np.int32)
        t8, p8 = np.asarray(sampler['T'], dtype=np.float32), np.asarray(sampler['P'], dtype=np.float32)
        LIB.call('pb_batch_decoder_sampler_init', dec, t8.ctypes.data, p8.ctypes.data, n8.ctypes.data, off8.ctypes.data, pad8.ctypes.data,
                 U.ctypes.data, B * S * 8, limit, int(fault[0]), int(fault[1]))
        if forced is not None:
            LIB.call('pb_batch_decoder_force', dec, forced.ctypes.data)
        svs = [stop_vector(pad_cpu, stop[b] if stop is not None else None) for b in range(B)]
        ended = ['limit'] * B
        if stop is not None:
            LIB.call('pb_batch_decoder_stop', dec, np.asarray(stop, dtype=np.int32).ctypes.data)
        if order is not None:
            LIB.call('pb_batch_decoder_order', dec, np.asarray(order, dtype=np.int32).ctypes.data)
        if allow is not None:
            LIB.call('pb_batch_decoder_allow', dec, allow[0].ctypes.data, allow[0].shape[0], allow[0].shape[1],
                     np.asarray(allow[1], dtype=np.int32).ctypes.data)
        if sched is not None:
            rs = np.asarray(sched[3], dtype=np.int32)                      # held until the call returns
            LIB.call('pb_batch_decoder_schedule', dec, sched[2].ctypes.data, sched[2].shape[0], sched[2].shape[1], rs.ctypes.data)
        if anchors is not None:                                            # behind the stop bars and floors it is checked against
            atab, abase, acnt = _anchor_table(anchors)                     # held until the call returns
            LIB.call('pb_batch_decoder_anchor', dec, atab.ctypes.data, atab.shape[0], abase.ctypes.data, acnt.ctypes.data)
        placed = [0] * B                           # anchors the HOST has written, per row
        masks = unpack_allow(allow, vocab)
        scheds = unpack_schedule(sched, vocab)
        sos = torch.from_numpy(self.pb.sos_word_np)
        lp, tp = ctypes.c_void_p(), ctypes.c_void_p()
        LIB.call('pb_batch_decoder_logs', dec, ctypes.byref(lp), ctypes.byref(tp))
        log_logits = torch.from_numpy(np.ctypeslib.as_array((ctypes.c_float * (B * S * vocab)).from_address(lp.value)).reshape(B, S, vocab))
        log_tok = np.ctypeslib.as_array((ctypes.c_int16 * (B * S * 8)).from_address(tp.value)).reshape(B, S, 8)
        first = np.ascontiguousarray(np.tile(np.asarray(self.pb.sos_word_np, dtype=np.int16), (B, 1)))
        for b in range(B):
            if starts[b]:
                first[b] = res_cpu[b, starts[b] - 1].numpy().astype(np.int16)
        last_pos, lim32 = np.asarray([k - 1 for k in starts], dtype=np.int32), np.asarray(lim, dtype=np.int32)
        LIB.call('pb_batch_decoder_start', dec, last_pos.ctypes.data, first.ctypes.data, lim32.ctypes.data)
        nxt = list(starts)                         # next position the enqueued work decodes, per row
        live = [lim[b] > starts[b] for b in range(B)]     # the host has not stopped the row
        tokens, rewinds = [0] * B, [0] * B
        runs = deque()
        steps, host_s = 0, 0.0

        def launch(tok=None):
            nonlocal steps
            cnt = min(K, max(lim[b] - nxt[b] for b in range(B) if live[b]))
            tk = int(LIB.query('pb_batch_decoder_launch', dec, cnt, None if tok is None else tok.ctypes.data))
            if tk < 0:
                raise PBError('pb_batch_decoder_launch failed (%d): %s' % (tk, LIB.load().pb_last_error().decode()))
            spans = []
            for b in range(B):
                s = nxt[b]
                e = min(lim[b], s + cnt) if live[b] else s
                spans.append([s, e])
                nxt[b] = e
            runs.append((tk, spans))
            steps += cnt

        def verify(b, s, e):                       # positions s .. e-1 of row b, in order: None, ('stop', i) or ('seek', i, ids)
            for i in range(s, e):
                tok = scheduled_token(forced[b, i] if forced is not None else None, lambda **kw: sample(b, log_logits[b, i], **kw),
                                    masks[b] if masks is not None else None, scheds[b] if scheds is not None else None, order[b] if order is not None else None,
                                    res_cpu[b, i - 1] if i else sos, pad_cpu)
                if anchors is not None:
                    tok, placed[b] = anchored_token(tok, anchors[b], placed[b], svs[b], pad_cpu)
                tokens[b] += 1
                if (tok >= svs[b]).any():
                    ended[b] = end_reason(tok, pad_cpu)
                    return ('stop', i)
                res_cpu[b, i] = tok
                t16 = tok.numpy().astype(np.int16)
                if not np.array_equal(t16, log_tok[b, i]):
                    return ('seek', i, t16)
            return None

        pending = lambda: any(live[b] and nxt[b] < lim[b] for b in range(B))
        t_loop = time.perf_counter()
        with (contextlib.nullcontext() if inline_verify else ThreadPoolExecutor(max_workers=min(B, 8))) as pool:
            while runs or pending():
                while len(runs) < 2 and pending():
                    launch()
                tk, spans = runs.popleft()
                LIB.call('pb_batch_decoder_wait', dec, tk)
                t_h = time.perf_counter()
                todo = [b for b in range(B) if live[b] and spans[b][1] > spans[b][0]]
                outcome = dict(zip(todo, (pool.map if pool else map)(lambda b: verify(b, *spans[b]), todo)))
                host_s += time.perf_counter() - t_h
                for b in todo:
                    r = outcome[b]
                    if r is None:
                        continue
                    if r[0] == 'stop':
                        live[b] = False
                        LIB.call('pb_batch_decoder_seek', dec, b, r[1], None)
                    else:                                                  # drain, move row b back; its spans in the queued runs are void
                        i = r[1]
                        rewinds[b] += 1
                        LIB.call('pb_batch_decoder_seek', dec, b, i, r[2].ctypes.data)
                        if anchors is not None and anchors[b] is not None:  # the device's counter ran ahead with the discarded positions
                            LIB.call('pb_batch_decoder_seek_anchor', dec, b, placed[b])
                        nxt[b] = i + 1
                        for _, sp in runs:
                            sp[b][0] = sp[b][1] = i + 1
        return dict(launches_per_token=int(LIB.query('pb_batch_decoder_launches', dec)), graph=bool(LIB.query('pb_batch_decoder_graph', dec)),
                    tokens=tokens, rewinds=rewinds, steps=steps, loop_ms=(time.perf_counter() - t_loop) * 1e3, host_ms=host_s * 1e3,
                    device_sampler=True, **self._note_sampler_form(dec), tokens_per_graph_replay=K, ended=ended,
                    **(dict(scheduled=True) if sched is not None else {}), **(dict(anchors_placed=placed) if anchors is not None else {}))

    def _generate_pyloop(self, enc_ids, emask, sample_row, k=0, pre=None, fr=None, stop=None, order=None, allow=None, sched=None, anchors=None):
        """KV-cached decode sequenced from Python with the training kernels (M = 1 GEMMs, flash attention with one query):
        kept as a cross-check of the native pb_decode_step path. k / pre (primed): positions 0 .. k-1 are stepped through with the prefix
        rows as their tokens (their K|V land in the cache one step at a time, independently of _prefill) and sample nothing.
        fr (S, 8): the row's forced table (forced_token); a position with all 8 heads given skips the LM heads.
        stop: the row's stop bar or None (stop_vector). order: the row's bar floor or None (ordered_token; prev is `cur`, the step's input).
        allow: the row's (V,) bool mask or None (allowed_token). sched: the row's schedule (unpack_schedule) or None (scheduled_token).
        anchors: the row's (n, 8) anchors or None (anchored_token)."""
        pb, d, H, X = self.pb, self.d, self.H, self.xdt
        S, dev = enc_ids.shape[1], enc_ids.device
        pad = torch.from_numpy(pb.pad_word_np).to(dev)
        pad_cpu = torch.from_numpy(pb.pad_word_np)
        sv = stop_vector(pad_cpu, stop)
        result = pad.repeat(1, S, 1)
        em, enc16 = self._prompt_inputs(enc_ids, emask)
        e = lambda *shape, dt=X: torch.empty(*shape, dtype=dt, device=dev)
        f = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        with torch.no_grad():
            _, enc_out = self.forward_hidden(enc16, None, em, None, False, 0)
            wf, ff = self.wf, self.fd
            kvc = [e(S, 2 * d) for _ in range(self.ND)]
            for l in range(self.ND):
                self._linear(enc_out, 'dec.%d.wkv_c' % l, 'dec.%d.bkv_c' % l, kvc[l], S, 2 * d, d)
            kvs = [e(S, 2 * d) for _ in range(self.ND)]
            x, q, ctx, a, y1, qc, ctxc, yc, y2 = (e(1, d) for _ in range(9))
            u, g = e(1, ff), e(1, ff)
            mr = f(8)
            logits = f(1, self.lay.vocab)
            save = dict(lse=f(1, H, 1)) if self.use_flash else dict(P=e(1, H, 1, S))
            cur = torch.tensor(pb.sos_word_np, device=dev).reshape(1, 1, 8)
            ak = 0
            for i in range(S):
                tok16 = ops.ids_to_i16(cur)
                ops.embed_ln_fwd(tok16.reshape(1, 8), self.ptab, wf['lin.b'], wf['dec.pos'][i:], wf['dec.lne.w'], wf['dec.lne.b'], x,
                                 mr[0:1], mr[1:2], 1, LN_EPS, 0, 0, 0.0, padded=True, layout=self.lay)
                h = x
                for l in range(self.ND):
                    pf = 'dec.%d.' % l
                    wqkv, bqkv = self.w[pf + 'wqkv'], wf[pf + 'bqkv']
                    ops.gemm(h, wqkv, q, M=1, N=d, K=d, dtype=self.gcode, bias=bqkv[:d])
                    ops.gemm(h, wqkv, kvs[l], M=1, N=2 * d, K=d, dtype=self.gcode, bias=bqkv[d:], b_off=d * d, c_off=i * 2 * d)
                    self._attn_fwd((q, 0, d), (kvs[l], 0, 2 * d), (kvs[l], d, 2 * d), (ctx, 0, d), None, False, 1, 1, i + 1, save)
                    self._linear(ctx, pf + 'wo', pf + 'bo', a, 1, d, d)
                    ops.add_ln_fwd(h, a, wf[pf + 'ln1.w'], wf[pf + 'ln1.b'], y1, mr[2:3], mr[3:4], LN_EPS, 0, 0, 0.0)
                    self._linear(y1, pf + 'wq_c', pf + 'bq_c', qc, 1, d, d)
                    self._attn_fwd((qc, 0, d), (kvc[l], 0, 2 * d), (kvc[l], d, 2 * d), (ctxc, 0, d), em, False, 1, 1, S, save)
                    self._linear(ctxc, pf + 'wo_c', pf + 'bo_c', a, 1, d, d)
                    ops.add_ln_fwd(y1, a, wf[pf + 'lnc.w'], wf[pf + 'lnc.b'], yc, mr[4:5], mr[5:6], LN_EPS, 0, 0, 0.0)
                    self._linear(yc, pf + 'w1', pf + 'b1', g, 1, ff, d, gelu_aux_out=u)
                    self._linear(g, pf + 'w2', pf + 'b2', a, 1, d, ff)
                    out = y2 if h is not y2 else x
                    ops.add_ln_fwd(yc, a, wf[pf + 'ln2.w'], wf[pf + 'ln2.b'], out, mr[6:7], mr[7:8], LN_EPS, 0, 0, 0.0)
                    h = out
                if i < k:                                                  # a forced position: its token is the prefix row, no draw
                    result[:, i, :] = pre[i].to(dev)
                    cur = pre[i].to(dev).reshape(1, 1, 8)
                    continue
                frow = fr[i] if fr is not None else None
                if frow is None or (frow < 0).any():
                    ops.gemm(h, self.w['head.w'], logits, M=1, N=self.lay.vocab, K=d, dtype=self.gcode, bias=wf['head.b'], c_f32=True)
                tok = scheduled_token(frow, lambda **kw: sample_row(logits[0].cpu(), **kw), allow, sched, order,
                                    cur.reshape(8).cpu() if order is not None else None, pad_cpu)
                tok, ak = anchored_token(tok, anchors, ak, sv, pad_cpu)
                if (tok >= sv).any():
                    break
                result[:, i, :] = tok.to(dev)
                cur = tok.to(dev).reshape(1, 1, 8)
        return result

    def _generate_nocache(self, enc_ids, emask, sample_row, k=0, pre=None, fr=None, stop=None, order=None, allow=None, sched=None, anchors=None):
        """The reference's schedule minus the redundant encoder re-runs: full decoder pass per position (kept as the
        cross-check of the cached path). k / pre (primed): decoder inputs 1 .. k and their mask hold the prefix, the loop starts at k.
        fr (S, 8): the row's forced table (forced_token). stop: the row's stop bar or None (stop_vector). order: the row's bar floor or None
        (ordered_token; prev is decoder input i, which the loop wrote at i - 1). allow: the row's (V,) bool mask or None (allowed_token).
        sched: the row's schedule (unpack_schedule) or None (scheduled_token). anchors: the row's (n, 8) anchors or None (anchored_token)."""
        pb = self.pb
        S = enc_ids.shape[1]
        dev = enc_ids.device
        pad = torch.from_numpy(pb.pad_word_np).to(dev)
        dec = pad.repeat(1, S, 1)
        result = pad.repeat(1, S, 1)
        dmask = torch.zeros(1, S, dtype=torch.float32, device=dev)
        dec[:, 0, :] = torch.tensor(pb.sos_word_np, device=dev)
        dmask[:, 0] = 1
        if k:
            n = min(k, S - 1)                                              # k = S: the last prefix row is no decoder input
            dec[0, 1:n + 1] = pre[:n].to(dev)
            dmask[0, :n + 1] = 1
            result[0, :k] = pre.to(dev)
        pad_cpu = torch.from_numpy(pb.pad_word_np)
        sv = stop_vector(pad_cpu, stop)
        em, enc16 = self._prompt_inputs(enc_ids, emask)
        ak = 0
        with torch.no_grad():
            for i in range(k, S):
                dec16 = ops.ids_to_i16(dec)
                dec_h, _ = self.forward_hidden(enc16, dec16, em, dmask, False, 0, reuse_encoder=(i > k))
                logits = self.heads_forward(dec_h)
                cur = scheduled_token(fr[i] if fr is not None else None, lambda **kw: sample_row(logits[i].float().cpu(), **kw), allow, sched, order,
                                    dec[0, i].cpu() if order is not None else None, pad_cpu)
                cur, ak = anchored_token(cur, anchors, ak, sv, pad_cpu)
                if i != S - 1:
                    dec[:, i + 1, :] = cur.to(dev)
                    dmask[:, i + 1] += 1
                if (cur >= sv).any():
                    break
                result[:, i, :] = cur.to(dev)
        return result
