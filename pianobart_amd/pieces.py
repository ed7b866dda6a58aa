"""The host front end of the evaluation families (metrics, novelty, structure, harmony, texture): what they all do with a set of pieces before a
kernel sees it. The tables of a dictionary, the checks of an (N, S, 8) id array and of `start`, the upload, the host
statement of which rows of a piece are its notes, and the stage timer. csrc/pb_pieces.h is the device half of the same rules."""
import json
import os
import re
from collections import OrderedDict, namedtuple

import numpy as np
import torch

from . import ops
from ._lib import PBError
from .octuple_midi import code_to_dur

VOCAB = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'data', 'octuple_vocab.json')
MAX_PITCH = ops.HEAD_MAX - 1                  # the kernel's pitch bitmap covers 0 .. HEAD_MAX - 1
MAX_BAR_POS = 1024                            # the positions of a bar at most: a position id is a 10-bit field of the bar keys

Tables = namedtuple('Tables', 'pitch_of dur_pos layout bar_pos')


def _words_by_id(e2w, name, n):
    """The words of ids 0 .. n - 1 of a class; PBError when an id has no word."""
    by_id = {int(i): w for w, i in e2w[name].items()}
    missing = [i for i in range(n) if i not in by_id]
    if missing:
        raise PBError('pieces: class %s has no word for id %d' % (name, missing[0]))
    return [by_id[i] for i in range(n)]


def tables(e2w=None):
    """Tables(pitch_of, dur_pos, layout, bar_pos) of a dictionary's event -> word half (None: the default dictionary; a Tables is returned
    as it is): pitch_of[id] = k for the word 'Pitch k' and -1 for 'Pitch percussion k' (int16, one entry per ordinary pitch id); dur_pos[id] =
    octuple_midi.code_to_dur(c) for the word 'Duration c' (int32, one entry per ordinary duration id). A pitch or duration word of another
    form is a PBError that names it. bar_pos[id] = n * 64 // d, the positions of a bar (octuple_midi.bar_length: 16 per beat), for the
    word 'TimeSig n/d' (int32, one entry per ordinary time-signature id), and 0 for a word of another form or a length outside 1 .. 1024:
    only the texture family needs bar lengths, and it refuses a table that holds a 0."""
    if isinstance(e2w, Tables):
        return e2w
    if e2w is None:
        e2w = json.load(open(VOCAB))['e2w']
    layout = ops.Layout.from_dict(e2w)
    pitch_of = np.empty(layout.pad8[3], dtype=np.int16)
    for i, w in enumerate(_words_by_id(e2w, 'Pitch', layout.pad8[3])):
        m = re.fullmatch(r'Pitch (percussion )?(\d+)', w)
        if not m:
            raise PBError("pieces: pitch word %r (id %d) is neither 'Pitch k' nor 'Pitch percussion k'" % (w, i))
        k = -1 if m.group(1) else int(m.group(2))
        if k > MAX_PITCH:
            raise PBError('pieces: pitch word %r (id %d): the pitch number must lie in 0 .. %d' % (w, i, MAX_PITCH))
        pitch_of[i] = k
    dur_pos = np.empty(layout.pad8[4], dtype=np.int32)
    for i, w in enumerate(_words_by_id(e2w, 'Duration', layout.pad8[4])):
        m = re.fullmatch(r'Duration (\d+)', w)
        if not m:
            raise PBError("pieces: duration word %r (id %d) is not 'Duration c'" % (w, i))
        dur_pos[i] = code_to_dur(int(m.group(1)))
    bar_pos = np.zeros(layout.pad8[6], dtype=np.int32)
    for i, w in enumerate(_words_by_id(e2w, 'TimeSig', layout.pad8[6])):
        m = re.fullmatch(r'TimeSig (\d+)/(\d+)', w)
        if m and int(m.group(2)) > 0 and 1 <= int(m.group(1)) * 64 // int(m.group(2)) <= MAX_BAR_POS:
            bar_pos[i] = int(m.group(1)) * 64 // int(m.group(2))
    return Tables(pitch_of, dur_pos, layout, bar_pos)


def host_ids(ids, layout):
    """ids as a host int64 (N, S, 8) array, every id checked against its head's size."""
    if torch.is_tensor(ids):
        ops._p(ids)                                   # a host tensor is refused as every op refuses it: there is no CPU path
        ids = ids.detach().cpu().numpy()
    a = np.asarray(ids)
    if a.ndim != 3 or a.shape[2] != 8 or a.shape[1] < 1:
        raise PBError('pieces: ids must be (N, S, 8) with S >= 1 (got %s)' % (a.shape,))
    if a.dtype.kind == 'f':
        r = np.rint(a)
        if not np.array_equal(r, a):                  # NaN included
            raise PBError('pieces: ids hold values that are not integers')
        a = r
    elif a.dtype.kind not in 'iu':
        raise PBError('pieces: ids must be integers or integer-valued floats (got %s)' % a.dtype)
    a = a.astype(np.int64)
    for h, n in enumerate(layout.sizes):
        col = a[:, :, h]
        if col.size and (col.min() < 0 or col.max() >= n):
            bad = col[(col < 0) | (col >= n)][0]
            raise PBError('pieces: head %d (%s) holds the id %d; its ids are 0 .. %d' % (h, ops.CLASS_NAMES[h], int(bad), n - 1))
    return a


def host_start(start, N):
    """start as a host int32 (N) array: one row index >= 0 for every piece, or one per piece."""
    if start is None:
        return None
    s = np.asarray(start.detach().cpu().numpy() if torch.is_tensor(start) else start)
    if s.ndim > 1 or (s.ndim == 1 and s.shape[0] != N) or s.dtype.kind not in 'iu' or (s.size and s.min() < 0):
        raise PBError('pieces: start must be one row index >= 0, or one per piece (%d)' % N)
    return np.array(np.broadcast_to(s, (N,)), dtype=np.int32)


def upload(ids, tab, start, device, max_S=None, **arrays):
    """The checked arguments every ops.piece_* wrapper takes, on the device, as its keywords: ids16, pitch_of, start, layout, and each of
    `arrays` (host arrays a wrapper takes besides, e.g. dur_pos). max_S: longer pieces are refused here, before anything is copied."""
    a = host_ids(ids, tab.layout)
    if max_S is not None and a.shape[1] > max_S:
        raise PBError('pieces: pieces of %d rows; the kernels take 1 .. %d' % (a.shape[1], max_S))
    dev = torch.device(device) if device is not None else ids.device if torch.is_tensor(ids) else torch.device('cuda', torch.cuda.current_device())
    s = host_start(start, a.shape[0])
    up = lambda x: torch.from_numpy(x).to(dev)
    return dict(ids16=up(a.astype(np.int16)), pitch_of=up(tab.pitch_of), start=None if s is None else up(s), layout=tab.layout,
                **{k: up(v) for k, v in arrays.items()})


def live_rows(ids, layout=None, start=None):
    """Host: (L, live) of an (N, S, 8) integer array. L (N): a piece's first row in which any head's id is >= its PAD id (the generator's
    stop rule; S if none). live (N, S) bool: the piece's notes, the rows start .. L - 1 (start: one row index or one per piece, None = 0)."""
    layout = layout or ops.DEFAULT_LAYOUT
    a = np.asarray(ids)
    special = (a >= np.asarray(layout.pad8)).any(-1)
    L = np.where(special.any(1), special.argmax(1), a.shape[1])
    s = np.zeros(a.shape[0], dtype=np.int32) if start is None else host_start(start, a.shape[0])
    r = np.arange(a.shape[1])
    return L, (r >= s[:, None]) & (r < L[:, None])


def bar_spans(ids, layout=None, start=None):
    """Host: W of every piece of an (N, S, 8) integer array, the largest minus the smallest bar id of its notes plus one (0 without a note)."""
    live = live_rows(ids, layout, start)[1]
    bars = np.asarray(ids)[:, :, 0].astype(np.int64)
    hi, lo = np.where(live, bars, -1).max(1), np.where(live, bars, 1 << 40).min(1)
    return np.where(live.any(1), hi - lo + 1, 0)


class Timer:
    """Device milliseconds per stage from pairs of events on the current stream, read after one synchronisation at the end."""

    def __init__(self, stages):
        self.pairs = []
        self.stages = tuple(stages)                   # the stages of totals(), in its order

    def run(self, stage, fn, *args, **kw):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn(*args, **kw)
        b.record()
        self.pairs.append((stage, a, b))
        return out

    def totals(self):
        torch.cuda.synchronize()
        ms = OrderedDict((stage, 0.0) for stage in self.stages)
        for stage, a, b in self.pairs:
            ms[stage] += a.elapsed_time(b)
        ms['total'] = sum(ms.values())
        return ms
