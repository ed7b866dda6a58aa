"""On-device Octuple augmentation: every piece of a training batch is transposed, and its dynamics and tempo nudged, AS A
WHOLE -- one shift per attribute, clamped by the piece's own extremes so that no note is clipped or wrapped. Percussion pitches and the
special rows are never touched. The work is one kernel (pb_augment) in front of the corruption; this module builds its tables from a
dictionary's NAMES on the host, before any device work, and keeps the seeds of the trainers' batches.

  plan = AugmentPlan(e2w, pitch=(-6, 5), velocity=(-2, 2), tempo=(-2, 2), pitch_bounds=(21, 108), prob=1.0)
  out16, shifts = apply(ids16, plan, batch_seed(seed, rank, epoch, index))          # shifts (B, 3) int32: pitch, velocity, tempo
"""
import ctypes
import json
import re

import numpy as np
import torch

from . import ops
from ._lib import PBError

AXES = ('pitch', 'velocity', 'tempo')
AXIS_HEAD = (3, 5, 7)                         # the head of every axis (ops.CLASS_NAMES)
ALWAYS = 0xFFFFFFFF                           # the apply threshold of prob = 1
_M64 = 0xFFFFFFFFFFFFFFFF


def _default_e2w():
    from .pieces import VOCAB
    return json.load(open(VOCAB))['e2w']


def _int_pair(what, v):
    try:
        lo, hi = v
    except (TypeError, ValueError):
        raise PBError('augment: %s must be a pair (lo, hi) of integers (got %r)' % (what, v))
    for x in (lo, hi):
        if isinstance(x, bool) or not isinstance(x, (int, np.integer)):
            raise PBError('augment: %s: the ends must be integers (got %r)' % (what, v))
    return int(lo), int(hi)


class AugmentPlan:
    """The tables and the request of pb_augment for one dictionary. e2w_or_layout: the dictionary's event -> word half ({class: {word: id}},
    PianoBart.e2w); None, or an ops.Layout equal to ops.DEFAULT_LAYOUT, means the default dictionary (data/octuple_vocab.json); any other
    bare Layout is refused, since a layout has no names. pitch / velocity / tempo: the inclusive request (lo, hi) with lo <= 0 <= hi, or
    None = the axis is off. Coordinates come from the names, as generation.allow_mask reads them:
      pitch     'Pitch k' has the coordinate k - (the smallest k), and the k must be a contiguous integer range; 'Pitch percussion k' (and any
                other word) is never touched. pitch_bounds=(lo, hi), in semitone numbers: a piece is shifted only inside lo .. hi, and a
                piece with a note outside stays as it is. Default: the dictionary's whole range.
      velocity  'Velocity v' / 'Tempo t' have the RANK of their number among the head's numbered words: a shift of 1 is the next bin.
      tempo
    prob in (0, 1]: every axis of every piece is shifted with this probability (else its shift is 0).
    PBError, before any device work, names the axis and the rule that is broken."""

    def __init__(self, e2w_or_layout=None, pitch=None, velocity=None, tempo=None, pitch_bounds=None, prob=1.0):
        if e2w_or_layout is None or (isinstance(e2w_or_layout, ops.Layout) and e2w_or_layout == ops.DEFAULT_LAYOUT):
            e2w = _default_e2w()
        elif isinstance(e2w_or_layout, ops.Layout):
            raise PBError('augment: the axes are read from the dictionary\'s names: pass e2w (PianoBart.e2w), not a Layout (%r)' % (e2w_or_layout,))
        else:
            e2w = e2w_or_layout
        self.layout = lay = ops.Layout.from_dict(e2w)
        if isinstance(prob, bool) or not isinstance(prob, (int, float, np.integer, np.floating)) or not 0.0 < float(prob) <= 1.0:
            raise PBError('augment: prob must lie in (0, 1] (got %r)' % (prob,))
        self.prob = float(prob)
        self.request = {}
        for name, v in zip(AXES, (pitch, velocity, tempo)):
            if v is None:
                continue
            lo, hi = _int_pair(name, v)
            if lo > 0 or hi < 0:
                raise PBError('augment: %s: the request %d .. %d must hold lo <= 0 <= hi' % (name, lo, hi))
            self.request[name] = (lo, hi)
        if pitch_bounds is not None and pitch is None:
            raise PBError('augment: pitch: pitch_bounds without a pitch request')
        thresh = ALWAYS if self.prob == 1.0 else min(int(self.prob * 4294967296.0), ALWAYS)
        self.coord = np.full((3, ops.HEAD_MAX), -1, dtype=np.int16)
        self.id_at = np.zeros((3, ops.HEAD_MAX), dtype=np.int16)
        self.plan = np.zeros((3, 6), dtype=np.int64)                   # lo, hi, blo, bhi, ncoord, thresh
        self.pitch_base = 0                                            # the semitone number of pitch coordinate 0
        for a, name in enumerate(AXES):
            self.plan[a] = (0, 0, 0, 0, 1, ALWAYS)                     # an axis that is off: no id has a coordinate
            if name not in self.request:
                continue
            h, cls = AXIS_HEAD[a], ops.CLASS_NAMES[AXIS_HEAD[a]]
            numbered = []                                              # (number, id) of the head's ordinary numbered words
            for w, i in e2w[cls].items():
                m = re.fullmatch(r'%s (\d+(?:\.\d+)?(?:[eE][-+]?\d+)?)' % cls if a else r'Pitch (\d+)', w)
                if m and int(i) < lay.pad8[h]:
                    numbered.append((float(m.group(1)) if a else int(m.group(1)), int(i), w))
            if not numbered:
                raise PBError('augment: %s: head %d (%s) has no numbered word (\'%s <number>\')' % (name, h, cls, cls))
            numbered.sort()
            values = [v for v, _, _ in numbered]
            for (v0, _, w0), (v1, _, w1) in zip(numbered, numbered[1:]):
                if v0 == v1:
                    raise PBError('augment: %s: the words %r and %r carry the same number: the coordinates must be distinct' % (name, w0, w1))
                if a == 0 and v1 != v0 + 1:
                    raise PBError('augment: pitch: gap in the coordinates between %r and %r: the pitches must be a contiguous integer range' % (w0, w1))
            n = len(numbered)
            blo, bhi = 0, n - 1
            if a == 0:
                self.pitch_base = values[0]
                if pitch_bounds is not None:
                    plo, phi = _int_pair('pitch_bounds', pitch_bounds)
                    if plo > phi or plo < values[0] or phi > values[-1]:
                        raise PBError('augment: pitch: the bounds %d .. %d lie outside the axis %d .. %d' % (plo, phi, values[0], values[-1]))
                    blo, bhi = plo - self.pitch_base, phi - self.pitch_base
            for c, (_, i, _) in enumerate(numbered):
                self.coord[a, i] = c
                self.id_at[a, c] = i
            lo, hi = self.request[name]
            self.plan[a] = (max(lo, -ops.HEAD_MAX), min(hi, ops.HEAD_MAX), blo, bhi, n, thresh)
        self.pitch_bounds = (int(self.plan[0][2]) + self.pitch_base, int(self.plan[0][3]) + self.pitch_base) if 'pitch' in self.request else None
        self._plan18 = (ctypes.c_int32 * 18)(*[int(v) - (1 << 32) if int(v) >= (1 << 31) else int(v) for v in self.plan.reshape(-1)])
        self._dev = {}

    def axes(self):
        """The names of the axes that are on."""
        return tuple(n for n in AXES if n in self.request)

    def tables(self, device):
        """(coord, id_at) as (3, HEAD_MAX) int16 tensors on `device`: uploaded once per device."""
        key = str(device)
        if key not in self._dev:
            self._dev[key] = (torch.from_numpy(self.coord).to(device), torch.from_numpy(self.id_at).to(device))
        return self._dev[key]

    @property
    def spec(self):
        """The command-line form of the request (parse's inverse; prob travels in --augment_prob)."""
        parts = ['%s=%d:%d' % (n, *self.request[n]) for n in AXES if n in self.request]
        if self.pitch_bounds is not None:
            parts.append('bounds=%d:%d' % self.pitch_bounds)
        return ','.join(parts)

    def __repr__(self):
        return 'AugmentPlan(%s, prob=%g)' % (self.spec, self.prob)


def parse(spec):
    """The keyword arguments of AugmentPlan from the command-line form `pitch=-6:5,velocity=-2:2,tempo=-2:2[,bounds=21:108]`: every item
    is NAME=LO:HI with integer ends, each name at most once, `bounds` = pitch_bounds."""
    kw = {}
    items = [s.strip() for s in str(spec).split(',')]
    if not any(items):
        raise PBError('augment: empty specification (expected e.g. pitch=-6:5,velocity=-2:2,tempo=-2:2)')
    for item in items:
        m = re.fullmatch(r'(\w+)\s*=\s*([-+]?\d+)\s*:\s*([-+]?\d+)', item)
        if not m:
            raise PBError('augment: %r is not NAME=LO:HI with integer ends' % item)
        name = 'pitch_bounds' if m.group(1) == 'bounds' else m.group(1)
        if name not in AXES + ('pitch_bounds',):
            raise PBError('augment: unknown axis %r (%s, bounds)' % (m.group(1), ', '.join(AXES)))
        if name in kw:
            raise PBError('augment: %s is given twice' % m.group(1))
        kw[name] = (int(m.group(2)), int(m.group(3)))
    return kw


def format_spec(pitch=None, velocity=None, tempo=None, pitch_bounds=None):
    """parse's inverse on its own output."""
    parts = ['%s=%d:%d' % (n, *v) for n, v in zip(AXES + ('bounds',), (pitch, velocity, tempo, pitch_bounds)) if v is not None]
    return ','.join(parts)


def _splitmix64(x):
    z = (x + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def batch_seed(seed, rank, epoch, index):
    """The 64-bit seed of one training batch: splitmix64 folded over (seed, rank, epoch, index), h = mix(seed), then h = mix(h ^ x) for
    x = rank, epoch, index. A function of these four numbers and of nothing else: ranks draw different shifts, and a resumed run draws at
    epoch e what the uninterrupted run drew there. mix is a bijection, so changing any one argument changes the result."""
    h = _splitmix64(int(seed) & _M64)
    for x in (rank, epoch, index):
        h = _splitmix64(h ^ (int(x) & _M64))
    return h


def apply(ids16, plan, seed, out=None):
    """ids16 (B, S, 8) int16 on the device -> (out16, shifts): the augmented pieces (out=None: a new tensor; out=ids16: in place) and the
    (B, 3) int32 shifts (pitch, velocity, tempo) that were applied."""
    if not isinstance(plan, AugmentPlan):
        raise PBError('augment.apply: plan must be an AugmentPlan (got %s)' % type(plan).__name__)
    ops._p(ids16)
    if ids16.dtype != torch.int16 or ids16.dim() != 3 or ids16.shape[2] != 8 or not ids16.is_contiguous():
        raise PBError('augment.apply: ids must be a contiguous (B, S, 8) int16 tensor (got %s %s)' % (tuple(ids16.shape), ids16.dtype))
    if out is None:
        out = torch.empty_like(ids16)
    elif out.dtype != torch.int16 or out.shape != ids16.shape or not out.is_contiguous() or out.device != ids16.device:
        raise PBError('augment.apply: out must match ids (contiguous %s int16 on %s)' % (tuple(ids16.shape), ids16.device))
    shifts = torch.empty(ids16.shape[0], 3, dtype=torch.int32, device=ids16.device)
    coord, id_at = plan.tables(ids16.device)
    ops.augment(ids16, out, shifts, coord, id_at, plan._plan18, int(seed) & _M64)
    return out, shifts


# ---- the trainers' side --------------------------------------------------------------------------------------------------------------

def add_arguments(parser):
    """--augment / --augment_prob / --augment_seed of the three drivers (off unless --augment is given)."""
    parser.add_argument('--augment', type=str, default=None, metavar='SPEC',
                        help='whole-piece augmentation of the training batches on the device, e.g. pitch=-6:5,velocity=-2:2,tempo=-2:2[,bounds=21:108] '
                             '(not in the reference; off by default)')
    parser.add_argument('--augment_prob', type=float, default=1.0, help='probability that an axis of a piece is shifted')
    parser.add_argument('--augment_seed', type=int, default=0, help='seed of the augmentation stream (with the rank, the epoch and the batch index)')


def check_task(plan, task):
    """The fine-tune tasks and the axes: composer, emotion and melody take all three (melody's labels are per position and do not move);
    velocity refuses the velocity axis, because its label IS the velocity."""
    if plan is not None and task == 'velocity' and 'velocity' in plan.request:
        raise PBError('augment: velocity: the velocity task predicts the velocity: its labels would no longer match the shifted input (drop the velocity axis)')
    return plan


def from_args(args, e2w, task=None):
    """The AugmentPlan of a driver's arguments, or None when --augment is not given."""
    if not getattr(args, 'augment', None):
        return None
    return check_task(AugmentPlan(e2w, prob=args.augment_prob, **parse(args.augment)), task)
