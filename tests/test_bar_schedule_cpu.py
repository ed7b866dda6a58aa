"""Bar schedules ("Bar schedules"), the host half, no GPU: chord_mask / chord_schedule / check_bar_allow on the
default and the 2 470-id dictionary (packing, de-duplication, the AND with the row mask, owner expansion, every refusal by name);
PianoBartLM.sample_row(sched=...) through scheduled_token against an independent restatement with the oracle's sampling() -- head 0, the
mask of its bar, heads 1 .. 7 -- token for token and np.random state for state, given bars and ordered rows included; follows_schedule;
the flags; the header's declarations of the two entry points and their null-argument refusals."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import pianobart_oracle as O
from pianobart_amd import _lib
from pianobart_amd import generation as G
from pianobart_amd import ops
from pianobart_amd._lib import PBError
from pianobart_amd.model import PianoBartLM
from tests.test_allowed_generation_cpu import _e2w, _head, _mask, _row
from tests.test_ordered_generation_cpu import _same_state
from tests.vocab_layout_util import D_WIDE, make_dict

PAD = np.asarray([256, 128, 129, 256, 128, 32, 254, 49])
SOS = PAD + 2
OFF = ops.SEG_OFF
V = ops.VOCAB
TRIADS = {'C:maj': {0, 4, 7}, 'G:maj': {7, 11, 2}, 'A:min': {9, 0, 4}, 'F:maj': {5, 9, 0}}
PROG = ['C:maj', 'G:maj', 'A:min', 'F:maj']


def _pitches(pcs, lo=0, hi=128):
    return {k for k in range(lo, hi) if k % 12 in pcs}


# ---------------------------------------------------------------------------------------------------------------- chord_mask, chord_schedule
def test_chord_mask_on_the_default_dictionary():
    e2w = _e2w()
    for name, pcs in TRIADS.items():
        m = G.chord_mask(e2w, name)
        assert m.shape == (V,) and m.dtype == np.bool_
        assert _head(m, 3) == _pitches(pcs)                            # melodic pitches 0 .. 127 are ids 0 .. 127; percussion (128 ..) removed
        assert all(_head(m, h) == set(range(PAD[h])) for h in (0, 1, 2, 4, 5, 6, 7))
        assert m[OFF[3] + PAD[3]:OFF[4]].all()                          # the special ids
    want = {'maj': {0, 4, 7}, 'min': {0, 3, 7}, 'dim': {0, 3, 6}, 'aug': {0, 4, 8}, '7': {0, 4, 7, 10}, 'maj7': {0, 4, 7, 11}, 'min7': {0, 3, 7, 10},
            'sus2': {0, 2, 7}, 'sus4': {0, 5, 7}}
    for q, iv in want.items():
        assert _head(G.chord_mask(e2w, 'Eb:' + q), 3) == _pitches({(3 + d) % 12 for d in iv}), q
    assert np.array_equal(G.chord_mask(e2w, 'C#:maj'), G.chord_mask(e2w, 'Db:maj'))
    with pytest.raises(PBError, match='root.*C, C#'):
        G.chord_mask(e2w, 'H:maj')
    with pytest.raises(PBError, match='quality.*maj, min, dim'):
        G.chord_mask(e2w, 'C:major')
    with pytest.raises(PBError, match='ROOT:QUALITY'):
        G.chord_mask(e2w, 'Cmaj')


def test_chord_schedule_places_the_chords():
    e2w = _e2w()
    s = G.chord_schedule(e2w, PROG)
    assert len(s) == 256 and all(np.array_equal(s[k], G.chord_mask(e2w, PROG[k % 4])) for k in range(256))
    assert s[0] is s[4]                                                # one mask object per chord
    s = G.chord_schedule(e2w, PROG, bars_per_chord=2, start_bar=3, repeat=False)
    assert s[:3] == [None] * 3 and all(np.array_equal(s[3 + j], G.chord_mask(e2w, PROG[j // 2])) for j in range(8)) and s[11:] == [None] * 245
    s = G.chord_schedule(e2w, 'C:maj', start_bar=250, n_bars=3)
    assert [m is not None for m in s[248:]] == [False, False, True, True, True, False, False, False]
    assert G.chord_schedule(e2w, PROG, start_bar=256) == [None] * 256
    for kw in (dict(bars_per_chord=0), dict(start_bar=-1), dict(n_bars=-2), dict(bars_per_chord=1.5)):
        with pytest.raises(PBError, match=list(kw)[0]):
            G.chord_schedule(e2w, PROG, **kw)
    with pytest.raises(PBError, match='no chord'):
        G.chord_schedule(e2w, [])
    with pytest.raises(PBError, match='quality'):
        G.chord_schedule(e2w, ['C:maj', 'G:dom'])


def test_the_wide_dictionary():
    e2w, _ = make_dict(D_WIDE)                                         # 'Pitch 0' .. 'Pitch 511', 1024 bars, total 2470
    lay = ops.Layout.from_dict(e2w)
    assert lay.vocab == 2470 and lay.pad8[0] == 1024
    m = G.chord_mask(e2w, 'G:maj')
    assert _head(m, 3, lay) == _pitches({7, 11, 2}, 0, 512)
    s = G.chord_schedule(e2w, PROG)
    assert len(s) == 1024
    packed, index, table, sched = G.check_bar_allow([s], None, 1, lay)
    assert packed.shape == (4, 78) and index == [-1] and table.shape == (1, 1024) and sched == [0]       # ceil(2470 / 32)
    assert table.dtype == np.int32 and table[0].tolist() == [k % 4 for k in range(1024)]
    got = G.unpack_schedule((packed, index, table, sched), 2470)[0]
    assert len(got) == 1024 and all(np.array_equal(got[k].numpy(), s[k]) for k in (0, 1, 2, 3, 1023))
    with pytest.raises(PBError, match='at most'):
        G.check_bar_allow([s], None, 1)                                # against the default layout: too many bars
    with pytest.raises(PBError, match='shape'):
        G.check_bar_allow([s[:4]], None, 1)                            # ... and another V
    with pytest.raises(PBError, match='at most'):
        G.check_bar_allow([[None] * 1025], None, 1, lay)


# ---------------------------------------------------------------------------------------------------------------- check_bar_allow
def test_check_bar_allow_packs_dedups_and_intersects():
    e2w = _e2w()
    c, g = G.chord_mask(e2w, 'C:maj'), G.chord_mask(e2w, 'G:maj')
    low = G.allow_mask(e2w, pitch_range=(48, 84))
    assert G.check_bar_allow(None, None, 2) is None and G.check_bar_allow([None, None], [low, None], 2) is None
    assert G.check_bar_allow([{}, [None, None]], None, 2) is None
    assert G.check_bar_allow([{3: np.ones(V, dtype=bool)}], None, 1) is None                      # an all-true entry is no entry
    assert G.check_bar_allow([{3: G.allow_mask(e2w, pitch_range=(40, 90))}], [low], 1) is None     # ... nor one that removes nothing beyond the row mask
    packed, index, table, sched = G.check_bar_allow([{0: c, 1: g, 5: c}, None, [c, g], {0: c, 1: g, 5: torch.from_numpy(c)}], [None, low, low, None], 4)
    bits = G._unpack_bits(packed, V)
    assert packed.dtype == np.uint32 and packed.shape == (5, 40) and index == [-1, 0, 0, -1] and sched == [0, -1, 1, 0]
    assert np.array_equal(bits[0], low)                               # the rows' own masks first: check_allow's table, then the bars'
    assert np.array_equal(bits[1], c) and np.array_equal(bits[2], g) and np.array_equal(bits[3], c & low) and np.array_equal(bits[4], g & low)
    assert table.shape == (2, 256) and table[0, :6].tolist() == [1, 2, -1, -1, -1, 1] and table[1, :3].tolist() == [3, 4, -1]
    assert (table[:, 6:] == -1).all()
    assert _head(bits[3], 3) == _pitches({0, 4, 7}, 48, 84)
    for m in bits:                                                     # the special ids of every head
        assert all(m[OFF[h] + PAD[h]:OFF[h + 1]].all() for h in range(8))
    # head 0's columns of a bar's mask are the row's: the schedule never touches head 0
    nobar = np.ones(V, dtype=bool)
    nobar[OFF[0]:OFF[0] + 200] = False
    assert G.check_bar_allow([{2: nobar}], None, 1) is None
    both = nobar & c
    p2 = G.check_bar_allow([{2: both}], None, 1)
    assert np.array_equal(G._unpack_bits(p2[0], V)[0], c)
    # columns that straddle a word (pitch ids 12, 13, 14 = columns 543, 544, 545), the last bar id
    one = np.ones(V, dtype=bool)
    one[[543, 544, 545]] = False
    p3 = G.check_bar_allow([{255: one}], None, 1)
    assert p3[0][0, 16] == 0x7fffffff and p3[0][0, 17] == 0xfffffffc and p3[2][0, 255] == 0 and (p3[2][0, :255] == -1).all()
    assert (p3[0][0, -1] == 0xffffffff) and p3[0].shape == (1, 40)
    rows = G.unpack_schedule(p3, V)
    assert rows[0][255].dtype == torch.bool and np.array_equal(rows[0][255].numpy(), one) and rows[0][0] is None


def test_check_bar_allow_expands_through_owner():
    e2w = _e2w()
    c, g = G.chord_mask(e2w, 'C:maj'), G.chord_mask(e2w, 'G:maj')
    low = G.allow_mask(e2w, pitch_range=(48, 84))
    packed, index, table, sched = G.check_bar_allow([[c, g], None, [g]], [None, low, None], 3, owner=[0, 0, 1, 2, 2, 2])
    assert index == [-1, -1, 0, -1, -1, -1] and sched == [0, 0, -1, 1, 1, 1] and table.shape == (2, 256) and packed.shape == (3, 40)
    plan = (packed, index, table, sched)
    assert G._slice_schedule(plan, 2, 3) is None and G._slice_schedule(plan, 1, 4)[3] == [0, -1, 1] and G._slice_schedule(plan, 1, 4)[1] == [-1, 0, -1]
    got = G.unpack_schedule(plan, V)
    assert got[2] is None and np.array_equal(got[5][0].numpy(), g) and got[5][1] is None and np.array_equal(got[1][1].numpy(), g)


def test_check_bar_allow_refusals():
    e2w = _e2w()
    c = G.chord_mask(e2w, 'C:maj')
    with pytest.raises(PBError, match='2 entries for 3'):
        G.check_bar_allow([None, None], None, 3)
    with pytest.raises(PBError, match='list of 2 schedules'):
        G.check_bar_allow('C:maj', None, 2)
    with pytest.raises(PBError, match=r'bar_allow\[1\].*bar 256'):
        G.check_bar_allow([None, {256: c}], None, 2)
    with pytest.raises(PBError, match=r'bar_allow\[0\].*bar -1'):
        G.check_bar_allow([{-1: c}], None, 1)
    with pytest.raises(PBError, match=r'bar_allow\[0\].*bar True'):
        G.check_bar_allow([{True: c}], None, 1)
    with pytest.raises(PBError, match='at most'):
        G.check_bar_allow([[None] * 257], None, 1)
    with pytest.raises(PBError, match=r'bar_allow\[0\], bar 4.*bool'):
        G.check_bar_allow([{4: c.astype(np.int64)}], None, 1)
    with pytest.raises(PBError, match=r'bar_allow\[0\], bar 4.*shape'):
        G.check_bar_allow([{4: c[:-1]}], None, 1)
    with pytest.raises(PBError, match='neither None, a dict'):
        G.check_bar_allow([7], None, 1)
    # a pair (row mask, bar mask) that leaves a head without an ordinary class: prompt, bar and head are named
    high = G.allow_mask(e2w, heads={3: [61, 62]})                     # C#, D: no tone of C major's triad
    with pytest.raises(PBError, match=r'bar_allow\[1\].*bar 7 .*head 3 \(Pitch\)'):
        G.check_bar_allow([None, {6: G.chord_mask(e2w, 'D:maj'), 7: c}], [None, high], 2)
    empty = np.ones(V, dtype=bool)
    empty[OFF[5]:OFF[5] + PAD[5]] = False
    with pytest.raises(PBError, match=r'bar_allow\[0\].*bar 0 .*head 5 \(Velocity\)'):
        G.check_bar_allow([[empty]], None, 1)
    with pytest.raises(PBError, match=r'^allow\[0\] leaves head 0'):      # the row mask's own refusals are check_allow's
        G.check_bar_allow([[c]], [np.zeros(V, dtype=bool)], 1)


class _NoDevice:
    """An engine stand-in whose every attribute access fails: the calls must refuse before they touch anything but the layout."""
    BATCH_MAX = 16
    lay = ops.DEFAULT_LAYOUT

    class pb:
        pad_word_np = PAD

    def __getattr__(self, name):
        raise AssertionError('device work before the argument check: %s' % name)


def test_generate_refuses_before_any_device_work():
    x = torch.zeros(2, 8, 8, dtype=torch.long)
    empty = np.ones(V, dtype=bool)
    empty[OFF[3]:OFF[3] + PAD[3]] = False
    for bad in ([None, {300: empty}], [None, [empty]], [None]):
        with pytest.raises(PBError, match='bar_allow'):
            G.GenerationMixin.generate_batch(_NoDevice(), x, None, None, [np.random.RandomState(0), np.random.RandomState(1)], bar_allow=bad)
    with pytest.raises(PBError, match=r'bar_allow\[0\].*bar 2 .*head 3'):
        G.GenerationMixin.generate(_NoDevice(), x[:1], None, None, bar_allow={2: empty})


# ---------------------------------------------------------------------------------------------------------------- the changed line
def _special_set(m):
    m = m.copy()
    for h in range(8):
        m[OFF[h] + PAD[h]:OFF[h + 1]] = True
    return m


def _reference_token(row, own, sched, prev, floor, frow):
    """The contract's steps, restated with the oracle's sampling(): head 0 under the row's own mask (and the bar floor); b0 = its id after
    forcing; heads 1 .. 7 under own AND sched[b0] where b0 is an ordinary bar with an entry, else under own; an ordered row's head 1 loses
    the positions below prev's inside prev's bar. One draw per head in head order; none where all 8 heads are given."""
    if frow is not None and (frow >= 0).all():
        return torch.as_tensor(frow.astype(np.int64))
    own = _special_set(own)
    x = [row[OFF[j]:OFF[j + 1]].clone() for j in range(8)]
    x[0][torch.from_numpy(~own[OFF[0]:OFF[1]])] = -np.inf
    if floor >= 0:
        x[0][:max(floor, int(prev[0]) if prev[0] < PAD[0] else 0)] = -np.inf
    ids = [int(O.sampling(x[0], O.SAMPLE_P[0], O.SAMPLE_T[0]))]
    b0 = int(frow[0]) if frow is not None and frow[0] >= 0 else ids[0]
    m = own
    if b0 < PAD[0] and sched.get(b0) is not None:
        m = _special_set(own & sched[b0])
    for j in range(1, 8):
        x[j][torch.from_numpy(~m[OFF[j]:OFF[j + 1]])] = -np.inf
        if j == 1 and floor >= 0 and prev[0] < PAD[0] and prev[1] < PAD[1] and b0 == prev[0]:
            x[1][:int(prev[1])] = -np.inf
        ids.append(int(O.sampling(x[j], O.SAMPLE_P[j], O.SAMPLE_T[j])))
    tok = torch.tensor(ids)
    if frow is not None:
        given = torch.as_tensor(frow >= 0)
        tok[given] = torch.as_tensor(frow.astype(np.int64))[given]
    return tok


def _bar_masks(rng, n=5):
    """n masks that differ in heads 1 .. 7: a random set of pitch classes (head 3, so that a row mask over a pitch RANGE always leaves a
    class), and random halves of some other heads."""
    out = []
    for _ in range(n):
        m = np.ones(V, dtype=bool)
        pcs = set(rng.choice(12, size=int(rng.randint(1, 5)), replace=False).tolist())
        m[OFF[3]:OFF[3] + PAD[3]] = [k < 128 and k % 12 in pcs for k in range(PAD[3])]
        for h in (1, 2, 4, 5, 6, 7):
            if rng.random_sample() < 0.5:
                keep = rng.random_sample(PAD[h]) > 0.5
                keep[rng.randint(0, PAD[h])] = True
                m[OFF[h]:OFF[h] + PAD[h]] = keep
        out.append(m)
    return out


def _own_mask(rng):
    """A row mask (or None) whose head 3 is a pitch range and whose other heads keep a random part."""
    if rng.random_sample() < 0.3:
        return None
    m = np.ones(V, dtype=bool)
    m[OFF[3]:OFF[3] + PAD[3]] = [36 <= k < 96 for k in range(PAD[3])]
    for h in (0, 2, 5):
        if rng.random_sample() < 0.5:
            keep = rng.random_sample(PAD[h]) > 0.4
            keep[rng.randint(0, PAD[h])] = True
            m[OFF[h]:OFF[h] + PAD[h]] = keep
    return m


def _ours(row, own, sched, prev, floor, frow, rng=None):
    plan = G.check_bar_allow([sched], [own] if own is not None else None, 1)
    ab = G.unpack_allow(plan[:2], V)[0]
    sc = G.unpack_schedule(plan, V)[0]
    return G.scheduled_token(frow, lambda **kw: PianoBartLM.sample_row(PianoBartLM, row.clone(), rng, **kw), ab, sc, floor if floor >= 0 else None, prev, PAD)


def test_sample_row_with_a_schedule_equals_the_restated_reference():
    """300 random logits rows x row masks x schedules, with given bars, given other heads, ordered rows and special predecessors: ids and
    generator state bit for bit, from the global stream and from a generator of its own."""
    rng = np.random.RandomState(31)
    moved = second = given_bar = ordered_same = no_entry = 0
    for n in range(300):
        row, own = _row(rng), _own_mask(rng)
        ms = _bar_masks(rng)
        sched = {k: ms[k % 5] for k in range(256) if k % 7}            # every seventh bar has no entry
        prev = np.asarray([int(rng.randint(0, 250)), int(rng.randint(1, 128))] + [int(rng.randint(0, PAD[h])) for h in range(2, 8)])
        if n % 11 == 0:
            prev = SOS.copy()
        floor = int(rng.choice([-1, -1, 0, int(rng.randint(0, 200))]))
        if n % 3 == 1 and prev[0] < PAD[0]:                            # a peak at prev's bar: an ordered row's head 1 pass follows the schedule's
            row[OFF[0] + prev[0]] = 30.0
            floor = min(floor, int(prev[0]))
            if own is not None:
                own[OFF[0] + prev[0]] = True
        frow = None
        if n % 4 == 0:
            frow = np.full(8, -1, dtype=np.int16)
            frow[0] = int(rng.choice([int(rng.randint(0, 256)), 255, 258]))          # a given bar: ordinary, the last one, special
            if n % 8 == 0:
                frow[3] = 61                                           # a given pitch, inside its bar's mask or not
        elif n % 9 == 0:
            frow = np.full(8, -1, dtype=np.int16)
            frow[int(rng.randint(1, 8))] = 1
        np.random.seed(4000 + n)
        want = _reference_token(row, own if own is not None else np.ones(V, dtype=bool), sched, prev, floor, frow)
        w_state = np.random.get_state()
        np.random.seed(4000 + n)
        got = _ours(row, own, sched, prev, floor, frow)
        assert torch.equal(got, want), (n, got, want)
        assert _same_state(np.random.get_state(), w_state), n
        gen = np.random.RandomState(4000 + n)
        assert torch.equal(_ours(row, own, sched, prev, floor, frow, gen), want) and _same_state(gen.get_state(), w_state), n
        forced = None if frow is None else frow[None]
        assert G.follows_schedule(want[None].numpy(), sched, forced=forced), n
        if own is not None:
            assert G.is_allowed(want[None].numpy(), _special_set(own), forced=forced), n
        np.random.seed(4000 + n)                                       # the same position without the schedule: the same draws
        plain = G.allowed_token(frow, lambda **kw: PianoBartLM.sample_row(PianoBartLM, row.clone(), None, **kw),
                                torch.from_numpy(_special_set(own)) if own is not None else None, floor if floor >= 0 else None, prev, PAD)
        assert _same_state(np.random.get_state(), w_state), n
        assert int(plain[0]) == int(want[0]), n                        # the schedule never touches head 0
        b0 = int(want[0])
        moved += int(not torch.equal(plain, want))
        given_bar += int(frow is not None and frow[0] >= 0)
        no_entry += int(b0 >= 256 or b0 % 7 == 0)
        if b0 >= 256 or b0 % 7 == 0:
            assert torch.equal(plain, want), n                         # a special bar, a bar without an entry: the row's own mask, as today
        if floor >= 0 and b0 == prev[0] and prev[1] < PAD[1] and (frow is None or frow[1] < 0):
            ordered_same += 1
            assert int(want[1]) >= prev[1] or int(want[1]) >= PAD[1], n
    assert moved >= 150 and given_bar >= 70 and no_entry >= 20 and ordered_same >= 30, (moved, given_bar, no_entry, ordered_same)


def test_sample_row_without_a_schedule_is_unchanged():
    rng = np.random.RandomState(32)
    for n in range(50):
        row = _row(rng)
        np.random.seed(n)
        a = PianoBartLM.sample_row(PianoBartLM, row.clone())
        s = np.random.get_state()
        np.random.seed(n)
        b = PianoBartLM.sample_row(PianoBartLM, row.clone(), sched=([None] * 256, -1))
        assert torch.equal(a, b) and _same_state(np.random.get_state(), s)
        np.random.seed(n)
        c = PianoBartLM.sample_row(PianoBartLM, row.clone(), sched=([torch.ones(V, dtype=torch.bool)] * 256, -1))     # a mask that removes nothing
        assert torch.equal(a, c) and _same_state(np.random.get_state(), s)


def test_scheduled_token_passes_the_keywords():
    mask, bar = _mask(h2=[0]), torch.from_numpy(_mask(h3=[60, 62, 64]))
    sched = [None] * 256
    sched[4] = bar
    tok = torch.tensor([4, 2, 0, 60, 5, 6, 7, 8])
    seen = {}
    sample = lambda **kw: seen.update(kw) or tok
    assert torch.equal(G.scheduled_token(None, sample, mask, sched, None, SOS, PAD), tok)
    assert set(seen) == {'allow', 'sched'} and seen['allow'] is mask and seen['sched'][0] is sched and seen['sched'][1] == -1
    seen.clear()
    frow = np.asarray([9, -1, -1, 61, -1, -1, -1, -1], dtype=np.int16)
    got = G.scheduled_token(frow, sample, None, sched, 3, np.asarray([9, 5] + [0] * 6), PAD)
    assert got.tolist() == [9, 2, 0, 61, 5, 6, 7, 8] and set(seen) == {'sched', 'order'} and seen['sched'][1] == 9 and seen['order'] == (9, 9, 5, 9)
    seen.clear()
    assert torch.equal(G.scheduled_token(None, sample, mask, None, None, SOS, PAD), tok) and set(seen) == {'allow'}     # no schedule: allowed_token
    assert torch.equal(G.scheduled_token(None, lambda: tok, None, None, None, SOS, PAD), tok)

    def never(**kw):
        raise AssertionError('a fully given position samples nothing')
    full = np.arange(8, dtype=np.int16)
    assert G.scheduled_token(full, never, mask, sched, 0, SOS, PAD).tolist() == full.tolist()


def test_follows_schedule_on_hand_written_rows():
    e2w = _e2w()
    s = G.chord_schedule(e2w, ['C:maj', 'G:maj'], n_bars=2)            # bar 0: C E G, bar 1: G B D, bar 2 ..: free
    rows = np.ones((6, 8), dtype=np.int64)
    rows[:, 0] = [0, 0, 1, 1, 2, 2]
    rows[:, 3] = [60, 64, 62, 67, 61, 130]
    rows = np.concatenate([rows, (PAD + 3)[None], PAD[None]])
    assert G.follows_schedule(rows, s) and G.follows_schedule(torch.as_tensor(rows), {0: s[0], 1: s[1]})
    bad = rows.copy()
    bad[2, 3] = 60                                                     # a C in the G bar
    assert not G.follows_schedule(bad, s) and not G.follows_schedule(bad, s, start=2) and G.follows_schedule(bad, s, start=3)
    forced = np.full(bad.shape, -1, dtype=np.int64)
    forced[2, 3] = 60
    assert G.follows_schedule(bad, s, forced=forced)                   # a given head is not tested
    behind = rows.copy()
    behind[7, 0], behind[7, 3] = 0, 61                                  # behind the first special bar: not emitted
    assert G.follows_schedule(behind, s)
    spec = rows.copy()
    spec[1, 3] = 258                                                   # a special id counts as allowed
    assert G.follows_schedule(spec, s)
    drum = rows.copy()
    drum[0, 3] = 130                                                   # percussion in a chord's bar
    assert not G.follows_schedule(drum, s)


# ---------------------------------------------------------------------------------------------------------------- flags, header, binding
def test_cli_flag_rules():
    from pianobart_amd import demo as D
    from pianobart_amd import eval_generation as EG
    e2w = _e2w()
    base = ['--nopretrain', '--seed', '0']
    a = EG.get_args(base)
    assert a.chords is None and a.bars_per_chord == 1 and a.chord_start is None and G.schedule_from_args(a, e2w) is None
    assert G.ALLOW_FLAGS == ('key', 'pitch_range', 'instruments', 'tempo', 'max_duration', 'velocity')
    a = EG.get_args(base + ['--chords', 'C:maj,G:maj,A:min,F:maj'])
    s = G.schedule_from_args(a, e2w)
    assert all(np.array_equal(s[k], G.chord_mask(e2w, PROG[k % 4])) for k in range(256))
    prime = np.zeros((5, 8), dtype=np.int64)
    prime[:, 0] = [0, 0, 1, 2, 2]
    s = G.schedule_from_args(a, e2w, prime)                            # the bar after the one the prime ends in
    assert s[:3] == [None] * 3 and np.array_equal(s[3], G.chord_mask(e2w, 'C:maj')) and np.array_equal(s[4], G.chord_mask(e2w, 'G:maj'))
    a = EG.get_args(base + ['--chords', 'C:maj,G:maj', '--bars_per_chord', '2', '--chord_start', '1'])
    s = G.schedule_from_args(a, e2w, prime)
    assert s[0] is None and [np.array_equal(s[k], G.chord_mask(e2w, 'C:maj')) for k in (1, 2, 3, 4, 5)] == [True, True, False, False, True]
    d = D.get_args(['--chords', 'C:maj,G:maj', '--bars_per_chord', '2', '--chord_start', '1'])
    assert all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(G.schedule_from_args(d, e2w), s))
    assert D.Args().chords is None and D.Args(chords='C:maj').chords == 'C:maj'
    for extra in (['--chords', 'C:maj'], ['--chords', 'C:maj,G:maj', '--prime', 'half', '--key', 'C:major'], ['--chords', 'A:min', '--samples', '3'],
                  ['--chords', 'A:min', '--refill', '--ordered']):
        a = EG.get_args(base + extra)
        a.cpu = False
        EG.check_args(a)
    with pytest.raises(PBError, match='--chords'):
        EG.check_args(EG.get_args(base + ['--chords', 'C:maj', '--prime', '4', '--score_dataset']))
    with pytest.raises(PBError, match='need --chords'):
        G.schedule_from_args(EG.get_args(base + ['--chord_start', '2']), e2w)
    with pytest.raises(PBError, match='quality'):
        G.schedule_from_args(EG.get_args(base + ['--chords', 'C:maj,G:x']), e2w)


def test_header_and_binding_know_the_entry_points():
    decls = _lib.parse_header()
    assert decls['pb_batch_decoder_schedule'] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p])
    assert decls['pb_batch_decoder_admit_schedule'] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32])
    dll = _lib.LIB.load()
    assert dll.pb_abi_version() == 10                                  # additions only
    for name in ('pb_batch_decoder_schedule', 'pb_batch_decoder_admit_schedule'):
        assert getattr(dll, name).argtypes == decls[name][1]
    assert dll.pb_batch_decoder_admit_schedule(None, 0, 0) < 0 and b'pb_batch_decoder_admit_schedule' in dll.pb_last_error()
    assert dll.pb_batch_decoder_schedule(None, None, 1, 256, None) < 0 and b'pb_batch_decoder_schedule: null argument' in dll.pb_last_error()
