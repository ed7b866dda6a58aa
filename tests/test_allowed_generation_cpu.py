"""CPU: allowed-class generation (Engine.generate / generate_batch(allow=...)) -- the argument rules (generation.check_allow), the mask
builder (allow_mask) on the default and on one other dictionary, the changed line (allowed_token + PianoBartLM.sample_row's `allow`)
against the oracle's sampling() fed the masked logits, the property check (is_allowed), the flag rules and the two new entry points in
the header and the binding. No device work.

Contract ("Allowed classes"): the reference loop with sampling(logit, p, t) seeing -inf in place of every logit
whose bit is 0. The restatement is oracle.pianobart_oracle.sampling (the numpy nucleus rule behind a torch softmax), which divides by the
temperature itself: -inf / t = -inf, so masking the logit masks the quotient."""
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
from tests.test_ordered_generation_cpu import _reference_token, _same_state
from tests.vocab_layout_util import D_SMALL, make_dict

PAD = np.asarray([256, 128, 129, 256, 128, 32, 254, 49])
SOS = PAD + 2
EOS = PAD + 3
OFF = ops.SEG_OFF
V = ops.VOCAB
C_MAJOR = {0, 2, 4, 5, 7, 9, 11}


def _e2w():
    from pianobart_amd.eval_generation import _VOCAB
    from pianobart_amd.pretrain import _load_vocab
    return _load_vocab(_VOCAB)[0]


def _head(mask, h, lay=ops.DEFAULT_LAYOUT):
    """The ordinary ids head h admits."""
    return set(np.flatnonzero(np.asarray(mask)[lay.seg_off[h]:lay.seg_off[h] + lay.pad8[h]]).tolist())


def _mask(**heads):
    """A mask from raw ids per head: _mask(h3=[60, 62])."""
    return G.allow_mask(None, heads={int(k[1:]): v for k, v in heads.items()})


# ---------------------------------------------------------------------------------------------------------------- check_allow
def test_check_allow_accepts_and_normalises():
    m1, m2 = _mask(h3=[60, 62, 64]), _mask(h2=[0], h7=range(16, 33))
    assert G.check_allow(None, 3) is None
    assert G.check_allow(np.ones(V, dtype=bool), 1) is None            # all true: the caller runs what it ran before
    assert G.check_allow(np.ones((3, V), dtype=bool), 3) is None and G.check_allow([None, None], 2) is None
    assert G.check_allow(torch.ones(2, V, dtype=torch.bool), 2) is None
    packed, index = G.check_allow(m1, 1)                               # one prompt: (V,)
    assert packed.shape == (1, (V + 31) // 32) == (1, 40) and packed.dtype == np.uint32 and index == [0]
    for form in (m1[None], [m1], torch.from_numpy(m1)[None], [torch.from_numpy(m1)], (m1,)):
        p2, i2 = G.check_allow(form, 1)
        assert np.array_equal(p2, packed) and i2 == [0]
    packed, index = G.check_allow([m1, None, m2, m1.copy(), np.ones(V, dtype=bool), m2], 6)
    assert packed.shape == (2, 40) and index == [0, -1, 1, 0, -1, 1]   # equal masks share an entry; all-true rows are free rows
    assert all(type(i) is int for i in index)
    packed2, index2 = G.check_allow(np.stack([m1, m2]), 2)
    assert np.array_equal(packed2, packed) and index2 == [0, 1]
    back = G.unpack_allow((packed, index), V)
    assert back[1] is None and back[4] is None and back[0].dtype == torch.bool
    assert np.array_equal(back[0].numpy(), m1) and np.array_equal(back[2].numpy(), m2) and np.array_equal(back[3].numpy(), m1)


def test_check_allow_sets_the_special_bits():
    m = np.zeros(V, dtype=bool)
    for h in range(8):
        m[OFF[h] + 1] = True                                           # one ordinary class per head, no special id
    packed, index = G.check_allow(m, 1)
    got = G.unpack_allow((packed, index), V)[0].numpy()
    for h in range(8):
        assert _head(got, h) == {1}
        assert got[OFF[h] + PAD[h]:OFF[h + 1]].all(), h                # PAD, MASK, SOS, EOS, CLS, SEP: a row can still end
    assert not m[OFF[0] + PAD[0]]                                      # the caller's array is not written


def test_check_allow_packs_a_column_that_straddles_a_word():
    """Column 262 is head 1's first: bit 6 of word 8. Head offsets are no multiples of 32, so the packing is by column."""
    assert OFF[1] == 262
    for col in (262, 263, 0, 31, 32, 255, 287, 288, V - 7):
        m = np.ones(V, dtype=bool)
        m[col] = False
        packed, _ = G.check_allow(m, 1)
        want = np.full(40, 0xffffffff, dtype=np.uint64)
        want[col >> 5] &= ~np.uint64(1 << (col & 31))
        assert np.array_equal(packed[0].astype(np.uint64), want), col
    only = np.zeros(V, dtype=bool)
    for h in range(8):
        only[OFF[h]] = True
    packed, _ = G.check_allow(only, 1)
    assert (int(packed[0, 262 >> 5]) >> (262 & 31)) & 1 == 1 and (int(packed[0, 263 >> 5]) >> (263 & 31)) & 1 == 0
    assert int(packed[0, 39]) >> 31 == 1                               # column 1279 (the last special id) is the table's last bit: no bit beyond V


def test_check_allow_refusals():
    m = _mask(h3=[60])
    for bad, P in ((np.ones((2, V), dtype=bool), 3), ([m, m], 3), ([], 1), (m, 2), (np.ones((1, 1, V), dtype=bool), 1)):
        with pytest.raises(PBError, match='allow'):
            G.check_allow(bad, P)
    for bad in (np.ones(V, dtype=np.int64), np.ones(V, dtype=np.float32), torch.ones(V), np.ones(V, dtype=np.uint8)):
        with pytest.raises(PBError, match='bool'):
            G.check_allow(bad, 1)
        with pytest.raises(PBError, match='bool'):
            G.check_allow([None, bad], 2)
    for bad in (np.ones(V - 1, dtype=bool), np.ones(V + 1, dtype=bool), np.ones((2, 2), dtype=bool)):
        with pytest.raises(PBError, match='shape'):
            G.check_allow([bad], 1)
    for h, name in enumerate(ops.CLASS_NAMES):
        bad = np.ones(V, dtype=bool)
        bad[OFF[h]:OFF[h] + PAD[h]] = False                            # only its special ids are left
        with pytest.raises(PBError, match=r'head %d \(%s\)' % (h, name)):
            G.check_allow(bad, 1)


def test_check_allow_expands_through_owner():
    m1, m2 = _mask(h3=[60]), _mask(h3=[61])
    owner = G.check_samples([3, 1, 2], 3, 6)
    packed, index = G.check_allow([m1, None, m2], 3, None, owner)
    assert packed.shape[0] == 2 and index == [0, 0, 0, -1, 1, 1]
    assert G.check_allow([None] * 3, 3, None, owner) is None
    with pytest.raises(PBError, match='entries'):                      # `allow` describes the prompts, not the rows
        G.check_allow([m1] * 6, 3, None, owner)


class _NoDevice:
    """An engine stand-in whose every attribute access fails: the calls must refuse before they touch anything but the layout."""
    BATCH_MAX = 16
    lay = ops.DEFAULT_LAYOUT

    class pb:
        pad_word_np = PAD

    def __getattr__(self, name):
        raise AssertionError('device work before the argument check: %s' % name)


@pytest.mark.parametrize('allow', [np.ones((3, V), dtype=bool), np.ones((2, V), dtype=np.int64), [np.zeros(V, dtype=bool)] * 2, 'ab'])
def test_generate_batch_refuses_before_any_device_work(allow):
    x = torch.zeros(2, 8, 8, dtype=torch.long)
    with pytest.raises(PBError, match='allow'):
        G.GenerationMixin.generate_batch(_NoDevice(), x, None, None, [np.random.RandomState(0), np.random.RandomState(1)], allow=allow)
    with pytest.raises(PBError, match='allow'):
        G.GenerationMixin.generate(_NoDevice(), x[:1], None, None, allow=allow)


# ---------------------------------------------------------------------------------------------------------------- allow_mask
def test_allow_mask_on_the_default_dictionary():
    e2w = _e2w()
    m = G.allow_mask(e2w, key='C:major')
    assert m.shape == (V,) and m.dtype == np.bool_
    pitches = _head(m, 3)
    assert pitches == {k for k in range(128) if k % 12 in C_MAJOR} and len(pitches) == 75      # melodic ids ARE the pitches; no percussion (128 .. 255)
    assert m[OFF[3] + PAD[3]:OFF[4]].all()                             # plus the specials
    for h in (0, 1, 2, 4, 5, 6, 7):
        assert len(_head(m, h)) == PAD[h], h                           # the other heads stay free
    assert np.array_equal(G.allow_mask(e2w, key='A:minor'), m)         # the relative minor: the same set
    assert _head(G.allow_mask(e2w, key='Db:major'), 3) == _head(G.allow_mask(e2w, key='C#:major'), 3) == {k for k in range(128) if (k - 1) % 12 in C_MAJOR}
    both = G.allow_mask(e2w, key='C:major', pitch_range=(48, 84))
    assert _head(both, 3) == {k for k in range(48, 84) if k % 12 in C_MAJOR} and len(_head(both, 3)) == 21
    assert _head(G.allow_mask(e2w, pitch_range=(48, 84)), 3) == set(range(48, 84))             # lo <= k < hi, percussion removed
    tempo = G.allow_mask(e2w, tempo=(90, 130))
    names = {i: float(w.split()[1]) for w, i in e2w['Tempo'].items() if i < PAD[7]}
    assert _head(tempo, 7) == {i for i, v in names.items() if 90 <= v < 130} and 0 < len(_head(tempo, 7)) < 49
    vel = G.allow_mask(e2w, velocity=(40, 100))
    vnames = {i: float(w.split()[1]) for w, i in e2w['Velocity'].items() if i < PAD[5]}
    assert _head(vel, 5) == {i for i, v in vnames.items() if 40 <= v < 100} and len(_head(vel, 5)) == 15
    assert _head(G.allow_mask(e2w, instruments=[0, '40', 'percussion', 'Instrument 7']), 2) == {0, 40, 128, 7}
    assert _head(G.allow_mask(e2w, max_duration=31), 4) == set(range(32))
    assert _head(G.allow_mask(e2w, timesig=['4/4', 'TimeSig 3/4', 5]), 6) == {e2w['TimeSig']['TimeSig 4/4'], e2w['TimeSig']['TimeSig 3/4'], 5}
    raw = G.allow_mask(e2w, key='C:major', heads={3: [60, 61, 62], 0: range(4)})               # several rules on one head intersect
    assert _head(raw, 3) == {60, 62} and _head(raw, 0) == {0, 1, 2, 3}
    assert G.allow_mask(e2w).all() and G.allow_mask().all() and G.allow_mask(ops.DEFAULT_LAYOUT, heads={1: [5]})[OFF[1] + 5]
    assert G.check_allow(both, 1)[1] == [0]                            # what the builder makes passes the argument rules


def test_allow_mask_refusals():
    e2w = _e2w()
    with pytest.raises(PBError, match='tonic'):
        G.allow_mask(e2w, key='H:major')
    with pytest.raises(PBError, match='mode'):
        G.allow_mask(e2w, key='C:dorian')
    with pytest.raises(PBError, match='TONIC:MODE'):
        G.allow_mask(e2w, key='Cmajor')
    for kw in (dict(pitch_range=(60, 60)), dict(pitch_range=(70, 60)), dict(tempo=(130, 90)), dict(velocity=(5, 5)), dict(pitch_range=(200, 300)),
               dict(tempo=(1000, 2000)), dict(key='C:major', pitch_range=(61, 62)), dict(key='C:major', heads={3: [61]})):
        with pytest.raises(PBError, match='empty|without an ordinary class'):
            G.allow_mask(e2w, **kw)
    with pytest.raises(PBError, match='no word'):
        G.allow_mask(e2w, instruments=['tuba'])
    with pytest.raises(PBError, match='outside|head'):
        G.allow_mask(e2w, heads={3: [256]})                            # a special id is not the caller's to name
    with pytest.raises(PBError, match='head'):
        G.allow_mask(e2w, heads={8: [0]})
    with pytest.raises(PBError, match='names'):
        G.allow_mask(ops.DEFAULT_LAYOUT, key='C:major')                # a layout has no names


def test_allow_mask_on_another_dictionary():
    e2w, _ = make_dict(D_SMALL)                                        # 'Pitch 0' .. 'Pitch 38', 'Tempo 0' .. 'Tempo 13', no percussion
    lay = ops.Layout.from_dict(e2w)
    assert lay.vocab == 249
    m = G.allow_mask(e2w, key='C:major')
    assert m.shape == (249,) and _head(m, 3, lay) == {k for k in range(39) if k % 12 in C_MAJOR}
    assert np.array_equal(G.allow_mask(e2w, key='A:minor'), m)
    both = G.allow_mask(e2w, key='C:major', pitch_range=(12, 30))
    assert _head(both, 3, lay) == {k for k in range(12, 30) if k % 12 in C_MAJOR}
    assert _head(G.allow_mask(e2w, tempo=(3, 9)), 7, lay) == set(range(3, 9))
    assert _head(G.allow_mask(e2w, instruments=[2, 3]), 2, lay) == {2, 3} and _head(G.allow_mask(e2w, max_duration=4), 4, lay) == set(range(5))
    with pytest.raises(PBError, match='tonic'):
        G.allow_mask(e2w, key='X:minor')
    with pytest.raises(PBError, match='mode'):
        G.allow_mask(e2w, key='C:lydian')
    with pytest.raises(PBError, match='empty|without'):
        G.allow_mask(e2w, pitch_range=(39, 50))
    packed, index = G.check_allow(both, 1, lay)
    assert packed.shape == (1, 8) and index == [0]                     # ceil(249 / 32)
    assert np.array_equal(G.unpack_allow((packed, index), 249)[0].numpy(), both)
    with pytest.raises(PBError, match='shape'):
        G.check_allow(both, 1)                                         # against the default layout: another V


# ---------------------------------------------------------------------------------------------------------------- the changed line
def _masked(row, mask):
    x = row.clone()
    x[torch.from_numpy(~np.asarray(mask))] = -np.inf
    return x


def _restated_row(row, mask):
    """The 8 heads of one position with the masked columns at -inf, through the oracle's sampling(): one draw per head, in head order."""
    x = _masked(row, mask)
    return torch.tensor([int(O.sampling(x[OFF[j]:OFF[j + 1]].clone(), O.SAMPLE_P[j], O.SAMPLE_T[j])) for j in range(8)])


def _random_mask(rng):
    """A mask that removes 30 .. 95 % of the ordinary classes of a random subset of the heads (check_allow sets the specials)."""
    m = np.ones(V, dtype=bool)
    for h in range(8):
        if rng.random_sample() < 0.7:
            keep = rng.random_sample(PAD[h]) > rng.uniform(0.3, 0.95)
            keep[rng.randint(0, PAD[h])] = True
            m[OFF[h]:OFF[h] + PAD[h]] = keep
    return m


def _row(rng, scale=3.0):
    r = rng.standard_normal(V).astype(np.float32) * scale
    for h in range(8):
        r[OFF[h] + PAD[h]:OFF[h + 1]] -= 4.0                           # special ids stay rare, the ordinary ids compete
    return torch.from_numpy(r)


def test_sample_row_with_a_mask_equals_the_restated_reference():
    """200 random logits rows x random masks: ids and generator state bit for bit, from the global stream and from a generator of its own."""
    rng = np.random.RandomState(21)
    moved = 0
    for n in range(200):
        row, mask = _row(rng), _random_mask(rng)
        np.random.seed(2000 + n)
        want = _restated_row(row, mask)
        w_state = np.random.get_state()
        for m in (mask, torch.from_numpy(mask)):
            np.random.seed(2000 + n)
            got = PianoBartLM.sample_row(PianoBartLM, row.clone(), None, allow=m)
            assert torch.equal(got, want), (n, got, want)
            assert _same_state(np.random.get_state(), w_state), n
        own = np.random.RandomState(2000 + n)
        assert torch.equal(PianoBartLM.sample_row(PianoBartLM, row.clone(), own, allow=mask), want) and _same_state(own.get_state(), w_state), n
        assert G.is_allowed(want[None].numpy(), mask), n               # every id inside the mask (or special)
        np.random.seed(2000 + n)
        free = _restated_row(row, np.ones(V, dtype=bool))
        assert _same_state(np.random.get_state(), w_state), n           # the draws of the free sample of the position
        moved += int(not torch.equal(free, want))
        np.random.seed(2000 + n)                                       # an all-true mask and no mask: today's sample
        assert torch.equal(PianoBartLM.sample_row(PianoBartLM, row.clone(), None, allow=np.ones(V, dtype=bool)), free)
        np.random.seed(2000 + n)
        assert torch.equal(PianoBartLM.sample_row(PianoBartLM, row.clone()), free)
    assert moved >= 150, moved                                         # the masks bite


def test_sample_row_with_a_mask_and_an_order_equals_the_restated_reference():
    """The same with order=: the ordered restatement of tests/test_ordered_generation_cpu.py on the row whose masked logits are -inf.
    Head 1's second pass keeps the allow mask."""
    rng = np.random.RandomState(22)
    second = 0
    for n in range(200):
        row, mask = _row(rng), _random_mask(rng)
        prev = np.asarray([int(rng.randint(0, 250)), int(rng.randint(1, 128))] + [int(rng.randint(0, PAD[h])) for h in range(2, 8)])
        floor = int(rng.choice([0, 0, int(rng.randint(0, 256))]))
        if n % 2:                                                      # a peak at prev's bar, inside the mask: head 1's mask matters
            row[OFF[0] + prev[0]] = 30.0
            mask[OFF[0] + prev[0]] = True
            floor = min(floor, int(prev[0]))
        frow = None
        if n % 5 == 0:
            frow = np.full(8, -1, dtype=np.int16)
            frow[int(rng.randint(0, 8))] = 1
        np.random.seed(3000 + n)
        want = _reference_token(_masked(row, mask), prev, floor, frow)
        w_state = np.random.get_state()
        np.random.seed(3000 + n)
        got = G.allowed_token(frow, lambda **kw: PianoBartLM.sample_row(PianoBartLM, row.clone(), None, **kw), mask, floor, prev, PAD)
        assert torch.equal(got, want), (n, got, want)
        assert _same_state(np.random.get_state(), w_state), n
        given = (frow >= 0) if frow is not None else np.zeros(8, dtype=bool)
        assert G.is_allowed(want[None].numpy(), mask, forced=None if frow is None else frow[None]), n
        if int(want[0]) == prev[0] and not given[1] and not given[0]:
            second += 1
            assert int(want[1]) >= prev[1], n
    assert second >= 50, second


# ---------------------------------------------------------------------------------------------------------------- allowed_token, is_allowed
def test_allowed_token_and_forcing():
    mask = _mask(h3=[60, 62, 64], h2=[0])
    tok = torch.tensor([1, 2, 0, 60, 5, 6, 7, 8])
    seen = {}
    sample = lambda **kw: seen.update(kw) or tok
    assert torch.equal(G.allowed_token(None, sample, mask, None, SOS, PAD), tok) and set(seen) == {'allow'} and seen['allow'] is mask
    seen.clear()
    G.allowed_token(None, sample, mask, 4, np.asarray([9, 5] + [0] * 6), PAD)
    assert set(seen) == {'allow', 'order'} and seen['allow'] is mask and seen['order'] == (9, 9, 5, -1)       # the ordered inputs travel beside the mask
    seen.clear()
    assert torch.equal(G.allowed_token(None, lambda: tok, None, None, SOS, PAD), tok)          # a free row never passes the keyword
    assert torch.equal(G.allowed_token(None, lambda: tok, None, -1, SOS, PAD), tok)
    frow = np.asarray([-1, -1, -1, 61, -1, -1, -1, -1], dtype=np.int16)                          # a given pitch OUTSIDE the mask: written as given
    got = G.allowed_token(frow, sample, mask, None, SOS, PAD)
    assert got.tolist() == [1, 2, 0, 61, 5, 6, 7, 8] and 'allow' in seen
    full = np.arange(8, dtype=np.int16) + 100                          # all 8 given: nothing is sampled, nothing drawn
    full[5] = 3

    def never(**kw):
        raise AssertionError('a fully given position samples nothing')
    state = np.random.get_state()
    assert G.allowed_token(full, never, mask, 0, SOS, PAD).tolist() == full.tolist()
    assert _same_state(np.random.get_state(), state)
    # with the real sampler: the given head is outside, the free ones inside, one block of 8 draws
    rng = np.random.RandomState(5)
    row = _row(rng)
    own, ref = np.random.RandomState(9), np.random.RandomState(9)
    got = G.allowed_token(frow, lambda **kw: PianoBartLM.sample_row(PianoBartLM, row.clone(), own, **kw), mask, None, SOS, PAD)
    ref.random_sample(8)
    assert int(got[3]) == 61 and int(got[2]) in (0,) + tuple(range(129, 135)) and _same_state(own.get_state(), ref.get_state())


def test_is_allowed_on_hand_written_rows():
    mask = _mask(h3=[60, 62, 64], h2=[0])
    ok = np.ones((5, 8), dtype=np.int64)
    ok[:, 2], ok[:, 3] = 0, [60, 62, 64, 60, 62]
    rows = np.concatenate([ok, EOS[None], PAD[None], PAD[None]])
    assert G.is_allowed(rows, mask) and G.is_allowed(torch.as_tensor(rows), torch.from_numpy(mask)) and G.is_allowed(rows.astype(np.float32), mask)
    bad = rows.copy()
    bad[1, 3] = 61
    assert not G.is_allowed(bad, mask) and not G.is_allowed(bad, mask, start=1) and G.is_allowed(bad, mask, start=2)
    forced = np.full((len(rows), 8), -1, dtype=np.int64)
    forced[1, 3] = 61
    assert G.is_allowed(bad, mask, forced=forced)                      # a given head is not tested
    forced[1, 3], forced[1, 4] = -1, 1
    assert not G.is_allowed(bad, mask, forced=forced)
    behind = rows.copy()
    behind[7, 3] = 61                                                  # behind the first special bar: not emitted
    assert G.is_allowed(behind, mask)
    spec = rows.copy()
    spec[2, 3] = 258                                                   # a special id counts as allowed (a given one; a sampled one ends the row)
    assert G.is_allowed(spec, mask)
    assert G.is_allowed(np.tile(PAD, (4, 1)), mask) and G.is_allowed(bad, mask, start=9)
    assert G.is_allowed(bad, np.ones(V, dtype=bool))


# ---------------------------------------------------------------------------------------------------------------- flags, header, binding
def test_cli_flag_rules():
    from pianobart_amd import demo as D
    from pianobart_amd import eval_generation as EG
    base = ['--nopretrain', '--seed', '0']
    a = EG.get_args(base)
    assert all(getattr(a, f) is None for f in G.ALLOW_FLAGS) and G.allow_from_args(a, _e2w()) is None
    flags = ['--key', 'C:major', '--pitch_range', '48:84', '--instruments', '0,1', '--tempo', '90:130', '--max_duration', '31', '--velocity', '40:100']
    a = EG.get_args(base + flags)
    assert (a.key, a.pitch_range, a.instruments, a.tempo, a.max_duration, a.velocity) == ('C:major', '48:84', '0,1', '90:130', 31, '40:100')
    e2w = _e2w()
    assert np.array_equal(G.allow_from_args(a, e2w), G.allow_mask(e2w, key='C:major', pitch_range=(48, 84), instruments=[0, 1], tempo=(90, 130),
                                                                  max_duration=31, velocity=(40, 100)))
    d = D.get_args(flags)
    assert np.array_equal(G.allow_from_args(d, e2w), G.allow_from_args(a, e2w)) and D.Args().key is None and D.Args(key='C:major').key == 'C:major'
    for extra in (['--key', 'C:major'], ['--key', 'C:major', '--infill', '2:4', '--ordered'], ['--pitch_range', '48:84', '--prime', 'half', '--bars', '2',
                  '--keep', 'pitch'], ['--tempo', '90:130', '--samples', '3', '--score', '--pick', 'best'], ['--max_duration', '31', '--refill']):
        a = EG.get_args(base + extra)
        a.cpu = False
        EG.check_args(a)
    for flag, v in (('--key', 'C:major'), ('--pitch_range', '48:84'), ('--velocity', '1:99')):
        with pytest.raises(PBError, match=flag):
            EG.check_args(EG.get_args(base + [flag, v, '--prime', '4', '--score_dataset']))
    with pytest.raises(PBError, match='LO:HI'):
        G.allow_from_args(EG.get_args(base + ['--pitch_range', '48']), e2w)
    with pytest.raises(PBError, match='tonic'):
        G.allow_from_args(EG.get_args(base + ['--key', 'X:major']), e2w)


def test_header_and_binding_know_the_entry_points():
    decls = _lib.parse_header()
    assert decls['pb_batch_decoder_allow'] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p])
    assert decls['pb_batch_decoder_admit_allow'] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32])
    dll = _lib.LIB.load()
    assert dll.pb_abi_version() == 10                                  # additions only
    for name in ('pb_batch_decoder_allow', 'pb_batch_decoder_admit_allow'):
        assert getattr(dll, name).argtypes == decls[name][1]
    assert dll.pb_batch_decoder_admit_allow(None, 0, 0) < 0 and b'pb_batch_decoder_admit_allow' in dll.pb_last_error()
    assert dll.pb_batch_decoder_allow(None, None, 1, 40, None) < 0 and b'pb_batch_decoder_allow' in dll.pb_last_error()
