"""CPU: the host side of the Octuple augmentation (pianobart_amd/augment.py) and the properties of its numpy restatement
(tests/augment_ref.py). No device work: plan building from names, every refusal by message, the command-line form, the batch seeds, and
what the reference promises -- identity, invertibility, and that every value of the feasible interval is drawn."""
import numpy as np
import pytest

from pianobart_amd import augment, ops
from pianobart_amd._lib import PBError
from tests import augment_ref as R
from tests.golden_util import load_vocab
from tests.vocab_layout_util import D_SMALL, D_WIDE, make_dict


def _number(word):
    return float(word.split(' ', 1)[1])


# ---------------------------------------------------------------------------------------------------- plans
def test_plan_from_the_default_dictionary():
    e2w, _ = load_vocab()
    for src in (None, ops.DEFAULT_LAYOUT, ops.Layout(list(ops.DEFAULT_LAYOUT.sizes)), e2w):
        p = augment.AugmentPlan(src, pitch=(-6, 5), velocity=(-2, 2), tempo=(-3, 1))
        assert p.axes() == ('pitch', 'velocity', 'tempo')
        assert p.plan.tolist() == [[-6, 5, 0, 127, 128, 0xFFFFFFFF], [-2, 2, 0, 31, 32, 0xFFFFFFFF], [-3, 1, 0, 48, 49, 0xFFFFFFFF]]
        # pitch: 'Pitch k' has the coordinate k = 0 .. 127; the percussion pitches and the specials have none
        for w, i in e2w['Pitch'].items():
            k = w.split(' ', 1)[1]
            assert p.coord[0, i] == (int(k) if k.isdigit() else -1), w
        assert sorted(p.coord[0][p.coord[0] >= 0].tolist()) == list(range(128))
        assert (p.coord[0, 128:] == -1).all() and p.pitch_base == 0 and p.pitch_bounds == (0, 127)
        # velocity and tempo: the rank of the word's number, monotone in it; the specials (and everything behind the head) have none
        for a, cls, n in ((1, 'Velocity', 32), (2, 'Tempo', 49)):
            words = sorted((int(p.coord[a, i]), _number(w)) for w, i in e2w[cls].items() if '<' not in w)
            assert [c for c, _ in words] == list(range(n))
            assert all(x < y for (_, x), (_, y) in zip(words, words[1:]))
            assert (p.coord[a, n:] == -1).all()
        # the inverse is total on 0 .. ncoord - 1
        for a in range(3):
            n = int(p.plan[a][4])
            assert (p.coord[a][p.id_at[a, :n]] == np.arange(n)).all()


def test_plan_axes_off_and_bounds_and_prob():
    p = augment.AugmentPlan(None, pitch=(-6, 5), pitch_bounds=(21, 108), prob=0.25)
    assert p.axes() == ('pitch',) and p.pitch_bounds == (21, 108)
    assert p.plan.tolist() == [[-6, 5, 21, 108, 128, 1 << 30], [0, 0, 0, 0, 1, 0xFFFFFFFF], [0, 0, 0, 0, 1, 0xFFFFFFFF]]
    assert (p.coord[1:] == -1).all()                                 # an axis that is off moves nothing
    assert list(p._plan18)[:6] == [-6, 5, 21, 108, 128, 1 << 30]
    q = augment.AugmentPlan(None, tempo=(0, 0), prob=1)
    assert q.plan[2].tolist() == [0, 0, 0, 48, 49, 0xFFFFFFFF] and list(q._plan18)[17] == -1
    # a request wider than any head is cut to the head's width: the clamp would cut it anyway
    assert augment.AugmentPlan(None, pitch=(-10 ** 9, 10 ** 9)).plan[0][:2].tolist() == [-ops.HEAD_MAX, ops.HEAD_MAX]


@pytest.mark.parametrize('sizes', [D_SMALL, D_WIDE])
def test_plan_from_a_second_dictionary(sizes):
    e2w, _ = make_dict(sizes)
    p = augment.AugmentPlan(e2w, pitch=(-3, 3), velocity=(-1, 1), tempo=(-1, 1), pitch_bounds=(2, sizes[3] - 9))
    assert p.layout == ops.Layout(sizes)
    for a, h in enumerate((3, 5, 7)):
        n = sizes[h] - 6                                             # every ordinary word of these dictionaries is numbered
        assert int(p.plan[a][4]) == n
        ids = np.arange(sizes[h])
        c = p.coord[a, ids]
        assert (c[:n] == np.arange(n)).all() and (c[n:] == -1).all() and (p.coord[a, sizes[h]:] == -1).all()
        assert (p.id_at[a][c[:n]] == ids[:n]).all()                  # id_at[coord[id]] == id
    assert p.plan[0][2:4].tolist() == [2, sizes[3] - 9]


def test_plan_with_a_pitch_range_that_does_not_start_at_zero():
    e2w, _ = make_dict(D_SMALL)
    e2w = {k: dict(v) for k, v in e2w.items()}
    e2w['Pitch'] = {('Pitch %d' % (int(w.split()[1]) + 21) if '<' not in w else w): i for w, i in e2w['Pitch'].items()}
    p = augment.AugmentPlan(e2w, pitch=(-2, 2), pitch_bounds=(30, 50))
    assert p.pitch_base == 21 and p.plan[0].tolist() == [-2, 2, 9, 29, 39, 0xFFFFFFFF] and p.pitch_bounds == (30, 50)
    assert p.coord[0, :39].tolist() == list(range(39)) and p.spec == 'pitch=-2:2,bounds=30:50'


# ---------------------------------------------------------------------------------------------------- refusals
def _edited(cls, fn):
    e2w, _ = make_dict(D_SMALL)
    e2w = {k: dict(v) for k, v in e2w.items()}
    e2w[cls] = fn(e2w[cls])
    return e2w


@pytest.mark.parametrize('kw,names', [
    (dict(pitch=(1, 5)), ('pitch', 'lo <= 0 <= hi')),
    (dict(velocity=(-3, -1)), ('velocity', 'lo <= 0 <= hi')),
    (dict(tempo=(2, 1)), ('tempo', 'lo <= 0 <= hi')),
    (dict(pitch=(-1.0, 1)), ('pitch', 'integers')),
    (dict(velocity=(-1, 1.5)), ('velocity', 'integers')),
    (dict(tempo=(True, 1)), ('tempo', 'integers')),
    (dict(tempo=3), ('tempo', 'pair')),
    (dict(pitch=(-1, 1), pitch_bounds=(-1, 100)), ('pitch', 'bounds', 'outside the axis')),
    (dict(pitch=(-1, 1), pitch_bounds=(21, 128)), ('pitch', 'bounds', 'outside the axis')),
    (dict(pitch=(-1, 1), pitch_bounds=(60, 59)), ('pitch', 'bounds', 'outside the axis')),
    (dict(pitch=(-1, 1), pitch_bounds=(21.0, 108)), ('pitch_bounds', 'integers')),
    (dict(pitch_bounds=(21, 108)), ('pitch', 'without a pitch request')),
    (dict(pitch=(-1, 1), prob=0.0), ('prob', '(0, 1]')),
    (dict(pitch=(-1, 1), prob=1.5), ('prob', '(0, 1]')),
    (dict(pitch=(-1, 1), prob=-0.1), ('prob', '(0, 1]')),
    (dict(pitch=(-1, 1), prob=float('nan')), ('prob', '(0, 1]')),
    (dict(pitch=(-1, 1), prob='x'), ('prob', '(0, 1]')),
])
def test_plan_refusals_on_the_default_dictionary(kw, names):
    with pytest.raises(PBError) as e:
        augment.AugmentPlan(None, **kw)
    assert str(e.value).startswith('augment:') and all(n in str(e.value) for n in names), str(e.value)


def test_plan_refusals_from_the_dictionary():
    with pytest.raises(PBError, match='not a Layout'):                                    # a bare layout has no names
        augment.AugmentPlan(ops.Layout(D_SMALL), pitch=(-1, 1))
    # an axis whose head has no numbered word -- refused only when the axis is asked for
    named = _edited('Tempo', lambda t: {('Tempo slow%d' % i if '<' not in w else w): i for w, i in t.items()})
    with pytest.raises(PBError, match=r'augment: tempo: head 7 \(Tempo\) has no numbered word'):
        augment.AugmentPlan(named, tempo=(-1, 1))
    assert augment.AugmentPlan(named, pitch=(-1, 1)).axes() == ('pitch',)
    drums = _edited('Pitch', lambda t: {('Pitch percussion %s' % w.split()[1] if '<' not in w else w): i for w, i in t.items()})
    with pytest.raises(PBError, match=r'augment: pitch: head 3 \(Pitch\) has no numbered word'):
        augment.AugmentPlan(drums, pitch=(-1, 1))
    # gaps in the coordinates
    gap = _edited('Pitch', lambda t: {('Pitch 100' if w == 'Pitch 7' else w): i for w, i in t.items()})
    with pytest.raises(PBError, match=r"augment: pitch: gap in the coordinates between 'Pitch 6' and 'Pitch 8'"):
        augment.AugmentPlan(gap, pitch=(-1, 1))
    twice = _edited('Velocity', lambda t: {('Velocity 3.0' if w == 'Velocity 4' else w): i for w, i in t.items()})
    with pytest.raises(PBError, match=r'augment: velocity: .*carry the same number'):
        augment.AugmentPlan(twice, velocity=(-1, 1))
    with pytest.raises(PBError, match='Layout'):                                          # not an Octuple dictionary at all
        augment.AugmentPlan({'Pitch': {}}, pitch=(-1, 1))


def test_velocity_task_refuses_the_velocity_axis():
    plan = augment.AugmentPlan(None, pitch=(-2, 2), velocity=(-1, 1))
    with pytest.raises(PBError, match=r'augment: velocity: the velocity task predicts the velocity'):
        augment.check_task(plan, 'velocity')
    for task in ('composer', 'emotion', 'melody', None):
        assert augment.check_task(plan, task) is plan
    no_vel = augment.AugmentPlan(None, pitch=(-2, 2), tempo=(-1, 1))
    assert augment.check_task(no_vel, 'velocity') is no_vel and augment.check_task(None, 'velocity') is None
    # the driver refuses from its arguments, before any data is loaded
    from pianobart_amd.finetune import get_args_finetune
    args = get_args_finetune(['--task', 'velocity', '--dataset', 'asap', '--augment', 'pitch=-2:2,velocity=-1:1'])
    with pytest.raises(PBError, match='velocity task'):
        augment.from_args(args, load_vocab()[0], task=args.task)
    args = get_args_finetune(['--task', 'melody', '--dataset', 'POP909', '--augment', 'pitch=-2:2,velocity=-1:1', '--augment_prob', '0.5'])
    plan = augment.from_args(args, load_vocab()[0], task=args.task)
    assert plan.axes() == ('pitch', 'velocity') and plan.prob == 0.5


# ---------------------------------------------------------------------------------------------------- command line
def test_parse_round_trips():
    spec = 'pitch=-6:5,velocity=-2:2,tempo=-2:2,bounds=21:108'
    kw = augment.parse(spec)
    assert kw == dict(pitch=(-6, 5), velocity=(-2, 2), tempo=(-2, 2), pitch_bounds=(21, 108))
    assert augment.format_spec(**kw) == spec and augment.AugmentPlan(None, **kw).spec == spec
    for spec in ('pitch=-6:5', 'tempo=0:3', 'velocity=-1:0,tempo=-4:4', 'pitch=0:0,bounds=0:127'):
        assert augment.format_spec(**augment.parse(spec)) == spec
        p = augment.AugmentPlan(None, **augment.parse(spec))         # a plan's own spec spells the pitch bounds out: the same plan again
        assert (augment.AugmentPlan(None, **augment.parse(p.spec)).plan == p.plan).all()
    assert augment.parse(' pitch = -1 : +2 , tempo=0:0 ') == dict(pitch=(-1, 2), tempo=(0, 0))
    for bad, word in (('', 'empty'), ('pitch', 'NAME=LO:HI'), ('pitch=1', 'NAME=LO:HI'), ('pitch=-1.5:2', 'NAME=LO:HI'), ('key=-1:1', 'unknown axis'),
                      ('pitch=-1:1,pitch=-2:2', 'twice'), ('pitch=-1:1,,tempo=0:1', 'NAME=LO:HI')):
        with pytest.raises(PBError, match=word):
            augment.parse(bad)


@pytest.mark.parametrize('parse', ['pretrain', 'finetune', 'generation'])
def test_driver_flags_are_off_by_default(parse):
    from pianobart_amd.finetune import get_args_finetune
    from pianobart_amd.finetune_generation import get_args_generation
    from pianobart_amd.pretrain import get_args_pretrain
    fn, base = {'pretrain': (get_args_pretrain, []), 'generation': (get_args_generation, []),
                'finetune': (get_args_finetune, ['--task', 'composer', '--dataset', 'Pianist8'])}[parse]
    a = fn(base)
    assert a.augment is None and a.augment_prob == 1.0 and a.augment_seed == 0
    assert augment.from_args(a, None) is None                        # off: nothing is built, the dictionary is not even read
    a = fn(base + ['--augment', 'pitch=-6:5,tempo=-2:2', '--augment_prob', '0.75', '--augment_seed', '7'])
    plan = augment.from_args(a, load_vocab()[0])
    assert plan.spec == 'pitch=-6:5,tempo=-2:2,bounds=0:127' and plan.prob == 0.75 and a.augment_seed == 7


# ---------------------------------------------------------------------------------------------------- seeds
def _mix(x):
    """splitmix64's output function on the state x + golden gamma (Steele, Lea, Flood 2014), written out once more."""
    m = (1 << 64) - 1
    z = (x + 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def test_batch_seed():
    assert _mix(0) == 0xE220A8397B1DCDAF                             # the published first output of splitmix64 seeded with 0
    # three values worked out step by step from the four mixes
    assert augment.batch_seed(0, 0, 0, 0) == 0x2130748AAAC80268 == _mix(_mix(_mix(_mix(0))))
    assert augment.batch_seed(1, 2, 3, 4) == 0xD55CCD4AEB3CCAFB == _mix(_mix(_mix(_mix(1) ^ 2) ^ 3) ^ 4)
    assert augment.batch_seed(0xDEADBEEF, 1, 499, 1023) == 0xFFF774C0242C5A2F
    base = (5, 1, 17, 300)
    seen = {augment.batch_seed(*base)}
    for k in range(4):
        for v in range(base[k] + 1, base[k] + 65):
            args = list(base)
            args[k] = v
            seen.add(augment.batch_seed(*args))
    assert len(seen) == 1 + 4 * 64                                   # every argument matters, and no two of these collide
    assert augment.batch_seed(*base) == augment.batch_seed(*base) and 0 <= augment.batch_seed(*base) < 1 << 64
    assert augment.batch_seed(-1, 0, 0, 0) == augment.batch_seed((1 << 64) - 1, 0, 0, 0)


# ---------------------------------------------------------------------------------------------------- the reference
def _pieces(rng, B, S, sizes=ops.DEFAULT_LAYOUT.sizes):
    """Random pieces: ordinary rows (pitches in a window of the piece's own, so that there is room to move), a few special rows, PAD tail."""
    n = np.asarray(sizes)
    ids = np.empty((B, S, 8), dtype=np.int64)
    for b in range(B):
        rows = np.stack([rng.integers(0, n[h] - 6, size=S) for h in range(8)], axis=1)
        lo = rng.integers(0, 100)
        rows[:, 3] = rng.integers(lo, lo + rng.integers(1, 28), size=S)
        for h in (5, 7):                                             # dynamics and tempo in a window too
            m = n[h] - 6
            lo = rng.integers(0, m // 2)
            rows[:, h] = rng.integers(lo, lo + rng.integers(1, m // 4 + 1), size=S)
        rows[rng.random(S) < 0.1] = n - 6 + rng.integers(0, 6)       # a special row
        rows[int(rng.integers(1, S + 1)):] = n - 6                   # PAD tail
        ids[b] = rows
    return ids


def test_reference_zero_request_is_the_identity():
    ids = _pieces(np.random.default_rng(1), 8, 50)
    p = augment.AugmentPlan(None, pitch=(0, 0), velocity=(0, 0), tempo=(0, 0))
    out, s = R.reference(ids, p.coord, p.id_at, p.plan, 99)
    assert (out == ids).all() and (s == 0).all()


def test_reference_shift_then_its_negative_restores_the_input():
    rng = np.random.default_rng(2)
    ids = _pieces(rng, 64, 40)
    p = augment.AugmentPlan(None, pitch=(-6, 5), velocity=(-2, 2), tempo=(-2, 2))
    out, s = R.reference(ids, p.coord, p.id_at, p.plan, 1234)
    assert (s != 0).any(axis=0).all() and (out != ids).any()
    assert (out[:, :, [0, 1, 2, 4, 6]] == ids[:, :, [0, 1, 2, 4, 6]]).all()
    # Forcing -s on the shifted piece. A feasible interval always holds 0 (lo <= 0 <= hi, and a clamp that excludes 0 means "no shift"),
    # so no request can force a non-zero draw; the shift is forced through the apply step, under a plan whose request admits it.
    q = augment.AugmentPlan(None, **{n: (min(0, int(-s[:, a].max())), max(0, int(-s[:, a].min()))) for a, n in enumerate(augment.AXES)})
    back = R.apply_shifts(out, q.coord, q.id_at, q.plan, -s)
    assert (back == ids).all()
    # and the admitted draws of that plan on the shifted pieces stay inside what the clamp allows: shifting back never leaves the axis
    _, t = R.reference(out, q.coord, q.id_at, q.plan, 77)
    for a in range(3):
        c = R.coords(out, q.coord, q.plan, a)
        moved = np.where(c >= 0, c + t[:, a][:, None], 0)
        assert moved.min() >= 0 and moved.max() < int(q.plan[a][4])
    # and the shifted piece keeps its intervals: coordinate differences inside a piece are unchanged
    for a in range(3):
        c0, c1 = R.coords(ids, p.coord, p.plan, a), R.coords(out, p.coord, p.plan, a)
        assert ((c0 >= 0) == (c1 >= 0)).all() and (np.where(c0 >= 0, c1 - c0, 0) == np.where(c0 >= 0, s[:, a][:, None], 0)).all()


def draw_cases():
    """(w, ids, plan): 4096 single-note pieces whose feasible pitch interval holds exactly w values, w = 1 .. 12; shared with the GPU test."""
    ids = np.zeros((4096, 1, 8), dtype=np.int64)
    ids[:, 0, 3] = 60
    ids[:, 0, 5], ids[:, 0, 7] = 16, 24
    for w in range(1, 13):
        lo = -(w // 2)
        yield w, ids, augment.AugmentPlan(None, pitch=(lo, lo + w - 1))


def test_reference_draws_every_value_of_the_feasible_interval():
    for w, ids, p in draw_cases():
        _, s = R.reference(ids, p.coord, p.id_at, p.plan, 0xA5A5 + w)
        lo, hi = int(p.plan[0][0]), int(p.plan[0][1])
        assert sorted(set(s[:, 0].tolist())) == list(range(lo, hi + 1)), w
        assert (s[:, 1:] == 0).all()
        counts = np.bincount(s[:, 0] - lo, minlength=w)
        assert counts.min() > 4096 / w * 0.7                         # uniform: 4096 / 12 = 341 expected, sigma 18


def test_reference_clamps_by_the_pieces_own_extremes():
    p = augment.AugmentPlan(None, pitch=(-6, 5), pitch_bounds=(21, 108))
    ids = np.zeros((6, 3, 8), dtype=np.int64)
    ids[:, :, 3] = [[21, 60, 108], [21, 30, 40], [100, 104, 108], [24, 60, 106], [20, 60, 70], [130, 256, 259]]
    seen = [set() for _ in range(6)]
    for seed in range(300):
        out, s = R.reference(ids, p.coord, p.id_at, p.plan, seed)
        for b in range(6):
            seen[b].add(int(s[b, 0]))
        assert (out[5] == ids[5]).all() and (out[4] == ids[4]).all() and (out[0] == ids[0]).all()
        assert out[:, :, 3][:4].min() >= 21 and out[:, :, 3][:4].max() <= 108
    assert seen[0] == {0}                                            # fills the bounds
    assert seen[1] == set(range(0, 6)) and seen[2] == set(range(-6, 1)) and seen[3] == set(range(-3, 3))
    assert seen[4] == {0} and seen[5] == {0}                         # a note outside the bounds; only percussion and specials


def test_reference_prob_leaves_rows_alone():
    ids = _pieces(np.random.default_rng(3), 2000, 4)
    p = augment.AugmentPlan(None, pitch=(1 - 1, 5), prob=0.25)
    q = augment.AugmentPlan(None, pitch=(0, 5))
    _, s = R.reference(ids, p.coord, p.id_at, p.plan, 8)
    _, t = R.reference(ids, q.coord, q.id_at, q.plan, 8)
    applied = s[:, 0] != 0
    assert (s[applied] == t[applied]).all()                          # where it applies, it is the draw of prob = 1
    free = t[:, 0] != 0
    assert 0.19 < applied.sum() / free.sum() < 0.31                  # 0.25 +- 5 sigma over ~1600 rows
