"""CPU: time-ordered generation (Engine.generate / generate_batch(order=...)) -- the argument rules (generation.check_order), the property
check (is_time_ordered) on hand-written rows, the changed line (generation.ordered_token + PianoBartLM.sample_row's ordered inputs) against
a restatement of the contract written here with the oracle's sampling(), the infilling property, the flag rules and the two new entry
points in the header and the binding. No device work.

Contract ("Time-ordered sampling"): the reference loop with `current_output = self.sample(x, i)` replaced by the
ordered sample; `_reference_token` below restates it step by step."""
import numpy as np
import pytest
import torch

from oracle import pianobart_oracle as O
from pianobart_amd import _lib
from pianobart_amd import generation as G
from pianobart_amd import ops
from pianobart_amd._lib import PBError
from pianobart_amd.model import PianoBartLM

PAD = np.asarray([256, 128, 129, 256, 128, 32, 254, 49])
SOS = PAD + 2
MASK = PAD + 1
EOS = PAD + 3
OFF = ops.SEG_OFF


# ---------------------------------------------------------------------------------------------------------------- check_order
def test_check_order_accepts_and_normalises():
    assert G.check_order(None, 3) is None
    assert G.check_order([-1] * 3, 3) is None                          # no ordered row: the caller runs what it ran before
    assert G.check_order(np.full(2, -1), 2) is None and G.check_order(torch.full((2,), -1), 2) is None
    assert G.check_order([4, -1, 0], 3) == [4, -1, 0]
    assert G.check_order((0, 255), 2) == [0, 255]
    assert G.check_order(np.asarray([7, -1], dtype=np.int32), 2) == [7, -1]
    assert G.check_order(torch.tensor([7, 9]), 2) == [7, 9]
    got = G.check_order([np.int64(3)], 1)
    assert got == [3] and type(got[0]) is int
    assert G.check_order([0], 1) == [0]                                # 0 is "ordered, no extra floor", not "off"
    assert G.check_order([], 0) is None


def test_check_order_refusals():
    for bad, P in (([1, 2], 3), ([1, 2, 3], 2), ([], 1), (np.zeros((2, 2), dtype=np.int64), 4)):
        with pytest.raises(PBError, match='entries|integer'):
            G.check_order(bad, P)
    with pytest.raises(PBError, match='sequence'):
        G.check_order(5, 1)
    for bad in ([1.0, 2], [True, 2], ['3', 2], [None, 2], np.asarray([1.5, 2.0]), torch.tensor([1.0, 2.0])):
        with pytest.raises(PBError, match='not an integer'):
            G.check_order(bad, 2)
    for bad in ([-2, 2], [3, 256], [3, 1000]):
        with pytest.raises(PBError, match='outside -1 .. 255'):
            G.check_order(bad, 2)


def test_check_order_expands_through_owner():
    owner = G.check_samples([3, 1, 2], 3, 6)
    assert G.check_order([4, -1, 9], 3, owner) == [4, 4, 4, -1, 9, 9]
    assert G.check_order([-1] * 3, 3, owner) is None
    with pytest.raises(PBError, match='entries'):                      # `order` describes the prompts, not the rows
        G.check_order([4] * 6, 3, owner)


class _NoDevice:
    """An engine stand-in whose every attribute access fails: the calls must refuse before they touch anything but the PAD word."""
    BATCH_MAX = 16

    class pb:
        pad_word_np = PAD

    def __getattr__(self, name):
        raise AssertionError('device work before the argument check: %s' % name)


@pytest.mark.parametrize('order', [[1], [1, 2, 3], [1, 256], [-2, 2], [1.0, 2.0], 'ab'])
def test_generate_batch_refuses_before_any_device_work(order):
    x = torch.zeros(2, 8, 8, dtype=torch.long)
    with pytest.raises(PBError, match='order'):
        G.GenerationMixin.generate_batch(_NoDevice(), x, None, None, [np.random.RandomState(0), np.random.RandomState(1)], order=order)
    if len(order) != 1:                                                # one entry is what `generate` takes
        with pytest.raises(PBError, match='order'):
            G.GenerationMixin.generate(_NoDevice(), x[:1], None, None, order=order)


# ---------------------------------------------------------------------------------------------------------------- is_time_ordered
def _rows(pairs, tail=True):
    """Rows with the given (bar, position) pairs, the other heads 1; an EOS row and PAD behind them."""
    x = np.ones((len(pairs), 8), dtype=np.int64)
    x[:, :2] = np.asarray(pairs).reshape(-1, 2)
    return np.concatenate([x, EOS[None], PAD[None], PAD[None]]) if tail else x


def test_is_time_ordered_on_hand_written_rows():
    good = _rows([(0, 0), (0, 0), (0, 5), (1, 2), (1, 2), (3, 0), (3, 127)])
    assert G.is_time_ordered(good) and G.is_time_ordered(torch.as_tensor(good)) and G.is_time_ordered(good.astype(np.float32))
    assert G.is_time_ordered(good, start=3, floor=1) and not G.is_time_ordered(good, start=3, floor=2)
    assert G.is_time_ordered(good, start=0, floor=0) and not G.is_time_ordered(good, floor=1)
    assert not G.is_time_ordered(_rows([(0, 0), (1, 0), (0, 9)]))      # the bar goes back
    assert not G.is_time_ordered(_rows([(2, 8), (2, 7)]))              # the position goes back inside a bar
    assert G.is_time_ordered(_rows([(2, 8), (3, 0)]))                  # a new bar may start at any position
    back = _rows([(5, 9), (2, 0), (2, 4), (6, 0)])
    assert not G.is_time_ordered(back, start=1)                        # `start` compares with the row in front of it: from prev on
    assert G.is_time_ordered(back, start=2) and not G.is_time_ordered(back, start=2, floor=3)
    assert G.is_time_ordered(_rows([(9, 9), (1, 1)]), start=7)         # nothing emitted from `start` on
    assert G.is_time_ordered(np.concatenate([_rows([(4, 4)], tail=False), PAD[None], _rows([(0, 0)], tail=False)]))    # rows behind the first PAD are not emitted
    assert G.is_time_ordered(_rows([(0, 1), (0, 2)], tail=False))      # no special row at all: the window's end
    assert G.is_time_ordered(np.tile(PAD, (4, 1)))


# ---------------------------------------------------------------------------------------------------------------- the changed line
def _reference_token(row, prev, floor, frow):
    """The contract's steps, restated: the ordered sample of one position followed by forcing. row (1280,) f32 logits; prev (8,) ids; floor
    -1 .. 255; frow (8,) given ids (-1 = free) or None. sampling() is the oracle's (model.py:101-107): it divides by the temperature itself,
    and -inf / t = -inf, so masking the logit masks the quotient. Draws: one per head in head order from the global stream, none where all
    8 heads are given."""
    if frow is not None and (frow >= 0).all():
        return torch.as_tensor(frow.astype(np.int64))                  # 6: a position with all 8 heads given draws nothing
    x = [row[OFF[j]:OFF[j + 1]].clone() for j in range(8)]
    if floor >= 0:                                                     # 1: head 0
        low = max(floor, int(prev[0]) if prev[0] < PAD[0] else 0)
        x[0][:low] = -np.inf
    ids = [int(O.sampling(x[0], O.SAMPLE_P[0], O.SAMPLE_T[0]))]
    b0 = int(frow[0]) if frow is not None and frow[0] >= 0 else ids[0]  # 2: b0 is head 0's id after forcing
    if floor >= 0 and prev[0] < PAD[0] and prev[1] < PAD[1] and b0 == prev[0]:      # 3: head 1
        x[1][:int(prev[1])] = -np.inf
    for j in range(1, 8):                                              # 4: heads 2 .. 7 untouched
        ids.append(int(O.sampling(x[j], O.SAMPLE_P[j], O.SAMPLE_T[j])))
    tok = torch.tensor(ids)
    if frow is not None:                                               # 5: given heads are never masked or changed
        given = torch.as_tensor(frow >= 0)
        tok[given] = torch.as_tensor(frow.astype(np.int64))[given]
    return tok


def _ours(row, prev, floor, frow):
    return G.ordered_token(frow, lambda **kw: PianoBartLM.sample_row(PianoBartLM, row, None, **kw), floor, prev, PAD)


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def _cases():
    """A few hundred (logits row, prev, floor, forced row): random ones and the corners the contract names."""
    rng = np.random.RandomState(11)
    out = []

    def row(scale=3.0, flat01=True):
        r = rng.standard_normal(ops.VOCAB).astype(np.float32) * scale
        if flat01:                                                     # specials of heads 0 and 1 stay rare, the ordinary ids compete
            r[OFF[0] + 256:OFF[1]] -= 4.0
            r[OFF[1] + 128:OFF[2]] -= 4.0
        return torch.from_numpy(r)

    def prev(bar, pos):
        p = np.asarray([bar, pos] + [int(rng.randint(0, PAD[h])) for h in range(2, 8)])
        return p

    for i in range(240):
        p = prev(int(rng.randint(0, 256)), int(rng.randint(0, 128)))
        floor = int(rng.choice([-1, 0, 0, int(rng.randint(0, 256))]))
        frow = None
        if i % 3 == 0:
            frow = np.full(8, -1, dtype=np.int16)
            for h in range(8):
                if rng.random_sample() < 0.3:
                    frow[h] = int(rng.randint(0, ops.SEG_SIZES[h]))
        out.append((row(), p, floor, frow))
    # the rows below make the argmax of an unmasked head 0 equal prev's bar often: a peak at prev[0], so head 1's mask matters
    for i in range(60):
        p = prev(int(rng.randint(0, 250)), int(rng.randint(1, 128)))
        r = row()
        r[OFF[0] + p[0]] = 30.0
        out.append((r, p, int(rng.choice([0, p[0], max(0, p[0] - 3)])), None))
    g = lambda kw: np.asarray([kw.get(h, -1) for h in range(8)], dtype=np.int16)
    sos = SOS.copy()
    out.append((row(), sos, 0, None))                                  # prev = the SOS row: low = floor, head 1 free
    out.append((row(), sos, 17, None))
    out.append((row(), prev(5, 129), 0, None))                         # prev[1] special: head 1 free
    peak = row(); peak[OFF[0] + 5] = 30.0
    out.append((peak, prev(5, 129), 0, None))
    out.append((row(), prev(9, 40), 0, g({0: 9})))                   # b0 given, equal to prev's bar: head 1 masked whatever head 0 sampled
    out.append((row(), prev(9, 40), 0, g({0: 3})))                   # b0 given and BELOW prev: given heads are never masked; head 1 free
    out.append((row(), prev(9, 40), 0, g({0: 9, 1: 2})))             # head 1 given too: kept
    out.append((row(), prev(9, 40), 0, g({0: 258})))                 # b0 special (given)
    spec = row(); spec[OFF[0] + 259] = 40.0
    out.append((spec, prev(9, 40), 0, None))                           # b0 special (sampled): EOS stays reachable
    out.append((row(), prev(9, 40), 255, None))                        # floor 255: bar 255 or a special id
    out.append((row(), prev(255, 127), 255, None))
    peak = row(); peak[OFF[0] + 77] = 30.0
    out.append((peak, prev(77, 127), 0, None))                         # the head-1 mask removes every class below 127
    out.append((row(), prev(200, 3), 0, g({h: 1 for h in range(8)})))    # all 8 given: nothing drawn
    out.append((row(), prev(200, 3), -1, g({h: 1 for h in range(8)})))
    return out


def test_the_changed_line_equals_its_restatement():
    cases = _cases()
    masked1 = differs = 0
    for n, (row, prev, floor, frow) in enumerate(cases):
        np.random.seed(1000 + n)
        want = _reference_token(row, prev, floor, frow)
        w_state = np.random.get_state()
        np.random.seed(1000 + n)
        got = _ours(row.clone(), prev, floor, frow)
        assert torch.equal(got, want), (n, prev[:2], floor, frow, got, want)
        assert _same_state(np.random.get_state(), w_state), n           # the same draws consumed
        np.random.seed(1000 + n)
        free = _reference_token(row, prev, -1, frow)
        assert _same_state(np.random.get_state(), w_state), n           # ... as the unordered sample of the position consumes
        if floor >= 0:
            differs += int(not torch.equal(free, want))
            given = (frow >= 0) if frow is not None else np.zeros(8, dtype=bool)
            if not given[0]:
                assert int(want[0]) >= max(floor, prev[0] if prev[0] < PAD[0] else 0), n
            if prev[0] < PAD[0] and prev[1] < PAD[1] and int(want[0]) == prev[0] and not given[1]:
                masked1 += 1
                assert int(want[1]) >= prev[1], n
            assert torch.equal(want[2:], free[2:]), n                  # heads 2 .. 7 never change
    assert masked1 >= 40 and differs >= 100, (masked1, differs)        # the constraint bites in these cases


def test_sample_row_without_the_inputs_is_todays():
    rng = np.random.RandomState(3)
    for n in range(20):
        row = torch.from_numpy(rng.standard_normal(ops.VOCAB).astype(np.float32) * 3)
        np.random.seed(n)
        want = torch.tensor([int(O.sampling(row[OFF[j]:OFF[j + 1]].clone(), O.SAMPLE_P[j], O.SAMPLE_T[j])) for j in range(8)])
        state = np.random.get_state()
        for call in (lambda: PianoBartLM.sample_row(PianoBartLM, row), lambda: PianoBartLM.sample_row(PianoBartLM, row, None, order=None),
                     lambda: G.ordered_token(None, lambda **kw: PianoBartLM.sample_row(PianoBartLM, row, None, **kw), None, SOS, PAD),
                     lambda: G.ordered_token(None, lambda: PianoBartLM.sample_row(PianoBartLM, row), -1, SOS, PAD)):
            np.random.seed(n)
            assert torch.equal(call(), want) and _same_state(np.random.get_state(), state)
        r2 = np.random.RandomState(n)
        assert torch.equal(PianoBartLM.sample_row(PianoBartLM, row, r2, order=(0, 300, 0, -1)), want)      # an empty mask: the same ids
        assert _same_state(r2.get_state(), state)


def test_an_unordered_row_never_passes_the_keyword():
    """The paths call sample_row with `order` only for an ordered row: a caller's own sample_row without the keyword keeps working."""
    tok = torch.arange(8)
    assert torch.equal(G.ordered_token(None, lambda: tok, None, SOS, PAD), tok)
    assert torch.equal(G.ordered_token(None, lambda: tok, -1, SOS, PAD), tok)
    seen = {}
    G.ordered_token(np.asarray([7, -1, -1, -1, -1, -1, -1, -1], dtype=np.int16), lambda **kw: seen.update(kw) or tok, 4, np.asarray([9, 5] + [0] * 6), PAD)
    assert seen == dict(order=(9, 9, 5, 7))
    seen.clear()
    G.ordered_token(None, lambda **kw: seen.update(kw) or tok, 4, SOS, PAD)
    assert seen == dict(order=(4, int(SOS[0]), 0, -1))


# ---------------------------------------------------------------------------------------------------------------- infilling
def _piece(S=40):
    """An ordered piece: bar i // 4, positions rising inside a bar, an EOS row, PAD behind."""
    x = np.ones((S, 8), dtype=np.int64)
    n = 30
    x[:n, 0], x[:n, 1] = np.arange(n) // 4, (np.arange(n) % 4) * 16
    x[n], x[n + 1:] = EOS, PAD
    return x


def test_infill_splice_of_an_ordered_region_is_ordered():
    S, lo, hi = 40, 2, 4
    piece = _piece(S)
    assert G.is_time_ordered(piece)
    plan = G.infill_plan(piece, lo, hi, MASK, PAD)
    k = plan['k']
    assert k == 8

    def out_row(region):
        y = np.tile(PAD, (S, 1))
        y[:k] = plan['prefix']
        y[k:k + len(region)] = region
        return y
    region = np.ones((6, 8), dtype=np.int64)
    region[:, 0], region[:, 1] = [2, 2, 2, 3, 3, 3], [0, 0, 70, 5, 5, 127]
    row, cut = G.infill_splice(out_row(region), plan['suffix'], S, 256)
    assert not cut and G.is_time_ordered(row) and G.is_time_ordered(row, start=k, floor=lo)
    assert np.array_equal(row[k + 6:k + 6 + len(plan['suffix'])], plan['suffix'])
    bad = region.copy()
    bad[2, 0] = lo - 1                                                 # one row of the bar in front of the region: it would sound in the part left alone
    row, _ = G.infill_splice(out_row(bad), plan['suffix'], S, 256)
    assert not G.is_time_ordered(row) and not G.is_time_ordered(row, start=k, floor=lo)
    first = region.copy()
    first[0, :2] = lo - 1, 127                                         # ... even as the first new row, where the pairs still rise: the floor catches it
    row, _ = G.infill_splice(out_row(first), plan['suffix'], S, 256)
    assert G.is_time_ordered(row) and not G.is_time_ordered(row, start=k, floor=lo)
    with pytest.raises(ValueError, match='decrease'):                  # the generator's own output, fed back: only an ordered one is a piece again
        G.infill_plan(G.infill_splice(out_row(bad), plan['suffix'], S, 256)[0], lo, hi, MASK, PAD)


# ---------------------------------------------------------------------------------------------------------------- flags, header, binding
def test_cli_flag_rules():
    from pianobart_amd import demo as D
    from pianobart_amd import eval_generation as EG
    base = ['--nopretrain', '--seed', '0']
    assert EG.get_args(base).ordered is False and EG.get_args(base + ['--ordered']).ordered is True
    assert D.get_args([]).ordered is False and D.get_args(['--ordered']).ordered is True and D.Args().ordered is False and D.Args(ordered=True).ordered
    for extra in (['--ordered'], ['--ordered', '--infill', '2:4'], ['--ordered', '--prime', 'half', '--bars', '2', '--keep', 'pitch'],
                  ['--ordered', '--samples', '3', '--score', '--pick', 'best'], ['--ordered', '--refill']):
        a = EG.get_args(base + extra)
        a.cpu = False
        EG.check_args(a)
    with pytest.raises(PBError, match='--ordered'):
        EG.check_args(EG.get_args(base + ['--ordered', '--prime', '4', '--score_dataset']))


def test_header_and_binding_know_the_entry_points():
    decls = _lib.parse_header()
    import ctypes
    assert decls['pb_batch_decoder_order'] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p])
    assert decls['pb_batch_decoder_admit_order'] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32])
    dll = _lib.LIB.load()
    assert dll.pb_abi_version() == 10                                  # additions only
    for name in ('pb_batch_decoder_order', 'pb_batch_decoder_admit_order'):
        assert getattr(dll, name).argtypes == decls[name][1]
    assert dll.pb_batch_decoder_admit_order(None, 0, 0) < 0 and b'pb_batch_decoder_admit_order' in dll.pb_last_error()
