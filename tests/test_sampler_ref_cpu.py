"""CPU: the float64 sampler of tests/sampler_ref.py is sound, and the cases tests/test_sampler_kernel_gpu.py runs are decided.

  * hand-worked rows: the ids are written out by hand;
  * against the project's host sampler (PianoBartLM.sample_row -> pb_nucleus_rows / _nucleus_with_draw) on the random rows of the default
    setting, plain, time-ordered and masked: on every decided head the host's id is the reference's. Heads where two candidates have bit-equal
    f32 probabilities are skipped (numpy's sort order, not the kernel's rule, decides there on the host) and counted: 0 (3910 heads equal, 2 undecided).
  * the caps the GPU test re-asserts on its own chain: every crafted (position, head) of every setting is decided, and of the random ones at
    most 5 % per setting are not. By measure the draws within eps of one of kc boundaries are about 2 eps kc of all draws: below 1 % for a
    262-class head, and 5 % leaves room for the wide heads. The shares are printed; measured: see tests/test_sampler_kernel_gpu.py."""
import numpy as np
import pytest
import torch

from tests import sampler_ref as R

F32 = lambda v: np.asarray(v, dtype=np.float32)


def _one(probs, p, u, allowed=None, T=1.0):
    return R.head_ids(np.log(F32(probs)) * np.float32(T), T, p, u, allowed)


# ---------------------------------------------------------------------------------------------------------------- hand-worked rows
def test_hand_worked_nucleus():
    """Probabilities .5, .25, .125, .125 on the classes 2, 0, 3, 1: the order is 2, 0, 1, 3 (the tie by class), the cumulative sums .5, .75,
    .875, 1 (over 1.00001), so p = .9 keeps all four and the candidates' intervals are [0, .5), [.5, .75), [.75, .875), [.875, 1)."""
    probs = [.25, .125, .5, .125]
    for u, want in ((.25, 2), (.625, 0), (.8125, 1), (.9375, 3), (0.0, 2), (R.JUST_BELOW_1, 3)):
        assert _one(probs, .9, u) == {want}, u
    # p = .8: the first cumulative sum above it is .875 -> three candidates with the intervals [0, 4/7), [4/7, 6/7), [6/7, 1)
    for u, want in ((.3, 2), (.7, 0), (.9, 1), (0.0, 2), (R.JUST_BELOW_1, 1)):
        assert _one(probs, .8, u) == {want}, u
    assert _one(probs, 1.0, .7) == {2}                             # p = 1: the largest
    # a draw on a boundary is not decided: both neighbours are acceptable
    assert _one(probs, .9, .5) == {2, 0}
    # a threshold no prefix exceeds (the sums end at 1 / 1.00001): the top class
    assert _one(probs, .9999999, .99) == {2}
    # two tied classes over exact zeros: f32 arithmetic is exact, so a threshold ON the first cumulative sum is decided: `>` does not take it, both
    # classes are candidates and the draw chooses; the next f32 below it is exceeded by the first class alone
    pair = np.full(70, -300.0, dtype=np.float32)
    pair[[66, 3]] = 0
    for u, want in ((.26, 3), (.48, 3), (.52, 66), (.74, 66), (0.0, 3), (R.JUST_BELOW_1, 66)):
        assert R.head_ids(pair, 1.2, R.P_EXACT, u) == {want}, u
        assert R.head_ids(pair, 1.2, float(np.nextafter(np.float32(R.P_EXACT), np.float32(0))), u) == {3}, u
        assert R.head_ids(pair, 1.2, .9, u) == {want}, u


def test_hand_worked_ties_one_hot_floor_and_mask():
    flat = np.zeros(8, dtype=np.float32)
    assert R.head_ids(flat, 1.2, 1.0, .3) == {0}                   # a full tie, p = 1: the lowest class
    # ... p = .9: the cumulative sums are k / 8 (over 1.00001), the first above .9 is the last: 8 candidates in class order
    for k in range(8):
        assert R.head_ids(flat, 1.2, .9, (k + .5) / 8) == {k}
    ok = np.ones(8, dtype=bool)
    ok[[0, 1, 4]] = False
    assert R.head_ids(flat, 5.0, 1.0, .3, ok) == {2}               # the lowest ALLOWED class
    for k, want in enumerate((2, 3, 5, 6, 7)):
        assert R.head_ids(flat, 5.0, .9, (k + .5) / 5, ok) == {want}
    hot = np.zeros(70, dtype=np.float32)
    hot[64] = 60.0
    for p in (1.0, .9):
        for u in (0.0, .5, R.JUST_BELOW_1):
            assert R.head_ids(hot, 1.0, p, u) == {64}
    # the rules of one position: 8 heads of 10 classes (specials 4 .. 9), class 3 on top everywhere
    sizes, offs, pad = [10] * 8, list(range(0, 81, 10)), [4] * 8
    row = np.tile(F32([0, 1, 2, 9, -50, -50, -50, -50, -50, -50]), 8)
    T, P, u = F32([1] * 8), F32([1, 1, 1, .9, .9, 1, 1, .9]), [.5] * 8
    assert R.position(row, sizes, offs, T, P, u, pad)[0] == [{3}] * 8
    words = np.asarray([0xffffffff] * 3, dtype=np.uint32)
    for h in range(8):                                             # a mask without the top class of any head
        c = 10 * h + 3
        words[c >> 5] &= np.uint32(~(1 << (c & 31)) & 0xffffffff)
    assert R.position(row, sizes, offs, T, P, u, pad, allow=words)[0] == [{2}] * 8
    # a floor over the top class of head 0: the specials stay free, PAD (-50, first of the equal ones) is the largest that is left
    sets, logged = R.position(row, sizes, offs, T, P, u, pad, order=(0, 8, 8))       # prev is a special row: only the floor counts
    assert logged and sets == [{3}] * 8
    sets, _ = R.position(row, sizes, offs, T, P, u, pad, order=(4, 1, 2))
    assert sets[0] == {4} and R.done_flag(sets, pad, 4) is True
    # head 1's second pass: b0 == prev0 = 3 and prev1 = 3 keeps class 3; prev1 = 2 as well; a given head 0 breaks it; a given head 1 stays
    assert R.position(row, sizes, offs, T, P, u, pad, order=(0, 3, 3))[0][1] == {3}
    low = row.copy()
    low[13] = -50                                                  # head 1 without its top: class 2 leads, the second pass from 3 on leaves 3 .. 9 equal
    assert R.position(low, sizes, offs, T, P, u, pad, order=(0, 2, 1))[0][1] == {2}       # b0 = 3 != prev0: no second pass
    assert R.position(low, sizes, offs, T, P, u, pad, order=(0, 3, 3))[0][1] == {3}
    assert R.position(low, sizes, offs, T, P, u, pad, order=(0, 3, 3), given=[2] + [-1] * 7)[0][:2] == [{2}, {2}]
    assert R.position(low, sizes, offs, T, P, u, pad, order=(0, 2, 3), given=[2] + [-1] * 7)[0][:2] == [{2}, {3}]
    assert R.position(low, sizes, offs, T, P, u, pad, order=(0, 3, 3), given=[-1, 0] + [-1] * 6)[0][:2] == [{3}, {0}]
    sets, logged = R.position(low, sizes, offs, T, P, u, pad, given=[1, 2, 3, 0, 1, 2, 3, 5])
    assert not logged and sets == [{1}, {2}, {3}, {0}, {1}, {2}, {3}, {5}] and R.done_flag(sets, pad, 4) is True
    assert R.done_flag([{1}] * 8, pad, 4) is False and R.done_flag([{1}] * 8, pad, 1) is True and R.done_flag([{1, 5}] + [{1}] * 7, pad, 4) is None


def test_the_tables_hold_the_planned_settings_and_edges():
    assert set(R.SETTINGS) >= {'default', 'ranked-01', 'all-1', 'all-.9', 'cold', 'edge-narrow', 'edge-wide', 'edge-wide-1088'}
    forms = {R.SETTINGS[k][3] for k in R.SETTINGS}
    graphs = {R.SETTINGS[k][4] for k in R.SETTINGS}
    assert forms == {'narrow', 'wide'} and graphs == {0, 1}
    n, offs, pad, vocab = R.layout(R.D_EDGE_NARROW)
    assert vocab == 1341 and vocab % 32 == 29 and sum(s for s, p in zip(R.D_EDGE_NARROW, R.P_DEFAULT) if p < 1) == 512
    assert R.layout(R.D_DEFAULT)[3] == 1280 and max(R.D_EDGE_WIDE) == 1088 and len(R.PLAN) + R.EXTRA <= R.S
    for d in R.DICTS.values():
        masks = R.masks_for(d)
        n, offs, pad, vocab = R.layout(d)
        for m in range(4):
            for h in range(8):
                ok = R.allowed_bits(masks[m], offs[h], n[h])
                assert ok[pad[h]:].all(), (m, h)                    # every mask keeps the special ids
        assert masks[:, -1].max() < (1 << (vocab % 32 or 32))       # no bit behind the vocabulary
    c = R.case('edge-wide-1088')
    plateau = [i for i, k in enumerate(c['kinds']) if k == 'plateau']
    tied = sorted({int((c['logits'][i][:1088] == 0).sum()) for i in plateau})
    assert tied == [18, 19, 37, 38], tied                          # kc - 1 = K - 1, K, 2K - 1, 2K at K = 17


# ---------------------------------------------------------------------------------------------------------------- the host sampler
class _Draws:
    def __init__(self, u):
        self.u = np.asarray(u, dtype=np.float64)

    def random_sample(self, n):
        assert n == 8
        return self.u.copy()


def test_reference_against_the_host_sampler():
    from pianobart_amd.model import PianoBartLM
    c = R.case('default')
    assert list(c['T']) == list(F32(PianoBartLM.SAMPLE_T)) and list(c['P']) == list(F32(PianoBartLM.SAMPLE_P))
    rows = [i for i, k in enumerate(c['kinds']) if k == 'random']
    masks = R.masks_for(R.D_DEFAULT)
    checked = ties = undecided = 0
    for i in rows:
        row = c['logits'][i]
        for r in range(B_ROWS):
            u = c['U'][r, i]
            mode = r % 3
            words = masks[r % 2] if mode == 2 else None
            order = (int(63 + r), int(40 + 7 * r), int(3 * r)) if mode == 1 else None
            allow = np.concatenate([R.allowed_bits(words, c['offs'][h], c['sizes'][h]) for h in range(8)]) if words is not None else None
            for given0 in ((-1, 40 + 7 * r) if mode == 1 else (-1,)):
                given = [given0] + [-1] * 7
                sets, _ = R.position(row, c['sizes'], c['offs'], c['T'], c['P'], u, c['pad'], allow=words, order=order, given=given)
                kw = {}
                if order is not None:
                    low0 = max(order[0], order[1])
                    kw['order'] = (low0, order[1], order[2], given0)
                if allow is not None:
                    kw['allow'] = allow
                got = PianoBartLM.sample_row(PianoBartLM, torch.from_numpy(row.copy()), _Draws(u), **kw).tolist()
                for h in range(1 if given0 >= 0 else 0, 8):
                    if _host_tie(row, c, h, sets, allow, order, got[0] if given0 < 0 else given0):
                        ties += 1
                        continue
                    if len(sets[h]) > 1:
                        undecided += 1
                        assert got[h] in sets[h], (i, r, h, got[h], sets[h])
                        continue
                    checked += 1
                    assert {got[h]} == sets[h], (i, r, h, got[h], sets[h], kw.get('order'))
    print('host sampler: %d heads equal, %d undecided, %d skipped for bit-equal candidate probabilities' % (checked, undecided, ties))
    assert checked > 3000 and ties < 50


B_ROWS = 16


def _host_tie(row, c, h, sets, allow, order, b0):
    """Two of the head's candidates have bit-equal f32 probabilities (torch's softmax, as the host computes them)."""
    n, off = int(c['sizes'][h]), int(c['offs'][h])
    y = torch.from_numpy(row[off:off + n].copy()) / float(c['T'][h])
    ok = np.ones(n, dtype=bool) if allow is None else allow[off:off + n].copy()
    if order is not None:
        if h == 0:
            ok &= np.arange(n) >= max(order[0], order[1])
        if h == 1 and order[2] > 0 and b0 == order[1]:
            ok &= np.arange(n) >= order[2]
    y[torch.from_numpy(~ok)] = -np.inf
    pr = torch.softmax(y, dim=-1).numpy()
    kc, srt, _ = R.free_kc(row[off:off + n], float(c['T'][h]), float(np.float32(c['P'][h])), ok)
    cand = pr[srt[:kc + 1]] if c['P'][h] < 1 else np.sort(pr)[-2:]
    return len(np.unique(cand)) < len(cand)


# ---------------------------------------------------------------------------------------------------------------- the caps
def shares(c, toks=None, rows_form=True):
    """(crafted undecided, crafted total, random undecided, random total, the undecided crafted places) over the rows' chains."""
    cu = ct = ru = rt = 0
    where = []
    for r in range(len(c['rules'])):
        for i, sets, logged, done in R.follow(c, r, None if toks is None else toks[r], rows_form):
            und = sum(len(s) > 1 for s in sets)
            if c['kinds'][i] == 'random':
                ru, rt = ru + und, rt + 8
            else:
                cu, ct = cu + und, ct + 8
                if und:
                    where.append((r, i, c['kinds'][i], [h for h in range(8) if len(sets[h]) > 1]))
    return cu, ct, ru, rt, where


@pytest.mark.parametrize('name', list(R.SETTINGS))
def test_cases_are_decided(name):
    c = R.case(name)
    cu, ct, ru, rt, where = shares(c)
    print('sampler cases %-15s crafted %d of %d undecided, random %d of %d (%.2f %%)' % (name, cu, ct, ru, rt, 100.0 * ru / max(rt, 1)))
    assert cu == 0, where[:8]
    assert ru <= .05 * rt
    assert (ct > 1000 or name == 'exact-cut') and rt > 1000                                 # the rows live long enough to meet the cases


def test_cases_of_the_single_row_form_are_decided():
    for name in ('default', 'edge-wide-1088'):
        c = R.case(name, b1=True)
        cu, ct, ru, rt, where = shares(c, rows_form=False)
        print('sampler cases %-15s B = 1: crafted %d of %d undecided, random %d of %d' % (name, cu, ct, ru, rt))
        assert cu == 0, where[:8]
        assert ru <= .05 * rt
