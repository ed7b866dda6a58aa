"""GPU: bar schedules in dec_sample_kernel (csrc/pb_decode.hip), the sampler alone, position by position, against the float64 nucleus rule
of tests/sampler_ref.py -- driven through pb_batch_decoder_* on planted logits in the manner of tests/test_sampler_kernel_gpu.py (its model
with a zero LM-head weight, its decoder set-up and its NaN / -7 prefilled logs are imported, not copied).

The planted rows put a 60.0 peak on ONE bar of head 0 per position (p = 1: the arg-max, decided) and random logits under heads 1 .. 7, so the
bar sequence is known -- 0 0 1 1 2 2 2 7 7 8 9 9 last last last EOS -- and what the schedule does to heads 1 .. 7 is judged on non-trivial
heads. Two schedule tables over the masks of sampler_ref.masks_for ('notop', 'alternating', 'oneclass': ONE ordinary class per head):
  schedule 0   bar 0 -> 0, 1 -> 1, 2 -> 2, 3 -> 1, 7 -> none, 8 -> 0, 9 -> 0, last -> 1        schedule 1   0 -> 1, 1 -> 1, 2 -> 0, 3 -> 2, 7 -> 2, 9 -> 1, last -> 2
so the guess (the entry of the decoder input's bar) is right inside a bar and at 0 -> 1 of schedule 1 and 8 -> 9 of schedule 0, wrong at the
other bar changes, and the entry is the row's own mask in bars 7 (schedule 0) and 8 (schedule 1). The 16 rows: free and row-mask-only
controls; schedules with and without a row mask; time-ordered rows (head 1's pass inside a bar, the schedule's pass at a bar change, both
with a floor that moves head 0); given bars arange(S) // 4, a given last bar (wrong guess behind the SOS row), a given special bar (the row
ends; the guess stands), a given pitch outside the bar's mask, a given head 1, all 8 heads given, and a stop bar. B = 16 with the force
table and, for the rows without given ids, without it; B = 1 one rule per run; the narrow sampler on the default dictionary and the wide
one (K = 17) on sampler_ref's 'edge-wide' dictionary, whose last bar id is 1081.

Assertions, none with a tolerance: every (row, position, head) holds an id the reference accepts for the bar the device itself wrote; at
most 5 % of the judged heads are undecided; the cases above occur (counted from the tables, not from the device); finished rows stay
finished."""
import ctypes

import numpy as np
import pytest
import torch

from tests import sampler_ref as R
from tests.test_sampler_kernel_gpu import SENT, _bits, _decoder, _model

pytestmark = pytest.mark.gpu
S = R.S
NPOS = 16
_CASES = {}


def _case(dname):
    """The planted rows, draws, masks, schedule tables and the 16 rows' rules of one dictionary."""
    if dname in _CASES:
        return _CASES[dname]
    sizes = R.DICTS[dname]
    n, offs, pad, vocab = R.layout(sizes)
    pad0, last = int(pad[0]), int(pad[0]) - 1
    T, P = np.asarray(R.T_DEFAULT, dtype=np.float32), np.asarray(R.P_DEFAULT, dtype=np.float32)
    rng = np.random.RandomState(77 + len(dname))
    bars = [0, 0, 1, 1, 2, 2, 2, 7, 7, 8, 9, 9, last, last, last, pad0 + 3]
    assert len(bars) == NPOS
    logits = np.zeros((NPOS, vocab), dtype=np.float32)
    for i, bar in enumerate(bars):
        logits[i, bar] = 60.0                                          # head 0 starts at column 0
        for h in range(1, 8):
            lg = (rng.standard_normal(int(n[h])) * 3.0).astype(np.float32)
            lg[int(pad[h]):] -= np.float32(40.0 * T[h])                # no special id under heads 1 .. 7: the rows live
            logits[i, offs[h]:offs[h + 1]] = lg
    stab = np.full((2, pad0), -1, dtype=np.int32)
    for k, e in ((0, 0), (1, 1), (2, 2), (3, 1), (8, 0), (9, 0), (last, 1)):
        stab[0, k] = e
    for k, e in ((0, 1), (1, 1), (2, 0), (3, 2), (7, 2), (9, 1), (last, 2)):
        stab[1, k] = e
    rows = [dict(floor=-1, stop=pad0, mask=-1, sched=-1, given=np.full((S, 8), -1, dtype=np.int16)) for _ in range(R.B)]
    for r, kw in ((1, dict(sched=0)), (2, dict(sched=1)), (3, dict(sched=0, mask=1)), (4, dict(sched=0, floor=0)), (5, dict(sched=1, floor=0, mask=0)),
                  (6, dict(sched=0)), (7, dict(sched=0)), (8, dict(sched=0)), (9, dict(sched=0)), (10, dict(sched=1, stop=8)), (11, dict(mask=2)),
                  (12, dict(sched=0, floor=0)), (13, dict(sched=1, floor=2)), (14, dict(sched=0)), (15, dict(floor=0))):
        rows[r].update(kw)
    rows[6]['given'][:, 0] = np.arange(S) // 4                         # the mask changes every 4 positions, whatever head 0 samples
    rows[7]['given'][:, 0] = last                                      # the last ordinary bar id, from the SOS row on
    rows[8]['given'][6, 0] = pad0 + 3                                  # a given special bar: the guess stands, the row ends
    rows[9]['given'][:, 3] = 1                                         # a given pitch that 'alternating' and 'oneclass' remove
    rows[12]['given'][1::2, 1] = 5                                     # a given head 1: no time-ordered pass there
    for i in (3, 4):
        rows[14]['given'][i] = [(i + 11 * h) % int(pad[h]) for h in range(8)]
    c = dict(sizes=n, offs=offs, pad=pad, vocab=vocab, T=T, P=P, form=R.form_of(sizes, P), logits=logits, U=rng.random_sample((R.B, S, 8)), rules=rows,
             masks=R.masks_for(sizes), stab=stab, sos=pad + 2, bars=bars)
    _CASES[dname] = c
    return c


def _entry(c, rule, bar):
    """The index of the mask heads 1 .. 7 take in a token of `bar` under the rule (-1: every class), and whether the schedule named it."""
    if rule['sched'] >= 0 and 0 <= bar < int(c['pad'][0]) and c['stab'][rule['sched'], bar] >= 0:
        return int(c['stab'][rule['sched'], bar])
    return rule['mask']


def _position(c, rule, i, prev, logits, chosen0):
    """One position of one row under the bar-schedule contract: 8 sets of acceptable ids and whether the position logs its logits row."""
    given = [int(v) for v in rule['given'][i]]
    if all(v >= 0 for v in given):
        return [{v} for v in given], False
    sizes, offs, pad, u8 = c['sizes'], c['offs'], c['pad'], c['U'][rule['row'], i]
    own = c['masks'][rule['mask']] if rule['mask'] >= 0 else None
    low0 = low1 = 0
    prev0 = -1
    if rule['floor'] >= 0:
        bar = prev[0] < pad[0]
        low0 = max(rule['floor'], prev[0] if bar else 0)
        if bar and prev[1] < pad[1]:
            low1, prev0 = prev[1], prev[0]
    n0 = int(sizes[0])
    ok0 = R.allowed_bits(own, 0, n0) if own is not None else np.ones(n0, dtype=bool)
    sets = [R.head_ids(logits[:n0], c['T'][0], c['P'][0], u8[0], ok0 & (np.arange(n0) >= low0))] + [set() for _ in range(7)]
    b0s = {given[0]} if given[0] >= 0 else ({int(chosen0)} if int(chosen0) in sets[0] else sets[0])
    for b0 in b0s:                                                     # head 0's id after forcing picks the mask of heads 1 .. 7
        # a special b0 ends the row and its token is never written: the device keeps the mask it guessed (the entry of the decoder
        # input's bar, entry 0 behind a special one) in place of a second pass, and that is what its log holds
        e = _entry(c, rule, b0) if b0 < pad[0] else _entry(c, rule, prev[0] if prev[0] < pad[0] else 0)
        for h in range(1, 8):
            n, off = int(sizes[h]), int(offs[h])
            ok = R.allowed_bits(c['masks'][e], off, n) if e >= 0 else np.ones(n, dtype=bool)
            if h == 1 and low1 > 0 and given[1] < 0 and b0 == prev0:
                ok = ok & (np.arange(n) >= low1)
            sets[h] |= R.head_ids(logits[off:off + n], c['T'][h], c['P'][h], u8[h], ok)
    for h in range(8):
        if given[h] >= 0:
            sets[h] = {given[h]}
    return sets, True


def _run(eng, enc, emask, c, rows, use_graph):
    """NPOS positions (and R.EXTRA further steps) on the device for the given rows of the case; returns copies of the logs."""
    from pianobart_amd._lib import LIB
    n, vocab = len(rows), c['vocab']
    rules = [c['rules'][r] for r in rows]
    head_b = eng.wf['head.b']
    assert head_b.dtype == torch.float32 and head_b.numel() == vocab and not bool(eng.w['head.w'].any())
    bias = torch.from_numpy(c['logits']).cuda()
    with torch.no_grad(), _decoder(eng, enc, emask, n, use_graph) as (dec, _, _):
        U = np.ascontiguousarray(c['U'][rows].reshape(n, S * 8))
        n8, off8, pad8 = (np.ascontiguousarray(v, dtype=np.int32) for v in (c['sizes'], c['offs'][:8], c['pad']))
        LIB.call('pb_batch_decoder_sampler_init', dec, c['T'].ctypes.data, c['P'].ctypes.data, n8.ctypes.data, off8.ctypes.data, pad8.ctypes.data,
                 U.ctypes.data, n * S * 8, S, -1, 0)
        assert int(LIB.query('pb_batch_decoder_sampler_form', dec)) == (1 if c['form'] == 'wide' else 0)
        forced = np.ascontiguousarray(np.stack([r['given'] for r in rules]), dtype=np.int16)
        if (forced >= 0).any():
            LIB.call('pb_batch_decoder_force', dec, forced.ctypes.data)
        per_row = {key: np.asarray([r[key] for r in rules], dtype=np.int32) for key in ('stop', 'floor', 'mask', 'sched')}      # held while the calls read them
        LIB.call('pb_batch_decoder_stop', dec, per_row['stop'].ctypes.data)
        LIB.call('pb_batch_decoder_order', dec, per_row['floor'].ctypes.data)
        masks = np.ascontiguousarray(c['masks'], dtype=np.uint32)
        LIB.call('pb_batch_decoder_allow', dec, masks.ctypes.data, masks.shape[0], masks.shape[1], per_row['mask'].ctypes.data)
        stab = np.ascontiguousarray(c['stab'], dtype=np.int32)
        LIB.call('pb_batch_decoder_schedule', dec, stab.ctypes.data, stab.shape[0], stab.shape[1], per_row['sched'].ctypes.data)
        lp, tp = ctypes.c_void_p(), ctypes.c_void_p()
        LIB.call('pb_batch_decoder_logs', dec, ctypes.byref(lp), ctypes.byref(tp))
        logits = np.ctypeslib.as_array((ctypes.c_float * (n * S * vocab)).from_address(lp.value)).reshape(n, S, vocab)
        tok = np.ctypeslib.as_array((ctypes.c_int16 * (n * S * 8)).from_address(tp.value)).reshape(n, S, 8)
        logits[:] = np.nan
        tok[:] = SENT
        first = np.ascontiguousarray(np.tile(c['sos'].astype(np.int16), (n, 1)))
        last_pos, lim = np.full(n, -1, dtype=np.int32), np.full(n, S, dtype=np.int32)
        LIB.call('pb_batch_decoder_start', dec, last_pos.ctypes.data, first.ctypes.data, lim.ctypes.data)
        for i in range(NPOS + R.EXTRA):
            if i < NPOS:
                head_b.copy_(bias[i])
            torch.cuda.synchronize()
            tk = int(LIB.query('pb_batch_decoder_launch', dec, 1, None))
            assert tk >= 0, LIB.load().pb_last_error().decode()
            LIB.call('pb_batch_decoder_wait', dec, tk)
        assert bool(LIB.query('pb_batch_decoder_graph', dec)) == bool(use_graph)
        return logits.copy(), tok.copy()


def _judge(c, rows, logits, tok, rows_form):
    """Every (row, position, head) against the reference, each row followed on the ids the device wrote. Returns (failures, undecided heads,
    judged heads, tally): tally counts, over scheduled rows, the positions whose guess was wrong / right at a bar change, whose b0 was
    given, special or without an entry, that took head 1's time-ordered pass, and that sampled under 'oneclass' or in the last bar."""
    fails, und, tot = [], 0, 0
    tally = dict(wrong=0, right_change=0, given0=0, special=0, no_entry=0, head1=0, oneclass=0, last=0)
    pad0 = int(c['pad'][0])
    for k, r in enumerate(rows):
        rule = dict(c['rules'][r], row=r)
        prev = [int(v) for v in c['sos']]
        end = None
        for i in range(NPOS):
            if (tok[k, i] == SENT).all():
                fails.append((r, i, 'no ids written: the row ended early'))
                end = i - 1
                break
            sets, logged = _position(c, rule, i, prev, c['logits'][i], tok[k, i, 0])
            if logged and not np.array_equal(_bits(logits[k, i]), _bits(c['logits'][i])):
                fails.append((r, i, 'the logged row is not the bias row'))
                end = i
                break
            if not logged and not np.isnan(logits[k, i]).all():
                fails.append((r, i, 'a position with all 8 heads given logged a logits row'))
            ids = [int(v) for v in tok[k, i]]
            for h in range(8):
                if ids[h] not in sets[h]:
                    fails.append((r, i, 'head %d: %d, acceptable %s' % (h, ids[h], sorted(sets[h])[:6])))
                und, tot = und + (len(sets[h]) > 1), tot + 1
            if rule['sched'] >= 0 and logged:
                b0, p0 = ids[0], prev[0]
                guess = _entry(c, rule, p0 if p0 < pad0 else 0)
                want = _entry(c, rule, b0) if b0 < pad0 else guess
                tally['wrong'] += want != guess
                tally['right_change'] += want == guess and b0 != p0 and b0 < pad0 and p0 < pad0
                tally['given0'] += rule['given'][i][0] >= 0
                tally['special'] += b0 >= pad0
                tally['no_entry'] += b0 < pad0 and c['stab'][rule['sched'], b0] < 0
                tally['head1'] += rule['floor'] >= 0 and p0 < pad0 and prev[1] < c['pad'][1] and b0 == p0 and rule['given'][i][1] < 0 and prev[1] > 0
                tally['oneclass'] += want == 2
                tally['last'] += b0 == pad0 - 1
            done = R.done_of(ids, c['pad'], rule['stop'])
            if done and rows_form:
                end = i
                break
            prev = ids
        last = end if end is not None else NPOS + R.EXTRA - 1
        if end is None and not (tok[k, :last + 1] != SENT).all():
            fails.append((r, last, 'a live row has untouched id log rows'))
        if not ((tok[k, last + 1:] == SENT).all() and np.isnan(logits[k, last + 1:]).all()):
            fails.append((r, last, 'log rows were written behind the position that ended the row'))
    return fails, und, tot, tally


@pytest.mark.parametrize('dname,use_graph', [('default', 1), ('edge-wide', 0)])
def test_scheduled_rows_against_float64(dname, use_graph):
    """B = 16: the force table's kernels, then the rows without given ids alone (the unforced kernels)."""
    c = _case(dname)
    m, eng, enc, emask = _model(dname)
    rows = list(range(R.B))
    logits, tok = _run(eng, enc, emask, c, rows, use_graph)
    fails, und, tot, tally = _judge(c, rows, logits, tok, True)
    print('bar schedule kernel %-9s %s forced: %d of %d heads undecided; %s; %d wrong' % (dname, c['form'], und, tot, tally, len(fails)))
    assert not fails, (len(fails), sorted({f[:2] for f in fails})[:40], fails[:12])
    assert und <= .05 * tot and tot > 1200
    # both passes are taken, and every case of the list occurs
    assert tally['wrong'] >= 30 and tally['right_change'] >= 4 and tally['given0'] >= 25 and tally['special'] >= 3 and tally['no_entry'] >= 10
    assert tally['head1'] >= 8 and tally['oneclass'] >= 15 and tally['last'] >= 20
    # a schedule changes what heads 1 .. 7 hold: row 1 (schedule 0) against row 0 (free) on the same draws would be equal only by accident
    free = [r for r in rows if not (c['rules'][r]['given'] >= 0).any()]
    assert len(free) >= 9 and sum(c['rules'][r]['sched'] >= 0 for r in free) >= 6
    logits, tok = _run(eng, enc, emask, c, free, 1 - use_graph)
    fails, und, tot, tally = _judge(c, free, logits, tok, True)
    print('bar schedule kernel %-9s %s unforced: %d of %d heads undecided; %s; %d wrong' % (dname, c['form'], und, tot, tally, len(fails)))
    assert not fails, (len(fails), sorted({f[:2] for f in fails})[:40], fails[:12])
    assert und <= .05 * tot and tally['wrong'] >= 20 and tally['right_change'] >= 3 and tally['head1'] >= 8 and tally['special'] >= 3


@pytest.mark.parametrize('dname,use_graph', [('default', 0), ('edge-wide', 1)])
def test_single_row_form_against_float64(dname, use_graph):
    """B = 1 (the kernels without a done flag): a scheduled row, an ordered one with a row mask, given bars, the given last bar."""
    c = _case(dname)
    m, eng, enc, emask = _model(dname)
    fails, und, tot = [], 0, 0
    total = dict()
    for r in (1, 5, 6, 7, 13):                                         # 1, 5, 13: no force table; 6, 7: with one
        logits, tok = _run(eng, enc, emask, c, [r], use_graph)
        f, u, t, tally = _judge(c, [r], logits, tok, False)
        fails += f
        und, tot = und + u, tot + t
        for k, v in tally.items():
            total[k] = total.get(k, 0) + int(v)
    print('bar schedule kernel %-9s B = 1, %s: %d of %d heads undecided; %s; %d wrong' % (dname, c['form'], und, tot, total, len(fails)))
    assert not fails, (len(fails), sorted({f[:2] for f in fails})[:40], fails[:12])
    assert und <= .05 * tot and total['wrong'] >= 12 and total['head1'] >= 4 and total['given0'] >= 20 and total['last'] >= 10


def test_refusals_leave_the_decoder_working():
    """Every refusal of the two entry points by name; nothing changes, and the run that follows is the scheduled one."""
    from pianobart_amd._lib import LIB
    c = _case('default')
    m, eng, enc, emask = _model('default')
    dll = LIB.load()
    err = lambda: dll.pb_last_error().decode()
    stab = np.ascontiguousarray(c['stab'], dtype=np.int32)
    idx, own, bad_idx = np.asarray([0, 1], dtype=np.int32), np.asarray([-1, 1], dtype=np.int32), np.asarray([0, 2], dtype=np.int32)
    last_pos, lim = np.full(2, -1, dtype=np.int32), np.full(2, S, dtype=np.int32)      # every array outlives the call it is passed to
    masks = np.ascontiguousarray(c['masks'], dtype=np.uint32)
    with torch.no_grad(), _decoder(eng, enc, emask, 2, 1) as (dec, _, _):
        d = dec
        call = lambda *a: dll.pb_batch_decoder_schedule(d, *a)
        assert call(stab.ctypes.data, 2, 256, idx.ctypes.data) < 0 and 'sampler_init first' in err()
        assert dll.pb_batch_decoder_admit_schedule(d, 0, 0) < 0 and 'not a dynamic decoder' in err()
        U = np.ascontiguousarray(c['U'][:2].reshape(2, S * 8))
        n8, off8, pad8 = (np.ascontiguousarray(v, dtype=np.int32) for v in (c['sizes'], c['offs'][:8], c['pad']))
        LIB.call('pb_batch_decoder_sampler_init', dec, c['T'].ctypes.data, c['P'].ctypes.data, n8.ctypes.data, off8.ctypes.data, pad8.ctypes.data,
                 U.ctypes.data, 2 * S * 8, S, -1, 0)
        assert call(None, 2, 256, idx.ctypes.data) < 0 and 'null argument' in err()
        assert call(stab.ctypes.data, 2, 256, None) < 0 and 'null argument' in err()
        assert call(stab.ctypes.data, 2, 256, idx.ctypes.data) < 0 and 'mask index 0 outside -1..-1' in err()      # no mask table yet: an entry >= 0 points nowhere
        LIB.call('pb_batch_decoder_allow', dec, masks.ctypes.data, masks.shape[0], masks.shape[1], own.ctypes.data)
        assert call(stab.ctypes.data, 2, 255, idx.ctypes.data) < 0 and '255 entries per schedule for 256' in err()
        assert call(stab.ctypes.data, 0, 256, idx.ctypes.data) < 0 and '0 schedules' in err()
        bad = stab.copy()
        bad[1, 200] = 4
        assert call(bad.ctypes.data, 2, 256, idx.ctypes.data) < 0 and 'schedule 1, bar 200: mask index 4 outside -1..3' in err()
        bad[1, 200] = -2
        assert call(bad.ctypes.data, 2, 256, idx.ctypes.data) < 0 and 'mask index -2' in err()
        assert call(stab.ctypes.data, 2, 256, bad_idx.ctypes.data) < 0 and 'row 1: schedule index 2 outside -1..1' in err()
        LIB.call('pb_batch_decoder_schedule', dec, stab.ctypes.data, 2, 256, idx.ctypes.data)
        assert dll.pb_batch_decoder_allow(d, masks.ctypes.data, masks.shape[0], masks.shape[1], idx.ctypes.data) < 0 and 'bar schedule points into the table' in err()
        first = np.ascontiguousarray(np.tile(c['sos'].astype(np.int16), (2, 1)))
        LIB.call('pb_batch_decoder_start', dec, last_pos.ctypes.data, first.ctypes.data, lim.ctypes.data)
        eng.wf['head.b'].copy_(torch.from_numpy(c['logits'][0]).cuda())
        torch.cuda.synchronize()
        tk = int(LIB.query('pb_batch_decoder_launch', dec, 1, None))
        assert tk >= 0, err()
        LIB.call('pb_batch_decoder_wait', dec, tk)
        assert call(stab.ctypes.data, 2, 256, idx.ctypes.data) < 0 and 'a step was already issued' in err()
        lp, tp = ctypes.c_void_p(), ctypes.c_void_p()
        LIB.call('pb_batch_decoder_logs', dec, ctypes.byref(lp), ctypes.byref(tp))
        tok = np.ctypeslib.as_array((ctypes.c_int16 * (2 * S * 8)).from_address(tp.value)).reshape(2, S, 8)
        for k, rule in enumerate((dict(floor=-1, stop=256, mask=-1, sched=0), dict(floor=-1, stop=256, mask=1, sched=1))):
            rule.update(row=k, given=np.full((S, 8), -1, dtype=np.int16))
            sets, _ = _position(c, rule, 0, [int(v) for v in c['sos']], c['logits'][0], tok[k, 0, 0])
            assert all(int(tok[k, 0, h]) in sets[h] for h in range(8)), (k, tok[k, 0], sets)
