"""GPU: anchored notes in dec_sample_kernel (csrc/pb_decode.hip), the sampler alone, position by position, against the float64 nucleus rule
of tests/sampler_ref.py -- driven through pb_batch_decoder_* on planted logits in the manner of tests/test_bar_schedule_kernel_gpu.py (the
model with a zero LM-head weight, the decoder set-up and the NaN / -7 prefilled logs of tests/test_sampler_kernel_gpu.py and the
schedule-aware position rule of tests/test_bar_schedule_kernel_gpu.py are imported, not copied).

The planted rows put a 60.0 peak on ONE bar of head 0 and ONE position of head 1 per decoder position (both p = 1: the arg-max, decided), so
the candidate's time is known, and N(0, 3^2) logits under heads 2 .. 7 with the special ids pushed down. The candidate times (CAND) are
non-decreasing, with an EOS candidate at position 10 and another at 19 (and at the further steps): no time-order mask ever removes a peak,
because an anchor is only written where its time is at or below the candidate's, or where the candidate ends the row -- and the one
anchor an ending candidate lets through at position 10 is planned at or below the next candidate's time (8, 5).

The 16 rows (RULES) make every case of the contract occur; which cases occur is counted from the TABLES (_table: the rule walked over
CAND alone), never from the device: free and ordered controls; an anchor tying the first candidate; one strictly between two
candidates; three at one time; one in a later bar at a lower position; anchors left at the EOS candidate; anchors left at a stop-bar
candidate; a position limit reached with an anchor unplaced; an anchor whose pitch the row's mask removes; anchored rows under a bar
schedule; an anchor identical to its candidate; anchors in front of the first candidate; eight anchors along the whole row.

Assertions, none with a tolerance: every written token is the anchor the table expects, all 8 heads, or all its heads lie in the
reference's acceptable sets for the `prev` the device itself wrote; heads 0 and 1 of every candidate are decided and equal CAND, and no
head 2 .. 7 of a candidate that decides an anchor holds an acceptable special id (no anchor decision is undecided); at most 5 % of the
judged heads 2 .. 7 are undecided; pb_batch_decoder_anchors_placed equals the table's count; finished rows stay finished. B = 16 with and
without the graph, B = 1 one rule per run (the kernels without a done flag), the narrow sampler on the default dictionary and the wide
one on 'edge-wide'."""
import ctypes

import numpy as np
import pytest
import torch

from tests import sampler_ref as R
from tests.test_bar_schedule_kernel_gpu import _position
from tests.test_sampler_kernel_gpu import SENT, _bits, _decoder, _model

pytestmark = pytest.mark.gpu
S = R.S
NPOS = 20
NSTEP = NPOS + R.EXTRA
EOS = -1                                                               # in CAND: the bar head's special id pad0 + 3
LAST = -2                                                              # ... and the dictionary's last ordinary bar id
CAND = [(0, 4), (0, 4), (0, 20), (1, 0), (1, 30), (2, 40), (3, 10), (3, 10), (4, 2), (4, 60), (EOS, 0),
        (8, 5), (8, 5), (9, 0), (9, 33), (LAST, 7), (LAST, 50), (LAST, 50), (LAST, 100), (EOS, 0)]
_CASES = {}


def _pack(bits):
    vocab = bits.shape[1]
    out = np.zeros((len(bits), (vocab + 31) // 32), dtype=np.uint32)
    for m in range(len(bits)):
        for c in np.flatnonzero(bits[m]):
            out[m, c >> 5] |= np.uint32(1) << np.uint32(c & 31)
    return out


def _case(dname):
    """The planted rows, draws, masks, schedule table and the 16 rows' rules of one dictionary."""
    if dname in _CASES:
        return _CASES[dname]
    sizes = R.DICTS[dname]
    n, offs, pad, vocab = R.layout(sizes)
    pad0, last = int(pad[0]), int(pad[0]) - 1
    T, P = np.asarray(R.T_DEFAULT, dtype=np.float32), np.asarray(R.P_DEFAULT, dtype=np.float32)
    rng = np.random.RandomState(311 + len(dname))
    cand = [(pad0 + 3 if b == EOS else last if b == LAST else b, p) for b, p in CAND]
    logits = np.zeros((NPOS, vocab), dtype=np.float32)
    for i, (bar, posn) in enumerate(cand):
        logits[i, offs[0] + bar] = 60.0
        logits[i, offs[1] + posn] = 60.0
        for h in range(2, 8):
            lg = (rng.standard_normal(int(n[h])) * 3.0).astype(np.float32)
            lg[int(pad[h]):] -= np.float32(40.0 * T[h])                # no special id under heads 2 .. 7
            logits[i, offs[h]:offs[h + 1]] = lg
    # masks: 0 = melodic pitches 60 .. only (a row's own mask), 1 = odd pitch ids, 2 = durations 0 .. 31; heads 0 and 1 stay whole
    bits = np.ones((3, vocab), dtype=bool)
    bits[0, offs[3]:offs[3] + 60] = False
    bits[1, offs[3]:offs[3] + int(pad[3]):2] = False
    bits[2, offs[4] + 32:offs[4] + int(pad[4])] = False
    stab = np.full((1, pad0), -1, dtype=np.int32)
    for k, e in ((0, 1), (1, 2), (3, 1), (8, 2), (last, 1)):
        stab[0, k] = e
    U = rng.random_sample((R.B, S, 8))
    tok = lambda bar, posn, salt: [bar, posn] + [(7 * salt + 3 * h) % int(pad[h]) for h in range(2, 8)]
    rows = [dict(floor=0, stop=pad0, mask=-1, sched=-1, lim=S, anchors=[], given=np.full((S, 8), -1, dtype=np.int16)) for _ in range(R.B)]
    rows[0].update(floor=-1)                                           # the free control; row 1: the ordered control
    rows[2].update(anchors=[tok(0, 4, 1)])                             # ties the first candidate: written at position 0, behind the SOS row
    rows[3].update(anchors=[tok(1, 12, 2)])                            # strictly between (1, 0) and (1, 30)
    rows[4].update(anchors=[tok(2, 8, 3), tok(2, 8, 4), tok(2, 8, 5)])  # three at one time: positions 5, 6, 7
    rows[5].update(anchors=[tok(3, 5, 6)])                             # a later bar, a lower position than (2, 40): position 6, not 5
    rows[6].update(anchors=[tok(5, 3, 7), tok(6, 9, 8)])               # left at the EOS candidate: positions 10 and 11, the row ends at 19
    rows[7].update(stop=8, anchors=[tok(7, 1, 9), tok(7, 2, 10), tok(7, 3, 11)])        # EOS, then two stop-bar candidates; 'bar' at 13
    rows[8].update(lim=5, anchors=[tok(0, 20, 12), tok(6, 0, 13)])      # the limit comes with one anchor unplaced
    rows[9].update(mask=0, anchors=[tok(1, 0, 14)[:3] + [10] + tok(1, 0, 14)[4:], tok(3, 10, 15)[:3] + [59] + tok(3, 10, 15)[4:]])   # pitches the mask removes
    rows[10].update(sched=0, anchors=[tok(0, 10, 16), tok(1, 30, 17), tok(4, 0, 18)])
    rows[12].update(anchors=[tok(0, 4, 19), tok(0, 10, 20), tok(1, 30, 21), tok(3, 0, 22), tok(6, 0, 23), tok(8, 5, 24), tok(9, 10, 25), tok(last, 50, 26)])
    rows[13].update(anchors=[tok(0, 0, 27), tok(0, 1, 28)])            # in front of the first candidate: positions 0 and 1
    rows[14].update(stop=9, mask=0, anchors=[tok(2, 40, 29), tok(8, 0, 30)])
    rows[15].update(sched=0, mask=-1, anchors=[tok(0, 4, 31), tok(8, 2, 32), tok(last, 100, 33)])
    c = dict(sizes=n, offs=offs, pad=pad, vocab=vocab, T=T, P=P, form=R.form_of(sizes, P), logits=logits, U=U, rules=rows, masks=_pack(bits), stab=stab,
             sos=pad + 2, cand=cand)
    # row 11: an anchor identical to its candidate -- the reference's own ids of a position where all 8 heads are decided
    for i in (2, 3, 4, 5, 6, 8, 9):                                    # a candidate whose time differs from its predecessor's
        sets, _ = _position(c, dict(rows[11], row=11), i, list(cand[i - 1]) + [0] * 6, logits[i], -1)
        if all(len(s) == 1 for s in sets):
            rows[11].update(anchors=[[next(iter(s)) for s in sets]], same=i)
            break
    assert rows[11]['anchors'] and tuple(rows[11]['anchors'][0][:2]) == cand[rows[11]['same']] and cand[rows[11]['same']] != cand[rows[11]['same'] - 1]
    _CASES[dname] = c
    return c


def _ends(c, rule, c0, c1):
    return c0 >= rule['stop'] or c1 >= int(c['pad'][1])                # heads 2 .. 7 of a candidate are never special (checked on the device's rows)


def _table(c, rule, rows_form):
    """The rule walked over CAND alone: (what: per position ('anchor', j) or ('cand',), end: the position that ended the row or None,
    placed, tally)."""
    A, k, what, end = rule['anchors'], 0, [], None
    tally = dict(tie=0, between=0, by_end=0, by_stop=0, same_time=0, lower_pos=0)
    for i in range(NSTEP):
        if rows_form and i >= rule['lim']:
            end = i - 1
            break
        c0, c1 = c['cand'][min(i, NPOS - 1)]
        ends = _ends(c, rule, c0, c1)
        if k < len(A) and (ends or (c0, c1) >= (A[k][0], A[k][1])):
            tally['tie'] += (c0, c1) == (A[k][0], A[k][1])
            tally['between'] += not ends and (c0, c1) > (A[k][0], A[k][1])
            tally['by_end'] += c0 >= int(c['pad'][0])
            tally['by_stop'] += rule['stop'] <= c0 < int(c['pad'][0])
            tally['same_time'] += k > 0 and tuple(A[k][:2]) == tuple(A[k - 1][:2])
            tally['lower_pos'] += i > 0 and A[k][1] < c['cand'][i - 1][1] and A[k][0] > c['cand'][i - 1][0]
            what.append(('anchor', k))
            k += 1
            continue
        what.append(('cand',))
        if ends and rows_form:
            end = i
            break
    return what, end, k, tally


def _run(eng, enc, emask, c, rows, use_graph):
    """NSTEP steps on the device for the given rows of the case; returns copies of the logs and the device's counters."""
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
        per_row = {key: np.asarray([r[key] for r in rules], dtype=np.int32) for key in ('stop', 'floor', 'mask', 'sched')}      # held while the calls read them
        LIB.call('pb_batch_decoder_stop', dec, per_row['stop'].ctypes.data)
        LIB.call('pb_batch_decoder_order', dec, per_row['floor'].ctypes.data)
        masks = np.ascontiguousarray(c['masks'], dtype=np.uint32)
        LIB.call('pb_batch_decoder_allow', dec, masks.ctypes.data, masks.shape[0], masks.shape[1], per_row['mask'].ctypes.data)
        stab = np.ascontiguousarray(c['stab'], dtype=np.int32)
        LIB.call('pb_batch_decoder_schedule', dec, stab.ctypes.data, stab.shape[0], stab.shape[1], per_row['sched'].ctypes.data)
        cnt = np.asarray([len(r['anchors']) for r in rules], dtype=np.int32)
        base = np.asarray(np.concatenate([[0], np.cumsum(cnt)[:-1]]), dtype=np.int32)
        table = np.ascontiguousarray(np.asarray([a for r in rules for a in r['anchors']] or [[0] * 8], dtype=np.int16).reshape(-1, 8))
        LIB.call('pb_batch_decoder_anchor', dec, table.ctypes.data, table.shape[0], base.ctypes.data, cnt.ctypes.data)
        lp, tp = ctypes.c_void_p(), ctypes.c_void_p()
        LIB.call('pb_batch_decoder_logs', dec, ctypes.byref(lp), ctypes.byref(tp))
        logits = np.ctypeslib.as_array((ctypes.c_float * (n * S * vocab)).from_address(lp.value)).reshape(n, S, vocab)
        tok = np.ctypeslib.as_array((ctypes.c_int16 * (n * S * 8)).from_address(tp.value)).reshape(n, S, 8)
        logits[:] = np.nan
        tok[:] = SENT
        first = np.ascontiguousarray(np.tile(c['sos'].astype(np.int16), (n, 1)))
        last_pos, lim = np.full(n, -1, dtype=np.int32), np.asarray([r['lim'] for r in rules], dtype=np.int32)
        LIB.call('pb_batch_decoder_start', dec, last_pos.ctypes.data, first.ctypes.data, lim.ctypes.data)
        for i in range(NSTEP):
            if i < NPOS:
                head_b.copy_(bias[i])
            torch.cuda.synchronize()
            tk = int(LIB.query('pb_batch_decoder_launch', dec, 1, None))
            assert tk >= 0, LIB.load().pb_last_error().decode()
            LIB.call('pb_batch_decoder_wait', dec, tk)
        assert bool(LIB.query('pb_batch_decoder_graph', dec)) == bool(use_graph)
        placed = np.full(n, -1, dtype=np.int32)
        LIB.call('pb_batch_decoder_anchors_placed', dec, placed.ctypes.data)
        return logits.copy(), tok.copy(), placed


def _judge(c, rows, logits, tok, placed, rows_form):
    """Every (row, position, head) against the table and the reference, each row followed on the ids the device wrote. Returns (failures,
    undecided heads 2 .. 7, judged heads 2 .. 7)."""
    fails, und, tot = [], 0, 0
    pad = c['pad']
    for k, r in enumerate(rows):
        rule = dict(c['rules'][r], row=r)
        what, end, want_placed, _ = _table(c, rule, rows_form)
        if int(placed[k]) != want_placed:
            fails.append((r, -1, 'anchors_placed %d, the table says %d' % (int(placed[k]), want_placed)))
        prev = [int(v) for v in c['sos']]
        for i, w in enumerate(what):
            L = c['logits'][min(i, NPOS - 1)]
            if (tok[k, i] == SENT).all():
                fails.append((r, i, 'no ids written: the row ended early'))
                break
            if not np.array_equal(_bits(logits[k, i]), _bits(L)):
                fails.append((r, i, 'the logged row is not the bias row'))
                break
            sets, _ = _position(c, rule, i, prev, L, -1)
            ids = [int(v) for v in tok[k, i]]
            if [sorted(sets[0]), sorted(sets[1])] != [[c['cand'][min(i, NPOS - 1)][0]], [c['cand'][min(i, NPOS - 1)][1]]]:
                fails.append((r, i, 'the candidate\'s time is not decided as planted: %s %s' % (sorted(sets[0])[:4], sorted(sets[1])[:4])))
            if len(rule['anchors']) and any(v >= pad[h] for h in range(2, 8) for v in sets[h]):
                fails.append((r, i, 'an anchor decision is undecided: a special id is acceptable under heads 2 .. 7'))
            if w[0] == 'anchor':
                if ids != [int(v) for v in rule['anchors'][w[1]]]:
                    fails.append((r, i, 'anchor %d expected %s, written %s' % (w[1], rule['anchors'][w[1]], ids)))
            else:
                for h in range(8):
                    if ids[h] not in sets[h]:
                        fails.append((r, i, 'head %d: %d, acceptable %s' % (h, ids[h], sorted(sets[h])[:6])))
                    if h >= 2:
                        und, tot = und + (len(sets[h]) > 1), tot + 1
            prev = ids
        last = end if end is not None else NSTEP - 1
        if end is None and not (tok[k, :last + 1] != SENT).all():
            fails.append((r, last, 'a live row has untouched id log rows'))
        if not ((tok[k, last + 1:] == SENT).all() and np.isnan(logits[k, last + 1:]).all()):
            fails.append((r, last, 'log rows were written behind the position that ended the row'))
    return fails, und, tot


def test_tables_hold_every_case():
    """Counted from the tables: each case of the contract occurs among the 16 rows (no device result enters)."""
    for dname in ('default', 'edge-wide'):
        c = _case(dname)
        pad0 = int(c['pad'][0])
        t = {r: _table(c, c['rules'][r], True) for r in range(R.B)}
        assert all(a <= b for a, b in zip(c['cand'][:10], c['cand'][1:10])) and all(a <= b for a, b in zip(c['cand'][11:19], c['cand'][12:19]))
        assert c['cand'][10][0] >= pad0 and c['cand'][19][0] >= pad0
        assert t[0][1:3] == (10, 0) and t[1][1:3] == (10, 0)                                   # the controls end at the first EOS candidate
        assert t[2][0][0] == ('anchor', 0) and t[2][3]['tie'] == 1                              # behind the SOS row
        assert t[3][0][4] == ('anchor', 0) and t[3][3]['between'] == 1
        assert t[4][0][5:8] == [('anchor', 0), ('anchor', 1), ('anchor', 2)] and t[4][3]['same_time'] == 2
        assert t[5][0][5] == ('cand',) and t[5][0][6] == ('anchor', 0) and t[5][3]['lower_pos'] == 1
        assert t[6][0][10:12] == [('anchor', 0), ('anchor', 1)] and t[6][3]['by_end'] == 1 and t[6][1] == 19
        assert t[7][0][10:13] == [('anchor', 0), ('anchor', 1), ('anchor', 2)] and t[7][3]['by_stop'] == 2 and t[7][1] == 13
        assert t[8][1] == 4 and t[8][2] == 1 < len(c['rules'][8]['anchors'])                   # the limit, one anchor unplaced
        assert c['rules'][9]['mask'] == 0 and all(a[3] < 60 for a in c['rules'][9]['anchors']) and t[9][2] == 2
        assert c['rules'][10]['sched'] == 0 and t[10][2] == 3 and c['rules'][15]['sched'] == 0 and t[15][2] == 3
        assert t[11][0][c['rules'][11]['same']] == ('anchor', 0) and t[11][3]['tie'] == 1
        assert t[12][2] == 8 and t[12][1] == 19 and t[13][0][:2] == [('anchor', 0), ('anchor', 1)]
        assert t[14][2] == 2 and t[14][1] == 13
        for r in range(R.B):                                           # every anchor but row 8's last is written, and every row form row ends
            assert t[r][1] is not None and (r == 8 or t[r][2] == len(c['rules'][r]['anchors']))


@pytest.mark.parametrize('dname,use_graph', [('default', 1), ('edge-wide', 0)])
def test_anchored_rows_against_float64(dname, use_graph):
    """B = 16, with the graph and without it (the second run swaps the launch mode)."""
    c = _case(dname)
    m, eng, enc, emask = _model(dname)
    rows = list(range(R.B))
    for graph in (use_graph, 1 - use_graph):
        logits, tok, placed = _run(eng, enc, emask, c, rows, graph)
        fails, und, tot = _judge(c, rows, logits, tok, placed, True)
        print('anchor kernel %-9s %s graph %d: %d of %d heads 2 .. 7 undecided; placed %s; %d wrong' % (dname, c['form'], graph, und, tot, placed.tolist(), len(fails)))
        assert not fails, (len(fails), sorted({f[:2] for f in fails})[:40], fails[:12])
        assert und <= .05 * tot and tot > 800
        assert placed.tolist() == [_table(c, c['rules'][r], True)[2] for r in rows] and placed.sum() >= 30


@pytest.mark.parametrize('dname,use_graph', [('default', 0), ('edge-wide', 1)])
def test_single_row_form_against_float64(dname, use_graph):
    """B = 1 (the kernels without a done flag: the chain runs on behind a token that ends the row): one rule per run."""
    c = _case(dname)
    m, eng, enc, emask = _model(dname)
    fails, und, tot = [], 0, 0
    for r in (1, 4, 5, 6, 7, 9, 10, 12):
        logits, tok, placed = _run(eng, enc, emask, c, [r], use_graph)
        f, u, t = _judge(c, [r], logits, tok, placed, False)
        fails += f
        und, tot = und + u, tot + t
        assert int(placed[0]) == len(c['rules'][r]['anchors'])
    print('anchor kernel %-9s B = 1, %s: %d of %d heads 2 .. 7 undecided; %d wrong' % (dname, c['form'], und, tot, len(fails)))
    assert not fails, (len(fails), sorted({f[:2] for f in fails})[:40], fails[:12])
    assert und <= .05 * tot and tot > 600


def test_refusals_leave_the_decoder_working():
    """Every refusal of the four entry points by name; nothing changes, and the run that follows is the anchored one."""
    from pianobart_amd._lib import LIB
    c = _case('default')
    m, eng, enc, emask = _model('default')
    dll = LIB.load()
    err = lambda: dll.pb_last_error().decode()
    good = np.ascontiguousarray(np.asarray(c['rules'][4]['anchors'] + c['rules'][2]['anchors'], dtype=np.int16))
    base, cnt = np.asarray([0, 3], dtype=np.int32), np.asarray([3, 1], dtype=np.int32)
    out = np.zeros(2, dtype=np.int32)
    last_pos, lim = np.full(2, -1, dtype=np.int32), np.full(2, S, dtype=np.int32)      # every array outlives the call it is passed to
    floor, stop = np.asarray([0, 0], dtype=np.int32), np.asarray([256, 2], dtype=np.int32)
    with torch.no_grad(), _decoder(eng, enc, emask, 2, 1) as (dec, _, _):
        d = dec
        call = lambda t, b=base, n=cnt: dll.pb_batch_decoder_anchor(d, t.ctypes.data, len(t), b.ctypes.data, n.ctypes.data)
        assert call(good) < 0 and 'sampler_init first' in err()
        assert dll.pb_batch_decoder_admit_anchor(d, 0, 0, 1) < 0 and 'not a dynamic decoder' in err()
        assert dll.pb_batch_decoder_seek_anchor(d, 0, 0) < 0 and 'sampler_init first' in err()
        U = np.ascontiguousarray(c['U'][:2].reshape(2, S * 8))
        n8, off8, pad8 = (np.ascontiguousarray(v, dtype=np.int32) for v in (c['sizes'], c['offs'][:8], c['pad']))
        LIB.call('pb_batch_decoder_sampler_init', dec, c['T'].ctypes.data, c['P'].ctypes.data, n8.ctypes.data, off8.ctypes.data, pad8.ctypes.data,
                 U.ctypes.data, 2 * S * 8, S, -1, 0)
        LIB.call('pb_batch_decoder_order', dec, floor.ctypes.data)
        assert dll.pb_batch_decoder_anchor(d, None, 4, base.ctypes.data, cnt.ctypes.data) < 0 and 'null argument' in err()
        assert call(good, n=np.asarray([3, 2], dtype=np.int32)) < 0 and 'outside the table' in err()
        bad = good.copy(); bad[1, 3] = 256
        assert call(bad) < 0 and 'head 3: id 256 is not an ordinary id' in err()
        bad = good.copy(); bad[1, 0] = -1
        assert call(bad) < 0 and 'id -1 is not an ordinary id' in err()
        bad = good.copy(); bad[2, 1] = 7
        assert call(bad) < 0 and 'anchors come in time order' in err()
        LIB.call('pb_batch_decoder_stop', dec, stop.ctypes.data)
        assert call(good, b=np.asarray([3, 0], dtype=np.int32), n=np.asarray([1, 3], dtype=np.int32)) < 0 and 'row 1, anchor 0: bar 2 outside' in err()
        LIB.call('pb_batch_decoder_anchor', dec, good.ctypes.data, len(good), base.ctypes.data, cnt.ctypes.data)
        forced = np.full((2, S, 8), -1, dtype=np.int16)
        assert dll.pb_batch_decoder_force(d, forced.ctypes.data) < 0 and 'carries anchors' in err()
        assert dll.pb_batch_decoder_seek_anchor(d, 1, 2) < 0 and '2 anchors placed of 1' in err()
        first = np.ascontiguousarray(np.tile(c['sos'].astype(np.int16), (2, 1)))
        LIB.call('pb_batch_decoder_start', dec, last_pos.ctypes.data, first.ctypes.data, lim.ctypes.data)
        eng.wf['head.b'].copy_(torch.from_numpy(c['logits'][0]).cuda())
        torch.cuda.synchronize()
        tk = int(LIB.query('pb_batch_decoder_launch', dec, 1, None))
        assert tk >= 0, err()
        LIB.call('pb_batch_decoder_wait', dec, tk)
        assert call(good) < 0 and 'a step was already issued' in err()
        LIB.call('pb_batch_decoder_anchors_placed', dec, out.ctypes.data)
        assert out.tolist() == [0, 1]                                  # (0, 4) < (2, 8): the candidate; (0, 4) ties row 1's anchor
        lp, tp = ctypes.c_void_p(), ctypes.c_void_p()
        LIB.call('pb_batch_decoder_logs', dec, ctypes.byref(lp), ctypes.byref(tp))
        tok = np.ctypeslib.as_array((ctypes.c_int16 * (2 * S * 8)).from_address(tp.value)).reshape(2, S, 8)
        assert tok[1, 0].tolist() == c['rules'][2]['anchors'][0] and tok[0, 0, :2].tolist() == [0, 4]
    with torch.no_grad(), _decoder(eng, enc, emask, 2, 1) as (dec, _, _):                      # a decoder with a force table refuses anchors
        LIB.call('pb_batch_decoder_sampler_init', dec, c['T'].ctypes.data, c['P'].ctypes.data, n8.ctypes.data, off8.ctypes.data, pad8.ctypes.data,
                 U.ctypes.data, 2 * S * 8, S, -1, 0)
        LIB.call('pb_batch_decoder_force', dec, forced.ctypes.data)
        assert dll.pb_batch_decoder_anchor(dec, good.ctypes.data, len(good), base.ctypes.data, cnt.ctypes.data) < 0 and 'has a force table' in err()
