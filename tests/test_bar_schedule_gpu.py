"""GPU: bar schedules -- Engine.generate(bar_allow=...), Engine.generate_batch(bar_allow=...), PianoBartLM's decoder_bar_allow,
pb_batch_decoder_schedule / pb_batch_decoder_admit_schedule, eval_generation --chords.

Contract ("Bar schedules"): head 0 of a token is sampled as without a schedule; with b0 = head 0's id after forcing,
heads 1 .. 7 are sampled from `row mask AND schedule[b0]` where b0 is an ordinary bar with an entry, else from the row mask. The draws, the
given heads, the stop test and the prefix are untouched. The device sampler picks the mask by the bar it sampled (a second pass where its
guess, the decoder input's bar, names another mask), and the host's verification decides.

The models are those of tests/test_ordered_generation_gpu.py (S = 48, d = 256, 2 layers, ffn 256, 4 heads; flat bar / position bias and a
thinned decoder): the sampled bars wander over the whole table, so the mask of heads 1 .. 7 changes at nearly every position -- a sampler
that ignored the schedule, or took the mask of the predecessor's bar, would be rewound at most of them."""
import numpy as np
import pytest
import torch

from tests.test_allowed_generation_cpu import _e2w
from tests.test_allowed_generation_gpu import _M, _length_of
from tests.test_bar_schedule_cpu import _reference_token
from tests.test_bar_stop_gpu import PAD, PAD0, _free, _length, _need_gpu, _prompts, _same_state, _sampler
from tests.test_ordered_generation_gpu import S, _model, _prime

pytestmark = pytest.mark.gpu
PADV = np.asarray(PAD)
V = 1280
PROG = ['C:maj', 'G:maj', 'A:min', 'F:maj']
_SCHED = {}


def _SA():
    """The chord progression, one chord per bar, repeated over all 256 bars: the pitch set changes every bar."""
    from pianobart_amd import generation as G
    if 'A' not in _SCHED:
        _SCHED['A'] = G.chord_schedule(_e2w(), PROG)
    return _SCHED['A']


def _SB():
    """A second schedule, as a dict: bar k takes the pitches 36 .. 59, 60 .. 83 or (with the short durations only) 48 .. 71 by k % 3; every
    seventh bar has no entry."""
    from pianobart_amd import generation as G
    if 'B' not in _SCHED:
        ms = [G.allow_mask(_e2w(), pitch_range=(36, 60)), G.allow_mask(_e2w(), pitch_range=(60, 84)), G.allow_mask(_e2w(), pitch_range=(48, 72), max_duration=15)]
        _SCHED['B'] = {k: ms[k % 3] for k in range(256) if k % 7}
    return _SCHED['B']


def _R():
    """A row mask that meets every bar's mask of both schedules: the melodic pitches 48 .. 83."""
    from pianobart_amd import generation as G
    return G.allow_mask(_e2w(), pitch_range=(48, 84))


def _as_dict(sched):
    return sched if isinstance(sched, dict) else {k: m for k, m in enumerate(sched) if m is not None}


def _leaves(G, row, k, sched, forced=None):
    """Emitted positions >= k of one output row that do not follow the schedule."""
    x = np.asarray(row.cpu() if isinstance(row, torch.Tensor) else row).astype(np.int64)
    return sum(not G.follows_schedule(x[i:i + 1], sched, forced=None if forced is None else forced[i:i + 1]) for i in range(k, _length(x)))


def _batched(eng, m, enc, emask, seeds, bar, allow=None, prefix=None, lens=None, forced=None, stop=None, order=None, **kw):
    rngs = [np.random.RandomState(s) for s in seeds]
    out = eng.generate_batch(enc, emask, m.sample_row, rngs, sampler=_sampler(m), prefix=prefix, prefix_len=lens, forced=forced, stop=stop,
                             order=order, allow=allow, **(dict(bar_allow=bar) if bar is not None else {}), **kw).cpu()
    return out, [r.get_state() for r in rngs], dict(eng.last_decode)


def _per_prompt(eng, m, enc, emask, seeds, bar, allow=None, prefix=None, lens=None, forced=None, stop=None, order=None, pad0=PAD0):
    """Row b through the batch-1 `generate` of its prompt under its own generator: (tokens, generator state, last_decode) per row."""
    outs, states, infos = {}, {}, {}
    for b in range(len(seeds)):
        np.random.set_state(np.random.RandomState(seeds[b]).get_state())
        outs[b] = eng.generate(enc[b:b + 1], emask[b:b + 1], m.sample_row, sampler=_sampler(m),
                               prefix=prefix[b:b + 1, :lens[b]] if prefix is not None and lens[b] else None,
                               forced=forced[b:b + 1] if forced is not None else None, stop=stop[b] if stop is not None else pad0,
                               order=order[b] if order is not None else None, allow=allow[b] if allow is not None else None,
                               bar_allow=[bar[b]] if bar[b] is not None else None).cpu()[0]
        states[b] = np.random.get_state()
        infos[b] = dict(eng.last_decode)
    return outs, states, infos


# ---------------------------------------------------------------------------------------------------------------- paths, reference
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_scheduled_paths_agree_and_equal_the_restated_reference(precision):
    """One prompt, primed with 6 rows, row mask R, schedule SA. generate (bf16: the fused decoder, device-sampled with the sampler named and
    host-sampled without; fp32: the pb_decode_step loop), _generate_nocache, _generate_pyloop and generate_batch of the one row. Then every
    path's row is rebuilt position by position from the logits rows its host saw, with the restatement of tests/test_bar_schedule_cpu.py:
    bit for bit, the final np.random state included."""
    _need_gpu()
    from pianobart_amd import generation as G
    k = 6
    own, SA = _R(), _SA()
    m = _model(78, precision)
    enc, emask = _prompts(1, S, seed=4)
    pre = _prime(k, 5)
    eng = m._get_engine()
    seen = []

    def recording(row, rng=None, **kw):
        seen.append((row.clone(), dict(kw)))
        return m.sample_row(row, rng, **kw)

    def run(fn):
        np.random.seed(5)
        del seen[:]
        out = fn().cpu()
        return out, np.random.get_state(), dict(eng.last_decode) if eng.last_decode else None, list(seen)

    base = dict(prefix=pre[None], stop=PAD0)
    plan = G.check_bar_allow([SA], [own], 1)
    ab, sc = G.unpack_allow(plan[:2], V)[0], G.unpack_schedule(plan, V)[0]
    a = run(lambda: eng.generate(enc, emask, recording, allow=own, bar_allow=SA, **base))
    s = run(lambda: eng.generate(enc, emask, recording, sampler=_sampler(m), allow=own, bar_allow=SA, **base))
    b = run(lambda: eng.generate(enc, emask, recording, use_cache=False, allow=own, bar_allow=SA, **base))
    c = run(lambda: eng._generate_pyloop(enc, emask, recording, k, pre, None, None, None, ab, sc))
    rng = np.random.RandomState(5)
    del seen[:]
    g_out = eng.generate_batch(enc, emask, recording, [rng], sampler=_sampler(m), prefix=pre[None], prefix_len=[k], stop=[PAD0], allow=[own],
                               bar_allow=[SA]).cpu()
    g = (g_out, rng.get_state(), dict(eng.last_decode), list(seen))
    free = run(lambda: eng.generate(enc, emask, recording, sampler=_sampler(m), allow=own, **base))
    assert all('sched' not in kw for _, kw in free[3])                 # a row without a schedule is never handed the keyword
    assert g[2]['scheduled'] is True
    bites = _leaves(G, free[0][0], k, SA)
    print('scheduled paths (%s): positions of the unscheduled row outside its bar\'s chord' % precision, bites, 'of', _length(free[0][0]) - k,
          'rewinds', (s[2] or {}).get('rewinds'), g[2].get('rewinds'))
    assert bites >= 10, bites
    print('scheduled paths (%s): equal to generate:' % precision, {name: bool(torch.equal(a[0], other[0])) for name, other in
                                                                  (('device-sampled', s), ('nocache', b), ('pyloop', c), ('generate_batch', g))})
    # fp32 (exact f32 arithmetic on every path): all five are one row. bf16: nocache and pyloop run the training kernels, whose bf16 rounding
    # is not the fused decoder's (tests/test_allowed_generation_gpu.py); they are held to the restatement below, each from its own logits rows
    same = ('device-sampled', 'nocache', 'pyloop', 'generate_batch') if precision == 'fp32' else ('device-sampled', 'generate_batch')
    runs = {'generate': a, 'device-sampled': s, 'nocache': b, 'pyloop': c, 'generate_batch': g}
    for name in same:
        assert torch.equal(a[0], runs[name][0]), name
        assert _same_state(a[1], runs[name][1]), name
    if precision == 'bf16':
        assert a[2]['ended'] == s[2]['ended'] == g[2]['ended'][0] and s[2]['device_sampler'] and s[2]['rewinds'] <= 2
        assert g[2]['device_sampler'] and g[2]['rewinds'][0] <= 2 and a[2]['scheduled'] is True and s[2]['scheduled'] is True and 'scheduled' not in free[2]
    sched = _as_dict(SA)
    for name, (out, state, _, rows) in runs.items():
        out = out[0]
        n = _length(out)
        assert torch.equal(out[:k], pre) and n > k + 10 and G.follows_schedule(out, SA, start=k) and G.is_allowed(out, own, start=k), name
        assert len(rows) == S - k and all('sched' in kw and 'allow' in kw for _, kw in rows), name
        np.random.seed(5)
        for i, (row, _) in enumerate(rows):
            tok = _reference_token(row, own, sched, out[k + i - 1].numpy(), -1, None)
            if (tok.numpy() >= PADV).any():
                assert k + i == n, (name, i, tok)                      # the token that ended the row
                break
            assert torch.equal(tok, out[k + i]), (name, k + i, tok, out[k + i])
        assert _same_state(np.random.get_state(), state), name


# ---------------------------------------------------------------------------------------------------------------- row form, mixed batch
MIXED_LENS = [0, 0, 6, 0, 0, 0, 0, 0, 0, 6, 0, 0, 0, 0, 0, 0]


def _mixed():
    m = _model(32, 'bf16')
    enc, emask = _prompts(16, S, seed=41)
    prefix = torch.stack([_prime(6, 900 + b) for b in range(16)])
    SA, SB, own, M = _SA(), _SB(), _R(), _M()
    #      0     1     2    3    4     5    6     7    8    9    10    11  12    13    14   15
    bar = [SA, None, SA, SA, None, SA, None, SB, SB, SB, None, SB, None, None, SA, SB]
    allow = [None, None, own, None, own, None, None, None, None, own, None, M, own, None, None, None]      # rows 4 and 12: a row mask only
    order = [-1, -1, -1, 0, -1, -1, -1, -1, -1, -1, 0, -1, -1, -1, -1, -1]     # row 3: scheduled and ordered; row 10: ordered and free
    forced = _free(16, S)
    forced[5, [10, 20, 30], 3] = 61                                    # row 5: a given pitch (C#) outside every chord of its schedule
    forced[6, 12, 3] = 200                                             # ... and a free row with a given head
    stops = [PAD0] * 16
    forced[7, :, 0] = forced[8, :, 0] = np.arange(S) // 4              # rows 7 and 8: given bars, so the mask changes every 4 positions ...
    stops[8] = 8                                                       # ... and row 8 a stop bar: it ends at position 32
    return m, enc, emask, prefix, list(range(300, 316)), bar, allow, order, forced, stops


def test_mixed_batch_equals_the_batch_1_runs():
    """16 rows: two schedules, with and without a row mask; rows with a row mask only; free rows; one scheduled and ordered; given bars; a
    given pitch outside its bar's mask; a stop bar; two primed. generate_batch equals the batch-1 `generate` of every row under its own
    generator (tokens, states, `ended`); the rows without a schedule are the rows of the same call without the argument; every scheduled
    row follows its schedule where the same row sampled without it leaves it at 10 or more positions; rewinds stay <= 2 per row in both
    forms; the launches per token are unchanged."""
    _need_gpu()
    from pianobart_amd import generation as G
    m, enc, emask, prefix, seeds, bar, allow, order, forced, stops = _mixed()
    eng = m._get_engine()
    got, g_state, info = _batched(eng, m, enc, emask, seeds, bar, allow, prefix, MIXED_LENS, forced, stops, order)
    plain, p_state, p_info = _batched(eng, m, enc, emask, seeds, None, allow, prefix, MIXED_LENS, forced, stops, order)
    want, w_state, w_info = _per_prompt(eng, m, enc, emask, seeds, bar, allow, prefix, MIXED_LENS, forced, stops, order)
    bites = [_leaves(G, plain[b], MIXED_LENS[b], bar[b], forced[b]) if bar[b] is not None else 0 for b in range(16)]
    print('scheduled batch: positions of the unscheduled rows outside their schedule', bites, 'rewinds', info['rewinds'], 'B = 1 rewinds',
          [w_info[b]['rewinds'] for b in range(16)], 'lengths', [_length(got[b]) for b in range(16)], 'ended', info['ended'])
    assert info['batched'] and info['batch'] == 16 and info['device_sampler'] and info['launches_per_token'] == p_info['launches_per_token'] == 6 * 2 + 3
    assert set(info) == set(p_info) | {'scheduled'} and 'scheduled' not in p_info
    for b in range(16):
        k = MIXED_LENS[b]
        assert torch.equal(got[b], want[b]), b
        assert _same_state(g_state[b], w_state[b]) and info['ended'][b] == w_info[b]['ended'], b
        assert w_info[b]['device_sampler'] and w_info[b]['rewinds'] <= 2, (b, w_info[b]['rewinds'])
        assert ('scheduled' in w_info[b]) == (bar[b] is not None), b
        assert torch.equal(got[b][:k], prefix[b, :k]), b
        if allow[b] is not None:
            assert G.is_allowed(got[b], allow[b], start=k, forced=forced[b]), b
        if bar[b] is None:
            assert torch.equal(got[b], plain[b]) and _same_state(g_state[b], p_state[b]), b
            continue
        assert G.follows_schedule(got[b], bar[b], start=k, forced=forced[b]), b
        assert bites[b] >= 10, (b, bites)                              # a sampler that ignored the schedule would be rewound there
    assert all(r <= 2 for r in info['rewinds']), info['rewinds']
    n5 = _length(got[5])
    assert n5 > 30 and [int(got[5][i, 3]) for i in (10, 20, 30)] == [61, 61, 61] and not G.follows_schedule(got[5], bar[5])      # given: written though outside
    assert G.is_time_ordered(got[3]) and G.is_time_ordered(got[10])
    assert info['ended'][8] == 'bar' and _length(got[8]) == 32 and _length(got[7]) == S
    # the mask follows the GIVEN bar, not the sampled one: rows 7 and 8 change their pitch window every 4 positions
    assert [int(got[7][i, 0]) for i in (0, 3, 4, 47)] == [0, 0, 1, 11]


# ---------------------------------------------------------------------------------------------------------------- the wide sampler
def test_wide_sampler_follows_the_schedule():
    """The 2 470-id dictionary of tests/vocab_layout_util.py (1024 bars; heads 0 and 3 over the narrow sampler's rows), schedules built from
    its names; 4 rows, one free, one also ordered with a row mask. The batch equals the batch-1 runs, on the wide form of the sampler."""
    _need_gpu()
    from pianobart_amd import generation as G
    from tests.test_vocab_layout_gpu import _gen_model
    from tests.vocab_layout_util import synth_batch
    m, _, _, sizes = _gen_model('wide')
    lay = m.pianobart.layout
    e2w = m.pianobart.e2w
    pad0 = sizes[0] - 6
    enc = synth_batch(sizes, 4, S, seed=18, min_len=S - 9)[5].cuda()
    emask = (enc[:, :, 0] != pad0).float()
    A = G.chord_schedule(e2w, PROG)
    lo, hi = G.allow_mask(e2w, pitch_range=(0, 256)), G.allow_mask(e2w, pitch_range=(256, 512), max_duration=100)
    Bs = {k: (lo if k % 2 else hi) for k in range(1024)}               # the lower half of the pitches in the odd bars, the upper half in the even ones
    own = G.allow_mask(e2w, pitch_range=(100, 480), instruments=[0, 1, 2])
    assert len(A) == 1024 and lay.vocab == 2470
    bar, allow, order, seeds = [A, None, Bs, A], [None, None, None, own], [-1, -1, -1, 0], [61, 62, 63, 64]
    eng = m._get_engine()
    got, g_state, info = _batched(eng, m, enc, emask, seeds, bar, allow, order=order)
    assert eng.last_sampler_form == 'wide' and info['sampler_form'] == 'wide' and info['batched'] and info['device_sampler'] and info['scheduled']
    plain, p_state, _ = _batched(eng, m, enc, emask, seeds, None, allow, order=order)
    want, w_state, w_info = _per_prompt(eng, m, enc, emask, seeds, bar, allow, order=order, pad0=pad0)
    assert eng.last_sampler_form == 'wide'
    print('scheduled wide: lengths', [_length_of(got[b], pad0) for b in range(4)], 'rewinds', info['rewinds'], [w_info[b]['rewinds'] for b in range(4)])
    for b in range(4):
        assert torch.equal(got[b], want[b]) and _same_state(g_state[b], w_state[b]), b
        assert w_info[b]['rewinds'] <= 2 and info['rewinds'][b] <= 2, b
        if bar[b] is None:
            assert torch.equal(got[b], plain[b]), b
            continue
        assert _length_of(got[b], pad0) > 4 and G.follows_schedule(got[b], bar[b], layout=lay), b
        assert not G.follows_schedule(plain[b], bar[b], layout=lay), b      # the unscheduled row leaves the schedule
    assert G.is_allowed(got[3], own, layout=lay)
    bars3 = got[3][:_length_of(got[3], pad0), 0].numpy()
    assert (np.diff(bars3) >= 0).all()                                 # row 3 is time-ordered too


# ---------------------------------------------------------------------------------------------------------------- refill and samples
def test_schedule_under_refill():
    """12 prompts in 4 slots, two schedules and free rows in between. The result and the generator states are those of refill=False. A
    slot passes from a scheduled row to a free one and from a free row to a scheduled one: a leaked index would keep the free successor
    inside its predecessor's schedule, and a lost one would let the scheduled successor out."""
    _need_gpu()
    from pianobart_amd import generation as G
    m = _model(34, 'bf16')
    enc, emask = _prompts(12, S, seed=44)
    eng = m._get_engine()
    SA, SB = _SA(), _SB()
    # rows are admitted in row order: rows 4 .. 7 follow rows 0 .. 3 (three of them scheduled), rows 8 .. 11 follow rows 4 .. 7 (all free)
    bar = [SA, SB, None, SA, None, None, None, None, SA, SB, SB, SA]
    allow = [None, _R(), None, None, None, _R(), None, None, None, None, _R(), None]
    seeds = list(range(70, 82))
    plain, p_state, _ = _batched(eng, m, enc, emask, seeds, bar, allow, refill=False, max_new=20)
    got, g_state, info = _batched(eng, m, enc, emask, seeds, bar, allow, refill=4, max_new=20)
    free, _, f_info = _batched(eng, m, enc, emask, seeds, None, allow, refill=4, max_new=20)
    print('schedule under refill: lengths', [_length(got[b]) for b in range(12)], 'slots', info['row_slot'], 'rewinds', info['rewinds'])
    assert info['refill'] == 4 and info['admissions'] == 8 and info['scheduled'] is True and 'scheduled' not in f_info
    assert info['launches_per_token'] == f_info['launches_per_token']
    for b in range(12):
        assert torch.equal(got[b], plain[b]) and _same_state(g_state[b], p_state[b]), b
        if bar[b] is None:
            assert torch.equal(got[b], free[b]), b
        else:
            assert _length(got[b]) > 10 and G.follows_schedule(got[b], bar[b]) and not G.follows_schedule(free[b], bar[b]), b
    assert all(r <= 2 for r in info['rewinds']), info['rewinds']
    by_slot = {}
    for r, s in enumerate(info['row_slot']):                           # rows are admitted in row order
        by_slot.setdefault(s, []).append(r)
    hand = [(bar[a] is not None, bar[b] is not None) for rows in by_slot.values() for a, b in zip(rows, rows[1:])]
    assert (True, False) in hand and (False, True) in hand, (info['row_slot'], hand)
    for rows in by_slot.values():                                      # the free successor of a scheduled row really leaves that schedule
        for a, b in zip(rows, rows[1:]):
            if bar[a] is not None and bar[b] is None:
                assert not G.follows_schedule(got[b], bar[a]), (a, b)


def test_schedule_with_samples_of_one_prompt():
    _need_gpu()
    from pianobart_amd import generation as G
    m = _model(33, 'bf16')
    enc, emask = _prompts(2, S, seed=43)
    eng = m._get_engine()
    counts, owner = [3, 2], [0, 0, 0, 1, 1]
    bar, allow = [_SA(), _SB()], [None, _R()]                          # per PROMPT, expanded through the owner map
    seeds = [3000 + 5 * r for r in range(5)]
    idx = torch.as_tensor(owner).cuda()
    want, w_state, _ = _per_prompt(eng, m, enc[idx], emask[idx], seeds, [bar[p] for p in owner], [allow[p] for p in owner])
    got, g_state, info = _batched(eng, m, enc, emask, seeds, bar, allow, samples=counts)
    assert info['batched'] and info['groups'] == owner and info['encoder_passes'] == 2 and info['scheduled']
    for r, p in enumerate(owner):
        assert torch.equal(got[r], want[r]) and _same_state(g_state[r], w_state[r]), r
        assert G.follows_schedule(got[r], bar[p]) and _length(got[r]) > 10, r
    with pytest.raises(Exception, match='entries'):                    # `bar_allow` describes the prompts, not the rows
        _batched(eng, m, enc, emask, seeds, [bar[p] for p in owner], None, samples=counts)


# ---------------------------------------------------------------------------------------------------------------- no schedule
def test_no_schedule_is_todays_call():
    """bar_allow=None, a list of None, empty schedules and all-true entries: the tokens, generator states, launches and record keys of the
    call without the argument; the public interface takes the argument."""
    _need_gpu()
    m = _model(32, 'bf16', specials='eos')
    enc, emask = _prompts(5, S, seed=41)
    eng = m._get_engine()
    seeds = [11, 12, 13, 14, 15]
    rngs = [np.random.RandomState(s) for s in seeds]
    want = eng.generate_batch(enc, emask, m.sample_row, rngs, sampler=_sampler(m)).cpu()
    w_info = dict(eng.last_decode)
    ones = np.ones(V, dtype=bool)
    for bar in (None, [None] * 5, [{}] * 5, [[ones, None, ones]] + [None] * 4, [{255: torch.from_numpy(ones)}, None, [], None, None]):
        got, states, info = _batched(eng, m, enc, emask, seeds, None, bar_allow=bar)
        assert torch.equal(got, want)
        assert all(_same_state(a, r.get_state()) for a, r in zip(states, rngs))
        for key in ('launches_per_token', 'graph', 'tokens', 'steps', 'batch', 'batched', 'tokens_per_graph_replay'):
            assert info[key] == w_info[key], key
        assert set(info) == set(w_info)
    np.random.seed(9)
    a = eng.generate(enc[:1], emask[:1], m.sample_row, sampler=_sampler(m)).cpu()
    a_info, sa = dict(eng.last_decode), np.random.get_state()
    for bar in (None, [None], {}, [ones, ones], {3: ones}):
        np.random.seed(9)
        b = eng.generate(enc[:1], emask[:1], m.sample_row, sampler=_sampler(m), bar_allow=bar).cpu()
        assert torch.equal(a, b) and _same_state(sa, np.random.get_state())
        assert all(eng.last_decode[key] == a_info[key] for key in ('launches_per_token', 'graph', 'tokens'))
        assert set(eng.last_decode) == set(a_info)
    plain = lambda row, rng=None: m.sample_row(row, rng)                 # a caller's sample_row without the keyword: never handed it
    rngs2 = [np.random.RandomState(s) for s in seeds]
    assert torch.equal(eng.generate_batch(enc, emask, plain, rngs2, sampler=_sampler(m), bar_allow=[None] * 5).cpu(), want)
    y = m.generate_batch(enc, emask, seeds=seeds, decoder_bar_allow=[{}] * 5)      # the public interface
    assert torch.equal(y, want)
    sched = m.generate_batch(enc, emask, seeds=seeds, decoder_bar_allow=[_SA()] + [None] * 4)
    assert eng.last_decode['launches_per_token'] == w_info['launches_per_token'] and eng.last_decode['scheduled'] is True
    assert torch.equal(sched[1:], want[1:]) and not torch.equal(sched[0], want[0])
    from pianobart_amd import generation as G
    assert G.follows_schedule(sched[0], _SA()) and not G.follows_schedule(want[0], _SA())
    np.random.seed(11)                                                 # forward(generate=True): the row of generate_batch under the same generator
    one = m(input_ids_encoder=enc[:1], encoder_attention_mask=emask[:1], generate=True, decoder_bar_allow=_SA())
    assert torch.equal(one[0], sched[0])
    with pytest.raises(Exception, match='generate=True'):
        m(input_ids_encoder=enc[:1], input_ids_decoder=enc[:1], encoder_attention_mask=emask[:1], decoder_attention_mask=emask[:1],
          decoder_bar_allow=_SA())


# ---------------------------------------------------------------------------------------------------------------- the command line
def test_eval_generation_with_chords(tmp_path):
    _need_gpu()
    from pianobart_amd import eval_generation as EG
    from pianobart_amd import generation as G
    from tests.golden_util import synth_octuple_batch
    N = 6
    x = synth_octuple_batch(N, S, seed=5, min_len=S // 2)[5].numpy()
    np.save(str(tmp_path / 'prompts.npy'), x)
    base = ['--dataset_path', str(tmp_path), '--dataset_name', 'prompts.npy', '--max_seq_len', str(S), '--hs', '256', '--layers', '2',
            '--ffn_dims', '256', '--heads', '4', '--nopretrain', '--seed', '0', '--batch_size', '16', '--prime', 'half']

    def run(name, *extra, strip=False):
        torch.manual_seed(0)
        out = str(tmp_path / name)
        args = EG.get_args(base + ['--output', out] + list(extra))
        if strip:
            for f in ('chords', 'bars_per_chord', 'chord_start'):      # the namespace a caller built before the flags existed
                delattr(args, f)
        EG.eval_generation(args)
        return out
    o = run('o.npy', '--chords', 'C:maj,G:maj,A:min,F:maj')
    p = run('p.npy')
    q = run('q.npy', strip=True)
    assert open(p, 'rb').read() == open(q, 'rb').read()                # without the flags: the bytes of a run that never heard of them
    y, free = np.load(o), np.load(p)
    assert y.shape == (N, S, 8) and y.dtype == np.float32
    ks = EG.prime_lengths(x, 'half', PAD0, PADV)
    new = left = 0
    args = EG.get_args(base + ['--chords', 'C:maj,G:maj,A:min,F:maj'])
    for i in range(N):
        sched = G.schedule_from_args(args, _e2w(), x[i, :ks[i]])      # the first chord in the bar after the one the piece's prime ends in
        assert sched[int(x[i, ks[i] - 1, 0])] is None and sched[int(x[i, ks[i] - 1, 0]) + 1] is not None, i
        assert np.array_equal(y[i, :ks[i]], x[i, :ks[i]].astype(np.float32)), i
        assert G.follows_schedule(y[i], sched, start=ks[i]), i
        new += _length(y[i]) - ks[i]
        left += not G.follows_schedule(free[i], sched, start=ks[i])
    print('eval_generation --chords: new rows', new, 'pieces of the run without the flags outside their schedule:', left)
    assert new > 0
