"""GPU: allowed-class generation -- Engine.generate(allow=...), Engine.generate_batch(allow=...), PianoBartLM's decoder_allow,
pb_batch_decoder_allow / pb_batch_decoder_admit_allow, eval_generation --key / --pitch_range.

Contract ("Allowed classes"): a row may carry an allow mask, one bit per vocabulary column. The result is the reference
loop with sampling(logit, p, t) seeing -inf in place of every logit whose bit is 0: such a class has probability exactly 0. The draws,
the given heads, the stop test and the prefix are untouched; the special ids stay reachable; a row that is time-ordered too loses the
classes either rule removes. Both forms and both widths of the device sampler (dec_sample_kernel) test the bit where they form the
quotient, and the host's verification decides.

The models are those of tests/test_ordered_generation_gpu.py (S = 48, d = 256, 2 layers, ffn 256, 4 heads; flat bar / position bias and a
thinned decoder, so that the sampled ids wander over the whole table and a free row leaves the mask at most of its positions)."""
import ctypes

import numpy as np
import pytest
import torch

from tests.test_allowed_generation_cpu import _e2w, _restated_row
from tests.test_bar_stop_gpu import PAD, PAD0, SOS, _free, _length, _need_gpu, _prompts, _same_state, _sampler
from tests.test_ordered_generation_gpu import S, _model, _prime

pytestmark = pytest.mark.gpu
PADV = np.asarray(PAD)
V = 1280
C_MAJOR = {0, 2, 4, 5, 7, 9, 11}
PITCHES_M = {k for k in range(48, 84) if k % 12 in C_MAJOR}


def _M():
    """The reference mask: instrument {0}, pitch = C major within 48 .. 83, duration ids 0 .. 31, velocity ids 8 .. 23, time-signature ids
    with id % 7 == 3, tempo ids 16 .. 32; bar and position free."""
    from pianobart_amd import generation as G
    return G.allow_mask(_e2w(), instruments=[0], key='C:major', pitch_range=(48, 84), max_duration=31,
                        heads={5: range(8, 24), 6: [i for i in range(PAD[6]) if i % 7 == 3], 7: range(16, 33)})


def _M2():
    """The second mask: a pitch range only."""
    from pianobart_amd import generation as G
    return G.allow_mask(_e2w(), pitch_range=(60, 72))


def _M3():
    from pianobart_amd import generation as G
    return G.allow_mask(_e2w(), tempo=(90, 130), max_duration=15)


def _outside(row, k, ids, head):
    """Emitted positions >= k of one output row whose `head` id is not in ids."""
    x = np.asarray(row.cpu() if isinstance(row, torch.Tensor) else row).astype(np.int64)
    return sum(int(x[i, head]) not in ids for i in range(k, _length(x)))


def _batched(eng, m, enc, emask, seeds, allow, prefix=None, lens=None, forced=None, stop=None, order=None, **kw):
    rngs = [np.random.RandomState(s) for s in seeds]
    out = eng.generate_batch(enc, emask, m.sample_row, rngs, sampler=_sampler(m), prefix=prefix, prefix_len=lens, forced=forced, stop=stop,
                             order=order, allow=allow, **kw).cpu()
    return out, [r.get_state() for r in rngs], dict(eng.last_decode)


def _per_prompt(eng, m, enc, emask, seeds, allow, prefix=None, lens=None, forced=None, stop=None, order=None, rows=None, max_new=None, pad0=PAD0):
    """Row b through the batch-1 `generate` of its prompt under its own generator: (tokens, generator state, last_decode) per row."""
    outs, states, infos = {}, {}, {}
    for b in (range(len(seeds)) if rows is None else rows):
        np.random.set_state(np.random.RandomState(seeds[b]).get_state())
        outs[b] = eng.generate(enc[b:b + 1], emask[b:b + 1], m.sample_row, sampler=_sampler(m), max_new=max_new,
                               prefix=prefix[b:b + 1, :lens[b]] if prefix is not None and lens[b] else None,
                               forced=forced[b:b + 1] if forced is not None else None, stop=stop[b] if stop is not None else pad0,
                               order=order[b] if order is not None else None, allow=allow[b] if allow is not None else None).cpu()[0]
        states[b] = np.random.get_state()
        infos[b] = dict(eng.last_decode)
    return outs, states, infos


# ---------------------------------------------------------------------------------------------------------------- 5. paths, reference
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_allowed_paths_agree_and_equal_the_restated_reference(precision):
    """One prompt, primed with 6 rows, mask M. generate (bf16: the fused decoder, device-sampled with the sampler named and host-sampled
    without; fp32: the pb_decode_step loop), _generate_nocache, _generate_pyloop and generate_batch of the one row. Then every path's row is
    rebuilt position by position from the logits rows its host saw, with the restatement of tests/test_allowed_generation_cpu.py: bit for
    bit, the final np.random state included."""
    _need_gpu()
    from pianobart_amd import generation as G
    k = 6
    M = _M()
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
    a = run(lambda: eng.generate(enc, emask, recording, allow=M, **base))
    s = run(lambda: eng.generate(enc, emask, recording, sampler=_sampler(m), allow=M, **base))
    b = run(lambda: eng.generate(enc, emask, recording, use_cache=False, allow=M, **base))
    c = run(lambda: eng._generate_pyloop(enc, emask, recording, k, pre, None, None, None, torch.from_numpy(M)))
    rng = np.random.RandomState(5)
    del seen[:]
    g_out = eng.generate_batch(enc, emask, recording, [rng], sampler=_sampler(m), prefix=pre[None], prefix_len=[k], stop=[PAD0], allow=[M]).cpu()
    g = (g_out, rng.get_state(), dict(eng.last_decode), list(seen))
    free = run(lambda: eng.generate(enc, emask, recording, sampler=_sampler(m), **base))
    assert all('allow' not in kw for _, kw in free[3])                 # a free row is never handed the keyword
    bites = {name: _outside(free[0][0], k, ids, h) for name, h, ids in (('pitch', 3, PITCHES_M), ('duration', 4, set(range(32))),
                                                                         ('tempo', 7, set(range(16, 33))))}
    print('allowed paths (%s): positions of the free row outside the mask' % precision, bites, 'of', _length(free[0][0]) - k, 'rewinds',
          (s[2] or {}).get('rewinds'), g[2].get('rewinds'))
    assert bites['pitch'] >= 20, bites                                 # the mask bites on this prompt
    print('allowed paths (%s): equal to generate:' % precision, {name: bool(torch.equal(a[0], other[0])) for name, other in
                                                                (('device-sampled', s), ('nocache', b), ('pyloop', c), ('generate_batch', g))})
    # fp32 (exact f32 arithmetic on every path): all five are one row. bf16: nocache and pyloop run the training kernels, whose bf16 rounding
    # is not the fused decoder's (tests/test_ordered_generation_gpu.py); they are held to the restatement below, each from the logits rows
    # of its own run.
    same = ('device-sampled', 'nocache', 'pyloop', 'generate_batch') if precision == 'fp32' else ('device-sampled', 'generate_batch')
    runs = {'generate': a, 'device-sampled': s, 'nocache': b, 'pyloop': c, 'generate_batch': g}
    for name in same:
        assert torch.equal(a[0], runs[name][0]), name
        assert _same_state(a[1], runs[name][1]), name
    if precision == 'bf16':                                            # the fused decoder's record (fp32 runs the pb_decode_step loop: no record)
        assert a[2]['ended'] == s[2]['ended'] == g[2]['ended'][0] and s[2]['device_sampler'] and s[2]['rewinds'] <= 2
        assert g[2]['device_sampler'] and g[2]['rewinds'][0] <= 2
    for name, (out, state, _, rows) in runs.items():
        out = out[0]
        n = _length(out)
        assert torch.equal(out[:k], pre) and n > k + 10 and G.is_allowed(out, M, start=k), name
        assert len(rows) == S - k and all('allow' in kw for _, kw in rows), name
        np.random.seed(5)
        for i, (row, _) in enumerate(rows):
            tok = _restated_row(row, M)
            if (tok.numpy() >= PADV).any():
                assert k + i == n, (name, i, tok)                      # the token that ended the row
                break
            assert torch.equal(tok, out[k + i]), (name, k + i, tok, out[k + i])
        assert _same_state(np.random.get_state(), state), name


# ---------------------------------------------------------------------------------------------------------------- 6. row form, mixed batch
MIXED_LENS = [0, 0, 6, 0, 0, 0, 0, 0, 0, 6, 0, 0, 0, 0, 0, 0]


def _mixed():
    m = _model(32, 'bf16')
    enc, emask = _prompts(16, S, seed=41)
    prefix = torch.stack([_prime(6, 900 + b) for b in range(16)])
    M, M2 = _M(), _M2()
    allow = [M, None, M, M, M2, M, None, M2, M, M2, None, M, M2, None, M, None]
    order = [-1, -1, -1, 0, -1, -1, -1, -1, -1, -1, 0, -1, -1, -1, -1, -1]     # row 3: masked and ordered; row 10: ordered and free
    forced = _free(16, S)
    forced[5, [10, 20, 30], 3] = 61                                    # row 5: a given pitch outside its mask at three positions
    forced[6, 12, 3] = 200                                             # ... and a free row with a given head
    stops = [PAD0] * 16
    forced[7, :, 0] = forced[8, :, 0] = np.arange(S) // 4              # rows 7 and 8: given bars (the bar head is free in both masks) ...
    stops[7], stops[8] = 5, 8                                          # ... and a stop bar: they end at positions 20 and 32
    return m, enc, emask, prefix, list(range(300, 316)), allow, order, forced, stops


def test_mixed_batch_equals_the_batch_1_runs():
    """16 rows: mask M, a second mask, free rows; two primed, one also ordered, one with a given pitch outside its mask, two with a stop bar.
    generate_batch equals the batch-1 `generate` of every row under its own generator (tokens, states, `ended`) -- the B = 1 runs are the
    single-row form of the sampler; the free rows are the rows of the same call without `allow`; rewinds stay <= 2 per row in both forms."""
    _need_gpu()
    from pianobart_amd import generation as G
    m, enc, emask, prefix, seeds, allow, order, forced, stops = _mixed()
    eng = m._get_engine()
    got, g_state, info = _batched(eng, m, enc, emask, seeds, allow, prefix, MIXED_LENS, forced, stops, order)
    plain, p_state, p_info = _batched(eng, m, enc, emask, seeds, None, prefix, MIXED_LENS, forced, stops, order)
    want, w_state, w_info = _per_prompt(eng, m, enc, emask, seeds, allow, prefix, MIXED_LENS, forced, stops, order)
    pitches = lambda mask: set(np.flatnonzero(mask[531:531 + 256]).tolist())      # the pitch head starts at column 531
    bites = [_outside(plain[b], MIXED_LENS[b], pitches(allow[b]), 3) if allow[b] is not None else 0 for b in range(16)]
    print('allowed batch: positions of the unmasked rows outside the pitch set', bites, 'rewinds', info['rewinds'], 'B = 1 rewinds',
          [w_info[b]['rewinds'] for b in range(16)], 'lengths', [_length(got[b]) for b in range(16)], 'ended', info['ended'])
    assert info['batched'] and info['batch'] == 16 and info['device_sampler'] and info['launches_per_token'] == p_info['launches_per_token'] == 6 * 2 + 3
    assert set(info) == set(p_info)
    for b in range(16):
        k = MIXED_LENS[b]
        assert torch.equal(got[b], want[b]), b
        assert _same_state(g_state[b], w_state[b]) and info['ended'][b] == w_info[b]['ended'], b
        assert w_info[b]['device_sampler'] and w_info[b]['rewinds'] <= 2, (b, w_info[b]['rewinds'])
        assert torch.equal(got[b][:k], prefix[b, :k]), b
        if allow[b] is None:
            assert torch.equal(got[b], plain[b]) and _same_state(g_state[b], p_state[b]), b
            continue
        assert G.is_allowed(got[b], allow[b], start=k, forced=forced[b]), b
        if stops[b] == PAD0:                                           # a row that runs to the window's end
            assert bites[b] >= 10, (b, bites)                          # a sampler that ignored the mask would be rewound there
            assert _length(got[b]) == S, b
    assert all(r <= 2 for r in info['rewinds']), info['rewinds']
    n5 = _length(got[5])
    assert n5 > 30 and [int(got[5][i, 3]) for i in (10, 20, 30)] == [61, 61, 61] and not G.is_allowed(got[5], allow[5])      # given: written though outside
    assert G.is_time_ordered(got[3]) and G.is_time_ordered(got[10])
    assert (info['ended'][7], info['ended'][8]) == ('bar', 'bar') and (_length(got[7]), _length(got[8])) == (20, 32)


# ---------------------------------------------------------------------------------------------------------------- 7. the wide sampler
def test_wide_sampler_honours_the_mask():
    """The 2 470-id dictionary of tests/vocab_layout_util.py (heads 0 and 3 over the narrow sampler's rows), masks built by allow_mask from
    its names; 4 rows, one free, one also ordered. The batch equals the batch-1 runs, on the wide form of the sampler."""
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
    A = G.allow_mask(e2w, key='C:major', pitch_range=(100, 480), instruments=[0, 1, 2], max_duration=100, tempo=(10, 40),
                     heads={0: range(300, 900)})
    B = G.allow_mask(e2w, key='A:minor', heads={0: range(0, 1024, 2)})     # the even bars, up to the last ordinary one
    assert A.shape == (2470,) and (lay.vocab + 31) // 32 == 78 and lay.seg_off[3] % 32 != 0
    allow, order, seeds = [A, None, B, A], [-1, -1, -1, 0], [61, 62, 63, 64]
    eng = m._get_engine()
    got, g_state, info = _batched(eng, m, enc, emask, seeds, allow, order=order)
    assert eng.last_sampler_form == 'wide' and info['sampler_form'] == 'wide' and info['batched'] and info['device_sampler']
    plain, p_state, _ = _batched(eng, m, enc, emask, seeds, None, order=order)
    want, w_state, w_info = _per_prompt(eng, m, enc, emask, seeds, allow, order=order, pad0=pad0)
    assert eng.last_sampler_form == 'wide'
    print('allowed wide: lengths', [_length_of(got[b], pad0) for b in range(4)], 'rewinds', info['rewinds'], [w_info[b]['rewinds'] for b in range(4)])
    for b in range(4):
        assert torch.equal(got[b], want[b]) and _same_state(g_state[b], w_state[b]), b
        assert w_info[b]['rewinds'] <= 2 and info['rewinds'][b] <= 2, b
        n = _length_of(got[b], pad0)
        if allow[b] is None:
            assert torch.equal(got[b], plain[b]), b
            continue
        assert n > 4 and G.is_allowed(got[b], allow[b], layout=lay), b
        assert not G.is_allowed(plain[b], allow[b], layout=lay), b      # the unmasked row leaves the mask
    bars = got[0][:_length_of(got[0], pad0), 0]
    assert int(bars.min()) >= 300 and int(bars.max()) < 900 and int(bars.max()) > 272       # head 0 sampled beyond the narrow rows, inside its mask


def _length_of(row, pad0):
    bar = np.asarray(row.cpu())[:, 0]
    pad = np.flatnonzero(bar == pad0)
    return int(pad[0]) if len(pad) else len(bar)


# ---------------------------------------------------------------------------------------------------------------- 8. refill and samples
def test_allow_under_refill():
    """12 prompts in 4 slots, three distinct masks and free rows in between. The result and the generator states are those of refill=False.
    A slot passes from a masked row to a free one and from a free row to a masked one: a leaked index would keep the free successor
    inside its predecessor's mask, and a lost one would let the masked successor out."""
    _need_gpu()
    from pianobart_amd import generation as G
    m = _model(34, 'bf16')
    enc, emask = _prompts(12, S, seed=44)
    eng = m._get_engine()
    M, M2, M3 = _M(), _M2(), _M3()
    # rows are admitted in row order: rows 4 .. 7 follow rows 0 .. 3 (three of them masked), rows 8 .. 11 follow rows 4 .. 7 (all free)
    allow = [M, M2, None, M3, None, None, None, None, M, M2, M3, M]
    seeds = list(range(70, 82))
    plain, p_state, _ = _batched(eng, m, enc, emask, seeds, allow, refill=False, max_new=20)
    got, g_state, info = _batched(eng, m, enc, emask, seeds, allow, refill=4, max_new=20)
    free, _, _ = _batched(eng, m, enc, emask, seeds, None, refill=False, max_new=20)
    print('allow under refill: lengths', [_length(got[b]) for b in range(12)], 'slots', info['row_slot'], 'rewinds', info['rewinds'])
    assert info['refill'] == 4 and info['admissions'] == 8
    for b in range(12):
        assert torch.equal(got[b], plain[b]) and _same_state(g_state[b], p_state[b]), b
        if allow[b] is None:
            assert torch.equal(got[b], free[b]), b
        else:
            assert _length(got[b]) > 10 and G.is_allowed(got[b], allow[b]) and not G.is_allowed(free[b], allow[b]), b
    assert all(r <= 2 for r in info['rewinds']), info['rewinds']
    by_slot = {}
    for r, s in enumerate(info['row_slot']):                           # rows are admitted in row order
        by_slot.setdefault(s, []).append(r)
    hand = [(allow[a] is not None, allow[b] is not None) for rows in by_slot.values() for a, b in zip(rows, rows[1:])]
    assert (True, False) in hand and (False, True) in hand, (info['row_slot'], hand)
    for rows in by_slot.values():                                      # the free successor of a masked row really leaves that mask
        for a, b in zip(rows, rows[1:]):
            if allow[a] is not None and allow[b] is None:
                assert not G.is_allowed(got[b], allow[a]), (a, b)


def test_allow_with_samples_of_one_prompt():
    _need_gpu()
    from pianobart_amd import generation as G
    m = _model(33, 'bf16')
    enc, emask = _prompts(2, S, seed=43)
    eng = m._get_engine()
    counts, owner = [3, 2], [0, 0, 0, 1, 1]
    allow = [_M(), _M2()]                                              # per PROMPT, expanded through the owner map
    seeds = [3000 + 5 * r for r in range(5)]
    idx = torch.as_tensor(owner).cuda()
    want, w_state, _ = _per_prompt(eng, m, enc[idx], emask[idx], seeds, [allow[p] for p in owner])
    got, g_state, info = _batched(eng, m, enc, emask, seeds, allow, samples=counts)
    assert info['batched'] and info['groups'] == owner and info['encoder_passes'] == 2
    for r, p in enumerate(owner):
        assert torch.equal(got[r], want[r]) and _same_state(g_state[r], w_state[r]), r
        assert G.is_allowed(got[r], allow[p]) and _length(got[r]) > 10, r
    with pytest.raises(Exception, match='entries'):                    # `allow` describes the prompts, not the rows
        _batched(eng, m, enc, emask, seeds, [allow[p] for p in owner], samples=counts)


# ---------------------------------------------------------------------------------------------------------------- 9. mask meets order
def test_a_mask_below_the_bar_floor_ends_the_row():
    """order = 20 and a bar mask whose ordinary bars are 0 .. 9: the two rules leave head 0 its special ids only, so the row samples one at
    its first sampled position and ends with 'special' -- on the device-sampled and on the host-sampled path alike, and in the row form.
    specials=None: the special logits are finite, not pushed to -30."""
    _need_gpu()
    from pianobart_amd import generation as G
    m = _model(78, 'bf16', specials=None)
    enc, emask = _prompts(2, S, seed=4)
    eng = m._get_engine()
    mask = G.allow_mask(_e2w(), heads={0: range(10)})
    outs = {}
    for name, kw in (('device', dict(sampler=_sampler(m))), ('host', {})):
        np.random.seed(7)
        y = eng.generate(enc[:1], emask[:1], m.sample_row, stop=PAD0, order=20, allow=mask, **kw).cpu()
        outs[name] = (y, np.random.get_state(), dict(eng.last_decode))
    (yd, sd, idev), (yh, sh, ih) = outs['device'], outs['host']
    assert idev['device_sampler'] and not ih.get('device_sampler')
    assert idev['ended'] == ih['ended'] == 'special' and torch.equal(yd, yh) and _same_state(sd, sh)
    assert _length(yd[0]) == 0 and idev['tokens'] == ih['tokens'] == 1 and idev['rewinds'] <= 2
    want = np.random.RandomState(7)
    want.random_sample(8)                                              # one position was sampled: its 8 draws
    assert _same_state(sd, want.get_state())
    got, states, info = _batched(eng, m, enc, emask, [7, 8], [mask, None], stop=[PAD0, PAD0], order=[20, -1])
    assert info['ended'][0] == 'special' and _length(got[0]) == 0 and info['tokens'][0] == 1 and info['rewinds'][0] <= 2
    # with the floor inside the mask's bars the row lives on: bars 5 .. 9 only
    np.random.seed(7)
    y = eng.generate(enc[:1], emask[:1], m.sample_row, sampler=_sampler(m), stop=PAD0, order=5, allow=mask).cpu()[0]
    n = _length(y)
    assert n == 0 or (5 <= int(y[:n, 0].min()) and int(y[:n, 0].max()) <= 9)


# ---------------------------------------------------------------------------------------------------------------- 10. no mask
def test_no_mask_is_todays_call():
    """allow=None, an all-true mask and a list of None: the tokens, generator states, launches and record keys of the call without the
    argument."""
    _need_gpu()
    m = _model(32, 'bf16', specials='eos')
    enc, emask = _prompts(5, S, seed=41)
    eng = m._get_engine()
    seeds = [11, 12, 13, 14, 15]
    rngs = [np.random.RandomState(s) for s in seeds]
    want = eng.generate_batch(enc, emask, m.sample_row, rngs, sampler=_sampler(m)).cpu()
    w_info = dict(eng.last_decode)
    for allow in (None, [None] * 5, np.ones((5, V), dtype=bool), torch.ones(5, V, dtype=torch.bool), [None, np.ones(V, dtype=bool), None, None, None]):
        got, states, info = _batched(eng, m, enc, emask, seeds, allow)
        assert torch.equal(got, want)
        assert all(_same_state(a, r.get_state()) for a, r in zip(states, rngs))
        for key in ('launches_per_token', 'graph', 'tokens', 'steps', 'batch', 'batched', 'tokens_per_graph_replay'):
            assert info[key] == w_info[key], key
        assert set(info) == set(w_info)
    np.random.seed(9)
    a = eng.generate(enc[:1], emask[:1], m.sample_row, sampler=_sampler(m)).cpu()
    a_info, sa = dict(eng.last_decode), np.random.get_state()
    for allow in (None, np.ones(V, dtype=bool), [None], torch.ones(1, V, dtype=torch.bool)):
        np.random.seed(9)
        b = eng.generate(enc[:1], emask[:1], m.sample_row, sampler=_sampler(m), allow=allow).cpu()
        assert torch.equal(a, b) and _same_state(sa, np.random.get_state())
        assert all(eng.last_decode[key] == a_info[key] for key in ('launches_per_token', 'graph', 'tokens'))
        assert set(eng.last_decode) == set(a_info)
    plain = lambda row, rng=None: m.sample_row(row, rng)                 # a caller's sample_row without the keyword: never handed it
    rngs2 = [np.random.RandomState(s) for s in seeds]
    assert torch.equal(eng.generate_batch(enc, emask, plain, rngs2, sampler=_sampler(m), allow=[None] * 5).cpu(), want)
    y = m.generate_batch(enc, emask, seeds=seeds, decoder_allow=np.ones((5, V), dtype=bool))      # the public interface
    assert torch.equal(y, want)
    masked = m.generate_batch(enc, emask, seeds=seeds, decoder_allow=[_M()] + [None] * 4)
    assert eng.last_decode['launches_per_token'] == w_info['launches_per_token'] and torch.equal(masked[1:], want[1:]) and not torch.equal(masked[0], want[0])


# ---------------------------------------------------------------------------------------------------------------- 11. refusals
def test_allow_refusals_leave_the_decoder_working():
    """pb_batch_decoder_allow is refused before sampler_init, with an index outside the table, with a wrong word count and after a step was
    issued; pb_batch_decoder_admit_allow on a decoder that is not dynamic. Host-side checks: a refused call enqueues nothing, names itself
    in pb_last_error, and the decoder goes on with the values of the good call."""
    _need_gpu()
    from pianobart_amd import generation as G
    from pianobart_amd import ops
    from pianobart_amd._lib import LIB
    B = 2
    m = _model(36, 'bf16')
    enc, emask = _prompts(B, S, seed=46)
    eng = m._get_engine()
    err = lambda: LIB.load().pb_last_error().decode()
    i32 = lambda *v: np.asarray(v, dtype=np.int32)
    n8, off8, pad8 = np.asarray(ops.SEG_SIZES, dtype=np.int32), np.asarray(ops.SEG_OFF[:8], dtype=np.int32), np.asarray(PAD, dtype=np.int32)
    t8, p8 = np.asarray(m.SAMPLE_T, dtype=np.float32), np.asarray(m.SAMPLE_P, dtype=np.float32)
    U = np.random.RandomState(0).random_sample((B, S * 8))
    first = np.ascontiguousarray(np.tile(np.asarray(SOS, dtype=np.int16), (B, 1)))
    last_pos, lim = np.full(B, -1, dtype=np.int32), np.full(B, S, dtype=np.int32)
    packed, _ = G.check_allow([G.allow_mask(None, heads={3: [60], 2: [7]})], 1)
    words = packed.shape[1]

    def steps(dec, count):
        tk = int(LIB.query('pb_batch_decoder_launch', dec, count, None))
        assert tk >= 0, err()
        LIB.call('pb_batch_decoder_wait', dec, tk)

    with torch.no_grad(), eng._decoder_run(enc, emask, [0, 0], None) as run:
        dec = run.dec
        assert dec is not None
        good = i32(0, -1)
        assert LIB.query('pb_batch_decoder_allow', dec, packed.ctypes.data, 1, words, good.ctypes.data) < 0
        assert 'pb_batch_decoder_allow' in err() and 'sampler_init' in err()
        assert LIB.query('pb_batch_decoder_admit_allow', dec, 0, 0) < 0 and 'pb_batch_decoder_admit_allow' in err() and 'not a dynamic decoder' in err()
        LIB.call('pb_batch_decoder_sampler_init', dec, t8.ctypes.data, p8.ctypes.data, n8.ctypes.data, off8.ctypes.data, pad8.ctypes.data,
                 U.ctypes.data, B * S * 8, S, -1, 0)
        lp, tp = ctypes.c_void_p(), ctypes.c_void_p()
        LIB.call('pb_batch_decoder_logs', dec, ctypes.byref(lp), ctypes.byref(tp))
        log_tok = np.ctypeslib.as_array((ctypes.c_int16 * (B * S * 8)).from_address(tp.value)).reshape(B, S, 8)
        log_tok[:] = -7
        for bad, word in ((i32(1, -1), 'index 1'), (i32(0, -2), 'index -2')):
            assert LIB.query('pb_batch_decoder_allow', dec, packed.ctypes.data, 1, words, bad.ctypes.data) < 0
            assert 'pb_batch_decoder_allow' in err() and word in err(), err()
        assert LIB.query('pb_batch_decoder_allow', dec, packed.ctypes.data, 1, words - 1, good.ctypes.data) < 0 and 'words' in err()
        assert LIB.query('pb_batch_decoder_allow', dec, packed.ctypes.data, 0, words, good.ctypes.data) < 0 and 'pb_batch_decoder_allow' in err()
        assert LIB.query('pb_batch_decoder_allow', dec, None, 1, words, good.ctypes.data) < 0 and 'pb_batch_decoder_allow' in err()
        assert LIB.query('pb_batch_decoder_admit_allow', dec, 0, 0) < 0 and 'not a dynamic decoder' in err()
        LIB.call('pb_batch_decoder_allow', dec, packed.ctypes.data, 1, words, good.ctypes.data)      # row 0: pitch 60, instrument 7; row 1 free
        LIB.call('pb_batch_decoder_start', dec, last_pos.ctypes.data, first.ctypes.data, lim.ctypes.data)
        steps(dec, 4)
        assert LIB.query('pb_batch_decoder_allow', dec, packed.ctypes.data, 1, words, i32(-1, 0).ctypes.data) < 0
        assert 'pb_batch_decoder_allow' in err() and 'already issued' in err()
        steps(dec, 8)
        steps(dec, 4)                                                  # the run completes with the values of the good call
        got = log_tok.copy()
    assert (got[0, :16, 3] == 60).all() and (got[0, :16, 2] == 7).all()      # specials='off': an ordinary id at every position
    assert ((got[:, :16] >= 0) & (got[:, :16] < PADV)).all() and (got[1, :16, 3] != 60).any() and (got[:, 16:] == -7).all()


# ---------------------------------------------------------------------------------------------------------------- 12. the command line
def test_eval_generation_with_a_key_and_a_range(tmp_path):
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
            for f in G.ALLOW_FLAGS:                                    # the namespace a caller built before the flags existed
                delattr(args, f)
        EG.eval_generation(args)
        return out
    o = run('o.npy', '--key', 'C:major', '--pitch_range', '48:84')
    p = run('p.npy')
    q = run('q.npy', strip=True)
    assert open(p, 'rb').read() == open(q, 'rb').read()                # without the flags: the bytes of a run that never heard of them
    y, free = np.load(o), np.load(p)
    assert y.shape == (N, S, 8) and y.dtype == np.float32
    mask = G.allow_mask(_e2w(), key='C:major', pitch_range=(48, 84))
    ks = EG.prime_lengths(x, 'half', PAD0, PADV)
    new = 0
    for i in range(N):
        assert np.array_equal(y[i, :ks[i]], x[i, :ks[i]].astype(np.float32)), i
        assert G.is_allowed(y[i], mask, start=ks[i]), i
        new += _length(y[i]) - ks[i]
    print('eval_generation --key: new rows', new, 'pieces of the run without the flags outside the mask:',
          sum(not G.is_allowed(free[i], mask, start=ks[i]) for i in range(N)))
