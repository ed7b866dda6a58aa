"""GPU: bar-bounded generation -- Engine.generate(stop=...), Engine.generate_batch(stop=...), PianoBartLM's decoder_stop,
pb_batch_decoder_stop / pb_batch_decoder_admit_stop, eval_generation --bars / --infill.

Contract ("Stop at a bar; infilling"): `stop` is one bar id s_b per row, 0 <= s_b <= pad[0] (256 = no stop). The result
is the reference loop (model.py:42-65) with the stop test `(current_output >= pad).any()` replaced, for row b, by `(current_output >=
pad).any() or current_output[0] >= s_b`. So a stopped row equals the unstopped row cut at its first position i >= k_b whose bar is >= s_b,
and its generator state is the unstopped run's after the draws of positions k_b .. i. The fused decoder makes the same test in its device
sampler (dec_sample_kernel<true, *> against BState.stop) and the host's verification decides.

Bars are made controllable by giving head 0 through `forced` (bar = i // 4), so where a row stops does not depend on the random weights."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

from tests.golden_util import load_vocab, randomize_params, synth_octuple_batch

pytestmark = pytest.mark.gpu
E2W, W2E = load_vocab()
PAD = [256, 128, 129, 256, 128, 32, 254, 49]
SOS = [258, 130, 131, 258, 130, 34, 256, 51]
EOS = [p + 3 for p in PAD]
PAD0 = PAD[0]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


def _cfg(S, d, L, f, h):
    from pianobart_amd.model import BartConfig
    return BartConfig(max_position_embeddings=S, d_model=d, encoder_layers=L, decoder_layers=L, encoder_ffn_dim=f, decoder_ffn_dim=f,
                      encoder_attention_heads=h, decoder_attention_heads=h, dropout=0.0)


def _lm(S, d, L, f, h, seed, precision, specials=None):
    """specials None: random weights as they come; 'off': special ids unsamplable; 'eos': only EOS of the tempo head reachable, as likely
    as its favourite class (rows stop at different positions)."""
    from pianobart_amd.model import PianoBart, PianoBartLM
    m = PianoBartLM(PianoBart(_cfg(S, d, L, f, h), E2W, W2E, precision=precision))
    randomize_params(m, seed)
    with torch.no_grad():
        if specials is not None:
            for i, p0 in enumerate(PAD):
                m.mask_lm.proj[i].bias[p0:] = -30.0
        if specials == 'eos':
            m.mask_lm.proj[7].bias[PAD[7] + 3] = m.mask_lm.proj[7].bias[:PAD[7]].max()
    return m.eval()


def _flat_bar_head(m):
    """The bar head of a model made on the CPU (before .cuda() and the engine) without its ordinary ids' bias. The head samples at p = 1, which
    takes the largest logit: without the random bias the bar follows the hidden state alone, so a free bar head changes its bar where the
    decoder's inputs (the heads sampled at p < 1, or given ones) move it -- for some prompts more than for others."""
    with torch.no_grad():
        m.mask_lm.proj[0].bias[:PAD0] = 0.0
    return m


def _piece(n, seed):
    """n ordinary Octuple rows (no special id)."""
    t = synth_octuple_batch(1, n + 2, seed=seed, min_len=n + 2)[5][0]
    return t[:n].clone()


def _prompts(n, S, seed):
    enc = synth_octuple_batch(n, S, seed=seed, min_len=S // 2)[5].cuda()
    return enc, (enc[:, :, 0] != 256).float()


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def _sampler(m):
    return dict(T=m.SAMPLE_T, P=m.SAMPLE_P)


def _free(*shape):
    return np.full(shape + (8,), -1, dtype=np.int64)


def _length(row):
    """Emitted positions of one output row (S, 8): the rows in front of its first bar PAD."""
    bar = np.asarray(row.cpu() if isinstance(row, torch.Tensor) else row)[:, 0]
    pad = np.flatnonzero(bar == PAD0)
    return int(pad[0]) if len(pad) else len(bar)


def _bars(S):
    return np.arange(S) // 4


def _cut(row, k, stop):
    """The corollary of the contract: the unstopped row (S, 8) cut at its first emitted position i >= k whose bar is >= stop. Returns
    (row, i), i None where no emitted position trips the stop (the row is the unstopped row)."""
    row = row.clone()
    n = _length(row)
    hit = [i for i in range(k, n) if int(row[i, 0]) >= stop]
    if not hit:
        return row, None
    row[hit[0]:] = torch.tensor(PAD)
    return row, hit[0]


def _state_after(seed_state, frow, k, i):
    """The generator state after the draws of positions k .. i: one block of 8 per position with a free head."""
    rng = np.random.RandomState()
    rng.set_state(seed_state)
    free = int((np.asarray(frow)[k:i + 1] < 0).any(1).sum()) if frow is not None else i + 1 - k
    rng.random_sample(8 * free)
    return rng.get_state()


# ---------------------------------------------------------------------------------------------------------------- 1. the paths agree
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_stop_paths_agree(precision):
    _need_gpu()
    S, k, stop = 48, 6, 6
    m = _lm(S, 256, 2, 256, 4, 78, precision, specials='eos').cuda()
    enc, emask = _prompts(1, S, seed=4)
    pre = _piece(k, 5)
    pre[2, 0] = 9                                                      # a prefix bar past the stop: positions below k are not tested
    piece = _piece(S, 6).numpy()
    forced = _free(S)
    forced[k:, 0] = _bars(S)[k:]                                       # the bar of position i is i // 4: the stop trips at position 24
    forced[k:34, 7] = piece[k:34, 7]                                   # the one head that can sample a special id: ordinary ids up to position 33
    eng = m._get_engine()
    seed_state = np.random.RandomState(5).get_state()

    def run(fn):
        np.random.seed(5)
        out = fn().cpu()
        return out, np.random.get_state(), dict(eng.last_decode) if eng.last_decode else None

    def four(**kw):
        base = dict(prefix=pre[None], forced=forced[None])
        a = run(lambda: eng.generate(enc, emask, m.sample_row, **base, **kw))                       # fp32: pb_decode_step, bf16: fused host-sampled
        s = run(lambda: eng.generate(enc, emask, m.sample_row, sampler=_sampler(m), **base, **kw))  # bf16: fused device-sampled
        b = run(lambda: eng.generate(enc, emask, m.sample_row, use_cache=False, **base, **kw))
        c = run(lambda: eng._generate_pyloop(enc, emask, m.sample_row, k, pre, forced.astype(np.int16), kw.get('stop')))
        return a, s, b, c

    free = four()
    (a, sa, ia), (s, ss, is_), (b, sb, _), (c, sc, _) = four(stop=stop)
    assert torch.equal(b, c) and _same_state(sb, sc)                        # same kernels: bitwise
    assert torch.equal(a, s) and _same_state(sa, ss)                        # the host's token always wins
    if precision == 'fp32':
        assert torch.equal(a, b) and _same_state(sa, sb)
    else:
        assert ia['ended'] == 'bar' and is_['ended'] == 'bar'
    for (out, state, _), (whole, _, _) in zip(((a, sa, 0), (s, ss, 0), (b, sb, 0), (c, sc, 0)), free):
        assert _length(whole[0]) >= 34
        want, i = _cut(whole[0], k, stop)
        assert i == 24 and torch.equal(out[0], want) and torch.equal(out[0, :k], pre)
        assert _same_state(state, _state_after(seed_state, forced, k, i))  # the tripping token's draws are consumed, nothing behind it


# ---------------------------------------------------------------------------------------------------------------- 2. batch contract
def _batch_setup(n=17, S=64, seed=32):
    """17 rows: given monotone bars with stops at different positions (0 .. 7, 14); a row that a fully given position stops (8); free bar
    heads whose stop comes from their own unstopped run (9, 15: filled in by the test); no stop (10, 16); a primed row (11); a row whose
    prefix already passes its stop (12); stop = 0 (13)."""
    m = _flat_bar_head(_lm(S, 256, 2, 512, 4, seed, 'bf16', specials='eos')).cuda()
    enc, emask = _prompts(n, S, seed=41)
    prefix = torch.stack([_piece(S, 600 + b) for b in range(n)])
    pieces = np.stack([_piece(S, 700 + b).numpy() for b in range(n)])
    lens, forced, stops = [0] * n, _free(n, S), [PAD0] * n
    bars = _bars(S)
    for b in list(range(8)) + [14]:
        forced[b, :, 0], forced[b, :, 7] = bars, pieces[b, :, 7]       # bars given, the stopping head ordinary: unstopped, the row fills the window
        stops[b] = 2 + (3 * b) % 11                                    # bars 2, 5, 8, 11, 3, 6, 9, 12 and 11: positions 8 .. 48
    forced[8, :12] = pieces[8, :12]
    forced[8, :12, 0] = bars[:12]
    forced[8, 12] = pieces[8, 12]                                      # a fully given position whose bar trips the stop: nothing drawn at all
    forced[8, 12, 0], stops[8] = 50, 40
    lens[11] = 10
    forced[11, 10:, 0], forced[11, 10:, 7] = bars[10:], pieces[11, 10:, 7]
    stops[11] = 5                                                      # primed: position 20
    lens[12] = 8
    prefix[12, :8, 0] = 9
    stops[12] = 5                                                      # the prefix already holds bars >= 5: legal, tested from position 8 on
    stops[13] = 0                                                      # the first token ends the row
    for b in (9, 15):
        forced[b, :, 7] = pieces[b, :, 7]                              # free bar heads on rows that no special id ends early
    return m, enc, emask, prefix, lens, forced, stops


def _reference(eng, m, enc, emask, prefix, lens, forced, stops, seeds, max_new=None, rows=None):
    outs, states, infos = {}, {}, {}
    for b in (range(len(seeds)) if rows is None else rows):
        np.random.set_state(np.random.RandomState(seeds[b]).get_state())
        outs[b] = eng.generate(enc[b:b + 1], emask[b:b + 1], m.sample_row, max_new=max_new, sampler=_sampler(m),
                               prefix=prefix[b:b + 1, :lens[b]] if prefix is not None else None,
                               forced=forced[b:b + 1] if forced is not None else None, stop=stops[b] if stops is not None else None).cpu()[0]
        states[b] = np.random.get_state()
        infos[b] = dict(eng.last_decode)
    return outs, states, infos


def _batched(eng, m, enc, emask, prefix, lens, forced, stops, seeds, max_new=None, **kw):
    rngs = [np.random.RandomState(s) for s in seeds]
    out = eng.generate_batch(enc, emask, m.sample_row, rngs, max_new=max_new, sampler=_sampler(m), prefix=prefix, prefix_len=lens, forced=forced,
                             stop=stops, **kw).cpu()
    return out, [r.get_state() for r in rngs], dict(eng.last_decode)


def test_stop_batch_equals_batch1_per_row():
    _need_gpu()
    m, enc, emask, prefix, lens, forced, stops = _batch_setup()
    n, S = forced.shape[:2]
    eng = m._get_engine()
    seeds = [2000 + 7 * b for b in range(n)]
    whole, whole_state, _ = _reference(eng, m, enc, emask, prefix, lens, forced, None, seeds)
    for b in (9, 15):                                                  # the largest bar of the first half of what the row wrote by itself
        k, e = lens[b], _length(whole[b])
        half = whole[b][k:k + max(1, (e - k) // 2), 0]
        stops[b] = int(half.max()) if e > k else 0
    want, w_state, w_info = _reference(eng, m, enc, emask, prefix, lens, forced, stops, seeds)
    print('stop batch-1: stops', stops, 'lengths', [_length(want[b]) for b in range(n)], 'unstopped', [_length(whole[b]) for b in range(n)],
          'ended', [w_info[b]['ended'] for b in range(n)])
    inside = [b for b in range(n) if w_info[b]['ended'] == 'bar' and lens[b] < _length(want[b]) < _length(whole[b]) - 1]
    assert len(inside) >= 8, inside                                    # on the reference alone: the stop really cuts rows mid-way
    for b in list(range(8)) + [14]:
        assert _length(want[b]) == 4 * stops[b] and _length(whole[b]) == S, b
    assert _length(want[8]) == 12 and _same_state(w_state[8], np.random.RandomState(seeds[8]).get_state())      # given all the way: no draw
    assert _length(want[11]) == 20 and _length(want[13]) == 0 and w_info[13]['ended'] in ('bar', 'special')
    assert _same_state(w_state[13], _state_after(np.random.RandomState(seeds[13]).get_state(), None, 0, 0))      # the one token's 8 draws
    for b in (10, 16):
        assert torch.equal(want[b], whole[b]) and _same_state(w_state[b], whole_state[b]) and w_info[b]['ended'] != 'bar', b
    for b in range(n):                                                 # the corollary, row by row
        cut, i = _cut(whole[b], lens[b], stops[b])
        assert torch.equal(want[b], cut), b
        if i is not None:
            assert _same_state(w_state[b], _state_after(np.random.RandomState(seeds[b]).get_state(), forced[b], lens[b], i)), b
        else:
            assert _same_state(w_state[b], whole_state[b]), b

    def check(idx, tag, max_new=None, ref=(want, w_state, w_info)):
        got, states, info = _batched(eng, m, enc[idx], emask[idx], prefix[idx], [lens[i] for i in idx], forced[idx], [stops[i] for i in idx],
                                     [seeds[i] for i in idx], max_new)
        for j, i in enumerate(idx):
            assert torch.equal(got[j], ref[0][i]), (tag, j, i)
            assert _same_state(states[j], ref[1][i]), (tag, j, i)
            assert info['ended'][j] == ref[2][i]['ended'], (tag, j, i)
        return info

    info = check(list(range(n)), 'B=17 (one full chunk plus one row)')
    assert info['batched'] and info['batch'] == 1 and len(info['ended']) == n
    info = check(list(range(16)), 'B=16')
    assert info['batched'] and info['batch'] == 16 and info['launches_per_token'] == 6 * 2 + 3
    check([int(v) for v in np.random.RandomState(3).permutation(n)[:9]], 'B=9 shuffled')
    ref = _reference(eng, m, enc, emask, prefix, lens, forced, stops, seeds, max_new=9)
    info = check(list(range(16)), 'max_new=9', max_new=9, ref=ref)
    assert all(t <= 9 for t in info['tokens'])
    assert 'limit' in info['ended'] and 'bar' in info['ended']         # whichever comes first ends the row


# ---------------------------------------------------------------------------------------------------------------- 3. no stop
def test_no_stop_is_todays_call():
    """stop=None and stop = 256 everywhere: the launches, the graph and the bytes of a call without the argument. The record: stop=None
    leaves the keys of the call without the argument; a call that passes `stop` adds `ended` and nothing else."""
    _need_gpu()
    m = _lm(64, 256, 2, 512, 4, 32, 'bf16', specials='eos').cuda()
    enc, emask = _prompts(5, 64, seed=41)
    eng = m._get_engine()
    seeds = [11, 12, 13, 14, 15]
    rngs = [np.random.RandomState(s) for s in seeds]
    want = eng.generate_batch(enc, emask, m.sample_row, rngs, sampler=_sampler(m)).cpu()
    w_info = dict(eng.last_decode)
    for stop in (None, [PAD0] * 5, np.full(5, PAD0), torch.full((5,), PAD0)):
        got, states, info = _batched(eng, m, enc, emask, None, None, None, stop, seeds)
        assert torch.equal(got, want)
        assert all(_same_state(a, r.get_state()) for a, r in zip(states, rngs))
        for key in ('launches_per_token', 'graph', 'tokens', 'steps', 'batch', 'batched', 'tokens_per_graph_replay'):
            assert info[key] == w_info[key], key
        assert set(info) == set(w_info) | ({'ended'} if stop is not None else set()) and 'ended' not in w_info
        if stop is not None:
            assert len(info['ended']) == 5 and set(info['ended']) <= {'special', 'limit'}
    np.random.seed(9)
    a = eng.generate(enc[:1], emask[:1], m.sample_row, sampler=_sampler(m)).cpu()
    a_info, sa = dict(eng.last_decode), np.random.get_state()
    for stop in (None, PAD0, [PAD0]):
        np.random.seed(9)
        b = eng.generate(enc[:1], emask[:1], m.sample_row, sampler=_sampler(m), stop=stop).cpu()
        assert torch.equal(a, b) and _same_state(sa, np.random.get_state())
        assert all(eng.last_decode[key] == a_info[key] for key in ('launches_per_token', 'graph', 'tokens'))
        assert set(eng.last_decode) == set(a_info) | ({'ended'} if stop is not None else set()) and 'ended' not in a_info
        if stop is not None:
            assert eng.last_decode['ended'] in ('special', 'limit')


# ---------------------------------------------------------------------------------------------------------------- 4. rewind
def test_rewind_of_a_stopped_row():
    """The device's bar id of one row is corrupted (+ 1) at every third position; the row's bar head is free. Its stop is one above the bar the
    host samples at such a position p where the bar is the largest so far: the device's id crosses the stop there, the host's does not, so
    the device marks the row done where the host goes on, and the rewind path brings it back. (The reverse -- the host's bar at or above
    the stop, the device's below -- cannot come from a + 1 corruption; both then stop.) The row is its fault-free row, its siblings are
    untouched. Test-only fault injection of the sampler's choice: no GPU fault is involved."""
    _need_gpu()
    S, fr = 64, 2
    m = _flat_bar_head(_lm(S, 256, 2, 512, 4, 32, 'bf16', specials='off')).cuda()
    enc, emask = _prompts(4, S, seed=41)
    eng = m._get_engine()
    forced = _free(4, S)
    pieces = np.stack([_piece(S, 800 + b).numpy() for b in range(4)])
    forced[:, :, 3] = pieces[:, :, 3]                                  # the bar head stays free
    seeds, p = [21, 22, 23, 24], None
    for seed in range(23, 23 + 16):                                    # a generator under which such a position exists (host runs only)
        seeds[fr] = seed
        whole, _, _ = _reference(eng, m, enc, emask, None, [0] * 4, forced, None, seeds, rows=[fr])
        bar = whole[fr][:, 0].numpy()
        cand = [i for i in range(5, 40, 3) if bar[i] == bar[:i + 1].max() and bar[i] < 255 and (bar[i + 1:] > bar[i]).any()]
        if cand:
            p = cand[0]
            break
    assert p is not None and p % 3 == 2
    stops = [PAD0, 7, int(bar[p]) + 1, PAD0]
    want, w_state, w_info = _reference(eng, m, enc, emask, None, [0] * 4, forced, stops, seeds)
    assert w_info[fr]['ended'] == 'bar' and p < _length(want[fr]) < S          # the host walks past p and stops at a later bar
    clean, _, c_info = _batched(eng, m, enc, emask, None, None, forced, stops, seeds)
    eng.decode_fault_row = (fr, 3)
    try:
        got, g_state, g_info = _batched(eng, m, enc, emask, None, None, forced, stops, seeds)
    finally:
        eng.decode_fault_row = None
    print('rewind of a stopped row: p', p, 'stop', stops[fr], 'length', _length(want[fr]), 'rewinds', g_info['rewinds'])
    for b in range(4):
        assert torch.equal(got[b], want[b]) and torch.equal(clean[b], want[b]), b
        assert _same_state(g_state[b], w_state[b]), b
        assert g_info['ended'][b] == w_info[b]['ended'], b
        if b != fr:
            assert g_info['rewinds'][b] == 0 and c_info['rewinds'][b] == 0, b
    assert g_info['rewinds'][fr] > 0


# ---------------------------------------------------------------------------------------------------------------- 5. the decode ends early
def test_the_stop_ends_the_decode_early():
    """16 rows whose given bar reaches the stop at position 10. 8 steps per replay and two replays in flight: the device's stop shows at
    most 3 replays late, so the loop enqueues at most 11 + 3 * 8 steps -- the bound of the design, not a measurement."""
    _need_gpu()
    S, B = 64, 16
    m = _lm(S, 256, 2, 512, 4, 33, 'bf16', specials='off').cuda()
    enc, emask = _prompts(B, S, seed=43)
    eng = m._get_engine()
    forced = _free(B, S)
    forced[:, :, 0] = np.where(np.arange(S) < 10, 0, 5)
    seeds = list(range(50, 50 + B))
    got, _, info = _batched(eng, m, enc, emask, None, None, forced, [5] * B, seeds)
    whole, _, w_info = _batched(eng, m, enc, emask, None, None, forced, None, seeds)
    print('early end: steps %d with the stop, %d without' % (info['steps'], w_info['steps']))
    assert all(_length(got[b]) == 10 for b in range(B)) and info['ended'] == ['bar'] * B and info['tokens'] == [11] * B
    assert torch.equal(got[:, :10], whole[:, :10]) and all(_length(whole[b]) == S for b in range(B))
    assert info['steps'] <= 11 + 3 * info['tokens_per_graph_replay']
    assert info['steps'] < w_info['steps']


# ---------------------------------------------------------------------------------------------------------------- 6. refill
def test_refill_of_stopped_rows():
    """12 rows L, s, s, s, L, s, s, s, L, s, s, s in 4 slots: an s row stops by its bar at position 4, an L row has no stop (256) and fills
    the window. The second and third L rows are admitted into slots that s rows just left: the slot's old stop must not leak (their own
    bars pass it at position 4). The steps are compared with the same rows in chunks of 4 -- a decoder as wide as the 4 slots; refill=False on
    all 12 rows is ONE chunk of 12, three times as wide, and serves for the tokens and the generator states."""
    _need_gpu()
    S = 64
    m = _lm(S, 256, 2, 512, 4, 34, 'bf16', specials='off').cuda()
    enc, emask = _prompts(12, S, seed=44)
    eng = m._get_engine()
    forced = _free(12, S)
    forced[:, :, 0] = _bars(S)
    stops = [PAD0, 1, 1, 1] * 3
    seeds = list(range(70, 82))
    plain, p_state, p_info = _batched(eng, m, enc, emask, None, None, forced, stops, seeds, refill=False)
    got, g_state, info = _batched(eng, m, enc, emask, None, None, forced, stops, seeds, refill=4)
    assert info['refill'] == 4 and torch.equal(got, plain)
    chunk_steps = 0
    for c in range(0, 12, 4):
        _, _, ci = _batched(eng, m, enc[c:c + 4], emask[c:c + 4], None, None, forced[c:c + 4], stops[c:c + 4], seeds[c:c + 4], refill=False)
        chunk_steps += ci['steps']
    print('refill of stopped rows: admissions %d, steps %d refilled (row_steps %d), %d in chunks of 4, %d in one chunk of 12'
          % (info['admissions'], info['steps'], info['row_steps'], chunk_steps, p_info['steps']))
    for b in range(12):
        assert _same_state(g_state[b], p_state[b]), b
        assert _length(got[b]) == (S if b % 4 == 0 else 4), b          # an L row runs to its own end whatever slot it got
        assert info['ended'][b] == p_info['ended'][b] == ('limit' if b % 4 == 0 else 'bar'), b
    assert info['admissions'] == 8 and info['row_slot'][4] != 0 and info['row_slot'][8] != 0
    assert info['steps'] < chunk_steps


# ---------------------------------------------------------------------------------------------------------------- 7. samples
def test_stop_with_samples_of_one_prompt():
    _need_gpu()
    S = 64
    m = _flat_bar_head(_lm(S, 256, 2, 512, 4, 33, 'bf16', specials='off')).cuda()
    enc, emask = _prompts(4, S, seed=43)
    enc, emask = enc[[0, 2, 3]], emask[[0, 2, 3]]                       # prompts under which this model's bar moves between two or three values
    eng = m._get_engine()
    counts, owner = [3, 1, 2], [0, 0, 0, 1, 2, 2]
    seeds = [3000 + 5 * r for r in range(6)]
    idx = torch.as_tensor(owner)
    e6, m6 = enc[idx.cuda()], emask[idx.cuda()]
    whole, _, _ = _reference(eng, m, e6, m6, None, [0] * 6, None, None, seeds)
    stops = []
    for p in range(3):                                                 # one stop per PROMPT, chosen on the unstopped runs: the bar at which
        mine = [r for r in range(6) if owner[r] == p]                  # its samples stop at the most different positions
        cuts = lambda s_: [_cut(whole[r], 0, s_)[1] for r in mine]
        cands = sorted({int(v) + 1 for r in mine for v in whole[r][:_length(whole[r]), 0].tolist() if int(v) < 255})
        stops.append(max(cands, key=lambda s_: (len(set(cuts(s_))), sum(c is not None for c in cuts(s_)), -s_)))
    print('stop with samples: unstopped bars of prompt 0', [whole[r][:16, 0].tolist() for r in range(3)])
    want, w_state, w_info = _reference(eng, m, e6, m6, None, [0] * 6, None, [stops[p] for p in owner], seeds)
    got, g_state, info = _batched(eng, m, enc, emask, None, None, None, stops, seeds, samples=counts)
    lengths = [_length(got[r]) for r in range(6)]
    print('stop with samples: stops', stops, 'lengths', lengths)
    assert info['batched'] and info['groups'] == owner and info['encoder_passes'] == 3
    for r, p in enumerate(owner):
        assert torch.equal(got[r], want[r]) and _same_state(g_state[r], w_state[r]), r
        assert torch.equal(got[r], _cut(whole[r], 0, stops[p])[0]), r
        assert info['ended'][r] == w_info[r]['ended'], r
    assert len(set(lengths[:3])) > 1                                   # the samples of a prompt stop where their own bars say
    with pytest.raises(Exception, match='entries'):                    # `stop` describes the prompts, not the rows
        _batched(eng, m, enc, emask, None, None, None, [stops[p] for p in owner], seeds, samples=counts)


# ---------------------------------------------------------------------------------------------------------------- 8. refusals
@contextlib.contextmanager
def _dynamic_decoder(eng, enc, emask, n, slices):
    """A dynamic fused decoder of n rows and `slices` cross slices, every prompt of enc (<= slices) encoded and projected into the slice of
    its index, set up as _decoder_run sets one up. Yields (dec, em, s_enc)."""
    from pianobart_amd import ops
    from pianobart_amd._lib import LIB
    S, dev = int(enc.shape[1]), enc.device
    em, enc16 = eng._prompt_inputs(enc, emask)
    s_enc = [eng._key_extent(em[r:r + 1], S) for r in range(int(enc.shape[0]))]
    em_rows = em[:n].clone()                                           # the decoder's mask rows: alive as long as the decoder
    bp, bufs = eng._decode_plan(n, S, s_enc[:n], em_rows, dev, G=slices)
    dec = eng._decoder_create(bp)
    assert dec is not None
    try:
        LIB.call('pb_batch_decoder_dynamic', dec, slices)
        for g in range(int(enc.shape[0])):
            _, enc_out = eng.forward_hidden(enc16[g:g + 1], None, em[g:g + 1], None, False, 0)
            for l in range(eng.ND):
                eng._linear(enc_out, 'dec.%d.wkv_c' % l, 'dec.%d.bkv_c' % l, bufs['kvc'][l][g], S, 2 * eng.d, eng.d)
        LIB.call('pb_batch_decoder_reset', dec, ops._stream(), 1)
        torch.cuda.current_stream().synchronize()
        yield dec, em, s_enc
    finally:
        LIB.call('pb_batch_decoder_destroy', dec)


def test_stop_refusals_leave_the_decoder_working():
    """pb_batch_decoder_stop is refused before sampler_init, for a bar outside 0 .. 256 and after a step; pb_batch_decoder_admit_stop for a bad
    row, a bad bar and a decoder that is not dynamic. Host-side checks: a refused call enqueues nothing, names itself in pb_last_error,
    and the decoder goes on with the values it had."""
    _need_gpu()
    from pianobart_amd import ops
    from pianobart_amd._lib import LIB
    S, B = 64, 2
    m = _lm(S, 256, 2, 512, 4, 36, 'bf16', specials='off').cuda()
    enc, emask = _prompts(3, S, seed=46)
    eng = m._get_engine()
    tab = np.full((B, S, 8), -1, dtype=np.int16)
    tab[:, :, 0] = _bars(S)
    err = lambda: LIB.load().pb_last_error().decode()
    i32 = lambda *v: np.asarray(v, dtype=np.int32)
    n8, off8, pad8 = np.asarray(ops.SEG_SIZES, dtype=np.int32), np.asarray(ops.SEG_OFF[:8], dtype=np.int32), np.asarray(PAD, dtype=np.int32)
    t8, p8 = np.asarray(m.SAMPLE_T, dtype=np.float32), np.asarray(m.SAMPLE_P, dtype=np.float32)
    U = np.random.RandomState(0).random_sample((B, S * 8))
    first = np.ascontiguousarray(np.tile(np.asarray(SOS, dtype=np.int16), (B, 1)))
    last_pos, lim = np.full(B, -1, dtype=np.int32), np.full(B, S, dtype=np.int32)

    def init(dec):
        LIB.call('pb_batch_decoder_sampler_init', dec, t8.ctypes.data, p8.ctypes.data, n8.ctypes.data, off8.ctypes.data, pad8.ctypes.data,
                 U.ctypes.data, B * S * 8, S, -1, 0)
        LIB.call('pb_batch_decoder_force', dec, tab.ctypes.data)
        lp, tp = ctypes.c_void_p(), ctypes.c_void_p()
        LIB.call('pb_batch_decoder_logs', dec, ctypes.byref(lp), ctypes.byref(tp))
        return np.ctypeslib.as_array((ctypes.c_int16 * (B * S * 8)).from_address(tp.value)).reshape(B, S, 8)

    def steps(dec, count):
        tk = int(LIB.query('pb_batch_decoder_launch', dec, count, None))
        assert tk >= 0, err()
        LIB.call('pb_batch_decoder_wait', dec, tk)

    with torch.no_grad(), eng._decoder_run(enc[:B], emask[:B], [0, 0], None) as run:
        dec = run.dec
        assert dec is not None
        good = i32(2, PAD0)
        assert LIB.query('pb_batch_decoder_stop', dec, good.ctypes.data) < 0 and 'pb_batch_decoder_stop' in err() and 'sampler_init' in err()
        log_tok = init(dec)
        log_tok[:] = -7
        for bad in (i32(2, 257), i32(-1, 4)):
            assert LIB.query('pb_batch_decoder_stop', dec, bad.ctypes.data) < 0
            assert 'pb_batch_decoder_stop' in err() and 'bar %d' % (257 if bad[1] == 257 else -1) in err(), err()
        assert LIB.query('pb_batch_decoder_stop', dec, None) < 0 and 'pb_batch_decoder_stop' in err()
        assert LIB.query('pb_batch_decoder_admit_stop', dec, 0, 4) < 0 and 'pb_batch_decoder_admit_stop' in err() and 'not a dynamic decoder' in err()
        LIB.call('pb_batch_decoder_stop', dec, good.ctypes.data)      # row 0 stops at bar 2 (position 8), row 1 has no stop
        LIB.call('pb_batch_decoder_start', dec, last_pos.ctypes.data, first.ctypes.data, lim.ctypes.data)
        steps(dec, 4)
        assert LIB.query('pb_batch_decoder_stop', dec, i32(9, 9).ctypes.data) < 0 and 'pb_batch_decoder_stop' in err() and 'already issued' in err()
        steps(dec, 8)
        steps(dec, 4)                                                  # the run completes with the values of the good call
        got = log_tok.copy()
    assert np.array_equal(got[0, :9, 0], _bars(S)[:9]) and (got[0, 9:16] == -7).all()      # row 0: done behind position 8, nothing logged there
    assert np.array_equal(got[1, :16, 0], _bars(S)[:16]) and ((got[1, :16] >= 0) & (got[1, :16] < np.asarray(PAD))).all()

    u_row = np.random.RandomState(10).random_sample(S * 8)
    sos = np.asarray(SOS, dtype=np.int16)
    frow = np.ascontiguousarray(tab[0])
    with torch.no_grad(), _dynamic_decoder(eng, enc, emask, B, 3) as (dec, em, s_enc):
        assert LIB.query('pb_batch_decoder_admit_stop', dec, 0, 4) < 0 and 'pb_batch_decoder_admit_stop' in err() and 'sampler_init' in err()
        log_tok = init(dec)
        log_tok[:] = -7
        for row, bar, words in ((2, 4, 'row 2'), (-1, 4, 'row -1'), (0, 257, 'bar 257'), (1, -1, 'bar -1')):
            assert LIB.query('pb_batch_decoder_admit_stop', dec, row, bar) < 0
            assert 'pb_batch_decoder_admit_stop' in err() and words in err(), err()
        LIB.call('pb_batch_decoder_stop', dec, i32(1, PAD0).ctypes.data)   # row 0 stops at bar 1 (position 4)
        LIB.call('pb_batch_decoder_start', dec, last_pos.ctypes.data, first.ctypes.data, lim.ctypes.data)
        steps(dec, 8)
        assert (log_tok[0, 5:8] == -7).all() and np.array_equal(log_tok[0, :5, 0], _bars(S)[:5])
        LIB.call('pb_batch_decoder_seek', dec, 0, 4, None)
        mask_row = np.ascontiguousarray(em[2].cpu().numpy(), dtype=np.float32)
        log_tok[0] = -7
        # an admission without a staged value: the new occupant has no stop, whatever the slot's previous one had
        LIB.call('pb_batch_decoder_admit', dec, 0, 2, s_enc[2], -1, sos.ctypes.data, S, u_row.ctypes.data, frow.ctypes.data, mask_row.ctypes.data,
                 ops._stream())
        steps(dec, 8)
        steps(dec, 4)
        got = log_tok.copy()
    assert np.array_equal(got[0, :12, 0], _bars(S)[:12])               # bars 1 and 2 did not stop it
    assert np.array_equal(got[1, :20, 0], _bars(S)[:20])


# ---------------------------------------------------------------------------------------------------------------- 9. the command line
def _dataset(tmp_path, N, S):
    """N pieces whose bar is i // 4 over their ordinary rows (sorted, several bars), EOS row and PAD tail as synth_octuple_batch makes them."""
    x = synth_octuple_batch(N, S, seed=5, min_len=S // 2)[5].numpy()
    for i in range(N):
        e = int(np.flatnonzero(x[i, :, 0] >= PAD0)[0])
        x[i, :e, 0] = _bars(S)[:e]
    np.save(str(tmp_path / 'prompts.npy'), x)
    base = ['--dataset_path', str(tmp_path), '--dataset_name', 'prompts.npy', '--max_seq_len', str(S), '--hs', '256', '--layers', '2',
            '--ffn_dims', '512', '--heads', '4', '--nopretrain', '--seed', '0']
    return x, base


def _run_cli(tmp_path, base, name, *extra):
    from pianobart_amd import eval_generation as EG
    torch.manual_seed(0)
    out = str(tmp_path / name)
    EG.eval_generation(EG.get_args(base + ['--output', out] + list(extra)))
    return out


def test_eval_generation_bars(tmp_path):
    _need_gpu()
    from pianobart_amd import eval_generation as EG
    S, N = 48, 9
    x, base = _dataset(tmp_path, N, S)
    base = base + ['--prime', 'half', '--bars', '2']
    a = _run_cli(tmp_path, base, 'b1.npy', '--batch_size', '1')
    b = _run_cli(tmp_path, base, 'b16.npy', '--batch_size', '16')
    c = _run_cli(tmp_path, base, 'br.npy', '--batch_size', '4', '--refill', '4')
    assert open(a, 'rb').read() == open(b, 'rb').read() == open(c, 'rb').read()
    y = np.load(a)
    assert y.shape == (N, S, 8) and y.dtype == np.float32
    for i, k in enumerate(EG.prime_lengths(x, 'half', PAD0, PAD)):
        n, q = _length(y[i]), int(x[i, k - 1, 0])
        assert k > 0 and n >= k and np.array_equal(y[i, :k], x[i, :k].astype(np.float32)), i
        assert (y[i, k:n, 0] < q + 3).all(), i                         # the bar the prime ends in and 2 new ones, nothing behind them


def test_eval_generation_infill(tmp_path, capsys):
    _need_gpu()
    S, N = 48, 9
    x, base = _dataset(tmp_path, N, S)
    base = base + ['--infill', '2:4']
    a = _run_cli(tmp_path, base, 'i1.npy', '--batch_size', '1')
    printed = capsys.readouterr().out
    b = _run_cli(tmp_path, base, 'i16.npy', '--batch_size', '16')
    c = _run_cli(tmp_path, base, 'ir.npy', '--batch_size', '4', '--refill', '4')
    assert open(a, 'rb').read() == open(b, 'rb').read() == open(c, 'rb').read()
    y = np.load(a)
    assert y.shape == (N, S, 8) and y.dtype == np.float32
    truncated = 0
    for i in range(N):
        e = int(np.flatnonzero(x[i, :, 0] >= PAD0)[0])
        k, mm = int((x[i, :e, 0] < 2).sum()), int((x[i, :e, 0] < 4).sum())
        suffix = x[i, mm:e + 1].astype(np.float32)                     # the rows of bars >= 4 and the EOS row
        n = _length(y[i]) if (y[i, :, 0] == PAD0).any() else S
        assert k == 8 and np.array_equal(y[i, :k], x[i, :k].astype(np.float32)), i
        if n >= len(suffix) + k and np.array_equal(y[i, n - len(suffix):n], suffix):
            assert (y[i, k:n - len(suffix), 0] < 4).all(), i           # what was written in between stays below the stop bar
        else:
            assert n == S, i                                           # cut at the window: reported
            truncated += 1
    assert 'Truncated pieces: %d' % truncated in printed
