"""GPU: time-ordered generation -- Engine.generate(order=...), Engine.generate_batch(order=...), PianoBartLM's decoder_order,
pb_batch_decoder_order / pb_batch_decoder_admit_order, eval_generation --ordered.

Contract ("Time-ordered sampling"): `order` is one integer per row, -1 = the row is sampled as ever, f_b = 0 .. 255 = the
row is time-ordered with bar floor f_b. The result is the reference loop (model.py:42-65) with `current_output = self.sample(x, i)` replaced
by the ordered sample: with prev = the decoder's input row at position i, head 0's classes below max(f_b, prev's bar) and -- where the
token's bar after forcing equals prev's -- head 1's classes below prev's position have probability exactly 0. So over the emitted
positions >= k_b of an ordered row the pairs (bar, position) never decrease and every bar is >= f_b, except where a given head says
otherwise. Both forms of the device sampler (dec_sample_kernel) apply the mask, and the host's verification decides.

The bar and position heads sample at p = 1 (an arg-max). Their random bias would pin them to one class, so the models here have it
flattened over the ordinary ids of both heads (_flat_heads). That alone is not enough: with the random weights of golden_util the
decoder's sublayers put a component into the hidden state that hardly depends on the position, the arg-max settles on two or three
classes and a free row goes back at 0 .. 15 of 48 positions, depending on the prompt. So the models also get their decoder's sublayer
outputs (out_proj of both attentions, fc2) scaled by 0.1 (_thin_decoder): the hidden state then follows the decoder's input token, whose
nucleus-sampled heads differ from position to position, and the (bar, position) of a free row wanders over the whole table: 22 .. 26 of
48 positions go back (the float32 oracle, 3 model seeds x 8 prompts). Every kernel of the step still runs on non-trivial numbers."""
import numpy as np
import pytest
import torch

from tests.test_bar_stop_gpu import PAD, PAD0, SOS, _free, _length, _lm, _need_gpu, _piece, _prompts, _same_state, _sampler
from tests.test_ordered_generation_cpu import _reference_token

pytestmark = pytest.mark.gpu
S = 48
PADV = np.asarray(PAD)


def _flat_heads(m):
    """A model made on the CPU (before .cuda() and the engine) without the bias of the ordinary ids of the bar and the position head (see
    the module's docstring; tests/test_bar_stop_gpu.py does it for the bar head)."""
    with torch.no_grad():
        m.mask_lm.proj[0].bias[:PAD[0]] = 0.0
        m.mask_lm.proj[1].bias[:PAD[1]] = 0.0
    return m


def _thin_decoder(m, c=0.1):
    """The decoder's sublayer outputs scaled by c, on the CPU model (see the module's docstring)."""
    n = 0
    with torch.no_grad():
        for name, p in m.named_parameters():
            if '.decoder.layers.' in name and ('out_proj' in name or 'fc2' in name):
                p.mul_(c)
                n += 1
    assert n == 12, n                                                  # 2 layers x (self out_proj, cross out_proj, fc2) x (weight, bias)
    return m


def _model(seed, precision, specials='off'):
    return _thin_decoder(_flat_heads(_lm(S, 256, 2, 256, 4, seed, precision, specials=specials))).cuda()


def _prime(k, seed, bar=1):
    """k ordinary rows in time order: bars 0 .. `bar`, positions rising."""
    p = _piece(k, seed)
    p[:, 0] = torch.as_tensor(np.minimum(np.arange(k) // 2, bar))
    p[:, 1] = torch.as_tensor((np.arange(k) % 2) * 30 + 7)
    return p


def _violations(row, k=0, floor=0):
    """The emitted positions i >= k of one output row at which it breaks the ordered contract: a bar below the floor, or a (bar, position)
    below that of the row in front (the prime's last row at k; nothing at 0)."""
    x = np.asarray(row.cpu() if isinstance(row, torch.Tensor) else row).astype(np.int64)
    n = _length(x)
    t = x[:, 0] * 1024 + x[:, 1]
    return [i for i in range(k, n) if x[i, 0] < floor or (i > 0 and t[i] < t[i - 1])]


def _ordered(G, row, k, f):
    return G.is_time_ordered(row, start=k, floor=max(f, 0))


def _batched(eng, m, enc, emask, seeds, order, prefix=None, lens=None, forced=None, stop=None, **kw):
    rngs = [np.random.RandomState(s) for s in seeds]
    out = eng.generate_batch(enc, emask, m.sample_row, rngs, sampler=_sampler(m), prefix=prefix, prefix_len=lens, forced=forced, stop=stop,
                             order=order, **kw).cpu()
    return out, [r.get_state() for r in rngs], dict(eng.last_decode)


def _per_prompt(eng, m, enc, emask, seeds, order, prefix=None, lens=None, forced=None, stop=None, rows=None, max_new=None):
    """Row b through the batch-1 `generate` of its prompt under its own generator: (tokens, generator state, last_decode) per row."""
    outs, states, infos = {}, {}, {}
    for b in (range(len(seeds)) if rows is None else rows):
        np.random.set_state(np.random.RandomState(seeds[b]).get_state())
        outs[b] = eng.generate(enc[b:b + 1], emask[b:b + 1], m.sample_row, sampler=_sampler(m), max_new=max_new,
                               prefix=prefix[b:b + 1, :lens[b]] if prefix is not None and lens[b] else None,
                               forced=forced[b:b + 1] if forced is not None else None, stop=stop[b] if stop is not None else PAD0,
                               order=order[b] if order is not None else None).cpu()[0]
        states[b] = np.random.get_state()
        infos[b] = dict(eng.last_decode)
    return outs, states, infos


# ---------------------------------------------------------------------------------------------------------------- 1. + 2. paths, reference
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_ordered_paths_agree_and_equal_the_restated_reference(precision):
    """One prompt, primed with 6 rows whose last bar (1) is below the floor (3). generate (bf16: the fused decoder, device-sampled with the
    sampler named and host-sampled without; fp32: the pb_decode_step loop), _generate_nocache, _generate_pyloop and generate_batch of the
    one row. Then every path's row is rebuilt position by position from the logits rows its host saw, with the restatement of
    tests/test_ordered_generation_cpu.py: bit for bit."""
    _need_gpu()
    from pianobart_amd import generation as G
    k, f = 6, 3
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
    a = run(lambda: eng.generate(enc, emask, recording, order=f, **base))
    s = run(lambda: eng.generate(enc, emask, recording, sampler=_sampler(m), order=f, **base))
    b = run(lambda: eng.generate(enc, emask, recording, use_cache=False, order=f, **base))
    c = run(lambda: eng._generate_pyloop(enc, emask, recording, k, pre, None, None, f))
    rng = np.random.RandomState(5)
    del seen[:]
    g_out = eng.generate_batch(enc, emask, recording, [rng], sampler=_sampler(m), prefix=pre[None], prefix_len=[k], stop=[PAD0], order=[f]).cpu()
    g = (g_out, rng.get_state(), dict(eng.last_decode), list(seen))
    free = run(lambda: eng.generate(enc, emask, recording, sampler=_sampler(m), **base))
    print('ordered paths (%s): bars' % precision, a[0][0, :, 0].tolist(), 'positions', a[0][0, :, 1].tolist(), 'free bars', free[0][0, :, 0].tolist(),
          'violations of the free row', len(_violations(free[0][0], k, f)), 'rewinds', (s[2] or {}).get('rewinds'), g[2].get('rewinds'))
    assert len(_violations(free[0][0], k, f)) >= 10                   # the constraint bites on this prompt
    print('ordered paths (%s): equal to generate:' % precision, {name: bool(torch.equal(a[0], other[0])) for name, other in
                                                                (('device-sampled', s), ('nocache', b), ('pyloop', c), ('generate_batch', g))})
    # fp32 (exact f32 arithmetic on every path): all five are one row. bf16: nocache and pyloop run the training kernels, whose bf16 rounding
    # is not the fused decoder's; on this model, whose arg-max wanders over nearly flat logits, their rows leave the fused decoder's after a
    # few positions (seen on an MI355X), which tests/test_bar_stop_gpu.py allows for as well. They are held to the
    # restatement below instead, each from the logits rows of its own run.
    same = ('device-sampled', 'nocache', 'pyloop', 'generate_batch') if precision == 'fp32' else ('device-sampled', 'generate_batch')
    runs = {'generate': a, 'device-sampled': s, 'nocache': b, 'pyloop': c, 'generate_batch': g}
    for name in same:
        assert torch.equal(a[0], runs[name][0]), name
        assert _same_state(a[1], runs[name][1]), name
    if precision == 'bf16':                                            # the fused decoder's record (fp32 runs the pb_decode_step loop: no record)
        assert a[2]['ended'] == s[2]['ended'] == g[2]['ended'][0] and s[2]['device_sampler'] and s[2]['rewinds'] <= 2
    # 2. the restated reference, from the logits rows the host of each run sampled from (one per position, in position order: the host
    # samples every position once, whatever the device predicted)
    for name, (out, state, _, rows) in runs.items():
        out = out[0]
        n = _length(out)
        assert torch.equal(out[:k], pre) and n > k + 10 and _ordered(G, out, k, f) and not _violations(out, k, f), name
        assert len(rows) == S - k and all('order' in kw for _, kw in rows), name
        np.random.seed(5)
        prev = pre[k - 1].numpy()
        for i, (row, _) in enumerate(rows):
            tok = _reference_token(row, prev, f, None)
            if (tok.numpy() >= PADV).any():
                assert k + i == n, (name, i, tok)                      # the token that ended the row
                break
            assert torch.equal(tok, out[k + i]), (name, k + i, tok, out[k + i])
            prev = tok.numpy()
        assert _same_state(np.random.get_state(), state), name


# ---------------------------------------------------------------------------------------------------------------- 3. + 4. property, device
MIXED_MODEL, MIXED_PROMPTS = 32, 41
MIXED_FLOORS = [0, -1, 3, 0, 100, -1, 0, 255, 0, 7, -1, 0, 40, 0, -1, 0]
MIXED_LENS = [0, 0, 6, 0, 0, 0, 0, 0, 0, 6, 0, 0, 0, 0, 0, 0]


def _mixed():
    m = _model(MIXED_MODEL, 'bf16')
    enc, emask = _prompts(16, S, seed=MIXED_PROMPTS)
    prefix = torch.stack([_prime(6, 900 + b) for b in range(16)])
    return m, enc, emask, prefix, list(range(300, 316))


def test_ordered_rows_are_ordered_and_the_device_knows_it():
    """16 rows with mixed floors, -1 rows among them, two rows primed. Every ordered row is in time order from its prime on and stays at or
    above its floor; the -1 rows are the rows of the call without `order`; the unordered run of the same prompts and seeds breaks the
    contract at >= 10 positions of EVERY ordered row, so a device sampler that ignored the mask would be rewound >= 10 times per row --
    the run's rewinds stay within the project's bar for a whole row (tests/test_model_gpu.py: <= 2). The same for a B = 1 `generate`."""
    _need_gpu()
    from pianobart_amd import generation as G
    m, enc, emask, prefix, seeds = _mixed()
    eng = m._get_engine()
    got, g_state, info = _batched(eng, m, enc, emask, seeds, MIXED_FLOORS, prefix, MIXED_LENS)
    free, f_state, f_info = _batched(eng, m, enc, emask, seeds, None, prefix, MIXED_LENS)
    bites = [len(_violations(free[b], MIXED_LENS[b], max(MIXED_FLOORS[b], 0))) for b in range(16)]
    print('ordered batch: violations of the unordered rows', bites, 'rewinds', info['rewinds'], 'unordered rewinds', f_info['rewinds'],
          'lengths', [_length(got[b]) for b in range(16)])
    assert info['batched'] and info['batch'] == 16 and info['launches_per_token'] == f_info['launches_per_token'] == 6 * 2 + 3
    for b, f in enumerate(MIXED_FLOORS):
        k = MIXED_LENS[b]
        if f < 0:
            assert torch.equal(got[b], free[b]) and _same_state(g_state[b], f_state[b]), b
            continue
        assert bites[b] >= 10, (b, bites)
        assert _ordered(G, got[b], k, f) and not _violations(got[b], k, f), b
        assert _length(got[b]) > k and (got[b][k:_length(got[b]), 0] >= f).all(), b
        assert torch.equal(got[b][:k], prefix[b, :k]), b
        assert _same_state(g_state[b], f_state[b]) or _length(got[b]) != _length(free[b]), b     # the draws do not move: same length, same state
    assert all(r <= 2 for r in info['rewinds']), info['rewinds']
    b = 4                                                              # B = 1: the single-row sampler
    want, w_state, w_info = _per_prompt(eng, m, enc, emask, seeds, MIXED_FLOORS, prefix, MIXED_LENS, rows=[b, 2])
    for r in (b, 2):
        assert torch.equal(want[r], got[r]) and _same_state(w_state[r], g_state[r]), r
        assert w_info[r]['device_sampler'] and w_info[r]['rewinds'] <= 2, (r, w_info[r]['rewinds'])


# ---------------------------------------------------------------------------------------------------------------- 5. rewind
def test_rewind_of_an_ordered_row():
    """The device's bar id of one ordered row is corrupted (+ 1) at every third position (the sampler's fault_period: test-only injection of
    its choice, no GPU fault is involved). The host's token wins: the row is its fault-free row, and the rewound row's next mask is built
    from the host's token (pb_batch_decoder_seek puts it into the row's decoder input). The other rows' rewinds do not move."""
    _need_gpu()
    from pianobart_amd import generation as G
    m, enc, emask, prefix, seeds = _mixed()
    enc, emask, seeds, floors, fr = enc[:4], emask[:4], seeds[:4], [0, -1, 3, 0], 2
    eng = m._get_engine()
    clean, c_state, c_info = _batched(eng, m, enc, emask, seeds, floors)
    eng.decode_fault_row = (fr, 3)
    try:
        got, g_state, g_info = _batched(eng, m, enc, emask, seeds, floors)
    finally:
        eng.decode_fault_row = None
    print('rewind of an ordered row: rewinds', g_info['rewinds'], 'clean', c_info['rewinds'])
    for b in range(4):
        assert torch.equal(got[b], clean[b]) and _same_state(g_state[b], c_state[b]), b
        assert floors[b] < 0 or _ordered(G, got[b], 0, floors[b]), b
        if b != fr:
            assert g_info['rewinds'][b] == c_info['rewinds'][b], b
    assert g_info['rewinds'][fr] > c_info['rewinds'][fr]


# ---------------------------------------------------------------------------------------------------------------- 6. no order
def test_no_order_is_todays_call():
    """order=None and -1 everywhere: the tokens, generator states, launches and record of the call without the argument."""
    _need_gpu()
    m = _model(32, 'bf16', specials='eos')
    enc, emask = _prompts(5, S, seed=41)
    eng = m._get_engine()
    seeds = [11, 12, 13, 14, 15]
    rngs = [np.random.RandomState(s) for s in seeds]
    want = eng.generate_batch(enc, emask, m.sample_row, rngs, sampler=_sampler(m)).cpu()
    w_info = dict(eng.last_decode)
    for order in (None, [-1] * 5, np.full(5, -1), torch.full((5,), -1)):
        got, states, info = _batched(eng, m, enc, emask, seeds, order)
        assert torch.equal(got, want)
        assert all(_same_state(a, r.get_state()) for a, r in zip(states, rngs))
        for key in ('launches_per_token', 'graph', 'tokens', 'steps', 'batch', 'batched', 'tokens_per_graph_replay'):
            assert info[key] == w_info[key], key
        assert set(info) == set(w_info)
    np.random.seed(9)
    a = eng.generate(enc[:1], emask[:1], m.sample_row, sampler=_sampler(m)).cpu()
    a_info, sa = dict(eng.last_decode), np.random.get_state()
    for order in (None, -1, [-1]):
        np.random.seed(9)
        b = eng.generate(enc[:1], emask[:1], m.sample_row, sampler=_sampler(m), order=order).cpu()
        assert torch.equal(a, b) and _same_state(sa, np.random.get_state())
        assert all(eng.last_decode[key] == a_info[key] for key in ('launches_per_token', 'graph', 'tokens'))
        assert set(eng.last_decode) == set(a_info)
    plain = lambda row, rng=None: m.sample_row(row, rng)                 # a caller's sample_row without the keyword: never handed it
    rngs2 = [np.random.RandomState(s) for s in seeds]
    assert torch.equal(eng.generate_batch(enc, emask, plain, rngs2, sampler=_sampler(m), order=[-1] * 5).cpu(), want)


# ---------------------------------------------------------------------------------------------------------------- 7. the neighbours
def _free_heads_keep_order(row, frow, floor):
    """The contract position by position, for a row with given heads: where head 0 is free its bar is >= max(floor, the previous bar); where
    head 1 is free and the bar is the previous row's, its position is >= the previous one. Returns the positions that break it."""
    x = np.asarray(row).astype(np.int64)
    bad = []
    for i in range(_length(x)):
        prev = x[i - 1] if i else np.asarray(SOS)
        bar = prev[0] < PAD[0]
        if frow[i, 0] < 0 and x[i, 0] < max(floor, prev[0] if bar else 0):
            bad.append(i)
        if frow[i, 1] < 0 and bar and prev[1] < PAD[1] and x[i, 0] == prev[0] and x[i, 1] < prev[1]:
            bad.append(i)
    return bad


def test_order_with_stop_and_forced():
    """6 rows: bars given at positions 10 .. 19 (wherever the free bars in front of them have got to: a given head is never masked or
    changed, and the row goes on from it), free elsewhere; positions given at 24 .. 27; a stop bar on some rows. Each row against the
    per-prompt `generate` of the row."""
    _need_gpu()
    m = _model(32, 'bf16')
    enc, emask = _prompts(6, S, seed=41)
    eng = m._get_engine()
    forced = _free(6, S)
    forced[:, 10:20, 0] = [20, 20, 21, 22, 22, 9, 22, 23, 23, 24]      # position 15 goes back to bar 9: the caller's business
    forced[:, 24:28, 1] = [5, 3, 90, 90]
    floors = [0, 4, -1, 0, 30, 0]
    stops = [PAD0, 256, 200, 240, PAD0, 128]
    seeds = list(range(500, 506))
    want, w_state, w_info = _per_prompt(eng, m, enc, emask, seeds, floors, forced=forced, stop=stops)
    got, g_state, info = _batched(eng, m, enc, emask, seeds, floors, forced=forced, stop=stops)
    print('order + stop + forced: lengths', [_length(got[b]) for b in range(6)], 'ended', info['ended'], 'rewinds', info['rewinds'],
          'bars of row 0', got[0][:, 0].tolist())
    for b in range(6):
        assert torch.equal(got[b], want[b]) and _same_state(g_state[b], w_state[b]) and info['ended'][b] == w_info[b]['ended'], b
        n = _length(got[b])
        given = forced[b, :n] >= 0
        assert (got[b][:n].numpy()[given] == forced[b, :n][given]).all(), b
        if floors[b] >= 0:
            assert not _free_heads_keep_order(got[b], forced[b], floors[b]), b
    assert 'bar' in info['ended'] and _length(got[0]) == S and _length(got[4]) == S      # rows stop by their bar; rows without a stop fill the window


def test_order_with_samples_of_one_prompt():
    _need_gpu()
    from pianobart_amd import generation as G
    m = _model(33, 'bf16')
    enc, emask = _prompts(3, S, seed=43)
    eng = m._get_engine()
    counts, owner = [3, 1, 2], [0, 0, 0, 1, 2, 2]
    floors = [0, -1, 50]                                               # per PROMPT, expanded through the owner map
    seeds = [3000 + 5 * r for r in range(6)]
    idx = torch.as_tensor(owner).cuda()
    want, w_state, _ = _per_prompt(eng, m, enc[idx], emask[idx], seeds, [floors[p] for p in owner])
    got, g_state, info = _batched(eng, m, enc, emask, seeds, floors, samples=counts)
    assert info['batched'] and info['groups'] == owner and info['encoder_passes'] == 3
    for r, p in enumerate(owner):
        assert torch.equal(got[r], want[r]) and _same_state(g_state[r], w_state[r]), r
        assert floors[p] < 0 or (_ordered(G, got[r], 0, floors[p]) and _length(got[r]) > 10), r
    with pytest.raises(Exception, match='entries'):                    # `order` describes the prompts, not the rows
        _batched(eng, m, enc, emask, seeds, [floors[p] for p in owner], samples=counts)


def test_order_under_refill():
    """10 prompts in 4 slots: rows 0 .. 3 are ordered with floor 200, rows 4 .. 7 are free, rows 8 and 9 have floors 5 and -1. Whatever slot
    a free row gets, its previous occupant was a floor-200 row: a leaked floor would push its bars to 200 and beyond. Row 8 (floor 5)
    follows a free row, and must not stay free."""
    _need_gpu()
    from pianobart_amd import generation as G
    m = _model(34, 'bf16')
    enc, emask = _prompts(10, S, seed=44)
    eng = m._get_engine()
    floors = [200] * 4 + [-1] * 4 + [5, -1]
    seeds = list(range(70, 80))
    want, w_state, _ = _per_prompt(eng, m, enc, emask, seeds, floors, max_new=20)
    plain, p_state, _ = _batched(eng, m, enc, emask, seeds, floors, refill=False, max_new=20)
    got, g_state, info = _batched(eng, m, enc, emask, seeds, floors, refill=4, max_new=20)
    print('order under refill: lengths', [_length(got[b]) for b in range(10)], 'slots', info['row_slot'], 'rewinds', info['rewinds'])
    assert info['refill'] == 4 and info['admissions'] == 6
    for b in range(10):
        assert torch.equal(got[b], want[b]) and torch.equal(plain[b], want[b]), b
        assert _same_state(g_state[b], w_state[b]) and _same_state(p_state[b], w_state[b]), b
        if floors[b] >= 0:
            assert _ordered(G, got[b], 0, floors[b]), b
    for b in range(4, 8):                                              # the free successors of the floor-200 rows
        assert 0 <= info['row_slot'][b] < 4 and _length(got[b]) > 0 and int(got[b][:_length(got[b]), 0].min()) < 200, b
    assert _length(got[8]) > 0 and int(got[8][:_length(got[8]), 0].min()) >= 5


# ---------------------------------------------------------------------------------------------------------------- 8. the command line
def _dataset(tmp_path, N):
    """N pieces in time order: bar i // 4 and rising positions over their ordinary rows, the EOS row and PAD tail as synth_octuple_batch makes them."""
    from tests.golden_util import synth_octuple_batch
    x = synth_octuple_batch(N, S, seed=5, min_len=S // 2)[5].numpy()
    for i in range(N):
        e = int(np.flatnonzero(x[i, :, 0] >= PAD0)[0])
        x[i, :e, 0], x[i, :e, 1] = np.arange(e) // 4, (np.arange(e) % 4) * 20
    np.save(str(tmp_path / 'prompts.npy'), x)
    base = ['--dataset_path', str(tmp_path), '--dataset_name', 'prompts.npy', '--max_seq_len', str(S), '--hs', '256', '--layers', '2',
            '--ffn_dims', '256', '--heads', '4', '--nopretrain', '--seed', '0', '--batch_size', '16', '--infill', '2:4']
    return x, base


def test_eval_generation_ordered(tmp_path):
    _need_gpu()
    from pianobart_amd import eval_generation as EG
    from pianobart_amd import generation as G
    N = 6
    x, base = _dataset(tmp_path, N)

    def run(name, *extra, strip=False):
        torch.manual_seed(0)
        out = str(tmp_path / name)
        args = EG.get_args(base + ['--output', out] + list(extra))
        if strip:
            del args.ordered                                           # the namespace a caller built before the flag existed
        EG.eval_generation(args)
        return out
    o = run('o.npy', '--ordered')
    p = run('p.npy')
    q = run('q.npy', strip=True)
    assert open(p, 'rb').read() == open(q, 'rb').read()                # without the flag: the bytes of a run that never heard of it
    y, free = np.load(o), np.load(p)
    assert y.shape == (N, S, 8) and y.dtype == np.float32
    for i in range(N):
        assert G.is_time_ordered(x[i]), i
        assert G.is_time_ordered(y[i]) and G.is_time_ordered(y[i], start=8, floor=2), i      # every written piece; its new rows stay in bars >= 2
        assert np.array_equal(y[i, :8], x[i, :8].astype(np.float32)), i
    print('eval_generation --ordered: pieces of the run without the flag that are out of order:', sum(not G.is_time_ordered(free[i]) for i in range(N)))
