"""GPU: anchored generation -- Engine.generate(anchors=...), Engine.generate_batch(anchors=...), PianoBartLM's decoder_anchors,
pb_batch_decoder_anchor / _admit_anchor / _seek_anchor / _anchors_placed, eval_generation --accompany.

Contract ("Anchored notes"): a row may carry a list of complete tokens in (bar, position) order. Every position is
sampled as without them (the candidate); while anchors remain, a candidate that would end the row or whose (bar, position) has reached the
next anchor's gives way to that anchor. So every anchor is written, in order, the row is time-ordered, and it cannot end while one remains.
The device sampler applies the rule in its last stage and keeps the row's counter; the host's verification decides, and restores the
counter where it rewinds a row.

The models are the S = 48 ones of tests/test_ordered_generation_gpu.py, whose (bar, position) wanders over the whole table."""
import numpy as np
import pytest
import torch

from tests.test_bar_stop_gpu import PAD, PAD0, _length, _need_gpu, _piece, _prompts, _same_state, _sampler
from tests.test_ordered_generation_cpu import _reference_token
from tests.test_ordered_generation_gpu import S, _model, _prime

pytestmark = pytest.mark.gpu
PADV = np.asarray(PAD)
PAD_T = torch.as_tensor(PADV)


def _anchors(times, seed):
    """Anchors at the given (bar, position) times: the other heads from a seeded piece."""
    a = _piece(len(times), seed).clone()
    for i, (bar, pos) in enumerate(times):
        a[i, 0], a[i, 1] = bar, pos
    return a.numpy().astype(np.int64)


PATH_TIMES = [(1, 40), (2, 5), (5, 0), (5, 0), (20, 64), (60, 3), (90, 100), (90, 101)]


# ---------------------------------------------------------------------------------------------------------------- 1. paths, restatement
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_anchored_paths_agree_and_equal_the_restatement(precision):
    """One prompt, primed with 6 rows that end at (1, 37), 8 anchors from (1, 40) on. generate (bf16: the fused decoder, device-sampled with
    the sampler named and host-sampled without; fp32: the pb_decode_step loop), _generate_nocache, _generate_pyloop and generate_batch of
    the one row. Then every path's row is rebuilt position by position from the logits rows its host saw: the restated ordered sample of
    tests/test_ordered_generation_cpu.py gives the candidate, anchored_token decides what is written."""
    _need_gpu()
    from pianobart_amd import generation as G
    k = 6
    m = _model(78, precision)
    enc, emask = _prompts(1, S, seed=4)
    pre = _prime(k, 5)
    A = _anchors(PATH_TIMES, 17)
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

    base = dict(prefix=pre[None], stop=PAD0, anchors=A)
    a = run(lambda: eng.generate(enc, emask, recording, **base))
    s = run(lambda: eng.generate(enc, emask, recording, sampler=_sampler(m), **base))
    b = run(lambda: eng.generate(enc, emask, recording, use_cache=False, **base))
    c = run(lambda: eng._generate_pyloop(enc, emask, recording, k, pre, None, None, 0, None, None, torch.as_tensor(A)))
    rng = np.random.RandomState(5)
    del seen[:]
    g_out = eng.generate_batch(enc, emask, recording, [rng], sampler=_sampler(m), prefix=pre[None], prefix_len=[k], stop=[PAD0], anchors=[A]).cpu()
    g = (g_out, rng.get_state(), dict(eng.last_decode), list(seen))
    print('anchored paths (%s): bars' % precision, a[0][0, :, 0].tolist(), 'positions', a[0][0, :, 1].tolist(), 'rewinds', (s[2] or {}).get('rewinds'),
          g[2].get('rewinds'), 'placed', (s[2] or {}).get('anchors_placed'), g[2].get('anchors_placed'))
    # fp32: all five are one row. bf16: nocache and pyloop run the training kernels, whose rounding is not the fused decoder's (the remark of
    # tests/test_ordered_generation_gpu.py); they are held to the restatement below, each from the logits rows of its own run.
    same = ('device-sampled', 'nocache', 'pyloop', 'generate_batch') if precision == 'fp32' else ('device-sampled', 'generate_batch')
    runs = {'generate': a, 'device-sampled': s, 'nocache': b, 'pyloop': c, 'generate_batch': g}
    for name in same:
        assert torch.equal(a[0], runs[name][0]), name
        assert _same_state(a[1], runs[name][1]), name
    if precision == 'bf16':                                            # the fused decoder's record (fp32 runs the pb_decode_step loop: no record)
        assert a[2]['anchors_placed'] == s[2]['anchors_placed'] == g[2]['anchors_placed'] == [len(A)]
        assert s[2]['device_sampler'] and s[2]['rewinds'] <= 2 and g[2]['rewinds'][0] <= 2
    sv = G.stop_vector(PAD_T, None)
    for name, (out, state, _, rows) in runs.items():
        out = out[0]
        n = _length(out)
        assert torch.equal(out[:k], pre) and n > k + 10, name
        assert G.follows_anchors(out, A, start=k) == (True, len(A)) and G.is_time_ordered(out, start=k), name
        assert len(rows) == S - k and all('order' in kw for _, kw in rows), name
        np.random.seed(5)
        prev, placed = pre[k - 1].numpy(), 0
        for i, (row, _) in enumerate(rows):
            tok, placed = G.anchored_token(_reference_token(row, prev, 0, None), torch.as_tensor(A), placed, sv, PAD_T)
            if (tok.numpy() >= PADV).any():
                assert k + i == n, (name, i, tok)                      # the token that ended the row
                break
            assert torch.equal(tok, out[k + i]), (name, k + i, tok, out[k + i])
            prev = tok.numpy()
        assert placed == len(A) and _same_state(np.random.get_state(), state), name


# ---------------------------------------------------------------------------------------------------------------- 2. the mixed batch
MIXED_LENS = [0, 0, 6, 0, 0, 0, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0]


def _mixed(specials='eos'):
    """16 rows: free (0, 5, 10), ordered without anchors (1), anchored (2 primed, 3, 4, 11 .. 15), anchored + mask (6, 7 primed), anchored +
    schedule (8), anchored + stop (9)."""
    from pianobart_amd import generation as G
    from tests.golden_util import load_vocab
    m = _model(32, 'bf16', specials=specials)
    enc, emask = _prompts(16, S, seed=41)
    prefix = torch.stack([_prime(6, 900 + b) for b in range(16)])
    e2w = load_vocab()[0]
    anchors = [None] * 16
    for b, times in ((2, [(1, 37), (3, 0), (3, 0), (40, 9)]), (3, [(0, 0)]), (4, [(0, 50), (2, 2), (2, 90), (7, 7), (30, 1), (30, 1), (31, 0), (50, 5)]),
                     (6, [(4, 4), (9, 9)]), (7, [(2, 0), (2, 64), (80, 1)]), (8, [(0, 5), (1, 5), (2, 5), (3, 5)]), (9, [(1, 1), (5, 100), (11, 0)]),
                     (11, [(10, 10)]), (12, [(0, 1), (0, 2), (0, 3)]), (13, [(100, 0), (100, 64)]), (14, [(3, 3), (60, 6)]), (15, [(25, 25)])):
        anchors[b] = _anchors(times, 50 + b)
    order = [-1, 0] + [-1] * 14
    allow = [None] * 16
    allow[6] = allow[7] = G.allow_mask(e2w, pitch_range=(60, 128))     # the anchors' pitches are not held to it
    bar_allow = [None] * 16
    bar_allow[8] = G.chord_schedule(e2w, ['C:maj', 'G:maj'])
    stop = [PAD0] * 16
    stop[9] = 12
    return m, enc, emask, prefix, list(range(300, 316)), dict(anchors=anchors, order=order, allow=allow, bar_allow=bar_allow, stop=stop)


def _batched(eng, m, enc, emask, seeds, rules, prefix=None, lens=None, **kw):
    rngs = [np.random.RandomState(s) for s in seeds]
    out = eng.generate_batch(enc, emask, m.sample_row, rngs, sampler=_sampler(m), prefix=prefix, prefix_len=lens, **rules, **kw).cpu()
    return out, [r.get_state() for r in rngs], dict(eng.last_decode)


def _per_prompt(eng, m, enc, emask, seeds, rules, prefix=None, lens=None, rows=None, max_new=None):
    outs, states, infos = {}, {}, {}
    for b in (range(len(seeds)) if rows is None else rows):
        np.random.set_state(np.random.RandomState(seeds[b]).get_state())
        outs[b] = eng.generate(enc[b:b + 1], emask[b:b + 1], m.sample_row, sampler=_sampler(m), max_new=max_new,
                               prefix=prefix[b:b + 1, :lens[b]] if prefix is not None and lens[b] else None,
                               stop=rules['stop'][b], order=rules['order'][b], allow=rules['allow'][b],
                               bar_allow=[rules['bar_allow'][b]] if rules['bar_allow'][b] is not None else None,
                               anchors=rules['anchors'][b]).cpu()[0]
        states[b] = np.random.get_state()
        infos[b] = dict(eng.last_decode)
    return outs, states, infos


def test_mixed_batch_equals_batch1_and_keeps_its_anchors():
    _need_gpu()
    from pianobart_amd import generation as G
    m, enc, emask, prefix, seeds, rules = _mixed()
    eng = m._get_engine()
    got, g_state, info = _batched(eng, m, enc, emask, seeds, rules, prefix, MIXED_LENS)
    free, f_state, f_info = _batched(eng, m, enc, emask, seeds, dict(rules, anchors=None), prefix, MIXED_LENS)
    want, w_state, w_info = _per_prompt(eng, m, enc, emask, seeds, rules, prefix, MIXED_LENS)
    A = rules['anchors']
    print('anchored batch: placed', info['anchors_placed'], 'rewinds', info['rewinds'], 'without anchors', f_info['rewinds'], 'ended', info['ended'],
          'lengths', [_length(got[b]) for b in range(16)])
    assert info['batched'] and info['batch'] == 16 and info['launches_per_token'] == f_info['launches_per_token'] == 6 * 2 + 3
    assert 'anchors_placed' not in f_info
    for b in range(16):
        k = MIXED_LENS[b]
        assert torch.equal(got[b], want[b]) and _same_state(g_state[b], w_state[b]), b
        assert w_info[b]['device_sampler'] and w_info[b]['rewinds'] <= 2, (b, w_info[b]['rewinds'])
        if A[b] is None:
            assert torch.equal(got[b], free[b]) and _same_state(g_state[b], f_state[b]) and info['anchors_placed'][b] == 0, b
            continue
        assert G.follows_anchors(got[b], A[b], start=k) == (True, len(A[b])) and G.is_time_ordered(got[b], start=k), b
        assert info['anchors_placed'][b] == len(A[b]) == w_info[b]['anchors_placed'][0], b
        assert not G.follows_anchors(free[b], A[b], start=k)[0], b   # the same row sampled without anchors does not hold them
        assert torch.equal(got[b][:k], prefix[b, :k]), b
    assert all(r <= 2 for r in info['rewinds']), info['rewinds']
    n9 = _length(got[9])
    assert (got[9][:n9, 0] < 12).all() and info['ended'][9] in ('bar', 'special', 'limit')
    for b in (6, 7):                                                   # the mask holds for what the model wrote; the anchors are written as given
        mine = {tuple(a) for a in A[b].tolist()}
        assert all(60 <= int(r[3]) < 128 or tuple(r.tolist()) in mine for r in got[b][MIXED_LENS[b]:_length(got[b])]), b


def test_anchors_under_refill_and_with_samples():
    """12 prompts in 4 slots equal the chunked call and the batch-1 rows; then 3 prompts with 3 + 1 + 2 samples."""
    _need_gpu()
    from pianobart_amd import generation as G
    m, enc, emask, prefix, seeds, rules = _mixed()
    eng = m._get_engine()
    cut = lambda r, n: {key: v[:n] for key, v in r.items()}
    r12 = cut(rules, 12)
    want, w_state, _ = _per_prompt(eng, m, enc[:12], emask[:12], seeds[:12], r12, max_new=24)
    plain, p_state, p_info = _batched(eng, m, enc[:12], emask[:12], seeds[:12], r12, refill=False, max_new=24)
    got, g_state, info = _batched(eng, m, enc[:12], emask[:12], seeds[:12], r12, refill=4, max_new=24)
    print('anchors under refill: placed', info['anchors_placed'], 'slots', info['row_slot'], 'rewinds', info['rewinds'])
    assert info['refill'] == 4 and info['admissions'] == 8 and info['anchors_placed'] == p_info['anchors_placed']
    for b in range(12):
        assert torch.equal(got[b], want[b]) and torch.equal(plain[b], want[b]), b
        assert _same_state(g_state[b], w_state[b]) and _same_state(p_state[b], w_state[b]), b
        if r12['anchors'][b] is not None:                              # 24 positions may end a row in front of its last anchor: the count is the row's own
            assert info['anchors_placed'][b] == G.follows_anchors(got[b], r12['anchors'][b])[1] >= 1 and G.is_time_ordered(got[b]), b
        else:
            assert info['anchors_placed'][b] == 0, b
    assert sum(info['anchors_placed'][b] == len(a) for b, a in enumerate(r12['anchors']) if a is not None) >= 5
    counts, owner = [3, 1, 2], [0, 0, 0, 1, 2, 2]
    per_prompt = dict(anchors=[rules['anchors'][4], None, rules['anchors'][9]], order=[-1, 0, -1], allow=[None] * 3, bar_allow=[None] * 3, stop=[PAD0, PAD0, 12])
    s_seeds = [3000 + 5 * r for r in range(6)]
    idx = torch.as_tensor(owner).cuda()
    want, w_state, _ = _per_prompt(eng, m, enc[idx], emask[idx], s_seeds, {key: [v[p] for p in owner] for key, v in per_prompt.items()})
    got, g_state, info = _batched(eng, m, enc[:3], emask[:3], s_seeds, per_prompt, samples=counts)
    assert info['batched'] and info['groups'] == owner and info['encoder_passes'] == 3
    for r, p in enumerate(owner):
        assert torch.equal(got[r], want[r]) and _same_state(g_state[r], w_state[r]), r
        n = 0 if per_prompt['anchors'][p] is None else len(per_prompt['anchors'][p])
        assert info['anchors_placed'][r] == n and (n == 0 or G.follows_anchors(got[r], per_prompt['anchors'][p]) == (True, n)), r
    with pytest.raises(Exception, match='entries'):                    # `anchors` describes the prompts, not the rows
        _batched(eng, m, enc[:3], emask[:3], s_seeds, dict(per_prompt, anchors=[per_prompt['anchors'][p] for p in owner]), samples=counts)


def test_the_wide_sampler_keeps_anchors():
    """The 2 470-id dictionary of tests/test_vocab_layout_gpu.py: the wide form of the sampler, batched and batch-1."""
    _need_gpu()
    from pianobart_amd import generation as G
    from tests.test_vocab_layout_gpu import _gen_model
    from tests.vocab_layout_util import synth_batch
    m, _, _, sizes = _gen_model('wide')
    lay = m.pianobart.layout
    eng = m._get_engine()
    enc = synth_batch(sizes, 4, S, seed=18, min_len=S - 9)[5].cuda()
    emask = (enc[:, :, 0] != lay.pad8[0]).float()
    pad = np.asarray(lay.pad8)
    rs = np.random.RandomState(2)
    anchors = [None]
    for b in range(1, 4):                                              # the first anchor at (0, 0): written at once, whatever the model samples
        a = np.stack([rs.randint(0, pad[h], size=3 + b) for h in range(8)], 1).astype(np.int64)
        a[:, 0] = np.sort(rs.randint(0, int(pad[0]), size=3 + b))
        a[:, 1] = np.sort(a[:, 1])
        a[0, :2] = 0
        anchors.append(a)
    assert lay.vocab == 2470 and max(int(a[:, 0].max()) for a in anchors[1:]) > 272       # bars beyond the narrow sampler's rows
    rngs = [np.random.RandomState(s) for s in range(40, 44)]
    got = eng.generate_batch(enc, emask, m.sample_row, rngs, sampler=_sampler(m), anchors=anchors).cpu()
    info = dict(eng.last_decode)
    print('wide anchors: placed', info['anchors_placed'], 'of', [0] + [len(a) for a in anchors[1:]], 'rewinds', info['rewinds'], info.get('sampler_form'))
    assert info.get('sampler_form') == 'wide' and eng.last_sampler_form == 'wide' and all(r <= 2 for r in info['rewinds'])
    assert info['anchors_placed'][0] == 0
    for b in range(1, 4):                                              # a row that fills the window may leave anchors unplaced: the count is the row's own
        ok, placed = G.follows_anchors(got[b], anchors[b], layout=lay)
        assert info['anchors_placed'][b] == placed >= 1 and (ok or placed < len(anchors[b])), b
    assert sum(info['anchors_placed']) >= 6
    np.random.set_state(np.random.RandomState(42).get_state())
    one = eng.generate(enc[2:3], emask[2:3], m.sample_row, sampler=_sampler(m), anchors=anchors[2]).cpu()[0]
    assert torch.equal(one, got[2]) and _same_state(np.random.get_state(), rngs[2].get_state())
    assert eng.last_decode['anchors_placed'] == [info['anchors_placed'][2]] and eng.last_sampler_form == 'wide'


# ---------------------------------------------------------------------------------------------------------------- 3. rewind
def test_rewind_restores_the_counter():
    """The device's bar id of one anchored row is corrupted (+ 1) at every third position (the sampler's fault_period: a test-only change of
    its choice of a token; no GPU fault is involved). The device then runs ahead on a wrong token, placing anchors the host has not; the
    host's token wins, the row is rewound with ITS counter (pb_batch_decoder_seek_anchor), and the result is the clean run's, token for token."""
    _need_gpu()
    from pianobart_amd import generation as G
    m, enc, emask, prefix, seeds, rules = _mixed()
    rows = [0, 4, 2, 9]
    idx = torch.as_tensor(rows).cuda()
    enc, emask, seeds = enc[idx], emask[idx], [seeds[b] for b in rows]
    r4 = {key: [v[b] for b in rows] for key, v in rules.items()}
    eng = m._get_engine()
    fr = 1                                                             # the row with 8 anchors
    clean, c_state, c_info = _batched(eng, m, enc, emask, seeds, r4)
    eng.decode_fault_row = (fr, 3)
    try:
        got, g_state, g_info = _batched(eng, m, enc, emask, seeds, r4)
    finally:
        eng.decode_fault_row = None
    print('rewind of an anchored row: rewinds', g_info['rewinds'], 'clean', c_info['rewinds'], 'placed', g_info['anchors_placed'])
    for b in range(4):
        assert torch.equal(got[b], clean[b]) and _same_state(g_state[b], c_state[b]), b
        if b != fr:
            assert g_info['rewinds'][b] == c_info['rewinds'][b], b
    assert g_info['rewinds'][fr] > c_info['rewinds'][fr] and g_info['rewinds'][fr] >= 3
    assert g_info['anchors_placed'] == c_info['anchors_placed'] == [0, 8, 4, 3]
    assert G.follows_anchors(got[fr], r4['anchors'][fr]) == (True, 8)
    # B = 1: the single-row sampler under the same hook
    np.random.set_state(np.random.RandomState(seeds[fr]).get_state())
    eng.decode_fault_period = 3
    try:
        one = eng.generate(enc[fr:fr + 1], emask[fr:fr + 1], m.sample_row, sampler=_sampler(m), anchors=r4['anchors'][fr]).cpu()[0]
    finally:
        eng.decode_fault_period = 0
    assert torch.equal(one, clean[fr]) and eng.last_decode['anchors_placed'] == [8] and eng.last_decode['rewinds'] >= 3


# ---------------------------------------------------------------------------------------------------------------- 4. no anchors
def test_no_anchors_is_todays_call():
    """anchors=None and an empty list for every row: the tokens, generator states, launches and record of the call without the argument."""
    _need_gpu()
    m = _model(32, 'bf16', specials='eos')
    enc, emask = _prompts(5, S, seed=41)
    eng = m._get_engine()
    seeds = [11, 12, 13, 14, 15]
    rngs = [np.random.RandomState(s) for s in seeds]
    want = eng.generate_batch(enc, emask, m.sample_row, rngs, sampler=_sampler(m)).cpu()
    w_info = dict(eng.last_decode)
    for anchors in (None, [None] * 5, [[]] * 5, [np.zeros((0, 8), dtype=np.int64)] * 2 + [None] * 3):
        rs = [np.random.RandomState(s) for s in seeds]
        got = eng.generate_batch(enc, emask, m.sample_row, rs, sampler=_sampler(m), anchors=anchors).cpu()
        info = dict(eng.last_decode)
        assert torch.equal(got, want)
        assert all(_same_state(a.get_state(), r.get_state()) for a, r in zip(rs, rngs))
        for key in ('launches_per_token', 'graph', 'tokens', 'steps', 'batch', 'batched', 'tokens_per_graph_replay'):
            assert info[key] == w_info[key], key
        assert set(info) == set(w_info)
    np.random.seed(9)
    a = eng.generate(enc[:1], emask[:1], m.sample_row, sampler=_sampler(m)).cpu()
    a_info, sa = dict(eng.last_decode), np.random.get_state()
    for anchors in (None, [], [None], np.zeros((0, 8), dtype=np.int64)):
        np.random.seed(9)
        b = eng.generate(enc[:1], emask[:1], m.sample_row, sampler=_sampler(m), anchors=anchors).cpu()
        assert torch.equal(a, b) and _same_state(sa, np.random.get_state())
        assert all(eng.last_decode[key] == a_info[key] for key in ('launches_per_token', 'graph', 'tokens'))
        assert set(eng.last_decode) == set(a_info)
    np.random.seed(9)
    c = m(enc[:1], encoder_attention_mask=emask[:1], generate=True, decoder_anchors=None)
    assert torch.equal(a, c.cpu())


# ---------------------------------------------------------------------------------------------------------------- 5. the command line
def test_eval_generation_accompany(tmp_path):
    """--prime half --accompany skyline on a tiny dataset in time order: every written piece holds the skyline of its own rows behind the
    prime, in time order, and stops at the bar after its last anchor."""
    _need_gpu()
    from pianobart_amd import eval_generation as EG
    from pianobart_amd import generation as G
    from tests.golden_util import synth_octuple_batch
    N = 5
    x = synth_octuple_batch(N, S, seed=5, min_len=S // 2)[5].numpy()
    for i in range(N):
        e = int(np.flatnonzero(x[i, :, 0] >= PAD0)[0])
        x[i, :e, 0], x[i, :e, 1] = np.arange(e) // 4, (np.arange(e) % 4) * 20
    np.save(str(tmp_path / 'prompts.npy'), x)
    out = str(tmp_path / 'o.npy')
    torch.manual_seed(0)
    EG.eval_generation(EG.get_args(['--dataset_path', str(tmp_path), '--dataset_name', 'prompts.npy', '--max_seq_len', str(S), '--hs', '256', '--layers', '2',
                                    '--ffn_dims', '256', '--heads', '4', '--nopretrain', '--seed', '0', '--batch_size', '16', '--prime', 'half',
                                    '--accompany', 'skyline', '--output', out]))
    y = np.load(out)
    assert y.shape == (N, S, 8) and y.dtype == np.float32
    ks = EG.prime_lengths(x, 'half', PAD0, PADV)
    total = 0
    for i in range(N):
        sky = G.anchor_rows(x[i][ks[i]:], 'skyline')
        total += len(sky)
        assert np.array_equal(y[i, :ks[i]], x[i, :ks[i]].astype(np.float32)), i
        assert G.follows_anchors(y[i], sky, start=ks[i]) == (True, len(sky)) and G.is_time_ordered(y[i], start=ks[i]), i
        n = _length(y[i])
        assert len(sky) == 0 or (y[i, ks[i]:n, 0] <= sky[-1, 0]).all(), i       # the stop: the bar after the last anchor
    assert total >= 10
