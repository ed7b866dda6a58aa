"""GPU: refilled batched generation -- Engine.generate_batch(refill=...), pb_batch_decoder_dynamic / pb_batch_decoder_admit, eval_generation
--refill.

Contract ("Refill: slots, slices and admission"): one fused decoder of n slots serves the whole call; a slot whose
row has stopped goes to the next waiting prompt while the other slots decode on. Every row is still the batch-1 `generate` of its prompt
under its own generator; the result and the final generator states are those of refill=False. On the device a dynamic decoder reads each
row's cross-attention geometry from device memory; its logits are bit for bit those of a decoder without the call, and an admission
touches no other row."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

from tests.golden_util import synth_octuple_batch
from tests.test_generate_batch_gpu import PAD, _lm, _need_gpu, _prompts, _reference, _same_state

pytestmark = pytest.mark.gpu
SOS = [258, 130, 131, 258, 130, 34, 256, 51]
EOS = [p + 3 for p in PAD]
MAIN = (256, 4, 200, 1.0)
HD128 = (1024, 8, 40, 8.0)
SHARP = (512, 8, 72, 40.0)


def _sampler(m):
    return dict(T=m.SAMPLE_T, P=m.SAMPLE_P)


def _no_stop(m):
    """No special id can be sampled: rows run to their limit. For a model whose engine is not built yet."""
    with torch.no_grad():
        m.mask_lm.proj[7].bias[PAD[7] + 3] = -30.0
    return m


def _piece(n, seed):
    """n ordinary Octuple rows."""
    return synth_octuple_batch(1, n + 2, seed=seed, min_len=n + 2)[5][0][:n].clone()


def _visible(n, S, lens, seed):
    """n prompts whose first lens[b] rows are ordinary events and the rest PAD (lens[b] = S: every key visible)."""
    enc = synth_octuple_batch(n, S + 1, seed=seed, min_len=S + 1)[5][:, :S].clone()
    for b, L in enumerate(lens):
        enc[b, L:] = torch.tensor(PAD)
    enc = enc.cuda()
    mask = (enc[:, :, 0] != 256).float()
    assert [int(v) for v in mask.sum(1).tolist()] == list(lens)
    return enc, mask


def _batched(eng, m, enc, emask, seeds, **kw):
    rngs = [np.random.RandomState(s) for s in seeds]
    out = eng.generate_batch(enc, emask, m.sample_row, rngs, sampler=_sampler(m), **kw).cpu()
    return out, [r.get_state() for r in rngs], dict(eng.last_decode)


# ---------------------------------------------------------------------------------------------------------------- the C ABI, driven directly
@contextlib.contextmanager
def _decoder(eng, enc, emask, n, slices=None):
    """A fused decoder of n rows over the first n prompts, set up as _decoder_run sets one up; slices: made dynamic with that many cross
    slices, every prompt of enc (<= slices) encoded and projected into the slice of its index. Yields (dec, bufs, em, enc16, s_enc)."""
    from pianobart_amd import ops
    from pianobart_amd._lib import LIB
    S, dev = int(enc.shape[1]), enc.device
    em, enc16 = eng._prompt_inputs(enc, emask)
    s_enc = [eng._key_extent(em[r:r + 1], S) for r in range(int(enc.shape[0]))]
    em_rows = em[:n].clone()
    bp, bufs = eng._decode_plan(n, S, s_enc[:n], em_rows, dev, G=slices)
    dec = eng._decoder_create(bp)
    assert dec is not None
    try:
        if slices is not None:
            LIB.call('pb_batch_decoder_dynamic', dec, slices)
        for g in range(int(enc.shape[0]) if slices is not None else n):
            _, enc_out = eng.forward_hidden(enc16[g:g + 1], None, em[g:g + 1], None, False, 0)
            for l in range(eng.ND):
                eng._linear(enc_out, 'dec.%d.wkv_c' % l, 'dec.%d.bkv_c' % l, bufs['kvc'][l][g], S, 2 * eng.d, eng.d)
        LIB.call('pb_batch_decoder_reset', dec, ops._stream(), 1)
        torch.cuda.current_stream().synchronize()
        yield dec, bufs, em, enc16, s_enc, em_rows
    finally:
        LIB.call('pb_batch_decoder_destroy', dec)


def _sampler_init(m, dec, U, n, S, forced=None):
    """sampler_init (+ force) + the logs; returns (log_logits (n, S, vocab), log_tok (n, S, 8)) as views of the pinned logs."""
    from pianobart_amd import ops
    from pianobart_amd._lib import LIB
    n8 = np.asarray(ops.SEG_SIZES, dtype=np.int32)
    off8 = np.asarray(ops.SEG_OFF[:8], dtype=np.int32)
    pad8 = np.asarray(PAD, dtype=np.int32)
    t8, p8 = np.asarray(m.SAMPLE_T, dtype=np.float32), np.asarray(m.SAMPLE_P, dtype=np.float32)
    LIB.call('pb_batch_decoder_sampler_init', dec, t8.ctypes.data, p8.ctypes.data, n8.ctypes.data, off8.ctypes.data, pad8.ctypes.data,
             U.ctypes.data, n * S * 8, S, -1, 0)
    if forced is not None:
        LIB.call('pb_batch_decoder_force', dec, forced.ctypes.data)
    lp, tp = ctypes.c_void_p(), ctypes.c_void_p()
    LIB.call('pb_batch_decoder_logs', dec, ctypes.byref(lp), ctypes.byref(tp))
    logits = np.ctypeslib.as_array((ctypes.c_float * (n * S * ops.VOCAB)).from_address(lp.value)).reshape(n, S, ops.VOCAB)
    tok = np.ctypeslib.as_array((ctypes.c_int16 * (n * S * 8)).from_address(tp.value)).reshape(n, S, 8)
    return logits, tok


def _start(dec, n, S):
    from pianobart_amd._lib import LIB
    first = np.ascontiguousarray(np.tile(np.asarray(SOS, dtype=np.int16), (n, 1)))
    last_pos, lim = np.full(n, -1, dtype=np.int32), np.full(n, S, dtype=np.int32)
    LIB.call('pb_batch_decoder_start', dec, last_pos.ctypes.data, first.ctypes.data, lim.ctypes.data)


def _steps(dec, count):
    """`count` steps, a run of <= 8 at a time, each waited for."""
    from pianobart_amd._lib import LIB
    left = count
    while left > 0:
        tk = int(LIB.query('pb_batch_decoder_launch', dec, min(8, left), None))
        assert tk >= 0, LIB.load().pb_last_error().decode()
        LIB.call('pb_batch_decoder_wait', dec, tk)
        left -= min(8, left)


# ---------------------------------------------------------------------------------------------------------------- 1. the dynamic kernel
@pytest.mark.parametrize('d,heads,S,sharp', [MAIN, HD128])
def test_dynamic_decoder_logits_are_bit_identical(d, heads, S, sharp, monkeypatch):
    """The same 4 prompts through a plain decoder and a dynamic one: one visible key row, every key visible, an s_enc with more than 64
    keys per split (S = 200, two cross splits), and a short one. Same draws, so the same tokens are fed as long as the logits agree."""
    _need_gpu()
    monkeypatch.setenv('PB_DECODE_SPLITS_CROSS', '2')
    m = _no_stop(_lm(S, d, 2, 512, heads, 35, 'bf16', sharp))
    eng = m._get_engine()
    lens = [1, S, 150, 70] if S == 200 else [1, S, 30, 17]
    enc, emask = _visible(4, S, lens, seed=110 + d)
    U = np.random.RandomState(6).random_sample((4, S * 8))
    got = {}
    for kind in ('plain', 'dynamic'):
        with torch.no_grad(), _decoder(eng, enc, emask, 4, slices=4 if kind == 'dynamic' else None) as (dec, _, _, _, s_enc, _):
            assert s_enc == lens
            logits, tok = _sampler_init(m, dec, U, 4, S)
            _start(dec, 4, S)
            _steps(dec, S)
            got[kind] = (logits.copy(), tok.copy())
    if S == 200:
        assert (150 + 1) // 2 > 64                                     # the third prompt's splits hold more than 64 keys
    for b in range(4):
        assert np.array_equal(got['plain'][1][b], got['dynamic'][1][b]), b
        for i in range(S):
            assert np.array_equal(got['plain'][0][b, i].view(np.int32), got['dynamic'][0][b, i].view(np.int32)), (b, i)
    assert ((got['plain'][1] >= 0) & (got['plain'][1] < np.asarray(PAD))).all()


# ---------------------------------------------------------------------------------------------------------------- 2. admission
def test_admission_leaves_the_neighbours_alone():
    """A 4-slot dynamic decoder: after 16 steps row 2 is ended and another prompt admitted into its slot, with another s_enc, a prefix of
    5 rows and a forced row. The other rows' logits and ids equal those of a run where row 2 was only ended; the admitted row's logits
    equal the batch-1 decoder's for that prompt."""
    _need_gpu()
    from pianobart_amd import ops
    from pianobart_amd._lib import LIB
    d, heads, S, sharp = MAIN
    m = _no_stop(_lm(S, d, 2, 512, heads, 36, 'bf16', sharp))
    eng = m._get_engine()
    lens = [90, S, 140, 33, 57]
    enc, emask = _visible(5, S, lens, seed=120)
    k, n_before, n_after = 5, 16, 16
    pre = _piece(k, 121)
    piece = _piece(S, 122).numpy()
    frow = np.full((S, 8), -1, dtype=np.int16)
    frow[k:, 3] = piece[k:, 3]                                         # pitch given behind the prefix
    frow[k + 3] = piece[k + 3]                                         # one fully given position
    U = np.random.RandomState(7).random_sample((4, S * 8))
    u_new = np.random.RandomState(8).random_sample(S * 8)
    free = np.full((4, S, 8), -1, dtype=np.int16)
    got = {}
    for kind in ('ended', 'admitted'):
        with torch.no_grad(), _decoder(eng, enc, emask, 4, slices=5) as (dec, bufs, em, enc16, s_enc, em_rows):
            logits, tok = _sampler_init(m, dec, U, 4, S, forced=free)
            _start(dec, 4, S)
            _steps(dec, n_before)
            LIB.call('pb_batch_decoder_seek', dec, 2, n_before - 1, None)
            if kind == 'admitted':
                LIB.call('pb_batch_decoder_fence', dec, ops._stream())
                eng._prefill(enc16[4:5], em[4:5], pre, k, [t[2] for t in bufs['kvs']])      # prompt 4's encoder pass was the last one run
                nxt = np.ascontiguousarray(pre[k - 1].numpy().astype(np.int16))
                mask_row = np.ascontiguousarray(em[4].cpu().numpy(), dtype=np.float32)
                LIB.call('pb_batch_decoder_admit', dec, 2, 4, s_enc[4], k - 1, nxt.ctypes.data, S, u_new.ctypes.data, frow.ctypes.data,
                         mask_row.ctypes.data, ops._stream())
            _steps(dec, n_after)
            got[kind] = (logits.copy(), tok.copy())
            if kind == 'admitted':
                assert torch.equal(em_rows[2], em[4]) and torch.equal(em_rows[1], em[1])
    for b in (0, 1, 3):
        n = n_before + n_after
        assert np.array_equal(got['ended'][1][b, :n], got['admitted'][1][b, :n]), b
        assert np.array_equal(got['ended'][0][b, :n].view(np.int32), got['admitted'][0][b, :n].view(np.int32)), b
    dyn_logits, dyn_tok = got['admitted'][0][2], got['admitted'][1][2]
    new = range(k, k + n_after)
    assert all(np.array_equal(dyn_tok[i][frow[i] >= 0], frow[i][frow[i] >= 0]) for i in new)
    # the batch-1 decoder of prompt 4, fed the tokens the slot decoded
    seen = []
    sampled = [i for i in new if (frow[i] < 0).any()]                  # a fully given position logs no logits row and samples nothing

    def cb(row):
        seen.append(row.clone())
        return torch.from_numpy(dyn_tok[sampled[len(seen) - 1]].astype(np.int64))
    np.random.seed(1)
    out = eng.generate(enc[4:5], emask[4:5], cb, max_new=n_after, sampler=_sampler(m), prefix=pre[None], forced=frow[None].astype(np.int64)).cpu()
    assert len(seen) == len(sampled) == n_after - 1
    for row, i in zip(seen, sampled):
        assert np.array_equal(row.numpy().view(np.int32), dyn_logits[i].view(np.int32)), i
    assert np.array_equal(out[0, k:k + n_after].numpy(), dyn_tok[k:k + n_after].astype(np.int64))


# ---------------------------------------------------------------------------------------------------------------- 3. the contract
def test_refill_equals_chunks_equals_batch1():
    _need_gpu()
    d, heads, S, sharp = MAIN
    m = _lm(S, d, 2, 512, heads, 31, 'bf16', sharp)
    eng = m._get_engine()
    enc, emask = _prompts(19, S, seed=140)
    seeds = [1000 + 7 * b for b in range(19)]
    want, w_state, w_info = _reference(eng, m, enc, emask, seeds)
    print('refill: batch-1 positions per prompt', [int(i['tokens']) for i in w_info])

    def check(idx, refill, tag):
        before = np.random.get_state()
        got, states, info = _batched(eng, m, enc[idx], emask[idx], [seeds[i] for i in idx], refill=refill)
        assert _same_state(before, np.random.get_state()), tag         # the global stream is not touched
        for j, i in enumerate(idx):
            assert torch.equal(got[j], want[i]), (tag, j, i)
            assert _same_state(states[j], w_state[i]), (tag, j, i)
        plain, p_states, _ = _batched(eng, m, enc[idx], emask[idx], [seeds[i] for i in idx], refill=False)
        assert torch.equal(got, plain) and all(_same_state(a, b) for a, b in zip(states, p_states)), tag
        return info

    info = check(list(range(11)), 4, 'refill=4')
    assert info['refill'] == 4 and info['batched'] and info['graph'] and info['launches_per_token'] == 6 * 2 + 3
    assert info['admissions'] == 7 and info['encoder_passes'] == 11 and len(info['tokens']) == len(info['rewinds']) == 11
    assert info['tokens'] == [int(i['tokens']) for i in w_info[:11]]
    assert 0 < info['row_steps'] <= info['steps'] * 4 and info['setup_ms'] > 0
    check([int(v) for v in np.random.RandomState(3).permutation(11)], 4, 'refill=4 shuffled')
    info = check(list(range(19)), True, 'refill=True, 19 prompts')
    assert info['refill'] == 16 and info['admissions'] == 3
    _, _, info = _batched(eng, m, enc[:4], emask[:4], seeds[:4], refill=4)     # no more rows than slots: a single chunk
    assert 'refill' not in info and info['batch'] == 4


# ---------------------------------------------------------------------------------------------------------------- 4. mixed batches
def test_refill_of_primed_and_forced_rows():
    _need_gpu()
    from pianobart_amd.generation import keep_mask
    d, heads, S, sharp = MAIN
    m = _lm(S, d, 2, 512, heads, 37, 'bf16', sharp)
    eng = m._get_engine()
    n = 10
    enc, emask = _prompts(n, S, seed=150)
    prefix = torch.stack([_piece(S, 600 + b) for b in range(n)])
    pieces = torch.stack([_piece(S, 700 + b) for b in range(n)])
    lens = [(0, 1, S // 2)[b % 3] for b in range(n)]
    ends = [20 + 9 * b for b in range(n)]
    forced = np.full((n, S, 8), -1, dtype=np.int64)
    for b in range(n):
        if b % 2 == 0:                                                 # kept attributes behind the prefix, up to a given EOS row
            p = pieces[b:b + 1].clone()
            p[0, lens[b] + ends[b]] = torch.tensor(EOS)
            forced[b] = keep_mask(p, 'bar,tempo', [lens[b]])[0]
            forced[b, lens[b] + ends[b]] = EOS
    seeds = [500 + 3 * b for b in range(n)]
    kw = dict(prefix=prefix, prefix_len=lens, forced=forced)
    plain, p_states, _ = _batched(eng, m, enc, emask, seeds, refill=False, **kw)
    got, g_states, info = _batched(eng, m, enc, emask, seeds, refill=3, **kw)
    assert info['refill'] == 3 and info['admissions'] == n - 3 and info['prefill_passes'] == sum(1 for k in lens if k)
    assert torch.equal(got, plain)
    assert all(_same_state(a, b) for a, b in zip(g_states, p_states))
    for b in range(0, n, 2):                                           # a given EOS row ends the row there at the latest
        assert info['tokens'][b] <= ends[b] + 1, b
    got5, s5, _ = _batched(eng, m, enc, emask, seeds, refill=3, max_new=5, **kw)
    plain5, p5, _ = _batched(eng, m, enc, emask, seeds, refill=False, max_new=5, **kw)
    assert torch.equal(got5, plain5) and all(_same_state(a, b) for a, b in zip(s5, p5))


# ---------------------------------------------------------------------------------------------------------------- 5. rewinds
def test_rewind_of_an_admitted_row():
    """The device's choice in ONE SLOT is corrupted at every third position, and the slot changes its occupant during the run: each
    row that sat in it is rewound alone, and no other row's rewinds move."""
    _need_gpu()
    d, heads, S, sharp = SHARP
    m = _lm(S, d, 2, 512, heads, 33, 'bf16', sharp)
    eng = m._get_engine()
    enc, emask = _prompts(11, S, seed=160)
    seeds = [11 + b for b in range(11)]
    want, w_state, w_info = _reference(eng, m, enc, emask, seeds)
    tokens = [int(i['tokens']) for i in w_info]
    clean, c_state, c_info = _batched(eng, m, enc, emask, seeds, refill=4)
    fs = int(np.argmin(tokens[:4]))                                    # the slot whose first row stops first
    eng.decode_fault_row = (fs, 3)
    try:
        got, g_state, g_info = _batched(eng, m, enc, emask, seeds, refill=4)
    finally:
        eng.decode_fault_row = None
    print('rewind: tokens', tokens, 'slots', g_info['row_slot'], 'rewinds', g_info['rewinds'], 'clean', c_info['rewinds'])
    sat = [r for r in range(11) if g_info['row_slot'][r] == fs]
    assert len(sat) >= 2 and sat[0] == fs                              # the slot changed its occupant
    for r in range(11):
        assert torch.equal(got[r], want[r]) and torch.equal(clean[r], want[r]), r
        assert _same_state(g_state[r], w_state[r]) and _same_state(c_state[r], w_state[r]), r
        assert g_info['tokens'][r] == c_info['tokens'][r] == tokens[r], r
        if r not in sat:
            assert g_info['rewinds'][r] == c_info['rewinds'][r], (r, g_info['rewinds'], c_info['rewinds'])
        elif tokens[r] >= 4:                                           # position 2 is corrupted and is not the row's stop
            assert g_info['rewinds'][r] > c_info['rewinds'][r], (r, g_info['rewinds'], c_info['rewinds'])
    assert any(tokens[r] >= 4 for r in sat[1:]), (sat, tokens)         # an ADMITTED row was rewound, not only the slot's first


# ---------------------------------------------------------------------------------------------------------------- 6. refill fills
def test_refill_actually_fills():
    """12 fully given rows of lengths L, s, s, s, L, s, s, s, L, s, s, s (L = 160, s = 4) in 4 slots. In chunks of 4 every chunk lasts as
    long as its long row: about 3 x 168 steps. Refilled, a hand-over takes effect at most 3 replays (24 steps) behind a row's last
    position, so the third long row starts by about step 40 and the call ends by about step 210: at most 0.6 of the chunks' steps."""
    _need_gpu()
    d, heads, S, sharp = MAIN
    m = _lm(S, d, 2, 512, heads, 38, 'bf16', sharp)
    eng = m._get_engine()
    L, s = 160, 4
    lengths = [L, s, s, s] * 3
    enc, emask = _prompts(12, S, seed=170)
    forced = np.full((12, S, 8), -1, dtype=np.int64)
    for b, n in enumerate(lengths):
        forced[b, :n] = _piece(n, 800 + b).numpy()
        forced[b, n] = EOS
    seeds = list(range(12))
    got, g_state, info = _batched(eng, m, enc, emask, seeds, refill=4, forced=forced)
    chunk_steps, outs = 0, []
    for c in range(0, 12, 4):
        out, _, ci = _batched(eng, m, enc[c:c + 4], emask[c:c + 4], seeds[c:c + 4], refill=False, forced=forced[c:c + 4])
        outs.append(out)
        chunk_steps += ci['steps']
    occupancy = info['row_steps'] / (info['steps'] * 4)
    print('refill fills: steps %d refilled, %d in chunks of 4; occupancy %.3f' % (info['steps'], chunk_steps, occupancy))
    assert torch.equal(got, torch.cat(outs))
    for b, n in enumerate(lengths):
        assert np.array_equal(got[b, :n].numpy(), forced[b, :n]) and (got[b, n:] == torch.tensor(PAD)).all(), b
        assert _same_state(g_state[b], np.random.RandomState(seeds[b]).get_state()), b        # nothing sampled: no draw
    assert info['rewinds'] == [0] * 12 and info['tokens'] == [n + 1 for n in lengths]
    assert info['admissions'] == 8
    assert info['steps'] <= 0.6 * chunk_steps


# ---------------------------------------------------------------------------------------------------------------- 7. eval_generation
def test_eval_generation_refill_writes_the_same_bytes(tmp_path):
    _need_gpu()
    from pianobart_amd import eval_generation as EG
    S, N = 40, 9
    enc = synth_octuple_batch(N, S, seed=5, min_len=S // 2)[5].numpy()
    np.save(str(tmp_path / 'prompts.npy'), enc)
    base = ['--dataset_path', str(tmp_path), '--dataset_name', 'prompts.npy', '--max_seq_len', str(S), '--hs', '256', '--layers', '2',
            '--ffn_dims', '512', '--heads', '4', '--nopretrain', '--prime', 'half', '--keep', 'bar,position', '--seed', '3', '--score']

    def run(name, *extra):
        torch.manual_seed(0)
        out = str(tmp_path / name)
        EG.eval_generation(EG.get_args(base + ['--output', out] + list(extra)))
        return out

    a = run('plain.npy', '--batch_size', '16')
    b = run('refill.npy', '--batch_size', '4', '--refill', '4')
    assert open(a, 'rb').read() == open(b, 'rb').read()
    assert np.load(a).shape == (N, S, 8)
    sa, sb = np.load(a[:-4] + '_score.npy'), np.load(b[:-4] + '_score.npy')
    assert sa.shape == sb.shape == (N, 9) and np.array_equal(sa[:, 8], sb[:, 8]) and np.allclose(sa, sb, rtol=1e-5, atol=1e-5)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_decoder_working():
    """Every refusal is a host-side check in front of any launch or copy; the decoder goes on afterwards."""
    _need_gpu()
    from pianobart_amd import ops
    from pianobart_amd._lib import LIB
    d, heads, S, sharp = HD128
    m = _no_stop(_lm(S, d, 2, 512, heads, 39, 'bf16', sharp))
    eng = m._get_engine()
    enc, emask = _visible(3, S, [12, S, 25], seed=180)
    err = lambda: LIB.load().pb_last_error().decode()
    U = np.random.RandomState(9).random_sample((2, S * 8))
    u_row = np.random.RandomState(10).random_sample(S * 8)
    sos = np.asarray(SOS, dtype=np.int16)
    ordinary = lambda tok: ((tok >= 0) & (tok < np.asarray(PAD))).all()
    # a plain decoder: dynamic after share_cross, share_cross / dynamic after a step, admit on a decoder that is not dynamic
    with torch.no_grad(), _decoder(eng, enc[:2], emask[:2], 2) as (dec, _, em, _, s_enc, _):
        kv_row = np.asarray([0, 1], dtype=np.int32)
        LIB.call('pb_batch_decoder_share_cross', dec, 2, kv_row.ctypes.data)
        assert LIB.query('pb_batch_decoder_dynamic', dec, 2) < 0 and 'share_cross' in err()
        logits, tok = _sampler_init(m, dec, U, 2, S)
        _start(dec, 2, S)
        _steps(dec, 4)
        assert LIB.query('pb_batch_decoder_dynamic', dec, 2) < 0 and 'already issued' in err()
        mask_row = np.ascontiguousarray(em[0].cpu().numpy(), dtype=np.float32)
        assert LIB.query('pb_batch_decoder_admit', dec, 0, 0, s_enc[0], -1, sos.ctypes.data, S, u_row.ctypes.data, None, mask_row.ctypes.data,
                         ops._stream()) < 0 and 'not a dynamic decoder' in err()
        _steps(dec, 4)
        assert ordinary(tok[:, :8])
    # a dynamic decoder of 2 slots and 3 slices, no force table
    with torch.no_grad(), _decoder(eng, enc, emask, 2, slices=3) as (dec, _, em, _, s_enc, _):
        assert LIB.query('pb_batch_decoder_dynamic', dec, 3) < 0 and 'already dynamic' in err()
        kv_row = np.asarray([0, 1], dtype=np.int32)
        assert LIB.query('pb_batch_decoder_share_cross', dec, 2, kv_row.ctypes.data) < 0 and 'dynamic' in err()
        logits, tok = _sampler_init(m, dec, U, 2, S)
        _start(dec, 2, S)
        mask_row = np.ascontiguousarray(em[2].cpu().numpy(), dtype=np.float32)

        def admit(row=0, slice_=2, se=None, last=-1, nxt=sos, limit=S, forced_row=None, mask=mask_row):
            return LIB.query('pb_batch_decoder_admit', dec, row, slice_, s_enc[2] if se is None else se, last, nxt.ctypes.data, limit,
                             u_row.ctypes.data, forced_row.ctypes.data if forced_row is not None else None,
                             mask.ctypes.data if mask is not None else None, ops._stream())
        assert admit() < 0 and 'live' in err()                         # row 0 was started and not ended
        _steps(dec, 4)
        LIB.call('pb_batch_decoder_seek', dec, 0, 3, None)
        assert admit(row=2) < 0 and 'row 2' in err()
        assert admit(slice_=3) < 0 and 'slice 3' in err()
        assert admit(slice_=1) < 0 and 'live row 1' in err()           # the slice a live row reads
        assert admit(se=0) < 0 and 's_enc 0' in err()
        assert admit(se=S + 1) < 0 and 's_enc %d' % (S + 1) in err()
        assert admit(last=S, limit=S) < 0 and 'limit' in err()
        assert admit(limit=S + 1) < 0 and 'limit' in err()
        bad = sos.copy()
        bad[5] = 38
        assert admit(nxt=bad) < 0 and 'head 5' in err() and 'id 38' in err()
        assert admit(forced_row=np.full((S, 8), -1, dtype=np.int16)) < 0 and 'force table' in err()
        assert admit(mask=None) < 0 and 'mask' in err()
        _steps(dec, 4)                                                 # row 1 decodes on, row 0 stays ended
        assert ordinary(tok[1, :8]) and ordinary(tok[0, :4])
        assert admit() == 0, err()                                     # and a good admission still goes through
        _steps(dec, 4)
        assert ordinary(tok[0, :4]) and ordinary(tok[1, :12])
    # forced ids are checked against their tables where the decoder has one
    with torch.no_grad(), _decoder(eng, enc, emask, 2, slices=3) as (dec, _, em, _, s_enc, _):
        logits, tok = _sampler_init(m, dec, U, 2, S, forced=np.full((2, S, 8), -1, dtype=np.int16))
        _start(dec, 2, S)
        _steps(dec, 4)
        LIB.call('pb_batch_decoder_seek', dec, 0, 3, None)
        mask_row = np.ascontiguousarray(em[2].cpu().numpy(), dtype=np.float32)
        for h, v in ((5, 38), (0, 262), (7, -2)):
            frow = np.full((S, 8), -1, dtype=np.int16)
            frow[S - 1, h] = v
            assert LIB.query('pb_batch_decoder_admit', dec, 0, 2, s_enc[2], -1, sos.ctypes.data, S, u_row.ctypes.data, frow.ctypes.data,
                             mask_row.ctypes.data, ops._stream()) < 0
            assert 'head %d' % h in err() and 'position %d' % (S - 1) in err() and 'id %d' % v in err(), err()
        _steps(dec, 4)
        assert ordinary(tok[1, :8])
