"""GPU: forced tokens -- part of a piece is given per position and head, the model samples the rest (Engine.generate(forced=...),
Engine.generate_batch(forced=...), PianoBartLM.forward(generate=True, decoder_forced=...), pb_batch_decoder_force, eval_generation --keep).

Contract ("Forced tokens"): `forced` (B, S, 8), -1 = free, v >= 0 = "head h of position i of row b is v". The result is
the reference loop (model.py:42-65) with the given heads of `current_output` overwritten right after `self.sample(x, i)`: the stop rule sees
the token after forcing, a position with a free head draws its 8 uniforms, a position with all 8 heads given draws nothing. The fused
decoder applies the table in its device sampler (dec_sample_kernel<ROWS, true>) and the host's verification applies it to its own tokens."""
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


def _free(S):
    return np.full((S, 8), -1, dtype=np.int64)


def _length(row):
    """Emitted positions of one output row (S, 8): the rows in front of its first bar PAD."""
    bar = np.asarray(row.cpu() if isinstance(row, torch.Tensor) else row)[:, 0]
    pad = np.flatnonzero(bar == PAD[0])
    return int(pad[0]) if len(pad) else len(bar)


def _given_appear(out, frow, k=0):
    """The given heads of positions k .. the row's stop appear verbatim in the output row."""
    n = _length(out)
    f = torch.as_tensor(np.asarray(frow))[k:n]
    return bool(((f < 0) | (f == out[k:n].cpu())).all())


# ---------------------------------------------------------------------------------------------------------------- 1. against the oracle
def _oracle_forced(o, enc, emask, pre, forced):
    """The reference loop (model.py:28-66) with the prefix filled in, plus the one line of the contract: the given heads overwrite the
    sampled token (a position whose 8 heads are given samples nothing, so it draws nothing). On the CPU oracle."""
    S, k = enc.shape[1], pre.shape[0]
    pad = torch.from_numpy(o.pianobart.pad_word_np)
    dec, result = pad.repeat(1, S, 1), pad.repeat(1, S, 1)
    dmask = torch.zeros_like(emask)
    dec[:, 0] = torch.tensor(o.pianobart.sos_word_np)
    dmask[:, 0] = 1
    n = min(k, S - 1)
    dec[0, 1:n + 1] = pre[:n]
    dmask[:, :n + 1] = 1
    result[0, :k] = pre
    for i in range(k, S):
        f = torch.as_tensor(forced[i])
        if bool((f >= 0).all()):
            cur = f.clone()
        else:
            x = o.mask_lm(o.pianobart(enc, dec, emask, dmask))
            cur = o.sample(x, i)
            cur[f >= 0] = f[f >= 0]                                    # the line the contract adds
        if i != S - 1:
            dec[:, i + 1] = cur
            dmask[:, i + 1] += 1
        if (cur >= pad).any():
            break
        result[:, i] = cur
    return result


def _oracle_masks(S):
    piece = _piece(S, 900).numpy()
    head = _free(S)
    head[:, 3] = piece[:, 3]                                           # one head given everywhere
    stretch = _free(S)
    stretch[3:7] = piece[3:7]                                          # all heads given at positions 3 .. 6
    eos = _free(S)
    eos[11, 7] = EOS[7]                                                # a forced EOS id at position 11
    primed = _free(S)
    primed[5:, 0], primed[5:, 1] = piece[5:, 0], piece[5:, 1]          # a prefix of 5 plus forcing behind it
    primed[9:11] = piece[9:11]
    return dict(head=(0, head), stretch=(0, stretch), eos=(0, eos), primed=(5, primed))


@pytest.mark.parametrize('case', ['head', 'stretch', 'eos', 'primed'])
def test_forced_generate_against_the_oracle(case):
    _need_gpu()
    from oracle import pianobart_oracle as O
    S = 20
    k, forced = _oracle_masks(S)[case]
    m = _lm(S, 64, 2, 128, 2, 61, 'fp32', specials='off')              # no sampled special: a row ends only where a given id ends it
    o = O.PianoBartLM(O.PianoBart(O.BartConfig(max_position_embeddings=S, d_model=64, encoder_layers=2, decoder_layers=2, encoder_ffn_dim=128,
                                               decoder_ffn_dim=128, encoder_attention_heads=2, decoder_attention_heads=2), E2W, W2E)).eval()
    o.load_state_dict(m.state_dict(), strict=True)
    m = m.cuda()
    enc = synth_octuple_batch(1, S, seed=301, min_len=12)[5]
    emask = (enc[:, :, 0] != 256).float()
    pre = _piece(k, 401)
    with torch.no_grad():
        np.random.seed(778)
        want = _oracle_forced(o, enc, emask, pre, forced)
        st_o = np.random.get_state()
        np.random.seed(778)
        got = m(enc.cuda(), None, emask.cuda(), None, generate=True, device_num=0, decoder_prefix=pre[None] if k else None,
                decoder_forced=forced[None])
        st_m = np.random.get_state()
    assert got.shape == want.shape and torch.equal(got.cpu(), want)
    assert _same_state(st_o, st_m)
    assert _length(want[0]) == (11 if case == 'eos' else S) and _given_appear(want[0], forced, k)
    if case == 'stretch':                                              # 4 of 20 positions drew nothing
        np.random.seed(778)
        np.random.random_sample(8 * (S - 4))
        assert _same_state(np.random.get_state(), st_m)


# ---------------------------------------------------------------------------------------------------------------- 2. the paths agree
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_forced_paths_agree(precision):
    _need_gpu()
    S, k = 48, 6
    m = _lm(S, 256, 2, 256, 4, 78, precision, specials='eos').cuda()
    enc, emask = _prompts(1, S, seed=4)
    pre = _piece(k, 5)
    piece = _piece(S, 6).numpy()
    forced = _free(S)
    forced[k:, 3] = piece[k:, 3]                                       # pitch given behind the prefix
    forced[k:34, 7] = piece[k:34, 7]                                   # the one head that can stop the row: ordinary ids up to position 33
    forced[12:15] = piece[12:15]                                       # three fully given positions
    forced[20, 0] = PAD[0] - 1
    eng = m._get_engine()

    def run(fn):
        np.random.seed(5)
        out = fn().cpu()
        return out, np.random.get_state()

    kw = dict(prefix=pre[None], forced=forced[None])
    a, sa = run(lambda: eng.generate(enc, emask, m.sample_row, **kw))                       # fp32: pb_decode_step, bf16: fused host-sampled
    s, ss = run(lambda: eng.generate(enc, emask, m.sample_row, sampler=_sampler(m), **kw))  # bf16: fused device-sampled
    b, sb = run(lambda: eng.generate(enc, emask, m.sample_row, use_cache=False, **kw))
    c, sc = run(lambda: eng._generate_pyloop(enc, emask, m.sample_row, k, pre, forced.astype(np.int16)))
    assert torch.equal(b, c) and _same_state(sb, sc)                        # same kernels: bitwise
    assert torch.equal(a, s) and _same_state(sa, ss)                        # the host's token always wins
    if precision == 'fp32':
        assert torch.equal(a, b) and _same_state(sa, sb)
    for out in (a, s, b, c):
        assert torch.equal(out[0, :k], pre) and _length(out[0]) >= 34 and _given_appear(out[0], forced, k)


# ---------------------------------------------------------------------------------------------------------------- 3. batch contract
def _batch_setup(n=17, S=64, seed=32, specials='eos'):
    """n rows, each with another mask: unforced, a fully given stretch (leading, or in the middle), single heads, a forced stop, a primed row,
    a row given at every position."""
    m = _lm(S, 256, 2, 512, 4, seed, 'bf16', specials=specials).cuda()
    enc, emask = _prompts(n, S, seed=41)
    prefix = torch.stack([_piece(S, 600 + b) for b in range(n)])
    pieces = np.stack([_piece(S, 700 + b).numpy() for b in range(n)])
    lens, forced = [0] * n, np.full((n, S, 8), -1, dtype=np.int64)
    for b in range(n):
        kind, p, f = b % 8, pieces[b], forced[b]
        if kind == 1:
            f[4:13] = p[4:13]                                          # a fully given stretch
        elif kind == 2:
            f[:, 7] = p[:, 7]                                          # the stopping head given everywhere: the row runs to the window's end
        elif kind == 3:
            f[:20 + b, 7] = p[:20 + b, 7]                              # a forced stop: ordinary ids, then the EOS id
            f[20 + b, 7] = EOS[7]
        elif kind == 4:
            lens[b] = 10 + b                                           # a primed row with heads given behind its prefix
            f[lens[b]:, [0, 1, 4]] = p[lens[b]:][:, [0, 1, 4]]
        elif kind == 5:
            f[:6] = p[:6]                                              # leading given positions: stepped through, not prefilled
            f[6:, 3] = p[6:, 3]
        elif kind == 6:
            f[:] = p                                                   # every position given, ended by a given EOS row: no draw at all
            f[30 + b] = EOS
        elif kind == 7:
            f[::3, 5] = p[::3, 5]                                      # one head at every third position
            f[1::2, 0] = p[1::2, 0]
    return m, enc, emask, prefix, lens, forced


def _reference(eng, m, enc, emask, prefix, lens, forced, seeds, max_new=None):
    outs, states, infos = [], [], []
    for b, s in enumerate(seeds):
        np.random.set_state(np.random.RandomState(s).get_state())
        outs.append(eng.generate(enc[b:b + 1], emask[b:b + 1], m.sample_row, max_new=max_new, sampler=_sampler(m),
                                 prefix=prefix[b:b + 1, :lens[b]] if prefix is not None else None, forced=forced[b:b + 1]).cpu()[0])
        states.append(np.random.get_state())
        infos.append(dict(eng.last_decode))
    return outs, states, infos


def _batched(eng, m, enc, emask, prefix, lens, forced, seeds, max_new=None, **kw):
    rngs = [np.random.RandomState(s) for s in seeds]
    out = eng.generate_batch(enc, emask, m.sample_row, rngs, max_new=max_new, sampler=_sampler(m), prefix=prefix, prefix_len=lens, forced=forced,
                             **kw).cpu()
    return out, [r.get_state() for r in rngs], dict(eng.last_decode)


def test_forced_batch_equals_batch1_per_row():
    _need_gpu()
    m, enc, emask, prefix, lens, forced = _batch_setup()
    n, S = forced.shape[:2]
    eng = m._get_engine()
    seeds = [2000 + 7 * b for b in range(n)]
    want, w_state, w_info = _reference(eng, m, enc, emask, prefix, lens, forced, seeds)
    print('forced batch-1 positions per row', [int(i['tokens']) for i in w_info])
    for b in range(n):
        assert _given_appear(want[b], forced[b], lens[b]), b
        if b % 8 == 2:
            assert _length(want[b]) == S, b                            # a given ordinary id keeps the row going
        if b % 8 == 3:
            assert _length(want[b]) == 20 + b, b                       # a given special id ends it
        if b % 8 == 6:                                                 # nothing drawn: the generator has not moved
            assert _length(want[b]) == 30 + b and _same_state(w_state[b], np.random.RandomState(seeds[b]).get_state()), b

    def check(idx, tag, max_new=None, ref=(want, w_state)):
        got, states, info = _batched(eng, m, enc[idx], emask[idx], prefix[idx], [lens[i] for i in idx], forced[idx], [seeds[i] for i in idx], max_new)
        for j, i in enumerate(idx):
            assert torch.equal(got[j], ref[0][i]), (tag, j, i)
            assert _same_state(states[j], ref[1][i]), (tag, j, i)
        return info

    info = check(list(range(n)), 'B=17 (one full chunk plus one row)')
    assert info['batched'] and info['batch'] == 1
    info = check(list(range(16)), 'B=16')
    assert info['batched'] and info['batch'] == 16 and info['launches_per_token'] == 6 * 2 + 3
    check([int(v) for v in np.random.RandomState(3).permutation(n)[:9]], 'B=9 shuffled')
    ref = _reference(eng, m, enc, emask, prefix, lens, forced, seeds, max_new=9)
    info = check(list(range(16)), 'max_new=9', max_new=9, ref=ref[:2])
    assert all(t <= 9 for t in info['tokens'])                         # positions from k_b on, given or sampled


# ---------------------------------------------------------------------------------------------------------------- 4. no forcing
def test_unforced_rows_are_todays_rows():
    """forced = -1 everywhere: the launches, the graph and the bytes of a call without the argument."""
    _need_gpu()
    m, enc, emask, _, _, _ = _batch_setup(n=5)
    S = int(enc.shape[1])
    eng = m._get_engine()
    seeds = [11, 12, 13, 14, 15]
    rngs = [np.random.RandomState(s) for s in seeds]
    want = eng.generate_batch(enc, emask, m.sample_row, rngs, sampler=_sampler(m)).cpu()
    w_info = dict(eng.last_decode)
    got, states, info = _batched(eng, m, enc, emask, None, None, np.full((5, S, 8), -1), seeds)
    assert torch.equal(got, want)
    assert all(_same_state(a, r.get_state()) for a, r in zip(states, rngs))
    for key in ('launches_per_token', 'graph', 'tokens', 'steps', 'batch', 'batched', 'tokens_per_graph_replay'):
        assert info[key] == w_info[key], key
    np.random.seed(9)
    a = eng.generate(enc[:1], emask[:1], m.sample_row, sampler=_sampler(m)).cpu()
    a_info, sa = dict(eng.last_decode), np.random.get_state()
    np.random.seed(9)
    b = eng.generate(enc[:1], emask[:1], m.sample_row, sampler=_sampler(m), forced=torch.full((1, S, 8), -1)).cpu()
    assert torch.equal(a, b) and _same_state(sa, np.random.get_state())
    assert all(eng.last_decode[key] == a_info[key] for key in ('launches_per_token', 'graph', 'tokens'))


# ---------------------------------------------------------------------------------------------------------------- 5. rewinds
@pytest.mark.parametrize('head0', ['free', 'given'])
def test_rewind_of_a_forced_row(head0):
    """The device's id of head 0 of one row is corrupted at every third position. head 0 free there: the row rewinds to the host's sampled
    token. head 0 given there: the host's given id wins over the corrupted one. Either way the row is its batch-1 row and its siblings
    are untouched."""
    _need_gpu()
    m, enc, emask, _, _, _ = _batch_setup(n=4, specials='off')
    S = int(enc.shape[1])
    pieces = np.stack([_piece(S, 800 + b).numpy() for b in range(4)])
    forced = np.full((4, S, 8), -1, dtype=np.int64)
    forced[:, :, 3] = pieces[:, :, 3]                                  # every row has given heads
    forced[1, 10:14] = pieces[1, 10:14]
    fr = 2
    if head0 == 'given':
        forced[fr, :, 0] = pieces[fr, :, 0]
    eng = m._get_engine()
    seeds = [21, 22, 23, 24]
    want, w_state, w_info = _reference(eng, m, enc, emask, None, None, forced, seeds)
    clean, _, c_info = _batched(eng, m, enc, emask, None, None, forced, seeds)
    assert w_info[fr]['tokens'] == S
    eng.decode_fault_row = (fr, 3)
    try:
        got, g_state, g_info = _batched(eng, m, enc, emask, None, None, forced, seeds)
    finally:
        eng.decode_fault_row = None
    for b in range(4):
        assert torch.equal(got[b], want[b]) and torch.equal(clean[b], want[b]), b
        assert _same_state(g_state[b], w_state[b]), b
        assert _given_appear(got[b], forced[b]), b
        if b != fr:
            assert g_info['rewinds'][b] == c_info['rewinds'][b], b
    assert g_info['rewinds'][fr] > c_info['rewinds'][fr]


# ---------------------------------------------------------------------------------------------------------------- 6. samples of one prompt
def test_forced_samples_of_one_prompt():
    _need_gpu()
    m, enc, emask, prefix, _, forced = _batch_setup(n=6)
    S = int(enc.shape[1])
    enc, emask, prefix = enc[:2], emask[:2], prefix[:2]
    masks = np.stack([forced[5], forced[4]])                           # prompt 0: leading given positions + pitch; prompt 1: primed, heads behind it
    lens = [0, 14]
    counts = [3, 3]
    owner = [0, 0, 0, 1, 1, 1]
    seeds = [3000 + 5 * r for r in range(6)]
    eng = m._get_engine()
    idx = torch.as_tensor(owner)
    want, w_state, _ = _reference(eng, m, enc[idx.cuda()], emask[idx.cuda()], prefix[idx], [lens[p] for p in owner], masks[owner], seeds)
    got, g_state, info = _batched(eng, m, enc, emask, prefix, lens, masks, seeds, samples=counts)
    assert info['batched'] and info['groups'] == owner and info['encoder_passes'] == 2
    for r, p in enumerate(owner):
        assert torch.equal(got[r], want[r]) and _same_state(g_state[r], w_state[r]), r
        assert _given_appear(got[r], masks[p], lens[p]), r
    assert not torch.equal(got[0], got[1]) and not torch.equal(got[3], got[4])      # the samples of a prompt differ where it is free


# ---------------------------------------------------------------------------------------------------------------- 7. refusals
def test_force_refusals_leave_the_decoder_working():
    """pb_batch_decoder_force is refused before sampler_init, for a value outside its table and after a launch (host-side checks: nothing
    is enqueued by a refused call), and the decoder goes on with the table it had."""
    _need_gpu()
    from pianobart_amd import ops
    from pianobart_amd._lib import LIB
    m, enc, emask, _, _, _ = _batch_setup(n=2, specials='off')
    S, B = int(enc.shape[1]), 2
    eng = m._get_engine()
    piece = np.stack([_piece(S, 850 + b).numpy() for b in range(B)])
    tab = np.full((B, S, 8), -1, dtype=np.int16)
    tab[:, :, 3] = piece[:, :, 3]
    tab[1, 2:4] = piece[1, 2:4]
    err = lambda: LIB.load().pb_last_error().decode()
    with torch.no_grad(), eng._decoder_run(enc, emask, [0, 0], None) as run:
        dec = run.dec
        assert dec is not None
        assert LIB.query('pb_batch_decoder_force', dec, tab.ctypes.data) < 0 and 'sampler_init' in err()
        n8 = np.asarray(ops.SEG_SIZES, dtype=np.int32)
        off8 = np.asarray(ops.SEG_OFF[:8], dtype=np.int32)
        pad8 = np.asarray(PAD, dtype=np.int32)
        t8, p8 = np.asarray(m.SAMPLE_T, dtype=np.float32), np.asarray(m.SAMPLE_P, dtype=np.float32)
        U = np.random.RandomState(0).random_sample((B, S * 8))
        LIB.call('pb_batch_decoder_sampler_init', dec, t8.ctypes.data, p8.ctypes.data, n8.ctypes.data, off8.ctypes.data, pad8.ctypes.data,
                 U.ctypes.data, B * S * 8, S, -1, 0)
        for h, v in ((5, 38), (0, 262), (7, -2), (2, 135)):
            bad = tab.copy()
            bad[1, S - 1, h] = v
            assert LIB.query('pb_batch_decoder_force', dec, bad.ctypes.data) < 0
            assert 'head %d' % h in err() and 'position %d' % (S - 1) in err() and 'id %d' % v in err(), err()
        assert LIB.query('pb_batch_decoder_force', dec, None) < 0
        LIB.call('pb_batch_decoder_force', dec, tab.ctypes.data)
        lp, tp = ctypes.c_void_p(), ctypes.c_void_p()
        LIB.call('pb_batch_decoder_logs', dec, ctypes.byref(lp), ctypes.byref(tp))
        log_tok = np.ctypeslib.as_array((ctypes.c_int16 * (B * S * 8)).from_address(tp.value)).reshape(B, S, 8)
        first = np.ascontiguousarray(np.tile(np.asarray(SOS, dtype=np.int16), (B, 1)))
        last_pos, lim = np.full(B, -1, dtype=np.int32), np.full(B, S, dtype=np.int32)
        LIB.call('pb_batch_decoder_start', dec, last_pos.ctypes.data, first.ctypes.data, lim.ctypes.data)
        tk = int(LIB.query('pb_batch_decoder_launch', dec, 4, None))
        assert tk >= 0
        LIB.call('pb_batch_decoder_wait', dec, tk)
        other = np.full((B, S, 8), -1, dtype=np.int16)
        assert LIB.query('pb_batch_decoder_force', dec, other.ctypes.data) < 0 and 'already issued' in err()
        tk = int(LIB.query('pb_batch_decoder_launch', dec, 4, None))          # still working, still with its table
        assert tk >= 0
        LIB.call('pb_batch_decoder_wait', dec, tk)
        got = log_tok[:, :8].copy()
    assert np.array_equal(got[:, :, 3], tab[:, :8, 3]) and np.array_equal(got[1, 2:4], tab[1, 2:4])
    assert ((got >= 0) & (got < np.asarray(PAD))).all()


# ---------------------------------------------------------------------------------------------------------------- 8. eval_generation --keep
def test_eval_generation_prime_half_keep(tmp_path):
    _need_gpu()
    from pianobart_amd import eval_generation as EG
    S, N = 40, 5
    enc = synth_octuple_batch(N, S, seed=5, min_len=S // 2)[5].numpy()
    np.save(str(tmp_path / 'prompts.npy'), enc)
    base = ['--dataset_path', str(tmp_path), '--dataset_name', 'prompts.npy', '--max_seq_len', str(S), '--hs', '256', '--layers', '2',
            '--ffn_dims', '512', '--heads', '4', '--nopretrain', '--prime', 'half', '--seed', '3']

    def run(name, bs, *extra):
        torch.manual_seed(0)
        out = str(tmp_path / name)
        EG.eval_generation(EG.get_args(base + ['--output', out, '--batch_size', str(bs)] + list(extra)))
        return out

    a, b = run('k1.npy', 1, '--keep', 'bar,position,duration'), run('k16.npy', 16, '--keep', 'bar,position,duration')
    plain = np.load(run('p16.npy', 16))
    assert open(a, 'rb').read() == open(b, 'rb').read()
    y = np.load(a)
    assert y.shape == plain.shape == (N, S, 8) and y.dtype == plain.dtype == np.float32
    ks = EG.prime_lengths(enc, 'half', 256, PAD)
    kept = [0, 1, 4]
    lengths = []
    for i, k in enumerate(ks):
        n = _length(y[i])
        end = int(np.flatnonzero(enc[i, :, 0] >= 256)[0])              # the piece's EOS row: the kept bar id ends the row there at the latest
        assert k > 0 and k <= n <= end, (i, k, n, end)
        assert np.array_equal(y[i, :k], enc[i, :k].astype(np.float32)), i
        assert np.array_equal(y[i, k:n][:, kept], enc[i, k:n][:, kept].astype(np.float32)), i
        lengths.append(n - k)
    assert max(lengths) > 0
    assert not np.array_equal(y, plain)
