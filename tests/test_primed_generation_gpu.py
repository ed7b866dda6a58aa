"""GPU: primed generation -- continue a piece from a given decoder prefix (Engine.generate(prefix=...), Engine.generate_batch(prefix=...,
prefix_len=...), PianoBartLM.forward(generate=True, decoder_prefix=...), eval_generation --prime).

Contract: primed generation of prompt b is the reference loop (model.py:28-66) with decoder inputs 1 .. k_b and their mask set to the prefix,
the loop starting at position k_b and result[:, :k_b] = prefix; forced positions draw nothing. The self-attention cache rows of the prefix come
from one teacher-forced decoder pass per prompt (Engine._prefill); the fused decoder starts each row at its own position with its own limit
(pb_batch_decoder_start)."""
import numpy as np
import pytest
import torch

from tests.golden_util import load_vocab, randomize_params, synth_octuple_batch

pytestmark = pytest.mark.gpu
E2W, W2E = load_vocab()
PAD = [256, 128, 129, 256, 128, 32, 254, 49]
SOS = [258, 130, 131, 258, 130, 34, 256, 51]


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


def _oracle_primed(o, enc, emask, pre):
    """The reference loop (model.py:28-66) with the prefix filled in, on the CPU oracle."""
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
        x = o.mask_lm(o.pianobart(enc, dec, emask, dmask))
        cur = o.sample(x, i)
        if i != S - 1:
            dec[:, i + 1] = cur
            dmask[:, i + 1] += 1
        if (cur >= pad).any():
            break
        result[:, i] = cur
    return result


@pytest.mark.parametrize('k', [0, 1, 7, 19, 20])
def test_primed_generate_against_the_oracle(k):
    _need_gpu()
    from oracle import pianobart_oracle as O
    S = 20
    m = _lm(S, 64, 2, 128, 2, 60 + k, 'fp32')
    o = O.PianoBartLM(O.PianoBart(O.BartConfig(max_position_embeddings=S, d_model=64, encoder_layers=2, decoder_layers=2, encoder_ffn_dim=128,
                                               decoder_ffn_dim=128, encoder_attention_heads=2, decoder_attention_heads=2), E2W, W2E)).eval()
    o.load_state_dict(m.state_dict(), strict=True)
    m = m.cuda()
    enc = synth_octuple_batch(1, S, seed=300 + k, min_len=12)[5]
    emask = (enc[:, :, 0] != 256).float()
    pre = _piece(k, 400 + k)
    with torch.no_grad():
        np.random.seed(777 + k)
        want = _oracle_primed(o, enc, emask, pre)
        st_o = np.random.get_state()
        np.random.seed(777 + k)
        got = m(enc.cuda(), None, emask.cuda(), None, generate=True, device_num=0, decoder_prefix=pre[None])
        st_m = np.random.get_state()
    assert got.shape == want.shape and torch.equal(got.cpu(), want)
    assert _same_state(st_o, st_m)
    assert torch.equal(got[0, :k].cpu(), pre)


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_primed_paths_agree(precision):
    _need_gpu()
    S, k = 48, 17
    m = _lm(S, 256, 2, 256, 4, 77, precision, specials='off').cuda()
    enc, emask = _prompts(1, S, seed=4)
    pre = _piece(k, 5)
    eng = m._get_engine()
    sampler = dict(T=m.SAMPLE_T, P=m.SAMPLE_P)

    def run(fn):
        np.random.seed(5)
        out = fn().cpu()
        return out, np.random.get_state()

    a, sa = run(lambda: eng.generate(enc, emask, m.sample_row, prefix=pre[None]))                       # fp32: pb_decode_step, bf16: fused host-sampled
    s, ss = run(lambda: eng.generate(enc, emask, m.sample_row, sampler=sampler, prefix=pre[None]))      # bf16: fused device-sampled
    b, sb = run(lambda: eng.generate(enc, emask, m.sample_row, use_cache=False, prefix=pre[None]))
    c, sc = run(lambda: eng._generate_pyloop(enc, emask, m.sample_row, k, pre))
    assert torch.equal(b, c) and _same_state(sb, sc)                        # same kernels: bitwise
    assert torch.equal(a, s) and _same_state(sa, ss)                        # the host's token always wins
    if precision == 'fp32':
        assert torch.equal(a, b) and _same_state(sa, sb)
    for out in (a, b):
        assert torch.equal(out[0, :k], pre) and int((out[0, :, 0] != 256).sum()) == S
    # the forced-token logits rows of the cached path against the python-sequenced cache (as test_generate_kv_cache_equals_full_rerun)
    forced = b[0]

    def recorder(store):
        def fn(row):
            store.append(row.clone())
            return forced[k + len(store) - 1].clone()
        return fn
    la, lc = [], []
    eng.generate(enc, emask, recorder(la), prefix=pre[None])
    eng._generate_pyloop(enc, emask, recorder(lc), k, pre)
    assert len(la) == len(lc) == S - k
    tol = 1e-4 if precision == 'fp32' else 3e-2
    for i, (x, y) in enumerate(zip(la, lc)):
        keep = y > -20
        rel = float((x[keep] - y[keep]).abs().max() / y[keep].abs().max())
        assert rel < tol, (i, rel)


@pytest.mark.parametrize('precision,tol', [('fp32', 2e-4), ('bf16', 4e-2)])
def test_prefill_at_cfg2_size_matches_teacher_forced_full_pass(precision, tol):
    """configs[3] shape (12L / 768 / 12 heads, S = 1024): primed with 512 rows, then 96 forced tokens; every logits row from position 512 on
    against ONE teacher-forced full pass over prefix + forced tokens."""
    _need_gpu()
    S, k, N = 1024, 512, 96
    m = _lm(S, 768, 12, 3072, 12, 41, precision, specials='off').cuda()
    enc = synth_octuple_batch(1, S, seed=19, min_len=700)[5].cuda()
    emask = (enc[:, :, 0] != 256).float()
    pre = _piece(k, 21)
    forced = _piece(N, 23)
    rows = []

    def feed(row):
        rows.append(row.clone())
        return forced[len(rows) - 1].clone() if len(rows) <= N else torch.tensor(PAD)

    eng = m._get_engine()
    out = eng.generate(enc, emask, feed, prefix=pre[None])
    assert len(rows) == N + 1 and torch.equal(out[0, :k].cpu(), pre) and torch.equal(out[0, k:k + N].cpu(), forced)
    if precision == 'bf16':
        print('prefill %d rows (bf16, 12L/768): %.2f ms' % (k, eng.last_decode['prefill_ms']))
    dec = torch.tensor(PAD).repeat(1, S, 1)
    dec[0, 0] = torch.tensor(SOS)
    dec[0, 1:k + 1] = pre
    dec[0, k + 1:k + N + 1] = forced
    dmask = torch.zeros(1, S)
    dmask[0, :k + N + 1] = 1
    with torch.no_grad():
        full = torch.cat(m(enc, dec.cuda(), emask, dmask.cuda()), dim=-1)[0].float().cpu()
    worst = 0.0
    for j in range(N + 1):
        keep = full[k + j] > -20
        worst = max(worst, float((rows[j][keep] - full[k + j][keep]).abs().max() / full[k + j][keep].abs().max()))
    print('primed decode 12L/768 S=1024 k=512 (%s): worst logits rel over %d steps = %.2e' % (precision, N + 1, worst))
    assert worst < tol
    if precision == 'fp32':
        offs = np.cumsum([0, 262, 134, 135, 262, 134, 38, 260, 55])
        a = torch.stack([torch.stack([r[offs[h]:offs[h + 1]].argmax() for h in range(8)]) for r in rows])
        b = torch.stack([torch.stack([full[k + j][offs[h]:offs[h + 1]].argmax() for h in range(8)]) for j in range(N + 1)])
        assert float((a == b).float().mean()) > 0.995


def _batch_setup(S=64, n=17, seed=31):
    m = _lm(S, 256, 2, 512, 4, seed, 'bf16', specials='eos').cuda()
    enc, emask = _prompts(n, S, seed=40)
    prefix = torch.stack([_piece(S, 500 + b) for b in range(n)])
    lens = [0, 1, 23, S - 1, S, 5, 0, 40, 2, S - 1, 31, 0, 7, 60, 12, 3, 33][:n]
    return m, enc, emask, prefix, lens


def _reference(eng, m, enc, emask, prefix, lens, seeds, max_new=None):
    outs, states, infos = [], [], []
    for b, s in enumerate(seeds):
        np.random.set_state(np.random.RandomState(s).get_state())
        outs.append(eng.generate(enc[b:b + 1], emask[b:b + 1], m.sample_row, max_new=max_new, sampler=dict(T=m.SAMPLE_T, P=m.SAMPLE_P),
                                 prefix=prefix[b:b + 1, :lens[b]]).cpu()[0])
        states.append(np.random.get_state())
        infos.append(dict(eng.last_decode))
    return outs, states, infos


def _batched(eng, m, enc, emask, prefix, lens, seeds, max_new=None):
    rngs = [np.random.RandomState(s) for s in seeds]
    out = eng.generate_batch(enc, emask, m.sample_row, rngs, max_new=max_new, sampler=dict(T=m.SAMPLE_T, P=m.SAMPLE_P),
                             prefix=prefix, prefix_len=lens).cpu()
    return out, [r.get_state() for r in rngs], dict(eng.last_decode)


def test_primed_batch_equals_batch1_per_prompt():
    _need_gpu()
    m, enc, emask, prefix, lens = _batch_setup()
    eng = m._get_engine()
    seeds = [1000 + 7 * b for b in range(len(lens))]
    want, w_state, w_info = _reference(eng, m, enc, emask, prefix, lens, seeds)
    print('primed batch-1 positions per prompt', [int(i['tokens']) for i in w_info])

    def check(idx, tag, max_new=None, ref=(want, w_state)):
        got, states, info = _batched(eng, m, enc[idx], emask[idx], prefix[idx], [lens[i] for i in idx], [seeds[i] for i in idx], max_new)
        for j, i in enumerate(idx):
            assert torch.equal(got[j], ref[0][i]), (tag, j, i)
            assert _same_state(states[j], ref[1][i]), (tag, j, i)
            assert torch.equal(got[j, :lens[i]], prefix[i, :lens[i]]), (tag, j, i)
        return info

    info = check(list(range(16)), 'B=16')
    assert info['batched'] and info['prefix'] == lens[:16]
    check(list(np.random.RandomState(3).permutation(16)), 'B=16 shuffled')
    check(list(range(17)), 'B=17 (chunks of 16 + 1)')
    check([4, 0], 'B=2')
    for cut in (1, 9):
        ref = _reference(eng, m, enc, emask, prefix, lens, seeds, max_new=cut)
        info = check(list(range(16)), 'max_new=%d' % cut, max_new=cut, ref=ref[:2])
        assert all(t <= cut for t in info['tokens'])


def test_unprimed_rows_are_todays_rows():
    """prefix_len = 0 everywhere: bit for bit what generate_batch returns without a prefix."""
    _need_gpu()
    m, enc, emask, prefix, _ = _batch_setup(n=5)
    eng = m._get_engine()
    seeds = [11, 12, 13, 14, 15]
    rngs = [np.random.RandomState(s) for s in seeds]
    want = eng.generate_batch(enc, emask, m.sample_row, rngs, sampler=dict(T=m.SAMPLE_T, P=m.SAMPLE_P)).cpu()
    got, states, _ = _batched(eng, m, enc, emask, prefix, [0] * 5, seeds)
    assert torch.equal(got, want)
    assert all(_same_state(a, r.get_state()) for a, r in zip(states, rngs))


def test_rewind_of_a_primed_row():
    _need_gpu()
    m, enc, emask, prefix, lens = _batch_setup(n=4)
    lens = [9, 0, 30, 17]
    eng = m._get_engine()
    seeds = [21, 22, 23, 24]
    want, w_state, w_info = _reference(eng, m, enc, emask, prefix, lens, seeds)
    clean, _, c_info = _batched(eng, m, enc, emask, prefix, lens, seeds)
    fr = max((b for b in (0, 2, 3)), key=lambda b: w_info[b]['tokens'])
    assert w_info[fr]['tokens'] >= 6, w_info
    eng.decode_fault_row = (fr, 3)
    try:
        got, g_state, g_info = _batched(eng, m, enc, emask, prefix, lens, seeds)
    finally:
        eng.decode_fault_row = None
    for b in range(4):
        assert torch.equal(got[b], want[b]) and torch.equal(clean[b], want[b]), b
        assert _same_state(g_state[b], w_state[b]), b
        if b != fr:
            assert g_info['rewinds'][b] == c_info['rewinds'][b], b
    assert g_info['rewinds'][fr] > c_info['rewinds'][fr]


def test_eval_generation_prime_half(tmp_path):
    _need_gpu()
    from pianobart_amd import eval_generation as EG
    S, N = 40, 5
    enc = synth_octuple_batch(N, S, seed=5, min_len=S // 2)[5].numpy()
    np.save(str(tmp_path / 'prompts.npy'), enc)
    base = ['--dataset_path', str(tmp_path), '--dataset_name', 'prompts.npy', '--max_seq_len', str(S), '--hs', '256', '--layers', '2',
            '--ffn_dims', '512', '--heads', '4', '--nopretrain', '--prime', 'half', '--seed', '3']

    def run(name, bs):
        torch.manual_seed(0)
        out = str(tmp_path / name)
        EG.eval_generation(EG.get_args(base + ['--output', out, '--batch_size', str(bs)]))
        return out

    a, b = run('p1.npy', 1), run('p16.npy', 16)
    assert open(a, 'rb').read() == open(b, 'rb').read()
    y = np.load(a)
    ks = EG.prime_lengths(enc, 'half', 256, PAD)
    assert all(k > 0 for k in ks)
    for i, k in enumerate(ks):
        assert np.array_equal(y[i, :k], enc[i, :k].astype(np.float32)), i
