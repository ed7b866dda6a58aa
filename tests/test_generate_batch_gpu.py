"""GPU: batched KV-cached generation (Engine.generate_batch / PianoBartLM.generate_batch, pb_batch_decoder_*) against the batch-1 path.

Contract: for every prompt b, the batched result equals the batch-1 device-sampled `generate` of that prompt alone with the global RNG set
to rngs[b]'s state, token for token, and rngs[b] ends where the global RNG ends -- for any batch composition, order and size. The logged
logits rows are bit-identical to the batch-1 fused decoder's for the same fed tokens; a row whose device choice is corrupted is rewound
alone; shapes the batched decoder does not cover run the per-prompt loop. eval_generation writes the same file for every --batch_size.
"""
import os

import numpy as np
import pytest
import torch

from tests.golden_util import load_vocab, randomize_params, synth_octuple_batch

pytestmark = pytest.mark.gpu
E2W, W2E = load_vocab()
PAD = [256, 128, 129, 256, 128, 32, 254, 49]
SHAPES = [(256, 4, 200, 1.0), (768, 12, 130, 1.0), (512, 8, 72, 40.0), (1024, 8, 40, 8.0)]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


def _lm(S, d, L, f, h, seed, precision, sharp=1.0):
    from pianobart_amd.model import BartConfig, PianoBart, PianoBartLM
    cfg = BartConfig(max_position_embeddings=S, d_model=d, encoder_layers=L, decoder_layers=L, encoder_ffn_dim=f, decoder_ffn_dim=f,
                     encoder_attention_heads=h, decoder_attention_heads=h, dropout=0.0)
    m = PianoBartLM(PianoBart(cfg, E2W, W2E, precision=precision))
    randomize_params(m, seed)
    with torch.no_grad():                      # the LM biases of tests/test_model_gpu.py's device-sampled test: flat or peaked heads
        for i, p0 in enumerate(PAD):
            m.mask_lm.proj[i].weight.mul_(sharp)
            m.mask_lm.proj[i].bias[p0 + 3:] = -30.0
            m.mask_lm.proj[i].bias[p0:p0 + 3] = -30.0
        # EOS of the tempo head (nucleus p = 0.9) as likely as its most favoured class: rows stop at different positions
        m.mask_lm.proj[7].bias[PAD[7] + 3] = m.mask_lm.proj[7].bias[:PAD[7]].max()
    return m.cuda().eval()


def _prompts(n, S, seed):
    """n prompts of different visible lengths: #0 nearly all PAD (one row + EOS), #1 without PAD, the others S/2 .. S."""
    enc = synth_octuple_batch(n, S, seed=seed, min_len=S // 2)[5]
    full = synth_octuple_batch(1, S, seed=seed + 1, min_len=S)[5]
    enc[1] = full[0]
    enc[1, -1] = enc[1, 0]                      # no EOS / PAD row: every encoder position visible
    enc[0, 2:] = torch.tensor(PAD)
    enc[0, 1] = torch.tensor(PAD) + 3
    enc = enc.cuda()
    return enc, (enc[:, :, 0] != 256).float()


def _reference(eng, m, enc, emask, seeds, max_new=None):
    """The batch-1 device-sampled generate of each prompt under its generator's state: (tokens, final states, infos)."""
    sampler = dict(T=m.SAMPLE_T, P=m.SAMPLE_P)
    outs, states, infos = [], [], []
    for b, s in enumerate(seeds):
        np.random.set_state(np.random.RandomState(s).get_state())
        outs.append(eng.generate(enc[b:b + 1], emask[b:b + 1], m.sample_row, max_new=max_new, sampler=sampler).cpu()[0])
        states.append(np.random.get_state())
        infos.append(dict(eng.last_decode or {}))
    return outs, states, infos


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def _batched(eng, m, enc, emask, seeds, max_new=None):
    rngs = [np.random.RandomState(s) for s in seeds]
    out = eng.generate_batch(enc, emask, m.sample_row, rngs, max_new=max_new, sampler=dict(T=m.SAMPLE_T, P=m.SAMPLE_P)).cpu()
    return out, [r.get_state() for r in rngs], dict(eng.last_decode)


@pytest.mark.parametrize('d,heads,S,sharp', SHAPES)
def test_generate_batch_matches_batch1_per_prompt(d, heads, S, sharp):
    _need_gpu()
    m = _lm(S, d, 2, 512, heads, 31, 'bf16', sharp)
    eng = m._get_engine()
    enc, emask = _prompts(17, S, seed=40 + d)
    seeds = [1000 + 7 * b for b in range(17)]
    want, w_state, w_info = _reference(eng, m, enc, emask, seeds)
    lens = [int(i['tokens']) for i in w_info]
    print('d=%d S=%d: batch-1 positions per prompt %s' % (d, S, lens))

    def check(idx, tag):
        global_before = np.random.get_state()
        got, states, info = _batched(eng, m, enc[idx], emask[idx], [seeds[i] for i in idx])
        assert _same_state(global_before, np.random.get_state()), tag          # the global stream is not touched
        assert got.shape == (len(idx), S, 8), tag
        for k, i in enumerate(idx):
            assert torch.equal(got[k], want[i]), (tag, k, i)
            assert _same_state(states[k], w_state[i]), (tag, k, i)
        return info

    info = check([0], 'B=1')
    assert info['batched'] and info['graph'] and info['launches_per_token'] == 6 * 2 + 3
    check([5, 0, 1], 'B=3')
    info = check(list(range(16)), 'B=16')
    assert info['batch'] == 16
    check(list(np.random.RandomState(3).permutation(16)), 'B=16 shuffled')
    check(list(range(17)), 'B=17 (chunks of 16 + 1)')


def _forced_rows(eng, m, enc, emask, forced, batched):
    """Feed `forced[b]` (S, 8) through a sample_row-shaped callback; returns the logits rows the callback saw, per prompt."""
    B, S = enc.shape[0], enc.shape[1]
    seen = [[] for _ in range(B)]
    sampler = dict(T=m.SAMPLE_T, P=m.SAMPLE_P)
    if batched:
        rngs = [np.random.RandomState(b) for b in range(B)]
        row_of = {id(r): b for b, r in enumerate(rngs)}

        def cb(row, rng):
            b = row_of[id(rng)]
            seen[b].append(row.clone())
            return forced[b, len(seen[b]) - 1].clone()
        eng.generate_batch(enc, emask, cb, rngs, sampler=sampler)
    else:
        for b in range(B):
            def cb(row, b=b):
                seen[b].append(row.clone())
                return forced[b, len(seen[b]) - 1].clone()
            eng.generate(enc[b:b + 1], emask[b:b + 1], cb, sampler=sampler)
    return seen, dict(eng.last_decode)


@pytest.mark.parametrize('d,heads,S,sharp', SHAPES)
def test_batched_decoder_logits_are_bit_identical(d, heads, S, sharp):
    _need_gpu()
    m = _lm(S, d, 2, 512, heads, 32, 'bf16', sharp)
    eng = m._get_engine()
    enc, emask = _prompts(3, S, seed=60 + d)
    g = np.random.RandomState(5)
    forced = torch.from_numpy(np.stack([g.randint(0, np.asarray(PAD), size=(S, 8)) for _ in range(3)]).astype(np.int64))
    want, info1 = _forced_rows(eng, m, enc, emask, forced, batched=False)
    got, infob = _forced_rows(eng, m, enc, emask, forced, batched=True)
    assert infob['batched'] and infob['launches_per_token'] == info1['launches_per_token'] == 6 * 2 + 3
    for b in range(3):
        assert len(got[b]) == len(want[b]) == S
        for i in range(S):
            assert torch.equal(got[b][i], want[b][i]), (b, i, float((got[b][i] - want[b][i]).abs().max()))


@pytest.mark.parametrize('d,heads,S,sharp', [SHAPES[0], SHAPES[3]])
def test_rewind_of_one_row_leaves_the_others_alone(d, heads, S, sharp):
    _need_gpu()
    m = _lm(S, d, 2, 512, heads, 33, 'bf16', sharp)
    eng = m._get_engine()
    enc, emask = _prompts(4, S, seed=80 + d)
    seeds = [11, 12, 13, 14]
    want, w_state, w_info = _reference(eng, m, enc, emask, seeds)
    clean, c_state, c_info = _batched(eng, m, enc, emask, seeds)
    fr = int(np.argmax([i['tokens'] for i in w_info]))
    assert w_info[fr]['tokens'] >= 6, w_info
    eng.decode_fault_row = (fr, 3)                # head 0's id of row fr corrupted at every 3rd position: a logical substitution
    try:
        got, g_state, g_info = _batched(eng, m, enc, emask, seeds)
    finally:
        eng.decode_fault_row = None
    for b in range(4):
        assert torch.equal(got[b], want[b]) and torch.equal(clean[b], want[b]), b
        assert _same_state(g_state[b], w_state[b]) and _same_state(c_state[b], w_state[b]), b
        assert g_info['tokens'][b] == c_info['tokens'][b] == w_info[b]['tokens'], b
        if b != fr:
            assert g_info['rewinds'][b] == c_info['rewinds'][b], (b, g_info['rewinds'], c_info['rewinds'])
    assert g_info['rewinds'][fr] > c_info['rewinds'][fr] and g_info['rewinds'][fr] >= min(w_info[fr]['tokens'], S) // 3 - 1, g_info
    for cut in (1, 8, 13):
        want_c, ws_c, _ = _reference(eng, m, enc, emask, seeds, max_new=cut)
        got_c, gs_c, gi_c = _batched(eng, m, enc, emask, seeds, max_new=cut)
        for b in range(4):
            assert torch.equal(got_c[b], want_c[b]) and _same_state(gs_c[b], ws_c[b]), (cut, b)
            assert gi_c['tokens'][b] <= cut


def test_generate_batch_falls_back_to_the_per_prompt_loop():
    _need_gpu()
    S = 40
    m = _lm(S, 256, 2, 512, 4, 34, 'fp32')
    eng = m._get_engine()
    enc, emask = _prompts(3, S, seed=90)
    seeds = [21, 22, 23]
    want, w_state, _ = _reference(eng, m, enc, emask, seeds)
    np.random.seed(77)
    before = np.random.get_state()
    got, states, info = _batched(eng, m, enc, emask, seeds)
    assert not info['batched']
    assert _same_state(before, np.random.get_state())
    for b in range(3):
        assert torch.equal(got[b], want[b]) and _same_state(states[b], w_state[b]), b
    # the module surface: seeds, placement as forward(generate=True)
    y = m.generate_batch(enc, emask, seeds=seeds, device_num=-1)
    assert y.device.type == 'cpu' and all(torch.equal(y[b], want[b]) for b in range(3))


def test_eval_generation_end_to_end(tmp_path):
    _need_gpu()
    from pianobart_amd import eval_generation as EG
    S, N = 40, 5
    enc = synth_octuple_batch(N, S, seed=5, min_len=S // 2)[5].numpy()
    np.save(str(tmp_path / 'prompts.npy'), enc)
    base = ['--dataset_path', str(tmp_path), '--dataset_name', 'prompts.npy', '--max_seq_len', str(S), '--hs', '256', '--layers', '2',
            '--ffn_dims', '512', '--heads', '4', '--nopretrain']

    def run(name, *extra):
        torch.manual_seed(0)                     # --nopretrain: the same random initialisation in every run
        out = str(tmp_path / name)
        EG.eval_generation(EG.get_args(base + ['--output', out] + list(extra)))
        return out

    a = run('s1.npy', '--seed', '3', '--batch_size', '1')
    b = run('s4.npy', '--seed', '3', '--batch_size', '4')
    ya = np.load(a)
    assert ya.shape == (N, S, 8) and ya.dtype == np.float32
    assert open(a, 'rb').read() == open(b, 'rb').read()
    np.random.seed(11)
    c = np.load(run('g1.npy', '--batch_size', '1'))
    # the reference's loop: one global stream, forward(generate=True) per prompt
    torch.manual_seed(0)
    args = EG.get_args(base)
    model = EG.build_model(args, E2W, W2E).cuda().eval()
    np.random.seed(11)
    x = torch.from_numpy(enc).long().cuda()
    loop = [model(input_ids_encoder=x[i:i + 1], encoder_attention_mask=(x[i:i + 1, :, 0] != 256).float(), generate=True, device_num=-1)
            for i in range(N)]
    assert np.array_equal(c, torch.cat(loop).float().numpy())
