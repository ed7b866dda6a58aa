"""GPU: several samples of one prompt from one shared encoder pass and cross K/V (PianoBartLM.generate_batch(samples_per_prompt=...),
Engine.generate_batch(samples=...), pb_batch_decoder_share_cross, eval_generation --samples).

Contract: every output row is the batch-1 `generate` of its prompt under its own generator (the contract of test_generate_batch_gpu.py), so a
grouped call equals generate_batch on the explicitly repeated prompts with the same seeds, token for token and generator state for generator
state, and the logits rows the host sees are bit-identical -- with the grouped cross-attention kernel and with the per-row kernel reading the
shared slice (PB_DECODE_CROSS_GROUPED=0). What changes is the accounting: encoder passes, prefill passes and cross-cache bytes per distinct
prompt of a chunk, not per row."""
import os

import numpy as np
import pytest
import torch

from tests.golden_util import synth_octuple_batch
from tests.test_generate_batch_gpu import E2W, PAD, SHAPES, W2E, _forced_rows, _lm, _need_gpu, _prompts, _same_state

pytestmark = pytest.mark.gpu


def _sampler(m):
    return dict(T=m.SAMPLE_T, P=m.SAMPLE_P)


def _three_prompts(S, seed):
    """#0 nearly all PAD, #1 without PAD, #2 an ordinary one."""
    return _prompts(3, S, seed)


def _expand(t, counts):
    idx = torch.as_tensor([p for p, n in enumerate(counts) for _ in range(n)], device=t.device)
    return t[idx]


def _grouped(eng, m, enc, emask, seeds, counts, **kw):
    rngs = [np.random.RandomState(s) for s in seeds]
    out = eng.generate_batch(enc, emask, m.sample_row, rngs, sampler=_sampler(m), samples=counts, **kw).cpu()
    return out, [r.get_state() for r in rngs], dict(eng.last_decode)


def _repeated(eng, m, enc, emask, seeds, counts, prefix=None, prefix_len=None, **kw):
    counts = [counts] * int(enc.shape[0]) if isinstance(counts, int) else list(counts)
    rngs = [np.random.RandomState(s) for s in seeds]
    if prefix is not None:
        kw['prefix'] = _expand(prefix, counts)
        kw['prefix_len'] = [k for k, n in zip(prefix_len, counts) for _ in range(n)] if prefix_len is not None else None
    out = eng.generate_batch(_expand(enc, counts), _expand(emask, counts), m.sample_row, rngs, sampler=_sampler(m), **kw).cpu()
    return out, [r.get_state() for r in rngs], dict(eng.last_decode)


def _batch1(eng, m, enc1, emask1, seed):
    np.random.set_state(np.random.RandomState(seed).get_state())
    out = eng.generate(enc1, emask1, m.sample_row, sampler=_sampler(m)).cpu()[0]
    return out, np.random.get_state()


@pytest.mark.parametrize('d,heads,S,sharp', SHAPES)
def test_samples_equal_the_repeated_prompts_and_batch1(d, heads, S, sharp):
    _need_gpu()
    m = _lm(S, d, 2, 512, heads, 41, 'bf16', sharp)
    eng = m._get_engine()
    enc, emask = _three_prompts(S, seed=140 + d)

    def check(enc_, emask_, counts, tag):
        P = int(enc_.shape[0])
        cl = [counts] * P if isinstance(counts, int) else list(counts)
        owner = [p for p, n in enumerate(cl) for _ in range(n)]
        seeds = [500 + 3 * r for r in range(len(owner))]
        want, w_state, _ = _repeated(eng, m, enc_, emask_, seeds, cl)
        np.random.seed(123)
        before = np.random.get_state()
        got, g_state, info = _grouped(eng, m, enc_, emask_, seeds, counts)
        assert _same_state(before, np.random.get_state()), tag              # the global stream is not touched
        assert got.shape == (len(owner), S, 8), tag
        assert torch.equal(got, want), tag
        for r in range(len(owner)):
            assert _same_state(g_state[r], w_state[r]), (tag, r)
        for r in sorted({0, len(owner) // 2, len(owner) - 1, min(len(owner) - 1, 1)})[:4]:      # and the batch-1 generate of the row's prompt
            p = owner[r]
            ref, ref_state = _batch1(eng, m, enc_[p:p + 1], emask_[p:p + 1], seeds[r])
            assert torch.equal(got[r], ref) and _same_state(g_state[r], ref_state), (tag, r)
        np.random.set_state(before)
        return info, owner

    info, owner = check(enc, emask, [1, 5, 10], 'counts 1, 5, 10')
    assert info['batched'] and info['groups'] == owner and info['encoder_passes'] == 3
    info, owner = check(enc, emask, 4, 'uniform 4')
    assert info['groups'] == owner and info['batch'] == 12
    info, _ = check(enc[2:3], emask[2:3], 17, 'one prompt, 17 samples (chunks of 16 + 1)')
    assert info['batch'] == 1 and info['groups'] == [0] and info['encoder_passes'] == 1
    # the module surface
    y = m.generate_batch(enc, emask, seeds=list(range(7)), samples_per_prompt=[2, 4, 1], device_num=-1)
    want, _, _ = _repeated(eng, m, enc, emask, list(range(7)), [2, 4, 1])
    assert y.device.type == 'cpu' and torch.equal(y, want)


@pytest.mark.parametrize('variant', ['grouped', 'indirect'])
@pytest.mark.parametrize('d,heads,S,sharp', SHAPES)
def test_grouped_logits_are_bit_identical(d, heads, S, sharp, variant, monkeypatch):
    _need_gpu()
    monkeypatch.setenv('PB_DECODE_CROSS_GROUPED', '1' if variant == 'grouped' else '0')
    m = _lm(S, d, 2, 512, heads, 42, 'bf16', sharp)
    eng = m._get_engine()
    enc, emask = _three_prompts(S, seed=160 + d)
    counts = [3, 6, 5]                                 # tiles of 3, 3 + 3 and 3 + 2 rows
    owner = [p for p, n in enumerate(counts) for _ in range(n)]
    R = len(owner)
    g = np.random.RandomState(6)
    forced = torch.from_numpy(np.stack([g.randint(0, np.asarray(PAD), size=(S, 8)) for _ in range(R)]).astype(np.int64))
    want, info_r = _forced_rows(eng, m, _expand(enc, counts), _expand(emask, counts), forced, batched=True)
    assert 'groups' in info_r and info_r['encoder_passes'] == R          # the repeated prompts: one pass and one cache slice per row

    seen = [[] for _ in range(R)]
    rngs = [np.random.RandomState(b) for b in range(R)]
    row_of = {id(r): b for b, r in enumerate(rngs)}

    def cb(row, rng):
        b = row_of[id(rng)]
        seen[b].append(row.clone())
        return forced[b, len(seen[b]) - 1].clone()
    eng.generate_batch(enc, emask, cb, rngs, sampler=_sampler(m), samples=counts)
    info = dict(eng.last_decode)
    assert info['batched'] and info['groups'] == owner and info['encoder_passes'] == 3
    assert info['launches_per_token'] == info_r['launches_per_token'] == 6 * 2 + 3
    for b in range(R):
        assert len(seen[b]) == len(want[b]) == S
        for i in range(S):
            assert torch.equal(seen[b][i], want[b][i]), (variant, b, i, float((seen[b][i] - want[b][i]).abs().max()))


@pytest.mark.parametrize('d,heads,S,sharp', [SHAPES[0], SHAPES[1]])
def test_samples_share_their_prompts_prefix(d, heads, S, sharp):
    _need_gpu()
    m = _lm(S, d, 2, 512, heads, 43, 'bf16', sharp)
    eng = m._get_engine()
    enc, emask = _three_prompts(S, seed=180 + d)
    enc = torch.cat([enc, enc[2:3]], 0)
    emask = torch.cat([emask, emask[2:3]], 0)
    K = S // 2 + 3
    piece = synth_octuple_batch(4, K + 2, seed=9, min_len=K + 2)[5][:, :K]           # ordinary rows only
    ks = [0, 5, K, 1]                                   # unprimed, short, k >= S // 2, one row
    counts = [2, 4, 5, 3]
    seeds = [900 + r for r in range(sum(counts))]
    want, w_state, info_r = _repeated(eng, m, enc, emask, seeds, counts, prefix=piece, prefix_len=ks)
    assert info_r['prefill_passes'] == 4 + 5 + 3
    got, g_state, info = _grouped(eng, m, enc, emask, seeds, counts, prefix=piece, prefix_len=ks)
    assert torch.equal(got, want)
    assert all(_same_state(a, b) for a, b in zip(g_state, w_state))
    assert info['prefill_passes'] == 3 and info['encoder_passes'] == 4
    assert info['prefix'] == [k for k, n in zip(ks, counts) for _ in range(n)]
    r = 2 + 4                                            # first sample of the long-prefix prompt
    assert torch.equal(got[r, :K], piece[2]) and torch.equal(got[r + 4, :K], piece[2])
    # every prompt primed with the whole prefix (prefix_len None), through the module surface
    y = m.generate_batch(enc[1:3], emask[1:3], seeds=[1, 2, 3, 4], decoder_prefix=piece[1:3], samples_per_prompt=2, device_num=-1)
    assert eng.last_decode['prefill_passes'] == 2 and eng.last_decode['groups'] == [0, 0, 1, 1]
    want2, _, _ = _repeated(eng, m, enc[1:3], emask[1:3], [1, 2, 3, 4], [2, 2], prefix=piece[1:3], prefix_len=[K, K])
    assert torch.equal(y, want2)


@pytest.mark.parametrize('d,heads,S,sharp', [SHAPES[0], SHAPES[3]])
def test_rewind_of_one_sample_leaves_its_siblings_alone(d, heads, S, sharp):
    _need_gpu()
    m = _lm(S, d, 2, 512, heads, 44, 'bf16', sharp)
    eng = m._get_engine()
    enc, emask = _three_prompts(S, seed=200 + d)
    counts = [4, 4, 4]                                  # every row sits in a group of four
    seeds = [31 + r for r in range(12)]
    clean, c_state, c_info = _grouped(eng, m, enc, emask, seeds, counts)
    fr = int(np.argmax(c_info['tokens']))               # the row that decodes the most positions
    assert c_info['tokens'][fr] >= 6, c_info
    eng.decode_fault_row = (fr, 3)                     # head 0's id of row fr corrupted at every 3rd position
    try:
        got, g_state, g_info = _grouped(eng, m, enc, emask, seeds, counts)
    finally:
        eng.decode_fault_row = None
    assert g_info['rewinds'][fr] > 0 and g_info['rewinds'][fr] > c_info['rewinds'][fr], (g_info['rewinds'], c_info['rewinds'])
    assert torch.equal(got, clean)
    for b in range(12):
        assert _same_state(g_state[b], c_state[b]), b
        assert g_info['tokens'][b] == c_info['tokens'][b], b
        if b != fr:
            assert g_info['rewinds'][b] == c_info['rewinds'][b], (b, g_info['rewinds'], c_info['rewinds'])
    want, w_state, _ = _repeated(eng, m, enc, emask, seeds, counts)
    assert torch.equal(clean, want) and all(_same_state(a, b) for a, b in zip(c_state, w_state))


def test_accounting_of_a_grouped_chunk():
    _need_gpu()
    d, heads, S, sharp = SHAPES[1]
    L = 2
    m = _lm(S, d, L, 512, heads, 45, 'bf16', sharp)
    eng = m._get_engine()
    enc, emask = _three_prompts(S, seed=220)
    _, _, info = _grouped(eng, m, enc, emask, list(range(16)), [1, 5, 10])
    assert info['batched'] and info['batch'] == 16 and info['groups'] == [0] + [1] * 5 + [2] * 10
    assert info['encoder_passes'] == 3 and info['prefill_passes'] == 0
    assert info['cross_cache_bytes'] == 3 * S * 2 * d * 2 * L
    assert info['launches_per_token'] == 6 * 2 + 3 and info['graph'] is True
    # the last chunk of 20 rows: rows 16 .. 19 are the last four samples of prompt 2
    _, _, info = _grouped(eng, m, enc, emask, list(range(20)), [1, 5, 14])
    assert info['batch'] == 4 and info['groups'] == [0] * 4 and info['encoder_passes'] == 1
    assert info['cross_cache_bytes'] == 1 * S * 2 * d * 2 * L
    _, _, info = _repeated(eng, m, enc, emask, list(range(16)), [1, 5, 10])
    assert info['encoder_passes'] == 16 and info['cross_cache_bytes'] == 16 * S * 2 * d * 2 * L and info['launches_per_token'] == 6 * 2 + 3


@pytest.mark.parametrize('precision,d,heads', [('fp32', 256, 4), ('bf16', 256, 8)])
def test_uncovered_shapes_run_the_per_prompt_loop(precision, d, heads):
    _need_gpu()
    S = 40
    m = _lm(S, d, 2, 512, heads, 46, precision)          # fp32, or head_dim 32: the fused decoder declines
    eng = m._get_engine()
    enc, emask = _three_prompts(S, seed=240)
    counts = [2, 1, 3]
    owner = [0, 0, 1, 2, 2, 2]
    seeds = [61 + r for r in range(6)]
    np.random.seed(78)
    before = np.random.get_state()
    got, g_state, info = _grouped(eng, m, enc, emask, seeds, counts)
    assert not info['batched']
    assert _same_state(before, np.random.get_state())
    want, w_state, _ = _repeated(eng, m, enc, emask, seeds, counts)
    assert torch.equal(got, want)
    for r in range(6):
        assert _same_state(g_state[r], w_state[r]), r
    for r in (0, 2, 5):
        ref, ref_state = _batch1(eng, m, enc[owner[r]:owner[r] + 1], emask[owner[r]:owner[r] + 1], seeds[r])
        assert torch.equal(got[r], ref) and _same_state(g_state[r], ref_state), r
    y = m.generate_batch(enc, emask, seeds=seeds, samples_per_prompt=counts, device_num=-1)
    assert torch.equal(y, want)


def test_share_cross_refuses_bad_maps_and_late_calls():
    _need_gpu()
    import ctypes
    from pianobart_amd._lib import LIB
    d, heads, S, sharp = SHAPES[0]
    m = _lm(S, d, 2, 512, heads, 47, 'bf16', sharp)
    eng = m._get_engine()
    dev = torch.device('cuda', 0)
    eng.bind(dev)
    em = torch.ones(4, S, device=dev)
    bp, bufs = eng._decode_plan(4, S, [S, S, S - 8, S - 8], em, dev, G=2)
    dec = eng._decoder_create(bp)
    assert dec is not None
    err = lambda: LIB.load().pb_last_error().decode()
    try:
        call = lambda g, rows: int(LIB.query('pb_batch_decoder_share_cross', dec, g, np.asarray(rows, dtype=np.int32).ctypes.data))
        assert call(2, [0, 0, 1, 2]) < 0 and 'slice' in err()             # out of range
        assert call(2, [0, -1, 1, 1]) < 0
        assert call(0, [0, 0, 0, 0]) < 0 and call(5, [0, 1, 2, 3]) < 0     # group count outside 1 .. B
        assert call(2, [0, 0, 0, 0]) < 0                                   # slice 1 unused (and rows of unequal s_enc in slice 0)
        assert call(2, [0, 1, 1, 1]) < 0 and 's_enc' in err()              # rows of one slice must have one extent
        assert call(2, [0, 0, 1, 1]) == 0
    finally:
        LIB.call('pb_batch_decoder_destroy', dec)
    # after a step was issued the layout is fixed
    bp, bufs = eng._decode_plan(1, S, [S], em[:1], dev)
    dec = eng._decoder_create(bp)
    try:
        for t in bufs['kvc']:
            t.zero_()
        LIB.call('pb_batch_decoder_reset', dec, torch.cuda.current_stream().cuda_stream, 1)
        tok = np.asarray(eng.pb.sos_word_np, dtype=np.int16)
        out = np.zeros(1280, dtype=np.float32)
        LIB.call('pb_batch_decoder_step', dec, tok.ctypes.data, out.ctypes.data)
        assert int(LIB.query('pb_batch_decoder_share_cross', dec, 1, np.zeros(1, dtype=np.int32).ctypes.data)) < 0
        assert 'already issued' in err()
    finally:
        LIB.call('pb_batch_decoder_destroy', dec)


def test_eval_generation_samples(tmp_path):
    _need_gpu()
    from pianobart_amd import eval_generation as EG
    from pianobart_amd.engine import sample_seed
    S, N, n, seed = 40, 5, 3, 3
    enc = synth_octuple_batch(N, S, seed=5, min_len=S // 2)[5].numpy()
    np.save(str(tmp_path / 'prompts.npy'), enc)
    base = ['--dataset_path', str(tmp_path), '--dataset_name', 'prompts.npy', '--max_seq_len', str(S), '--hs', '256', '--layers', '2',
            '--ffn_dims', '512', '--heads', '4', '--nopretrain']

    def run(name, *extra):
        torch.manual_seed(0)                     # --nopretrain: the same random initialisation in every run
        out = str(tmp_path / name)
        EG.eval_generation(EG.get_args(base + ['--output', out, '--seed', str(seed)] + list(extra)))
        return out

    one = run('one.npy', '--batch_size', '4')
    explicit = run('one_explicit.npy', '--batch_size', '4', '--samples', '1')
    assert open(one, 'rb').read() == open(explicit, 'rb').read()
    files = [run('s3_b%d.npy' % b, '--samples', str(n), '--batch_size', str(b)) for b in (1, 4, 16)]
    y = np.load(files[0])
    assert y.shape == (N, n, S, 8) and y.dtype == np.float32
    assert open(files[0], 'rb').read() == open(files[1], 'rb').read() == open(files[2], 'rb').read()
    assert np.array_equal(y[:, 0], np.load(one))
    torch.manual_seed(0)
    model = EG.build_model(EG.get_args(base), E2W, W2E).cuda().eval()
    x = torch.from_numpy(enc).long().cuda()
    emask = (x[:, :, 0] != 256).float()
    for i in range(N):
        for j in range(n):
            ref = model.generate_batch(x[i:i + 1], emask[i:i + 1], seeds=[sample_seed(seed, j, i, N)], device_num=-1)
            assert sample_seed(seed, j, i, N) == seed + j * N + i
            assert np.array_equal(y[i, j], ref[0].float().numpy()), (i, j)
