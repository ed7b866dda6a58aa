"""GPU: the record a generation call leaves in `Engine.last_decode` -- what bench.py (--mode decode), tools/decode_batch_bench.py and
tools/decode_full_window_check.py read. Pinned per path: the exact key set and, per key, scalar or per-row list (`generate` reports
scalars, the fused batched path one entry per row, the per-prompt loop only that it was not batched, the round-2 per-launch loop nothing).
The batched cases also hold the contract of tests/test_generate_batch_gpu.py at this shape: row b is the batch-1 `generate` of its prompt
under the same generator state. bf16, d 256, 4 heads, 2 + 2 layers, ffn 512, S = 48; the model of tests/test_generate_batch_gpu.py.
"""
import numpy as np
import pytest
import torch

from tests.test_generate_batch_gpu import _lm, _need_gpu, _prompts, _same_state
from tests.test_primed_generation_gpu import _piece

pytestmark = pytest.mark.gpu
S, K_PRIMED = 48, 5

NUM = (int, float)
# the loop records (_decode_device_sampled / _decode_host_sampled) and what `generate` / a fused batch of B rows add to them
DEVICE_LOOP = dict(launches_per_token=int, graph=bool, tokens=int, rewinds=int, steps=int, loop_ms=float, host_ms=float, device_sampler=bool,
                   tokens_per_graph_replay=int)
HOST_LOOP = dict(launches_per_token=int, graph=bool, tokens=int, loop_ms=float)
GENERATE = dict(s_enc=int, prefix=int, prefill_ms=float)
BATCHED = dict(DEVICE_LOOP, tokens=[int], rewinds=[int], s_enc=[int], batched=bool, batch=int, prefix=[int], prefill_ms=NUM, groups=[int],
               encoder_passes=int, prefill_passes=int, setup_ms=float, cross_cache_bytes=int)


def _check_record(info, want, rows=None):
    assert set(info) == set(want), sorted(set(info) ^ set(want))
    for key, t in want.items():
        v = info[key]
        if isinstance(t, list):
            assert isinstance(v, list) and len(v) == rows and all(type(x) is t[0] for x in v), (key, v)
        elif t is NUM:
            assert type(v) in NUM, (key, v)
        else:
            assert type(v) is t, (key, v)


@pytest.fixture(scope='module')
def ctx():
    _need_gpu()
    m = _lm(S, 256, 2, 512, 4, 31, 'bf16')
    eng = m._get_engine()
    enc, emask = _prompts(3, S, seed=77)
    pre = _piece(K_PRIMED, seed=78)
    sampler = dict(T=m.SAMPLE_T, P=m.SAMPLE_P)
    refs = {}

    def ref(p, seed, primed=False):
        """Batch-1 device-sampled `generate` of prompt p under RandomState(seed): (tokens, final state, record), computed once."""
        if (p, seed, primed) not in refs:
            saved = np.random.get_state()
            np.random.set_state(np.random.RandomState(seed).get_state())
            out = eng.generate(enc[p:p + 1], emask[p:p + 1], m.sample_row, sampler=sampler, prefix=pre[None] if primed else None).cpu()[0]
            refs[(p, seed, primed)] = (out, np.random.get_state(), dict(eng.last_decode))
            np.random.set_state(saved)
        return refs[(p, seed, primed)]
    return m, eng, enc, emask, pre, sampler, ref


def _rows_match(ref, got, states, rows):
    """rows: [(prompt, seed, primed)] of the batch, in row order."""
    assert got.shape == (len(rows), S, 8)
    for b, key in enumerate(rows):
        want, w_state, _ = ref(*key)
        assert torch.equal(got[b], want), (b, key)
        assert _same_state(states[b], w_state), (b, key)


def test_generate_device_sampled_record(ctx):
    m, eng, enc, emask, pre, sampler, ref = ctx
    for primed in (False, True):
        out, _, info = ref(1, 1007, primed)
        _check_record(info, dict(DEVICE_LOOP, **GENERATE))
        assert info['device_sampler'] is True and info['graph'] is True and info['tokens_per_graph_replay'] == 8
        assert info['launches_per_token'] == 6 * 2 + 3 and info['prefix'] == (K_PRIMED if primed else 0) and 1 <= info['s_enc'] <= S
        assert info['tokens'] >= 1 and (info['prefill_ms'] > 0) == primed
        if primed:
            assert torch.equal(out[:K_PRIMED], pre)


def test_generate_host_sampled_record(ctx):
    m, eng, enc, emask, pre, sampler, ref = ctx
    want, w_state, w_info = ref(1, 1007)
    saved = np.random.get_state()
    try:
        np.random.set_state(np.random.RandomState(1007).get_state())
        got = eng.generate(enc[1:2], emask[1:2], m.sample_row, sampler=None).cpu()[0]
        state, info = np.random.get_state(), eng.last_decode
    finally:
        np.random.set_state(saved)
    _check_record(info, dict(HOST_LOOP, **GENERATE))
    assert info['graph'] is True and info['launches_per_token'] == 6 * 2 + 2 and info['prefix'] == 0 and info['s_enc'] == w_info['s_enc']     # no sampler launch
    assert torch.equal(got, want) and _same_state(state, w_state) and info['tokens'] == w_info['tokens']


def test_generate_round2_loop_leaves_no_record(ctx, monkeypatch):
    from pianobart_amd import generation
    m, eng, enc, emask, pre, sampler, ref = ctx
    ref(1, 1007)                                   # a record is there before the call
    monkeypatch.setattr(generation, '_DECODE_GRAPH', -1)
    created = []
    monkeypatch.setattr(generation.GenerationMixin, '_decoder_create', staticmethod(lambda bp: created.append(bp)))
    saved = np.random.get_state()
    try:
        np.random.set_state(np.random.RandomState(1007).get_state())
        got = eng.generate(enc[1:2], emask[1:2], m.sample_row, sampler=sampler)
    finally:
        np.random.set_state(saved)
    assert eng.last_decode is None and not created          # no native decoder at this setting
    assert got.shape == (1, S, 8)


def test_generate_batch_record_three_prompts_one_primed(ctx):
    m, eng, enc, emask, pre, sampler, ref = ctx
    seeds, lens = [1000, 1007, 1014], [0, K_PRIMED, 0]
    prefix = pre[None].repeat(3, 1, 1)
    rngs = [np.random.RandomState(s) for s in seeds]
    got = eng.generate_batch(enc, emask, m.sample_row, rngs, sampler=sampler, prefix=prefix, prefix_len=lens).cpu()
    info = eng.last_decode
    _check_record(info, BATCHED, rows=3)
    assert info['batched'] is True and info['batch'] == 3 and info['prefix'] == lens and info['groups'] == [0, 1, 2]
    assert info['encoder_passes'] == 3 and info['prefill_passes'] == 1 and info['prefill_ms'] > 0 and info['setup_ms'] > 0
    assert info['cross_cache_bytes'] == 2 * 3 * S * 2 * 256 * 2 and info['graph'] is True and info['device_sampler'] is True
    rows = [(0, 1000, False), (1, 1007, True), (2, 1014, False)]
    _rows_match(ref, got, [r.get_state() for r in rngs], rows)
    assert info['tokens'] == [ref(*k)[2]['tokens'] for k in rows] and info['s_enc'] == [ref(*k)[2]['s_enc'] for k in rows]


def test_generate_batch_record_samples_per_prompt(ctx):
    m, eng, enc, emask, pre, sampler, ref = ctx
    seeds = [1000, 2000, 1007]
    rngs = [np.random.RandomState(s) for s in seeds]
    got = eng.generate_batch(enc[:2], emask[:2], m.sample_row, rngs, sampler=sampler, samples=[2, 1]).cpu()
    info = eng.last_decode
    _check_record(info, BATCHED, rows=3)
    assert info['batched'] is True and info['batch'] == 3 and info['prefix'] == [0, 0, 0] and info['groups'] == [0, 0, 1]
    assert info['encoder_passes'] == 2 and info['prefill_passes'] == 0 and info['prefill_ms'] == 0
    assert info['cross_cache_bytes'] == 2 * 2 * S * 2 * 256 * 2                # two slices for three rows
    rows = [(0, 1000, False), (0, 2000, False), (1, 1007, False)]
    _rows_match(ref, got, [r.get_state() for r in rngs], rows)
    assert info['tokens'] == [ref(*k)[2]['tokens'] for k in rows]


def test_per_prompt_loop_record(ctx):
    m, eng, enc, emask, pre, sampler, ref = ctx
    seeds = [1000, 1007, 1014]
    rngs = [np.random.RandomState(s) for s in seeds]
    before = np.random.get_state()
    got = eng.generate_batch(enc, emask, m.sample_row, rngs, sampler=None).cpu()
    assert eng.last_decode == dict(batched=False, batch=3) and type(eng.last_decode['batched']) is bool and type(eng.last_decode['batch']) is int
    assert _same_state(before, np.random.get_state())
    _rows_match(ref, got, [r.get_state() for r in rngs], [(0, 1000, False), (1, 1007, False), (2, 1014, False)])
