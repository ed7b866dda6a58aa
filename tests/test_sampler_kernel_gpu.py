"""GPU: dec_sample_kernel (csrc/pb_decode.hip), position by position, against the float64 nucleus rule of tests/sampler_ref.py.

The sampler's result is a prediction that the host replays and rewinds, so a defect in it changes no generated token; here every id it
writes is judged. The C ABI is driven directly (as tests/test_refill_generation_gpu.py does). The decoder reads plan.head_w / plan.head_b at run
time: head.w is zeroed once, so the LM-head GEMV gives 0 + bias and the logits row of every row of the batch IS head.b, bit for bit; between
two single-step launches the next row of the case tables is copied into head.b. The sampler's pinned logs (prefilled with NaN and -7) give the
row it read and the 8 ids it wrote per (row, position); the LOGGED row goes to the reference, and each row is followed on the tokens the device
itself wrote, so one wrong position is reported once.

Assertions, none with a tolerance: a decided (row, position, head) holds the reference's single id, an undecided one an acceptable id; no
crafted case is undecided and at most 5 % of a setting's random ones are (the caps of tests/test_sampler_ref_cpu.py, re-asserted on the
device's chain); a row the reference calls done at position i has untouched log rows from i + 1 on, however many further steps are launched,
a live row has none, and a position with all 8 heads given keeps its NaN logits row and holds the given ids.

Settings (tests/sampler_ref.py SETTINGS): eight planned ones and two more. 'no-prefix': p = 0.9999999 on heads 4 and 7, which no prefix exceeds.
'exact-cut': two tied classes over exact zeros, where f32 arithmetic is exact in any order (sampler_ref._exact_pair), with p ON the first
cumulative sum; it is the one case in which `> p` and `>= p` differ and the reference is still decided. Narrow and wide forms, graph replays
and direct launches, 16 rows with and without a force table, and the single-row form with one rule per run. ops.Layout accepts the 1088 head.

Measured: undecided (position, head) pairs, the reference's own chain on the CPU = the MI355X's chain (the device took the same ids):
  setting          crafted   random                  setting          crafted   random
  default          0 / 3192  1 / 2312 (0.04 %)       no-prefix        0 / 3432  2 / 2312 (0.09 %)
  ranked-01        0 / 2584  1 / 2112 (0.05 %)       edge-narrow      0 / 3136  0 / 2312
  all-1            0 / 3680  0 / 2504                edge-wide        0 / 2984  2 / 2304 (0.09 %)
  all-.9           0 / 2512  0 / 2112                edge-wide-1088   0 / 1968  8 / 1152 (0.69 %)
  cold             0 / 2472  0 / 1144                exact-cut        0 /  784  2 / 2432 (0.08 %)
  B = 1, default and edge-wide-1088: 0 / 504 crafted, 0 / 336 random each.
The unchanged kernel: 0 wrong ids in every setting. Heads skipped in tests/test_sampler_ref_cpu.py because two candidates had bit-equal host
probabilities: 0 (3910 heads equal, 2 undecided).

Scratch builds of csrc/pb_decode.hip with one token changed (never committed), wrong (row, position, head) or log findings over all settings:
  * the nucleus test `base + pre[k] > ph` made `>=`: 117, all 'pair' rows of exact-cut (heads 3, 4, 7 take the lower class where the draw
    asks for the upper one), none elsewhere: wherever else the two differ, a cumulative sum is within eps of p and the head is undecided.
  * the p = 1 butterfly's `oi < bi` made `oi > bi`: 7074 crafted (plateau 6724, flat 100, one-hot 206, ladder 44), in every setting with a
    p = 1 head and in both B = 1 runs; all-.9 has none (no such head).
  * the mask bit `col & 31` made `(col + 1) & 31`: 3174 crafted and 1317 random, rows 1, 13, 14, 15 (the masked ones) of every setting.
  * `K * lane + k < kc` made `<= kc`: 0, and no case can fail: every lane starts from best = kc - 1 and the butterfly takes the minimum, so a
    lane that offers kc changes nothing. The change is equivalent.
  * head 1's `lane + 64 * k < low1` made `<=`: 895 crafted and 66 random, head 1 of the time-ordered rows 2 .. 9 and 15 of every setting."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

from tests import sampler_ref as R
from tests.golden_util import load_vocab, randomize_params
from tests.vocab_layout_util import make_dict, synth_batch

pytestmark = pytest.mark.gpu
S = R.S
SENT = -7                                                          # the id log's prefill
_MODELS = {}


def _model(dname):
    """bf16, d = 256, 4 heads of 64, 2 layers, ffn 512, S = 64, with a zero LM-head weight; one prompt of 8 visible rows. Once per dictionary."""
    if dname not in _MODELS:
        if not torch.cuda.is_available():
            pytest.skip('no GPU')
        from pianobart_amd.model import BartConfig, PianoBart, PianoBartLM
        sizes = R.DICTS[dname]
        e2w, w2e = load_vocab() if dname == 'default' else make_dict(sizes)
        cfg = BartConfig(max_position_embeddings=S, d_model=256, encoder_layers=2, decoder_layers=2, encoder_ffn_dim=512, decoder_ffn_dim=512,
                         encoder_attention_heads=4, decoder_attention_heads=4)
        m = PianoBartLM(PianoBart(cfg, e2w, w2e, precision='bf16')).eval()
        randomize_params(m, 31)
        with torch.no_grad():
            for proj in m.mask_lm.proj:
                proj.weight.zero_()
        m = m.cuda()
        eng = m._get_engine()
        enc = synth_batch(sizes, 1, S, seed=8, min_len=S)[5].cuda()
        enc[:, 8:] = torch.tensor([n - 6 for n in sizes], device='cuda')
        emask = (enc[:, :, 0] != sizes[0] - 6).float()
        eng.bind(enc.device)
        assert list(eng.lay.sizes) == list(sizes)
        eng.w['head.w'].zero_()                                    # in place: the decoder's plan points at it
        _MODELS[dname] = (m, eng, enc, emask)
    return _MODELS[dname]


@contextlib.contextmanager
def _decoder(eng, enc, emask, n, use_graph):
    """A fused decoder of n rows, every row on the one prompt (tests/test_refill_generation_gpu.py::_decoder with the launch mode as an argument)."""
    from pianobart_amd import ops
    from pianobart_amd._lib import LIB
    em, enc16 = eng._prompt_inputs(enc, emask)
    s_enc = eng._key_extent(em[:1], S)
    assert s_enc == 8
    em_rows = em[:1].repeat(n, 1).contiguous()
    bp, bufs = eng._decode_plan(n, S, [s_enc] * n, em_rows, enc.device)
    dec = eng._decoder_create(bp)
    assert dec is not None
    try:
        _, enc_out = eng.forward_hidden(enc16[:1], None, em[:1], None, False, 0)
        for l in range(eng.ND):
            eng._linear(enc_out, 'dec.%d.wkv_c' % l, 'dec.%d.bkv_c' % l, bufs['kvc'][l][0], S, 2 * eng.d, eng.d)
            for g in range(1, n):
                bufs['kvc'][l][g].copy_(bufs['kvc'][l][0])
        LIB.call('pb_batch_decoder_reset', dec, ops._stream(), use_graph)
        torch.cuda.current_stream().synchronize()
        yield dec, bufs, em_rows
    finally:
        LIB.call('pb_batch_decoder_destroy', dec)


def _run(eng, enc, emask, c, rows, use_graph):
    """The case's positions (and R.EXTRA further steps) on the device for the given rows of the case; returns copies of the logs,
    (logits (n, S, vocab), tok (n, S, 8))."""
    from pianobart_amd._lib import LIB
    n, vocab, npos = len(rows), c['vocab'], len(c['kinds'])
    rules = [c['rules'][r] for r in rows]
    head_b = eng.wf['head.b']
    assert head_b.dtype == torch.float32 and head_b.numel() == vocab and not bool(eng.w['head.w'].any())
    bias = torch.from_numpy(c['logits']).cuda()
    with torch.no_grad(), _decoder(eng, enc, emask, n, use_graph) as (dec, _, _):
        U = np.ascontiguousarray(c['U'][rows].reshape(n, S * 8))
        n8, off8, pad8 = (np.ascontiguousarray(v, dtype=np.int32) for v in (c['sizes'], c['offs'][:8], c['pad']))
        LIB.call('pb_batch_decoder_sampler_init', dec, c['T'].ctypes.data, c['P'].ctypes.data, n8.ctypes.data, off8.ctypes.data, pad8.ctypes.data,
                 U.ctypes.data, n * S * 8, S, -1, 0)
        assert int(LIB.query('pb_batch_decoder_sampler_form', dec)) == (1 if c['form'] == 'wide' else 0)
        forced = np.ascontiguousarray(np.stack([r['given'] for r in rules]), dtype=np.int16)
        if (forced >= 0).any():
            LIB.call('pb_batch_decoder_force', dec, forced.ctypes.data)
        LIB.call('pb_batch_decoder_stop', dec, np.asarray([r['stop'] for r in rules], dtype=np.int32).ctypes.data)
        LIB.call('pb_batch_decoder_order', dec, np.asarray([r['floor'] for r in rules], dtype=np.int32).ctypes.data)
        masks = np.ascontiguousarray(c['masks'], dtype=np.uint32)
        LIB.call('pb_batch_decoder_allow', dec, masks.ctypes.data, masks.shape[0], masks.shape[1],
                 np.asarray([r['mask'] for r in rules], dtype=np.int32).ctypes.data)
        lp, tp = ctypes.c_void_p(), ctypes.c_void_p()
        LIB.call('pb_batch_decoder_logs', dec, ctypes.byref(lp), ctypes.byref(tp))
        logits = np.ctypeslib.as_array((ctypes.c_float * (n * S * vocab)).from_address(lp.value)).reshape(n, S, vocab)
        tok = np.ctypeslib.as_array((ctypes.c_int16 * (n * S * 8)).from_address(tp.value)).reshape(n, S, 8)
        logits[:] = np.nan
        tok[:] = SENT
        first = np.ascontiguousarray(np.tile(c['sos'].astype(np.int16), (n, 1)))
        last_pos, lim = np.full(n, -1, dtype=np.int32), np.full(n, S, dtype=np.int32)
        LIB.call('pb_batch_decoder_start', dec, last_pos.ctypes.data, first.ctypes.data, lim.ctypes.data)
        for i in range(npos + R.EXTRA):
            if i < npos:
                head_b.copy_(bias[i])
            torch.cuda.synchronize()
            tk = int(LIB.query('pb_batch_decoder_launch', dec, 1, None))
            assert tk >= 0, LIB.load().pb_last_error().decode()
            LIB.call('pb_batch_decoder_wait', dec, tk)
        assert bool(LIB.query('pb_batch_decoder_graph', dec)) == bool(use_graph)
        return logits.copy(), tok.copy()


def _bits(x):
    return (np.asarray(x, dtype=np.float32) + np.float32(0)).view(np.int32)      # -0 -> +0


def _judge(c, rows, logits, tok, rows_form):
    """Every (row, position, head) against the reference; returns (failures, crafted undecided, crafted, random undecided, random)."""
    npos = len(c['kinds'])
    fails = []
    cu = ct = ru = rt = 0
    for k, r in enumerate(rows):
        end = None
        sub = dict(c, rules=[c['rules'][r]], U=c['U'][r:r + 1])
        for i, sets, logged, done in R.follow(sub, 0, tok[k, :npos], rows_form, logits=logits[k]):
            if (tok[k, i] == SENT).all():
                fails.append((r, i, c['kinds'][i], 'no ids written: the row ended early'))
                end = i - 1
                break
            if logged:
                if not np.array_equal(_bits(logits[k, i]), _bits(c['logits'][i])):
                    fails.append((r, i, c['kinds'][i], 'the logged row is not the bias row'))
                    end = i
                    break
            elif not np.isnan(logits[k, i]).all():
                fails.append((r, i, c['kinds'][i], 'a position with all 8 heads given logged a logits row'))
            for h in range(8):
                got, und = int(tok[k, i, h]), len(sets[h]) > 1
                if got not in sets[h]:
                    fails.append((r, i, c['kinds'][i], 'head %d: %d, acceptable %s' % (h, got, sorted(sets[h])[:6])))
                if c['kinds'][i] == 'random':
                    ru, rt = ru + und, rt + 1
                else:
                    cu, ct = cu + und, ct + 1
            if done and rows_form:
                end = i
                break
        last = end if end is not None else npos + R.EXTRA - 1     # a live row decodes the further steps too
        if end is None and not (tok[k, :last + 1] != SENT).all():
            fails.append((r, last, '', 'a live row has untouched id log rows'))
        if not ((tok[k, last + 1:] == SENT).all() and np.isnan(logits[k, last + 1:]).all()):
            fails.append((r, last, c['kinds'][min(last, npos - 1)], 'log rows were written behind the position that ended the row'))
    return fails, cu, ct, ru, rt


@pytest.mark.parametrize('name', list(R.SETTINGS))
def test_sampler_ids_against_float64(name):
    c = R.case(name)
    m, eng, enc, emask = _model(R.SETTINGS[name][0])
    rows = list(range(R.B))
    logits, tok = _run(eng, enc, emask, c, rows, c['use_graph'])
    fails, cu, ct, ru, rt = _judge(c, rows, logits, tok, True)
    print('sampler kernel %-15s %s, %s: crafted %d of %d undecided, random %d of %d (%.2f %%); %d wrong' %
          (name, c['form'], 'graph' if c['use_graph'] else 'direct', cu, ct, ru, rt, 100.0 * ru / max(rt, 1), len(fails)))
    assert not fails, (len(fails), fails[:12])
    assert cu == 0 and ru <= .05 * rt and (ct > 1000 or name == 'exact-cut') and rt > 1000
    if name in ('default', 'edge-wide'):                           # the rows without given ids, alone: no force table, the unforced kernels of both forms
        free = [r for r in rows if not (c['rules'][r]['given'] >= 0).any()]
        assert len(free) >= 10
        logits, tok = _run(eng, enc, emask, c, free, 1 - c['use_graph'])
        fails, cu, ct, ru, rt = _judge(c, free, logits, tok, True)
        print('sampler kernel %-15s unforced: crafted %d of %d undecided, random %d of %d; %d wrong' % (name, cu, ct, ru, rt, len(fails)))
        assert not fails, (len(fails), fails[:12])
        assert cu == 0 and ru <= .05 * rt


@pytest.mark.parametrize('name,use_graph', [('default', 0), ('edge-wide-1088', 1)])
def test_single_row_form_against_float64(name, use_graph):
    """B = 1 (the kernels without a done flag; the host stays inside the limit): each rule once, a run of its own."""
    c = R.case(name, b1=True)
    m, eng, enc, emask = _model(R.SETTINGS[name][0])
    fails, und, tot = [], 0, 0
    for r in range(len(c['rules'])):
        logits, tok = _run(eng, enc, emask, c, [r], use_graph)
        f, cu, ct, ru, rt = _judge(c, [r], logits, tok, False)
        fails += f
        und, tot = und + ru, tot + rt
        assert cu == 0 and ct > 0
    print('sampler kernel %-15s B = 1, %s: random %d of %d undecided; %d wrong' % (name, c['form'], und, tot, len(fails)))
    assert not fails, (len(fails), fails[:12])
    assert und <= .05 * tot
