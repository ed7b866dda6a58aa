"""Gradient accumulation on the GPU: pb_accum_f32, Engine.loss_and_grads(micro=(i, K)), Engine.mask_counts, Pretrainer --accum_steps.

Model: d = 256, 2 + 2 layers, 4 heads, ffn 512 (the _lm shapes of tests/test_score_gpu.py), dropout 0, B = 4. The sequences are 32 .. 64
rows long in a window of S = 128: the B = 4 batch of the bf16 engine (512 rows, fewer than 256 alive) is one the packed step takes, while
its micro-batches of 2 and 1 rows have nothing to gain from packing and run dense -- accumulation has to agree across the two schedules.

Bounds and where they come from:
  * kernel: exact. One f32 addition per element, correctly rounded, as torch's.
  * K = 1 and "the same micro-batch twice": bit-identical wherever the step itself is. Two plain steps on the same batch are compared
    first, slot by slot of the flat gradient buffer. A slot they agree on bit for bit must come out bit-identical from the accumulated
    step. A slot they do not agree on (f32 atomics of the exact-f32 embedding path, whose order of summation changes from run to run)
    is compared against that run-to-run spread instead: the accumulated step is two more draws of the same noise, each halved, so its
    distance from run A is a sum of three such terms and is bounded here by 4x the spread measured between runs A and B; the test
    prints which slots took that route.
  * split batch, fp32: max|dG| / max|G| <= 1e-5, the bound of tests/test_parallel_cpu.py for the same comparison (half-batches under
    the global counts against the global batch). Teeth: the halves under their OWN counts, averaged, must miss it by 100x.
  * split batch, bf16: at most 2x the distance between the bf16 and the fp32 one-batch gradients of the same weights, measured in the
    same test: f32 accumulation must not add more than bf16's own rounding.

Measured on an MI355X (max|dG| / max|G|): split 2 + 2 and 2 + 1 + 1 fp32 2.3e-7; own counts averaged 5.8e-1; bf16 split 6.7e-5 with bf16 2.2e-2
from fp32; fp32 "twice": 69 of 73 slots bit-identical, emb / lin.w / enc.pos / dec.pos (f32 atomics) within their run-to-run spread."""
import numpy as np
import pytest
import torch

from tests.golden_util import synth_octuple_batch

gpu = pytest.mark.gpu
B, S = 4, 128
_CACHE = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


def _engine(precision):
    if precision not in _CACHE:
        from tests.test_generate_batch_gpu import _lm
        m = _lm(S, 256, 2, 512, 4, 51, precision)             # same seed: the same weights in every precision
        eng = m._get_engine()
        eng.bind(torch.device('cuda', 0))
        _CACHE[precision] = (m, eng)
    return _CACHE[precision][1]


def _batch():
    """(enc16, dec16, tgt16, loss_mask, emask, dmask) on the device; rows 0 - 1 carry 12 loss positions, rows 2 - 3 about 40."""
    if 'batch' not in _CACHE:
        from pianobart_amd import ops
        from tests.golden_util import PAD
        enc, _, lm, _, _, tgt = synth_octuple_batch(B, S // 2, seed=3)
        tail = torch.from_numpy(PAD).expand(B, S - S // 2, 8)
        enc, tgt = torch.cat([enc, tail], 1), torch.cat([tgt, tail], 1)
        lm = torch.cat([lm, torch.zeros(B, S - S // 2, 8)], 1)
        dec = torch.empty_like(tgt)
        dec[:, 1:] = tgt[:, :-1]
        dec[:, 0] = torch.from_numpy(PAD + 2)                 # SOS row
        em, dm = (enc[:, :, 0] != 256).float(), (dec[:, :, 0] != 256).float()
        lm[0] = 0; lm[0, :9] = 1                              # the trick of tests/test_parallel_cpu.py, sharpened: very different counts per half
        lm[1] = 0; lm[1, :3] = 1
        lm[2, :S // 4] = 1                                    # every sequence has at least S / 4 visible positions
        c = lm.reshape(B, -1, 8).sum(1)[:, 0]
        assert float(c[0] + c[1]) == 12 and float(c[2] + c[3]) >= 32
        _CACHE['batch'] = tuple(t.cuda().contiguous() for t in (ops.ids_to_i16(enc.cuda()), ops.ids_to_i16(dec.cuda()), ops.ids_to_i16(tgt.cuda()), lm, em, dm))
    return _CACHE['batch']


def _rows(batch, lo, hi):
    return tuple(t[lo:hi].contiguous() for t in batch)


def _grads(eng, batch, **kw):
    """One loss_and_grads; returns (copy of G32, copy of the 24 sums)."""
    sums = eng.loss_and_grads(*batch, train=True, **kw)
    return eng.G32.clone(), sums.clone()


def _total_counts(eng, parts):
    from pianobart_amd import ops
    total = eng.mask_counts(parts[0][3])
    for p in parts[1:]:
        ops.accum_f32(total, eng.mask_counts(p[3]), add=True)
    return total


def _accumulated(eng, parts, total=None):
    """An optimizer step's worth of micro-batches; returns (G32, [sums of each])."""
    if total is None:
        total = _total_counts(eng, parts)
    hook = lambda c: c.copy_(total)
    sums = []
    for i, p in enumerate(parts):
        sums.append(eng.loss_and_grads(*p, train=True, count_hook=hook, micro=(i, len(parts))).clone())
    return eng.G32.clone(), sums


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def _bitwise_where_the_step_is(eng, Ga, Gb, Gx, what):
    """Ga, Gb: two plain runs; Gx: the run under test. Slot by slot: bit-identical where Ga and Gb are, within 4x their spread elsewhere."""
    noisy = []
    for name, s in eng.slots.items():
        a, b, x = (g[s.off:s.off + s.numel] for g in (Ga, Gb, Gx))
        if torch.equal(a, b):
            assert torch.equal(a, x), '%s: slot %s differs from the plain step (max |d| %.3e)' % (what, name, float((a - x).abs().max()))
        else:
            spread, d = float((a - b).abs().max()), float((a - x).abs().max())
            noisy.append((name, spread, d))
            assert d <= 4 * spread, '%s: slot %s is %.3e from the plain step, run-to-run spread %.3e' % (what, name, d, spread)
    print('%s: %d of %d slots bit-identical to the plain step; compared against the run-to-run spread instead (slot, spread, distance): %s'
          % (what, len(eng.slots) - len(noisy), len(eng.slots), noisy))
    return noisy


# ---------------------------------------------------------------------------------------------------- 1. kernel
@gpu
@pytest.mark.parametrize('add', [False, True])
def test_accum_kernel_is_exact_and_stays_inside_its_range(add):
    _need_gpu()
    from pianobart_amd import ops
    g = torch.Generator().manual_seed(7)
    for n in (1, 3, 4, 5, 1023, 4101):
        for start in range(4):
            for src_start in {start, 0}:                       # the engine's case (both offset alike) and pointers offset differently
                pad = 8
                dst0 = (torch.randn(start + n + 2 * pad, generator=g) * 3).cuda()
                src0 = (torch.randn(src_start + n + 2 * pad, generator=g) * 3).cuda()
                dst, src = dst0.clone(), src0.clone()
                lo, slo = pad + start, pad + src_start
                want = dst0.clone()
                want[lo:lo + n] = (dst0[lo:lo + n] + src0[slo:slo + n]) if add else src0[slo:slo + n]
                ops.accum_f32(dst[lo:lo + n], src[slo:slo + n], add=add)
                assert torch.equal(dst, want), (n, start, src_start, add)          # the range bit for bit, the canaries around it untouched
                assert torch.equal(src, src0)
    dst, src = torch.ones(16, device='cuda'), torch.full((16,), 2.0, device='cuda')
    ops.accum_f32(dst[4:4], src[4:4], add=add)                                     # n = 0
    assert torch.equal(dst, torch.ones(16, device='cuda'))
    big = 2048 * 256 * 4 * 2 + 7                                                    # more elements than one pass of the capped grid covers
    a, b = torch.randn(big, generator=g).cuda(), torch.randn(big, generator=g).cuda()
    want = a + b if add else b.clone()
    ops.accum_f32(a, b, add=add)
    assert torch.equal(a, want)


# ---------------------------------------------------------------------------------------------------- 2. K = 1 is today's step
@gpu
def test_micro_0_of_1_is_the_plain_step():
    _need_gpu()
    eng, batch = _engine('bf16'), _batch()
    Ga, sa = _grads(eng, batch)
    assert eng.last_rows[0] < B * S                             # the packed step took the batch
    Gb, sb = _grads(eng, batch)
    Gx, sx = _grads(eng, batch, micro=(0, 1))
    assert torch.equal(sa, sb) and torch.equal(sa, sx)
    _bitwise_where_the_step_is(eng, Ga, Gb, Gx, 'micro=(0, 1), bf16')
    assert eng.G_acc is None


# ---------------------------------------------------------------------------------------------------- 3. the same micro-batch twice
@gpu
def test_same_micro_batch_twice_is_the_single_step_fp32():
    _need_gpu()
    from pianobart_amd import ops
    eng, batch = _engine('fp32'), _batch()
    P0 = eng.P32.clone()

    def restore():
        eng.P32.copy_(P0)
        eng.opt_m = eng.opt_v = None
        eng.step_count = 0
        eng.refresh_shadow(force=True)

    try:
        Ga, sa = _grads(eng, batch)
        eng.optimizer_step(lr=1e-3)
        Pa = eng.P32.clone()
        restore()
        Gb, sb = _grads(eng, batch)
        eng.optimizer_step(lr=1e-3)
        Pb = eng.P32.clone()
        restore()
        assert torch.equal(sa, sb)
        total = _total_counts(eng, [batch, batch])              # doubled counts: coef is halved exactly, and g / 2 + g / 2 = g
        assert torch.equal(total, 2 * eng.mask_counts(batch[3]))
        Gx, sums = _accumulated(eng, [batch, batch], total)
        assert eng.G_acc is not None and eng.G_acc.shape == eng.G32.shape and eng.G_acc.dtype == torch.float32
        both = sums[0].clone()
        ops.accum_f32(both, sums[1], add=True)
        assert torch.equal(both, 2 * sa)
        noisy = _bitwise_where_the_step_is(eng, Ga, Gb, Gx, 'same micro-batch twice, fp32')
        assert eng.step_count == 0
        eng.optimizer_step(lr=1e-3)
        assert eng.step_count == 1
        Px = eng.P32.clone()
        if not noisy and torch.equal(Pa, Pb):
            assert torch.equal(Px, Pa)
        else:
            spread, d = float((Pa - Pb).abs().max()), float((Pa - Px).abs().max())
            print('parameters after the step: run-to-run spread %.3e, accumulated step %.3e from run A' % (spread, d))
            assert d <= 4 * spread
        assert not torch.equal(Px, P0)
    finally:
        restore()


# ---------------------------------------------------------------------------------------------------- 4. split batch, fp32
def _one_batch(precision):
    key = 'one_' + precision
    if key not in _CACHE:
        _CACHE[key] = _grads(_engine(precision), _batch())
    return _CACHE[key]


@gpu
@pytest.mark.parametrize('cuts', [(0, 2, 4), (0, 2, 3, 4)], ids=['2+2', '2+1+1'])
def test_split_batch_matches_the_one_batch_step_fp32(cuts):
    """Measured on an MI355X: 2.3e-7 for 2 + 2 rows and for 2 + 1 + 1 rows against the B = 4 step (bound 1e-5); teeth 5.8e-1."""
    _need_gpu()
    eng, batch = _engine('fp32'), _batch()
    G, s = _one_batch('fp32')
    parts = [_rows(batch, a, b) for a, b in zip(cuts[:-1], cuts[1:])]
    Gx, sums = _accumulated(eng, parts)
    err = _rel(Gx, G)
    tot = torch.stack(sums).double().sum(0)
    print('split %s fp32: max|dG| / max|G| = %.3e; sums rel %.3e' % (cuts, err, _rel(tot, s)))
    assert err < 1e-5
    assert torch.equal(tot[8:24], s[8:24].double())             # counts and hits are integers
    assert _rel(tot[0:8], s[0:8]) < 1e-5
    if len(cuts) == 3:
        # teeth: each half normalised by its OWN counts, the two gradients averaged -- what accumulation without the global counts would give
        g0, _ = _grads(eng, parts[0])
        g1, _ = _grads(eng, parts[1])
        miss = _rel((g0 + g1) / 2, G)
        print('halves under their own counts, averaged: max|dG| / max|G| = %.3e' % miss)
        assert miss >= 100 * 1e-5


# ---------------------------------------------------------------------------------------------------- 5. bf16
@gpu
def test_split_batch_bf16_adds_no_more_than_bf16_rounding():
    _need_gpu()
    eng, batch = _engine('bf16'), _batch()
    G16, _ = _one_batch('bf16')
    G32, _ = _one_batch('fp32')
    own = _rel(G16, G32)
    for cuts in ((0, 2, 4), (0, 2, 3, 4)):
        Gx, _ = _accumulated(eng, [_rows(batch, a, b) for a, b in zip(cuts[:-1], cuts[1:])])
        err = _rel(Gx, G16)
        print('split %s bf16: %.3e from the bf16 one-batch step; bf16 one-batch is %.3e from fp32' % (cuts, err, own))
        assert err <= 2 * own


# ---------------------------------------------------------------------------------------------------- 6. hook
@gpu
def test_grad_hook_runs_once_per_step_on_summed_ranges():
    _need_gpu()
    eng, batch = _engine('bf16'), _batch()
    parts = [_rows(batch, 0, 2), _rows(batch, 2, 4)]
    total = _total_counts(eng, parts)
    seen = []
    eng.grad_hook = lambda lo, hi: seen.append((lo, hi, eng.G32[lo:hi].clone()))      # a snapshot on the issuing stream
    try:
        eng.loss_and_grads(*parts[1], train=True)                                      # K = 1
        plain = [(lo, hi) for lo, hi, _ in seen]
        seen.clear()
        hook = lambda c: c.copy_(total)
        ga, _ = _grads(eng, parts[0], count_hook=hook)
        ga2, _ = _grads(eng, parts[0], count_hook=hook)
        gb, _ = _grads(eng, parts[1], count_hook=hook)
        seen.clear()
        eng.loss_and_grads(*parts[0], train=True, count_hook=hook, micro=(0, 2))
        assert seen == []
        eng.loss_and_grads(*parts[1], train=True, count_hook=hook, micro=(1, 2))
        torch.cuda.synchronize()
        G = eng.G32.clone()
    finally:
        eng.grad_hook = None
    assert [(lo, hi) for lo, hi, _ in seen] == plain
    cover = np.zeros(eng.n_total, dtype=np.int64)
    for lo, hi, _ in seen:
        cover[lo:hi] += 1
    assert (cover == 1).all()                                                          # [0, n_total), each element once
    for lo, hi, snap in seen:
        assert torch.equal(snap, G[lo:hi]), (lo, hi)                                   # the range was already summed when the hook saw it
    # and what it saw is the sum of the two micro-gradients: one f32 addition per element, so bit for bit when the step itself is reproducible
    d, spread = float((G - (ga + gb)).abs().max()), float((ga - ga2).abs().max())
    print('hooked accumulated step against the sum of its two micro-gradients: max |d| %.3e (run-to-run spread of one micro-gradient %.3e)' % (d, spread))
    assert d <= 4 * spread


# ---------------------------------------------------------------------------------------------------- 7. trainer
@gpu
def test_pretrainer_accum_steps(capsys):
    _need_gpu()
    from pianobart_amd.model import BartConfig, PianoBart
    from pianobart_amd.pretrain import Pretrainer, get_args_pretrain
    from tests.golden_util import load_vocab, randomize_params
    e2w, w2e = load_vocab()
    S = 64
    kw = dict(max_position_embeddings=S, d_model=256, encoder_layers=2, decoder_layers=2, encoder_ffn_dim=512, decoder_ffn_dim=512,
              encoder_attention_heads=4, decoder_attention_heads=4, dropout=0.0)
    tr = Pretrainer(PianoBart(BartConfig(**kw), e2w, w2e), None, None, 1e-3, B, S, 0.15, False, [0])
    randomize_params(tr.model, 5)
    tr.engine.bind(tr.device)
    tr.engine.refresh_shadow(force=True)
    loader = [synth_octuple_batch(B, S, seed=20 + i)[5] for i in range(5)]
    for flag, steps in (('2', 3), ('1', 5)):
        tr.accum_steps = get_args_pretrain(['--accum_steps', flag]).accum_steps
        before, P0 = tr.engine.step_count, tr.engine.P32.clone()
        capsys.readouterr()
        loss, accs = tr.iteration(loader, S)
        torch.cuda.synchronize()
        out = capsys.readouterr().out.splitlines()
        loss_lines = [l for l in out if l.startswith('Loss:')]
        assert tr.engine.step_count - before == steps
        assert len(loss_lines) == steps and len([l for l in out if l.startswith('Acc:')]) == steps
        vals = [float(x) for l in loss_lines for x in l.replace('Loss:', '').replace('| loss:', ',').split(',')]
        assert len(vals) == 9 * steps and np.isfinite(vals).all() and min(vals) > 0
        assert np.isfinite(loss) and len(accs) == 8
        tr.engine.finish_updates()
        assert not torch.equal(tr.engine.P32, P0) and bool(torch.isfinite(tr.engine.P32).all())
    tr.accum_steps = 2
    before = tr.engine.step_count
    tr.iteration(loader, S, train=False)                                               # validation ignores the flag and takes no step
    assert tr.engine.step_count == before
    assert len([l for l in capsys.readouterr().out.splitlines() if l.startswith('Loss:')]) == 5
