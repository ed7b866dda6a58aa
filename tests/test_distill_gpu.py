"""GPU: distillation through the engine (Engine.loss_and_grads(distill=..., smooth=...), Engine.teacher_logits).

Models as small as tests/test_packed_gpu.py uses: the student has d = 256, 2 + 2 layers, 4 heads, S = 256, B = 6 with ragged PAD tails and
sparse loss rows; the teacher is another size (d = 128, 1 + 1 layers, 2 heads). What is held to what:
  * wiring: after one distilled step the student's and the teacher's logits are read out of their workspaces and the float64 restatement
    (tests/distill_ref.py) is evaluated on them with the student's own row map; the engine's dlogits buffer and its five sums must meet the
    bounds of tests/test_distill_kernels_gpu.py (4 x the float32 restatement's error);
  * row map: the same bf16 step packed and dense, tolerances of tests/test_packed_gpu.py (rtol 1e-3 on the sums, 2e-2 relative per
    gradient slot: the project's measured bf16 figures for packed against dense). A wrong teacher row is a KL wrong by orders of magnitude;
  * self-distillation (fp32, no dropout, dense, teacher = a copy of the student, alpha 0.5, tau 1): the KL plane is exactly 0 and every
    gradient slot is 0.5 x the plain step's to 1e-6 relative in norm: both forwards run the same kernels on the same shapes, the soft
    term is exactly 0, halving is exact, at most two roundings of 2^-24 per dlogit are left;
  * accumulation: K = 2 micro-batches against the one-batch step, fp32, the comparison and the bounds of tests/test_grad_accum_gpu.py
    (max|dG| / max|G| < 1e-5, loss sums 1e-5 relative, counts equal);
  * direction: 30 optimizer steps at alpha = 1 against a fixed random teacher lower the KL (no threshold);
  * every refusal by name, and the plain call leaves last_distill_sums unset.

Measured on an MI355X: wiring ratios (bound 4) loss 1.43, hard 1.53, kl 1.27, dlogits 0.007 (bf16 storage); packed against dense: sums 4e-4
relative, KL sums 77 .. 112 per head on both sides, worst gradient slot dec.pos 6.1e-3; self-distillation: KL exactly 0, worst slot emb 2.0e-7;
accumulation 3 + 3: max|dG| / max|G| 3.5e-7, sums 6.3e-8; 30 steps: KL sum 770.6 -> 182.3.
"""
import numpy as np
import pytest
import torch

from tests import distill_ref as DR
from tests.golden_util import load_vocab, randomize_params, synth_octuple_batch

pytestmark = pytest.mark.gpu
B, S = 6, 256
_CACHE = {}


class Plan:
    def __init__(self, teacher, alpha, tau):
        self.teacher, self.alpha, self.tau = teacher, alpha, tau


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from pianobart_amd import ops as o
    return o


def _model(d, layers, heads, precision, seed, dropout=0.0, window=S, vocab=None, lm=True, cuda=True):
    from pianobart_amd.model import BartConfig, PianoBart, PianoBartLM
    e2w, w2e = vocab if vocab is not None else load_vocab()
    cfg = BartConfig(max_position_embeddings=window, d_model=d, encoder_layers=layers, decoder_layers=layers, encoder_ffn_dim=2 * d,
                     decoder_ffn_dim=2 * d, encoder_attention_heads=heads, decoder_attention_heads=heads, dropout=dropout)
    pb = PianoBart(cfg, e2w, w2e, precision=precision)
    m = PianoBartLM(pb) if lm else pb
    randomize_params(m, seed)
    m.train()
    if cuda:
        m = m.cuda()
    eng = m._get_engine()
    if cuda:
        eng.bind(torch.device('cuda', 0))
    return m, eng


def _engine(key, *args, **kw):
    if key not in _CACHE:
        _CACHE[key] = _model(*args, **kw)
    return _CACHE[key][1]


def _student(precision, dropout=0.0):
    return _engine(('student', precision, dropout), 256, 2, 4, precision, 11, dropout)


def _teacher(precision):
    eng = _engine(('teacher', precision), 128, 1, 2, precision, 23)
    eng.pb.eval()
    return eng


def _batch(ops):
    """(enc16, dec16, tgt16, loss_mask, emask, dmask): ragged PAD tails on both sides, sparse loss rows in head 0, loss terms on a few rows
    that are not visible as keys (tests/test_packed_gpu.py)."""
    if 'batch' not in _CACHE:
        enc, dec, loss_mask, emask, dmask, target = [t.cuda() for t in synth_octuple_batch(B, S, seed=9)]
        rng = np.random.default_rng(3)
        Le, Ld = rng.integers(40, S + 1, size=B), rng.integers(40, S + 1, size=B)
        Le[0], Ld[1] = S, S
        emask, dmask, loss_mask = emask.clone().float(), dmask.clone().float(), loss_mask.clone().float()
        for b in range(B):
            emask[b, :Le[b]] = 1; emask[b, Le[b]:] = 0
            dmask[b, :Ld[b]] = 1; dmask[b, Ld[b]:] = 0
            loss_mask[b, Ld[b]:] = 0
            loss_mask[b, :Ld[b], 0] = torch.tensor((rng.random(Ld[b]) < 0.15).astype(np.float32), device='cuda')
            loss_mask[b, 1, 0] = 1
            if Ld[b] + 5 < S:
                loss_mask[b, Ld[b] + 2, :] = 1
                loss_mask[b, S - 1, 2] = 1
        _CACHE['batch'] = (ops.ids_to_i16(enc), ops.ids_to_i16(dec), ops.ids_to_i16(target), loss_mask.contiguous(), emask, dmask)
    return _CACHE['batch']


def _step(eng, args, pack, monkeypatch, seed=77, train=True, **kw):
    """tests/test_packed_gpu.py's _step with the new arguments: returns (24 sums, 16 distill sums or None, G32, last_rows)."""
    from pianobart_amd import engine as E
    monkeypatch.setattr(E, '_PACK_ROWS', 1 if pack else 0)
    monkeypatch.setattr(E, '_ATTN_BWD1', 0)
    eng._seed = seed
    sums = eng.loss_and_grads(*args, train=train, **kw).clone()
    extra = eng.last_distill_sums.clone() if eng.last_distill_sums is not None else None
    torch.cuda.synchronize()
    return sums, extra, eng.G32.clone(), eng.last_rows


def _slot_errors(eng, want, got):
    worst = ('', 0.0)
    for name, sl in eng.slots.items():
        a, b_ = want[sl.off:sl.off + sl.numel], got[sl.off:sl.off + sl.numel]
        worst = max(worst, (name, float((a - b_).norm()) / (float(a.norm()) + 1e-12)), key=lambda t: t[1])
    return worst


# ---------------------------------------------------------------- wiring
@pytest.mark.parametrize('pack', [True, False])
def test_engine_hands_the_kernel_the_right_rows(ops, monkeypatch, pack):
    from tests.test_distill_kernels_gpu import _bound, _col_err, _row_err
    eng, tch, args = _student('bf16', 0.1), _teacher('bf16'), _batch(ops)
    alpha, tau, eps = 0.5, 2.0, 0.1
    sums, extra, _, rows = _step(eng, args, pack, monkeypatch, distill=Plan(tch, alpha, tau), smooth=eps)
    n = rows[3]
    assert (n < rows[1] < B * S) if pack else n == B * S
    pk = eng._saved['pack']
    ws, tws = eng._cur_ws, tch._cur_ws
    z, u = ws['logits'][:n].clone(), tws['logits'].clone()
    assert u.shape == (B * S, eng.lay.vocab) and bool(torch.isfinite(u).all())
    if pack:
        t_row = (pk.sub.src if pk.sub is not None else pk.src_d)[:n].long()
        tgt, lm = (pk.sub.tgt16, pk.sub.loss_mask) if pk.sub is not None else (pk.tgt16, pk.loss_mask)
        assert pk.sub is not None
        # the map is the student's own: its packed targets are the batch's targets at those rows
        assert torch.equal(tgt[:n], args[2].reshape(-1, 8)[t_row]) and torch.equal(lm[:n], args[3].reshape(-1, 8)[t_row])
    else:
        t_row, tgt, lm = torch.arange(n, device='cuda'), args[2].reshape(-1, 8), args[3].reshape(-1, 8)
    tgt, lm, coef = tgt[:n].long(), lm[:n], eng.scal[32:40].clone()
    off = list(eng.lay.seg_off)
    r64 = DR.distill_fwd_bwd(z.double(), u.double(), tgt, lm.double(), off, coef.double(), alpha, tau, eps, t_row=t_row)
    r32 = DR.distill_fwd_bwd(z, u, tgt, lm, off, coef, alpha, tau, eps, t_row=t_row)
    got = torch.cat([sums, extra]).reshape(5, 8)
    zero = torch.zeros(8, device='cuda', dtype=torch.float64)
    assert torch.equal(got[1:3].double(), r64['terms'][1:3].sum(1))
    tag = 'engine %s' % ('packed' if pack else 'dense')
    for plane, name, mags in ((0, 'loss', None), (3, 'hard', None), (4, 'kl', r64['kl_abs'])):
        _bound('%s %s' % (tag, name), _col_err(got[plane], zero, r64['terms'][plane], mags), _col_err(r32['terms'][plane].sum(0), zero, r64['terms'][plane], mags))
    dl = ws['dlogits'][:n]
    assert dl.dtype == torch.bfloat16 and bool(torch.isfinite(dl).all())
    sizes = eng.lay.sizes
    sc = torch.cat([r64['gscale'][:, i:i + 1].expand(n, sizes[i]) for i in range(8)], 1)
    on = sc > 0
    assert bool((dl[~on] == 0).all())
    _bound(tag + ' dlogits', _row_err(dl[on], r64['dlogits'][on], sc[on], True), _row_err(r32['dlogits'][on], r64['dlogits'][on], sc[on], False))
    # the teacher was not trained on: no gradient buffer of it was touched
    assert float(tch.G32.abs().max()) == 0.0


# ---------------------------------------------------------------- row map
@pytest.mark.parametrize('dropout', [0.0, 0.1])
def test_packed_distilled_step_equals_dense_distilled_step(ops, monkeypatch, dropout):
    eng, tch, args = _student('bf16', dropout), _teacher('bf16'), _batch(ops)
    plan = Plan(tch, 0.5, 2.0)
    s0, x0, g0, r0 = _step(eng, args, False, monkeypatch, distill=plan, smooth=0.1)
    s1, x1, g1, r1 = _step(eng, args, True, monkeypatch, distill=plan, smooth=0.1)
    assert r0 == (B * S,) * 4 and r1[0] < B * S and r1[1] < B * S and r1[0] % 256 == 0 and r1[1] % 256 == 0, (r0, r1)
    assert r1[3] < r1[1] and r1[3] % 256 == 0, r1                      # sparse loss rows: the loss-row subset shrinks too
    assert torch.equal(s0[8:16], s1[8:16])
    print('packed vs dense distilled: loss', (s0[:8] - s1[:8]).abs().max().item(), 'hard / kl', (x0 - x1).abs().max().item(), 'kl sums', x0[8:].tolist())
    assert torch.allclose(s0[:8], s1[:8], rtol=1e-3) and torch.allclose(x0, x1, rtol=1e-3)
    assert float(x0[8:].min()) > 0
    assert float((s0[16:] - s1[16:]).abs().max()) <= 2                  # argmax hits: a near tie may flip
    assert torch.isfinite(g1).all()
    worst = _slot_errors(eng, g0, g1)
    print('packed vs dense distilled: worst gradient slot', worst)
    assert worst[1] < 2e-2, worst
    # evaluation: the five planes, no gradient
    before = eng.G32.clone()
    e0, y0, _, _ = _step(eng, args, False, monkeypatch, train=False, distill=plan, smooth=0.1)
    e1, y1, ge, _ = _step(eng, args, True, monkeypatch, train=False, distill=plan, smooth=0.1)
    assert torch.allclose(e0[:16], e1[:16], rtol=1e-3) and torch.allclose(y0, y1, rtol=1e-3) and torch.equal(ge, before)
    if dropout == 0.0:
        assert torch.allclose(e0[:8], s0[:8], rtol=1e-3)


# ---------------------------------------------------------------- self-distillation
def test_self_distillation_halves_the_plain_gradient(ops, monkeypatch):
    eng, args = _student('fp32'), _batch(ops)
    twin = _engine(('twin', 'fp32'), 256, 2, 4, 'fp32', 11)           # the same seed: a copy of the student with a workspace of its own
    assert torch.equal(twin.P32, eng.P32)
    sp, xp, gp, _ = _step(eng, args, False, monkeypatch)
    assert xp is None
    sd, xd, gd, _ = _step(eng, args, False, monkeypatch, distill=Plan(twin, 0.5, 1.0))
    assert bool((xd[8:16] == 0).all()), xd[8:16]                       # KL(student || student): exactly 0
    assert torch.allclose(xd[0:8], sp[0:8], rtol=1e-5) and torch.allclose(sd[0:8], 0.5 * sp[0:8], rtol=1e-5) and torch.equal(sd[8:], sp[8:])
    worst = _slot_errors(eng, 0.5 * gp, gd)
    print('self-distillation: worst gradient slot against half the plain step', worst)
    assert worst[1] <= 1e-6, worst


# ---------------------------------------------------------------- accumulation
def test_two_micro_batches_match_the_one_batch_distilled_step(ops, monkeypatch):
    from pianobart_amd import engine as E
    monkeypatch.setattr(E, '_PACK_ROWS', 0)
    eng, tch, args = _student('fp32'), _teacher('fp32'), _batch(ops)
    plan = Plan(tch, 0.5, 2.0)
    s = eng.loss_and_grads(*args, train=True, distill=plan, smooth=0.1).clone()
    x, G = eng.last_distill_sums.clone(), eng.G32.clone()
    parts = [tuple(t[a:b].contiguous() for t in args) for a, b in ((0, 3), (3, 6))]
    total = eng.mask_counts(parts[0][3])
    ops.accum_f32(total, eng.mask_counts(parts[1][3]), add=True)
    tot_s, tot_x = torch.zeros(24, device='cuda', dtype=torch.float64), torch.zeros(16, device='cuda', dtype=torch.float64)
    for i, p in enumerate(parts):
        tot_s += eng.loss_and_grads(*p, train=True, count_hook=lambda c: c.copy_(total), micro=(i, 2), distill=plan, smooth=0.1).double()
        tot_x += eng.last_distill_sums.double()
    rel = lambda a, b: float((a.double() - b.double()).abs().max() / b.double().abs().max())
    err = rel(eng.G32, G)
    print('distilled 3 + 3 fp32: max|dG| / max|G| = %.3e; sums rel %.3e, hard / kl rel %.3e' % (err, rel(tot_s[:8], s[:8]), rel(tot_x, x)))
    assert err < 1e-5
    assert torch.equal(tot_s[8:24], s[8:24].double())
    assert rel(tot_s[0:8], s[0:8]) < 1e-5 and rel(tot_x, x) < 1e-5


# ---------------------------------------------------------------- direction
def test_thirty_steps_lower_the_kl(ops, monkeypatch):
    _, eng = _model(256, 2, 4, 'bf16', 31)
    tch, args = _teacher('bf16'), _batch(ops)
    plan = Plan(tch, 1.0, 2.0)
    kl = []
    for _ in range(30):
        eng.loss_and_grads(*args, train=True, distill=plan)
        kl.append(eng.last_distill_sums[8:16].clone())
        eng.optimizer_step(lr=1e-3)
    eng.loss_and_grads(*args, train=False, distill=plan)
    kl.append(eng.last_distill_sums[8:16].clone())
    eng.finish_updates()
    first, last = float(kl[0].sum()), float(kl[-1].sum())
    print('KL sum over the batch: first step %.4f, after 30 steps %.4f' % (first, last))
    assert np.isfinite(last) and last < first


# ---------------------------------------------------------------- refusals, and the plain call
def test_engine_refusals_by_name(ops):
    from pianobart_amd._lib import PBError
    from tests.vocab_layout_util import D_SMALL, make_dict
    eng, tch, args = _student('bf16'), _teacher('bf16'), _batch(ops)
    G = eng.G32.clone()
    cases = [(_model(64, 1, 2, 'bf16', 1, vocab=make_dict(D_SMALL), cuda=False)[1], 'layout'),
             (_model(64, 1, 2, 'bf16', 1, window=S // 2, cuda=False)[1], 'window'),
             (_model(64, 1, 2, 'bf16', 1, lm=False, cuda=False)[1], 'no LM heads'),
             (_model(64, 1, 2, 'bf16', 1, cuda=False)[1], 'another device')]
    for teacher, word in cases:
        with pytest.raises(PBError, match=word):
            eng.loss_and_grads(*args, distill=Plan(teacher, 0.5, 2.0))
    for plan, smooth, word in ((Plan(tch, 1.5, 2.0), 0.0, 'alpha'), (Plan(tch, 0.5, 0.0), 0.0, 'tau'), (Plan(tch, 0.5, float('inf')), 0.0, 'tau'),
                               (None, 1.0, 'smooth'), (None, -0.1, 'smooth'), (Plan(eng, 0.5, 2.0), 0.0, 'student engine itself'),
                               (Plan(object(), 0.5, 2.0), 0.0, 'Engine')):
        with pytest.raises(PBError, match=word):
            eng.loss_and_grads(*args, distill=plan, smooth=smooth)
    torch.cuda.synchronize()
    assert torch.equal(eng.G32, G)                                       # refused before any device work


def test_plain_call_leaves_the_distill_sums_unset(ops):
    eng, tch, args = _student('bf16'), _teacher('bf16'), _batch(ops)
    eng._seed = 5
    a = eng.loss_and_grads(*args, train=True).clone()
    assert eng.last_distill_sums is None and a.shape == (24,)
    eng.loss_and_grads(*args, train=True, smooth=0.1)
    assert eng.last_distill_sums is not None and eng.last_distill_sums.shape == (16,)
    assert bool((eng.last_distill_sums[8:] == 0).all())                 # smoothing alone: no teacher, no KL
    eng._seed = 5
    b = eng.loss_and_grads(*args, train=True, distill=None, smooth=0.0).clone()
    assert eng.last_distill_sums is None and torch.equal(a, b)
    assert eng.loss_and_grads(*args, train=False).data_ptr() == eng.scal.data_ptr()      # the plain call's own (24,) buffer, as before
