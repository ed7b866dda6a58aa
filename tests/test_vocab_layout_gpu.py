"""The vocabulary layout on the GPU: the kernels take the dictionary's layout from the caller, and the model trains, scores and generates
with any legal dictionary. Dictionaries and helpers: tests/test_vocab_layout_cpu.py (D_SMALL: total 249, odd, slot 72, every head narrow;
D_WIDE: total 2470, heads of 1030 / 518 / 300 classes).

Bounds (none is new; each is the bound the same kernel or path has at the default layout):
  * pb_token_scores against float64: 1e-4 absolute on logp and entropy, rank exact (tests/test_score_gpu.py). The wide form sums a lane's 17
    terms and then the wave's 64 partial sums: 23 roundings of 6e-8 relative on a sum >= 1, far inside the bound, as the narrow form's 11 are.
  * pb_ce_fwd_bwd: tests/test_kernels_gpu.py::test_ce_fwd_bwd (loss 1e-5 relative, hits 1e-3, argmax equal, gradient 1e-5 f32 / 1e-2 bf16).
  * column sums: 2e-5 (tests/test_kernels_gpu.py::test_colsum). pb_embed_ln_fwd / _bwd: TOL forward, 1e-4 backward (test_embed_ln_fwd_bwd).
  * pb_corrupt: bit parity with the oracle's gen_mask under replayed decisions (tests/test_corrupt_gpu.py).
  * model against the oracle: the per-precision bounds of tests/test_model_gpu.py::test_shape_sweep_forward_loss_and_gradients_against_the_oracle;
    one fused step: the bounds of test_five_training_steps_follow_the_oracle at lr 2e-5 (one step is inside what five may drift).
  * generation: equality with the host loop, token for token and RNG state for RNG state; rewinds <= 2
    (tests/test_model_gpu.py::test_device_sampled_decode_emits_the_host_loops_tokens)."""
import random

import numpy as np
import pytest
import torch

from tests.golden_util import load_vocab, randomize_params
from tests.vocab_layout_util import D_DEFAULT, D_RANKED, D_SMALL, D_WIDE, make_dict, synth_batch

pytestmark = pytest.mark.gpu
TOL = {torch.float32: 2e-5, torch.bfloat16: 2e-2}                  # tests/test_kernels_gpu.py
BF16_LOGITS, BF16_LOSS, BF16_NORM = 5e-2, 2e-3, 2e-2               # tests/test_model_gpu.py
DICTS = {'small': D_SMALL, 'wide': D_WIDE}
T_ROWS = 37


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from pianobart_amd import ops as o
    return o


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _kernel_rows(sizes, seed):
    """T_ROWS rows of N(0, 4) logits over the dictionary's total, targets in range with the edge cases planted (class 0, the head's last id
    n - 1, a special id = PAD), and a 0 / 1 row mask with zeros at the first, a middle and the last row."""
    g = torch.Generator().manual_seed(seed)
    V = sum(sizes)
    x = 2.0 * torch.randn(T_ROWS, V, generator=g)
    tgt = torch.stack([torch.randint(0, n, (T_ROWS,), generator=g) for n in sizes], 1)
    tgt[1] = 0
    tgt[2] = torch.tensor([n - 1 for n in sizes])
    tgt[3] = torch.tensor([n - 6 for n in sizes])
    off = np.concatenate([[0], np.cumsum(sizes)])
    x[4, off[0]] = x[4, off[0] + 1] = 50.0                          # a tie at the top of head 0: the lower index wins
    tgt[4, 0] = 1
    mask = torch.ones(T_ROWS)
    mask[0] = mask[17] = mask[T_ROWS - 1] = 0
    return x, tgt, mask, off


# ---------------------------------------------------------------------------------------------------- kernels against float64
@pytest.mark.parametrize('name', ['small', 'wide'])
def test_token_scores_against_float64(ops, name):
    sizes = DICTS[name]
    lay = ops.Layout(sizes)
    x, tgt, mask, off = _kernel_rows(sizes, 11)
    t16 = tgt.to(torch.int16)
    t16[mask == 0] = 32767                                         # never read under a zero of the mask
    x64, xn = x.double(), x.numpy()
    ref_lp, ref_en, ref_rk = torch.zeros(T_ROWS, 8, dtype=torch.double), torch.zeros(T_ROWS, 8, dtype=torch.double), -np.ones((T_ROWS, 8), dtype=np.int64)
    for i in range(8):
        lsm = torch.log_softmax(x64[:, off[i]:off[i + 1]], dim=-1)
        p = lsm.exp()
        e = -torch.where(p > 0, p * lsm, torch.zeros_like(p)).sum(-1)
        for r in range(T_ROWS):
            if mask[r] == 0:
                continue
            t = int(tgt[r, i])
            ref_lp[r, i], ref_en[r, i] = lsm[r, t], e[r]
            seg = xn[r, off[i]:off[i + 1]]
            ref_rk[r, i] = int((seg > seg[t]).sum() + (seg[:t] == seg[t]).sum())
    assert ref_rk[4, 0] == 1                                       # the planted tie
    for extras in (True, False):
        logp = torch.full((T_ROWS, 8), 7.0, device='cuda')
        ent = torch.full((T_ROWS, 8), 7.0, device='cuda') if extras else None
        rank = torch.full((T_ROWS, 8), 7, dtype=torch.int16, device='cuda') if extras else None
        ops.token_scores(x.cuda(), t16.cuda(), mask.cuda(), logp, ent, rank, layout=lay)
        torch.cuda.synchronize()
        dead = mask == 0
        e_lp = float((logp.cpu().double() - ref_lp).abs().max())
        assert (logp.cpu()[dead] == 0).all()
        if extras:
            e_en = float((ent.cpu().double() - ref_en).abs().max())
            print('token_scores %s: max |logp - f64| = %.3e, max |entropy - f64| = %.3e' % (name, e_lp, e_en))
            assert e_en < 1e-4 and (ent.cpu()[dead] == 0).all() and (rank.cpu()[dead] == -1).all()
            assert np.array_equal(rank.cpu().numpy().astype(np.int64), ref_rk)
        assert e_lp < 1e-4


@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('name', ['small', 'wide'])
def test_ce_fwd_bwd_against_float64(ops, name, dt):
    """tests/test_kernels_gpu.py::test_ce_fwd_bwd at another dictionary: D_WIDE runs the kernel's general form end to end (a head over 320
    classes), D_SMALL the register form at a row stride of 249 floats."""
    sizes = DICTS[name]
    lay = ops.Layout(sizes)
    x, tgt, mask, off = _kernel_rows(sizes, 12)
    V = lay.vocab
    g = torch.Generator().manual_seed(5)
    m = (torch.rand(T_ROWS, 8, generator=g) < 0.4).float() * mask[:, None]
    m[:, 5] = 0
    m[1, 5] = 1                                                    # one loss position in head 5
    m[1:5] = 1                                                     # the planted targets count
    logits, target, md = x.cuda(), tgt.cuda(), m.cuda().contiguous()
    w = torch.tensor([sizes[i] for i in (0, 1, 3, 4, 5, 2, 7, 6)], device='cuda', dtype=torch.float32)      # dictionary key order, as the engine's loss_w
    counts, coef = torch.empty(8, device='cuda'), torch.empty(8, device='cuda')
    partials = torch.empty(int(ops.LIB.query('pb_ce_partials_floats')), device='cuda')
    ops.mask_count(md, counts, partials)
    ops.loss_coef(counts, w, coef)
    sums = torch.zeros(24, device='cuda')
    dl = torch.full((T_ROWS, V), 9.0, device='cuda', dtype=dt)
    am = torch.empty(T_ROWS, 8, device='cuda', dtype=torch.int16)
    ops.ce_fwd_bwd(logits, target.to(torch.int16), md, sums, partials, coef, dl, am, layout=lay)
    ld = logits.double().requires_grad_(True)
    total = 0
    for i in range(8):
        seg = ld[:, off[i]:off[i + 1]]
        ce = torch.nn.functional.cross_entropy(seg, target[:, i], reduction='none')
        li = (ce * md[:, i].double()).sum() / md[:, i].double().sum()
        assert abs(float(sums[i]) / float(sums[8 + i]) - float(li)) < 1e-5 * max(1, abs(float(li))), i
        first = torch.from_numpy(np.argmax(seg.detach().cpu().numpy(), -1))                     # np.argmax: the lowest index among equals
        ok = ((first == target[:, i].cpu()).double() * md[:, i].double().cpu()).sum()
        assert abs(float(sums[16 + i]) - float(ok)) < 1e-3
        assert torch.equal(am[:, i].long().cpu(), first)
        total = total + li * w[i].double()
    (total / w.double().sum()).backward()
    assert _rel(dl, ld.grad) < (1e-5 if dt == torch.float32 else 1e-2)
    assert int(am[4, 0]) == 0                                      # the tie: the lower index


@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('T', [T_ROWS, 301])
def test_colsum_any_at_an_odd_total(ops, T, dt):
    """The head-bias gradient's column sums at V = 249 (pb_colsum needs multiples of 4 and keeps refusing others): accumulates, deterministic,
    also for a column slice of a wider matrix and an output that is not 16-byte aligned; T = 301: several row blocks."""
    from pianobart_amd._lib import PBError
    N, W = 249, 253
    g = torch.Generator(device='cuda').manual_seed(T)
    wide = torch.full((T, W), 1e6, device='cuda', dtype=dt)
    wide[:, 3:3 + N] = torch.randn(T, N, device='cuda', generator=g).to(dt)
    dense = wide[:, 3:3 + N].contiguous()
    partials = torch.empty(int(ops.LIB.query('pb_colsum_partials_floats', N)), device='cuda')
    buf = torch.full((N + 5,), 0.25, device='cuda')
    runs = []
    for src, ld in ((dense, None), (dense, None), (wide[:, 3:3 + N], W)):
        buf.fill_(0.25)
        ops.colsum_any(src, buf[1:1 + N], partials, T, N, ld=ld)
        assert bool((buf[:1] == 0.25).all()) and bool((buf[1 + N:] == 0.25).all())
        runs.append(buf[1:1 + N].clone())
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    assert _rel(runs[0], 0.25 + dense.double().sum(0)) < 2e-5
    with pytest.raises(PBError, match='pb_colsum'):
        ops.colsum(dense, buf[1:1 + N], partials, T, N)            # the 4-column kernel still says no


@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('name', ['small', 'wide'])
def test_embed_ln_fwd_bwd_with_the_dictionarys_table_slots(ops, name, dt):
    """tests/test_kernels_gpu.py::test_embed_ln_fwd_bwd on the projected table of another dictionary: 8 slots of 72 / 1032 rows, ids up to
    each head's last one."""
    sizes = DICTS[name]
    lay = ops.Layout(sizes)
    assert lay.tab_rows == (72 if name == 'small' else 1032)
    d, B, S = 128, 1, T_ROWS
    T = B * S
    g = torch.Generator(device='cuda').manual_seed(9)
    ids = torch.stack([torch.randint(0, n, (T,), device='cuda', generator=g) for n in sizes], dim=1)
    ids[0] = torch.tensor([n - 1 for n in sizes], device='cuda')
    ids[1] = 0
    P = torch.randn(lay.tab_total, d, device='cuda', generator=g)
    lb = torch.randn(d, device='cuda', generator=g); pos = torch.randn(S + 2, d, device='cuda', generator=g)
    w = 1 + 0.2 * torch.randn(d, device='cuda', generator=g); b = 0.2 * torch.randn(d, device='cuda', generator=g)
    ids16 = ops.ids_to_i16(ids)
    y = torch.empty(T, d, device='cuda', dtype=dt); mean = torch.empty(T, device='cuda'); rstd = torch.empty(T, device='cuda')
    ops.embed_ln_fwd(ids16, P, lb, pos, w, b, y, mean, rstd, S, 1e-5, 0, 0, 0.0, padded=True, layout=lay)
    Pd = P.double().requires_grad_(True); lbd = lb.double().requires_grad_(True); posd = pos.double().requires_grad_(True)
    wd = w.double().requires_grad_(True); bd = b.double().requires_grad_(True)
    off = torch.tensor(lay.tab_off[:8], device='cuda')
    z = Pd[(ids + off).reshape(-1)].reshape(T, 8, d).sum(1) + lbd + posd[2:2 + S].repeat(B, 1)
    yr = torch.nn.functional.layer_norm(z, (d,), wd, bd, 1e-5)
    assert _rel(y, yr) < TOL[dt]
    dy = torch.randn(T, d, device='cuda', generator=g).to(dt)
    dy[7] = 0
    yr.backward(dy.double())
    dP = torch.zeros_like(P); dpos = torch.zeros_like(pos); dlb = torch.zeros(d, device='cuda')
    dg = torch.zeros(d, device='cuda'); db = torch.zeros(d, device='cuda')
    partials = torch.empty(int(ops.LIB.query('pb_ln_partials_floats', d)), device='cuda')
    ops.embed_ln_bwd(dy, ids16, P, lb, pos, w, mean, rstd, dP, dpos, dlb, dg, db, partials, S, 0, 0, 0.0, padded=True, layout=lay)
    assert _rel(dP, Pd.grad) < 1e-4 and _rel(dpos, posd.grad) < 1e-4 and _rel(dlb, lbd.grad) < 1e-4
    assert _rel(dg, wd.grad) < 1e-4 and _rel(db, bd.grad) < 1e-4
    # the one-hot route's matrix over the same slots: ones at tab_off[h] + id, nothing else
    oh = torch.full((T, lay.tab_total), 3.0, device='cuda', dtype=torch.bfloat16)
    ops.onehot_build(ids16, oh, padded=True, layout=lay)
    want = torch.zeros(T, lay.tab_total, device='cuda')
    want.scatter_(1, ids + off, 1.0)
    assert torch.equal(oh.float(), want)


def test_corrupt_on_the_small_dictionary_replays_the_oracles_decisions(ops):
    """tests/test_corrupt_gpu.py's differential run with D_SMALL's PAD / MASK rows and tables: the oracle's gen_mask under its own seeds, its
    random decisions replayed through pb_corrupt_replay -- rows and loss mask bit for bit; and the Philox-driven kernel draws its random rows
    inside this dictionary's tables."""
    from oracle import pianobart_oracle as O
    from pianobart_amd._lib import LIB
    e2w, w2e = make_dict(D_SMALL)
    S = 40
    pb = O.PianoBart(O.BartConfig(max_position_embeddings=S, d_model=32, encoder_layers=1, decoder_layers=1, encoder_ffn_dim=64,
                                  decoder_ffn_dim=64, encoder_attention_heads=4, decoder_attention_heads=4), e2w, w2e)
    corr = O.Corruptor(pb, S, 0.15)
    pad, mask_row = pb.pad_word_np.astype(np.int64), pb.mask_word_np.astype(np.int64)
    assert pad.tolist() == [n - 6 for n in D_SMALL]
    seqs = [synth_batch(D_SMALL, 1, S, seed=70 + k, min_len=3)[5][0].numpy() for k in range(6)]
    seqs[0][:] = pad                                               # an all-PAD window
    cases = []
    for k, x in enumerate(seqs):
        for choice in range(1, 6):
            random.seed(500 + 7 * k + choice); np.random.seed(500 + 7 * k + choice)
            corr.trace = {}
            masked, pos = corr.gen_mask(torch.from_numpy(x).long(), choice)
            tr = corr.trace
            cases.append(dict(ids=x.astype(np.int64), choice=tr['choice'], dec=tr['dec'], rand_rows=tr.get('rand_rows'),
                              masked=np.asarray(masked).astype(np.int64), pos=np.asarray(pos).astype(np.int64).reshape(S, -1)[:, 0]))
    corr.trace = None
    B = len(cases)
    stride = int(LIB.query('pb_corrupt_replay_stride', S))
    dec = np.zeros((B, stride), dtype=np.int32)
    rr = np.zeros((B, S, 8), dtype=np.int16)
    for b, c in enumerate(cases):
        dec[b, :len(c['dec'])] = c['dec']
        if c['rand_rows'] is not None:
            rr[b] = c['rand_rows']
    ids = torch.from_numpy(np.stack([c['ids'] for c in cases]))
    ids16 = ops.ids_to_i16(ids.cuda())
    out = torch.full_like(ids16, -1); lm = torch.full((B, S, 8), -1.0, device='cuda')
    ch = torch.tensor([c['choice'] for c in cases], dtype=torch.int32, device='cuda')
    ops.corrupt_replay(ids16, out, lm, ch, 0.15, torch.from_numpy(dec).cuda(), torch.from_numpy(rr).cuda(), pad, mask_row)
    torch.cuda.synchronize()
    out, lm = out.cpu().numpy().astype(np.int64), lm.cpu().numpy()
    for b, c in enumerate(cases):
        assert np.array_equal(out[b], c['masked']), ('rows', c['choice'], b)
        assert np.array_equal(lm[b], np.repeat(c['pos'][:, None], 8, 1).astype(np.float32)), ('loss mask', c['choice'], b)
    # the device's own decisions (token mask): the random rows stay inside D_SMALL's tables, the MASK rows are D_SMALL's
    x = torch.from_numpy(np.stack(seqs[1:])).cuda()
    x16 = ops.ids_to_i16(x)
    out = torch.empty_like(x16); lm = torch.empty(len(seqs) - 1, S, 8, device='cuda')
    ch = torch.full((len(seqs) - 1,), 2, dtype=torch.int32, device='cuda')
    ops.corrupt(x16, out, lm, ch, None, 0.15, 7, pad, mask_row, D_SMALL)
    o = out.cpu().numpy().astype(np.int64)
    sel = lm.cpu().numpy()[:, :, 0] == 1
    assert all((o[:, :, c] < D_SMALL[c]).all() and (o[:, :, c] >= 0).all() for c in range(8))
    assert (o[~sel] == x.cpu().numpy()[~sel]).all() and ((o == mask_row).all(-1) & sel).sum() == (len(seqs) - 1) * round(round(S * 0.15) * 0.8)


# ---------------------------------------------------------------------------------------------------- model against the oracle
_MODEL_KW = dict(max_position_embeddings=40, d_model=128, encoder_layers=2, decoder_layers=2, encoder_ffn_dim=512, decoder_ffn_dim=512,
                 encoder_attention_heads=4, decoder_attention_heads=4, dropout=0.0)
_ORACLE = {}


def _oracle_case(name):
    """The oracle's side of the model test, computed once per dictionary and left unchanged: state_dict, batch, logits, loss, gradients and
    the parameters after one clipped AdamW step at lr 2e-5."""
    if name not in _ORACLE:
        from oracle import pianobart_oracle as O
        sizes = DICTS[name]
        e2w, w2e = make_dict(sizes)
        o = O.PianoBartLM(O.PianoBart(O.BartConfig(**_MODEL_KW), e2w, w2e)).train()
        randomize_params(o, 5)
        sd = {k: v.clone() for k, v in o.state_dict().items()}
        batch = synth_batch(sizes, 2, 40, seed=168, min_len=13)
        enc, dec, loss_mask, emask, dmask, target = batch
        yo = o(enc, dec, emask, dmask)
        tot, *_ = O.pretrain_loss(yo, target, loss_mask, e2w)
        tot.backward()
        grads = {k: p.grad.clone() for k, p in o.named_parameters() if p.grad is not None}
        live = [p for p in o.parameters() if p.grad is not None]
        gl = [p.grad for p in live]
        O.clip_grad_norm(gl, 3.0)
        with torch.no_grad():
            O.hf_adamw_step([p.data for p in live], gl, [torch.zeros_like(p) for p in live], [torch.zeros_like(p) for p in live], step=1, lr=2e-5)
        after = {k: p.detach().clone() for k, p in o.named_parameters()}
        _ORACLE[name] = dict(e2w=e2w, w2e=w2e, sd=sd, batch=batch, logits=torch.cat(yo, -1).detach(), loss=float(tot.detach()), grads=grads, after=after,
                             weights=O.loss_weights(e2w))
    return _ORACLE[name]


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3', 'bf16'])
@pytest.mark.parametrize('name', ['small', 'wide'])
def test_model_forward_loss_gradients_and_one_fused_step_against_the_oracle(ops, name, precision):
    from oracle import pianobart_oracle as O
    from pianobart_amd.model import BartConfig, PianoBart, PianoBartLM
    c = _oracle_case(name)
    sizes, e2w = DICTS[name], c['e2w']
    m = PianoBartLM(PianoBart(BartConfig(**_MODEL_KW), e2w, c['w2e'], precision=precision))
    m.load_state_dict(c['sd'], strict=True)
    m = m.train().cuda()
    enc, dec, loss_mask, emask, dmask, target = [t.cuda() for t in c['batch']]
    y = m(enc, dec, emask, dmask)
    assert [t.shape[-1] for t in y] == sizes and all(t.shape[:2] == (2, 40) for t in y)          # callers see exactly V columns, split at the heads
    tot, *_ = O.pretrain_loss(y, target, loss_mask, e2w)
    tot.backward()
    tl, tloss, tnorm, tgrad = {'fp32': (1e-4, 1e-4, 1e-3, 2e-3), 'bf16x3': (2e-4, 1e-5, 1e-4, 2e-3), 'bf16': (BF16_LOGITS, BF16_LOSS, BF16_NORM, None)}[precision]
    e_l = _rel(torch.cat(y, -1).detach(), c['logits'])
    e_loss = abs(float(tot.detach()) - c['loss']) / c['loss']
    go = c['grads']
    gm = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    assert sorted(go) == sorted(gm)
    n_o = float(torch.sqrt(sum((g.double() ** 2).sum() for g in go.values())))
    n_m = float(torch.sqrt(sum((g.double().cpu() ** 2).sum() for g in gm.values())))
    e_n = abs(n_m - n_o) / n_o
    print('layout %s %s: logits %.2e loss %.2e grad-norm %.2e' % (name, precision, e_l, e_loss, e_n))
    assert e_l < tl and e_loss < tloss and e_n < tnorm, (e_l, e_loss, e_n)
    if tgrad is not None:
        scale = max(float(g.abs().max()) for g in go.values())
        for k, g in go.items():
            err = float((gm[k].cpu().double() - g.double()).abs().max())
            assert err < tgrad * max(float(g.abs().max()), 1e-3 * scale), (k, err, float(g.abs().max()))
    # an id equal to a head's size: IndexError that names this dictionary's tables
    with torch.no_grad():
        for col in (0, 4):
            bad = enc.clone()
            bad[1, 3, col] = sizes[col]
            with pytest.raises(IndexError, match=str(sizes).replace('[', r'\[').replace(']', r'\]')):
                m(bad, dec, emask, dmask)
        m(enc, dec, emask, dmask)                                  # the mark does not stick
    # one fused step: loss_and_grads + clip + AdamW
    for p in m.parameters():
        p.grad = None
    eng = m._get_engine()
    sums = eng.loss_and_grads(ops.ids_to_i16(enc), ops.ids_to_i16(dec), ops.ids_to_i16(target), loss_mask.contiguous(), emask, dmask, train=True)
    s = sums.double().cpu()
    w = torch.tensor(c['weights'], dtype=torch.double)
    f_loss = float(((s[0:8] / s[8:16]) * w).sum() / w.sum())
    gn = float(torch.sqrt(sum((g.double() ** 2).sum() for g in eng.grad_views)))
    assert abs(f_loss - c['loss']) / c['loss'] < max(tloss, 2e-4), (f_loss, c['loss'])          # 2e-4: the fused loss bound of the five-steps test
    assert abs(gn - n_o) / n_o < tnorm, (gn, n_o)
    eng.optimizer_step(lr=2e-5)
    eng.finish_updates()
    torch.cuda.synchronize()
    worst, worst_k = 0.0, ''
    for k, p in m.named_parameters():
        if k not in go:
            continue
        assert torch.isfinite(p).all(), k
        if k.endswith('k_proj.bias'):                              # a zero gradient's rounding noise through AdamW's 1 / (sqrt(v) + eps): bounded by lr
            assert float((p.detach().cpu().double() - c['after'][k].double()).abs().max()) <= 2e-5 * 1.01
            continue
        r = _rel(p.detach(), c['after'][k])
        if r > worst:
            worst, worst_k = r, k
    print('layout %s %s: worst parameter after one fused step %.2e (%s)' % (name, precision, worst, worst_k))
    if precision != 'bf16':
        assert worst < (2e-5 if precision == 'fp32' else 3e-4), (worst, worst_k)
    else:                                                          # bf16 gradients: the step's direction may differ where |g| ~ eps; its size may not
        for k, p in m.named_parameters():
            if k in go:
                assert float((p.detach().cpu().double() - c['sd'][k].double()).abs().max()) <= 2e-5 * (1 + 0.01 * float(c['sd'][k].abs().max())) * 1.01, k


# ---------------------------------------------------------------------------------------------------- generation
_GEN = {}


def _gen_model(name):
    """d = 256, 4 heads (head dim 64: the fused decoder covers it), 2 layers, ffn 512, S = 48, bf16; every special id is biased away but the bar
    head's EOS, so EOS stays reachable (about one draw in a head's size) and most rows live long enough to meet their stop bar. Built once per
    dictionary."""
    if name not in _GEN:
        from pianobart_amd.model import BartConfig, PianoBart, PianoBartLM
        sizes = {'small': D_SMALL, 'wide': D_WIDE, 'default': D_DEFAULT, 'ranked': D_RANKED}[name]
        e2w, w2e = load_vocab() if name == 'default' else make_dict(sizes)
        S = 48
        cfg = BartConfig(max_position_embeddings=S, d_model=256, encoder_layers=2, decoder_layers=2, encoder_ffn_dim=512, decoder_ffn_dim=512,
                         encoder_attention_heads=4, decoder_attention_heads=4)
        m = PianoBartLM(PianoBart(cfg, e2w, w2e, precision='bf16')).eval()
        randomize_params(m, 31)
        with torch.no_grad():
            for i, n in enumerate(sizes):
                m.mask_lm.proj[i].bias[n - 6:] = -30.0
            m.mask_lm.proj[0].bias[sizes[0] - 3] = 0.0               # the bar head's EOS
        m = m.cuda()
        enc = synth_batch(sizes, 3, S, seed=8, min_len=S - 9)[5].cuda()
        emask = (enc[:, :, 0] != sizes[0] - 6).float()
        _GEN[name] = (m, enc, emask, sizes)
    return _GEN[name]


def _single(m, enc, emask, b, seed, **kw):
    np.random.set_state(np.random.RandomState(seed).get_state())
    y = m(enc[b:b + 1], None, emask[b:b + 1], None, generate=True, device_num=-1, **kw)
    return y[0], np.random.get_state()[1].copy(), dict(m._get_engine().last_decode)


def test_wide_device_sampler_emits_the_host_loops_tokens(ops, monkeypatch):
    from pianobart_amd import generation as E
    m, enc, emask, sizes = _gen_model('wide')
    eng = m._get_engine()
    sampler = dict(T=m.SAMPLE_T, P=m.SAMPLE_P)

    def run(spec, fault=0, seed=5):
        monkeypatch.setattr(E, '_DECODE_SPEC', spec)
        eng.decode_fault_period = fault
        np.random.seed(seed)
        out = eng.generate(enc[:1], emask[:1], m.sample_row, sampler=sampler)
        return out.cpu(), np.random.get_state()[1].copy(), dict(eng.last_decode)

    try:
        want, st_w, info_w = run(0)
        got, st_g, info_g = run(1)
        assert not info_w.get('device_sampler') and info_g['device_sampler'] is True and info_g['sampler_form'] == 'wide' and eng.last_sampler_form == 'wide' and info_g['graph']
        assert info_g['tokens'] == info_w['tokens'] and torch.equal(got, want) and np.array_equal(st_g, st_w)
        assert info_g['rewinds'] <= 2, info_g
        assert int(want[0, :, 0].max()) > 272 and int(want[0, :, 3].max()) > 272          # the wide heads really sampled beyond the narrow rows
        got_f, st_f, info_f = run(1, fault=7)
        assert torch.equal(got_f, want) and np.array_equal(st_f, st_w) and info_f['rewinds'] > 0, info_f
    finally:
        eng.decode_fault_period = 0


@pytest.mark.parametrize('name', ['wide', 'small'])
def test_generate_batch_equals_the_batch_1_runs(ops, name):
    """Three prompts at once: row 0 with a forced head-0 id (1000 on the wide dictionary: beyond the narrow sampler's rows), row 1 stopped at a
    bar, row 2 time-ordered. Each row is what forward(generate=True) gives for it alone under its own generator."""
    from pianobart_amd import generation as G
    from pianobart_amd.generation import is_time_ordered
    m, enc, emask, sizes = _gen_model(name)
    S, pad0 = enc.shape[1], sizes[0] - 6
    given, stop_bar = (1000, 700) if name == 'wide' else (60, 45)
    forced = -torch.ones(3, S, 8, dtype=torch.long)
    forced[0, 2, 0] = given
    stops, orders, seeds = [pad0, stop_bar, pad0], [-1, -1, 0], [21, 22, 23]
    y = m.generate_batch(enc, emask, seeds=seeds, decoder_forced=forced, decoder_stop=stops, decoder_order=orders)
    info = dict(m._get_engine().last_decode)
    assert info['batched'] and info['device_sampler'] and info.get('sampler_form', 'narrow') == m._get_engine().last_sampler_form == ('wide' if name == 'wide' else 'narrow')
    assert m._get_engine().last_sampler_form == G.sampler_form_for(sizes, m.SAMPLE_P)
    # the forced, stopped and ordered rows run the device sampler's own branches; the host's verification would hide a defect there behind
    # rewinds, so they are bounded per row as for the unconstrained generate (tests/test_model_gpu.py: <= 2)
    assert len(info['rewinds']) == 3 and max(info['rewinds']) <= 2, info['rewinds']
    for b in range(3):
        one, _, _ = _single(m, enc, emask, b, seeds[b], decoder_forced=forced[b:b + 1] if b == 0 else None,
                            decoder_stop=stops[b] if b == 1 else None, decoder_order=orders[b] if b == 2 else None)
        assert torch.equal(y[b], one), b
    if name != 'wide':                                             # the small dictionary: the batch equality above, once
        return
    assert int(y[0, 2, 0]) == given
    # row 1 ends at its first bar >= the stop bar: the unstopped run of the same generator, cut there
    free, _, _ = _single(m, enc, emask, 1, seeds[1])
    hit = np.flatnonzero(free[:, 0].numpy() >= stop_bar)
    assert len(hit) and int(free[hit[0], 0]) < pad0, 'the free run never reaches bar %d' % stop_bar
    cut = int(hit[0])
    assert torch.equal(y[1, :cut], free[:cut]) and bool((y[1, cut:, 0] == pad0).all()) and bool((y[1, :cut, 0] < stop_bar).all())
    assert info['ended'][1] == 'bar'
    n2 = int((y[2, :, 0] != pad0).sum())
    assert n2 > 4 and is_time_ordered(y[2, :n2].numpy())
    # score() of the generated rows: rank == 0 exactly where the target is the (first) argmax of the pass's logits
    lay = m.pianobart.layout
    r = m.score(enc, y.cuda(), emask, device_num=-1)
    eng = m._get_engine()
    logits = eng._cur_ws['logits'][:3 * S].float().cpu().numpy().reshape(3, S, lay.vocab)
    scored = (r.rank >= 0).all(-1).numpy()
    assert scored.sum() == int(r.count.sum()) > 20
    for h in range(8):
        am = np.argmax(logits[:, :, lay.seg_off[h]:lay.seg_off[h + 1]], -1)
        assert np.array_equal((r.rank[:, :, h].numpy() == 0)[scored], (am == y[:, :, h].numpy())[scored]), h
    assert (r.rank.numpy()[~scored] == -1).all() and bool((r.logp[torch.from_numpy(scored)] <= 0).all())


def test_many_ranked_classes_select_the_wide_sampler_and_generate(ops, monkeypatch):
    """D_RANKED (pos_resolution doubled): every head fits the narrow sampler's rows, but the heads with p < 1 hold 579 classes, more than its
    512 rank threads. The decoder takes the wide sampler instead of refusing: generate gives the host loop's tokens and np.random state with at
    most 2 rewinds, and a batch equals its batch-1 runs."""
    from pianobart_amd import generation as E
    m, enc, emask, sizes = _gen_model('ranked')
    assert max(sizes) <= 272 and E.sampler_form_for(sizes, m.SAMPLE_P) == 'wide'
    eng = m._get_engine()
    sampler = dict(T=m.SAMPLE_T, P=m.SAMPLE_P)

    def run(spec, seed=5):
        monkeypatch.setattr(E, '_DECODE_SPEC', spec)
        np.random.seed(seed)
        out = eng.generate(enc[:1], emask[:1], m.sample_row, sampler=sampler)
        return out.cpu(), np.random.get_state()[1].copy(), dict(eng.last_decode)

    want, st_w, info_w = run(0)
    got, st_g, info_g = run(1)
    assert info_g['device_sampler'] is True and info_g['sampler_form'] == 'wide' and eng.last_sampler_form == 'wide'
    assert info_g['tokens'] == info_w['tokens'] and torch.equal(got, want) and np.array_equal(st_g, st_w)
    assert info_g['rewinds'] <= 2, info_g
    yb = m.generate_batch(enc, emask, seeds=[31, 32, 33])
    info = dict(eng.last_decode)
    assert info['batched'] and info['sampler_form'] == 'wide' and max(info['rewinds']) <= 2, info
    for b in range(3):
        one, _, _ = _single(m, enc, emask, b, 31 + b)
        assert torch.equal(yb[b], one), b


def test_default_dictionary_keeps_the_narrow_sampler(ops):
    m, enc, emask, sizes = _gen_model('default')
    assert m.pianobart.layout == ops.DEFAULT_LAYOUT
    eng = m._get_engine()
    eng.last_sampler_form = None
    y, _, info = _single(m, enc, emask, 0, 3)
    # the record names the sampler only when it is the wide one (tests/test_decode_info_gpu.py pins the default record's keys); the engine says which
    assert info['device_sampler'] is True and 'sampler_form' not in info and eng.last_sampler_form == 'narrow'
    eng.last_sampler_form = None
    yb = m.generate_batch(enc[:2], emask[:2], seeds=[3, 4])
    assert 'sampler_form' not in eng.last_decode and eng.last_sampler_form == 'narrow' and torch.equal(yb[0], y)
