"""GPU: LoRA through the engine (Engine.attach_lora / merge_lora, pianobart_amd.lora) against the oracle evaluated on merged weights
W + s B A (tests/lora_ref.py).

Models: that of test_five_training_steps_follow_the_oracle (S 48, d 64, 2 + 2 layers, ffn 128, 4 heads, B 3, dropout 0) and the shape sweep's
(24, 96, 1, 2, 160, 96, 1, 3), whose two decoder layers on one encoder layer exercise the stacked cross K / V strides; neither is large enough for
the bf16 engine to pack its rows, so the packed step has a shape of its own ('pack' below). All six targets are adapted unless a test says otherwise, so every column slice is exercised.

bf16 against the existing path (test_bf16_adapter_path_is_as_close_to_the_oracle_as_the_full_path), distances from the oracle on the merged
weights, measured on an MI355X (logits rel | loss rel), adapter path | this commit's unfrozen bf16 engine on the merged checkpoint:
  see DESIGN.md 5 "LoRA" for the recorded values; the test prints both and holds the adapter path to 2 times the existing one."""
import os

import numpy as np
import pytest
import torch

from tests import lora_ref as R
from tests.golden_util import load_vocab, randomize_params, synth_octuple_batch

pytestmark = pytest.mark.gpu
E2W, W2E = load_vocab()
# S, d, Le, Ld, fe, fd, h, B. 'pack': head_dim 64, B * S = 4 tiles of 256 rows and short pieces, so that the bf16 engine packs its rows (rowpack.pack_batch
# rounds the packed row counts up to whole 256-row tiles and stays dense unless 3 % of the rows go)
SHAPES = {'five': (48, 64, 2, 2, 128, 128, 4, 3), 'sweep': (24, 96, 1, 2, 160, 96, 1, 3), 'pack': (128, 128, 1, 2, 256, 256, 2, 8)}
ALL = ('q', 'k', 'v', 'cq', 'ck', 'cv')


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


def _kw(shape):
    S, d, Le, Ld, fe, fd, h, B = SHAPES[shape]
    return dict(max_position_embeddings=S, d_model=d, encoder_layers=Le, decoder_layers=Ld, encoder_ffn_dim=fe, decoder_ffn_dim=fd,
                encoder_attention_heads=h, decoder_attention_heads=h, dropout=0.0)


def _lm(shape, precision, seed=61, sd=None):
    from pianobart_amd.model import BartConfig, PianoBart, PianoBartLM
    m = PianoBartLM(PianoBart(BartConfig(**_kw(shape)), E2W, W2E, precision=precision))
    if sd is None:
        randomize_params(m, seed)
    else:
        m.load_state_dict(sd, strict=True)
    return m


def _oracle(shape, sd):
    from oracle import pianobart_oracle as O
    o = O.PianoBartLM(O.PianoBart(O.BartConfig(**_kw(shape)), E2W, W2E)).train()
    o.load_state_dict(sd, strict=True)
    return o


def _batch(shape, seed):
    S, B = SHAPES[shape][0], SHAPES[shape][7]
    return synth_octuple_batch(B, S, seed=seed, min_len=8 if shape == 'pack' else max(2, S // 3))


def _args(batch):
    from pianobart_amd import ops
    enc, dec, loss_mask, emask, dmask, target = [t.cuda() for t in batch]
    return (ops.ids_to_i16(enc), ops.ids_to_i16(dec), ops.ids_to_i16(target), loss_mask.contiguous(), emask, dmask)


def _engine(m):
    m = m.cuda().train()
    eng = m._get_engine()
    eng.bind(torch.device('cuda', 0))
    return m, eng


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max())


def _loss(sums):
    from oracle import pianobart_oracle as O
    s = sums.double().cpu()
    w = torch.tensor(O.loss_weights(E2W), dtype=torch.double)
    return float(((s[0:8] / s[8:16]) * w).sum() / w.sum())


def _dense(eng, args, train=False):
    """A dense step (argmax_out keeps the rows unpacked): (sums, logits (T, V)) as clones."""
    T = args[0].shape[0] * args[0].shape[1]
    am = torch.empty(T, 8, dtype=torch.int16, device='cuda')
    sums = eng.loss_and_grads(*args, train=train, argmax_out=am).clone()
    return sums, eng._cur_ws['logits'][:T].clone()


def _randomize_adapters(st, seed, b_scale=0.1):
    """A ~ N(0, 1 / K), B ~ N(0, b_scale^2): non-zero both, so every term of the backward is live."""
    g = torch.Generator().manual_seed(seed)
    for s in st.sites:
        s.A.copy_((torch.randn(st.r, s.K, generator=g) / s.K ** 0.5).cuda())
        s.B.copy_((torch.randn(s.N, st.r, generator=g) * b_scale).cuda())


def _adapters_cpu(m, st):
    from pianobart_amd import lora
    names = lora._site_names(m, st)
    return {names[s.key] + '.weight': (s.A.detach().cpu().clone(), s.B.detach().cpu().clone()) for s in st.sites}


def _merged_sd(sd, adapters, scale):
    out = {k: v.clone() for k, v in sd.items()}
    for k, (A, B) in adapters.items():
        out[k] = (sd[k].double() + scale * (B.double() @ A.double())).float()
    return out


def _cfg(rank=8, alpha=16, targets=ALL):
    from pianobart_amd.lora import LoraConfig
    return LoraConfig(rank=rank, alpha=alpha, targets=targets)


# ---------------------------------------------------------------------------------------------------------------------- B = 0 identity
@pytest.mark.parametrize('shape,precision', [('five', 'fp32'), ('five', 'bf16'), ('sweep', 'fp32'), ('sweep', 'bf16'), ('pack', 'bf16')])
def test_zero_B_is_the_base_model_bit_for_bit(shape, precision):
    """Freshly attached adapters (B = 0) add exact zeros: the 24 sums and the logits of loss_and_grads(train=False) are torch.equal to the same
    engine's without adapters, packed (where the engine packs) and dense (argmax_out)."""
    _need_gpu()
    m, eng = _engine(_lm(shape, precision))
    args = _args(_batch(shape, 301))
    base_packed = eng.loss_and_grads(*args, train=False).clone()
    rows = eng.last_rows[3]                                     # rows the LM heads ran on (a packed step: the rows with a loss term); the rest of the buffer is stale
    base_packed_logits = eng._cur_ws['logits'][:rows].clone()
    packed = eng._saved.get('pack') is not None
    base_dense = _dense(eng, args)
    eng.attach_lora(_cfg(), seed=3)
    got_packed = eng.loss_and_grads(*args, train=False).clone()
    assert (eng._saved.get('pack') is not None) == packed
    assert eng.last_rows[3] == rows
    assert torch.equal(got_packed, base_packed) and torch.equal(eng._cur_ws['logits'][:rows], base_packed_logits)
    got_dense = _dense(eng, args)
    assert torch.equal(got_dense[0], base_dense[0]) and torch.equal(got_dense[1], base_dense[1])
    print('B = 0 identity %s %s: packed step %s' % (shape, precision, packed))
    assert packed == (shape == 'pack')


# ---------------------------------------------------------------------------------------------------------------------- fp32 against the oracle
@pytest.mark.parametrize('shape', ['five', 'sweep'])
def test_fp32_forward_loss_and_adapter_gradients_against_the_oracle_on_merged_weights(shape):
    """A and B random and non-zero. Bounds of test_shape_sweep_forward_loss_and_gradients_against_the_oracle: logits 1e-4 (_rel), loss 1e-4,
    every dA, dB and head gradient within 2e-3 max(|g|max, 1e-3 scale)."""
    _need_gpu()
    from oracle import pianobart_oracle as O
    m0 = _lm(shape, 'fp32')
    sd = {k: v.detach().clone() for k, v in m0.state_dict().items()}
    o = _oracle(shape, sd)
    m, eng = _engine(m0)
    st = eng.attach_lora(_cfg(), seed=1)
    _randomize_adapters(st, 5)
    batch = _batch(shape, 302)
    enc, dec, loss_mask, emask, dmask, target = batch
    ad = {k: (A.requires_grad_(), B.requires_grad_()) for k, (A, B) in _adapters_cpu(m, st).items()}
    base = {k: v.detach() for k, v in o.state_dict().items() if not k.startswith('mask_lm.')}
    yo = R.oracle_forward(o, base, ad, st.s, enc, dec, emask, dmask)
    tot_o, *_ = O.pretrain_loss(yo, target, loss_mask, E2W)
    heads = [p for k, p in o.named_parameters() if k.startswith('mask_lm.')]
    leaves = [t for pair in ad.values() for t in pair] + heads
    grads = torch.autograd.grad(tot_o, leaves)
    T = enc.shape[0] * enc.shape[1]
    am = torch.empty(T, 8, dtype=torch.int16, device='cuda')
    sums = eng.loss_and_grads(*_args(batch), train=True, argmax_out=am)
    logits = eng._cur_ws['logits'][:T]
    e_l = _rel(logits, torch.cat(yo, -1).detach().reshape(T, -1))
    e_loss = abs(_loss(sums) - float(tot_o.detach())) / float(tot_o.detach())
    print('lora fp32 %s: logits %.2e loss %.2e' % (shape, e_l, e_loss))
    assert e_l < 1e-4 and e_loss < 1e-4, (e_l, e_loss)
    names = [k[:-len('.weight')] + tag for k in ad for tag in ('.lora_A', '.lora_B')] + [k for k, _ in o.named_parameters() if k.startswith('mask_lm.')]
    go = dict(zip(names, grads))
    gm = {}
    from pianobart_amd import lora
    sn = lora._site_names(m, st)
    for s in st.sites:
        gm[sn[s.key] + '.lora_A'], gm[sn[s.key] + '.lora_B'] = s.gA, s.gB
    off = 0
    for i in range(8):
        n = eng.lay.sizes[i]
        gm['mask_lm.proj.%d.weight' % i], gm['mask_lm.proj.%d.bias' % i] = eng.g['head.w'][off:off + n], eng.g['head.b'][off:off + n]
        off += n
    assert sorted(go) == sorted(gm)
    scale = max(float(g.abs().max()) for g in go.values())
    worst = 0.0
    for k, g in go.items():
        assert float(g.abs().max()) > 0.0, k                       # every adapter term is live
        err = float((gm[k].detach().cpu().double() - g.double()).abs().max())
        lim = 2e-3 * max(float(g.abs().max()), 1e-3 * scale)
        worst = max(worst, err / lim)
        assert err < lim, (k, err, float(g.abs().max()))
    print('lora fp32 %s: worst gradient error / bound %.3f over %d tensors' % (shape, worst, len(go)))


# ---------------------------------------------------------------------------------------------------------------------- bf16 against the existing path
@pytest.mark.parametrize('shape', ['five', 'sweep'])
def test_bf16_adapter_path_is_as_close_to_the_oracle_as_the_full_path(shape):
    """The yardstick is existing code: this commit's unfrozen bf16 engine run on the merged checkpoint, and its distance from the oracle (on the
    same merged weights) in logits and loss. The adapter path (bf16 backbone, f32 adapter term) may be at most 2 times that distance."""
    _need_gpu()
    from oracle import pianobart_oracle as O
    m0 = _lm(shape, 'bf16')
    sd = {k: v.detach().clone() for k, v in m0.state_dict().items()}
    m, eng = _engine(m0)
    st = eng.attach_lora(_cfg(), seed=1)
    _randomize_adapters(st, 6)
    merged = _merged_sd(sd, _adapters_cpu(m, st), st.s)
    o = _oracle(shape, merged)
    batch = _batch(shape, 303)
    enc, dec, loss_mask, emask, dmask, target = batch
    with torch.no_grad():
        yo = o(enc, dec, emask, dmask)
        tot_o = float(O.pretrain_loss(yo, target, loss_mask, E2W)[0])
    T = enc.shape[0] * enc.shape[1]
    ref = torch.cat(yo, -1).reshape(T, -1)
    sums, logits = _dense(eng, _args(batch))
    d_ad = (_rel(logits, ref), abs(_loss(sums) - tot_o) / tot_o)
    m2, eng2 = _engine(_lm(shape, 'bf16', sd=merged))
    sums2, logits2 = _dense(eng2, _args(batch))
    d_full = (_rel(logits2, ref), abs(_loss(sums2) - tot_o) / tot_o)
    print('lora bf16 %s: adapter path logits %.3e loss %.3e | full path on the merged checkpoint logits %.3e loss %.3e' % ((shape,) + d_ad + d_full))
    assert d_ad[0] <= 2 * d_full[0] and d_ad[1] <= 2 * d_full[1], (d_ad, d_full)


# ---------------------------------------------------------------------------------------------------------------------- training
def test_five_adapter_steps_follow_the_oracle():
    """Five loss_and_grads + optimizer_step calls, fp32, lr 1e-3, A and B random; the oracle steps only A, B and the heads with
    O.clip_grad_norm and O.hf_adamw_step. Every loss agrees to 2e-4, A, B and the heads end within 2e-3 (_rel). The backbone is never written,
    the optimizer state holds exactly 2 x (adapter + head) elements and no backbone weight-gradient GEMM is launched."""
    _need_gpu()
    from oracle import pianobart_oracle as O
    from pianobart_amd import lora
    shape, lr = 'five', 1e-3
    m0 = _lm(shape, 'fp32')
    sd = {k: v.detach().clone() for k, v in m0.state_dict().items()}
    o = _oracle(shape, sd)
    m, eng = _engine(m0)
    eng.pipeline_updates = True                                     # ignored while adapters are attached
    st = eng.attach_lora(_cfg(), seed=1)
    _randomize_adapters(st, 7)
    ad = {k: (A.requires_grad_(), B.requires_grad_()) for k, (A, B) in _adapters_cpu(m, st).items()}
    base = {k: v.detach() for k, v in o.state_dict().items() if not k.startswith('mask_lm.')}
    heads = [p for k, p in o.named_parameters() if k.startswith('mask_lm.')]
    leaves = [t for pair in ad.values() for t in pair] + heads
    mo, vo = [torch.zeros_like(p) for p in leaves], [torch.zeros_like(p) for p in leaves]
    torch.cuda.synchronize()
    p_before = eng.P32.clone()
    launches = eng.wgrad_launches
    for step in range(1, 6):
        batch = synth_octuple_batch(3, 48, seed=300 + step)
        enc, dec, loss_mask, emask, dmask, target = batch
        tot, *_ = O.pretrain_loss(R.oracle_forward(o, base, ad, st.s, enc, dec, emask, dmask), target, loss_mask, E2W)
        grads = [g.clone() for g in torch.autograd.grad(tot, leaves)]
        O.clip_grad_norm(grads, 3.0)
        with torch.no_grad():
            O.hf_adamw_step([p.data for p in leaves], grads, mo, vo, step=step, lr=lr)
        sums = eng.loss_and_grads(*_args(batch), train=True)
        eng.optimizer_step(lr=lr)
        assert abs(_loss(sums) - float(tot.detach())) / float(tot.detach()) < 2e-4, step
    torch.cuda.synchronize()
    sn = lora._site_names(m, st)
    worst, worst_k = 0.0, ''
    for s in st.sites:
        A, B = ad[sn[s.key] + '.weight']
        for k, got, want in ((s.key + '.A', s.A, A), (s.key + '.B', s.B, B)):
            r = _rel(got.detach(), want.detach())
            worst, worst_k = max((worst, worst_k), (r, k))
    po = dict(o.named_parameters())
    for k, p in m.named_parameters():
        if k.startswith('mask_lm.'):
            r = _rel(p.detach(), po[k].detach())
            worst, worst_k = max((worst, worst_k), (r, k))
    print('five adapter steps: worst parameter %.2e (%s)' % (worst, worst_k))
    assert worst < 2e-3, (worst, worst_k)
    # the backbone: every P32 element outside the head ranges is what it was
    keep = torch.ones_like(p_before, dtype=torch.bool)
    n_head = 0
    for name in ('head.w', 'head.b'):
        h = eng.slots[name]
        keep[h.off:h.off + h.numel] = False
        n_head += h.numel
        assert not torch.equal(eng.P32[h.off:h.off + h.numel], p_before[h.off:h.off + h.numel]), name        # the heads did train
    assert torch.equal(eng.P32[keep], p_before[keep])
    assert eng.opt_m is None and eng.opt_v is None
    assert st.optimizer_numel() == 2 * (st.n + n_head)
    assert eng.wgrad_launches == launches
    # and the counter does count: one plain step of the same engine without adapters launches the backbone's weight gradients
    eng.detach_lora()
    eng.loss_and_grads(*_args(_batch(shape, 1)), train=True)
    assert eng.wgrad_launches > launches


def test_thirty_bf16_steps_lower_the_loss():
    """Default targets, B = 0 at the start, one fixed batch: thirty bf16 steps end with a lower loss than they started with."""
    _need_gpu()
    m, eng = _engine(_lm('pack', 'bf16'))
    eng.attach_lora(_cfg(targets=('q', 'v', 'cq', 'cv')), seed=0)
    args = _args(_batch('pack', 304))
    losses = []
    for _ in range(30):
        losses.append(_loss(eng.loss_and_grads(*args, train=True)))
        assert eng._saved.get('pack') is not None and eng._saved.get('sub_layer') is not None       # packed rows, loss rows only in the last layer
        eng.optimizer_step(lr=1e-3)
    losses.append(_loss(eng.loss_and_grads(*args, train=False)))
    print('thirty bf16 adapter steps: loss %.4f -> %.4f' % (losses[0], losses[-1]))
    assert np.isfinite(losses).all() and losses[-1] < losses[0]


def test_packed_and_dense_steps_give_the_same_adapter_gradients():
    """bf16, rows packed (the last decoder layer's cq site runs on the loss rows only) against the same step dense (argmax_out): the loss and the norm
    of every adapter gradient. Each form lies within the bf16 engine's bounds of the oracle (loss 2e-3, gradient norm 2e-2: tests/test_model_gpu.py,
    BF16_LOSS / BF16_NORM), so the two lie within twice that of each other."""
    _need_gpu()
    m, eng = _engine(_lm('pack', 'bf16'))
    st = eng.attach_lora(_cfg(), seed=1)
    _randomize_adapters(st, 11)
    args = _args(_batch('pack', 310))
    l_packed = _loss(eng.loss_and_grads(*args, train=True))
    assert eng._saved.get('pack') is not None
    g_packed = st.G.clone()
    T = args[0].shape[0] * args[0].shape[1]
    l_dense = _loss(eng.loss_and_grads(*args, train=True, argmax_out=torch.empty(T, 8, dtype=torch.int16, device='cuda')))
    assert eng._saved.get('pack') is None
    e_loss = abs(l_packed - l_dense) / l_dense
    e_norm = abs(float(g_packed.double().norm()) - float(st.G.double().norm())) / float(st.G.double().norm())
    worst = max(abs(float(a.double().norm()) - float(b.double().norm())) / float(b.double().norm())
                for s in st.sites for a, b in ((g_packed[s.off_a:s.off_b], s.gA), (g_packed[s.off_b:s.off_b + s.N * st.r], s.gB)))
    print('lora bf16 packed against dense: loss %.2e, gradient norm %.2e, worst site %.2e' % (e_loss, e_norm, worst))
    assert e_loss < 4e-3 and e_norm < 4e-2 and worst < 4e-2, (e_loss, e_norm, worst)


def test_frozen_heads_leave_every_master_weight_alone():
    _need_gpu()
    m, eng = _engine(_lm('five', 'fp32'))
    st = eng.attach_lora(_cfg(), seed=2, train_heads=False)
    _randomize_adapters(st, 8)
    before, a_before = eng.P32.clone(), st.P.clone()
    eng.loss_and_grads(*_args(_batch('five', 305)), train=True)
    eng.optimizer_step(lr=1e-3)
    assert torch.equal(eng.P32, before) and not torch.equal(st.P, a_before)
    assert st.optimizer_numel() == 2 * st.n


# ---------------------------------------------------------------------------------------------------------------------- merging
def test_merge_folds_the_adapters_into_the_masters():
    """After merge_lora() the plain forward is within 1e-4 (_rel, fp32) of the adapter forward taken just before, and each merged weight within
    (r + 2) 2^-24 (|W| + s sum |B| |A|) of float64."""
    _need_gpu()
    m, eng = _engine(_lm('sweep', 'fp32'))
    st = eng.attach_lora(_cfg(rank=16, alpha=24), seed=1)
    _randomize_adapters(st, 9)
    args = _args(_batch('sweep', 306))
    _, logits_ad = _dense(eng, args)
    want = {}
    for s in st.sites:
        w = eng.wf[s.slot][s.row:s.row + s.N].detach().cpu().double()
        term, mag = R.merge_term(s.B, s.A, st.s)
        want[s.key] = (s.slot, s.row, s.N, w + term, R.bound(st.r, w.abs() + mag))
    eng.merge_lora()
    assert eng.lora is None
    _, logits_m = _dense(eng, args)
    assert _rel(logits_m, logits_ad) < 1e-4
    for key, (slot, row, N, ref, bnd) in want.items():
        err = (eng.wf[slot][row:row + N].detach().cpu().double() - ref).abs()
        assert bool((err <= bnd).all()), key


def test_adapter_file_round_trip_and_merged_state_dict(tmp_path):
    """save, then load into a fresh model built from the base state dict: torch.equal sums; a model loaded from merged_state_dict generates the
    tokens of the merged live model; the file holds no backbone tensor."""
    _need_gpu()
    from pianobart_amd import lora
    shape = 'five'
    m0 = _lm(shape, 'fp32')
    sd = {k: v.detach().clone() for k, v in m0.state_dict().items()}
    m, eng = _engine(m0)
    st = eng.attach_lora(_cfg(), seed=4)
    _randomize_adapters(st, 10)
    args = _args(_batch(shape, 307))
    for _ in range(2):
        eng.loss_and_grads(*args, train=True)
        eng.optimizer_step(lr=1e-3)
    sums = eng.loss_and_grads(*args, train=False).clone()
    path = str(tmp_path / 'a.lora.pt')
    lora.save(path, m)
    f = torch.load(path, map_location='cpu', weights_only=False)
    assert all(k.endswith('.lora_A') or k.endswith('.lora_B') or k.startswith('mask_lm.') for k in f['state_dict'])
    assert {k: tuple(v.shape) for k, v in f['state_dict'].items()} == lora.adapter_keys(m, st.cfg, train_heads=True)
    m2, eng2 = _engine(_lm(shape, 'fp32', sd=sd))
    st2 = lora.load(path, m2)
    assert torch.equal(eng2.loss_and_grads(*args, train=False), sums)
    assert eng2.step_count == eng.step_count == 2 and torch.equal(st2.m, st.m) and torch.equal(st2.head_v[0], st.head_v[0])
    # the resumed model takes the same third step
    for e in (eng, eng2):
        e.loss_and_grads(*args, train=True)
        e.optimizer_step(lr=1e-3)
    assert torch.equal(eng2.lora.P, eng.lora.P)
    merged = lora.merged_state_dict(m)
    assert sorted(merged) == sorted(sd)
    m3, eng3 = _engine(_lm(shape, 'fp32', sd=merged))
    eng.merge_lora()
    enc = _batch(shape, 308)[0][:1].cuda()
    emask = torch.ones(1, enc.shape[1], device='cuda')
    outs = []
    for mod in (m, m3):
        np.random.seed(5)
        outs.append(mod.eval()(enc, encoder_attention_mask=emask, generate=True))
    assert torch.equal(outs[0], outs[1])


# ---------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_name_what_was_wrong(tmp_path, monkeypatch):
    _need_gpu()
    from pianobart_amd import lora
    from pianobart_amd._lib import PBError
    m, eng = _engine(_lm('five', 'fp32'))
    args = _args(_batch('five', 309))
    for bad, word in ((dict(rank=2), 'rank'), (dict(rank=68), 'rank'), (dict(rank=10), 'multiple of 4')):
        with pytest.raises(PBError, match=word):
            eng.attach_lora(lora.LoraConfig(**bad))
    m96, eng96 = _engine(_lm('sweep', 'fp32'))
    with pytest.raises(PBError, match='d_model'):
        _small_d_model_engine().attach_lora(lora.LoraConfig(rank=64))          # d_model 32: refused before any device work
    with pytest.raises(PBError, match="unknown LoRA target 'wo'"):
        eng.attach_lora(lora.LoraConfig(targets=('q', 'wo')))
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(PBError, match='WORLD_SIZE'):
        eng.attach_lora(_cfg())
    monkeypatch.delenv('WORLD_SIZE')
    assert eng.lora is None
    eng.attach_lora(_cfg())
    with pytest.raises(PBError, match='second time'):
        eng.attach_lora(_cfg())
    with pytest.raises(PBError, match='micro'):
        eng.loss_and_grads(*args, train=True, micro=(0, 2))
    enc, dec, loss_mask, emask, dmask, target = [t.cuda() for t in _batch('five', 309)]
    with pytest.raises(PBError, match='autograd module path'):
        m(enc, dec, emask, dmask)
    with pytest.raises(PBError, match='autograd module path'):
        m.pianobart(enc, dec, emask, dmask)
    with torch.no_grad():
        m(enc, dec, emask, dmask)                                    # an inference forward sees the adapters without further work
    with pytest.raises(PBError, match=r'merge_lora\(\)'):
        m.eval()(enc[:1], encoder_attention_mask=emask[:1], generate=True)
    with pytest.raises(PBError, match=r'merge_lora\(\)'):
        m.generate_batch(enc, emask, seeds=[1, 2, 3])
    with pytest.raises(PBError, match=r'merge_lora\(\)'):
        eng._decode_plan(1, 48, [48], emask[:1], enc.device)
    # an adapter file from another model
    path = str(tmp_path / 'a.lora.pt')
    lora.save(path, m)
    with pytest.raises(PBError, match='d_model'):
        lora.load(path, m96)
    with pytest.raises(PBError, match='second time'):
        lora.load(path, m)
    eng.detach_lora()
    with pytest.raises(PBError, match='no LoRA adapters'):
        eng.merge_lora()


def _small_d_model_engine():
    """d_model 32 < rank 64."""
    from pianobart_amd.model import BartConfig, PianoBart, PianoBartLM
    kw = dict(_kw('five'), d_model=32, encoder_attention_heads=2, decoder_attention_heads=2)
    m = PianoBartLM(PianoBart(BartConfig(**kw), E2W, W2E, precision='fp32'))
    return m._get_engine()
