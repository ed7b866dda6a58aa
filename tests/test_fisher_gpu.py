"""GPU: Fisher merging (csrc/pb_fisher.hip, merge.fisher_weights, python -m pianobart_amd.fisher, model_merge --method fisher_merging).

  * pb_fisher_rows against float64 autograd of sqrt(softmax).detach() * log_softmax, with test_ce_rows' bounds (the same reductions plus
    one square root per class): 1e-5 relative on the values, 1e-5 of the largest gradient on the gradient; masked rows exactly 0.
  * pb_fisher_accum / pb_fisher_finish / pb_fisher_merge against tests/fisher_ref.py bit for bit: one correctly rounded float32 operation
    each, in the same order; the recorded results of the reference (tests/golden/g16_fisher.npz) directly, with the recorded norms.
  * pb_fisher_norm against float32(sqrt(float64 numpy sum)) to 1 ulp; two runs give equal bytes.
  * merge.fisher_weights on the tiny fine-tune models against the oracle's classifiers in float64 autograd running the same loop.
  * the two command lines end to end.
Sizes: 1 (one thread), 3 (scalar tail only), 4, 5, 255 (vector body edge), 1027 (several workgroups, odd), 2^20 + 5 (the grid-stride loop);
every vector starts 0 .. 3 elements past a 16-byte boundary."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from tests import fisher_ref as R
from tests.test_fisher_cpu import GOLDEN, bits, golden_cases

gpu = pytest.mark.gpu
NS = [1, 3, 4, 5, 255, 1027, 2 ** 20 + 5]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _at(a, off):
    """a on the device, starting `off` elements past a 16-byte boundary."""
    buf = torch.zeros(a.size + 8, dtype=torch.float32, device='cuda')
    v = buf[off:off + a.size]
    v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    assert (v.data_ptr() % 16) // 4 == off
    return v


# ---- pb_fisher_rows -------------------------------------------------------------------------------------------------------------------
def _rows_case(rows, C, v, g):
    """Row i is random ((i + v) % 3 == 0), all-equal (1) or has one logit 1e4 above the rest (2: every other p underflows to 0);
    its weight is 0 where (i + v) % 4 == 3."""
    logits = torch.randn(rows, C, generator=g) * 3.0
    for i in range(rows):
        if (i + v) % 3 == 1:
            logits[i] = float(logits[i, 0])
        elif (i + v) % 3 == 2:
            logits[i, (i * 5) % C] += 1e4
    weight = 0.5 + torch.rand(rows, generator=g)
    weight[[(i + v) % 4 == 3 for i in range(rows)]] = 0.0
    return logits, weight


def _rows_reference(logits, weight):
    z = logits.double().requires_grad_(True)
    e = (torch.sqrt(torch.softmax(z, -1)).detach() * torch.log_softmax(z, -1)).sum(-1)
    (e * weight.double()).sum().backward()
    return e.detach(), z.grad


@gpu
@pytest.mark.parametrize('C', [1, 2, 4, 7, 63, 64, 65, 130])
def test_fisher_rows(C):
    _need_gpu()
    from pianobart_amd import ops
    for rows in (1, 3, 4, 5, 9):
        for v in range(4):
            g = torch.Generator().manual_seed(rows * 131 + C * 7 + v)
            logits, weight = _rows_case(rows, C, v, g)
            e_ref, d_ref = _rows_reference(logits, weight)
            e1_ref, d1_ref = _rows_reference(logits, torch.ones(rows))
            assert torch.isfinite(e_ref).all() and torch.isfinite(d_ref).all()
            lg, wg = logits.cuda(), weight.cuda()
            nan = lambda *s: torch.full(s, float('nan'), device='cuda')
            for use_w, use_d in ((False, False), (False, True), (True, True)):
                e, d = nan(rows), nan(rows, C) if use_d else None
                ops.fisher_rows(lg, wg if use_w else None, e, d)
                err = (e.double().cpu() - e_ref).abs()
                assert bool((err < 1e-5 * e_ref.abs().clamp_min(1.0)).all()), (rows, v, float(err.max()))
                if use_d:
                    want = d_ref if use_w else d1_ref
                    assert torch.isfinite(d).all()
                    if float(want.abs().max()) > 1e-12:
                        assert _rel(d, want) < 1e-5, (rows, v, use_w, _rel(d, want))
                    else:
                        # the exact gradient of the whole call is 0 (all-equal and one-hot rows only: sqrt(p_j) = p_j S there) and float64's own
                        # value is its rounding noise: the kernel's is held to 1e-5 of the terms whose difference it is, |w| sqrt(p_j) <= |w|
                        assert float(d.abs().max()) <= 1e-5 * float(weight.max() if use_w else 1.0), (rows, v, use_w, float(d.abs().max()))
                    if use_w:
                        assert bool((d[wg == 0] == 0).all())


@gpu
def test_fisher_expectation_rows_autograd():
    """(B, C), and (B, S, C) with a loss mask: values and the gradient that reaches the logits, against float64 autograd."""
    _need_gpu()
    from pianobart_amd import heads
    g = torch.Generator().manual_seed(5)
    for shape, masked in (((5, 8), False), ((3, 9, 7), True)):
        logits = torch.randn(*shape, generator=g) * 2.0
        mask = (torch.rand(*shape[:-1], generator=g) < 0.6).float() if masked else None
        scale = torch.randn(*shape[:-1], generator=g)                      # an upstream gradient that differs per row
        z = logits.double().requires_grad_(True)
        e_ref = (torch.sqrt(torch.softmax(z, -1)).detach() * torch.log_softmax(z, -1)).sum(-1) * (mask.double() if masked else 1.0)
        (e_ref * scale.double()).sum().backward()
        x = logits.cuda().requires_grad_(True)
        e = heads.fisher_expectation_rows(x, mask.cuda() if masked else None)
        assert e.shape == shape[:-1]
        (e * scale.cuda()).sum().backward()
        err = (e.detach().double().cpu() - e_ref.detach()).abs()
        assert bool((err < 1e-5 * e_ref.detach().abs().clamp_min(1.0)).all())
        assert _rel(x.grad, z.grad) < 1e-5
        if masked:
            off = (mask == 0)
            assert bool(off.any()) and bool((e.detach().cpu()[off] == 0).all()) and bool((x.grad.cpu()[off] == 0).all())


# ---- accumulate, finish, norm, merge ------------------------------------------------------------------------------------------------------
def _fisher_like(n, rng, m=0):
    f = (rng.standard_normal(n).astype(np.float32) * np.float32(1e-3)) ** 2
    f[rng.random(n) < 0.05] = 0.0
    return (f * np.float32(1 + m)).astype(np.float32)


@gpu
@pytest.mark.parametrize('n', NS)
def test_accum_and_finish_equal_the_restatement(n):
    _need_gpu()
    from pianobart_amd import ops
    rng = np.random.default_rng(n)
    for off_f in range(4):
        for off_g in ((off_f, (off_f + 1) % 4) if n > 5 else range(4)):
            F0 = _fisher_like(n, rng)
            gs = [(rng.standard_normal(n) * 10.0 ** rng.integers(-4, 2, n)).astype(np.float32) for _ in range(3)]
            F, want = _at(F0, off_f), F0
            guard = F.data_ptr()
            for gv in gs:
                ops.fisher_accum(F, _at(gv, off_g))
                want = R.accumulate(want, gv)
            assert F.data_ptr() == guard and np.array_equal(bits(F.cpu().numpy()), bits(want)), (off_f, off_g)
            flags = torch.zeros(1, dtype=torch.int32, device='cuda')
            ops.fisher_finish(F, 12, flags)
            assert np.array_equal(bits(F.cpu().numpy()), bits(R.finish(want, 12))) and int(flags.item()) == 0, (off_f, off_g)
    bad = _fisher_like(n, rng)
    bad[n // 2] = np.inf
    flags = torch.zeros(1, dtype=torch.int32, device='cuda')
    ops.fisher_finish(_at(bad, 1), 7, flags)
    assert int(flags.item()) == 1


@gpu
@pytest.mark.parametrize('n', NS)
def test_accum_and_finish_leave_their_neighbours_alone(n):
    _need_gpu()
    from pianobart_amd import ops
    rng = np.random.default_rng(n + 1)
    buf = torch.full((n + 8,), 7.25, device='cuda')
    for off in range(4):
        F = buf[off:off + n]
        F.zero_()
        ops.fisher_accum(F, _at(rng.standard_normal(n).astype(np.float32), off))
        ops.fisher_finish(F, 3, torch.zeros(1, dtype=torch.int32, device='cuda'))
        assert bool((buf[:off] == 7.25).all()) and bool((buf[off + n:] == 7.25).all())
        buf.fill_(7.25)


@gpu
@pytest.mark.parametrize('n', NS)
def test_norm_is_the_float64_norm_and_reproducible(n):
    _need_gpu()
    from pianobart_amd import ops
    rng = np.random.default_rng(n + 2)
    F = _fisher_like(n, rng) + np.float32(1e-9)
    want = R.norm64(F)
    ws = ops.fisher_norm_ws('cuda')
    outs = []
    for off in (0, 0, 1, 2, 3):                                             # the order of the additions depends on n alone: not on the alignment
        out = torch.full((1,), float('nan'), device='cuda')
        ops.fisher_norm(_at(F, off), ws, out)
        outs.append(out.cpu().numpy())
    assert all(np.array_equal(bits(o), bits(outs[0])) for o in outs)
    assert abs(int(bits(outs[0])[0]) - int(bits(np.array([want]))[0])) <= 1, (outs[0], want)


@gpu
@pytest.mark.parametrize('N', [2, 3, 8])
@pytest.mark.parametrize('n', NS)
def test_merge_equals_the_restatement(n, N):
    _need_gpu()
    from pianobart_amd import ops
    rng = np.random.default_rng(n * 11 + N)
    ws = [(rng.standard_normal(n) * 0.1).astype(np.float32) for _ in range(N)]
    fs = [_fisher_like(n, rng, m) for m in range(N)]
    dead = rng.random(n) < 0.03
    for f in fs:
        f[dead] = 0.0                                                       # F = 0 in every model: the denominator is N c minimal
    norms = np.array([R.norm64(f) for f in fs], dtype=np.float32)
    given = [0.3, 1.7, 0.9, 0.4, 1.1, 0.6, 2.0, 0.8][:N]
    for kw in ({}, dict(normalize_fisher_weight=False), dict(fisher_scaling_coefficients=given), dict(minimal_fisher_weight=1e-3)):
        want = R.merge(ws, fs, norms=norms, **kw)
        coef = R.coefficients(N, norms=norms, **kw)
        minimal = np.float32(kw.get('minimal_fisher_weight', 1e-6))
        for off in range(4):
            others = (off, (off + 1) % 4) if n > 5 else range(4)
            for off_in in others:                                           # off_in != off: the inputs reach no common 16-byte boundary (scalar throughout)
                out = _at(np.full(n, np.nan, dtype=np.float32), off)
                ops.fisher_merge(ops.fisher_desc([_at(w, off_in) for w in ws], [_at(f, off_in) for f in fs], out, coef, minimal))
                got = out.cpu().numpy()
                assert np.array_equal(bits(got), bits(want)), (kw, off, off_in, int((bits(got) != bits(want)).sum()))
    assert np.isfinite(want).all()


@gpu
@pytest.mark.parametrize('N', [3, 8])
def test_merge_flat_equals_the_reference_golden(N):
    """merge_flat on the recorded models and Fisher weights with the recorded norms: the reference's outputs, bit for bit. With the
    device's own norm: within the bound tests/test_fisher_cpu.py derives (2 eps times the spread of the models, 2 ulp), eps = eps_c plus
    the ulp test_norm_is_the_float64_norm_and_reproducible allows the device's norm."""
    _need_gpu()
    from pianobart_amd import merge as M
    from tests.test_fisher_cpu import _eps_c
    z = np.load(GOLDEN)
    shapes = {str(k): tuple(int(v) for v in sh if v) for k, sh in zip(z['names'], z['shapes'])}
    segs = M.segment_table(shapes)
    W, F = z['ft%d' % N], z['F%d' % N]
    dW, dF = [torch.from_numpy(w.copy()).cuda() for w in W], [torch.from_numpy(f.copy()).cuda() for f in F]
    for case, kw in golden_cases(z, N):
        want = z['out/%s/%d' % (case, N)]
        plan = M.MergePlan(N, method='fisher_merging', fisher_weights=[{}] * N, fisher_norms=list(z['norm%d' % N]), **kw)
        got = M.merge_flat(plan, dW[0], dW, segs, dF).cpu().numpy()
        assert np.array_equal(bits(got), bits(want)), (case, int((bits(got) != bits(want)).sum()))
        plan = M.MergePlan(N, method='fisher_merging', fisher_weights=[{}] * N, **kw)
        got = M.merge_flat(plan, dW[0], dW, segs, dF).cpu().numpy()
        eps = _eps_c(z) + 2.0 ** -23                                        # the device's norm is within 1 ulp (2^-23, relative) of the float64 norm
        bound = 2 * eps * (W.max(axis=0).astype(np.float64) - W.min(axis=0)) + 2 * np.spacing(np.abs(want)).astype(np.float64)
        assert (np.abs(got.astype(np.float64) - want) <= bound).all(), case


# ---- the pass ---------------------------------------------------------------------------------------------------------------------------
N_EX, BATCH = 10, 4
_ORACLE = {}


def _data(tag):
    from tests.golden_util import synth_octuple_batch
    from tests.test_finetune_heads import S
    X = synth_octuple_batch(N_EX, S, seed=3)[5].numpy().astype(np.int64)
    rng = np.random.default_rng(1)
    y = rng.integers(0, 8, size=(N_EX,)) if tag == 'seq' else rng.integers(0, 7, size=(N_EX, S))
    return X, y


def _batches(X, y):
    return [(torch.from_numpy(X[i:i + BATCH]), torch.from_numpy(y[i:i + BATCH])) for i in range(0, N_EX, BATCH)]


def _oracle_fisher(tag):
    """The reference's loop (merging_methods.py:201-249) on the oracle's classifier in float64; token logits summed over non-pad positions."""
    if tag in _ORACLE:
        return _ORACLE[tag]
    from oracle import pianobart_oracle as O
    from tests.test_finetune_heads import _build
    m = _build(O, O.BartConfig, O.PianoBart, tag).double()
    pad = m.pianobart.bar_pad_word
    X, y = _data(tag)
    total, computed = {}, 0
    for x, yb in _batches(X, y):
        if computed >= N_EX:
            break
        attn = (x[:, :, 0] != pad).double()
        if tag == 'seq':
            logits = m(input_ids_encoder=x, encoder_attention_mask=attn)
            w = torch.ones(x.shape[0], dtype=torch.float64)
        else:                                                               # velocity: labels shifted right, 7 = the pad label (finetune.py:190-196)
            y_shift = torch.zeros_like(yb) + 7
            y_shift[:, 1:] = yb[:, :-1]
            attn_shift = torch.zeros_like(attn)
            attn_shift[:, 1:] = attn[:, :-1]
            attn_shift[:, 0] = attn[:, 0]
            logits = m(input_ids_encoder=x, input_ids_decoder=y_shift, encoder_attention_mask=attn, decoder_attention_mask=attn_shift)
            w = attn
        e = ((torch.sqrt(torch.softmax(logits, -1)).detach() * torch.log_softmax(logits, -1)).sum(-1) * w).sum()
        m.zero_grad()
        e.backward()
        for k, p in m.named_parameters():
            if p.grad is not None:
                total[k] = total.get(k, 0) + p.grad.detach() ** 2
        computed += BATCH
    assert computed == 12
    _ORACLE[tag] = {k: v / computed for k, v in total.items()}
    return _ORACLE[tag]


@gpu
@pytest.mark.parametrize('precision,tol_grad', [('fp32', 2e-3), ('bf16x3', 2e-3), ('bf16', 2e-1)])
@pytest.mark.parametrize('tag', ['seq', 'tok8'])
def test_fisher_weights_match_the_oracle(tag, precision, tol_grad):
    """F is a sum of squares of gradients that test_heads_match_reference_golden already holds to tol_grad (largest error over largest
    value, per tensor): (g + dg)^2 - g^2 = 2 g dg + dg^2, so F is held to 2 tol_grad + tol_grad^2 in the same measure. The key biases'
    gradient is 0 in exact arithmetic (a softmax does not see a shift of all its scores): no relative measure there, their F is held to
    the same fraction of the largest F of any tensor."""
    _need_gpu()
    from pianobart_amd import merge as MG, model as M
    from tests.test_finetune_heads import _build
    ref = _oracle_fisher(tag)
    m = _build(M, M.BartConfig, M.PianoBart, tag, precision=precision).cuda()
    for x in m.modules():                                                   # the pass itself must switch dropout off and put it back
        if isinstance(x, torch.nn.Dropout):
            x.p = 0.1
    m.eval()
    eng = m.pianobart._get_engine()
    eng.bind(torch.device('cuda', torch.cuda.current_device()))
    eng.p_drop = 0.1
    before = eng.P32.clone()
    heads_before = {k: p.detach().clone() for k, p in m.named_parameters() if not k.startswith('pianobart.')}
    X, y = _data(tag)
    F, computed = MG.fisher_pass(m, _batches(X, y), N_EX, BATCH, tag == 'seq', 'cuda')
    assert computed == 12
    assert torch.equal(before, eng.P32) and all(torch.equal(v, dict(m.named_parameters())[k].detach()) for k, v in heads_before.items())
    assert eng.p_drop == 0.1 and not m.training and all(x.p == 0.1 for x in m.modules() if isinstance(x, torch.nn.Dropout))
    assert all(p.grad is None for p in m.parameters())
    own = m.pianobart.state_dict(keep_vars=True)
    held = {id(p) for p in eng.params}
    assert len(F) >= len(eng.params) and all(k in own and id(own[k]) in held for k in F)
    assert not any(k.startswith(('classifier', 'attention')) or 'decoder_emb' in k for k in F)
    bound = 2 * tol_grad + tol_grad ** 2
    top = max(float(v.abs().max()) for k, v in ref.items() if k.startswith('pianobart.'))
    checked = 0
    for k, want in ref.items():
        name = k[len('pianobart.'):]
        if not k.startswith('pianobart.') or name not in F:
            continue
        got = F[name].detach().double().cpu()
        assert got.shape == want.shape and torch.isfinite(got).all() and bool((got >= 0).all()), name
        if name.endswith('k_proj.bias'):
            assert float(got.max()) <= bound * top, (name, float(got.max()), top)
            continue
        r = float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))
        print('%s %s %-60s %.3g' % (tag, precision, name, r))
        assert r < bound, (name, r)
        checked += 1
    assert checked > 40


# ---- the command lines ----------------------------------------------------------------------------------------------------------------------
@gpu
def test_fisher_and_model_merge_command_lines(tmp_path, capsys):
    _need_gpu()
    import pickle
    from pianobart_amd._lib import PBError
    from pianobart_amd.fisher import fisher
    from pianobart_amd.merge import merge_state_dicts
    from pianobart_amd.model import BartConfig, PianoBart, SequenceClassification
    from pianobart_amd.model_merge import model_merge
    from tests.golden_util import load_vocab, randomize_params
    from tests.test_finetune_heads import _write_finetune_sets
    e2w, w2e = load_vocab()
    pickle.dump((e2w, w2e), open(tmp_path / 'dict.pkl', 'wb'))
    root = str(tmp_path / 'data')
    os.makedirs(root)
    _write_finetune_sets(root, 'Pianist8', True)                           # 4 training examples of length 64
    shape = dict(max_seq_len=64, hs=64, layers=1, ffn_dims=128, heads=4)
    cfg = BartConfig(max_position_embeddings=64, d_model=64, encoder_layers=1, decoder_layers=1, encoder_ffn_dim=128, decoder_ffn_dim=128,
                     encoder_attention_heads=4, decoder_attention_heads=4)
    pre = PianoBart(cfg, e2w, w2e)
    randomize_params(pre, 5)
    torch.save({'state_dict': pre.state_dict()}, str(tmp_path / 'pre.ckpt'))
    g = torch.Generator().manual_seed(6)
    fts = []
    for i in range(2):
        m = SequenceClassification(copy.deepcopy(pre), 8, 64)
        randomize_params(m.attention, 7 + i)
        randomize_params(m.classifier, 9 + i)
        with torch.no_grad():
            for q in m.pianobart.parameters():
                q.add_(torch.randn(q.shape, generator=g) * 0.01)
        torch.save({'state_dict': m.state_dict(), 'epoch': 1}, str(tmp_path / ('ft%d.ckpt' % i)))
        fts.append(m)
    flags = [x for k, v in shape.items() for x in ('--' + k, str(v))] + ['--dict_file', str(tmp_path / 'dict.pkl')]
    for i in range(2):
        fisher(flags + ['--ckpt', str(tmp_path / ('ft%d.ckpt' % i)), '--task', 'composer', '--dataset', 'Pianist8', '--dataroot', root, '--num_examples', '3',
                        '--batch_size', '2', '--precision', 'fp32', '--output', str(tmp_path / ('ft%d.fisher.pt' % i))])
    files = [torch.load(str(tmp_path / ('ft%d.fisher.pt' % i)), weights_only=False) for i in range(2)]
    assert all(set(f) == {'fisher', 'num_computed', 'task', 'precision'} and f['num_computed'] == 4 and f['task'] == 'composer' and f['precision'] == 'fp32'
               for f in files)
    assert all(v.dtype == torch.float32 and v.device.type == 'cpu' and bool((v >= 0).all()) for f in files for v in f['fisher'].values())
    assert any(bool((v > 0).any()) for v in files[0]['fisher'].values())
    out = str(tmp_path / 'merged.ckpt')
    mflags = flags + ['--pretrain_ckpt', str(tmp_path / 'pre.ckpt'), '--model_path', '%s,%s' % (tmp_path / 'ft0.ckpt', tmp_path / 'ft1.ckpt'), '--output_path', out]
    model_merge(mflags + ['--method', 'fisher_merging', '--fisher', '%s,%s' % (tmp_path / 'ft0.fisher.pt', tmp_path / 'ft1.fisher.pt')])
    said = capsys.readouterr().out
    assert 'Fisher weights of' in said and 'fisher_merging of 2 models' in said
    merged = torch.load(out, map_location='cpu', weights_only=False)['state_dict']
    sds = [f.pianobart.state_dict() for f in fts]
    want = merge_state_dicts(pre.state_dict(), sds, method='fisher_merging', fisher_weights=[f['fisher'] for f in files])
    assert list(merged) == list(pre.state_dict())
    for k in want:
        assert merged[k].numpy().tobytes() == want[k].numpy().tobytes(), k
    PianoBart(cfg, e2w, w2e).load_state_dict(merged, strict=True)
    average = merge_state_dicts(pre.state_dict(), sds, method='average_merging')
    assert any(not torch.equal(merged[k], average[k]) for k in merged)
    lo, hi = torch.minimum(sds[0]['encoder_linear.weight'], sds[1]['encoder_linear.weight']), torch.maximum(sds[0]['encoder_linear.weight'], sds[1]['encoder_linear.weight'])
    w = merged['encoder_linear.weight']
    assert bool(((w >= lo - 1e-6) & (w <= hi + 1e-6)).all())              # a weighted mean with positive weights lies between the models
    with pytest.raises(PBError, match='fisher_merging'):
        model_merge(mflags + ['--method', 'fisher_merging'])
