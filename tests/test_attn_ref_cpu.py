"""tests/attn_ref.py stands without a GPU: its float64 form equals float64 torch.autograd through softmax, its conventions for rows without a
visible key and keys no query sees hold, and every storage-model variant has a finite figure (printed with -s) at every input family the GPU
tests (tests/test_attention_kernels_gpu.py) use."""
import math

import pytest
import torch

from tests import attn_ref as A

CPU = torch.device('cpu')


def _inputs(B, H, Sq, Sk, hd, seed, amp=1.5):
    g = torch.Generator().manual_seed(seed)
    f = lambda *s: (torch.randn(*s, generator=g) * amp).to(torch.bfloat16).float()
    return f(B, H, Sq, hd), f(B, H, Sk, hd), f(B, H, Sk, hd), (f(B, H, Sq, hd) / amp), g


def _mask(kind, B, Sk, g):
    if kind == 'dense':
        return None
    km = (torch.rand(B, Sk, generator=g) > 0.25).float()
    km[0, 0] = 0
    km[1 % B, Sk // 2:] = 0
    if kind == 'dead_row':
        km[B - 1] = 0
    return km


def _autograd(q, k, v, dout, vis, scale):
    q, k, v = (x.double().requires_grad_(True) for x in (q, k, v))
    vis = vis.expand(q.shape[0], q.shape[1], q.shape[2], k.shape[2])
    s = (q @ k.transpose(-1, -2) * scale).masked_fill(~vis, float('-inf'))
    has = vis.any(-1, keepdim=True)
    p = torch.where(has, torch.softmax(torch.where(has, s, torch.zeros_like(s)), -1), torch.zeros_like(s))
    o = p @ v
    (o * dout.double()).sum().backward()
    lse = torch.where(has[..., 0], torch.logsumexp(torch.where(has, s, torch.zeros_like(s)), -1), torch.full_like(s[..., 0], float('inf')))
    return dict(o=o.detach(), lse=lse.detach(), dq=q.grad, dk=k.grad, dv=v.grad, delta=(o.detach() * dout.double()).sum(-1))


@pytest.mark.parametrize('kind', ['dense', 'masked', 'dead_row'])
@pytest.mark.parametrize('causal', [False, True])
@pytest.mark.parametrize('Sq,Sk', [(1, 1), (5, 5), (65, 63), (63, 65), (130, 257), (257, 1)])
def test_float64_form_equals_float64_autograd(kind, causal, Sq, Sk):
    B, H, hd = 3, 2, 32
    q, k, v, dout, g = _inputs(B, H, Sq, Sk, hd, 11 * Sq + Sk)
    vis = A.visible(B, Sq, Sk, CPU, _mask(kind, B, Sk, g), causal)
    scale = hd ** -0.5
    ref = _autograd(q, k, v, dout, vis, scale)
    got = A.attn(q.double(), k.double(), v.double(), dout.double(), vis, scale)
    for name, want in ref.items():
        have = got[name]
        inf = torch.isinf(want)
        assert torch.equal(torch.isinf(have), inf), name
        w0, h0 = torch.where(inf, torch.zeros_like(want), want), torch.where(inf, torch.zeros_like(have), have)
        err = float((h0 - w0).abs().max() / w0.abs().max().clamp_min(1e-300))
        print('%-6s Sq %3d Sk %3d %-8s causal %d   rel err %.3g' % (name, Sq, Sk, kind, causal, err))
        assert err <= 1e-12, (name, err)


@pytest.mark.parametrize('model', [None] + sorted(A.MODELS))
def test_rows_without_a_visible_key_and_keys_no_query_sees(model):
    """o = 0, lse = +inf, dq = 0 for a row without a visible key; dk = dv = 0 for a key no query sees: exactly, in the truth and in every model."""
    B, H, Sq, Sk, hd = 3, 2, 70, 90, 32
    q, k, v, dout, g = _inputs(B, H, Sq, Sk, hd, 5)
    km = (torch.rand(B, Sk, generator=g) > 0.3).float()
    km[0, :3] = 0                              # causal: queries 0..2 of batch 0 see nothing
    km[2] = 0                                  # a whole batch row without a visible key
    vis = A.visible(B, Sq, Sk, CPU, km, True)
    if model is None:
        r = A.attn(q.double(), k.double(), v.double(), dout.double(), vis, hd ** -0.5)
    else:
        r = A.attn(q, k, v, dout, vis, hd ** -0.5, **A.MODELS[model])
    dead_q = ~vis.any(-1).expand(B, H, Sq)
    dead_k = ~vis.any(-2).expand(B, H, Sk)
    assert bool(dead_q[0, :, :3].all()) and bool(dead_q[2].all()) and bool(dead_k[:, :, Sq:].all())      # causal, Sk > Sq: the keys beyond the last query
    assert bool((r['o'][dead_q] == 0).all()) and bool((r['dq'][dead_q] == 0).all()) and bool((r['delta'][dead_q] == 0).all())
    assert bool((r['lse'][dead_q] == float('inf')).all()) and bool(torch.isfinite(r['lse'][~dead_q]).all())
    assert bool((r['dk'][dead_k] == 0).all()) and bool((r['dv'][dead_k] == 0).all())
    assert bool((r['p'][~vis.expand_as(r['p'])] == 0).all())
    for name in ('o', 'dq', 'dk', 'dv', 'delta', 'p', 'dP', 'a'):
        assert bool(torch.isfinite(r[name]).all()), name


def _figures(model, q, k, v, dout, vis, scale):
    truth = A.attn(q.double(), k.double(), v.double(), dout.double(), vis, scale)
    S = A.scales(truth, q.double(), k.double(), v.double(), dout.double(), vis, scale)
    m = A.attn(q, k, v, dout, vis, scale, **A.MODELS[model])
    st = model != 'x3'
    figs = {n: A.figure(m[n], truth[n], S[n], st and n not in ('lse', 'delta')) for n in ('o', 'lse', 'delta', 'dq', 'dk', 'dv')}
    for n in ('dq', 'dk', 'dv'):
        figs['dbias_' + n[1]] = A.figure(A.colsum(m[n]), A.colsum(truth[n]), A.colsum(S[n]), False)
    return figs


@pytest.mark.parametrize('model', sorted(A.MODELS))
@pytest.mark.parametrize('causal', [False, True])
@pytest.mark.parametrize('hd,Sq,Sk', [(32, 63, 65), (64, 129, 193), (128, 65, 257), (64, 257, 1), (96, 1, 257)])
def test_model_figures_are_finite_masked_random_inputs(model, causal, hd, Sq, Sk):
    B, H = 3, 2
    q, k, v, dout, g = _inputs(B, H, Sq, Sk, hd, hd + Sq + Sk)
    if model == 'x3':
        q, k, v, dout = (x + 2.0 ** -12 * torch.randn(x.shape, generator=g) for x in (q, k, v, dout))       # f32 operands that use their low bits
    vis = A.visible(B, Sq, Sk, CPU, _mask('dead_row', B, Sk, g), causal)
    figs = _figures(model, q, k, v, dout, vis, hd ** -0.5)
    print('FIG %-9s hd %3d Sq %3d Sk %3d causal %d  ' % (model, hd, Sq, Sk, causal) + '  '.join('%s %.3g' % kv for kv in figs.items()))
    assert all(math.isfinite(x) for x in figs.values()), figs


@pytest.mark.parametrize('model', ['prescale', 'one_pass'])
@pytest.mark.parametrize('kind', A.LAZY_KINDS)
def test_model_figures_are_finite_lazy_maximum_inputs(model, kind):
    B, H, Sq, Sk, hd = 2, 2, 70, 513, 64
    g = torch.Generator().manual_seed(3)
    scale = hd ** -0.5
    q, k = (x.to(torch.bfloat16).float() for x in A.lazy_inputs(kind, B, H, Sq, Sk, hd, scale, g, CPU))
    v = (torch.randn(B, H, Sk, hd, generator=g) * 1.5).to(torch.bfloat16).float()
    dout = torch.randn(B, H, Sq, hd, generator=g).to(torch.bfloat16).float()
    for causal in (False, True):
        vis = A.visible(B, Sq, Sk, CPU, None, causal)
        figs = _figures(model, q, k, v, dout, vis, scale)
        print('FIG %-9s lazy %-5s causal %d  ' % (model, kind, causal) + '  '.join('%s %.3g' % kv for kv in figs.items()))
        assert all(math.isfinite(x) for x in figs.values()), figs
    if kind in ('rise', 'fall', 'edge'):                               # the profile is what its name says: tile means of a row's log2 scores
        s2 = (q.double() @ k.double().transpose(-1, -2) * scale * A.LOG2E)[0, 0, 0]
        means = torch.stack([s2[i:i + 64].mean() for i in range(0, 512, 64)])
        step = means[1:] - means[:-1]
        if kind == 'rise':
            assert bool((step > 8).all()), step
        elif kind == 'fall':
            assert bool((step < -8).all()), step
        else:
            assert bool((step.abs() > 6).all()) and bool((step.abs() > 8).any()) and bool((step.abs() < 8).any()), step
