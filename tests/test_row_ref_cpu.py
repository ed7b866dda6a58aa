"""CPU: the float64 references of tests/row_ref.py against float64 torch.autograd of layer_norm, softmax and cross_entropy (1e-12), so
that tests/test_row_kernels_gpu.py compares the kernels with references that are established without a GPU."""
import numpy as np
import pytest
import torch

from tests import row_ref as R
from tests.philox_ref import drop_mask

F = torch.nn.functional
TOL = 1e-12


def _close(a, b):
    return float((a - b).abs().max()) <= TOL * max(1.0, float(b.abs().max()))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize('T,d', [(1, 4), (5, 12), (9, 260)])
def test_add_ln_reference(T, d):
    g = _gen(d)
    res, a, dy = (torch.randn(T, d, generator=g, dtype=torch.float64) for _ in range(3))
    mask = (torch.rand(T, d, generator=g) > 0.1).double() / 0.9
    w = 1 + 0.2 * torch.randn(d, generator=g, dtype=torch.float64)
    b = 0.2 * torch.randn(d, generator=g, dtype=torch.float64)
    leaves = [t.clone().requires_grad_(True) for t in (res, a, w, b)]
    yr = F.layer_norm(leaves[0] + leaves[1] * mask, (d,), leaves[2], leaves[3], 1e-5)
    yr.backward(dy)
    y, mean, rstd = R.add_ln_fwd(res, a, mask, w, b, 1e-5)
    z = res + a * mask
    assert _close(y, yr.detach()) and _close(mean, z.mean(-1)) and _close(rstd, (z.var(-1, unbiased=False) + 1e-5).rsqrt())
    r = R.add_ln_bwd(dy, res, a, mask, w, mean, rstd)
    assert _close(r['dres'], leaves[0].grad) and _close(r['da'], leaves[1].grad)
    assert _close(r['t_dgamma'].sum(0), leaves[2].grad) and _close(r['t_dbeta'].sum(0), leaves[3].grad)
    assert _close(r['t_dbias'].sum(0), leaves[1].grad.sum(0))
    assert bool((r['dres'].abs().amax(-1) <= r['scale'] * (1 + 1e-12)).all())          # the row scale bounds the row


@pytest.mark.parametrize('p', [0.0, 0.1])
def test_embed_ln_reference(p):
    g = _gen(3)
    B, S, d, sizes = 3, 5, 12, [9, 7, 8, 11, 7, 7, 10, 13]
    seg_off = [0] + list(np.cumsum(sizes))
    T = B * S
    ids = torch.stack([torch.randint(0, n, (T,), generator=g) for n in sizes], 1)
    ids[0] = 0
    ids[1] = torch.tensor(sizes) - 1
    P = torch.randn(seg_off[8], d, generator=g, dtype=torch.float64)
    lb = torch.randn(d, generator=g, dtype=torch.float64)
    pos = torch.randn(S + 2, d, generator=g, dtype=torch.float64)
    w = 1 + 0.2 * torch.randn(d, generator=g, dtype=torch.float64)
    b = 0.2 * torch.randn(d, generator=g, dtype=torch.float64)
    dy = torch.randn(T, d, generator=g, dtype=torch.float64)
    mask = (torch.rand(T, d, generator=g) >= p).double() / (1 - p)
    pos_idx = torch.arange(T) % S
    Pl, lbl, posl, wl, bl = (t.clone().requires_grad_(True) for t in (P, lb, pos, w, b))
    z = lbl + posl[2:2 + S].repeat(B, 1)
    for i in range(8):
        z = z + Pl[seg_off[i] + ids[:, i]]
    yr = F.layer_norm(z, (d,), wl, bl, 1e-5) * mask
    yr.backward(dy)
    y, mean, rstd = R.embed_ln_fwd(ids, P, seg_off, lb, pos, pos_idx, w, b, 1e-5, mask)
    assert _close(y, yr.detach())
    r = R.embed_ln_bwd(dy, ids, P, seg_off, lb, pos, pos_idx, w, mean, rstd, mask)
    assert _close(r['dP'], Pl.grad) and _close(r['dpos'], posl.grad) and _close(r['t_dbias'].sum(0), lbl.grad)
    assert _close(r['t_dgamma'].sum(0), wl.grad) and _close(r['t_dbeta'].sum(0), bl.grad)
    assert bool((r['sP'][:, None] * (1 + 1e-12) >= r['dP'].abs()).all()) and bool((r['spos'][:, None] * (1 + 1e-12) >= r['dpos'].abs()).all())


@pytest.mark.parametrize('causal', [False, True])
@pytest.mark.parametrize('Sq,Sk', [(1, 1), (5, 7), (7, 5)])
@pytest.mark.parametrize('masked', [False, True])
def test_softmax_reference(causal, Sq, Sk, masked):
    g = _gen(Sq * 10 + Sk)
    B, H = 2, 2
    scores = (3 * torch.randn(B, H, Sq, Sk, generator=g, dtype=torch.float64)).requires_grad_(True)
    km = None
    if masked:
        km = (torch.rand(B, Sk, generator=g) > 0.3).float()
        km[1] = 0                                               # batch 1: no visible key
        km[0, 0] = 0                                            # causal query 0 of batch 0: its only candidate is masked
    vis = R.softmax_visible(B, H, Sq, Sk, km, causal, scores.device)
    s = (scores * 0.25).masked_fill(~vis, float('-inf'))
    ref = torch.where(vis.any(-1, keepdim=True), torch.softmax(s, -1), torch.zeros_like(s))
    dP = torch.randn(B, H, Sq, Sk, generator=g, dtype=torch.float64)
    live = vis.any(-1, keepdim=True).expand_as(vis)
    # autograd of the rows that see a key (a row of -inf has no gradient to speak of: the kernel defines it as 0)
    (torch.softmax(s.masked_fill(~live, 0.0), -1) * dP * live).sum().backward()
    P = R.softmax_fwd(scores.detach(), km, 0.25, causal)
    assert _close(P, torch.nan_to_num(ref.detach(), nan=0.0))
    assert bool((P[~vis] == 0).all())
    assert _close(R.softmax_bwd(dP, P, 1.0) * 0.25, scores.grad)
    assert _close(R.softmax_bwd(dP, P, 0.25), scores.grad)


def test_softmax_reference_extreme_scores():
    s = torch.tensor([80.0, -80.0, 80.0, 0.0], dtype=torch.float64).reshape(1, 1, 1, 4)
    P = R.softmax_fwd(s, None, 1.0, False)
    assert bool(torch.isfinite(P).all()) and abs(float(P.sum()) - 1) < 1e-15 and float(P[0, 0, 0, 0]) == float(P[0, 0, 0, 2])


def test_ce_reference():
    g = _gen(5)
    sizes = [9, 7, 70, 11, 7, 130, 10, 13]
    seg_off = [0] + [int(v) for v in np.cumsum(sizes)]
    T = 11
    logits = 2 * torch.randn(T, seg_off[8], generator=g, dtype=torch.float64)
    logits[3, 0] = logits[3, 8] = 50.0                          # ties: first / last class, and across the 64-class boundary
    logits[4, seg_off[5] + 63] = logits[4, seg_off[5] + 64] = logits[4, seg_off[5] + 128] = 50.0
    target = torch.stack([torch.randint(0, n, (T,), generator=g) for n in sizes], 1)
    target[0] = 0
    target[1] = torch.tensor(sizes) - 1
    m = (torch.rand(T, 8, generator=g) < 0.5).double()
    m[:, 6] = 0                                                 # a head without a loss position: coef = inf
    w = torch.tensor([3.0, 1, 4, 1, 5, 9, 2, 6], dtype=torch.float64)
    coef = R.loss_coef(m.sum(0), w)
    assert torch.isinf(coef[6])
    r = R.ce_fwd_bwd(logits, target, m, seg_off, coef)
    ld = logits.clone().requires_grad_(True)
    total = 0
    for i in range(8):
        seg = ld[:, seg_off[i]:seg_off[i + 1]]
        ce = F.cross_entropy(seg, target[:, i], reduction='none')
        assert _close(r['ce'][:, i], ce.detach())
        assert np.array_equal(r['argmax'][:, i].numpy(), np.argmax(seg.detach().numpy(), -1))
        if i != 6:
            total = total + (ce * m[:, i]).sum() / m[:, i].sum() * w[i]
    (total / w.sum()).backward()
    live = [c for i in range(8) if i != 6 for c in range(seg_off[i], seg_off[i + 1])]
    assert _close(r['dlogits'][:, live], ld.grad[:, live])
    assert bool(torch.isnan(r['dlogits'][:, seg_off[6]:seg_off[7]]).all())         # inf * 0
    assert int(r['argmax'][3, 0]) == 0 and int(r['argmax'][4, 5]) == 63
    assert _close(r['terms'].sum(1)[1], m.sum(0))
    # a target outside its head scores a logit of 0
    t2 = target.clone(); t2[2, 0] = 9
    r2 = R.ce_fwd_bwd(logits, t2, m, seg_off)
    assert _close(r2['ce'][2, 0], torch.logsumexp(logits[2, :9], 0))


def test_adamw_reference():
    """Against torch.optim.Adam-style moments written out per element, and the two places where HF-AdamW differs from torch.optim.AdamW:
    eps is added to sqrt(v) before the bias correction, and the decay comes after the update."""
    g = _gen(6)
    n = 7
    p, gr = torch.randn(n, generator=g, dtype=torch.float64), torch.randn(n, generator=g, dtype=torch.float64)
    m, v = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    lr, b1, b2, eps, wd = 1e-3, 0.9, 0.999, 1e-6, 0.01
    pp, mm, vv = p.clone(), m.clone(), v.clone()
    for step in (1, 2, 3):
        pp, mm, vv = R.adamw_step(pp, gr, mm, vv, torch.tensor(0.5, dtype=torch.float64), lr, b1, b2, eps, wd, step)
    q = p.clone()
    em, ev = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for step in (1, 2, 3):
        for j in range(n):
            gj = float(gr[j]) * 0.5
            em[j] = b1 * float(em[j]) + (1 - b1) * gj
            ev[j] = b2 * float(ev[j]) + (1 - b2) * gj * gj
            upd = lr * (1 - b2 ** step) ** 0.5 / (1 - b1 ** step) * float(em[j]) / (float(ev[j]) ** 0.5 + eps)
            q[j] = (float(q[j]) - upd) * (1 - lr * wd)
    assert _close(pp, q) and _close(mm, em) and _close(vv, ev)
    assert float(R.clip_coef(torch.tensor(16.0, dtype=torch.float64), 1.0, 0.5)) == pytest.approx(0.5 * 1.0 / (2.0 + 1e-6), rel=1e-15)
    assert float(R.clip_coef(torch.tensor(1.0, dtype=torch.float64), 3.0, 1.0)) == 1.0


def test_drop_mask_rows_is_the_flat_stream():
    d, T = 12, 9
    flat = torch.from_numpy(drop_mask(77, 3, 0.1, T * d)).reshape(T, d)
    assert torch.equal(R.drop_mask_rows(77, 3, 0.1, np.arange(T), d), flat)
    rows = np.array([0, 4, 8])
    assert torch.equal(R.drop_mask_rows(77, 3, 0.1, rows, d), flat[rows])
    assert torch.equal(R.drop_mask_rows(77, 3, 0.0, rows, d), torch.ones(3, d))
