"""GPU: every kernel of csrc/pb_heads.hip (the fine-tune heads: pb_eltwise_*, pb_softmax_dim1_*, pb_ce_rows, pb_gather_rows*) called
directly through the C ABI against a plain float64 PyTorch reference of the same op -- ragged n % 4 tails, the grid-stride loops behind
the 4096-block caps, dropout in the same launch (mask from tests/philox_ref.py), ties / class counts around the wave width / row weights
/ out-of-range targets of the row loss, the id clamp of the gathers -- and the autograd Functions of heads.py on non-contiguous and
3-D inputs. f32 results: max difference over max reference magnitude < 2e-5 (test_kernels_gpu.TOL) unless a bound is named."""
import numpy as np
import pytest
import torch

from tests.philox_ref import drop_mask

pytestmark = pytest.mark.gpu

SEED, SITE = 0x12345679ABCDEF1, 0x7001
BIG = 4 * 1048576                         # 4096 blocks x 256 threads x 4 elements
PLANT = [0.0, -0.0, 1e-8, -1e-8, 20.0, -20.0, 88.0, -88.0]      # relu's kink, saturated tanh / sigmoid, the edge of exp's f32 range
ACT = {1: torch.tanh, 2: torch.relu, 3: torch.sigmoid}


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from pianobart_amd import ops as o
    return o


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _gen(seed):
    return torch.Generator(device='cuda').manual_seed(seed)


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float('nan'), device='cuda', dtype=dtype)


def _planted(n, g, shift=0):
    x = 4 * torch.randn(n, device='cuda', generator=g)
    k = min(n, len(PLANT))
    x[:k] = torch.tensor((PLANT[shift:] + PLANT[:shift])[:k], device='cuda')
    return x


# ---------------------------------------------------------------------------------------------------------------- pb_eltwise_*
@pytest.mark.parametrize('op', [1, 2, 3, 5])
@pytest.mark.parametrize('p', [0.0, 0.1])
@pytest.mark.parametrize('n', [1, 2, 3, 4, 7, 1027, BIG + 1027])
def test_eltwise_fwd_bwd(ops, op, p, n):
    """tanh / relu / sigmoid / product, alone and with dropout in the same launch. The backward takes its derivative from the forward's
    PRE-dropout output (the kernel's own y of the p = 0 launch, not a recomputed one); relu'(0) = 0 as in torch."""
    g = _gen(op * 100 + n % 97)
    x, dy = _planted(n, g), torch.randn(n, device='cuda', generator=g)
    x2 = _planted(n, g, shift=3) if op == 5 else None
    mask = torch.from_numpy(drop_mask(SEED, SITE, p, n)).cuda() if p > 0 else torch.ones(n, device='cuda')
    xd = x.double().requires_grad_(True)
    x2d = x2.double().requires_grad_(True) if op == 5 else None
    pre = xd * x2d if op == 5 else ACT[op](xd)
    (pre * mask.double()).backward(dy.double())
    y0 = _nan(n)
    ops.eltwise_fwd(op, x, x2, y0, SEED, SITE, 0.0)
    assert _rel(y0, pre.detach()) < 2e-5
    if p > 0:
        yp = _nan(n)
        ops.eltwise_fwd(op, x, x2, yp, SEED, SITE, p)
        assert torch.equal(yp, y0 * mask)                            # one f32 multiply on top of the same activation
        assert _rel(yp, pre.detach() * mask.double()) < 2e-5
    dx = _nan(n); dx2 = _nan(n) if op == 5 else None
    ops.eltwise_bwd(op, x if op == 5 else y0, x2, dy, dx, dx2, SEED, SITE, p)
    assert _rel(dx, xd.grad) < 2e-5
    if op == 5:
        assert _rel(dx2, x2d.grad) < 2e-5
    if op == 2:
        assert bool((dx[x <= 0] == 0).all())
    if p > 0:
        assert bool((dx[mask == 0] == 0).all())


def test_eltwise_argument_checks(ops):
    from pianobart_amd._lib import PBError
    n = 8
    x = torch.ones(n, device='cuda'); out = torch.full((n,), 7.0, device='cuda'); out2 = torch.full((n,), 7.0, device='cuda')
    for op, x2 in ((0, None), (6, None), (0, x), (6, x), (5, None)):
        with pytest.raises(PBError, match='pb_eltwise_fwd: op=%d' % op):
            ops.eltwise_fwd(op, x, x2, out, 0, 0, 0.0)
        with pytest.raises(PBError, match='pb_eltwise_bwd: op=%d' % op):
            ops.eltwise_bwd(op, x, x2, x, out, out2 if x2 is not None else None, 0, 0, 0.0)
    with pytest.raises(PBError, match='pb_eltwise_bwd: op=5'):      # the product's backward writes two gradients
        ops.eltwise_bwd(5, x, x, x, out, None, 0, 0, 0.0)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((out2 == 7.0).all())   # refused before any launch


# ---------------------------------------------------------------------------------------------------------------- pb_softmax_dim1_*
@pytest.mark.parametrize('B,S,R,shift', [(1, 1, 1, 0.0), (2, 63, 4, 0.0), (3, 64, 4, 0.0), (2, 65, 5, 0.0), (2, 200, 4, 0.0), (1, 1024, 1, 0.0),
                                         (2, 200, 4, 80.0), (2, 200, 4, -80.0)])
def test_softmax_dim1_fwd_bwd(ops, B, S, R, shift):
    """Softmax over the SEQUENCE axis of (B, S, R): one wave per (b, r) column striding S in steps of 64. Bounds of test_softmax_fwd_bwd."""
    g = _gen(S * 7 + R)
    x = 3 * torch.randn(B, S, R, device='cuda', generator=g) + shift
    dy = torch.randn(B, S, R, device='cuda', generator=g)
    xd = x.double().requires_grad_(True)
    ref = torch.softmax(xd, dim=1)
    ref.backward(dy.double())
    y = _nan(B, S, R)
    ops.softmax_dim1_fwd(x, y)
    assert float((y.double() - ref).abs().max()) < 1e-6
    assert float((y.double().sum(1) - 1).abs().max()) < 1e-6
    dx = _nan(B, S, R)
    ops.softmax_dim1_bwd(y, dy, dx)
    assert float((dx.double() - xd.grad).abs().max()) < 1e-5


# ---------------------------------------------------------------------------------------------------------------- pb_ce_rows
def _ce_case(rows, C, g):
    """logits, targets and the rows with something planted, counted from the LAST row so that row 0 stays an ordinary one:
    targets -100 and C (no loss, no gradient), ties (the first maximum wins: inside one lane's strided columns, across lanes, in the
    first and the last two columns), an all-equal row, a row whose maximum is 1e4."""
    logits = 2 * torch.randn(rows, C, device='cuda', generator=g)
    target = torch.randint(0, C, (rows,), device='cuda', generator=g).to(torch.int32)
    plants = [('t', -100), ('t', C)]
    if C >= 65:
        plants.append(('tie', (C - 65, C - 1)))                      # the same lane, 64 columns apart
    if C >= 71:
        plants.append(('tie', (3, 70)))                              # lanes 3 and 6
    plants += [('eq', None), ('big', C // 2)]
    if C >= 2:
        plants += [('tie', (0, 1)), ('tie', (C - 2, C - 1))]
    if C >= 70:
        plants += [('tie', (5, 69)), ('tie+t', (5, 69))]
    bad = []
    for k, (kind, arg) in enumerate(plants):
        r = rows - 1 - k
        if r < 1:
            break
        if kind in ('t', 'tie+t'):
            target[r] = arg if kind == 't' else -100
            bad.append(r)
        if kind in ('tie', 'tie+t'):
            logits[r, arg[0]] = logits[r, arg[1]] = 12.0
        elif kind == 'eq':
            logits[r] = 0.75
        elif kind == 'big':
            logits[r, arg] = 1e4
    return logits, target, bad


@pytest.mark.parametrize('rows', [1, 3, 5, 258])
@pytest.mark.parametrize('C', [1, 2, 4, 63, 64, 65, 130, 1024])
def test_ce_rows(ops, rows, C):
    """Per-row cross entropy, its gradient scaled by coef[0] * weight[row], and the first-maximum argmax, in every form of the optional
    arguments. A target outside [0, C) is a row without loss: loss 0, an all-zero gradient row (nn.CrossEntropyLoss's ignore_index),
    argmax still written."""
    g = _gen(rows * 31 + C)
    logits, target, bad = _ce_case(rows, C, g)
    weight = 0.5 + torch.rand(rows, device='cuda', generator=g)
    coef = torch.tensor([0.37], device='cuda')
    valid = (target >= 0) & (target < C)
    ld = logits.double()
    lsm = torch.log_softmax(ld, -1)
    tc = target.long().clamp(0, C - 1)
    loss_ref = torch.where(valid, -lsm.gather(1, tc[:, None])[:, 0], torch.zeros_like(lsm[:, 0]))
    onehot = torch.zeros_like(ld).scatter_(1, tc[:, None], 1.0)
    base = (torch.softmax(ld, -1) - onehot) * valid[:, None].double()
    am_ref = torch.from_numpy(np.argmax(logits.cpu().numpy(), -1)).cuda()
    assert not bad or not bool(valid[bad].any())
    for form in range(16):
        use_w, use_c, use_d, use_a = (bool(form >> i & 1) for i in range(4))
        loss = _nan(rows)
        dl = _nan(rows, C) if use_d else None
        am = torch.full((rows,), -7, device='cuda', dtype=torch.int32) if use_a else None
        ops.ce_rows(logits, target, weight if use_w else None, coef if use_c else None, loss, dl, am)
        err = (loss.double() - loss_ref).abs()
        assert bool((err < 1e-5 * loss_ref.abs().clamp_min(1.0)).all()), (form, float(err.max()))
        assert bool((loss[~valid] == 0).all())
        if use_d:
            want = base * (0.37 if use_c else 1.0) * (weight.double()[:, None] if use_w else 1.0)
            assert torch.isfinite(dl).all() and _rel(dl, want) < 1e-5, (form, _rel(dl, want))
            assert bool((dl[~valid] == 0).all()), (form, float(dl[~valid].abs().max()))
        if use_a:
            assert torch.equal(am.long(), am_ref), form


# ---------------------------------------------------------------------------------------------------------------- pb_gather_rows*
@pytest.mark.parametrize('T,d,nrows', [(1, 4, 1), (37, 260, 5), (1000, 768, 4), (300, 1024, 129)])
@pytest.mark.parametrize('bias', [False, True])
def test_gather_rows_fwd_bwd(ops, T, d, nrows, bias):
    g = _gen(T + d + nrows)
    table = torch.randn(nrows, d, device='cuda', generator=g)
    b = torch.randn(d, device='cuda', generator=g) if bias else None
    ids = torch.randint(0, nrows, (T,), device='cuda', generator=g).to(torch.int32)
    unnamed = nrows // 2 if nrows > 2 else None                      # a table row that no id names
    if unnamed is not None:
        ids[ids == unnamed] = 0
    ids[0] = -3                                                      # clamped to row 0
    if T > 1:
        ids[-1] = nrows + 2                                          # clamped to the last row
    cl = ids.long().clamp(0, nrows - 1)
    out = _nan(T, d)
    ops.gather_rows(table, ids, b, out)
    assert torch.equal(out, table[cl] + b if bias else table[cl])
    dout = torch.randn(T, d, device='cuda', generator=g)
    runs = []
    for _ in range(2):
        dt_ = _nan(nrows, d)
        ops.gather_rows_bwd(dout, ids, dt_)
        runs.append(dt_)
    ref = torch.zeros(nrows, d, device='cuda', dtype=torch.double).index_add_(0, cl, dout.double())
    assert torch.equal(runs[0], runs[1])
    assert _rel(runs[0], ref) < 2e-5
    if unnamed is not None:
        assert bool((runs[0][unnamed] == 0).all())
    if T > 1:
        assert float(ref[0].abs().max()) > 0 and float(ref[nrows - 1].abs().max()) > 0


def test_gather_rows_bwd_without_tokens_writes_zeros(ops):
    dt_ = _nan(5, 260)
    ops.gather_rows_bwd(torch.empty(0, 260, device='cuda'), torch.empty(0, device='cuda', dtype=torch.int32), dt_)
    assert bool((dt_ == 0).all())


# ---------------------------------------------------------------------------------------------------------------- heads.py glue
def _nc(*shape, g, scale=1.0):
    """A non-contiguous tensor of this shape (the last two axes of its storage are swapped)."""
    t = scale * torch.randn(*shape[:-2], shape[-1], shape[-2], device='cuda', generator=g)
    t = t.transpose(-1, -2)
    assert not t.is_contiguous()
    return t


def _vs_float64(fn, ref_fn, inputs, gw):
    """fn on f32 leaves vs ref_fn on float64 leaves, outputs and every input gradient under the (non-contiguous) output weights gw."""
    leaves = [t.detach().requires_grad_(True) for t in inputs]         # detach() keeps the strides
    assert all(not l.is_contiguous() for l in leaves)
    dleaves = [t.double().requires_grad_(True) for t in inputs]
    y = fn(*leaves); yr = ref_fn(*dleaves)
    assert y.shape == yr.shape and _rel(y.detach(), yr.detach()) < 2e-5
    assert not gw.is_contiguous()
    y.backward(gw)
    yr.backward(gw.double())
    for l, dl in zip(leaves, dleaves):
        assert l.grad.shape == l.shape and _rel(l.grad, dl.grad) < 2e-5


@pytest.mark.parametrize('name', ['tanh', 'relu', 'sigmoid'])
def test_heads_act_function(ops, name):
    from pianobart_amd import heads
    g = _gen(1)
    _vs_float64(lambda x: heads.act(x, name), getattr(torch, name), [_nc(3, 5, 7, g=g, scale=2.0)], _nc(3, 5, 7, g=g))


def test_heads_mul_function(ops):
    from pianobart_amd import heads
    g = _gen(2)
    _vs_float64(heads.mul, lambda a, b: a * b, [_nc(3, 5, 7, g=g), _nc(3, 5, 7, g=g)], _nc(3, 5, 7, g=g))


def test_heads_softmax_dim1_function(ops):
    from pianobart_amd import heads
    g = _gen(3)
    _vs_float64(heads.softmax_dim1, lambda x: torch.softmax(x, dim=1), [_nc(2, 70, 4, g=g, scale=3.0)], _nc(2, 70, 4, g=g))


def test_heads_dropout_function(ops):
    """The forward's mask is the stream of site 0x7001 over the CONTIGUOUS element order, and the backward (dy passed in the place
    of y) applies the same mask to a non-contiguous dy."""
    from pianobart_amd import heads
    g = _gen(4)
    x = _nc(3, 5, 7, g=g).requires_grad_(True)
    gw = _nc(3, 5, 7, g=g)
    mask = torch.from_numpy(drop_mask(SEED, 0x7001, 0.1, x.numel())).cuda().reshape(3, 5, 7)
    y = heads._DropoutFn.apply(x, 0.1, SEED)
    assert torch.equal(y, x.detach() * mask)
    y.backward(gw)
    assert torch.equal(x.grad, gw * mask)
    assert heads.dropout(x, 0.1, False) is x and heads.dropout(x, 0.0, True) is x
    z = heads.dropout(x.detach(), 0.5, True)                          # the public wrapper draws its own seed: about half survives, scaled by 2
    kept = z != 0                                                     # 105 draws of Bernoulli(0.5): 0.25 .. 0.75 is +- 5 standard deviations
    assert torch.equal(z[kept], 2 * x.detach()[kept]) and 0.25 < float(kept.float().mean()) < 0.75


def test_heads_cross_entropy_function(ops):
    from pianobart_amd import heads
    g = _gen(5)
    B, S, C = 3, 9, 70
    logits = _nc(B, S, C, g=g, scale=2.0)
    target = torch.randint(0, C, (B, S), device='cuda', generator=g)
    target[1, 4] = -100                                               # nn.CrossEntropyLoss's ignore_index: no loss, no gradient
    gw = torch.randn(S, B, device='cuda', generator=g).t()            # per-row weights, non-contiguous
    ref = lambda x: torch.nn.functional.cross_entropy(x.reshape(-1, C), target.reshape(-1), reduction='none').reshape(B, S)
    leaf = logits.detach().requires_grad_(True); dleaf = logits.double().requires_grad_(True)
    loss = heads.cross_entropy_rows(leaf, target); lr = ref(dleaf)
    assert loss.shape == (B, S) and float(loss[1, 4]) == 0.0
    assert bool(((loss.double() - lr).abs() < 1e-5 * lr.abs().clamp_min(1.0)).all())
    loss.backward(gw)
    lr.backward(gw.double())
    assert _rel(leaf.grad, dleaf.grad) < 1e-5
    assert bool((leaf.grad[1, 4] == 0).all())


def test_heads_gather_function(ops):
    from pianobart_amd import heads
    g = _gen(6)
    n, d, B, S = 6, 260, 3, 11
    table = torch.randn(n, 2 * d, device='cuda', generator=g)[:, ::2]
    bias = torch.randn(2 * d, device='cuda', generator=g)[::2]
    ids = torch.randint(0, n, (S, B), device='cuda', generator=g).t()
    gw = _nc(B, S, d, g=g)
    assert not table.is_contiguous() and not bias.is_contiguous() and not ids.is_contiguous()
    _vs_float64(lambda t, b: heads.gather_rows(t, ids, b), lambda t, b: t[ids] + b, [table, bias], gw)
    t2 = table.clone().requires_grad_(True)
    out = heads.gather_rows(t2, ids)                                  # without bias
    assert torch.equal(out, table[ids])
    out.sum().backward()
    assert torch.equal(t2.grad, torch.bincount(ids.reshape(-1), minlength=n).float()[:, None].expand(n, d))
