"""GPU: the dropout mask of every kernel that draws one is the Philox4x32-7 stream of csrc/pb_common.h (drop_mask4), bit for bit against
the host restatement tests/philox_ref.py: element 4 i + e of a site takes word e of counter (i, site, 0x5EED, 0) under the key (low, high
half of the seed). A kept element is one f32 multiply by 1 / (1 - p), so every comparison here is exact."""
import functools

import numpy as np
import pytest
import torch

from tests.philox_ref import drop_consts, drop_mask

pytestmark = pytest.mark.gpu

SEED = 0x12345679ABCDEF1                  # the high 32 bits are part of the key
SITES = (5, 0x7001)
BIG = 4 * 1048576                         # 4096 blocks x 256 threads x 4 elements: beyond it the grid-stride loops take a second trip
TOL = {torch.float32: 2e-5, torch.bfloat16: 2e-2}


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from pianobart_amd import ops as o
    return o


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@functools.lru_cache(maxsize=8)
def _ref_np(seed, site, p, n):
    return drop_mask(seed, site, p, n)


def ref_mask(seed, site, p, n):
    return torch.from_numpy(_ref_np(seed, site, p, n)).cuda()


def _randn(n, dt, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    return torch.randn(n, device='cuda', generator=g).to(dt)


# ---------------------------------------------------------------------------------------------------------------- pb_dropout
def _dropout_mask(ops, n, dt, seed, site, p):
    """What pb_dropout multiplies an all-ones tensor with."""
    y = torch.full((n,), float('nan'), device='cuda', dtype=dt)
    ops.dropout(torch.ones(n, device='cuda', dtype=dt), y, seed, site, p)
    return y.float()


@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('n', [4, 1028, BIG + 1200])
@pytest.mark.parametrize('p', [0.1, 0.5])
def test_dropout_is_the_philox_stream(ops, dt, n, p):
    x, dy = _randn(n, dt, n), _randn(n, dt, n + 1)
    for site in SITES:
        mask = ref_mask(SEED, site, p, n)
        y = torch.full((n,), float('nan'), device='cuda', dtype=dt); dx = torch.full_like(y, float('nan'))
        ops.dropout(x, y, SEED, site, p)
        ops.dropout(dy, dx, SEED, site, p)                           # the same call on the gradient is the backward
        assert torch.equal(y, (x.float() * mask).to(dt))
        assert torch.equal(dx, (dy.float() * mask).to(dt))
    y0 = torch.full((n,), float('nan'), device='cuda', dtype=dt)
    ops.dropout(x, y0, SEED, SITES[0], 0.0)
    assert torch.equal(y0, x)


# ---------------------------------------------------------------------------------------------------------------- pb_eltwise_* op 4
@pytest.mark.parametrize('n', [1, 3, 5, 1027, BIG + 1027])
@pytest.mark.parametrize('p', [0.1, 0.5])
def test_eltwise_dropout_forward_and_backward_share_the_mask(ops, n, p):
    """op 4 = dropout only, the backward called as heads._DropoutFn.backward calls it (dy also in the place of y); the ragged n % 4 tail
    (one thread, counter n / 4) and the strided loop draw the same bits in both directions."""
    x, dy = _randn(n, torch.float32, n), _randn(n, torch.float32, n + 1)
    for site in SITES:
        mask = ref_mask(SEED, site, p, n)
        y = torch.full((n,), float('nan'), device='cuda'); dx = torch.full((n,), float('nan'), device='cuda')
        ops.eltwise_fwd(4, x, None, y, SEED, site, p)
        ops.eltwise_bwd(4, dy, None, dy, dx, None, SEED, site, p)
        assert torch.equal(y, x * mask)
        assert torch.equal(dx, dy * mask)


# ---------------------------------------------------------------------------------------------------------------- LayerNorm kernels
def _row_ids(T, seed):
    """T increasing, gapped row numbers (a packed batch: the rows kept out of a padded one)."""
    gaps = np.random.default_rng(seed).integers(1, 5, size=T)
    gaps[0] = 2
    return torch.from_numpy(np.cumsum(gaps).astype(np.int32)).cuda()


def _add_ln_mask(ops, T, d, dt, seed, site, p, row_ids=None):
    """The mask pb_add_ln_fwd applies, recovered from res = 0, a = 1 and an identity LayerNorm: z = mask, y = (z - mean) * rstd."""
    ones = torch.ones(T, d, device='cuda', dtype=dt)
    y = torch.full((T, d), float('nan'), device='cuda', dtype=dt)
    mean = torch.empty(T, device='cuda'); rstd = torch.empty(T, device='cuda')
    ops.add_ln_fwd(torch.zeros_like(ones), ones, torch.ones(d, device='cuda'), torch.zeros(d, device='cuda'), y, mean, rstd, 1e-5, seed, site, p, row_ids=row_ids)
    z = y.float() / rstd[:, None] + mean[:, None]
    scale = float(drop_consts(p)[1])
    assert float(torch.minimum(z.abs(), (z - scale).abs()).max()) < 0.05 * scale          # every z is 0 or scale, up to the storage rounding of y
    return torch.where(z > 0.5 * scale, scale, 0.0).float()


@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('d', [64, 128, 768, 1024])
@pytest.mark.parametrize('p', [0.1, 0.5])
def test_add_ln_mask_is_the_philox_stream(ops, dt, d, p):
    T, site = 37, SITES[0]
    assert torch.equal(_add_ln_mask(ops, T, d, dt, SEED, site, p), ref_mask(SEED, site, p, T * d).reshape(T, d))
    rid = _row_ids(T, d)                                             # packed row r carries the bits of row row_ids[r] of the padded batch
    padded = ref_mask(SEED, site, p, (int(rid[-1]) + 1) * d).reshape(-1, d)
    assert torch.equal(_add_ln_mask(ops, T, d, dt, SEED, site, p, row_ids=rid), padded[rid.long()])


def _embed_inputs(ops, B, S, d, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    ids = torch.stack([torch.randint(0, n, (B * S,), device='cuda', generator=g) for n in ops.SEG_SIZES], dim=1)
    rn = lambda *s: torch.randn(*s, device='cuda', generator=g)
    return ids, rn(ops.VOCAB, d), rn(d), rn(S + 2, d), 1 + 0.2 * rn(d), 0.2 * rn(d)


@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('d', [128, 1024])
@pytest.mark.parametrize('p', [0.1, 0.5])
@pytest.mark.parametrize('packed', [False, True])
def test_embed_ln_mask_is_the_philox_stream(ops, dt, d, p, packed):
    """pb_embed_ln_fwd drops AFTER the LayerNorm: y_p = y_0 * mask."""
    B, S, site = 3, 13, SITES[1]
    ids, P, lb, pos, w, b = _embed_inputs(ops, B, S, d, d)
    mask = ref_mask(SEED, site, p, B * S * d).reshape(B * S, d)
    rid = None
    if packed:
        rid = torch.tensor([0, 2, 3, 12, 13, 14, 20, 27, 30, 31, 38], device='cuda', dtype=torch.int32)
        ids, mask = ids[rid.long()], mask[rid.long()]
    ids16 = ops.ids_to_i16(ids.contiguous())
    T = ids16.shape[0]
    ys = []
    for pp in (0.0, p):
        y = torch.full((T, d), float('nan'), device='cuda', dtype=dt)
        ops.embed_ln_fwd(ids16, P, lb, pos, w, b, y, torch.empty(T, device='cuda'), torch.empty(T, device='cuda'), S, 1e-5, SEED, site, pp, row_ids=rid)
        ys.append(y)
    y0, yp = ys
    assert torch.isfinite(y0).all() and float((y0 != 0).float().mean()) > 0.99
    if dt == torch.float32:
        assert torch.equal(yp, y0 * mask)
    else:
        assert torch.equal(yp == 0, (mask == 0) | (y0 == 0))         # exactly 0 where dropped, not 0 where kept
        if p == 0.5:
            assert torch.equal(yp.float(), y0.float() * mask)        # times 2 commutes with the bf16 rounding


# ---------------------------------------------------------------------------------------------------------------- what enters the key
@pytest.mark.parametrize('kind', ['dropout_f32', 'dropout_bf16', 'eltwise', 'add_ln', 'add_ln_packed'])
def test_site_and_both_seed_halves_enter_the_mask(ops, kind):
    p, T, d = 0.1, 37, 64
    n = {'dropout_f32': 1028, 'dropout_bf16': 1028, 'eltwise': 1027}.get(kind, T * d)
    rid = _row_ids(T, 1) if kind == 'add_ln_packed' else None

    def got(seed, site):
        if kind.startswith('dropout'):
            return _dropout_mask(ops, n, torch.float32 if kind == 'dropout_f32' else torch.bfloat16, seed, site, p)
        if kind == 'eltwise':
            y = torch.full((n,), float('nan'), device='cuda')
            ops.eltwise_fwd(4, torch.ones(n, device='cuda'), None, y, seed, site, p)
            return y
        return _add_ln_mask(ops, T, d, torch.float32, seed, site, p, row_ids=rid).reshape(-1)

    def want(seed, site):
        if rid is None:
            m = ref_mask(seed, site, p, n)
        else:
            m = ref_mask(seed, site, p, (int(rid[-1]) + 1) * d).reshape(-1, d)[rid.long()].reshape(-1)
        return m.to(torch.bfloat16).float() if kind == 'dropout_bf16' else m

    variants = [(SEED, SITES[0]), (SEED, SITES[1]), (SEED, SITES[0] + 1), (SEED ^ (1 << 32), SITES[0]), (SEED ^ (1 << 63), SITES[0]), (SEED ^ 1, SITES[0])]
    masks = [got(*v) for v in variants]
    for v, m in zip(variants, masks):
        assert torch.equal(m, want(*v)), v
    for i in range(len(masks)):
        for j in range(i):
            assert not torch.equal(masks[i], masks[j]), (variants[i], variants[j])


# ---------------------------------------------------------------------------------------------------------------- the backward kernels
@pytest.mark.parametrize('dt,d', [(torch.float32, 768), (torch.bfloat16, 1024)])
@pytest.mark.parametrize('packed', [False, True])
def test_add_ln_bwd_regenerates_the_reference_mask(ops, dt, d, packed):
    """pb_add_ln_fwd / pb_add_ln_bwd against float64 autograd of layer_norm(res + a * mask) with the mask from philox_ref (the
    comparison of test_kernels_gpu.test_add_ln_fwd_bwd, whose bounds these are)."""
    T, p, site = 37, 0.1, SITES[0]
    g = torch.Generator(device='cuda').manual_seed(d)
    rn = lambda *s: torch.randn(*s, device='cuda', generator=g)
    res, a, dy = rn(T, d).to(dt), rn(T, d).to(dt), rn(T, d).to(dt)
    w, b = 1 + 0.2 * rn(d), 0.2 * rn(d)
    rid = _row_ids(T, 2) if packed else None
    mask = ref_mask(SEED, site, p, T * d).reshape(T, d) if rid is None else ref_mask(SEED, site, p, (int(rid[-1]) + 1) * d).reshape(-1, d)[rid.long()]
    y = torch.empty(T, d, device='cuda', dtype=dt); mean = torch.empty(T, device='cuda'); rstd = torch.empty(T, device='cuda')
    ops.add_ln_fwd(res, a, w, b, y, mean, rstd, 1e-5, SEED, site, p, row_ids=rid)
    rd, ad, wd, bd = (t.double().requires_grad_(True) for t in (res, a, w, b))
    yr = torch.nn.functional.layer_norm(rd + ad * mask.double(), (d,), wd, bd, 1e-5)
    yr.backward(dy.double())
    assert _rel(y, yr) < TOL[dt]
    dres = torch.empty(T, d, device='cuda', dtype=dt); da = torch.empty_like(dres)
    dg, db, dba = (torch.zeros(d, device='cuda') for _ in range(3))
    partials = torch.empty(int(ops.LIB.query('pb_ln_partials_floats', d)), device='cuda')
    ops.add_ln_bwd(dy, res, a, w, mean, rstd, dres, da, dg, db, dba, partials, False, SEED, site, p, row_ids=rid)
    assert _rel(dres, rd.grad) < TOL[dt] * 2
    assert _rel(da, ad.grad) < TOL[dt] * 2
    assert bool((da[mask == 0] == 0).all())                          # a dropped element gets no gradient at all
    assert _rel(dg, wd.grad) < TOL[dt] * 2 and _rel(db, bd.grad) < TOL[dt] * 2
    assert _rel(dba, ad.grad.sum(0)) < TOL[dt] * 4


@pytest.mark.parametrize('dt,d', [(torch.float32, 128), (torch.bfloat16, 768)])
@pytest.mark.parametrize('packed', [False, True])
def test_embed_ln_bwd_regenerates_the_reference_mask(ops, dt, d, packed):
    """pb_embed_ln_fwd / pb_embed_ln_bwd with dropout on against float64 autograd of layer_norm(z) * mask, the mask from philox_ref
    (the comparison and bounds of test_kernels_gpu.test_embed_ln_fwd_bwd, which runs at p = 0)."""
    B, S, p, site = 3, 13, 0.1, SITES[1]
    ids, P, lb, pos, w, b = _embed_inputs(ops, B, S, d, d + 1)
    rows = torch.arange(B * S, device='cuda')
    rid = None
    if packed:
        rid = torch.tensor([0, 2, 3, 12, 13, 14, 20, 27, 30, 31, 38], device='cuda', dtype=torch.int32)
        rows = rid.long()
    ids = ids[rows].contiguous()
    mask = ref_mask(SEED, site, p, B * S * d).reshape(B * S, d)[rows]
    ids16 = ops.ids_to_i16(ids)
    T = ids.shape[0]
    y = torch.empty(T, d, device='cuda', dtype=dt); mean = torch.empty(T, device='cuda'); rstd = torch.empty(T, device='cuda')
    ops.embed_ln_fwd(ids16, P, lb, pos, w, b, y, mean, rstd, S, 1e-5, SEED, site, p, row_ids=rid)
    Pd, lbd, posd, wd, bd = (t.double().requires_grad_(True) for t in (P, lb, pos, w, b))
    off = torch.tensor(ops.SEG_OFF[:8], device='cuda')
    z = Pd[(ids + off).reshape(-1)].reshape(T, 8, d).sum(1) + lbd + posd[2 + rows % S]
    yr = torch.nn.functional.layer_norm(z, (d,), wd, bd, 1e-5) * mask.double()
    assert _rel(y, yr) < TOL[dt]
    g = torch.Generator(device='cuda').manual_seed(3)
    dy = torch.randn(T, d, device='cuda', generator=g).to(dt)
    yr.backward(dy.double())
    dP = torch.zeros_like(P); dpos = torch.zeros_like(pos)
    dlb, dg, db = (torch.zeros(d, device='cuda') for _ in range(3))
    partials = torch.empty(int(ops.LIB.query('pb_ln_partials_floats', d)), device='cuda')
    ops.embed_ln_bwd(dy, ids16, P, lb, pos, w, mean, rstd, dP, dpos, dlb, dg, db, partials, S, SEED, site, p, row_ids=rid)
    assert _rel(dP, Pd.grad) < 1e-4 and _rel(dpos, posd.grad) < 1e-4 and _rel(dlb, lbd.grad) < 1e-4
    assert _rel(dg, wd.grad) < 1e-4 and _rel(db, bd.grad) < 1e-4
