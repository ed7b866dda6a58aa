"""No GPU: tests/score_ref.py, the reference of tests/test_score_kernels_gpu.py, is right.

float64 logp against torch.log_softmax, entropy against -(p log p).sum(), rank against the target's position in a stable argsort of -x
(an independent statement of the tie rule), the crafted rows against what they must give, the out-of-range rule against a direct
count, seq_sums against a loop, and the float32 model's own figures on every layout and row family of the GPU suite.

Measured (the last test, pytest -s): the float32 model's largest figure in units of 2^-24 S per (output, family) over the six layouts:
  logp     random 1.82  uniform 0.63  plateau 0.19  zero_tie 1.16  spike 0.00  offset 1.58  ladder 0.66  outside 0.98
  entropy  random 1.97  uniform 0.63  plateau 0.19  zero_tie 1.51  spike 0.00  offset 1.92  ladder 0.49  outside 1.66
and with the kernel's named roundings (exp2, log2) at most 1.77 (logp) and 2.55 (entropy, random rows).
"""
import numpy as np
import pytest
import torch

from tests import score_ref as R


@pytest.fixture(scope='module')
def cases():
    return {name: R.make_case(sizes) for name, sizes in R.LAYOUTS.items()}


@pytest.fixture(scope='module')
def refs(cases):
    return {name: R.token_scores(c['x'].double(), c['target'], c['mask'], c['off']) for name, c in cases.items()}


def test_layouts_reach_every_branch(cases):
    for name, sizes in R.LAYOUTS.items():
        assert len(sizes) == 8 and all(1 <= n <= 1088 for n in sizes)
    assert max(R.LAYOUTS['narrow_edges']) == 320 and max(R.LAYOUTS['switch']) == 321 and R.LAYOUTS['switch'][1:] == R.LAYOUTS['narrow_edges'][1:]
    assert R.edge_classes(1) == [0] and R.edge_classes(2) == [0, 1] and R.edge_classes(65) == [0, 1, 62, 63, 64]
    assert R.edge_classes(129) == [0, 1, 62, 63, 64, 65, 126, 127, 128]
    for name, c in cases.items():
        fam, t, m = c['fam'], c['target'], c['mask']
        T = len(fam)
        assert fam[0] == fam[1 + (T - 3) // 2] == fam[-1] == 'masked' and fam.count('masked') == 3 and int((m == 0).sum()) == 3
        assert bool(torch.isnan(c['x'][m == 0]).all()) and bool((t[m == 0] == 32767).all()) and bool(torch.isfinite(c['x'][m != 0]).all())
        for i, n in enumerate(c['sizes']):
            # every (tk, tl) corner of the head is a target in every family block
            for f in R.FAMILIES[:-1]:
                rows = [r for r in range(T) if fam[r] == f]
                assert set(R.edge_classes(n)) <= set(int(v) for v in t[rows, i]), (name, f, i)
            out = set(int(v) for v in t[[r for r in range(T) if fam[r] == 'outside'], i])
            assert out == {-1, n, 32767, -32768}, (name, i)
        zt = c['x'][[r for r in range(T) if fam[r] == 'zero_tie']]
        assert bool((zt <= 0).all()) and bool(((zt == 0) & torch.signbit(zt)).any()) and bool(((zt == 0) & ~torch.signbit(zt)).any())


def test_float64_against_log_softmax_entropy_and_stable_argsort(cases, refs):
    for name, c in cases.items():
        r, x, off = refs[name], c['x'].double(), c['off']
        T = x.shape[0]
        for i, n in enumerate(c['sizes']):
            t = c['target'][:, i].long()
            ok = (c['mask'] != 0) & (t >= 0) & (t < n)
            seg = x[ok][:, off[i]:off[i + 1]]
            lsm = torch.log_softmax(seg, -1)
            want = lsm.gather(1, t[ok][:, None])[:, 0]
            assert float((r['logp'][ok, i] - want).abs().max()) < 1e-12 * 3e4, (name, i)      # offset rows: |x| = 3e4 inside log_softmax
            fam_ok = [c['fam'][k] for k in range(T) if ok[k]]
            small = torch.tensor([f != 'offset' for f in fam_ok])
            assert float((r['logp'][ok, i] - want)[small].abs().max()) < 1e-12, (name, i)
            p = lsm.exp()
            ent = -torch.where(p > 0, p * lsm, torch.zeros_like(p)).sum(-1)
            assert float((r['entropy'][ok, i] - ent)[small].abs().max()) < 1e-12, (name, i)
            order = np.argsort(-seg.numpy(), axis=1, kind='stable')
            pos = (order == t[ok].numpy()[:, None]).argmax(1)
            assert np.array_equal(r['rank'][ok, i].numpy(), pos), (name, i)


def test_crafted_rows_give_what_they_must(cases, refs):
    for name, c in cases.items():
        r, fam, t = refs[name], c['fam'], c['target'].long()
        rows = lambda f: torch.tensor([k for k in range(len(fam)) if fam[k] == f])
        assert bool(torch.isfinite(r['logp']).all()) and bool(torch.isfinite(r['entropy']).all())
        dead = c['mask'] == 0
        assert bool((r['logp'][dead] == 0).all()) and bool((r['entropy'][dead] == 0).all()) and bool((r['rank'][dead] == -1).all())
        assert bool((r['s_logp'][dead] == 0).all()) and bool((r['s_entropy'][dead] == 0).all())
        for i, n in enumerate(c['sizes']):
            u = rows('uniform')
            assert float((r['logp'][u, i] + np.log(n)).abs().max()) < 1e-12 and float((r['entropy'][u, i] - np.log(n)).abs().max()) < 1e-12
            assert torch.equal(r['rank'][u, i], t[u, i])
            s = rows('spike')
            assert bool((r['entropy'][s, i] >= 0).all()) and bool((r['entropy'][s, i] < 1e-60).all())
            on = i % 2 == 0 or n == 1
            assert float((r['logp'][s, i] - (0.0 if on else -160.0)).abs().max()) < 1e-12
            assert bool((r['rank'][s, i] == 0).all()) if on else bool((r['rank'][s, i] >= 1).all())
            pl = rows('plateau')
            below = sum(((t[pl, i] - d) >= 0).long() for d in (64, 1))
            assert torch.equal(r['rank'][pl, i], below)                 # the plateau members at a lower index, nothing else
            if n == 1:
                live = ~dead & (t[:, i] == 0)
                for k in ('logp', 'entropy', 'rank', 's_logp', 's_entropy'):
                    assert bool((r[k][live, i] == 0).all()), (name, k)
        live = ~dead
        assert bool((r['rank'][live] >= 0).all()) and bool((r['entropy'][live] >= 0).all())


def test_a_target_outside_its_head_scores_a_logit_of_zero(cases, refs):
    """rank = #(x > 0) + #(x == 0 and column < target): a target < 0 counts none of the zeros, a target >= n all of them; logp is
    0 - logsumexp."""
    seen = 0
    for name, c in cases.items():
        r, x, off = refs[name], c['x'].double().numpy(), c['off']
        for k in range(x.shape[0]):
            if c['mask'][k] == 0:
                continue
            for i, n in enumerate(c['sizes']):
                t = int(c['target'][k, i])
                if 0 <= t < n:
                    continue
                seg = x[k, off[i]:off[i + 1]]
                zeros, pos = int((seg == 0).sum()), int((seg > 0).sum())
                assert int(r['rank'][k, i]) == pos + (zeros if t >= n else 0), (name, k, i)
                lse = float(torch.logsumexp(torch.from_numpy(seg), 0))
                assert abs(float(r['logp'][k, i]) + lse) < 1e-12
                seen += zeros > 0
    assert seen > 100                                                   # the zeros are there: the two sides of the rule differ


def test_seq_sums_against_a_loop():
    g = torch.Generator().manual_seed(3)
    B, S = 3, 37
    lp, en = torch.randn(B * S, 8, generator=g, dtype=torch.float64), torch.randn(B * S, 8, generator=g, dtype=torch.float64)
    rk = torch.randint(0, 3, (B * S, 8), generator=g).to(torch.int16)
    m = torch.tensor([0.0, 1.0, 2.0, 0.5])[torch.randint(0, 4, (B, S), generator=g)].double()
    lp[(m.view(-1) == 0)] = float('nan')                                # a masked position adds nothing, whatever it holds
    en[(m.view(-1) == 0)] = float('inf')
    out, ab = R.seq_sums(lp, en, rk, m)
    want, wab = torch.zeros(B, 4, 8, dtype=torch.float64), torch.zeros(B, 4, 8, dtype=torch.float64)
    for b in range(B):
        for s in range(S):
            w = float(m[b, s])
            if w == 0:
                continue
            for h in range(8):
                terms = (w * lp[b * S + s, h], w * en[b * S + s, h], w * float(rk[b * S + s, h] == 0), w)
                for p, v in enumerate(terms):
                    want[b, p, h] += v
                    wab[b, p, h] += abs(v)
    assert torch.allclose(out, want, rtol=1e-13, atol=1e-13) and torch.allclose(ab, wab, rtol=1e-13, atol=1e-13)
    ch, ab_ch = R.seq_sums(lp, en, rk, m, chain=True)                   # the kernel's documented order: the same sums
    assert torch.allclose(ch, want, rtol=1e-13, atol=1e-13) and torch.equal(ab_ch, ab)
    ints = torch.randint(-8, 9, (B * S, 8), generator=g).float()
    m32 = m.float()
    assert torch.equal(R.seq_sums(ints, ints, rk, m32, chain=True)[0], R.seq_sums(ints, ints, rk, m32)[0])          # exact either way
    out2, _ = R.seq_sums(lp, None, None, m)
    assert torch.equal(out2[:, 0], out[:, 0]) and torch.equal(out2[:, 3], out[:, 3]) and bool((out2[:, 1:3] == 0).all())
    o0, a0 = R.seq_sums(lp[:0], en[:0], rk[:0], m[:, :0])
    assert o0.shape == (B, 4, 8) and bool((o0 == 0).all()) and bool((a0 == 0).all())


def test_float32_model_figures_are_finite(cases, refs):
    """The float32 model (the same code on float32 tensors) on every layout and row family: finite figures, printed; its rank equals the
    float64 rank (comparisons only). With the named roundings of the kernel (exp2, log2) the figures stay finite as well."""
    worst, worst_opt = {}, {}
    for name, c in cases.items():
        for opts, acc in (({}, worst), (dict(exp2=True, log2=True), worst_opt)):
            m = R.token_scores(c['x'], c['target'], c['mask'], c['off'], **opts)
            assert torch.equal(m['rank'], refs[name]['rank'])
            assert bool(torch.isfinite(m['logp']).all()) and bool(torch.isfinite(m['entropy']).all())
            for key, v in R.worst_by_family(c, m, refs[name]).items():
                assert np.isfinite(v), (name, key)
                acc[key] = max(acc.get(key, 0.0), v)
    for out in ('logp', 'entropy'):
        print('float32 model %-8s' % out, '  '.join('%s %.2f' % (f, worst[(out, f)]) for f in R.FAMILIES))
        print('  with exp2, log2    ', '  '.join('%s %.2f' % (f, worst_opt[(out, f)]) for f in R.FAMILIES))
    assert max(worst.values()) < 16                                     # a float32 evaluation of about ten roundings: units, not hundreds
