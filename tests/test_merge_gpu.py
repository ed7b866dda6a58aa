"""GPU: the merge kernels of csrc/pb_merge.hip against tests/merge_ref.py, bit for bit.

  * pb_merge_kth_abs against np.sort: exact (integer counts over bit patterns).
  * pb_merge_apply / pb_merge_sign_tally through merge.merge_flat against the float32 restatement: bit for bit. Every operation is one
    correctly rounded float32 operation in both, in the same order; the restatement itself equals the reference's recorded results
    (tests/test_merge_cpu.py), and so must the kernels on the same fixture.
  * the random mask against the host words: bit for bit; its drop count at n = 2^20, rate 0.8 within 6 binomial standard deviations,
    n p +- 6 sqrt(n p (1 - p)) = 838 861 +- 2 458.
Sizes: 1 (one thread), 3 (scalar tail only), 255 / 256 / 257 (vector body edges), 4 099 (several workgroups, odd), 2^20 + 5 (the grid
stride loop). Segment tables cut the vectors at odd offsets, so per-tensor calls start off a 16-byte boundary."""
import numpy as np
import pytest
import torch

from tests import merge_ref as R
from tests.test_merge_cpu import bits, golden_cases, load_golden

gpu = pytest.mark.gpu
NS = [1, 3, 255, 256, 257, 4099, 2 ** 20 + 5]
BIG = NS[-1]
_CACHE = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _segs(n):
    """A segment table over n elements with odd cuts (a flat vector of several tensors)."""
    from pianobart_amd.merge import Segment
    cuts = sorted({c for c in (0, 1, 6, 131, 1030, 4097, 70001, 600003) if c < n} | {n})
    return [Segment('t%02d' % i, a, b - a, (b - a,)) for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:]))]


# ---- k-th smallest magnitude ----------------------------------------------------------------------------------------------------------
KINDS = ['normal', 'equal', 'zeros', 'pairs', 'denormal', 'top24']


def _values(kind, n, rng):
    if kind == 'normal':
        return (rng.standard_normal(n) * 0.02).astype(np.float32)
    if kind == 'equal':
        return np.full(n, 0.375, dtype=np.float32)
    if kind == 'zeros':
        x = rng.standard_normal(n).astype(np.float32)
        x[::2] = 0.0
        x[::4] = -0.0
        return x
    if kind == 'pairs':
        v = rng.standard_normal(n // 2 + 1).astype(np.float32)
        return np.stack([v, -v], 1).reshape(-1)[:n].copy()
    sign = (rng.integers(0, 2, n).astype(np.uint32) << np.uint32(31))
    if kind == 'denormal':
        return (rng.integers(1, 1 << 23, n).astype(np.uint32) | sign).view(np.float32)
    assert kind == 'top24'                                  # magnitudes that differ in their last 8 bits only: the fourth pass decides
    return (np.uint32(0x3C123400) | rng.integers(0, 256, n).astype(np.uint32) | sign).view(np.float32)


@gpu
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n', NS)
def test_kth_abs_equals_sort(n, kind):
    _need_gpu()
    from pianobart_amd import ops
    rng = np.random.default_rng(n * 7 + KINDS.index(kind))
    v = _values(kind, n, rng)
    pick = rng.integers(0, 2, n).astype(bool)               # x - base == v exactly: one of the two is 0 at every element
    cases = {'plain': (v, None), 'base': (np.where(pick, v, np.float32(0)).astype(np.float32), np.where(pick, np.float32(0), -v).astype(np.float32))}
    pad = 3                                                 # the vectors start 12 bytes past an allocation: head, body and tail all occur
    ws, flags = ops.merge_kth_ws('cuda'), torch.zeros(1, dtype=torch.int32, device='cuda')
    ks = sorted({1, max(1, int(0.8 * n)), n})
    out = torch.full((2, len(ks)), -1.0, device='cuda')
    want = np.sort(np.abs(v))
    for ci, (x, base) in enumerate(cases.values()):
        if base is not None:
            assert np.array_equal(bits(np.abs(x - base)), bits(np.abs(v)))
        xd = _dev(np.concatenate([np.zeros(pad, np.float32), x]))[pad:]
        bd = None if base is None else _dev(np.concatenate([np.zeros(pad, np.float32), base]))[pad:]
        for ki, k in enumerate(ks):
            ops.merge_kth_abs(xd, bd, k, out[ci, ki:ki + 1], flags, ws)
    got = out.cpu().numpy()
    for ci in range(2):
        assert np.array_equal(bits(got[ci]), bits(want[[k - 1 for k in ks]])), (ci, ks, got[ci], want[[k - 1 for k in ks]])
    assert int(flags.item()) == 0


@gpu
def test_kth_abs_misaligned_base_and_flags():
    _need_gpu()
    from pianobart_amd import ops
    rng = np.random.default_rng(5)
    n = 4099
    x, b = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    ws, out = ops.merge_kth_ws('cuda'), torch.zeros(4, device='cuda')
    flags = torch.zeros(4, dtype=torch.int32, device='cuda')
    xd, bd = _dev(np.concatenate([np.zeros(1, np.float32), x]))[1:], _dev(np.concatenate([np.zeros(2, np.float32), b]))[2:]     # offset differently: scalar path
    ops.merge_kth_abs(xd, bd, 1234, out[0:1], flags[0:1], ws)
    assert bits(out[0:1].cpu().numpy())[0] == bits(np.sort(np.abs(x - b))[1233:1234])[0] and int(flags[0]) == 0
    for i, bad in enumerate((np.inf, -np.inf, np.nan), start=1):
        y = x.copy()
        y[n - 2] = bad
        ops.merge_kth_abs(_dev(y), None, 7, out[i:i + 1], flags[i:i + 1], ws)
    assert flags.cpu().tolist() == [0, 1, 1, 1]
    huge = np.full(8, 3e38, dtype=np.float32)               # finite operands whose difference overflows
    f2 = torch.zeros(1, dtype=torch.int32, device='cuda')
    ops.merge_kth_abs(_dev(huge), _dev(-huge), 8, out[0:1], f2, ws)
    assert int(f2.item()) == 1


# ---- the fused pass -------------------------------------------------------------------------------------------------------------------
def _models(n, N, seed):
    key = (n, seed)
    if key not in _CACHE:
        rng = np.random.default_rng(seed)
        p = (rng.standard_normal(n) * 0.1).astype(np.float32)
        fs = []
        for m in range(8):
            d = (rng.standard_normal(n) * 0.01 * (m + 1)).astype(np.float32)
            d[rng.random(n) < 0.05] = 0.0                   # untouched elements: ties in the magnitude order, zero sums
            fs.append((p + d).astype(np.float32))
        _CACHE[key] = (p, fs, _dev(p), [_dev(f) for f in fs])
    p, fs, pd, fd = _CACHE[key]
    return p, fs[:N], pd, fd[:N]


def _words(seed, m, n):
    key = ('w', seed, m, n)
    if key not in _CACHE:
        _CACHE[key] = R.mask_words(seed, m, np.arange(n, dtype=np.uint64))
    return _CACHE[key]


def _plans():
    yield 'average', dict(method='average_merging')
    yield 'task', dict(method='task_arithmetic', scaling_coefficient=0.7)
    yield 'ties', dict(method='ties_merging', param_value_mask_rate=0.8, scaling_coefficient=0.7)
    for strategy in ('magnitude', 'random'):
        for apply in ('average_merging', 'task_arithmetic', 'ties_merging'):
            for fmt in ('delta_weight', 'finetuned_weight'):
                for rescale in (True, False):
                    yield '%s/%s/%s/%s' % (strategy, apply, fmt, 'rescale' if rescale else 'plain'), dict(
                        method='mask_merging', mask_apply_method=apply, mask_strategy=strategy, weight_format=fmt, use_weight_rescale=rescale,
                        scaling_coefficient=0.7, param_value_mask_rate=0.8, seed=0xC0FFEE12345)


def _rates(N):
    return [0.8, 0.5, 0.9, 0.25, 1.0, 0.0, 0.6, 0.99][:N]


def _ref_merge(p, fs, segs, kw):
    """merge_ref.merge with the mask words of the big vector computed once for all plans."""
    if kw.get('mask_strategy') != 'random':
        return R.merge(p, fs, segs, **kw)
    ws = []
    for m, f in enumerate(fs):
        rate = kw['weight_mask_rates'][m]
        x = f - p if kw['weight_format'] == 'delta_weight' else f.copy()
        x = x * (_words(kw['seed'], m, p.size).astype(np.uint64) >= np.uint64(R.drop_threshold(rate))).astype(np.float32)
        if kw['use_weight_rescale'] and rate != 1.0:
            x = x / np.float32(1.0 - rate)
        ws.append(p + x if kw['weight_format'] == 'delta_weight' else x)
    assert np.array_equal(bits(ws[0][:999]), bits(R.masked_model(p[:999], fs[0][:999], None, kw['weight_mask_rates'][0], 'random', kw['weight_format'],
                                                                 kw['use_weight_rescale'], kw['seed'], 0)))
    rest = {k: v for k, v in kw.items() if k in ('scaling_coefficient', 'param_value_mask_rate')}
    return R.merge(p, ws, segs, method=kw['mask_apply_method'], **rest)


@gpu
@pytest.mark.parametrize('name,kw', list(_plans()), ids=[n for n, _ in _plans()])
def test_merge_flat_equals_restatement(name, kw):
    """Every method x format x rescale; N in {2, 3, 8} at every n up to 4 099, N = 3 at 2^20 + 5."""
    _need_gpu()
    from pianobart_amd.merge import MergePlan, merge_flat
    for n in NS:
        for N in ((3,) if n == BIG else (2, 3, 8)):
            p, fs, pd, fd = _models(n, N, 11)
            segs = _segs(n)
            full = dict(kw, weight_mask_rates=_rates(N)) if kw['method'] == 'mask_merging' else dict(kw)
            got = merge_flat(MergePlan(N, **full), pd, fd, segs).cpu().numpy()
            want = _ref_merge(p, fs, segs, full)
            assert np.array_equal(bits(got), bits(want)), (name, n, N, int((bits(got) != bits(want)).sum()), np.flatnonzero(bits(got) != bits(want))[:5])


@gpu
def test_segment_call_draws_the_whole_vectors_mask():
    """pb_merge_apply over [5, n) with g0 = 5 equals the whole-vector call there, for every method that masks."""
    _need_gpu()
    from pianobart_amd import ops, _lib
    from pianobart_amd.merge import drop_threshold, rescale_divisor
    n, N = 4099, 3
    p, fs, pd, fd = _models(n, N, 11)
    kw = dict(fmt=_lib.MERGE_DELTA, lam=0.7, seed=99, kinds=[_lib.MERGE_MASK_RANDOM] * N, drop_thresh=[drop_threshold(r) for r in _rates(N)],
              rescale=[rescale_divisor(r, True) for r in _rates(N)])
    for method in (_lib.MERGE_AVERAGE, _lib.MERGE_TASK):
        whole, part = torch.zeros(n, device='cuda'), torch.zeros(n, device='cuda')
        ops.merge_apply(ops.merge_desc(pd, fd, whole, method=method, **kw))
        for g0 in (5, 6, 7, 8):
            part.zero_()
            ops.merge_apply(ops.merge_desc(pd[g0:], [f[g0:] for f in fd], part[g0:], method=method, g0=g0, **kw))
            assert torch.equal(part[g0:], whole[g0:]) and float(part[:g0].abs().sum()) == 0.0, (method, g0)
        want = R.merge(p, fs, None, method='mask_merging', mask_apply_method='average_merging' if method == _lib.MERGE_AVERAGE else 'task_arithmetic',
                       mask_strategy='random', weight_mask_rates=_rates(N), scaling_coefficient=0.7, seed=99)
        assert np.array_equal(bits(whole.cpu().numpy()), bits(want))


# ---- the random mask -----------------------------------------------------------------------------------------------------------------
def _keep_mask(n, rate, seed, model, g0=0):
    """1.0 where the element is kept: the masked model of an all-ones vector in the fine-tuned format, without rescale."""
    from pianobart_amd import ops, _lib
    from pianobart_amd.merge import drop_threshold
    ones, zeros, out = torch.ones(n, device='cuda'), torch.zeros(n, device='cuda'), torch.empty(n, device='cuda')
    ops.merge_apply(ops.merge_desc(zeros, [ones], out, method=_lib.MERGE_MASKED, fmt=_lib.MERGE_FINETUNED, kinds=[_lib.MERGE_MASK_RANDOM],
                                   drop_thresh=[drop_threshold(rate)], seed=seed, g0=g0, model_base=model))
    return out.cpu().numpy()


@gpu
def test_random_mask_equals_host_words_and_its_rate():
    _need_gpu()
    n, rate, seed = 2 ** 20, 0.8, 0x0123456789ABCDEF
    keep = _keep_mask(n, rate, seed, 0)
    want = (_words(seed, 0, n).astype(np.uint64) >= np.uint64(R.drop_threshold(rate))).astype(np.float32)
    assert np.array_equal(bits(keep), bits(want))
    dropped = int((keep == 0).sum())
    print('dropped %d of %d at rate %.1f' % (dropped, n, rate))
    assert abs(dropped - 838861) <= 2458, dropped
    again, other_seed, other_model = _keep_mask(n, rate, seed, 0), _keep_mask(n, rate, seed + 1, 0), _keep_mask(n, rate, seed, 1)
    assert np.array_equal(keep, again)
    assert 0.25 < (other_seed != keep).mean() < 0.40 and 0.25 < (other_model != keep).mean() < 0.40      # independent masks differ on 2 p (1 - p) = 0.32
    assert np.array_equal(bits(other_model), bits((_words(seed, 1, n).astype(np.uint64) >= np.uint64(R.drop_threshold(rate))).astype(np.float32)))
    assert _keep_mask(4099, 1.0, seed, 0).sum() == 0 and _keep_mask(4099, 0.0, seed, 0).sum() == 4099
    m7 = _keep_mask(257, 0.5, seed, 2, g0=7)
    assert np.array_equal(m7, (R.mask_words(seed, 2, np.arange(7, 7 + 257, dtype=np.uint64)).astype(np.uint64) >= np.uint64(R.drop_threshold(0.5))).astype(np.float32))


# ---- the reference's recorded results ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('case,kw', list(golden_cases()), ids=[c for c, _ in golden_cases()])
def test_merge_flat_equals_the_reference_bit_for_bit(case, kw):
    _need_gpu()
    from pianobart_amd.merge import MergePlan, merge_flat
    z, segs = load_golden()
    got = merge_flat(MergePlan(3, **kw), _dev(z['pre']), [_dev(f) for f in z['ft']], segs).cpu().numpy()
    assert np.array_equal(bits(got), bits(z['out/' + case])), int((bits(got) != bits(z['out/' + case])).sum())


@gpu
def test_ties_zero_sum_takes_the_majority_sign():
    _need_gpu()
    from pianobart_amd.merge import MergePlan, Segment, merge_flat

    def run(p, f0, f1, lam=0.5):
        p, f0, f1 = (np.asarray(a, dtype=np.float32) for a in (p, f0, f1))
        segs = [Segment('w', 0, p.size, (p.size,))]
        got = merge_flat(MergePlan(2, method='ties_merging', param_value_mask_rate=0.0, scaling_coefficient=lam), _dev(p), [_dev(f0), _dev(f1)], segs).cpu().numpy()
        assert np.array_equal(bits(got), bits(R.ties(p, [f0, f1], 0.0, lam)))
        return got

    # sums (+2, -2, 0): one positive, one negative sign -> no majority: element 2 (task vectors +0.5 and -0.5) merges to 0, the result is the pre-trained value
    out = run([0.25, 0.25, 0.25], [1.25, -0.75, 0.75], [1.25, -0.75, -0.25])
    assert out.tolist() == [0.25 + 0.5 * 1.0, 0.25 - 0.5 * 1.0, 0.25]
    # one more positive element: the majority is +, element 2 keeps its positive entry alone (+0.5 / 1)
    out = run([0.25, 0.25, 0.25, 0.0], [1.25, -0.75, 0.75, 2.0], [1.25, -0.75, -0.25, 4.0])
    assert out.tolist() == [0.75, -0.25, 0.25 + 0.5 * 0.5, 0.5 * 3.0]
    out = run([0.25, 0.25, 0.25, 0.0], [1.25, -0.75, 0.75, -2.0], [1.25, -0.75, -0.25, -4.0])
    assert out.tolist() == [0.75, -0.25, 0.25 - 0.5 * 0.5, -0.5 * 3.0]


# ---- state dicts -----------------------------------------------------------------------------------------------------------------------
@gpu
def test_merge_state_dicts_on_a_small_pianobart():
    _need_gpu()
    import copy
    from pianobart_amd.merge import merge_state_dicts, state_dict_layout
    from pianobart_amd.model import BartConfig, PianoBart
    from tests.golden_util import load_vocab, randomize_params, synth_octuple_batch
    e2w, w2e = load_vocab()
    S = 64
    cfg = BartConfig(max_position_embeddings=S, d_model=256, encoder_layers=2, decoder_layers=2, encoder_ffn_dim=512, decoder_ffn_dim=512,
                     encoder_attention_heads=4, decoder_attention_heads=4, dropout=0.0, vocab_size=128)
    pre = PianoBart(cfg, e2w, w2e, precision='fp32')
    randomize_params(pre, 3)
    g = torch.Generator().manual_seed(4)
    fts = []
    for i in range(3):
        m = copy.deepcopy(pre)
        with torch.no_grad():
            for q in m.parameters():
                q.add_(torch.randn(q.shape, generator=g) * 0.003 * (i + 1))
        fts.append(m.state_dict())
    pre_sd = pre.state_dict()
    segs, alias = state_dict_layout(pre_sd)
    assert sorted(n for names in alias.values() for n in names) == sorted(pre_sd)
    assert len(alias) == len(list(pre.parameters())) < len(pre_sd)                       # tied tables are one parameter, as in named_parameters()
    flat = lambda sd: np.concatenate([sd[s.name].numpy().reshape(-1) for s in segs])
    p, fs = flat(pre_sd), [flat(sd) for sd in fts]
    for kw in (dict(method='ties_merging', param_value_mask_rate=0.8, scaling_coefficient=0.9),
               dict(method='mask_merging', mask_strategy='magnitude', mask_apply_method='task_arithmetic', weight_mask_rates=[0.8, 0.5, 0.9], scaling_coefficient=0.7)):
        a = merge_state_dicts(pre_sd, fts, **kw)
        b = merge_state_dicts(pre_sd, fts, **kw)
        assert list(a) == list(pre_sd)
        want = R.merge(p, fs, segs, **kw)
        for s in segs:
            for name in alias[s.name]:
                assert a[name].shape == pre_sd[name].shape
                assert np.array_equal(bits(a[name].numpy().reshape(-1)), bits(want[s.offset:s.offset + s.numel])), name
                assert a[name].numpy().tobytes() == b[name].numpy().tobytes(), name
        assert not np.array_equal(want, p)
    merged = PianoBart(cfg, e2w, w2e, precision='fp32')
    merged.load_state_dict(a, strict=True)
    merged = merged.cuda().eval()
    enc, dec, _, emask, dmask, _ = synth_octuple_batch(2, S, seed=2)
    h = merged(enc.cuda(), dec.cuda(), emask.cuda(), dmask.cuda()).last_hidden_state
    assert h.shape == (2, S, 256) and bool(torch.isfinite(h).all())
