"""CPU: Fisher merging without a device -- the float32 restatement (tests/fisher_ref.py) against the reference's recorded results
(tests/golden/g16_fisher.npz, bit for bit), the bound on a merge that uses a float64 norm of its own, the coefficients merge.py forms, the
generated code of pb_fisher.hip, the flags, every refusal that comes before device work, and the exported symbols."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from pianobart_amd import _lib
from pianobart_amd._lib import PBError
from pianobart_amd import merge as M
from tests import fisher_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g16_fisher.npz')
NS = (3, 8)


def golden_cases(z, n):
    yield 'default', {}
    yield 'plain', dict(normalize_fisher_weight=False)
    yield 'coef', dict(fisher_scaling_coefficients=[float(c) for c in z['coef'][:n]])
    yield 'minimal', dict(minimal_fisher_weight=1e-3)


CASES = [(c, n) for n in NS for c in ('default', 'plain', 'coef', 'minimal')]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_golden_file_holds_the_toy_classifier_and_its_degenerate_elements():
    z = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 256 * 1024
    shapes = {str(n): tuple(int(v) for v in sh if v) for n, sh in zip(z['names'], z['shapes'])}
    segs = M.segment_table(shapes)
    n = segs[-1].offset + segs[-1].numel
    assert 1200 <= n <= 1400 and {len(s.shape) for s in segs} == {1, 2, 3}
    assert len([k for k in z.files if k.startswith('out/')]) == 8
    for N in NS:
        W, F = z['ft%d' % N], z['F%d' % N]
        assert W.shape == F.shape == (N, n) and W.dtype == F.dtype == np.float32 and z['norm%d' % N].shape == (N,)
        assert np.isfinite(F).all() and (F >= 0).all()
        assert ((F == 0).all(axis=0)).sum() >= 8                 # F = 0 in every model
        assert ((F == 0).sum(axis=0) == 1).sum() >= 8            # F = 0 in one model only


@pytest.mark.parametrize('case,N', CASES, ids=['%s-%d' % c for c in CASES])
def test_restatement_equals_the_reference_bit_for_bit(case, N):
    z = np.load(GOLDEN)
    kw = dict(golden_cases(z, N))[case]
    want = z['out/%s/%d' % (case, N)]
    got = R.merge(list(z['ft%d' % N]), list(z['F%d' % N]), norms=z['norm%d' % N], **kw)
    assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want)), int((bits(got) != bits(want)).sum())
    if case == 'plain':                                          # no norm is read at all
        got = R.merge(list(z['ft%d' % N]), list(z['F%d' % N]), norms=None, **kw)
        assert np.array_equal(bits(got), bits(want))
    avg = z['ft%d' % N].astype(np.float64).mean(axis=0)
    assert np.abs(want - avg).max() > 1e-4                       # the Fisher weights matter: not the plain mean


def _eps_c(z):
    eps = 0.0
    for N in NS:
        own = np.array([R.norm64(f) for f in z['F%d' % N]], dtype=np.float64)
        eps = max(eps, float(np.max(np.abs(z['norm%d' % N].astype(np.float64) - own) / own)))
    return eps


def test_reference_norms_are_close_to_the_float64_norm():
    """eps_c: the largest relative difference between the reference's norms (float32 torch.norm of per-tensor norms) and
    float32(sqrt(float64 sum)) of the recorded F. The toy was chosen so that it stays within 8 * 2^-24."""
    assert _eps_c(np.load(GOLDEN)) <= 8 * 2.0 ** -24


@pytest.mark.parametrize('case,N', [c for c in CASES if c[0] != 'plain'], ids=['%s-%d' % c for c in CASES if c[0] != 'plain'])
def test_own_float64_norm_stays_within_the_bound(case, N):
    """A merge that takes float32(sqrt(float64 sum)) for the norm: the coefficients move by at most eps_c (relative), which enters numerator
    and denominator alike, so an element moves by at most 2 eps_c times the spread of the models' values there; 2 ulp for the last roundings."""
    z = np.load(GOLDEN)
    kw = dict(golden_cases(z, N))[case]
    W = z['ft%d' % N]
    want = z['out/%s/%d' % (case, N)]
    got = R.merge(list(W), list(z['F%d' % N]), own_norm=True, **kw)
    eps_c = _eps_c(z)
    bound = 2 * eps_c * (W.max(axis=0).astype(np.float64) - W.min(axis=0)) + 2 * np.spacing(np.abs(want)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= bound).all(), float((err - bound).max())


def test_merge_py_forms_the_coefficients_of_the_restatement():
    z = np.load(GOLDEN)
    for N in NS:
        for case, kw in golden_cases(z, N):
            norms = z['norm%d' % N]
            want = R.coefficients(N, norms=norms, **kw)
            plan = M.MergePlan(N, method='fisher_merging', fisher_weights=[{}] * N, fisher_norms=list(norms), **kw)
            got = M.fisher_coefficients(N, plan.coefficients, plan.normalize, plan.minimal, plan.norms)
            assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want)), (case, N)
    g = torch.Generator().manual_seed(1)
    for N in range(2, 9):                                        # the order of torch's own sum of N values
        for _ in range(200):
            x = torch.rand(N, generator=g) * 10.0 ** torch.randint(-3, 4, (N,), generator=g).float()
            assert bits(M.torch_sum_f32(x.numpy())) == bits(x.sum().numpy()) == bits(R.small_sum(x.numpy())), N


def test_flags_and_their_defaults():
    from pianobart_amd.fisher import get_args_fisher
    from pianobart_amd.model_merge import fisher_kwargs, get_args_merge
    a = get_args_merge(['--method', 'fisher_merging'])
    assert fisher_kwargs(a) == ([], dict(fisher_scaling_coefficients=None, normalize_fisher_weight=True, minimal_fisher_weight=1e-6))
    a = get_args_merge(['--method', 'fisher_merging', '--fisher', 'a.pt,b.pt', '--fisher_scaling_coefficients', '0.25,0.75', '--no_normalize_fisher_weight',
                        '--minimal_fisher_weight', '1e-3'])
    assert fisher_kwargs(a) == (['a.pt', 'b.pt'], dict(fisher_scaling_coefficients=[0.25, 0.75], normalize_fisher_weight=False, minimal_fisher_weight=1e-3))
    assert not any(k.startswith('fisher') or 'fisher' in k for k in vars(get_args_merge([])))      # the other methods' namespace is as it was
    f = get_args_fisher(['--ckpt', 'ft.ckpt', '--task', 'composer', '--dataset', 'Pianist8', '--output', 'a.fisher.pt'])
    assert (f.num_examples, f.batch_size, f.precision, f.class_num, f.dataroot, f.hs, f.layers) == (256, 8, 'bf16', 8, None, 1024, 8)
    f = get_args_fisher(['--ckpt', 'x', '--task', 'velocity', '--dataset', 'GiantMIDI1k', '--output', 'o', '--num_examples', '10', '--batch_size', '4',
                         '--precision', 'fp32', '--dataroot', 'd'])
    assert (f.num_examples, f.batch_size, f.precision, f.class_num, f.dataroot) == (10, 4, 'fp32', 7, 'd')
    with pytest.raises(PBError, match='positive'):
        get_args_fisher(['--ckpt', 'x', '--task', 'melody', '--dataset', 'POP909', '--output', 'o', '--num_examples', '0'])


def _sd(seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return {'b.weight': torch.randn(3, 5, generator=g) * scale, 'a.bias': torch.randn(7, generator=g) * scale, 'c.k': torch.randn(2, 3, 4, generator=g) * scale}


def _fw(seed=0):
    return {k: v.abs() for k, v in _sd(seed).items()}


def test_refusals_come_before_device_work():
    """None of these reaches a device: they pass on a machine without one."""
    fish = dict(method='fisher_merging')
    with pytest.raises(PBError, match=r'fisher_merging.*pianobart_amd\.fisher'):
        M.merge_state_dicts(_sd(), [_sd(1), _sd(2)], **fish)
    for name in ('fisher_merging', 'regmean_merging'):
        with pytest.raises(PBError, match=name):
            M.merge_state_dicts(_sd(), [_sd(1), _sd(2)], mask_apply_method=name, fisher_weights=[_fw(1), _fw(2)])
    for name in ('regmean_merging', 'regmean'):
        with pytest.raises(PBError, match='regmean'):
            M.merge_state_dicts(_sd(), [_sd(1), _sd(2)], method=name, fisher_weights=[_fw(1), _fw(2)])
    with pytest.raises(PBError, match='1 sets of Fisher weights for 2 models'):
        M.merge_state_dicts(_sd(), [_sd(1), _sd(2)], fisher_weights=[_fw(1)], **fish)
    bad = _fw(2)
    bad['d.other'] = torch.zeros(3)
    with pytest.raises(PBError, match='d.other'):
        M.merge_state_dicts(_sd(), [_sd(1), _sd(2)], fisher_weights=[_fw(1), bad], **fish)
    bad = _fw(2)
    del bad['a.bias']
    with pytest.raises(PBError, match='different parameters.*a.bias'):
        M.merge_state_dicts(_sd(), [_sd(1), _sd(2)], fisher_weights=[_fw(1), bad], **fish)
    bad = _fw(2)
    bad['b.weight'] = torch.zeros(5, 3)
    with pytest.raises(PBError, match='b.weight'):
        M.merge_state_dicts(_sd(), [_sd(1), _sd(2)], fisher_weights=[_fw(1), bad], **fish)
    with pytest.raises(PBError, match='non-empty'):
        M.merge_state_dicts(_sd(), [_sd(1), _sd(2)], fisher_weights=[_fw(1), {}], **fish)
    for value in (-1e-9, float('inf'), float('nan')):
        bad = _fw(2)
        bad['c.k'][1, 2, 3] = value
        with pytest.raises(PBError, match='negative or non-finite'):
            M.merge_state_dicts(_sd(), [_sd(1), _sd(2)], fisher_weights=[_fw(1), bad], **fish)
    for value in (0.0, -1e-6, float('nan'), float('inf'), 1e-60):
        with pytest.raises(PBError, match='minimal_fisher_weight'):
            M.merge_state_dicts(_sd(), [_sd(1), _sd(2)], fisher_weights=[_fw(1), _fw(2)], minimal_fisher_weight=value, **fish)
    with pytest.raises(PBError, match='3 coefficients for 2 models'):
        M.merge_state_dicts(_sd(), [_sd(1), _sd(2)], fisher_weights=[_fw(1), _fw(2)], fisher_scaling_coefficients=[1.0, 1.0, 1.0], **fish)
    for value in (0.0, -0.5, float('nan')):
        with pytest.raises(PBError, match='positive and finite'):
            M.merge_state_dicts(_sd(), [_sd(1), _sd(2)], fisher_weights=[_fw(1), _fw(2)], fisher_scaling_coefficients=[1.0, value], **fish)
    with pytest.raises(PBError, match='fisher_norms'):
        M.merge_state_dicts(_sd(), [_sd(1), _sd(2)], fisher_weights=[_fw(1), _fw(2)], fisher_norms=[1.0], **fish)
    with pytest.raises(PBError, match='at least two'):
        M.merge_state_dicts(_sd(), [_sd(1)], fisher_weights=[_fw(1)], **fish)
    from pianobart_amd.model_merge import model_merge
    with pytest.raises(PBError, match='fisher_merging'):                     # before any file is opened: none of these exists
        model_merge(['--model_path', 'no/a.ckpt,no/b.ckpt', '--pretrain_ckpt', 'no/pre.ckpt', '--dict_file', 'no/dict.pkl', '--method', 'fisher_merging'])
    with pytest.raises(PBError, match='1 sets of Fisher weights for 2 models'):
        model_merge(['--model_path', 'no/a.ckpt,no/b.ckpt', '--pretrain_ckpt', 'no/pre.ckpt', '--dict_file', 'no/dict.pkl', '--method', 'fisher_merging',
                     '--fisher', 'no/a.fisher.pt'])
    with pytest.raises(PBError, match='no CPU'):
        M.fisher_weights(None, [], 10, 4, True, device='cpu')


def test_a_tied_table_may_come_under_any_of_its_names():
    pre = _sd()
    pre['z.alias'] = pre['b.weight']                             # shares storage: one parameter, two names
    segs, alias = M.state_dict_layout(pre)
    assert [s.name for s in segs] == ['a.bias', 'b.weight', 'c.k'] and alias['b.weight'] == ['b.weight', 'z.alias']
    one, other = _fw(1), _fw(2)
    other['z.alias'] = other.pop('b.weight')
    M.check_fisher_dicts([one, other], pre, segs, alias)
    flat = M.pack_fisher(other, segs, alias, 46, 1)
    assert np.array_equal(flat[7:22], other['z.alias'].numpy().reshape(-1)) and np.array_equal(flat[:7], other['a.bias'].numpy())
    del other['c.k']                                             # a parameter without Fisher weights in one model only
    with pytest.raises(PBError, match='different parameters.*c.k'):
        M.check_fisher_dicts([one, other], pre, segs, alias)
    del one['c.k']                                               # .. in every model: Fisher weight 0 there
    M.check_fisher_dicts([one, other], pre, segs, alias)
    assert not M.pack_fisher(one, segs, alias, 46, 0)[22:].any()


def test_exported_symbols_and_descriptor_layout():
    decls = _lib.parse_header()
    for name in ('pb_fisher_rows', 'pb_fisher_accum', 'pb_fisher_finish', 'pb_fisher_norm', 'pb_fisher_merge', 'pb_fisher_desc_bytes', 'pb_fisher_norm_ws_bytes'):
        assert name in decls, name
    assert ctypes.sizeof(_lib.FisherDesc) == _lib.LIB.query('pb_fisher_desc_bytes')
    assert ctypes.sizeof(_lib.FisherDesc) == sum(ctypes.sizeof(t) for _, t in _lib.FisherDesc._fields_)        # no implicit padding
    assert _lib.LIB.query('pb_fisher_norm_ws_bytes') == 2048 * 8
    assert _lib.LIB.query('pb_abi_version') == 10
    from pianobart_amd import build
    assert build.FILE_FLAGS['pb_fisher.hip'] == ['-ffp-contract=off']


def _desc(**over):
    d = _lib.FisherDesc()
    d.out, d.n, d.n_models, d.minimal = 0x20000, 16, 2, 1e-6
    for m in range(8):
        d.model[m] = 0x30000 + 0x1000 * m
        d.fisher[m] = 0x50000 + 0x1000 * m
        d.coef[m] = 0.5
    for k, v in over.items():
        if isinstance(v, tuple):
            getattr(d, k)[v[0]] = v[1]
        else:
            setattr(d, k, v)
    return d


@pytest.mark.parametrize('fields,names', [
    (dict(n_models=9), 'n_models = 9'),
    (dict(n_models=1), 'n_models = 1'),
    (dict(n=-1), 'n = -1'),
    (dict(out=0), 'out'),
    (dict(out=0x20002), 'out'),
    (dict(minimal=0.0), 'minimal'),
    (dict(minimal=float('nan')), 'minimal'),
    (dict(coef=(1, 0.0)), 'coef[1]'),
    (dict(coef=(0, float('inf'))), 'coef[0]'),
    (dict(model=(1, 0)), 'model[1]'),
    (dict(fisher=(0, 0)), 'fisher[0]'),
    (dict(fisher=(1, 0x50001)), 'fisher[1]'),
    (dict(out=0x31000), 'aliases model[1]'),
    (dict(out=0x50000), 'aliases model[0] or fisher[0]'),
])
def test_merge_descriptor_preconditions_refuse_without_a_gpu(fields, names):
    with pytest.raises(PBError) as e:
        _lib.LIB.call('pb_fisher_merge', ctypes.byref(_desc(**fields)), None)
    assert 'pb_fisher_merge' in str(e.value) and names in str(e.value), str(e.value)


def test_entry_preconditions_refuse_without_a_gpu():
    call = _lib.LIB.call
    for args, names in (((0x10000, None, 0x20000, None, -1, 4, None), 'rows = -1'), ((0x10000, None, 0x20000, None, 4, 0, None), 'C = 0'),
                        ((None, None, 0x20000, None, 4, 4, None), 'non-NULL'), ((0x10000, None, 0x20000, 0x10000, 4, 4, None), 'aliases')):
        with pytest.raises(PBError, match=re.escape(names)):
            call('pb_fisher_rows', *args)
    for args, names in (((0x10000, 0x20000, -1, None), 'n = -1'), ((None, 0x20000, 4, None), 'non-NULL'), ((0x10000, 0x10000, 4, None), 'aliases'),
                        ((0x10002, 0x20000, 4, None), 'non-NULL f32')):
        with pytest.raises(PBError, match=re.escape(names)):
            call('pb_fisher_accum', *args)
    for args, names in (((0x10000, 4, 0, 0x20000, None), 'divisor = 0'), ((0x10000, 4, 1 << 25, 0x20000, None), 'divisor'), ((0x10000, 4, 12, None, None), 'flags'),
                        ((None, 4, 12, 0x20000, None), 'non-NULL')):
        with pytest.raises(PBError, match=re.escape(names)):
            call('pb_fisher_finish', *args)
    for args, names in (((0x10000, 0, 0x20000, 0x30000, None), 'n = 0'), ((0x10000, 4, None, 0x30000, None), 'ws'), ((0x10000, 4, 0x20004, 0x30000, None), 'ws'),
                        ((0x10000, 4, 0x20000, None, None), 'non-NULL')):
        with pytest.raises(PBError, match=re.escape(names)):
            call('pb_fisher_norm', *args)
    call('pb_fisher_rows', 0x10000, None, 0x20000, None, 0, 4, None)             # empty ranges are no-ops
    call('pb_fisher_accum', 0x10000, 0x20000, 0, None)
    call('pb_fisher_finish', 0x10000, 0, 12, 0x20000, None)
    call('pb_fisher_merge', ctypes.byref(_desc(n=0)), None)


def test_ops_refuse_cpu_tensors():
    from pianobart_amd import heads, ops
    x = torch.zeros(8)
    with pytest.raises(PBError, match='HIP device tensors'):
        ops.fisher_accum(x, x.clone())
    with pytest.raises(PBError, match='HIP device tensors'):
        ops.fisher_desc([x, x], [x, x], x.clone(), [0.5, 0.5], 1e-6)
    with pytest.raises(PBError, match='at most 8'):
        ops.fisher_desc([x] * 9, [x] * 9, x, [1.0] * 9, 1e-6)
    with pytest.raises(PBError, match='HIP device tensors'):
        heads.fisher_expectation_rows(torch.zeros(2, 3))
    with pytest.raises(PBError, match='shape of logits'):
        heads.fisher_expectation_rows(torch.zeros(2, 3), torch.zeros(3))


def test_fisher_kernels_hold_no_fused_multiply_add_outside_divisions(tmp_path):
    """Bit parity needs every float32 operation rounded on its own. pb_fisher.hip is compiled with a flag of its own (build.FILE_FLAGS): in
    the gfx950 code of its accumulate, finish and merge kernels the only fused multiply-adds are the five of each IEEE division's
    expansion (one v_div_fixup_f32 per division); the accumulate kernels hold neither."""
    from pianobart_amd import build
    src = os.path.join(build.CSRC, 'pb_fisher.hip')
    out = str(tmp_path / 'pb_fisher.s')
    flags = [f for f in build.FLAGS if f != '-fPIC'] + build.FILE_FLAGS['pb_fisher.hip']
    r = subprocess.run([build._hipcc()] + flags + ['-S', '--cuda-device-only', src, '-o', out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    # a kernel's code runs to its .Lfunc_end label (a kernel may hold more than one s_endpgm: an early exit comes first)
    kernels = re.findall(r'^(_Z\w*fisher_(?:accum|finish|merge)_kernel\w*):[^\n]*\n(.*?)^\.Lfunc_end', open(out).read(), flags=re.S | re.M)
    assert len(kernels) == 2 + 1 + 2, [k for k, _ in kernels]
    divisions = {}
    for name, body in kernels:
        fused = len(re.findall(r'\bv_(?:fma|fmac|mad|mac|pk_fma)_f32', body))
        div = len(re.findall(r'\bv_div_fixup_f32', body))
        assert fused == 5 * div, (name, fused, div)
        kind = re.search(r'fisher_(accum|finish|merge)', name).group(1)
        divisions[kind] = divisions.get(kind, 0) + div
    assert divisions['accum'] == 0 and divisions['finish'] > 0 and divisions['merge'] > 0, divisions
