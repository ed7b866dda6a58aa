"""CPU: checkpoint merging without a device -- the float32 restatement (tests/merge_ref.py) against the reference's recorded results
(tests/golden/g15_merge.npz, bit for bit), the command line's flags and defaults, checkpoint reading, every refusal that comes before
device work, the canonical layout, and the exported symbols."""
import ctypes
import os

import numpy as np
import pytest
import torch

from pianobart_amd import _lib
from pianobart_amd._lib import PBError
from pianobart_amd import merge as M
from tests import merge_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g15_merge.npz')
RATES, LAMBDA, TIES_RATE = [0.8, 0.5, 0.9], 0.7, 0.8


def load_golden():
    z = np.load(GOLDEN)
    shapes = {str(n): tuple(int(v) for v in sh if v) for n, sh in zip(z['names'], z['shapes'])}
    return z, M.segment_table(shapes)


def golden_cases():
    """(case, keyword arguments of merge_ref.merge / MergePlan): what tests/golden/make_merge_goldens.py recorded."""
    yield 'average', dict(method='average_merging')
    yield 'task', dict(method='task_arithmetic', scaling_coefficient=LAMBDA)
    yield 'ties', dict(method='ties_merging', param_value_mask_rate=TIES_RATE, scaling_coefficient=1.0)
    for apply in ('average_merging', 'task_arithmetic', 'ties_merging'):
        for fmt in ('delta_weight', 'finetuned_weight'):
            for rescale in (True, False):
                yield 'mag/%s/%s/%s' % (apply, fmt, 'rescale' if rescale else 'plain'), dict(
                    method='mask_merging', mask_apply_method=apply, mask_strategy='magnitude', weight_format=fmt, use_weight_rescale=rescale,
                    weight_mask_rates=RATES, scaling_coefficient=LAMBDA, param_value_mask_rate=TIES_RATE)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_golden_file_is_small_and_holds_the_toy_module():
    z, segs = load_golden()
    assert os.path.getsize(GOLDEN) < 128 * 1024
    assert [s.name for s in segs] == [str(n) for n in z['names']] == sorted(str(n) for n in z['names'])
    n = segs[-1].offset + segs[-1].numel
    assert 1000 <= n <= 1500 and z['pre'].shape == (n,) and z['ft'].shape == (3, n)
    assert {len(s.shape) for s in segs} == {1, 2, 3}
    assert len([k for k in z.files if k.startswith('out/')]) == 15


@pytest.mark.parametrize('case,kw', list(golden_cases()), ids=[c for c, _ in golden_cases()])
def test_restatement_equals_the_reference_bit_for_bit(case, kw):
    z, segs = load_golden()
    got = R.merge(z['pre'], list(z['ft']), segs, **kw)
    want = z['out/' + case]
    assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want)), int((bits(got) != bits(want)).sum())
    assert not np.array_equal(bits(want), bits(z['pre']))


def test_mask_words_are_a_stream_of_their_own():
    from tests.philox_ref import drop_words, philox4x32
    g = np.arange(3, 3 + 41, dtype=np.uint64)
    seed = 0x1234567890ABCDEF
    w = R.mask_words(seed, 2, g)
    for gi, wi in zip(g, w):
        c = philox4x32(int(gi) >> 2, 2, 0x4D455247, 0, seed & 0xFFFFFFFF, seed >> 32, 7)
        assert int(c[int(gi) & 3]) == int(wi)
    site2 = drop_words(seed, 2, g >> np.uint64(2))[np.arange(len(g)), (g & np.uint64(3)).astype(np.int64)]
    assert (site2 != w).mean() > 0.9                       # dropout site 2 of the same seed draws other words
    assert (R.mask_words(seed, 1, g) != w).mean() > 0.9
    assert R.drop_threshold(0.8) == int(np.float32(0.8) * np.float32(2.0 ** 32)) and R.drop_threshold(1.0) == 2 ** 32 and R.drop_threshold(0.0) == 0
    assert M.drop_threshold(0.8) == R.drop_threshold(0.8)
    assert M.rescale_divisor(0.8, True) == float(np.float32(1.0 - 0.8)) and M.rescale_divisor(1.0, True) == 1.0 and M.rescale_divisor(0.8, False) == 1.0


def test_flags_and_defaults_are_the_references():
    from pianobart_amd.model_merge import get_args_merge, plan_kwargs
    a = get_args_merge([])
    reference = dict(dict_file='./Data/Octuple.pkl', pretrain_ckpt='./pianobart.ckpt', model_path='', output_path='./merge_pianobart.pth',
                     max_seq_len=1024, hs=1024, layers=8, ffn_dims=2048, heads=8, mask_apply_method='average_merging', mask_strategy='random',
                     use_weight_rescale=True, weight_format='delta_weight', weight_mask_rate=0.8)
    for k, v in reference.items():
        assert getattr(a, k) == v and type(getattr(a, k)) is type(v), k
    ours = dict(method='mask_merging', scaling_coefficient=1.0, param_value_mask_rate=0.8, weight_mask_rates='', seed=0, exclude=[])
    for k, v in ours.items():
        assert getattr(a, k) == v, k
    assert set(vars(a)) == set(reference) | set(ours)
    b = get_args_merge(['--use_weight_rescale', '--weight_mask_rates', '0.8,0.5', '--exclude', 'a.*', '--exclude', 'b', '--method', 'ties_merging',
                        '--model_path', 'x.ckpt,y.ckpt'])
    kw = plan_kwargs(b)
    assert b.use_weight_rescale is False and kw['weight_mask_rates'] == [0.8, 0.5] and kw['exclude'] == ['a.*', 'b']
    p = M.MergePlan(2, **kw)
    assert p.apply == 'ties_merging' and not p.masked
    p = M.MergePlan(3, **plan_kwargs(a))
    assert p.masked and p.apply == 'average_merging' and p.strategy == 'random' and p.rates == [0.8] * 3 and p.rescale and p.lam == 1.0


def _sd(seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return {'b.weight': torch.randn(3, 5, generator=g) * scale, 'a.bias': torch.randn(7, generator=g) * scale, 'c.k': torch.randn(2, 3, 4, generator=g) * scale}


@pytest.mark.parametrize('name', ['fisher_merging', 'regmean_merging'])
def test_trainer_methods_are_refused_by_name(name):
    with pytest.raises(PBError, match=name):
        M.merge_state_dicts(_sd(), [_sd(1), _sd(2)], method=name)
    with pytest.raises(PBError, match=name):
        M.merge_state_dicts(_sd(), [_sd(1), _sd(2)], method='mask_merging', mask_apply_method=name)


def test_refusals_come_before_device_work():
    """None of these reaches a device: they pass on a machine without one."""
    with pytest.raises(PBError, match='at least two'):
        M.merge_state_dicts(_sd(), [_sd(1)], method='average_merging')
    with pytest.raises(PBError, match='at most 8'):
        M.merge_state_dicts(_sd(), [_sd(i) for i in range(9)], method='average_merging')
    bad = _sd(2)
    bad['b.weight'] = torch.zeros(5, 3)
    with pytest.raises(PBError, match='b.weight'):
        M.merge_state_dicts(_sd(), [_sd(1), bad], method='average_merging')
    for value in (float('inf'), float('nan')):
        bad = _sd(2)
        bad['c.k'][1, 2, 3] = value
        with pytest.raises(PBError, match='non-finite'):
            M.merge_state_dicts(_sd(), [_sd(1), bad], method='task_arithmetic')
    bad = _sd(0)
    bad['a.bias'][0] = float('inf')
    with pytest.raises(PBError, match='pre-trained'):
        M.merge_state_dicts(bad, [_sd(1), _sd(2)], method='task_arithmetic')
    lacking = _sd(2)
    del lacking['a.bias']
    with pytest.raises(PBError, match='a.bias'):
        M.merge_state_dicts(_sd(), [_sd(1), lacking], method='average_merging')
    with pytest.raises(PBError, match='unknown method'):
        M.merge_state_dicts(_sd(), [_sd(1), _sd(2)], method='latent_merging')
    with pytest.raises(PBError, match='mask_strategy'):
        M.merge_state_dicts(_sd(), [_sd(1), _sd(2)], mask_strategy='bernoulli')
    with pytest.raises(PBError, match='weight_format'):
        M.merge_state_dicts(_sd(), [_sd(1), _sd(2)], weight_format='both')
    with pytest.raises(PBError, match=r'\[0, 1\]'):
        M.merge_state_dicts(_sd(), [_sd(1), _sd(2)], weight_mask_rate=1.5)
    with pytest.raises(PBError, match='rates for 2 models'):
        M.merge_state_dicts(_sd(), [_sd(1), _sd(2)], weight_mask_rates=[0.5])
    with pytest.raises(PBError, match='float32'):
        M.merge_state_dicts({k: v.bfloat16() for k, v in _sd().items()}, [_sd(1), _sd(2)], method='average_merging')
    with pytest.raises(PBError, match='nothing to merge'):
        M.merge_state_dicts(_sd(), [_sd(1), _sd(2)], method='average_merging', exclude=['.*'])


def test_checkpoint_reading(capsys):
    own = set(_sd())
    inner = dict(_sd(3))
    inner['classifier.weight'] = torch.zeros(2, 2)
    for wrap in (lambda d: d, lambda d: {'state_dict': d, 'epoch': 3}):
        for prefix in ('', 'module.', 'pianobart.', 'module.pianobart.'):
            got = M.backbone_state_dict(wrap({prefix + k: v for k, v in inner.items()}), own, 'f.ckpt')
            assert set(got) == own and all(torch.equal(got[k], inner[k]) for k in own)
            out = capsys.readouterr().out
            assert '3 of 3 backbone keys matched' in out and 'dropped 1 keys' in out and 'classifier.weight' in out
    with pytest.raises(PBError, match='none of its 2 keys'):
        M.backbone_state_dict({'state_dict': {'head.w': torch.zeros(1), 'head.b': torch.zeros(1)}}, own, 'heads.ckpt')


def test_sorted_layout_and_segment_table():
    sd = _sd()
    segs = M.segment_table({k: tuple(v.shape) for k, v in sd.items()})
    assert segs == [M.Segment('a.bias', 0, 7, (7,)), M.Segment('b.weight', 7, 15, (3, 5)), M.Segment('c.k', 22, 24, (2, 3, 4))]
    assert M.segment_table({'s': (), 'r': (4,)}) == [M.Segment('r', 0, 4, (4,)), M.Segment('s', 4, 1, ())]


def test_exported_symbols_and_descriptor_layout():
    decls = _lib.parse_header()
    for name in ('pb_merge_kth_abs', 'pb_merge_kth_ws_bytes', 'pb_merge_sign_tally', 'pb_merge_apply', 'pb_merge_desc_bytes'):
        assert name in decls, name
    assert ctypes.sizeof(_lib.MergeDesc) == _lib.LIB.query('pb_merge_desc_bytes')
    assert ctypes.sizeof(_lib.MergeDesc) == sum(ctypes.sizeof(t) for _, t in _lib.MergeDesc._fields_)          # no implicit padding
    assert _lib.LIB.query('pb_merge_kth_ws_bytes') == 4 * 256 * 8 + 16
    src = open(_lib.HEADER).read()
    for name, value in (('PB_MERGE_MAX_MODELS', _lib.MERGE_MAX_MODELS), ('PB_MERGE_AVERAGE', _lib.MERGE_AVERAGE), ('PB_MERGE_TASK', _lib.MERGE_TASK),
                        ('PB_MERGE_TIES', _lib.MERGE_TIES), ('PB_MERGE_MASKED', _lib.MERGE_MASKED), ('PB_MERGE_MASK_NONE', _lib.MERGE_MASK_NONE),
                        ('PB_MERGE_MASK_MAGNITUDE', _lib.MERGE_MASK_MAGNITUDE), ('PB_MERGE_MASK_RANDOM', _lib.MERGE_MASK_RANDOM),
                        ('PB_MERGE_DELTA', _lib.MERGE_DELTA), ('PB_MERGE_FINETUNED', _lib.MERGE_FINETUNED)):
        assert '#define %s %d\n' % (name, value) in src, name


def _desc(**over):
    d = _lib.MergeDesc()
    d.pre, d.out, d.n, d.n_models = 0x10000, 0x20000, 16, 2
    for m in range(8):
        d.model[m] = 0x30000 + 0x1000 * m
        d.rescale[m] = 1.0
    for k, v in over.items():
        if isinstance(v, tuple):
            getattr(d, k)[v[0]] = v[1]
        else:
            setattr(d, k, v)
    return d


@pytest.mark.parametrize('entry,fields,names', [
    ('pb_merge_apply', dict(n_models=9), 'n_models = 9'),
    ('pb_merge_apply', dict(n_models=1), 'n_models = 1'),
    ('pb_merge_apply', dict(method=7), 'unknown method 7'),
    ('pb_merge_apply', dict(mask_kind=(1, 1)), 'without a threshold'),
    ('pb_merge_apply', dict(method=_lib.MERGE_TIES), 'tally'),
    ('pb_merge_apply', dict(method=_lib.MERGE_TIES, tally=0x40000, mask_kind=(0, 2)), 'unmasked'),
    ('pb_merge_apply', dict(out=0x30000), 'aliases model[0]'),
    ('pb_merge_apply', dict(g0=1 << 35), 'out of range'),
    ('pb_merge_apply', dict(method=_lib.MERGE_MASKED, n_models=2), 'n_models = 2'),
    ('pb_merge_sign_tally', dict(), 'tally'),
    ('pb_merge_sign_tally', dict(tally=0x40000, n_models=9), 'n_models = 9'),
])
def test_descriptor_preconditions_refuse_without_a_gpu(entry, fields, names):
    with pytest.raises(PBError) as e:
        _lib.LIB.call(entry, ctypes.byref(_desc(**fields)), None)
    assert entry in str(e.value) and names in str(e.value), str(e.value)


def test_kth_preconditions_refuse_without_a_gpu():
    for n, k in ((0, 0), (4, 0), (4, 5)):
        with pytest.raises(PBError, match='1 <= k <= n'):
            _lib.LIB.call('pb_merge_kth_abs', 0x10000, None, n, k, 0x20000, 0x30000, 0x40000, None)
    _lib.LIB.call('pb_merge_apply', ctypes.byref(_desc(n=0)), None)          # an empty range is a no-op


def test_ops_refuse_cpu_tensors_and_too_many_models():
    from pianobart_amd import ops
    x = torch.zeros(8)
    with pytest.raises(PBError, match='HIP device tensors'):
        ops.merge_desc(x, [x, x], x)
    with pytest.raises(PBError, match='at most 8'):
        ops.merge_desc(x, [x] * 9, x)


def test_merge_kernels_hold_no_fused_multiply_add_outside_divisions(tmp_path):
    """Bit parity needs every float32 operation rounded on its own. The build contracts by default and pb_merge.hip is compiled with a flag
    of its own (build.FILE_FLAGS): in the gfx950 code of every merge kernel the only fused multiply-adds are the five of each IEEE
    division's expansion (one v_div_fixup_f32 per division)."""
    import re
    import subprocess
    from pianobart_amd import build
    src = os.path.join(build.CSRC, 'pb_merge.hip')
    out = str(tmp_path / 'pb_merge.s')
    flags = [f for f in build.FLAGS if f != '-fPIC'] + build.FILE_FLAGS['pb_merge.hip']
    r = subprocess.run([build._hipcc()] + flags + ['-S', '--cuda-device-only', src, '-o', out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r'^(_Z\w*(?:kth_hist|kth_pick|tally|apply)_kernel\w*):[^\n]*\n(.*?)s_endpgm', open(out).read(), flags=re.S | re.M)
    assert len(kernels) == 2 + 1 + 2 + 8, [k for k, _ in kernels]
    divisions = 0
    for name, body in kernels:
        fused = len(re.findall(r'\bv_(?:fma|fmac|mad|mac|pk_fma)_f32', body))
        div = len(re.findall(r'\bv_div_fixup_f32', body))
        assert fused == 5 * div, (name, fused, div)
        divisions += div
    assert divisions > 0


def test_radix_select_host_program_under_sanitizers(tmp_path):
    """tools/merge_select_check.cpp: the scalar logic the select kernels share (csrc/pb_merge_select.h), run serially on the CPU over the
    GPU test's edge-case inputs against a sort, as a stand-alone program built with AddressSanitizer and UBSan (host code only)."""
    import shutil
    import subprocess
    from pianobart_amd import build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which(build._hipcc()) or build._hipcc()
    near = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), 'lib', 'llvm', 'bin', 'clang++')
    cxx = near if os.path.exists(near) else (shutil.which('clang++') or shutil.which('g++') or shutil.which('c++'))
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'merge_select_check')
    r = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                        os.path.join(root, 'tools', 'merge_select_check.cpp'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith('ok') and r.stdout.count('21 selections equal the sort') == 6, (r.stdout[-1000:], r.stderr[-2000:])
