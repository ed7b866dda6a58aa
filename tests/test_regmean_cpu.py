"""CPU: RegMean merging: what is decided before any device work (MergePlan / merge_state_dicts refusals, the command line, the argument
checks of the pb_regmean.hip entries), the workspace rule of pb_gram_accum, and the identities of the float64 restatement the GPU
tests measure against (tests/regmean_ref.py)."""
import ctypes

import numpy as np
import pytest
import torch

from pianobart_amd import _lib, merge as M
from pianobart_amd._lib import PBError
from tests import regmean_ref as R


def _sd(seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return {'b.weight': torch.randn(3, 5, generator=g) * scale, 'a.bias': torch.randn(7, generator=g) * scale, 'c.k': torch.randn(2, 3, 4, generator=g) * scale}


def _rw(seed=0):
    return {'b.weight': R.gram_inputs(5, 16, 1, seed)[0]}


def test_plan_accepts_regmean_weights():
    p = M.MergePlan(2, method='regmean_merging', regmean_weights=[_rw(1), _rw(2)])
    assert p.regmean and not p.fisher and not p.masked and p.ratio == 1.0
    p = M.MergePlan(3, method='regmean_merging', regmean_weights=[_rw(1), _rw(2), _rw(3)], reduce_non_diagonal_ratio=0.9, exclude='a')
    assert p.ratio == 0.9 and p.exclude == ['a']
    assert not M.MergePlan(2, method='average_merging').regmean


def test_refusals_come_before_device_work():
    """None of these reaches a device: they pass on a machine without one."""
    reg = dict(method='regmean_merging')
    with pytest.raises(PBError, match=r'regmean_merging.*pianobart_amd\.regmean'):
        M.merge_state_dicts(_sd(), [_sd(1), _sd(2)], **reg)
    with pytest.raises(PBError, match='regmean_merging'):
        M.merge_state_dicts(_sd(), [_sd(1), _sd(2)], mask_apply_method='regmean_merging', regmean_weights=[_rw(1), _rw(2)])
    with pytest.raises(PBError, match='regmean'):
        M.merge_state_dicts(_sd(), [_sd(1), _sd(2)], method='regmean', regmean_weights=[_rw(1), _rw(2)])
    with pytest.raises(PBError, match='1 sets of Gram matrices for 2 models'):
        M.merge_state_dicts(_sd(), [_sd(1), _sd(2)], regmean_weights=[_rw(1)], **reg)
    with pytest.raises(PBError, match='non-empty'):
        M.merge_state_dicts(_sd(), [_sd(1), _sd(2)], regmean_weights=[_rw(1), {}], **reg)
    bad = _rw(2)
    bad['d.weight'] = torch.eye(5)
    with pytest.raises(PBError, match='no merged parameter.*d.weight'):
        M.merge_state_dicts(_sd(), [_sd(1), _sd(2)], regmean_weights=[_rw(1), bad], **reg)
    with pytest.raises(PBError, match='no merged parameter.*b.weight'):        # excluded: not merged
        M.merge_state_dicts(_sd(), [_sd(1), _sd(2)], regmean_weights=[_rw(1), _rw(2)], exclude=['b'], **reg)
    two = dict(_sd(), **{'e.weight': torch.zeros(2, 5)})
    more = dict(_rw(2), **{'e.weight': torch.eye(5)})
    with pytest.raises(PBError, match='different parameters.*e.weight'):
        M.merge_state_dicts(two, [two, two], regmean_weights=[_rw(1), more], **reg)
    with pytest.raises(PBError, match='a.bias is not the 2-D weight'):
        M.merge_state_dicts(_sd(), [_sd(1), _sd(2)], regmean_weights=[{'a.bias': torch.eye(7)}, {'a.bias': torch.eye(7)}], **reg)
    for wrong in (torch.eye(3), torch.eye(5).double(), torch.zeros(5, 4), torch.zeros(25), 'x'):
        with pytest.raises(PBError, match=r'b.weight is .*expected a float32 \(5, 5\)'):
            M.merge_state_dicts(_sd(), [_sd(1), _sd(2)], regmean_weights=[_rw(1), {'b.weight': wrong}], **reg)
    for value in (float('inf'), float('nan')):
        bad = _rw(2)
        bad['b.weight'][1, 2] = bad['b.weight'][2, 1] = value
        with pytest.raises(PBError, match='non-finite'):
            M.merge_state_dicts(_sd(), [_sd(1), _sd(2)], regmean_weights=[_rw(1), bad], **reg)
    bad = _rw(2)
    bad['b.weight'][1, 2] += 2e-6 * float(bad['b.weight'].diagonal().max())
    with pytest.raises(PBError, match='not symmetric'):
        M.merge_state_dicts(_sd(), [_sd(1), _sd(2)], regmean_weights=[_rw(1), bad], **reg)
    for value in (-1e-9, 1.0 + 1e-9, float('nan'), float('inf')):
        with pytest.raises(PBError, match='reduce_non_diagonal_ratio'):
            M.merge_state_dicts(_sd(), [_sd(1), _sd(2)], regmean_weights=[_rw(1), _rw(2)], reduce_non_diagonal_ratio=value, **reg)
    with pytest.raises(PBError, match='at least two'):
        M.merge_state_dicts(_sd(), [_sd(1)], regmean_weights=[_rw(1)], **reg)


def test_command_line_flags_are_absent_unless_given():
    from pianobart_amd.model_merge import get_args_merge
    from pianobart_amd.regmean import get_args_regmean
    a = vars(get_args_merge([]))
    assert 'regmean' not in a and 'reduce_non_diagonal_ratio' not in a and 'fisher' not in a and a['method'] == 'mask_merging'
    a = get_args_merge(['--method', 'regmean_merging', '--regmean', 'a.regmean.pt,b.regmean.pt', '--reduce_non_diagonal_ratio', '0.9'])
    assert (a.method, a.regmean, a.reduce_non_diagonal_ratio) == ('regmean_merging', 'a.regmean.pt,b.regmean.pt', 0.9)
    r = get_args_regmean(['--ckpt', 'ft.ckpt', '--task', 'composer', '--dataset', 'Pianist8', '--output', 'a.regmean.pt'])
    assert (r.num_examples, r.batch_size, r.precision, r.class_num, r.hs, r.layers) == (256, 8, 'bf16', 8, 1024, 8)
    with pytest.raises(PBError, match='positive'):
        get_args_regmean(['--ckpt', 'x', '--task', 'melody', '--dataset', 'POP909', '--output', 'o', '--num_examples', '0'])


def test_model_merge_refuses_regmean_without_files(tmp_path):
    from pianobart_amd.model_merge import model_merge
    with pytest.raises(PBError, match=r'regmean_merging.*pianobart_amd\.regmean'):
        model_merge(['--method', 'regmean_merging', '--model_path', 'a.ckpt,b.ckpt'])
    with pytest.raises(PBError, match='reduce_non_diagonal_ratio'):
        model_merge(['--method', 'regmean_merging', '--model_path', 'a.ckpt,b.ckpt', '--regmean', 'a.pt,b.pt', '--reduce_non_diagonal_ratio', '1.5'])


def test_factors_are_float32_and_match_the_restatement():
    for ratio in (1.0, 0.9, 0.5, 0.0, 0.3, 0.7, 1e-3):
        off, diag = M.regmean_factors(ratio)
        r_off, r_diag = R.factors(ratio)
        assert np.float32(off) == off == r_off and np.float32(diag) == diag == r_diag


def test_entries_are_declared_and_check_their_arguments_first():
    """-2 with the field's name before any HIP call: dummy addresses are never dereferenced."""
    decls = _lib.parse_header()
    for name in ('pb_gram_ws_bytes', 'pb_gram_accum', 'pb_regmean_scale', 'pb_chol_factor', 'pb_chol_solve', 'pb_transpose_f32'):
        assert name in decls
    a, b, c = (ctypes.c_void_p(v) for v in (0x10000, 0x20000, 0x30000))
    call = _lib.LIB.call
    for args, what in (((a, 8, 2, 4, 8, b, 8, c, None), 'dtype'), ((a, 8, 1, 0, 8, b, 8, c, None), 'T = 0'), ((a, 8, 1, 4, 0, b, 8, c, None), 'K = 0'),
                       ((a, 7, 1, 4, 8, b, 8, c, None), 'ldx = 7'), ((a, 8, 1, 4, 8, b, 7, c, None), 'ldg = 7'), ((None, 8, 1, 4, 8, b, 8, c, None), 'X must'),
                       ((a, 8, 1, 4, 8, None, 8, c, None), 'G must'), ((a, 8, 1, 4, 8, b, 8, ctypes.c_void_p(0x30004), None), 'ws must'),
                       ((a, 8, 0, 4, 8, a, 8, c, None), 'distinct')):
        with pytest.raises(PBError, match=what):
            call('pb_gram_accum', *args)
    for args, what in (((a, 8, b, 8, 0, 1.0, 1.0, None), 'K = 0'), ((a, 7, b, 8, 8, 1.0, 1.0, None), 'ldg = 7'), ((None, 8, b, 8, 8, 1.0, 1.0, None), 'non-NULL'),
                       ((a, 8, a, 9, 8, 1.0, 1.0, None), 'aliases')):
        with pytest.raises(PBError, match=what):
            call('pb_regmean_scale', *args)
    for args, what in (((a, 8, 0, b, None), 'K = 0'), ((a, 7, 8, b, None), 'ld = 7'), ((None, 8, 8, b, None), 'A must'), ((a, 8, 8, None, None), 'info must')):
        with pytest.raises(PBError, match=what):
            call('pb_chol_factor', *args)
    for args, what in (((a, 8, 0, b, 4, 4, None), 'K = 0'), ((a, 8, 8, b, 4, 0, None), 'nrhs = 0'), ((a, 7, 8, b, 4, 4, None), 'ldl = 7'),
                       ((a, 8, 8, b, 3, 4, None), 'ldr = 3'), ((a, 8, 8, None, 4, 4, None), 'non-NULL'), ((a, 8, 8, a, 8, 4, None), 'aliases')):
        with pytest.raises(PBError, match=what):
            call('pb_chol_solve', *args)
    for args, what in (((a, 8, b, 8, 0, 4, None), 'rows = 0'), ((a, 3, b, 8, 8, 4, None), 'lds = 3'), ((a, 4, b, 7, 8, 4, None), 'ldd = 7'), ((a, 4, a, 8, 8, 4, None), 'aliases')):
        with pytest.raises(PBError, match=what):
            call('pb_transpose_f32', *args)


def test_gram_workspace_is_a_function_of_the_sizes():
    """128 x 128 f32 slots: one per (tile on or below the diagonal, chunk of T). T is cut into at most ceil(T / 256) chunks of whole 64-row
    stages, as many as bring the grid to 512 workgroups."""
    q = lambda T, K: _lib.LIB.query('pb_gram_ws_bytes', T, K)
    slot = 128 * 128 * 4
    assert [q(T, 64) // slot for T in (1, 255, 256, 257, 512, 513, 1000)] == [1, 1, 1, 2, 2, 3, 4]
    assert [q(64, K) // slot for K in (1, 128, 129, 256, 257, 264)] == [1, 1, 3, 3, 6, 6]
    assert q(8192, 768) == 21 * 22 * slot                # 25 chunks wanted: 328 rows -> 384 (whole stages) -> 22 chunks
    assert q(8192, 3072) == 300 * 2 * slot and q(8192, 4096) == 528 * slot
    assert q(0, 8) == 0 and q(8, 0) == 0


def test_restatement_identities():
    """Identical Gram matrices in every model and ratio 1: the mean of the weights; one model: that model's weight."""
    g = torch.Generator().manual_seed(0)
    G = R.gram_inputs(24, 96, 1, 3)[0]
    Ws = [torch.randn(7, 24, generator=g) for _ in range(3)]
    mean = sum(W.double() for W in Ws) / 3
    assert float((R.merge64(Ws, [G, G, G]) - mean).abs().max()) < 1e-12
    assert float((R.merge32_recipe(Ws, [G, G, G]) - mean).abs().max()) < 1e-4
    for ratio in (1.0, 0.9):
        assert float((R.merge64(Ws[:1], [G], ratio) - Ws[0].double()).abs().max()) < 1e-12
    Gs = R.gram_inputs(24, 96, 3, 4)
    assert float((R.merge64(Ws, Gs) - mean).abs().max()) > 1e-4              # different inputs: no longer the mean
    assert all(torch.equal(G, G.t()) for G in Gs)
    assert torch.equal(R.scale32(G, 1.0), G) and torch.equal(R.scale32(G, 0.0), torch.diag(G.diagonal()))
    S, Rm = R.solve_case(33, 7, 66, 0.9, 5)
    e_inv, e_chol = R.yardsticks(S, Rm)
    assert 0 < e_inv < 1e-6 and 0 < e_chol < 1e-6
