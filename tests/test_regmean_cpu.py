"""CPU: RegMean merging: what is decided before any device work (MergePlan / merge_state_dicts refusals, the command line, the argument
checks of the pb_regmean.hip entries), the workspace rule of pb_gram_accum, and the identities of the float64 restatement the GPU
tests measure against (tests/regmean_ref.py), and that restatement against the reference's own recorded regmean_merging results on a toy
classifier (tests/golden/g17_regmean.npz, written by tests/golden/make_regmean_goldens.py; no test reads the reference)."""
import ctypes
import os
import re
from collections import OrderedDict
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from pianobart_amd import _lib, merge as M
from pianobart_amd._lib import PBError
from tests import merge_ref, regmean_ref as R


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


# ---- the reference's recorded results (tests/golden/g17_regmean.npz) ------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g17_regmean.npz')
GOLDEN_NS = (2, 3)
GOLDEN_CASES = [(c, n) for n in GOLDEN_NS for c in ('r1', 'r09', 'r03', 'r0', 'r09x')]
CASE_IDS = ['%s-%d' % c for c in GOLDEN_CASES]
ULP = 2.0 ** -24
MARGIN = 4                                                   # another summation order: tests/test_row_kernels_gpu.py, the attention suite
_GOLDEN = {}


def golden():
    """The recording, read once and left unchanged: state dicts, per model {weight name: Gram matrix} (q and k, which read one input, hold ONE
    tensor, as merge.regmean_weights hands them over), and per (case, N) the ratio, the exclude list and the reference's output by name."""
    if _GOLDEN:
        return _GOLDEN['g']
    z = np.load(GOLDEN)                                      # allow_pickle is False: arrays only
    names = [str(n) for n in z['names']]
    shapes = {n: tuple(int(v) for v in sh if v) for n, sh in zip(names, z['shapes'])}
    segs = M.segment_table(shapes)

    def sd(flat, keep=None):
        keep = names if keep is None else keep
        sub = M.segment_table({n: shapes[n] for n in keep})
        assert flat.shape == (sub[-1].offset + sub[-1].numel,)
        return OrderedDict((s.name, torch.from_numpy(flat[s.offset:s.offset + s.numel].reshape(s.shape).copy())) for s in sub)

    modules, gram_of = [str(m) for m in z['modules']], [str(m) for m in z['gram_of']]
    grams = []
    for m in range(3):
        own = {k: torch.from_numpy(z['G/%d/%s' % (m, k)].copy()) for k in sorted(set(gram_of))}
        grams.append({mod + '.weight': own[key] for mod, key in zip(modules, gram_of)})
    ratio_of = dict(zip((str(c) for c in z['ratio_names']), (float(r) for r in z['ratios'])))
    ratio_of['r09x'] = ratio_of['r09']
    pattern = str(z['exclude'])
    cases = {}
    for case, n in GOLDEN_CASES:
        exclude = [pattern] if case == 'r09x' else []
        kept = [k for k in names if not any(re.match(p, k) for p in exclude)]
        cases[(case, n)] = SimpleNamespace(ratio=ratio_of[case], exclude=exclude, kept=kept, out=sd(z['out/%s/%d' % (case, n)], kept))
    _GOLDEN['g'] = SimpleNamespace(z=z, names=names, shapes=shapes, segs=segs, modules=modules, gram_of=gram_of, pre=sd(z['pre']), fts=[sd(f) for f in z['ft']],
                                   grams=grams, cases=cases, solved=[m + '.weight' for m in modules], W64={})
    return _GOLDEN['g']


def golden_truth(case, n, name):
    """(W64 = regmean_ref.merge64 on the recorded weights and Gram matrices, e(the reference's recorded output))."""
    g = golden()
    if (case, n, name) not in g.W64:
        W64 = R.merge64([f[name] for f in g.fts[:n]], [G[name] for G in g.grams[:n]], g.cases[(case, n)].ratio)
        g.W64[(case, n, name)] = (W64, rel_error(g.cases[(case, n)].out[name], W64))
    return g.W64[(case, n, name)]


def rel_error(W, W64):
    """e(W) = ||W - W64||_F / ||W64||_F in float64."""
    return float(torch.linalg.norm(W.double() - W64) / torch.linalg.norm(W64))


def gram_figure(G, batches):
    """(max over the elements of |G - G64| / (sum_t |x_ti x_tj| / rows), G64): G64 = X^T X / rows in float64 over exactly the rows given."""
    X = torch.cat([b.double() for b in batches])
    G64 = X.t() @ X / X.shape[0]
    scale = X.abs().t() @ X.abs() / X.shape[0]
    return float(((G.double() - G64).abs() / scale).max()), G64


def golden_activations():
    """[(module, the recorded Gram matrix, [x of every batch as the hook saw it, (rows, K)])] for the 3-D-input and the 2-D-input layer."""
    g = golden()
    z, m, T = g.z, int(g.z['act_model']), int(g.z['T'])
    out = []
    for key, per in (('act3', T), ('act2', 1)):
        module = str(z[key + '_module'])
        X, edges = torch.from_numpy(z[key].copy()), np.concatenate([[0], np.cumsum(z['act_batches'] * per)])
        out.append((module, g.grams[m][module + '.weight'], [X[a:b] for a, b in zip(edges[:-1], edges[1:])]))
    return out


def test_golden_file_holds_arrays_of_the_shapes_its_table_names():
    g = golden()
    z = g.z
    assert os.path.getsize(GOLDEN) < 512 * 1024
    n = g.segs[-1].offset + g.segs[-1].numel
    assert all(s.numel % 64 == 0 and len(s.shape) in (1, 2) for s in g.segs)
    assert z['pre'].shape == (n,) and z['ft'].shape == (3, n) and z['pre'].dtype == z['ft'].dtype == np.float32
    K_of = {m: g.shapes[m + '.weight'][1] for m in g.modules}
    assert g.modules == ['head', 'k', 'mid', 'q', 'wide'] and g.gram_of == ['head', 'q', 'mid', 'q', 'wide']
    assert K_of == {'head': 16, 'k': 12, 'mid': 64, 'q': 12, 'wide': 80}      # no multiple of 8; one 64-column block of the factorisation; more than one
    assert 'k.bias' not in g.names and 'q.bias' in g.names and 'emb.weight' in g.names and 'norm.weight' in g.names
    for m in range(3):
        for mod in set(g.gram_of):
            G = z['G/%d/%s' % (m, mod)]
            assert G.dtype == np.float32 and G.shape == (K_of[mod], K_of[mod])
        assert z['ids/%d' % m].dtype == np.int64 and z['ids/%d' % m].shape[1] == int(z['T'])
    for (case, N), c in g.cases.items():
        assert sum(v.numel() for v in c.out.values()) == z['out/%s/%d' % (case, N)].size and z['out/%s/%d' % (case, N)].dtype == np.float32
    assert z['act3'].dtype == z['act2'].dtype == np.float32
    assert z['act3'].shape == (int(z['act_batches'].sum()) * int(z['T']), K_of[str(z['act3_module'])])
    assert z['act2'].shape == (int(z['act_batches'].sum()), K_of[str(z['act2_module'])])
    assert len([k for k in z.files if k.startswith('out/')]) == len(GOLDEN_CASES)
    for k in z.files:
        assert z[k].dtype.kind in 'fiUb', (k, z[k].dtype)
        if z[k].dtype.kind == 'f':
            assert np.isfinite(z[k]).all(), k
    assert [R.factors(c.ratio) for c in g.cases.values()] == [(np.float32(c.ratio), np.float32(1.0)) for c in g.cases.values()]


@pytest.mark.parametrize('case,N', GOLDEN_CASES, ids=CASE_IDS)
def test_restatement_is_as_close_to_float64_as_the_recorded_reference(case, N):
    """Per solved weight e(W) = ||W - W64||_F / ||W64||_F. The float32 recipe of regmean_ref.py, run here, is held to 4 times the error of the
    reference's recorded output (a yardstick below one float32 ulp counts as that ulp) -- not bit for bit: the BLAS and the inverse of this
    machine need not be those of the generating run."""
    g = golden()
    c = g.cases[(case, N)]
    for name in g.solved:
        if name not in c.out:
            continue
        W64, e_rec = golden_truth(case, N, name)
        e_own = rel_error(R.merge32_recipe([f[name] for f in g.fts[:N]], [G[name] for G in g.grams[:N]], c.ratio), W64)
        print('%-5s N=%d %-12s K %3d: recorded reference %.3g, float32 recipe here %.3g' % (case, N, name, W64.shape[1], e_rec, e_own))
        assert e_own <= MARGIN * max(e_rec, ULP), (name, e_own, e_rec)


def test_recorded_gram_matrices_are_the_mean_over_the_recorded_rows():
    """G64 = X^T X / rows in float64 over exactly the recorded rows. The recorded matrix's figure max |G - G64| / (sum_t |x_ti x_tj| / rows) is
    the yardstick of the GPU test of pb_gram_accum on the same activations. It is held here to what the float formats allow the reference's
    running average: a float32 sum of at most `b` products per batch (b 2^-24 of the scale) and three roundings per batch for the multiply,
    add and divide of the average, every intermediate at most the scale in size: (b + 3 batches) 2^-24. Dividing by examples where the rows
    are examples x T, or by another count, is off by a factor."""
    g = golden()
    sym = dict(zip(g.modules, (bool(v) for v in g.z['symmetric'])))
    for module, G, batches in golden_activations():
        fig, G64 = gram_figure(G, batches)
        rows = sum(b.shape[0] for b in batches)
        assert rows == int(g.z['rows'][int(g.z['act_model'])][g.modules.index(module)])
        print('%-5s K %3d rows %4d in %d batches: recorded figure %.3g (= %.2f * 2^-24), exactly symmetric: %s' % (module, G.shape[0], rows, len(batches), fig,
                                                                                                            fig / ULP, sym[module]))
        assert fig <= (max(b.shape[0] for b in batches) + 3 * len(batches)) * ULP
        assert torch.equal(G, G.t()) == sym[module]
    for m in range(3):                                       # every recorded matrix is as symmetric as the generating run reported
        for name, G in g.grams[m].items():
            assert torch.equal(G, G.t()) == sym[name[:-len('.weight')]]


def test_recorded_row_counts_follow_the_stop_rule():
    """rows = examples x T where the hook saw (B, T, K), examples where it saw (B, K); the examples are the first total of whole batches (the
    last one of the data may be short) at or above nums_regmean_examples: one more batch after the count is passed, never a part of one.
    merge.regmean_pass counts by the same rule (`num_counted >= num_examples` before each batch, += the batch's actual size, rows B x S), but
    it cannot be exercised here: it runs the engine's forward and refuses any device but a HIP one (asserted below). Its counts are checked
    on the GPU by test_regmean_weights_match_the_oracle (batches of 4, 4, 2) and test_regmean_and_model_merge_command_lines (3 asked for in
    batches of 2: 4 counted)."""
    g = golden()
    z = g.z
    B, T = int(z['batch']), int(z['T'])
    assert len(set(z['examples'] % B)) > 1                   # a model whose last batch is short and one whose batches are all whole
    for m in range(3):
        have, asked = z['ids/%d' % m].shape[0], int(z['num_examples'][m])
        assert asked % B != 0
        totals = [min(i + B, have) for i in range(0, have, B)]
        assert int(z['examples'][m]) == next(t for t in totals if t >= asked)
        for mod, rows in zip(g.modules, z['rows'][m]):
            assert int(rows) == int(z['examples'][m]) * (1 if mod == str(z['act2_module']) else T), (m, mod)
    assert int(z['examples'][1]) < z['ids/1'].shape[0]       # the stop rule bites: data left unread
    assert np.array_equal(z['act_batches'], [B] * 8 + [6]) and int(z['act_model']) == 0
    with pytest.raises(PBError, match='no CPU'):
        M.regmean_pass(None, [], 10, True, device='cpu')


@pytest.mark.parametrize('case,N', GOLDEN_CASES, ids=CASE_IDS)
def test_recording_solves_linear_weights_and_averages_the_rest(case, N):
    """The names whose recorded output differs from the plain float32 mean of the recorded models are exactly the `.weight`s of the Linears
    that were not excluded; a solved layer's bias, the embedding and the LayerNorm equal the mean bit for bit; excluded names are absent."""
    g = golden()
    c = g.cases[(case, N)]
    excluded = [k for k in g.names if k not in c.kept]
    assert excluded == (['q.bias', 'q.weight'] if case == 'r09x' else []) and list(c.out) == c.kept
    mean = {k: torch.from_numpy(merge_ref.average([f[k].numpy() for f in g.fts[:N]])) for k in c.kept}
    differs = [k for k in c.kept if not torch.equal(c.out[k], mean[k])]
    assert differs == [k for k in g.solved if k in c.kept]
    assert all(c.out[k].numpy().tobytes() == mean[k].numpy().tobytes() for k in c.kept if k not in g.solved)
    assert 'head.bias' in c.kept and 'head.bias' not in differs
    for name in differs:                                     # and not by a rounding: the Gram matrices matter
        assert float((c.out[name] - mean[name]).abs().max()) > 1e-4 * float(mean[name].abs().max())
