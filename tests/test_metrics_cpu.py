"""CPU: the host half of the set metrics (pianobart_amd.metrics, eval_metrics) and the yardstick itself (tests/metrics_ref.py).

  * the restatement's own invariants: every histogram sums to its divisor column (pitched notes, pitch pairs, notes, notes, notes,
    distinct bars) at S = 1 (L = 0 and L = 1), 7, 65 and 1 024 with the specials mid-window, and hand-counted columns of a small piece;
  * tables() on the default dictionary and on the 2 470-id one, and what it refuses;
  * the host refusals: a CPU tensor ("no CPU path"), a bad shape, an id past its head (named);
  * overlap_and_kl, the degenerate rule, feature_groups against the restatement on the restatement's own integer table;
  * the C entries' argument checks (-2, the field named) and the CLI's refusals, none of which needs a device;
  * the ABI version is still 10 and the header's new entries are exported."""
import ctypes
import os

import numpy as np
import pytest
import torch

from pianobart_amd import _lib, metrics, ops
from pianobart_amd._lib import PBError
from tests import metrics_ref as R
from tests.vocab_layout_util import D_DEFAULT, D_WIDE, make_dict


def default_tables():
    return R.tables_for(D_DEFAULT, 128)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S', [1, 7, 65, 1024])
def test_reference_histograms_sum_to_their_divisors(S):
    pad8, pitch_of, dur_pos = default_tables()
    ids = R.synth_pieces(D_DEFAULT, 3 if S < 1024 else 2, S, seed=S)
    if S > 1:
        ids[1] = ids[0]                                # piece 0 fills the window
        ids[1, S // 2, 5] = pad8[5]                    # one special id, one head, mid-window
    f = R.features(ids, pad8, pitch_of, dur_pos)
    assert f[0, 0] == S and (S == 1 or f[1, 0] == S // 2)
    for col, width, div in [(16, 12, 1), (28, 144, 8), (172, 16, 0), (188, 32, 0), (220, 32, 0), (252, 32, 2)]:
        assert (f[:, col:col + width].sum(1) == f[:, div]).all(), (col, div)
    assert (f[:, 8] == np.maximum(f[:, 1] - 1, 0)).all() and (f[:, 14:16] == 0).all() and (f[:, 284:] == 0).all()
    assert (f[:, 9] >= (f[:, 0] > 0)).all() and (f[:, 10] <= np.maximum(f[:, 0] - 1, 0)).all()


def test_reference_at_one_row():
    pad8, pitch_of, dur_pos = default_tables()
    note = np.array([[[3, 17, 0, 60, 8, 20, 9, 30]]])
    f = R.features(note, pad8, pitch_of, dur_pos)[0]                       # L = 1
    assert list(f[:14]) == [1, 1, 1, 1, 1, 60, 60, 0, 0, 1, 0, int(dur_pos[8]), 20, 1]
    assert f[16 + 0] == 1 and f[172 + 1] == 1 and f[188 + 2] == 1 and f[220 + 20] == 1 and f[252] == 1 and f.sum() == sum(f[:14]) + 5
    eos = np.array([[pad8]]) + 3
    f = R.features(eos, pad8, pitch_of, dur_pos)[0]                        # L = 0
    assert list(f[:14]) == [0, 0, 0, 0, 0, -1, -1, 0, 0, 0, 0, 0, 0, 0] and f[14:].sum() == 0
    assert R.features(note, pad8, pitch_of, dur_pos, start=1)[0, 0] == 0   # start >= L


def test_reference_hand_counted_piece():
    pad8, pitch_of, dur_pos = default_tables()
    #        bar pos ins pitch dur vel
    rows = [(0, 0, 0, 60, 4, 10), (0, 0, 0, 64, 4, 10), (0, 16, 1, 130, 0, 31), (1, 0, 0, 62, 9, 5), (0, 48, 0, 62, 130 - 3, 0), (200, 1, 0, 0, 0, 0)]
    ids = np.array([[list(r) + [0, 0] for r in rows] + [[pad8[0]] + [0] * 7]])
    f = R.features(ids, pad8, pitch_of, dur_pos)[0]
    # notes 6, pitched 5 (id 130 is percussion), bars {0, 1, 200}, span 201, pitches {60, 64, 62, 0}, min 0, max 64
    assert list(f[:7]) == [6, 5, 3, 201, 4, 0, 64]
    assert (f[7], f[8]) == (4 + 2 + 0 + 62, 4)                             # 60 -> 64 -> (drum skipped) 62 -> 62 -> 0
    assert (f[9], f[10]) == (5, 1)                                         # one chord (rows 0, 1); one step back (bar 1 -> bar 0)
    assert f[13] == 2 and f[252 + 3] == 1 and f[252] == 2                  # bar 0 holds 4 notes, bars 1 and 200 one each
    assert f[28 + 12 * 0 + 4] == 1 and f[28 + 12 * 4 + 2] == 1 and f[28 + 12 * 2 + 2] == 1 and f[28 + 12 * 2 + 0] == 1


# ---- tables ---------------------------------------------------------------------------------------------------------------------------
def test_tables_default_dictionary():
    t = metrics.tables()
    pad8, pitch_of, dur_pos = default_tables()
    assert t.layout == ops.DEFAULT_LAYOUT and t.pitch_of.dtype == np.int16 and t.dur_pos.dtype == np.int32
    assert (t.pitch_of == pitch_of).all() and (t.dur_pos == dur_pos).all()
    assert t.pitch_of[127] == 127 and t.pitch_of[128] == -1 and t.dur_pos[16] == 16 and t.dur_pos[17] == 18


def test_tables_wide_dictionary_and_refusals():
    e2w, _ = make_dict(D_WIDE)
    t = metrics.tables(e2w)
    pad8, pitch_of, dur_pos = R.tables_for(D_WIDE, 0)
    assert sum(t.layout.sizes) == 2470 and list(t.layout.pad8) == pad8
    assert (t.pitch_of == pitch_of).all() and (t.dur_pos == dur_pos).all() and t.dur_pos[-1] == dur_pos[127] and len(t.dur_pos) == 294
    bad = {k: dict(v) for k, v in e2w.items()}
    del bad['Pitch']['Pitch 7']
    bad['Pitch']['Pitch drum 7'] = 7
    with pytest.raises(PBError, match="'Pitch drum 7'"):
        metrics.tables(bad)
    bad = {k: dict(v) for k, v in e2w.items()}
    del bad['Pitch']['Pitch 7']
    bad['Pitch']['Pitch 5000'] = 7
    with pytest.raises(PBError, match='Pitch 5000'):
        metrics.tables(bad)
    with pytest.raises(PBError, match='Layout'):
        metrics.tables({'Pitch': {}})


# ---- host refusals ----------------------------------------------------------------------------------------------------------------------
def test_cpu_tensors_are_refused():
    ids = torch.zeros(2, 4, 8, dtype=torch.int64)
    with pytest.raises(PBError, match='no CPU path'):
        metrics.piece_features(ids)
    x = torch.zeros(3, 4)
    for call in (lambda: ops.pairwise_l2(x, x), lambda: ops.sample_moments(x), lambda: ops.kde_eval(x, torch.zeros(5), 1.0),
                 lambda: ops.piece_features(torch.zeros(2, 4, 8, dtype=torch.int16), torch.zeros(256, dtype=torch.int16), torch.zeros(128, dtype=torch.int32))):
        with pytest.raises(PBError, match='no CPU path'):
            call()


@pytest.mark.parametrize('shape', [(4, 8), (2, 4, 7), (2, 0, 8), (2, 2, 4, 8)])
def test_bad_shapes_are_refused(shape):
    with pytest.raises(PBError, match=r'\(N, S, 8\)'):
        metrics.piece_features(np.zeros(shape, dtype=np.int64))


@pytest.mark.parametrize('head,value', [(0, 262), (3, 300), (5, 38), (7, -1)])
def test_an_id_past_its_head_is_refused_by_name(head, value):
    ids = np.zeros((2, 4, 8), dtype=np.float32)
    ids[1, 2, head] = value
    with pytest.raises(PBError, match=r'head %d \(%s\)' % (head, ops.CLASS_NAMES[head])):
        metrics.piece_features(ids)
    with pytest.raises(PBError, match='not integers'):
        metrics.piece_features(np.full((1, 2, 8), 0.5, dtype=np.float32))


def test_start_is_checked():
    ids = np.zeros((3, 4, 8), dtype=np.int64)
    for start in (-1, [0, 1], 1.5):
        with pytest.raises(PBError, match='start'):
            metrics._host_start(start, ids.shape[0])
    assert list(metrics._host_start(2, 3)) == [2, 2, 2] and list(metrics.piece_lengths(ids, start=[0, 3, 9])) == [4, 1, 0]


# ---- host arithmetic ----------------------------------------------------------------------------------------------------------------------
def test_overlap_and_kl():
    x = np.linspace(-6, 6, 1201)
    dx = x[1] - x[0]
    p = np.exp(-x * x / 2) / np.sqrt(2 * np.pi)
    integral = float(dx * (p.sum() - 0.5 * (p[0] + p[-1])))
    oa, kl = metrics.overlap_and_kl(p, p, dx)
    assert oa == integral and abs(oa - 1.0) < 1e-8 and kl == 0.0
    a, b = np.where(x < -1, 1.0, 0.0), np.where(x > 1, 1.0, 0.0)
    oa, kl = metrics.overlap_and_kl(a, b, dx)
    assert oa == 0.0 and kl > 600.0                                        # disjoint supports: log(1 / 1e-300) over a length of 5
    q = np.exp(-(x - 1) ** 2 / 2) / np.sqrt(2 * np.pi)
    oa, kl = metrics.overlap_and_kl(p, q, dx)
    ro, rk = R.overlap_kl(p, q, dx)
    assert abs(oa - ro) < 1e-12 and abs(kl - rk) < 1e-12 and abs(kl - 0.5) < 1e-6     # KL of two unit normals one apart = 1 / 2
    with pytest.raises(PBError):
        metrics.overlap_and_kl(p, q[:-1], dx)


def test_degenerate_rule():
    rec = lambda v: [len(v), sum(v), sum(x * x for x in v), 0.0, min(v, default=np.inf), max(v, default=-np.inf)]
    ok, one, flat, none = (metrics.sample_stats(rec(v)) for v in ([1.0, 2.0, 4.0], [3.0], [2.5, 2.5, 2.5], []))
    assert ok['n'] == 3 and abs(ok['std'] - np.std([1, 2, 4], ddof=1)) < 1e-15 and abs(metrics.scott_bandwidth(ok) - ok['std'] * 3 ** -0.2) < 1e-15
    assert np.isnan(one['std']) and flat['std'] == 0.0 and none['n'] == 0 and np.isnan(none['mean'])
    assert metrics.densities_defined([ok, ok, ok])
    for bad in (one, flat, none):
        assert not metrics.densities_defined([ok, bad, ok])


def test_feature_groups_against_the_restatement():
    pad8, pitch_of, dur_pos = default_tables()
    ids = R.synth_pieces(D_DEFAULT, 6, 40, seed=3)
    ids[2, 0] = np.asarray(pad8) + 3                                       # an empty piece
    ids[4, :, 3] = 200                                                     # all percussion: zero divisors
    f = R.features(ids, pad8, pitch_of, dur_pos)
    got, empty = metrics.feature_groups(f)
    want, want_empty = R.groups(f)
    assert empty == want_empty == 1 and list(got) == list(metrics.GROUPS) and len(got) == 14 and set(got) == set(want)
    for k in got:
        assert got[k].dtype == np.float32 and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    assert got['pch'][3].sum() == 0 and got['pitch_range'][3] == 0 and got['avg_interval'][3] == 0
    with pytest.raises(PBError):
        metrics.feature_groups(np.zeros((2, 100)))


# ---- the C entries' own checks (no device needed) -------------------------------------------------------------------------------------
PTR = 0x10000
_PAD8 = (ctypes.c_int32 * 8)(*ops.DEFAULT_LAYOUT.pad8)
_WIDE_PAD8 = (ctypes.c_int32 * 8)(1100, 128, 129, 256, 128, 32, 254, 49)
_ENTRY_REFUSALS = [
    ('pb_piece_features', (PTR + 2, None, _PAD8, PTR, PTR, PTR, 4, 16, None), 'ids16'),
    ('pb_piece_features', (PTR, None, _PAD8, None, PTR, PTR, 4, 16, None), 'pitch_of'),
    ('pb_piece_features', (PTR, None, _PAD8, PTR, PTR, None, 4, 16, None), 'feat'),
    ('pb_piece_features', (PTR, None, _PAD8, PTR, PTR, PTR, 4, 0, None), 'S = 0'),
    ('pb_piece_features', (PTR, None, _PAD8, PTR, PTR, PTR, -1, 16, None), 'N = -1'),
    ('pb_piece_features', (PTR, None, _WIDE_PAD8, PTR, PTR, PTR, 4, 16, None), 'pad8[0] = 1100'),
    ('pb_pairwise_l2', (PTR, PTR, None, 4, 4, 8, None), 'D'),
    ('pb_pairwise_l2', (PTR, PTR, PTR + 64, 4, 4, 145, None), 'F = 145'),
    ('pb_pairwise_l2', (PTR, PTR, PTR + 64, 4, 4, 0, None), 'F = 0'),
    ('pb_pairwise_l2', (PTR, PTR, PTR + 64, 0, 4, 8, None), 'N = 0'),
    ('pb_pairwise_l2', (PTR, PTR + 64, PTR, 4, 4, 8, None), 'aliases'),
    ('pb_sample_moments', (PTR, 4, 5, 1, PTR, PTR, None), 'upper needs N == M'),
    ('pb_sample_moments', (PTR, 4, 4, 2, PTR, PTR, None), 'upper = 2'),
    ('pb_sample_moments', (PTR, 4, 4, 0, None, PTR, None), 'out'),
    ('pb_sample_moments', (PTR, 4, 4, 0, PTR, None, None), 'ws'),
    ('pb_kde_eval', (PTR, 4, 4, 0, PTR, 4097, 1.0, PTR, PTR, None), 'G = 4097'),
    ('pb_kde_eval', (PTR, 4, 4, 0, PTR, 0, 1.0, PTR, PTR, None), 'G = 0'),
    ('pb_kde_eval', (PTR, 4, 4, 0, PTR, 64, 0.0, PTR, PTR, None), 'h = 0'),
    ('pb_kde_eval', (PTR, 4, 4, 0, PTR, 64, float('nan'), PTR, PTR, None), 'h = nan'),
    ('pb_kde_eval', (PTR, 1, 1, 1, PTR, 64, 1.0, PTR, PTR, None), 'no samples'),
    ('pb_kde_eval', (PTR, 4, 4, 0, None, 64, 1.0, PTR, PTR, None), 'grid'),
    ('pb_kde_eval', (PTR, 4, 4, 0, PTR, 64, 1.0, None, PTR, None), 'dens'),
]


@pytest.mark.parametrize('entry,args,names', _ENTRY_REFUSALS, ids=['%s-%s' % (e, n) for e, _, n in _ENTRY_REFUSALS])
def test_entries_check_their_arguments_before_any_device_call(entry, args, names):
    with pytest.raises(PBError) as e:
        _lib.LIB.call(entry, *args)
    assert entry in str(e.value) and '(-2)' in str(e.value) and names in str(e.value), str(e.value)


def test_abi_version_is_still_10_and_the_entries_are_exported():
    decls = _lib.parse_header()
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert decls['pb_piece_features'] == (ctypes.c_int, [vp] * 6 + [i32, i32, vp])
    assert decls['pb_pairwise_l2'] == (ctypes.c_int, [vp] * 3 + [i32] * 3 + [vp])
    assert decls['pb_sample_moments'] == (ctypes.c_int, [vp, i64, i64, i32, vp, vp, vp])
    assert decls['pb_kde_eval'] == (ctypes.c_int, [vp, i64, i64, i32, vp, i32, ctypes.c_double, vp, vp, vp])
    assert decls['pb_metrics_ws_bytes'] == (i64, [i64, i64, i32])
    assert _lib.LIB.query('pb_abi_version') == 10
    q = lambda *a: _lib.LIB.query('pb_metrics_ws_bytes', *a)
    assert q(1, 1, 1) == 1024 * 5 * 8                                      # the moments' partial rows
    assert q(2048, 2048, 1024) == 1024 * 1024 * 8 and q(2048, 2048, 4096) == 256 * 4096 * 8 and q(128, 128, 1024) == 16 * 1024 * 8
    assert q(0, 4, 4) == 0


# ---- the CLI ----------------------------------------------------------------------------------------------------------------------------
def _files(tmp_path, gen, ref):
    g, r = str(tmp_path / 'g.npy'), str(tmp_path / 'r.npy')
    np.save(g, gen)
    np.save(r, ref)
    return ['--generated', g, '--reference', r, '--output', str(tmp_path / 'm.json')]


def test_cli_refusals(tmp_path):
    from pianobart_amd import eval_metrics
    ok = R.synth_pieces(D_DEFAULT, 4, 12, seed=1).astype(np.float32)
    argv = _files(tmp_path, ok, ok)
    with pytest.raises(PBError, match='--cpu'):
        eval_metrics.main(argv + ['--cpu'])
    with pytest.raises(PBError, match='no file'):
        eval_metrics.main(['--generated', str(tmp_path / 'missing.npy')] + argv[2:])
    with pytest.raises(PBError, match='no file'):
        eval_metrics.main(argv + ['--dict_file', str(tmp_path / 'missing.json')])
    with pytest.raises(PBError, match='rows of 8 ids'):
        eval_metrics.main(_files(tmp_path, ok[:, :, :7], ok))
    with pytest.raises(PBError, match='rows of 8 ids'):
        eval_metrics.main(_files(tmp_path, ok, ok[0, 0]))
    for flags in (['--grid', '1'], ['--grid', '5000'], ['--skip', '-1'], ['--max_pieces', '0']):
        with pytest.raises(PBError, match=flags[0]):
            eval_metrics.main(argv + flags)
    empty = ok.copy()
    empty[1:, 0] = np.asarray(ops.DEFAULT_LAYOUT.pad8) + 3                 # one piece with notes left
    with pytest.raises(PBError, match=r'--generated holds 1 pieces'):
        eval_metrics.main(_files(tmp_path, empty, ok))
    with pytest.raises(PBError, match=r'--reference holds 1 pieces'):
        eval_metrics.main(_files(tmp_path, ok, empty))
    with pytest.raises(PBError, match=r'--generated holds 0 pieces'):
        eval_metrics.main(_files(tmp_path, ok, ok) + ['--skip', '12'])
    with pytest.raises(PBError, match=r'--generated holds 1 pieces'):
        eval_metrics.main(_files(tmp_path, ok, ok) + ['--max_pieces', '1'])
    assert not os.path.exists(str(tmp_path / 'm.json'))


def test_cli_flattens_samples(tmp_path):
    from pianobart_amd import eval_metrics
    a = np.arange(2 * 3 * 5 * 8).reshape(2, 3, 5, 8)
    p = str(tmp_path / 'a.npy')
    np.save(p, a)
    flat = eval_metrics.load_pieces(p, '--generated')
    assert flat.shape == (6, 5, 8) and np.array_equal(flat[4], a[1, 1]) and eval_metrics.load_pieces(p, '--generated', 4).shape == (4, 5, 8)
