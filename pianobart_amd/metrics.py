"""Set metrics for generated pieces: does a generated SET look like the data? The protocol of Yang & Lerch, "On the evaluation of
generative models in music": per-piece musical features, the pairwise distances inside each set and between the sets, a Gaussian kernel
density estimate of each distance sample, and from those the KL divergence and the overlapped area of intra-set and inter-set distances.

The features (pb_piece_features), the N x M distances (pb_pairwise_l2), their moments (pb_sample_moments) and the n x G Gaussian terms
(pb_kde_eval) run in pb_metrics.hip; the host divides integer columns, picks bandwidths and integrates G-point curves.
There is no CPU path. The reference's own quality line (the `shapesimilarity` "FAD" of its GenerationTrainer) needs a third-party
package this project does not have and stays `n/a`; this module does not stand in for it, it measures something else."""
from collections import OrderedDict

import numpy as np
import torch

from . import ops, pieces
from ._lib import PBError
from .pieces import Tables, tables
from .pieces import host_start as _host_start      # noqa: F401 (the name metrics has always had for it)

SCALAR_GROUPS = ('note_count', 'pitch_count', 'pitch_range', 'avg_interval', 'notes_per_bar', 'avg_duration', 'avg_velocity', 'onset_ratio')
# histogram groups: (first column, width, divisor column)
HIST_GROUPS = OrderedDict([('pch', (16, 12, 1)), ('pctm', (28, 144, 8)), ('beat_grid', (172, 16, 0)), ('duration_hist', (188, 32, 0)),
                           ('velocity_hist', (220, 32, 0)), ('bar_density_hist', (252, 32, 2))])
GROUPS = SCALAR_GROUPS + tuple(HIST_GROUPS)
SET_STAGES = ('distances', 'moments', 'kde')     # the timed stages of compare_group, behind a family's per-piece stage


def piece_lengths(ids, layout=None, start=None):
    """Host: the number of notes of every piece of an (N, S, 8) integer array (pieces.live_rows), 0 where start lies at or behind its end."""
    return pieces.live_rows(ids, layout, start)[1].sum(1)


def piece_features(ids, e2w=None, start=None, device=None):
    """The (N, 288) int32 device tensor of pb_piece_features for (N, S, 8) ids: integer or integer-valued float arrays or device tensors
    (eval_generation writes float32). Every id is checked on the host against its head's size (PBError names the head). start: the
    first row that counts, one number or one per piece (e.g. the prime length). e2w: a dictionary, None (the default one) or tables()."""
    tab = tables(e2w)
    return ops.piece_features(**pieces.upload(ids, tab, start, device, dur_pos=tab.dur_pos))


def _ratio(num, den):
    out = np.zeros(np.broadcast(num, den).shape, dtype=np.float64)
    np.divide(num, den, out=out, where=den != 0)
    return out


def feature_groups(feat):
    """(groups, empty): the 14 feature groups of an (N, 288) feature tensor or array as float32 arrays, (n,) for the scalar groups and
    (n, width) for the histograms, over the n pieces that hold a note; empty = the number of pieces left out. Divisions in float64,
    a zero divisor gives zeros."""
    f = (feat.detach().cpu().numpy() if torch.is_tensor(feat) else np.asarray(feat)).astype(np.float64)
    if f.ndim != 2 or f.shape[1] != ops.FEATURE_COLS:
        raise PBError('feature_groups: need an (N, %d) feature array (got %s)' % (ops.FEATURE_COLS, f.shape))
    keep = f[:, 0] > 0
    empty = int((~keep).sum())
    f = f[keep]
    c = lambda i: f[:, i]
    g = OrderedDict()
    g['note_count'] = c(0)
    g['pitch_count'] = c(4)
    g['pitch_range'] = np.where(c(1) > 0, c(6) - c(5), 0.0)
    g['avg_interval'] = _ratio(c(7), c(8))
    g['notes_per_bar'] = _ratio(c(0), c(2))
    g['avg_duration'] = _ratio(c(11), c(0))
    g['avg_velocity'] = _ratio(c(12), c(0))
    g['onset_ratio'] = _ratio(c(9), c(0))
    for name, (col, width, div) in HIST_GROUPS.items():
        g[name] = _ratio(f[:, col:col + width], f[:, div:div + 1])
    return OrderedDict((k, v.astype(np.float32)) for k, v in g.items()), empty


def overlap_and_kl(p, q, dx):
    """Host, float64, trapezoid rule on a uniform grid of spacing dx: (oa, kl) with oa = the integral of min(p, q) and
    kl = KL(p || q) = the integral of p log(p / q), q floored at 1e-300 and points with p = 0 contributing nothing."""
    p, q = np.asarray(p, dtype=np.float64), np.asarray(q, dtype=np.float64)
    if p.shape != q.shape or p.ndim != 1:
        raise PBError('overlap_and_kl: two curves on one grid (got %s and %s)' % (p.shape, q.shape))
    trap = lambda y: float(dx * (y.sum() - 0.5 * (y[0] + y[-1]))) if y.size > 1 else 0.0
    with np.errstate(divide='ignore', invalid='ignore'):
        integrand = np.where(p > 0, p * (np.log(np.where(p > 0, p, 1.0)) - np.log(np.maximum(q, 1e-300))), 0.0)
    return trap(np.minimum(p, q)), trap(integrand)


def sample_stats(mom):
    """n, mean, std (ddof = 1), min, max of a pb_sample_moments record on the host. std is 0 when min == max, nan below two samples."""
    n, s, q, _, lo, hi = (float(v) for v in mom)
    if n < 1:
        return dict(n=0, mean=float('nan'), std=float('nan'), min=float('nan'), max=float('nan'))
    mean = s / n
    std = float('nan') if n < 2 else 0.0 if lo == hi else float(np.sqrt(max(q - s * s / n, 0.0) / (n - 1)))
    return dict(n=int(n), mean=mean, std=std, min=lo, max=hi)


def scott_bandwidth(stat):
    return stat['std'] * stat['n'] ** -0.2


def densities_defined(stats):
    """The degenerate rule: a density needs at least two samples with some spread, in every one of the samples compared."""
    return all(st['n'] >= 2 and st['std'] > 0 for st in stats)


def compare_group(xg, xr, G, ws, timer, dev):
    """One feature group of compare_sets: xg (n_gen, F) and xr (n_ref, F) float32 host rows -> the record of means, stds, distance means,
    kl and oa (see compare_sets). ws: ops.metrics_ws for the larger set and G grid points; timer: a pieces.Timer with SET_STAGES."""
    n_gen, n_ref = len(xg), len(xr)
    res = OrderedDict()
    for tag, x in (('gen', xg), ('ref', xr)):
        v = np.sqrt((x.astype(np.float64) ** 2).sum(1)) if x.shape[1] > 1 else x[:, 0].astype(np.float64)
        res['mean_' + tag] = float(v.mean()) if v.size else float('nan')
        res['std_' + tag] = float(v.std()) if v.size else float('nan')
    for k in ('dist_gen', 'dist_ref', 'dist_inter', 'kl', 'oa', 'kl_gen', 'oa_gen'):
        res[k] = float('nan')
    if n_gen < 1 or n_ref < 1:
        return res
    tg, tr = torch.from_numpy(np.ascontiguousarray(xg)).to(dev), torch.from_numpy(np.ascontiguousarray(xr)).to(dev)
    samples = OrderedDict()                           # name -> (distance matrix, upper)
    if n_gen >= 2:
        samples['gen'] = (timer.run('distances', ops.pairwise_l2, tg, tg), True)
    if n_ref >= 2:
        samples['ref'] = (timer.run('distances', ops.pairwise_l2, tr, tr), True)
    samples['inter'] = (timer.run('distances', ops.pairwise_l2, tg, tr), False)
    moms = torch.stack([timer.run('moments', ops.sample_moments, D, up, ws) for D, up in samples.values()]).cpu().numpy()
    stats = OrderedDict((k, sample_stats(m)) for k, m in zip(samples, moms))
    for k, st in stats.items():
        res['dist_' + k] = st['mean']
    if len(stats) < 3 or not densities_defined(stats.values()):
        return res                                    # no density of a sample without spread: kl and oa stay nan
    hs = OrderedDict((k, scott_bandwidth(st)) for k, st in stats.items())
    h_max = max(hs.values())
    lo, hi = min(st['min'] for st in stats.values()) - 3 * h_max, max(st['max'] for st in stats.values()) + 3 * h_max
    pts = torch.from_numpy(np.linspace(lo, hi, G).astype(np.float32)).to(dev)
    dens = torch.stack([timer.run('kde', ops.kde_eval, D, pts, hs[k], up, ws) for k, (D, up) in samples.items()]).cpu().numpy()
    dx = (hi - lo) / (G - 1)
    p = dict(zip(samples, dens))
    res['oa'], res['kl'] = overlap_and_kl(p['ref'], p['inter'], dx)
    res['oa_gen'], res['kl_gen'] = overlap_and_kl(p['gen'], p['inter'], dx)
    return res


def compare_pieces(who, stage, op, grouping, names, gen_ids, ref_ids, tab, grid, start, device, left_out='short', profile=None, **arrays):
    """The set comparison every family ends in. Per piece of both sets op(**pieces.upload(..)) (timed as `stage`) gives integer columns,
    grouping(columns) = (groups, pieces left out) turns them into float32 groups, and compare_group compares each group of `names`.
    start: one value or a (gen, ref) pair; arrays: see pieces.upload. Returns {'n_gen', 'n_ref', left_out + '_gen', left_out + '_ref',
    'device_ms', ['profile_gen', 'profile_ref': profile(columns),] 'groups'}."""
    G = int(grid)
    if not 2 <= G <= 4096:
        raise PBError('%s: grid = %r points; 2 .. 4096' % (who, grid))
    s_gen, s_ref = start if isinstance(start, tuple) else (start, start)
    timer = pieces.Timer((stage,) + SET_STAGES)
    c_gen, c_ref = (timer.run(stage, op, **pieces.upload(ids, tab, s, device, **arrays)) for ids, s in ((gen_ids, s_gen), (ref_ids, s_ref)))
    dev = c_gen.device
    g_gen, out_gen = grouping(c_gen)
    g_ref, out_ref = grouping(c_ref)
    n_gen, n_ref = len(g_gen[names[0]]), len(g_ref[names[0]])
    ws = ops.metrics_ws(max(n_gen, n_ref, 1), max(n_gen, n_ref, 1), G, dev)
    groups = OrderedDict((name, compare_group(g_gen[name].reshape(n_gen, -1), g_ref[name].reshape(n_ref, -1), G, ws, timer, dev)) for name in names)
    res = OrderedDict([('n_gen', n_gen), ('n_ref', n_ref), (left_out + '_gen', out_gen), (left_out + '_ref', out_ref), ('device_ms', timer.totals())])
    if profile is not None:
        res.update([('profile_gen', profile(c_gen)), ('profile_ref', profile(c_ref))])
    res['groups'] = groups
    return res


def describe_pieces(stage, op, grouping, names, profile, ids, tab, start, device, **arrays):
    """One set alone, the sibling of compare_pieces: {'n', 'short', 'device_ms', 'profile': profile(columns), 'means'}: means = the mean
    over the n kept pieces of the groups of `names` (nan when n = 0)."""
    timer = pieces.Timer((stage,) + SET_STAGES)
    cols = timer.run(stage, op, **pieces.upload(ids, tab, start, device, **arrays))
    ms = timer.totals()
    g, short = grouping(cols)
    n = len(g[names[0]])
    means = OrderedDict((k, float(g[k].astype(np.float64).mean()) if n else float('nan')) for k in names)
    return OrderedDict([('n', n), ('short', short), ('device_ms', ms), ('profile', profile(cols)), ('means', means)])


def compare_sets(gen_ids, ref_ids, e2w=None, grid=1024, start=None, device=None):
    """Compare a generated set with a reference set, both (N, S, 8) ids. Per feature group: the mean and std (numpy's, ddof = 0) of the
    feature in each set (of the row norm for the histogram groups), the means of the gen-gen, ref-ref and gen-ref distances, and from
    Gaussian kernel density estimates of the three distance samples (Scott's bandwidth std(ddof = 1) n^(-1/5) each, one common grid of
    `grid` points over [min - 3 h_max, max + 3 h_max]) kl = KL(intra-ref || inter) and oa = the overlapped area of the two (kl_gen, oa_gen:
    the same for intra-gen). A sample with fewer than two values or no spread gives nan for the group's kl and oa. start: see
    piece_features (one value or a (gen, ref) pair). Returns {'n_gen', 'n_ref', 'empty_gen', 'empty_ref', 'device_ms', 'groups'}."""
    tab = tables(e2w)
    return compare_pieces('compare_sets', 'features', ops.piece_features, feature_groups, GROUPS, gen_ids, ref_ids, tab, grid, start, device,
                          left_out='empty', dur_pos=tab.dur_pos)
