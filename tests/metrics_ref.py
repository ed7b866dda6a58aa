"""A loop-and-numpy float64 restatement of the set metrics, written from the definitions: the yardstick of
tests/test_metrics_cpu.py and tests/test_metrics_gpu.py. It imports nothing from pianobart_amd.metrics and shares no code with it.

  features(ids, pad8, pitch_of, dur_pos, start)   the (N, 288) integer table, one Python loop over the rows of a piece
  groups(feat)                                    the 14 feature groups (float64 divisions, then float32) and the number of empty pieces
  pairwise(A, B) / samples(D, upper)              float64 distances of float32 rows; the samples of a matrix
  kde(s, grid, h)                                 the Gaussian kernel density in float64
  overlap_kl(p, q, dx) / compare(...)             the host integrals and the whole pipeline
and synthetic pieces for both test files."""
import math

import numpy as np

COLS = 288
SCALARS = ('note_count', 'pitch_count', 'pitch_range', 'avg_interval', 'notes_per_bar', 'avg_duration', 'avg_velocity', 'onset_ratio')
HISTS = (('pch', 16, 12, 1), ('pctm', 28, 144, 8), ('beat_grid', 172, 16, 0), ('duration_hist', 188, 32, 0), ('velocity_hist', 220, 32, 0),
         ('bar_density_hist', 252, 32, 2))


def length(piece, pad8):
    for r in range(piece.shape[0]):
        if any(int(piece[r, h]) >= pad8[h] for h in range(8)):
            return r
    return piece.shape[0]


def features_one(piece, pad8, pitch_of, dur_pos, start=0):
    f = [0] * COLS
    L = length(piece, pad8)
    notes = [tuple(int(v) for v in piece[r]) for r in range(start, L)]
    bars, ks, inss, per_bar = set(), [], set(), {}
    prev_t = None
    for bar, pos, ins, pit, dur, vel, _, _ in notes:
        f[0] += 1
        bars.add(bar)
        inss.add(ins)
        per_bar[bar] = per_bar.get(bar, 0) + 1
        t = bar * 1024 + pos
        if prev_t is None or t != prev_t:
            f[9] += 1
        if prev_t is not None and t < prev_t:
            f[10] += 1
        prev_t = t
        f[11] += int(dur_pos[dur])
        f[12] += vel
        f[172 + pos % 16] += 1
        f[188 + min(dur >> 2, 31)] += 1
        f[220 + min(vel, 31)] += 1
        k = int(pitch_of[pit])
        if k >= 0:
            if ks:
                f[7] += abs(k - ks[-1])
                f[8] += 1
                f[28 + 12 * (ks[-1] % 12) + k % 12] += 1
            ks.append(k)
            f[16 + k % 12] += 1
    f[1] = len(ks)
    f[2] = len(bars)
    f[3] = max(bars) - min(bars) + 1 if bars else 0
    f[4] = len(set(ks))
    f[5], f[6] = (min(ks), max(ks)) if ks else (-1, -1)
    f[13] = len(inss)
    for c in per_bar.values():
        f[252 + min(c, 32) - 1] += 1
    return f


def features(ids, pad8, pitch_of, dur_pos, start=None):
    ids = np.asarray(ids)
    return np.array([features_one(ids[n], pad8, pitch_of, dur_pos, 0 if start is None else int(np.broadcast_to(start, (ids.shape[0],))[n]))
                     for n in range(ids.shape[0])], dtype=np.int64).reshape(ids.shape[0], COLS)


def groups(feat):
    f = np.asarray(feat, dtype=np.float64)
    rows = [r for r in f if r[0] > 0]
    empty = len(f) - len(rows)
    div = lambda a, b: a / b if b != 0 else 0.0
    out = {name: [] for name in SCALARS + tuple(h[0] for h in HISTS)}
    for r in rows:
        out['note_count'].append(r[0])
        out['pitch_count'].append(r[4])
        out['pitch_range'].append(r[6] - r[5] if r[1] > 0 else 0.0)
        out['avg_interval'].append(div(r[7], r[8]))
        out['notes_per_bar'].append(div(r[0], r[2]))
        out['avg_duration'].append(div(r[11], r[0]))
        out['avg_velocity'].append(div(r[12], r[0]))
        out['onset_ratio'].append(div(r[9], r[0]))
        for name, col, width, d in HISTS:
            out[name].append([div(v, r[d]) for v in r[col:col + width]])
    widths = dict((h[0], h[2]) for h in HISTS)
    return {k: np.asarray(v, dtype=np.float64).reshape((len(rows),) + ((widths[k],) if k in widths else ())).astype(np.float32) for k, v in out.items()}, empty


def pairwise(A, B):
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    return np.sqrt(((A[:, None, :] - B[None, :, :]) ** 2).sum(-1))


def samples(D, upper):
    D = np.asarray(D)
    return D[np.triu_indices(D.shape[0], 1)] if upper else D.reshape(-1)


def kde(s, grid, h):
    s, grid = np.asarray(s, dtype=np.float64), np.asarray(grid, dtype=np.float64)
    out = np.empty(len(grid))
    for g, x in enumerate(grid):
        out[g] = np.exp(-(x - s) ** 2 / (2.0 * h * h)).sum() / (len(s) * h * math.sqrt(2.0 * math.pi))
    return out


def trapezoid(y, dx):
    return sum(0.5 * (float(y[i]) + float(y[i + 1])) * dx for i in range(len(y) - 1))


def overlap_kl(p, q, dx):
    oa = trapezoid([min(a, b) for a, b in zip(p, q)], dx)
    kl = trapezoid([a * math.log(a / max(b, 1e-300)) if a > 0 else 0.0 for a, b in zip(p, q)], dx)
    return oa, kl


def compare(gen_ids, ref_ids, pad8, pitch_of, dur_pos, grid=1024, start=None, dist=None):
    """The pipeline in float64. dist(A, B): the distance matrices to take the samples from (default: pairwise, float64 of the float32
    rows), so that a test can feed the device's float32 distances and look at the later stages alone."""
    dist = dist or pairwise
    g_gen, e_gen = groups(features(gen_ids, pad8, pitch_of, dur_pos, start))
    g_ref, e_ref = groups(features(ref_ids, pad8, pitch_of, dur_pos, start))
    res = {}
    for name in g_gen:
        xg, xr = g_gen[name], g_ref[name]
        xg, xr = xg.reshape(len(xg), -1), xr.reshape(len(xr), -1)
        r = {}
        for tag, x in (('gen', xg), ('ref', xr)):
            v = np.sqrt((x.astype(np.float64) ** 2).sum(1)) if x.shape[1] > 1 else x[:, 0].astype(np.float64)
            r['mean_' + tag], r['std_' + tag] = float(np.mean(v)), float(np.std(v))
        sm = {'gen': samples(dist(xg, xg), True), 'ref': samples(dist(xr, xr), True), 'inter': samples(dist(xg, xr), False)}
        sm = {k: np.asarray(v, dtype=np.float64) for k, v in sm.items()}
        for k, v in sm.items():
            r['dist_' + k] = float(np.mean(v)) if len(v) else float('nan')
        r['kl'] = r['oa'] = float('nan')
        if all(len(v) >= 2 and v.min() != v.max() for v in sm.values()):
            hs = {k: float(np.std(v, ddof=1)) * len(v) ** -0.2 for k, v in sm.items()}
            h_max = max(hs.values())
            lo = min(v.min() for v in sm.values()) - 3 * h_max
            hi = max(v.max() for v in sm.values()) + 3 * h_max
            pts = np.linspace(lo, hi, grid).astype(np.float32)
            dens = {k: kde(v, pts, hs[k]) for k, v in sm.items()}
            r['oa'], r['kl'] = overlap_kl(dens['ref'], dens['inter'], (hi - lo) / (grid - 1))
        res[name] = r
    return {'n_gen': len(g_gen['note_count']), 'n_ref': len(g_ref['note_count']), 'empty_gen': e_gen, 'empty_ref': e_ref, 'groups': res}


# ---- synthetic pieces ---------------------------------------------------------------------------------------------------------------
def tables_for(sizes, n_perc):
    """pitch_of / dur_pos of a dictionary with the given head sizes whose last n_perc ordinary pitch ids are percussion and the others
    'Pitch id'; durations by the Octuple rule (octave i holds 16 codes, each 2^i positions wide, the last code repeated)."""
    pad8 = [n - 6 for n in sizes]
    pitch_of = np.array([i if i < pad8[3] - n_perc else -1 for i in range(pad8[3])], dtype=np.int16)
    dec, pos = [], 0
    for i in range(8):
        for _ in range(16):
            dec.append(pos)
            pos += 2 ** i
    dur_pos = np.array([dec[min(c, len(dec) - 1)] for c in range(pad8[4])], dtype=np.int32)
    return pad8, pitch_of, dur_pos


def synth_pieces(sizes, N, S, seed, style=0, n_perc=128):
    """(N, S, 8) int64 pieces: sorted bars with a few steps back, chords (repeated positions), percussion runs, ragged lengths ended by an
    EOS row and a PAD tail. style shifts the pitch register, the rhythm grid, the durations and the density a little, so that two sets differ
    and still overlap."""
    rng = np.random.default_rng(seed)
    pad = np.asarray(sizes) - 6
    out = np.empty((N, S, 8), dtype=np.int64)
    for n in range(N):
        L = S if n == 0 else int(rng.integers(max(1, S // 3), S + 1))
        rows = np.stack([rng.integers(0, pad[h], size=S) for h in range(8)], axis=1)
        n_bars = int(rng.integers(1, min(pad[0], max(2, L // (3 + style))) + 1))
        rows[:, 0] = np.sort(rng.integers(0, n_bars, size=S))
        rows[:, 1] = rng.integers(0, min(pad[1], 64), size=S)
        if style:
            even = rng.random(S) < 0.3
            rows[even, 1] = rows[even, 1] // 2 * 2
        chord = rng.random(S) < 0.3
        for r in range(1, S):
            if chord[r]:
                rows[r, 0:2] = rows[r - 1, 0:2]
        lo = 30 + 6 * style
        rows[:, 3] = np.clip(np.rint(rng.normal(lo + 12, 9, size=S)), 0, pad[3] - n_perc - 1).astype(np.int64)
        drums = rng.random(S) < 0.1
        if n_perc:
            rows[drums, 3] = rng.integers(pad[3] - n_perc, pad[3], size=int(drums.sum()))
        rows[:, 4] = rng.integers(0, min(pad[4], 40 + 8 * style), size=S)
        out[n] = rows
        if L < S:
            out[n, L] = pad + 3
            out[n, L + 1:] = pad
    return out
