"""A Python restatement of the harmony columns, written from the definitions: the yardstick of tests/test_harmony_cpu.py and
tests/test_harmony_gpu.py. It imports nothing from pianobart_amd.harmony and shares no code with it.

  table()                                    TL[k] = round(k log2(k) 2^20), by decimal arithmetic at 60 digits (with the distance of every
                                             entry from a rounding tie)
  harmony(ids, pad8, pitch_of, start)        the (N, 228) integer table: one Counter of pitch classes per bar (the lag sums take all bar
                                             pairs of a lag at once, as integer arrays, or 4 096-row pieces would take seconds)
  harmony_notes(...)                         the same table from the note list alone, with no per-bar histogram (a second opinion): a note
                                             of class c in bar b is the r-th such note; min(h_a[c], h_b[c']) counts the ranks both hold
  profiles(cols) / groups(cols, lags)        float64 restatements of the host half
  pooled(cols)                               the pooled profiles of a set
  compare(...)                               the whole pipeline, on the distance / KDE / KL-OA restatements of tests/metrics_ref.py
and the transposing-motif piece of both test files."""
import decimal
from collections import Counter

import numpy as np

from tests import metrics_ref as M

LAGS, COLS, SHIFT = 64, 228, 20
C_G, C_W1, C_W4, C_IH, C_TH, C_IX = 8, 20, 28, 36, 100, 164
MAJOR = (0, 2, 4, 5, 7, 9, 11)
WINDOWS = ((1, C_W1), (4, C_W4))
GROUPS = ('pc_entropy_1', 'pc_entropy_4', 'scale_consistency', 'local_scale_1', 'local_scale_4', 'key_stability', 'key_change_rate',
          'classes_per_bar', 'harmony_profile', 'sequence_profile', 'harmony_mean', 'sequence_gain')
_TABLE = {}


def table():
    """(TL, margin): the 4 097 integers and the smallest distance of k log2(k) 2^20 from a half-integer over k = 2 .. 4096."""
    if not _TABLE:
        ctx = decimal.Context(prec=60)
        ln2 = ctx.ln(decimal.Decimal(2))
        TL, margin = [0, 0], decimal.Decimal(1)
        for k in range(2, 4097):
            v = ctx.multiply(ctx.multiply(decimal.Decimal(k), ctx.divide(ctx.ln(decimal.Decimal(k)), ln2)), decimal.Decimal(1 << SHIFT))
            r = v.to_integral_value(rounding=decimal.ROUND_HALF_EVEN)
            TL.append(int(r))
            margin = min(margin, decimal.Decimal('0.5') - abs(v - r))
        _TABLE['v'] = (TL, float(margin))
    return _TABLE['v']


def notes_of(piece, pad8, pitch_of, start):
    """[(bar, class or None)] of rows start .. L - 1; None = percussion"""
    out = []
    for r in range(start, M.length(piece, pad8)):
        k = int(pitch_of[int(piece[r, 3])])
        out.append((int(piece[r, 0]), k % 12 if k >= 0 else None))
    return out


def key_of(h):
    """(best, key) of a histogram given as a mapping class -> count"""
    ins = [sum(h.get((k + d) % 12, 0) for d in MAJOR) for k in range(12)]
    best = max(ins)
    return best, ins.index(best)


def _finish_windows(c, base, wins, k_star, TL):
    """wins: the histograms (Counters) of the windows in bar order"""
    c[base] = len(wins)
    last = None
    for h in wins:
        n = sum(h.values())
        if n == 0:
            continue
        best, key = key_of(h)
        c[base + 1] += 1
        c[base + 2] += n
        c[base + 3] += TL[n] - sum(TL[v] for v in h.values())
        c[base + 4] += best
        c[base + 5] += key == k_star
        c[base + 6] += last is not None and key != last
        c[base + 7] += sum(1 for v in h.values() if v > 0)
        last = key


def harmony_one(piece, pad8, pitch_of, start=0):
    TL = table()[0]
    c = [0] * COLS
    notes = notes_of(piece, pad8, pitch_of, start)
    c[0] = len(notes)
    if not notes:
        return c
    b0 = min(b for b, _ in notes)
    W = max(b for b, _ in notes) - b0 + 1
    H = [Counter() for _ in range(W)]
    for b, k in notes:
        if k is not None:
            H[b - b0][k] += 1
    n = [sum(h.values()) for h in H]
    g = Counter()
    for h in H:
        g.update(h)
    c[1], c[2] = W, sum(n)
    c[3] = c[0] - c[2]
    c[4] = sum(1 for v in n if v > 0)
    c[6], c[5] = key_of(g)
    for k in range(12):
        c[C_G + k] = g[k]
    for w, base in WINDOWS:
        wins = []
        for b in range(0, W - w + 1):
            h = Counter()
            for j in range(w):
                h.update(H[b + j])
            wins.append(h)
        _finish_windows(c, base, wins, c[5], TL)
    # the lag sums, all bar pairs of a lag at once: A[b, c] = h_b[c], ROT[b, t, c] = h_b[(c + t) % 12]
    A = np.array([[h[k] for k in range(12)] for h in H], dtype=np.int64)
    ROT = np.stack([np.roll(A, -t, axis=1) for t in range(12)], axis=1)
    for l in range(1, min(LAGS, W - 1) + 1):
        meet = np.minimum(A[:W - l, None, :], ROT[l:, :, :]).sum(2)            # (bar pairs, t)
        c[C_IH + l - 1] = int(meet[:, 0].sum())
        c[C_TH + l - 1] = sum(n[b] + n[b + l] for b in range(W - l))
        c[C_IX + l - 1] = int(meet.max(1).sum())
    return c


def _each(fn, ids, pad8, pitch_of, start):
    ids = np.asarray(ids)
    st = np.zeros(ids.shape[0], dtype=np.int64) if start is None else np.broadcast_to(start, (ids.shape[0],))
    return np.array([fn(ids[n], pad8, pitch_of, int(st[n])) for n in range(ids.shape[0])], dtype=np.int64).reshape(ids.shape[0], COLS)


def harmony(ids, pad8, pitch_of, start=None):
    return _each(harmony_one, ids, pad8, pitch_of, start)


def harmony_notes_one(piece, pad8, pitch_of, start=0):
    """No per-bar histogram. The windows count classes in the list of the notes they hold. The lag sums go over note pairs: with r = the
    number of earlier rows of the same bar and class, min(h_a[c], h_b[c']) = the pairs (note of bar a and class c, note of bar b and class
    c') of equal r; the transposition sums are tallied per (bar, lag, t) and the largest t is taken per bar pair."""
    TL = table()[0]
    c = [0] * COLS
    notes = notes_of(piece, pad8, pitch_of, start)
    c[0] = len(notes)
    if not notes:
        return c
    b0 = min(b for b, _ in notes)
    W = max(b for b, _ in notes) - b0 + 1
    pitched = [(b - b0, k) for b, k in notes if k is not None]
    c[1], c[2], c[3] = W, len(pitched), len(notes) - len(pitched)
    c[4] = len(set(b for b, _ in pitched))
    for k in range(12):
        c[C_G + k] = sum(1 for _, kk in pitched if kk == k)
    c[6], c[5] = key_of({k: c[C_G + k] for k in range(12)})
    for w, base in WINDOWS:
        wins = []
        for b in range(0, W - w + 1):
            classes = [k for bb, k in pitched if b <= bb < b + w]
            wins.append({k: classes.count(k) for k in set(classes)})
        _finish_windows(c, base, wins, c[5], TL)
    rank = [sum(1 for j in range(i) if pitched[j] == pitched[i]) for i in range(len(pitched))]
    tally = {}
    for i, (ba, ka) in enumerate(pitched):
        for j, (bb, kb) in enumerate(pitched):
            l = bb - ba
            if 1 <= l <= LAGS and rank[i] == rank[j]:
                t = (kb - ka) % 12
                tally[(ba, l, t)] = tally.get((ba, l, t), 0) + 1
    for (ba, l, t), v in tally.items():
        if t == 0:
            c[C_IH + l - 1] += v
    for ba, l in set((ba, l) for ba, l, _ in tally):
        c[C_IX + l - 1] += max(tally.get((ba, l, t), 0) for t in range(12))
    for l in range(1, LAGS + 1):
        for b, _ in pitched:
            c[C_TH + l - 1] += (b + l < W) + (b - l >= 0)                  # a note counts once as the earlier bar's, once as the later bar's
    return c


def harmony_notes(ids, pad8, pitch_of, start=None):
    return _each(harmony_notes_one, ids, pad8, pitch_of, start)


# ---- the host half --------------------------------------------------------------------------------------------------------------------
def profiles(cols):
    """(harmony, sequence), (N, 64) float64, nan where T == 0"""
    cols = np.asarray(cols)
    out = []
    for i0 in (C_IH, C_IX):
        out.append(np.array([[2.0 * int(r[i0 + l]) / int(r[C_TH + l]) if r[C_TH + l] else float('nan') for l in range(LAGS)] for r in cols],
                            dtype=np.float64).reshape(len(cols), LAGS))
    return out[0], out[1]


def groups(cols, lags=16):
    rows = [[int(v) for v in r] for r in np.asarray(cols) if r[1] >= 2 and r[2] >= 1]
    short = len(cols) - len(rows)
    div = lambda a, b: a / b if b != 0 else 0.0
    out = {k: [] for k in GROUPS}
    for r in rows:
        w1, w4 = r[C_W1:C_W1 + 8], r[C_W4:C_W4 + 8]
        out['pc_entropy_1'].append(div(w1[3], float(1 << SHIFT) * w1[2]))
        out['pc_entropy_4'].append(div(w4[3], float(1 << SHIFT) * w4[2]))
        out['scale_consistency'].append(div(r[6], r[2]))
        out['local_scale_1'].append(div(w1[4], w1[2]))
        out['local_scale_4'].append(div(w4[4], w4[2]))
        out['key_stability'].append(div(w4[5], w4[1]))
        out['key_change_rate'].append(div(w1[6], w1[1] - 1))
        out['classes_per_bar'].append(div(w1[7], w1[1]))
        out['harmony_profile'].append([div(2.0 * r[C_IH + l], r[C_TH + l]) for l in range(lags)])
        out['sequence_profile'].append([div(2.0 * r[C_IX + l], r[C_TH + l]) for l in range(lags)])
        ih, ix, th = sum(r[C_IH:C_IH + lags]), sum(r[C_IX:C_IX + lags]), sum(r[C_TH:C_TH + lags])
        out['harmony_mean'].append(div(2.0 * ih, th))
        out['sequence_gain'].append(div(2.0 * (ix - ih), th))
    shape = lambda k: (len(rows), lags) if k.endswith('_profile') else (len(rows),)
    return {k: np.asarray(v, dtype=np.float64).reshape(shape(k)).astype(np.float32) for k, v in out.items()}, short


def pooled(cols):
    s = [int(v) for v in np.asarray(cols, dtype=np.int64).sum(0)]
    div = lambda a, b: 2.0 * a / b if b != 0 else float('nan')
    return {'harmony': [div(s[C_IH + l], s[C_TH + l]) for l in range(LAGS)], 'sequence': [div(s[C_IX + l], s[C_TH + l]) for l in range(LAGS)]}


def compare(gen_ids, ref_ids, pad8, pitch_of, lags=16, grid=1024):
    """The pipeline in float64: the per-group body is that of metrics_ref.compare."""
    c_gen, c_ref = harmony(gen_ids, pad8, pitch_of), harmony(ref_ids, pad8, pitch_of)
    g_gen, s_gen = groups(c_gen, lags)
    g_ref, s_ref = groups(c_ref, lags)
    res = {}
    for name in GROUPS:
        xg, xr = g_gen[name], g_ref[name]
        xg, xr = xg.reshape(len(xg), -1), xr.reshape(len(xr), -1)
        r = {}
        for tag, x in (('gen', xg), ('ref', xr)):
            v = np.sqrt((x.astype(np.float64) ** 2).sum(1)) if x.shape[1] > 1 else x[:, 0].astype(np.float64)
            r['mean_' + tag], r['std_' + tag] = float(np.mean(v)), float(np.std(v))
        sm = {'gen': M.samples(M.pairwise(xg, xg), True), 'ref': M.samples(M.pairwise(xr, xr), True), 'inter': M.samples(M.pairwise(xg, xr), False)}
        sm = {k: np.asarray(v, dtype=np.float64) for k, v in sm.items()}
        for k, v in sm.items():
            r['dist_' + k] = float(np.mean(v)) if len(v) else float('nan')
        r['kl'] = r['oa'] = r['kl_gen'] = r['oa_gen'] = float('nan')
        if all(len(v) >= 2 and v.min() != v.max() for v in sm.values()):
            hs = {k: float(np.std(v, ddof=1)) * len(v) ** -0.2 for k, v in sm.items()}
            h_max = max(hs.values())
            lo = min(v.min() for v in sm.values()) - 3 * h_max
            hi = max(v.max() for v in sm.values()) + 3 * h_max
            pts = np.linspace(lo, hi, grid).astype(np.float32)
            dens = {k: M.kde(v, pts, hs[k]) for k, v in sm.items()}
            dx = (hi - lo) / (grid - 1)
            r['oa'], r['kl'] = M.overlap_kl(dens['ref'], dens['inter'], dx)
            r['oa_gen'], r['kl_gen'] = M.overlap_kl(dens['gen'], dens['inter'], dx)
        res[name] = r
    return {'n_gen': len(g_gen['harmony_mean']), 'n_ref': len(g_ref['harmony_mean']), 'short_gen': s_gen, 'short_ref': s_ref,
            'profile_gen': pooled(c_gen), 'profile_ref': pooled(c_ref), 'group_arrays': (g_gen, g_ref), 'groups': res}


# ---- a transposing motif --------------------------------------------------------------------------------------------------------------
def sequence_piece(sizes, copies, step=2, first_bar=0, low=40):
    """(rows, 8) int64: a two-bar motif (pitch ids low + {0, 4, 7, 4} and low + {2, 5, 9}, the first bar's root doubled) written `copies`
    times, every copy `step` semitones above the one before, then an EOS row. Pitch ids below 128 are their own pitch numbers in the
    dictionaries of tests/metrics_ref.tables_for."""
    pad = np.asarray(sizes) - 6
    bars = ([0, 0, 4, 7, 4], [2, 5, 9])
    rows = []
    for copy in range(copies):
        for j, bar in enumerate(bars):
            for i, d in enumerate(bar):
                rows.append([first_bar + 2 * copy + j, 8 * i, 0, low + step * copy + d, 8, 20, 9, 30])
    rows.append(list(pad + 3))
    return np.asarray(rows, dtype=np.int64)
