"""A restatement of the texture columns and groups, written from the definitions with Python dicts and loops: the yardstick
of tests/test_texture_cpu.py and tests/test_texture_gpu.py. It imports nothing from pianobart_amd and shares no code with the module or
the kernel: the sounding count c(tau) is read off a piano roll (one boolean step array per pitch), collisions off a second roll of the
steps strictly inside a note, duplicates and chords off dicts and sorted lists.

  bar_pos_default()                                         the bar lengths of the default dictionary's time-signature ids
  texture(ids, pad8, pitch_of, dur_pos, bar_pos, start)     the (N, 64) integer table
  onsets(piece, ...)                                        (t, e) of the note rows of one piece, row by row (None for percussion)
  groups(cols) / pooled(cols) / compare(...)                the host half and the whole pipeline in float64
and pieces for both test files."""
import numpy as np

from tests import metrics_ref as M

COLS = 64
SCALARS = ('silence_ratio', 'polyphony_mean', 'polyphonic_rate', 'max_polyphony', 'overlap_ratio', 'collision_rate', 'duplicate_rate',
           'tie_rate', 'offbar_rate', 'chord_size_mean')
GROUPS = SCALARS + ('polyphony_hist', 'chord_hist', 'ioi_hist')
TS_44, TS_34, TS_21, TS_164, TS_68 = 9, 8, 1, 126, 19          # ids of the default dictionary: n/1, n/2, n/4, .. with n = 1 .. 2 d each


def ts_words():
    """The 254 time-signature words of the default dictionary, in id order."""
    return ['TimeSig %d/%d' % (n, 2 ** i) for i in range(7) for n in range(1, 2 * 2 ** i + 1)]


def bar_pos_default():
    return np.array([n * 64 // (2 ** i) for i in range(7) for n in range(1, 2 * 2 ** i + 1)], dtype=np.int32)


def _time_axis(notes, bar_pos):
    """b_lo, W, len[b], B[b] from all note rows."""
    b_lo, b_hi = min(r[0] for r in notes), max(r[0] for r in notes)
    W = b_hi - b_lo + 1
    first = {}
    for r in notes:
        cand = (r[1], r[6])
        if r[0] - b_lo not in first or cand < first[r[0] - b_lo]:
            first[r[0] - b_lo] = cand
    lens, starts, ts, now = [], [], None, 0
    for b in range(W):
        if b in first:
            ts = first[b][1]
        lens.append(int(bar_pos[ts]))
        starts.append(now)
        now += lens[-1]
    return b_lo, W, lens, starts


def onsets(piece, pad8, pitch_of, dur_pos, bar_pos, start=0):
    """Per note row of the piece (rows start .. L - 1): (t, e), or None for a percussion row."""
    L = M.length(piece, pad8)
    notes = [tuple(int(v) for v in piece[r]) for r in range(start, L)]
    if not notes:
        return []
    b_lo, _, _, starts = _time_axis(notes, bar_pos)
    out = []
    for bar, pos, _, pit, dur, _, _, _ in notes:
        if pitch_of[pit] < 0:
            out.append(None)
        else:
            t = starts[bar - b_lo] + pos
            out.append((t, t + max(int(dur_pos[dur]), 1)))
    return out


def texture_one(piece, pad8, pitch_of, dur_pos, bar_pos, start=0):
    c = [0] * COLS
    L = M.length(piece, pad8)
    notes = [tuple(int(v) for v in piece[r]) for r in range(start, L)]
    c[0] = len(notes)
    if not notes:
        return c
    b_lo, W, lens, starts = _time_axis(notes, bar_pos)
    c[2] = W
    sounding = []                                                # (k, t, d, e, bar index, position)
    for bar, pos, _, pit, dur, _, _, _ in notes:
        k = int(pitch_of[pit])
        if k >= 0:
            d = max(int(dur_pos[dur]), 1)
            t = starts[bar - b_lo] + pos
            sounding.append((k, t, d, t + d, bar - b_lo, pos))
    c[1] = len(sounding)
    if not sounding:
        return c
    t0, t1 = min(s[1] for s in sounding), max(s[3] for s in sounding)
    T = t1 - t0
    roll, inside = {}, {}
    for k, t, d, e, _, _ in sounding:
        if k not in roll:
            roll[k], inside[k] = np.zeros(T, dtype=bool), np.zeros(T + 1, dtype=bool)
        roll[k][t - t0:e - t0] = True
        inside[k][t - t0 + 1:e - t0] = True                      # the steps tau with t < tau < e
    count = np.zeros(T, dtype=np.int64)
    for k in roll:
        count += roll[k]
    c[3] = T
    c[4], c[5], c[6], c[7] = int((count >= 1).sum()), int((count >= 2).sum()), int(count.sum()), int(count.max())
    c[8] = sum(s[2] for s in sounding)
    per_group = {}
    for k, t, _, _, _, _ in sounding:
        per_group[(k, t)] = per_group.get((k, t), 0) + 1
    c[9] = sum(1 for (k, t) in per_group if inside[k][t - t0])
    c[10] = sum(m - 1 for m in per_group.values())
    starts_at = {}
    for k, t in per_group:
        starts_at.setdefault(t, set()).add(k)
    times = sorted(starts_at)
    c[11] = len(times)
    c[12] = sum(1 for _, _, _, e, b, _ in sounding if e > starts[b] + lens[b])
    c[13] = sum(1 for _, _, _, _, b, pos in sounding if pos >= lens[b])
    c[14] = len(per_group)
    for level, steps in enumerate(np.bincount(np.minimum(count, 16), minlength=17)):
        c[16 + level] = int(steps)
    for t in times:
        c[33 + min(len(starts_at[t]), 9) - 1] += 1
    for a, b in zip(times, times[1:]):
        c[42 + min((b - a).bit_length() - 1, 15)] += 1
    return c


def texture(ids, pad8, pitch_of, dur_pos, bar_pos, start=None):
    ids = np.asarray(ids)
    st = np.zeros(ids.shape[0], dtype=np.int64) if start is None else np.broadcast_to(np.asarray(start), (ids.shape[0],))
    return np.array([texture_one(ids[n], pad8, pitch_of, dur_pos, bar_pos, int(st[n])) for n in range(ids.shape[0])],
                    dtype=np.int64).reshape(ids.shape[0], COLS)


# ---- the host half --------------------------------------------------------------------------------------------------------------------
def groups(cols):
    rows = [[int(v) for v in r] for r in np.asarray(cols) if r[1] >= 1]
    unpitched = len(cols) - len(rows)
    div = lambda a, b: a / b if b != 0 else 0.0
    out = {k: [] for k in GROUPS}
    for r in rows:
        T, P, O = r[3], r[1], r[11]
        out['silence_ratio'].append(div(r[16], T))
        out['polyphony_mean'].append(div(r[6], r[4]))
        out['polyphonic_rate'].append(div(r[5], r[4]))
        out['max_polyphony'].append(float(r[7]))
        out['overlap_ratio'].append(div(r[8] - r[6], r[8]))
        out['collision_rate'].append(div(r[9], r[14]))
        out['duplicate_rate'].append(div(r[10], P))
        out['tie_rate'].append(div(r[12], P))
        out['offbar_rate'].append(div(r[13], P))
        out['chord_size_mean'].append(div(r[14], O))
        out['polyphony_hist'].append([div(v, T) for v in r[16:33]])
        out['chord_hist'].append([div(v, O) for v in r[33:42]])
        out['ioi_hist'].append([div(v, max(O - 1, 1)) for v in r[42:58]])
    width = {'polyphony_hist': 17, 'chord_hist': 9, 'ioi_hist': 16}
    shape = lambda k: (len(rows), width[k]) if k in width else (len(rows),)
    return {k: np.asarray(v, dtype=np.float64).reshape(shape(k)).astype(np.float32) for k, v in out.items()}, unpitched


def pooled(cols):
    s = [int(v) for v in np.asarray(cols, dtype=np.int64).sum(0)]
    div = lambda a, b: a / b if b != 0 else float('nan')
    return {'polyphony': [div(v, s[3]) for v in s[16:33]], 'chord': [div(v, s[11]) for v in s[33:42]]}


def compare(gen_ids, ref_ids, pad8, pitch_of, dur_pos, bar_pos, grid=1024):
    """The pipeline in float64: the per-group body is that of metrics_ref.compare, with the densities of the generated set besides."""
    c_gen, c_ref = texture(gen_ids, pad8, pitch_of, dur_pos, bar_pos), texture(ref_ids, pad8, pitch_of, dur_pos, bar_pos)
    g_gen, u_gen = groups(c_gen)
    g_ref, u_ref = groups(c_ref)
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
    return {'n_gen': len(g_gen['max_polyphony']), 'n_ref': len(g_ref['max_polyphony']), 'unpitched_gen': u_gen, 'unpitched_ref': u_ref,
            'profile_gen': pooled(c_gen), 'profile_ref': pooled(c_ref), 'group_arrays': (g_gen, g_ref), 'groups': res}


# ---- pieces ---------------------------------------------------------------------------------------------------------------------------
def from_notes(notes, S, pad, L=None):
    """(S, 8) int64 from rows of (bar, position, pitch id, duration id, time-signature id): the other heads fixed, then an EOS row and a
    PAD tail. L: keep the first L rows only."""
    rows = np.tile(np.asarray(pad, dtype=np.int64), (S, 1))
    notes = list(notes)[:S if L is None else L]
    for r, (bar, pos, pit, dur, ts) in enumerate(notes):
        rows[r] = (bar, pos, 0, pit, dur, 20, ts, 30)
    if len(notes) < S:
        rows[len(notes)] = np.asarray(pad) + 3
    return rows


def piano_notes(n, seed, n_perc_ids=128, first_bar=0, bars=None, style=0, ts_pool=(TS_44, TS_34, TS_68, TS_44)):
    """n rows of a piano-like piece over `bars` bars (default: about one per six rows): every bar has one time signature from ts_pool,
    onsets on a grid of two positions with chords, pitches around the middle of the keyboard so that notes of one pitch meet, durations of
    1 .. 60 positions, one row in ten percussion, a few rows written twice and a few positions behind the end of the bar. style moves
    the register, the durations and the chords, so that two sets differ and still overlap."""
    rng = np.random.default_rng(seed)
    bars = bars or max(1, min(n // 6, 200))
    bar_ts = rng.choice(ts_pool, size=bars)
    out = []
    for _ in range(n):
        if out and rng.random() < 0.25 + 0.1 * style:                                   # a chord: the onset of the row before
            bar, pos = out[-1][0] - first_bar, out[-1][1]
        else:
            bar, pos = int(rng.integers(0, bars)), int(rng.integers(0, 24)) * 2
            if rng.random() < 0.03:
                pos = int(rng.integers(48, 100))
        pit = int(np.clip(np.rint(rng.normal(60 + 5 * style, 7)), 0, 127))
        if n_perc_ids and rng.random() < 0.1:
            pit = 128 + int(rng.integers(0, n_perc_ids))
        dur = int(rng.integers(0, 36 + 10 * style))
        if out and rng.random() < 0.03:
            out.append(out[-1])
        else:
            out.append((first_bar + bar, pos, pit, dur, int(bar_ts[bar])))
    return out
