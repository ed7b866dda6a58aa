"""A Python-set restatement of the repetition structure columns, written from the definitions: the yardstick of
tests/test_structure_cpu.py and tests/test_structure_gpu.py. It imports nothing from pianobart_amd.structure and shares no code with it.

  structure(ids, pad8, pitch_of, start, mode)   the (N, 264) integer table: one set of positions and one of (position, field) per bar
  structure_pairs(...)                           the same table by a loop over note pairs, with no set of any kind (a second opinion)
  lag_profiles(cols) / groups(cols, lags)        float64 restatements of the host half
  pooled(cols)                                   the pooled profiles of a set
  compare(...)                                   the whole pipeline, on the distance / KDE / KL-OA restatements of tests/metrics_ref.py
and the seeded motif pieces of both test files."""
import numpy as np

from tests import metrics_ref as M

LAGS, COLS = 64, 264
GROUPS = ('groove_profile', 'repeat_profile', 'groove_mean', 'repeat_mean', 'repeat_period')


def notes_of(piece, pad8, pitch_of, start, mode):
    """[(bar, position, field)] of rows start .. L - 1"""
    out = []
    for r in range(start, M.length(piece, pad8)):
        bar, pos, pit = int(piece[r, 0]), int(piece[r, 1]), int(piece[r, 3])
        f = pit
        if mode == 1:
            k = int(pitch_of[pit])
            f = k % 12 if k >= 0 else 12 + pit
        out.append((bar, pos, f))
    return out


def structure_one(piece, pad8, pitch_of, start=0, mode=0):
    c = [0] * COLS
    notes = notes_of(piece, pad8, pitch_of, start, mode)
    c[0] = len(notes)
    if not notes:
        return c
    b0 = min(n[0] for n in notes)
    W = max(n[0] for n in notes) - b0 + 1
    O = [set() for _ in range(W)]
    Nn = [set() for _ in range(W)]
    for bar, pos, f in notes:
        O[bar - b0].add(pos)
        Nn[bar - b0].add((pos, f))
    c[1] = W
    c[2] = sum(len(s) for s in O)
    c[3] = sum(len(s) for s in Nn)
    c[4] = sum(1 for s in O if s)
    for l in range(1, LAGS + 1):
        for base, X in ((8, O), (136, Nn)):
            for b in range(0, W - l):
                c[base + l - 1] += len(X[b] & X[b + l])
                c[base + 64 + l - 1] += len(X[b]) + len(X[b + l])
    return c


def structure(ids, pad8, pitch_of, start=None, mode=0):
    ids = np.asarray(ids)
    st = np.zeros(ids.shape[0], dtype=np.int64) if start is None else np.broadcast_to(start, (ids.shape[0],))
    return np.array([structure_one(ids[n], pad8, pitch_of, int(st[n]), mode) for n in range(ids.shape[0])], dtype=np.int64).reshape(ids.shape[0], COLS)


def structure_pairs_one(piece, pad8, pitch_of, start=0, mode=0):
    """No sets: a note counts for an element when no earlier row holds the same element; the lag sums are counted pair by pair, T bar by
    bar from the definition."""
    c = [0] * COLS
    notes = notes_of(piece, pad8, pitch_of, start, mode)
    c[0] = len(notes)
    if not notes:
        return c
    first_o = [all(notes[j][:2] != notes[i][:2] for j in range(i)) for i in range(len(notes))]
    first_n = [all(notes[j] != notes[i] for j in range(i)) for i in range(len(notes))]
    b0 = min(n[0] for n in notes)
    W = max(n[0] for n in notes) - b0 + 1
    per_o, per_n = [0] * W, [0] * W
    for i, (bar, _, _) in enumerate(notes):
        per_o[bar - b0] += first_o[i]
        per_n[bar - b0] += first_n[i]
    c[1], c[2], c[3], c[4] = W, sum(per_o), sum(per_n), sum(1 for v in per_o if v)
    for a, (ba, pa, fa) in enumerate(notes):
        for cc, (bc, pc, fc) in enumerate(notes):
            l = bc - ba
            if 1 <= l <= LAGS and pa == pc:
                c[8 + l - 1] += first_o[a] and first_o[cc]
                c[136 + l - 1] += first_n[a] and first_n[cc] and fa == fc
    for l in range(1, LAGS + 1):
        for b in range(W):
            if b + l < W:
                c[72 + l - 1] += per_o[b] + per_o[b + l]
                c[200 + l - 1] += per_n[b] + per_n[b + l]
    return c


def structure_pairs(ids, pad8, pitch_of, start=None, mode=0):
    ids = np.asarray(ids)
    st = np.zeros(ids.shape[0], dtype=np.int64) if start is None else np.broadcast_to(start, (ids.shape[0],))
    return np.array([structure_pairs_one(ids[n], pad8, pitch_of, int(st[n]), mode) for n in range(ids.shape[0])], dtype=np.int64).reshape(ids.shape[0], COLS)


# ---- the host half --------------------------------------------------------------------------------------------------------------------
def lag_profiles(cols):
    """(groove, repeat), (N, 64) float64, nan where T == 0"""
    cols = np.asarray(cols)
    out = []
    for i0, t0 in ((8, 72), (136, 200)):
        out.append(np.array([[2.0 * int(r[i0 + l]) / int(r[t0 + l]) if r[t0 + l] else float('nan') for l in range(LAGS)] for r in cols],
                            dtype=np.float64).reshape(len(cols), LAGS))
    return out[0], out[1]


def groups(cols, lags=16):
    rows = [r for r in np.asarray(cols) if r[1] >= 2]
    short = len(cols) - len(rows)
    div = lambda a, b: 2.0 * a / b if b != 0 else 0.0
    out = {k: [] for k in GROUPS}
    for r in rows:
        r = [int(v) for v in r]
        d_o = [div(r[8 + l], r[72 + l]) for l in range(lags)]
        d_n = [div(r[136 + l], r[200 + l]) for l in range(lags)]
        out['groove_profile'].append(d_o)
        out['repeat_profile'].append(d_n)
        out['groove_mean'].append(div(sum(r[8:8 + lags]), sum(r[72:72 + lags])))
        out['repeat_mean'].append(div(sum(r[136:136 + lags]), sum(r[200:200 + lags])))
        period = 0
        for l in range(lags):
            if d_n[l] > (d_n[period - 1] if period else 0.0):
                period = l + 1
        out['repeat_period'].append(float(period))
    shape = lambda k: (len(rows), lags) if k.endswith('_profile') else (len(rows),)
    return {k: np.asarray(v, dtype=np.float64).reshape(shape(k)).astype(np.float32) for k, v in out.items()}, short


def pooled(cols):
    s = [int(v) for v in np.asarray(cols, dtype=np.int64).sum(0)]
    div = lambda a, b: 2.0 * a / b if b != 0 else float('nan')
    return {'groove': [div(s[8 + l], s[72 + l]) for l in range(LAGS)], 'repeat': [div(s[136 + l], s[200 + l]) for l in range(LAGS)]}


def compare(gen_ids, ref_ids, pad8, pitch_of, lags=16, grid=1024, mode=0):
    """The pipeline in float64: the per-group body is that of metrics_ref.compare."""
    c_gen, c_ref = structure(gen_ids, pad8, pitch_of, None, mode), structure(ref_ids, pad8, pitch_of, None, mode)
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
    return {'n_gen': len(g_gen['groove_mean']), 'n_ref': len(g_ref['groove_mean']), 'short_gen': s_gen, 'short_ref': s_ref,
            'profile_gen': pooled(c_gen), 'profile_ref': pooled(c_ref), 'group_arrays': (g_gen, g_ref), 'groups': res}


# ---- motif pieces -----------------------------------------------------------------------------------------------------------------------
def motif_piece(sizes, S, seed, mb=2, edit=0.2, first_bar=0):
    """(S, 8) int64: a motif of mb bars (2 to 5 notes per bar, positions from {0, 4, .., 60}, pitch ids from 12 neighbours) written over and
    over, bar ids rising from first_bar, until S rows are full; where the dictionary's bar ids run out the writing goes on from first_bar
    again, as one more voice over the same bars. Every copied note is dropped with probability edit / 2 and re-pitched (among the 12) with
    probability edit / 2. The other heads are random ordinary ids. No terminator: all S rows are notes."""
    rng = np.random.default_rng(seed)
    pad = np.asarray(sizes) - 6
    low = int(rng.integers(30, 60))
    motif = []
    for b in range(mb):
        k = int(rng.integers(2, 6))
        pos = np.sort(rng.choice(16, size=k, replace=False)) * 4
        motif.append([(int(p), low + int(rng.integers(0, 12))) for p in pos])
    rows = np.stack([rng.integers(0, pad[h], size=S) for h in range(8)], axis=1).astype(np.int64)
    span = (int(pad[0]) - first_bar) // mb * mb                 # where the bar ids run out the writing starts over at first_bar: one more voice
    r, t = 0, 0
    while r < S:
        for p, pit in motif[t % mb]:
            u = rng.random()
            if u < edit / 2:
                continue
            if u < edit:
                pit = low + int(rng.integers(0, 12))
            if r < S:
                rows[r, 0], rows[r, 1], rows[r, 3] = first_bar + t % span, p, pit
                r += 1
        t += 1
    return rows


def motif_pieces(sizes, N, S, seed, mb=2, edit=0.2):
    return np.stack([motif_piece(sizes, S, seed * 1000 + n, mb if isinstance(mb, int) else mb[n % len(mb)], edit) for n in range(N)])
