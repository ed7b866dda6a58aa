"""The device sampler's rule (dec_sample_kernel of csrc/pb_decode.hip; the header's "device-sampled decode", "Forced tokens", "Stop at a bar",
"Time-ordered sampling" and "Allowed classes") restated in float64 numpy, as the SET of ids a correct f32 implementation may return, and the
case tables that tests/test_sampler_ref_cpu.py judges and tests/test_sampler_kernel_gpu.py runs. No call into the engine, the library or
model.py.

One head: y = f32(logit) / f32(T) (an IEEE division: the same on both sides), -inf for a class the row's rules remove; the order is (y
descending, class ascending), the kernel's documented tie rule; q = exp(y - max) / sum / (1 + 1e-5) and its cumulative sums c_i in that order
are float64. eps = (n + 8) 2^-24, absolute on cumulative sums <= 1, is what an f32 implementation may be off by: at most n f32 additions
of partial sums <= 1 (2^-24 each), a few ulps of expf, the multiply by the reciprocal and the cast of u * qs. REL = 2^-21 relative is how
close two q of DIFFERENT y may be before f32 expf may tie or swap them (then the class index decides there, not y).
  p < 1: kc = 1 + (first i with c_i > p), none -> 1, taken at p - eps and at p + eps; for each kc, t = u c_{kc-1} and the index is the first
         i < kc with c_i > t (default kc - 1), taken at t - eps and t + eps. Every index in between is acceptable, and so is a neighbour in
         the order whose q is within REL of it at another y.
  p = 1: the classes within REL of the largest q; the lowest of them where they all have the bit-identical y.
A head is DECIDED when its set has one element."""
import numpy as np

REL = 2.0 ** -21
JUST_BELOW_1 = float(np.nextafter(1.0, 0.0))
MID0 = .4641                                                       # where in a candidate's interval the tables aim a draw: near the middle (a seed moves it a little)


def eps_of(n):
    return (n + 8) * 2.0 ** -24


def _first_above(c, x):
    """First i with c[i] > x in the non-decreasing c, or None."""
    i = int(np.searchsorted(c, x, side='right'))
    return i if i < len(c) else None


def quotients(logits_h, T, allowed=None):
    """y (f32, -inf where not allowed), the kernel's order, q (f64) of one head."""
    n = len(logits_h)
    y = (np.asarray(logits_h, dtype=np.float32) / np.float32(T)).astype(np.float32)
    if allowed is not None:
        y = np.where(allowed, y, np.float32(-np.inf)).astype(np.float32)
    y64 = y.astype(np.float64)
    order = np.lexsort((np.arange(n), -y64))
    with np.errstate(invalid='ignore'):
        e = np.exp(y64 - y64.max())
    q = e / e.sum() / (1.0 + 1e-5)
    return y, order, q


def free_kc(logits_h, T, p, allowed=None):
    """The number of nucleus candidates, exactly at p (the tables aim their draws with it)."""
    _, order, q = quotients(logits_h, T, allowed)
    if p >= 1.0:
        return 1, order, q
    first = _first_above(np.cumsum(q[order]), p)
    return (1 if first is None else first + 1), order, q


P_EXACT = float(np.float32(1) / (np.float32(2) * np.float32(1.00001)))      # the f32 probability of each of two classes that share a head


def _exact_pair(y, order, p, u):
    """A head whose two largest y are equal and whose every other y is 150 or more below them: f32 arithmetic is EXACT there, in any order of
    summation, so the answer is one id and eps is 0. expf(0) = 1 and expf(<= -150) = 0 (the least f32 is e^-103.3); the sum is 2; 2 * 1.00001f and
    the correctly rounded 1 / (2 * 1.00001f) are the same on both sides, as the division by T is; the two probabilities are that reciprocal, the
    cumulative sums it and its double (a power of two: exact), then unchanged by the zeros; u * qs is an IEEE double product and its cast to f32.
    This is what lets a case sit ON the threshold: p = P_EXACT is the first cumulative sum itself, which `> p` must not take and `>= p` would."""
    top = y[order[0]]
    if len(y) < 3 or not np.isfinite(top) or y[order[1]] != top or y[order[2]] > top - np.float32(150):
        return None
    inv = np.float32(1) / (np.float32(2) * np.float32(1.00001))
    c = [inv, np.float32(2) * inv]
    first = 0 if c[0] > np.float32(p) else (1 if c[1] > np.float32(p) else None)
    kc = 1 if first is None else first + 1
    thr = np.float32(float(u) * float(c[kc - 1]))
    best = kc - 1
    for i in range(kc - 1, -1, -1):
        if c[i] > thr:
            best = i
    return int(order[best])


def head_ids(logits_h, T, p, u, allowed=None):
    """The acceptable ids of one head: logits (n,) f32, T and p as the f32 values the kernel holds, u the f64 draw."""
    n = len(logits_h)
    p = float(np.float32(p))
    y, order, q = quotients(logits_h, T, allowed)
    bits = y.view(np.int32)
    if not np.isfinite(q).all():                                   # a NaN row (a log row nothing was written to), or no allowed class: nothing is acceptable
        return set()
    if p >= 1.0:
        near = np.flatnonzero(q >= q.max() * (1.0 - REL))
        if (bits[near] == bits[near[0]]).all():
            return {int(near.min())}
        return {int(v) for v in near}
    exact = _exact_pair(y, order, p, u)
    if exact is not None:
        return {exact}
    qo = q[order]
    c = np.cumsum(qo)
    eps = eps_of(n)
    lo, hi = _first_above(c, p - eps), _first_above(c, p + eps)
    if lo is None:
        kcs = [1]
    elif hi is None:                                               # an f32 cumsum may or may not pass p at any index from lo on
        kcs = sorted({1} | set(range(lo + 1, n + 1)))
    else:
        kcs = range(lo + 1, hi + 2)
    out = set()
    for kc in kcs:
        t = float(u) * c[kc - 1]
        a, b = _first_above(c[:kc], t - eps), _first_above(c[:kc], t + eps)
        a = kc - 1 if a is None else a
        b = kc - 1 if b is None else b
        for j in range(a, b + 1):
            out.add(int(order[j]))
            if qo[j] <= 0.0:
                continue
            for step in (-1, 1):                                   # neighbours in the order that f32 expf may tie with j or swap with it
                k = j + step
                while 0 <= k < n and abs(qo[k] - qo[j]) <= REL * max(qo[k], qo[j]):
                    if bits[order[k]] != bits[order[j]]:
                        out.add(int(order[k]))
                    k += step
    return out


def allowed_bits(words, off, n):
    """Bit off + c of the row's mask for the n classes of a head."""
    col = off + np.arange(n)
    return ((np.asarray(words, dtype=np.uint32)[col >> 5] >> (col & 31).astype(np.uint32)) & 1).astype(bool)


def position(logits, sizes, offs, T, P, u8, pad, allow=None, order=None, given=None, chosen0=None):
    """One position of one row. logits: the raw (vocab,) f32 row; T, P: 8 f32 each; u8: the 8 f64 draws; pad: the heads' first special ids;
    allow: the row's mask words or None; order = (floor, prev0, prev1) of a time-ordered row (floor >= 0) or None; given: 8 ids, -1 = free, or
    None. chosen0: head 0's id where the caller follows an implementation's own tokens (used only if it is acceptable and head 0 is not
    decided). Returns (sets, logged): 8 sets of acceptable ids, and whether the position logs its logits row (False: all 8 heads given)."""
    given = [-1] * 8 if given is None else [int(v) for v in given]
    if all(v >= 0 for v in given):
        return [{v} for v in given], False
    low0 = low1 = 0
    prev0 = -1
    if order is not None and order[0] >= 0:
        floor, p0, p1 = (int(v) for v in order)
        bar = p0 < pad[0]
        low0 = max(floor, p0 if bar else 0)
        if bar and p1 < pad[1]:
            low1, prev0 = p1, p0
    sets, alw = [], []
    for h in range(8):
        n, off = int(sizes[h]), int(offs[h])
        ok = allowed_bits(allow, off, n) if allow is not None else np.ones(n, dtype=bool)
        if h == 0 and low0 > 0:
            ok = ok & (np.arange(n) >= low0)
        alw.append(ok)
        sets.append(head_ids(logits[off:off + n], T[h], P[h], u8[h], ok))
    if low1 > 0 and given[1] < 0:                                  # head 1's second pass: b0 = head 0's id after forcing
        if given[0] >= 0:
            b0s = {given[0]}
        elif chosen0 is not None and int(chosen0) in sets[0]:
            b0s = {int(chosen0)}
        else:
            b0s = sets[0]
        same = {b0 == prev0 for b0 in b0s}
        if True in same:
            n, off = int(sizes[1]), int(offs[1])
            again = head_ids(logits[off:off + n], T[1], P[1], u8[1], alw[1] & (np.arange(n) >= low1))
            sets[1] = again | (sets[1] if False in same else set())
    for h in range(8):
        if given[h] >= 0:
            sets[h] = {given[h]}
    return sets, True


def done_flag(sets, pad, stop0):
    """The row form's done flag: any final id >= pad[h], head 0 tested against the row's stop bar. None where the acceptable ids disagree."""
    thr = [int(stop0)] + [int(v) for v in pad[1:]]
    if any(all(v >= thr[h] for v in s) for h, s in enumerate(sets)):
        return True
    if not any(v >= thr[h] for h, s in enumerate(sets) for v in s):
        return False
    return None


def done_of(ids, pad, stop0):
    return bool(ids[0] >= stop0 or any(int(ids[h]) >= int(pad[h]) for h in range(1, 8)))


# ================================================================================================================ the case tables
D_DEFAULT = [262, 134, 135, 262, 134, 38, 260, 55]                 # 1280 columns: 40 full mask words
D_EDGE_NARROW = [262, 134, 135, 272, 185, 38, 260, 55]             # 1341 columns (29 bits in the last word); 272 = SMP_W; 272 + 185 + 55 = 512 ranked
D_EDGE_WIDE = [1088, 134, 135, 273, 134, 38, 260, 55]              # the head limit, and the first head over SMP_W
DICTS = {'default': D_DEFAULT, 'edge-narrow': D_EDGE_NARROW, 'edge-wide': D_EDGE_WIDE}
T_DEFAULT = [1.2, 1.2, 5, 1, 2, 5, 5, 1.2]
P_DEFAULT = [1, 1, 1, .9, .9, 1, 1, .9]
S = 64                                                             # decoder positions
B = 16                                                             # rows (PB_DECODE_BATCH_MAX)
EXTRA = 2                                                          # steps launched behind the last position: finished rows must stay finished
# name -> (dictionary, T, P, form, use_graph). Beside the eight planned settings: 'no-prefix', a threshold above 1 / (1 + 1e-5), which no prefix
# exceeds, on the two ranked heads small enough that eps does not reach it (heads 4 and 7: (n + 8) 2^-24 < 1e-5 - 1e-7); and 'exact-cut', whose
# threshold IS the first cumulative sum of a 'pair' row (_exact_pair; PLAN_EXACT, since a ladder, an even plateau or an even flat head would
# put a cumulative sum on that threshold too, undecidably).
SETTINGS = {
    'default': ('default', T_DEFAULT, P_DEFAULT, 'narrow', 1),
    'ranked-01': ('default', T_DEFAULT, [.9, .9, 1, 1, 1, 1, 1, 1], 'narrow', 0),
    'all-1': ('default', T_DEFAULT, [1] * 8, 'narrow', 1),
    'all-.9': ('default', T_DEFAULT, [.9] * 8, 'wide', 1),
    'cold': ('default', [.05] * 8, P_DEFAULT, 'narrow', 0),
    'no-prefix': ('default', T_DEFAULT, [1, 1, 1, .9, .9999999, 1, 1, .9999999], 'narrow', 1),
    'edge-narrow': ('edge-narrow', T_DEFAULT, P_DEFAULT, 'narrow', 1),
    'edge-wide': ('edge-wide', T_DEFAULT, P_DEFAULT, 'wide', 0),
    'edge-wide-1088': ('edge-wide', T_DEFAULT, [.9, 1, 1, .9, 1, 1, 1, .9], 'wide', 1),
    'exact-cut': ('default', T_DEFAULT, [1, 1, 1, P_EXACT, P_EXACT, 1, 1, P_EXACT], 'narrow', 0),
}
# the order keeps the rows alive: a one-hot or flat row whose top class a floor or a mask removes leaves the special ids as likely as the rest
PLAN = ([('ladder', d) for d in range(6)] + [('plateau', (mi, d)) for mi in range(4) for d in range(4)] +
        [('random', (scale, k)) for scale in (.5, 3., 10.) for k in range(8)] + [('onehot', c) for c in (0, 1, 63, 64, 65)] +
        [('flat', d) for d in range(4)] + [('onehot', -1)])
PLAN_B1 = ([('ladder', 0), ('ladder', 4), ('plateau', (1, 1)), ('plateau', (2, 2)), ('onehot', 0), ('onehot', 64), ('onehot', 64)] +
           [('random', (scale, 8 + k)) for scale in (.5, 3., 10.) for k in range(2)] + [('flat', 1), ('flat', 2)])
PLAN_EXACT = [('pair', d) for d in range(6)] + [('random', (scale, k)) for scale in (.5, 3., 10.) for k in range(8)] + [('onehot', -1)]


def form_of(sizes, P):
    ranked = sum(n for n, p in zip(sizes, P) if np.float32(p) < 1)
    return 'wide' if max(sizes) > 272 or ranked > 512 else 'narrow'


def layout(sizes):
    n = np.asarray(sizes, dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(n)])
    return n, offs, n - 6, int(offs[8])


def _perm(h, n_ord, salt):
    return np.random.RandomState(1000 * salt + h).permutation(n_ord)


def _plateau_m(target_kc, T, p, n, n_ord):
    """The least m for which m classes tied at the top give target_kc candidates (the head's ordinary classes at the most)."""
    if np.float32(p) >= 1:
        return min(target_kc, n_ord)
    for m in range(1, n_ord + 1):
        lg = np.full(n, -60.0 * T, dtype=np.float32)
        lg[:m] = 0
        c = np.cumsum(np.sort(quotients(lg, T)[2])[::-1])
        lo, hi = _first_above(c, float(np.float32(p)) - eps_of(n)), _first_above(c, float(np.float32(p)) + eps_of(n))
        if lo is not None and lo == hi and lo + 1 == target_kc:     # target_kc candidates, and decided so
            return m
    return n_ord


def _decided_kc(lg, T, p, n):
    c = np.cumsum(np.sort(quotients(lg, T)[2])[::-1])
    lo, hi = _first_above(c, p - eps_of(n)), _first_above(c, p + eps_of(n))
    return p >= 1.0 or lo == hi


def _head_row(kind, arg, h, n, T, p, K, rng, seed=0):
    """(logits of the head, the draws aimed at it: row r of variant d takes draws[(r + d) % len])."""
    n_ord = n - 6
    T32, p32 = float(np.float32(T)), float(np.float32(p))
    MID = MID0 - .03 * (seed % 5)
    mids = lambda kc: [(min(j, kc - 1) + MID) / kc for j in (0, K - 1, K, kc - 1)]
    if kind == 'flat':
        lg = np.full(n, 1.5, dtype=np.float32)
        if not _decided_kc(lg, T32, p32, n):                       # 0.9 n is a whole number (n = 260): the flat head's own cut sits on p; all but the last class are flat then
            lg[n - 1] -= np.float32(60.0 * T32)
        return lg, mids(free_kc(lg, T32, p32)[0])
    if kind == 'onehot':
        lg = np.zeros(n, dtype=np.float32)
        lg[n - 1 if arg < 0 else arg % n_ord] = 60.0
        return lg, None
    if kind == 'pair':                                             # two tied classes, on both sides of class 64 where the head has one, and exact zeros
        lg = np.full(n, -200.0 * T32, dtype=np.float32)
        lg[[_perm(h, min(n_ord, 64), 3)[0], n_ord - 1 - _perm(h, min(n_ord, 64), 4)[0] % (n_ord // 2)]] = 0
        return lg, [.26, .74, 0.0, JUST_BELOW_1, .48, .52]
    if kind == 'ladder':
        perm, L = _perm(h, n_ord, 1), min(12, n_ord)
        lg = np.full(n, -60.0 * T32, dtype=np.float32)
        lg[perm[:L]] = (-np.arange(L) * T32 * np.log(2.0)).astype(np.float32)
        kc, order, q = free_kc(lg, T32, p32)
        cdf = np.concatenate([[0.0], np.cumsum(q[order])[:kc]])
        cdf /= cdf[-1]
        return lg, [float(v) for v in cdf[:-1] + MID * (cdf[1:] - cdf[:-1])] + [0.0, JUST_BELOW_1]
    if kind == 'plateau':
        target = (K, K + 1, 2 * K, 2 * K + 1)[arg[0]]
        m = _plateau_m(target, T32, p32, n, n_ord)
        lg = np.full(n, -60.0 * T32, dtype=np.float32)
        lg[_perm(h, n_ord, 2 + 10 * seed)[:m]] = 0
        return lg, mids(free_kc(lg, T32, p32)[0])
    if kind == 'random':
        lg = (rng.standard_normal(n) * arg[0]).astype(np.float32)
        lg[n_ord:] -= np.float32(40.0 * T32)                       # no special id is sampled: the rows live to meet the later positions
        return lg, None
    raise ValueError(kind)


def masks_for(sizes):
    """The allow masks of a dictionary, (4, words) uint32; every mask keeps each head's special ids.
      0 'notop'        classes 0 and 64 and the ladder's first class removed from every head: the arg-max of those positions
      1 'alternating'  in each head's first and last word only the odd columns
      2 'oneclass'     one ordinary class per head
      3 'lastcol'      only the last column of the vocabulary (and the specials): the partly filled last word"""
    n, offs, pad, vocab = layout(sizes)
    words = (vocab + 31) // 32
    bits = np.ones((4, vocab), dtype=bool)
    bits[2:] = False
    for h in range(8):
        o, nh, n_ord = int(offs[h]), int(n[h]), int(pad[h])
        for c in (0, 64 % n_ord, int(_perm(h, n_ord, 1)[0])):
            bits[0, o + c] = False
        if int(bits[0, o:o + nh].sum()) % 10 == 0:                 # a flat head of 10 k classes has a cumulative sum on p = 0.9: one class more goes
            bits[0, o + 1] = False
        cols = np.arange(o, o + nh)
        edge = ((cols >> 5) == (o >> 5)) | ((cols >> 5) == ((o + nh - 1) >> 5))
        bits[1, cols[edge & (cols % 2 == 0)]] = False
        bits[2, o + (37 * h + 5) % n_ord] = True
        bits[:, o + n_ord:o + nh] = True
    bits[3, vocab - 1] = True
    out = np.zeros((4, words), dtype=np.uint32)
    for m in range(4):
        for c in np.flatnonzero(bits[m]):
            out[m, c >> 5] |= np.uint32(1) << np.uint32(c & 31)
    return out


def rules_for(sizes, variant):
    """The 16 rows' rules: floor (-1 = not time-ordered), stop bar (pad0 = none), mask index (-1 = none), given ids (S, 8), -1 = free."""
    n, offs, pad, vocab = layout(sizes)
    pad0 = int(pad[0])
    rows = [dict(floor=-1, stop=pad0, mask=-1, given=np.full((S, 8), -1, dtype=np.int16)) for _ in range(B)]
    rows[1]['mask'] = 2 if variant % 2 == 0 else 3
    for r, fl in zip(range(2, 8), (0, 1, 63, 64, 65, pad0 - 1)):
        rows[r]['floor'] = fl
    rows[8]['floor'] = 0                                           # a given head 0 that makes b0 == prev0, and every fifth position breaks it
    rows[8]['given'][:, 0] = 7
    rows[8]['given'][4::5, 0] = 9
    rows[9]['floor'] = 0                                           # ... and a given head 1 at the odd positions: no second pass there
    rows[9]['given'][:, 0] = 7
    rows[9]['given'][1::2, 1] = 5
    for i in (3, 4):                                               # all 8 heads given
        rows[10]['given'][i] = [(i + 11 * h) % int(pad[h]) for h in range(8)]
    rows[10]['given'][20, 4] = int(pad[4]) + 3                     # a given special id ends the row
    rows[11]['stop'] = 100
    rows[12]['stop'] = 0
    rows[13]['mask'] = 0
    rows[14]['mask'] = 1
    rows[15].update(mask=1, floor=64)                              # a mask with a floor and with head 1's second pass
    rows[15]['given'][:, 0] = 70
    return rows


def rules_b1(sizes):
    """One rule each for the single-row form (it has no done flag: no given special id, and a stop bar changes nothing)."""
    r = rules_for(sizes, 0)
    r[10]['given'][20, 4] = -1
    return [r[0], r[6], r[13], r[8], r[10], r[15], r[11]]


_CASES = {}
# (setting, b1) -> the seed of its plateau classes, its random rows and draws and the aim point of its crafted draws (0 where none is named),
# chosen so that the reference alone decides every crafted case under every row's rule: a draw aimed at the free rule's interval j of kc can
# sit on a boundary i / kc' of the intervals that a mask or a floor leaves, and 10, 20 or 30 tied classes left of a plateau put a
# cumulative sum on p = 0.9. tests/test_sampler_ref_cpu.py asserts the outcome.
SEEDS = {('default', False): 1, ('default', True): 1, ('cold', False): 1, ('no-prefix', False): 1, ('edge-narrow', False): 12, ('edge-wide-1088', False): 3}


def case(name, b1=False):
    """The inputs of one setting: sizes / offs / pad / vocab, T / P (f32), form, use_graph, logits (npos, vocab) f32, kinds (npos), U (rows, S, 8)
    f64, rules (rows), masks. b1: the single-row form's runs, one row per run (rules_b1), over PLAN_B1."""
    key = (name, b1)
    if key in _CASES:
        return _CASES[key]
    dname, T, P, form, use_graph = SETTINGS[name]
    seed = SEEDS.get(key, 0)
    sizes = DICTS[dname]
    n, offs, pad, vocab = layout(sizes)
    assert form_of(sizes, P) == form
    K = 5 if form == 'narrow' else 17
    idx = list(SETTINGS).index(name)
    plan = PLAN_B1 if b1 else (PLAN_EXACT if name == 'exact-cut' else PLAN)
    rules = rules_b1(sizes) if b1 else rules_for(sizes, 0 if name == 'exact-cut' else idx)      # exact-cut: six tied specials alone ('lastcol') put the third sum on its threshold
    rng = np.random.RandomState(7000 + idx + (500 if b1 else 0) + 100 * seed)
    logits = np.zeros((len(plan), vocab), dtype=np.float32)
    U = rng.random_sample((len(rules), S, 8))
    for i, (kind, arg) in enumerate(plan):
        for h in range(8):
            lg, draws = _head_row(kind, arg, h, int(n[h]), T[h], P[h], K, rng, seed)
            logits[i, offs[h]:offs[h + 1]] = lg
            if draws is not None:
                d = arg if kind in ('flat', 'ladder', 'pair') else arg[1]
                for r in range(len(rules)):
                    U[r, i, h] = draws[((0 if b1 else r) + d) % len(draws)]
    c = dict(name=name, sizes=n, offs=offs, pad=pad, vocab=vocab, T=np.asarray(T, dtype=np.float32), P=np.asarray(P, dtype=np.float32), form=form,
             use_graph=use_graph, logits=logits, kinds=[k for k, _ in plan], U=U, rules=rules, masks=masks_for(sizes), sos=pad + 2)
    _CASES[key] = c
    return c


def follow(c, r, tok=None, rows_form=True, logits=None):
    """Row r of a case, position by position: yields (i, sets, logged, done). tok (npos, 8): the ids an implementation wrote; the row is then
    followed on THOSE (prev = tok[i - 1]), so one wrong position does not cascade. Without tok the lowest acceptable id is taken. Ends behind
    the position where the row is done (rows_form only). logits (npos, vocab): the rows an implementation logged, read in place of the table's."""
    rule = c['rules'][r]
    allow = c['masks'][rule['mask']] if rule['mask'] >= 0 else None
    prev = [int(v) for v in c['sos']]
    for i in range(len(c['kinds'])):
        order = (rule['floor'], prev[0], prev[1]) if rule['floor'] >= 0 else None
        sets, logged = position(c['logits'][i] if logits is None else logits[i], c['sizes'], c['offs'], c['T'], c['P'], c['U'][r, i], c['pad'], allow, order, rule['given'][i],
                                chosen0=None if tok is None else tok[i][0])
        done = done_flag(sets, c['pad'], rule['stop'])
        ids = [int(v) for v in tok[i]] if tok is not None else [min(s, default=0) for s in sets]
        if done is None:
            done = done_of(ids, c['pad'], rule['stop'])
        yield i, sets, logged, done
        if done and rows_form:
            return
        prev = ids
