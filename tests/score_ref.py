"""Reference of the scoring kernels (csrc/pb_score.hip: pb_token_scores, pb_seq_scores) in plain torch, and the inputs their tests share.

token_scores() is the header's definition per (row, head), on float64 tensors the reference and on float32 tensors the float32 model
the kernel's error is measured against (tests/test_score_kernels_gpu.py); tests/test_score_ref_cpu.py checks it against
torch.log_softmax, -(p log p).sum() and a stable argsort.
  logp     x[target] - max - log sum e,   e = exp(x - max)
  entropy  log sum e - sum e (x - max) / sum e,   a term with e == 0 counting as 0
  rank     columns with a greater logit, or an equal one at a lower index
  a target outside [0, n) has the logit 0 (as the kernel documents it): rank = #(x > 0) + #(x == 0 and column < target), so a
  target < 0 counts none of the zeros and a target >= n all of them
  mask == 0: 0 / 0 / -1, whatever the row holds
The scales of the measure, always in float64: S_entropy = [n > 1] + log sum e + sum p |x - max| and S_logp = |x_t - max| + S_entropy.
sum e >= 1 is rounded to float32 in front of the logarithm: an error of up to 2^-24 sum e / sum e = 2^-24 in log sum e, which is
the [n > 1] term (a head of one class has sum e = 1 exactly). Without it a two-class head, or a spike whose other terms underflow,
has a scale of 1e-70 under a float32 error of 2^-24.

OPTIONS names roundings the kernel documents and a plain float32 evaluation does not make; a test passes one only with a reason.
"""
import math

import torch

LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453

# exp2: __expf(d) is the hardware's 2^(d * log2 e): the float32 product d * log2 e is rounded before the exponential, an error of
#       up to 2^-24 |d| log2 e in the exponent, i.e. a relative 2^-24 |d| in e, where torch.exp is within an ulp for every d.
# log2: __logf(s) is log2(s) * ln 2, one more rounding than torch.log.
OPTIONS = ('exp2', 'log2')

DEFAULT_SIZES = [262, 134, 135, 262, 134, 38, 260, 55]
LAYOUTS = {
    'narrow_edges': [320, 1, 2, 63, 64, 65, 128, 129],          # the largest register-form row
    'switch': [321, 1, 2, 63, 64, 65, 128, 129],                # one class more in head 0: the whole row goes wide
    'narrow_b': [319, 256, 257, 192, 193, 7, 38, 262],          # other register-form widths
    'wide_edges': [1088, 1087, 1025, 1024, 641, 640, 321, 1],   # every wide-form sweep edge
    'sweep_wide': [321, 7, 7, 7, 7, 7, 7, 7],                   # the smallest wide row
    'default': DEFAULT_SIZES,
}
FAMILIES = ('random', 'uniform', 'plateau', 'zero_tie', 'spike', 'offset', 'ladder', 'outside')
OUTSIDE = (-1, None, 32767, -32768)                             # None: the head's n


def offsets(sizes):
    off = [0]
    for n in sizes:
        off.append(off[-1] + int(n))
    return off


def edge_classes(n):
    """{0, 1, n - 2, n - 1} and 64 k - 2 .. 64 k + 1 for every k >= 1, inside [0, n): both sides of every lane sweep of the head."""
    s = {0, 1, n - 2, n - 1}
    for k in range(64, n + 2, 64):
        s.update((k - 2, k - 1, k, k + 1))
    return sorted(c for c in s if 0 <= c < n)


# ------------------------------------------------------------------------------------------------------------------ token scores
def token_scores(x, target, mask, off, exp2=False, log2=False):
    """x (T, V) float64 or float32, target (T, 8) integer, mask (T,), off: 9 offsets. Returns a dict of (T, 8) tensors: logp, entropy in
    x's dtype, rank int64, s_logp, s_entropy float64."""
    T = x.shape[0]
    dt, dev = x.dtype, x.device
    live = (mask != 0).to(dev)
    target = target.to(dev).long()
    out = {k: torch.zeros(T, 8, dtype=dt, device=dev) for k in ('logp', 'entropy')}
    out['rank'] = torch.full((T, 8), -1, dtype=torch.int64, device=dev)
    out['s_logp'] = torch.zeros(T, 8, dtype=torch.float64, device=dev)
    out['s_entropy'] = torch.zeros(T, 8, dtype=torch.float64, device=dev)
    zero = torch.zeros((), dtype=dt, device=dev)
    for i in range(8):
        o, n = off[i], off[i + 1] - off[i]
        seg = x[:, o:o + n]
        t = target[:, i:i + 1]
        inside = (t >= 0) & (t < n)
        xt = torch.where(inside, seg.gather(1, t.clamp(0, n - 1)), zero)
        mx = seg.amax(-1, keepdim=True)
        d = seg - mx
        e = torch.exp2(d * LOG2E) if exp2 else torch.exp(d)
        se = e.sum(-1, keepdim=True)
        sed = torch.where(e > 0, e * d, zero).sum(-1, keepdim=True)
        lg = torch.log2(se) * LN2 if log2 else torch.log(se)
        col = torch.arange(n, device=dev)[None]
        rank = ((seg > xt) | ((seg == xt) & (col < t))).sum(-1)
        out['logp'][:, i] = torch.where(live, ((xt - mx) - lg)[:, 0], zero)
        out['entropy'][:, i] = torch.where(live, (lg - sed / se)[:, 0], zero)
        out['rank'][:, i] = torch.where(live, rank, torch.full_like(rank, -1))
        # the scales, in float64 whatever x is
        s64, xt64 = seg.double(), xt.double()
        mx64 = s64.amax(-1, keepdim=True)
        d64 = s64 - mx64
        e64 = torch.exp(d64)
        se64 = e64.sum(-1, keepdim=True)
        s_en = (float(n > 1) + torch.log(se64) + (e64 * d64.abs()).sum(-1, keepdim=True) / se64)[:, 0]
        z64 = torch.zeros((), dtype=torch.float64, device=dev)
        out['s_entropy'][:, i] = torch.where(live, s_en, z64)
        out['s_logp'][:, i] = torch.where(live, (xt64 - mx64).abs()[:, 0] + s_en, z64)
    return out


def figures(got, ref, scale, pick=None):
    """|got - ref| / (2^-24 scale) per element with a positive scale (of `pick`, a boolean mask, if given); an empty tensor if none."""
    use = scale > 0
    if pick is not None:
        use = use & pick
    return (got.double() - ref.double()).abs()[use] / (2.0 ** -24 * scale[use])


# ------------------------------------------------------------------------------------------------------------------ sequence sums
def _chain(p):
    """sum over dim 1 of (B, S, 8) in the order the header gives for pb_seq_scores: 32 running sums, sum g taking the positions g, g + 32,
    g + 64, ... in order, then the 32 sums added in order of g. Every addition is rounded to p's dtype."""
    B, S, _ = p.shape
    n = (S + 31) // 32
    q = torch.zeros(B, n * 32, 8, dtype=p.dtype, device=p.device)
    q[:, :S] = p
    q = q.view(B, n, 32, 8)
    acc = torch.zeros(B, 32, 8, dtype=p.dtype, device=p.device)
    for j in range(n):
        acc = acc + q[:, j]
    tot = torch.zeros(B, 8, dtype=p.dtype, device=p.device)
    for g in range(32):
        tot = tot + acc[:, g]
    return tot


def seq_sums(logp, entropy, rank, mask, chain=False):
    """logp, entropy (B * S, 8) or (B, S, 8), rank the same in any integer dtype, mask (B, S). Returns (out, absum), both (B, 4, 8): out in
    logp's dtype = {sum m logp, sum m entropy, sum m [rank == 0], sum m} over the positions with m != 0 (a masked position adds
    nothing, whatever it holds), absum float64 = the sums of |term| in float64. entropy / rank None: a plane of zeros.
    chain: the named option of the float32 model for pb_seq_scores. The header fixes the kernel's order of summation (what makes two
    launches bit-equal): running sums of S / 32 and then of 32 terms. torch.sum adds in a tree, and on terms of one sign -- logp <= 0,
    entropy >= 0, weights > 0 -- a chain's rounding errors, each half an ulp of a running sum that only grows, add up to about
    2^-24 sqrt(32 / 9) = 1.9 units of the total against a tree's 0.5 to 0.9: a chain of 32 passes 4 x the tree's figure at two standard
    deviations, with nothing wrong in it. The model therefore adds in the documented order; its products m * v are rounded on their own
    where the kernel may fuse them into the addition, and it knows nothing of the kernel's results."""
    B, S = mask.shape
    dt = logp.dtype

    def planes(dtype):
        m = mask.to(dtype)[:, :, None]
        on = (mask != 0)[:, :, None]
        z = torch.zeros((), dtype=dtype, device=mask.device)
        lp = torch.where(on, m * logp.reshape(B, S, 8).to(dtype), z)
        en = torch.where(on, m * entropy.reshape(B, S, 8).to(dtype), z) if entropy is not None else torch.zeros(B, S, 8, dtype=dtype, device=mask.device)
        hit = torch.where(on & (rank.reshape(B, S, 8) == 0), m, z).expand(B, S, 8) if rank is not None else torch.zeros(B, S, 8, dtype=dtype, device=mask.device)
        return lp, en, hit, m.expand(B, S, 8)

    out = torch.stack([_chain(p.contiguous()) if chain else p.sum(1) for p in planes(dt)], 1)
    absum = torch.stack([p.abs().sum(1) for p in planes(torch.float64)], 1)
    return out, absum


# ------------------------------------------------------------------------------------------------------------------ shared inputs
def _block(fam, sizes, off, R, g):
    """R rows of one family: (x float32 (R, V), target int64 (R, 8)). Row r gives head i the target edge_classes(n_i)[r mod len]."""
    V = off[8]
    x = torch.empty(R, V)
    tgt = torch.empty(R, 8, dtype=torch.int64)
    for i, n in enumerate(sizes):
        ed = edge_classes(n)
        t = torch.tensor([ed[r % len(ed)] for r in range(R)])
        rnd = 2.0 * torch.randn(R, n, generator=g)
        rows = torch.arange(R)
        if fam == 'random':
            seg = rnd
        elif fam == 'uniform':
            seg = (0.25 * i - 3.0 + (rows % 7).float())[:, None].expand(R, n).clone()
        elif fam == 'plateau':
            seg = rnd
            for dlt in (-64, -1, 0, 1, 64):
                c = t + dlt
                ok = (c >= 0) & (c < n)
                seg[rows[ok], c[ok]] = 50.0
        elif fam in ('zero_tie', 'outside'):
            # zero_tie: +0.0 and -0.0 among negative logits, and on t - 64, t - 1, t, t + 1, t + 64; outside: 2 randn with zeros planted
            seg = -rnd.abs() - 0.5 if fam == 'zero_tie' else rnd
            planted = torch.rand(R, n, generator=g) < 0.25
            sign = torch.where(torch.rand(R, n, generator=g) < 0.5, 0.0, -0.0)
            seg = torch.where(planted, sign, seg)
            for k, dlt in enumerate((-64, -1, 0, 1, 64)):
                c = t + dlt
                ok = (c >= 0) & (c < n)
                seg[rows[ok], c[ok]] = torch.where((rows[ok] + k) % 2 == 0, 0.0, -0.0)
        elif fam == 'spike':
            seg = torch.full((R, n), -80.0)
            s = t.clone()
            if i % 2 == 1 and n > 1:                                    # odd heads: the target is off the spike
                s = (t + 64) % n
                s = torch.where(s == t, (t + 1) % n, s)
            seg[rows, s] = 80.0
        elif fam == 'offset':
            seg = rnd + 3e4
        elif fam == 'ladder':
            seg = (-0.37 * torch.arange(n).float())[None].expand(R, n).clone()
        else:
            raise ValueError(fam)
        x[:, off[i]:off[i + 1]] = seg
        tgt[:, i] = t
    return x, tgt


def make_case(sizes, seed=0):
    """The rows of one layout: one block per family of FAMILIES, R = the longest edge list of the layout's heads. The zero_tie block ends
    with four more rows and the 'outside' block is four rows, in which head i of row j has the target OUTSIDE[(i + j) % 4]; then three
    masked rows (NaN logits, target 32767, mask 0) are put first, in the middle and last.
    Returns dict(x float32 (T, V), target int16 (T, 8), mask float32 (T,), fam: list of T family names ('masked' included), off)."""
    off = offsets(sizes)
    g = torch.Generator().manual_seed(7919 * seed + off[8])
    R = max(len(edge_classes(n)) for n in sizes)
    xs, ts, fams = [], [], []

    def outside(t):
        for j in range(t.shape[0]):
            for i, n in enumerate(sizes):
                v = OUTSIDE[(i + j) % 4]
                t[j, i] = n if v is None else v
        return t

    for fam in FAMILIES:
        if fam == 'outside':
            x, t = _block(fam, sizes, off, 4, g)
            t = outside(t)
        else:
            x, t = _block(fam, sizes, off, R, g)
        xs.append(x); ts.append(t); fams += [fam] * x.shape[0]
        if fam == 'zero_tie':
            x, t = _block(fam, sizes, off, 4, g)
            xs.append(x); ts.append(outside(t)); fams += [fam] * 4
    x, t = torch.cat(xs), torch.cat(ts)
    n = x.shape[0]
    nan_row, t_row = torch.full((1, off[8]), float('nan')), torch.full((1, 8), 32767, dtype=torch.int64)
    h = n // 2
    x = torch.cat([nan_row, x[:h], nan_row, x[h:], nan_row])
    t = torch.cat([t_row, t[:h], t_row, t[h:], t_row])
    fams = ['masked'] + fams[:h] + ['masked'] + fams[h:] + ['masked']
    mask = torch.tensor([0.0 if f == 'masked' else 1.0 for f in fams])
    return dict(x=x.contiguous(), target=t.to(torch.int16).contiguous(), mask=mask, fam=fams, off=off, sizes=list(sizes))


def worst_by_family(case, got, ref):
    """{(output, family): the largest figure of got against ref (dicts of logp / entropy; ref carries the scales)} over the live elements
    with a positive scale; families without such an element are left out."""
    res = {}
    for name, sc in (('logp', 's_logp'), ('entropy', 's_entropy')):
        for fam in FAMILIES:
            rows = torch.tensor([f == fam for f in case['fam']], device=ref[sc].device)[:, None].expand_as(ref[sc])
            f = figures(got[name], ref[name], ref[sc], rows)
            if f.numel():
                res[(name, fam)] = float(f.max())
    return res


assert math.isclose(LOG2E * LN2, 1.0)
