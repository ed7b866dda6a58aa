"""Host restatement (numpy and plain Python) of the whole corruption kernel (csrc/pb_corrupt.hip), in two layers.

decide() draws the random DECISIONS of one sample from the kernel's Philox stream and returns them in the layout pb_corrupt_replay takes
(include/pianobart_hip.h): counter (idx, sample, purpose, 0xC0221), key (seed low, seed high), 7 rounds (tests/philox_ref.py).
  purpose 0        the in-kernel choice, 1 + x % 5 (draw_choice)
  purpose 1        one selection key per position: deletion removes the int(S p) positions of lowest (key, index); the mask selects the
                   k = round(S p) lowest, of which the round(0.8 k) lowest become MASK rows, the next min(round(0.1 k), k - k80)
                   random rows, the rest keep their row (Python's round: halves go to the even neighbour)
  purpose 2        the random row of position i: counters 2 i and 2 i + 1, column c = word c mod n_tokens[c]
  purpose 3        one key per bar value; the bars are laid out by (key, bar value)
  purpose 4 + att  infilling attempt att, one counter per step: word x starts a span when u(x) < float32(p / 3), u(x) = (x >> 8) / 2^24;
                   word y gives the Poisson(3) length by inversion
  purpose 5        the rotation offset, x % S
apply() is the deterministic half, Pretrainer.gen_mask of the reference with its random draws replaced by the decisions: the rows are
built as Python lists, the way the reference builds them. tests/test_corrupt_ref_cpu.py holds apply() to the oracle's gen_mask and
to the goldens; tests/test_corrupt_kernels_gpu.py holds the kernel to apply(decide()) and to apply() on hand-made decisions.

The Poisson inversion is the one place where float32 operation order matters: the kernel accumulates the cdf in float32 and the
compiler may fuse `cdf += pk` with the multiply before it. decide() therefore computes the cdf in float32 AND in float64 and counts a
draw as ambiguous when u lies within AMBIGUITY = 2^-19 of a cdf value it is compared with (or when the two disagree): the float32 cdf
is the outcome of at most about 30 roundings of quantities below 1, each at most 2^-25, so it is within 2^-20 of the exact one. A
(seed, S, p) is used on the GPU only when its count is zero; the band selects inputs and loosens no comparison.
"""
import math

import numpy as np

from tests.philox_ref import philox4x32

TAG = 0xC0221
AMBIGUITY = 2.0 ** -19
ATTEMPTS = 10
SMAX = 2048

# Found by search_tie() (tests/test_corrupt_ref_cpu.py repeats the searches): the first seed from TIE_SEED0 on under which sample
# TIE_POS_SAMPLE holds two equal keys of purpose 1 among its 2048 positions / sample TIE_BAR_SAMPLE two equal keys of purpose 3 among the
# bar values 0 .. 2047.
TIE_SEED0 = (0x51ED << 32) + 1
TIE_POS_SAMPLE, TIE_BAR_SAMPLE = 2, 3
TIE_POS = (90078349099105, 1277, 1699)          # (seed, i, j): the keys of positions i < j are equal
TIE_BAR = (90078349103357, 675, 1646)           # (seed, i, j): the keys of bar values i < j are equal


def tie_percent(S=SMAX):
    """A mask_percent under which the tie of TIE_POS decides the outcome: with r the rank of position i by (key, index), position j
    has rank r + 1, and p = (r + 1.25) / S makes int(S p) = round(S p) = r + 1, so that i is taken and j is not."""
    seed, i, j = TIE_POS
    r = ranks(words(seed, TIE_POS_SAMPLE, 1, np.arange(S))[0], np.arange(S))
    assert r[j] == r[i] + 1
    p = (int(r[i]) + 1.25) / S
    assert int(S * p) == round(S * p) == r[i] + 1
    return p


def replay_stride(S):
    return max(10 * S, 65536)


def words(seed, sample, purpose, idx):
    """The four 32-bit words (uint64 arrays) of the counters (idx, sample, purpose, TAG) under the 64-bit seed."""
    seed = int(seed)
    return philox4x32(np.asarray(idx, dtype=np.uint64), sample, purpose, TAG, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, 7)


def draw_choice(seed, sample):
    return 1 + int(words(seed, sample, 0, [0])[0][0]) % 5


def ranks(key, tie):
    """rank[i] = place of i in the order by (key, tie)."""
    order = np.lexsort((tie, key))
    r = np.empty(len(key), dtype=np.int64)
    r[order] = np.arange(len(key))
    return r


def mask_counts(S, p):
    k = round(S * p)
    k80, k10 = round(k * 0.8), round(k * 0.1)
    return k, k80, min(k10, k - k80)


def _u01(x):
    return ((x >> np.uint64(8)).astype(np.float64) / 16777216.0).astype(np.float32)      # 24 bits: exact in float32


def _cdf32():
    pk = np.float32(0.049787068)
    cdf = [pk]
    for j in range(1, 65):
        pk = np.float32(pk * np.float32(np.float32(3.0) / np.float32(j)))
        cdf.append(np.float32(cdf[-1] + pk))
    return np.array(cdf, dtype=np.float32)


def _cdf64():
    out, acc = [], 0.0
    for j in range(65):
        acc += math.exp(-3.0) * 3.0 ** j / math.factorial(j)
        out.append(acc)
    return np.array(out)


CDF32, CDF64 = _cdf32(), _cdf64()


def poisson3(u):
    """Poisson(3) by inversion for float32 uniforms u: the smallest j <= 64 with u <= cdf[j] (j = 64 when there is none below it),
    and per draw whether it is ambiguous."""
    u = np.asarray(u, dtype=np.float32)
    z32 = (u[:, None] > CDF32[None, :64]).sum(1)                 # the cdf does not decrease: the count of cdf values below u
    z64 = (u.astype(np.float64)[:, None] > CDF64[None, :64]).sum(1)
    j = np.arange(64)[None, :]
    compared = j <= np.minimum(z32, 63)[:, None]
    near = (np.abs(u.astype(np.float64)[:, None] - CDF64[None, :64]) < AMBIGUITY) & compared
    return z32.astype(np.int64), near.any(1) | (z32 != z64)


def walk_spans(v, S):
    """The span process of one infilling attempt over its decisions v: the list of source indices (-1 = MASK row), or None when it
    has more than S entries."""
    src, i, s = [], 0, 0
    while i < S:
        d = int(v[s]); s += 1
        if d == 0:
            src += [i, -1]; i += 1
        elif d > 0:
            src.append(-1); i += d
        else:
            src.append(i); i += 1
    return src if len(src) <= S else None


def decide(seed, sample, choice, S, p, rows, n_tokens):
    """(dec int32[replay_stride(S)], rand_rows (S,8) int16 or None, number of ambiguous Poisson draws) of sample `sample`."""
    assert 1 <= choice <= 5 and 1 <= S <= SMAX
    dec = np.zeros(replay_stride(S), dtype=np.int32)
    rand_rows, ambiguous = None, 0
    idx = np.arange(S)
    if choice == 1:
        r = ranks(words(seed, sample, 1, idx)[0], idx)
        dec[:S] = r < int(S * p)
    elif choice == 2:
        k, k80, k10 = mask_counts(S, p)
        r = ranks(words(seed, sample, 1, idx)[0], idx)
        dec[:S] = np.where(r >= k, 0, np.where(r < k80, 1, np.where(r < k80 + k10, 2, 3)))
        a, c = words(seed, sample, 2, 2 * idx), words(seed, sample, 2, 2 * idx + 1)
        rand_rows = np.stack([w % np.uint64(n_tokens[col]) for col, w in enumerate(a + c)], axis=1).astype(np.int16)
    elif choice == 3:
        bars = np.unique(np.asarray(rows)[:, 0].astype(np.int64) & 0xFFFF)
        dec[bars] = ranks(words(seed, sample, 3, bars)[0], bars)
    elif choice == 4:
        thr = np.float32(p / 3.0)
        done = False
        for att in range(ATTEMPTS):
            x, y, _, _ = words(seed, sample, 4 + att, idx)
            start = _u01(x) < thr
            z, amb = poisson3(_u01(y[start]))
            v = np.full(S, -1, dtype=np.int32)
            v[start] = z
            dec[att * S:(att + 1) * S] = v
            if not done:                                          # the kernel stops drawing at the first attempt that fits
                ambiguous += int(amb.sum())
                done = walk_spans(v, S) is not None
    else:
        dec[0] = int(words(seed, sample, 5, [0])[0][0]) % S
    return dec, rand_rows, ambiguous


def apply(rows, choice, dec, rand_rows, S, p, pad_row, mask_row):
    """(out (S,8) int64, loss (S,) int64): gen_mask of the reference on `rows` (S,8) with the decisions `dec` in place of its draws."""
    rows = np.asarray(rows).astype(np.int64)
    pad, mask = (np.asarray(r).astype(np.int64) for r in (pad_row, mask_row))
    assert rows.shape == (S, 8)
    loss = np.zeros(S, dtype=np.int64)
    if choice == 1:
        k = int(S * p)
        deleted = [i for i in range(S) if dec[i] != 0]
        out = [rows[i] for i in range(S) if dec[i] == 0] + [pad] * k
        assert len(deleted) == k and len(out) == S, 'deletion takes exactly int(S p) positions'
        if deleted:
            loss[deleted[0]:] = 1
    elif choice == 2:
        out = []
        for i in range(S):
            kind = int(dec[i])
            out.append(mask if kind == 1 else np.asarray(rand_rows[i]).astype(np.int64) if kind == 2 else rows[i])
            loss[i] = kind != 0
    elif choice == 3:
        sentences = {}
        for row in rows:
            sentences.setdefault(int(row[0]) & 0xFFFF, []).append(row)
        out = []
        for bar in sorted(sentences, key=lambda b: (int(dec[b]), b)):
            out += sentences[bar]
        loss = (np.stack(out) != rows).any(1).astype(np.int64)
    elif choice == 4:
        for att in range(ATTEMPTS):
            src = walk_spans(dec[att * S:(att + 1) * S], S)
            if src is not None:
                out = [rows[s] if s >= 0 else mask for s in src] + [pad] * (S - len(src))
                loss = (np.stack(out) != rows).any(1).astype(np.int64)
                break
        else:
            out = list(rows)                                      # ten attempts too long: unchanged rows, no loss term
    else:
        ran = int(dec[0])
        out = list(rows[ran:]) + list(rows[:ran])
        loss[:] = ran != 0
    return np.stack(out).astype(np.int64), loss


def reference(seed, sample, choice, S, p, rows, n_tokens, pad_row, mask_row):
    """apply(decide()) of one sample; choice outside 1..5 draws it as the kernel does. Returns (out, loss, choice, ambiguous)."""
    if not 1 <= choice <= 5:
        choice = draw_choice(seed, sample)
    dec, rr, amb = decide(seed, sample, choice, S, p, rows, n_tokens)
    out, loss = apply(rows, choice, dec, rr, S, p, pad_row, mask_row)
    return out, loss, choice, amb


def search_tie(seed0, sample, purpose, n=SMAX, budget=200000, chunk=512):
    """The first seed in seed0 .. seed0 + budget - 1 under which the n keys of `purpose` (idx 0 .. n-1) of sample `sample` hold two equal
    ones: (seed, i, j) with i < j, or None."""
    idx = np.arange(n, dtype=np.uint64)[None, :]
    for lo in range(0, budget, chunk):
        seeds = np.arange(seed0 + lo, seed0 + min(lo + chunk, budget), dtype=np.uint64)[:, None]
        key = philox4x32(idx, sample, purpose, TAG, seeds & np.uint64(0xFFFFFFFF), seeds >> np.uint64(32), 7)[0]
        srt = np.sort(key, axis=1)
        hit = np.nonzero((srt[:, 1:] == srt[:, :-1]).any(1))[0]
        if len(hit):
            h = hit[0]
            val = srt[h][np.nonzero(srt[h, 1:] == srt[h, :-1])[0][0]]
            i, j = np.nonzero(key[h] == val)[0][:2]
            return int(seeds[h, 0]), int(i), int(j)
    return None


# ---------------------------------------------------------------- pieces and oracle cases shared by the CPU and the GPU tests
def piece(rng, S, L, bars, pad_row, eos_row):
    """(S,8) int64: L random Octuple rows ending in the EOS row, PAD behind. bars: 'walk' (non-decreasing), 'one', 'every' (every row a
    new bar, modulo 256)."""
    hi = np.array([256, 128, 129, 256, 128, 32, 254, 49])
    x = np.tile(np.asarray(pad_row).astype(np.int64), (S, 1))
    if L > 0:
        body = rng.integers(0, hi, size=(L, 8))
        if bars == 'one':
            body[:, 0] = 3
        elif bars == 'every':
            body[:, 0] = np.arange(L) % 256
        else:
            body[:, 0] = np.minimum(np.cumsum(rng.random(L) < 0.2), 255)
        x[:L] = body
        x[L - 1] = eos_row
    return x


def piece_set(rng, S, pad_row, eos_row):
    """The piece shapes of tests/test_corrupt_gpu.py at length S: a walk, one bar, every row a new bar (full and half windows), all PAD."""
    Ls = sorted({S, max(1, S // 2)})
    return [piece(rng, S, L, b, pad_row, eos_row) for L in Ls for b in ('walk', 'one', 'every')] + [piece(rng, S, 0, 'walk', pad_row, eos_row)]


def six_pieces(S, pad_row, eos_row):
    """The batch of the Philox tests at length S: walk, one bar, every row a new bar, a half window, all PAD, and rows without PAD."""
    rng = np.random.default_rng(7000 + S)
    half = max(1, S // 2)
    full = piece(rng, S, S, 'walk', pad_row, eos_row)
    full[-1] = full[0]
    return np.stack([piece(rng, S, S, 'walk', pad_row, eos_row), piece(rng, S, S, 'one', pad_row, eos_row), piece(rng, S, S, 'every', pad_row, eos_row),
                     piece(rng, S, half, 'walk', pad_row, eos_row), piece(rng, S, 0, 'walk', pad_row, eos_row), full])


# The Philox configurations the GPU test runs, (S, p): p = 0.15 at every length on both sides of one, two, four and eight trips of the
# kernel's 256-thread loops (10, 30 and 50 put S * 0.15 on .5), p = 0.5 and 0.9 where infilling needs retries and spans pass the end.
GRID = [(S, 0.15) for S in (1, 2, 3, 10, 30, 50, 255, 256, 257, 511, 513, 1024, 2047, 2048)] + [(S, p) for p in (0.5, 0.9) for S in (3, 64, 257)]
GRID_B = 6
MANY = (300, 64, 0.15)              # one launch of B = 300 samples of S = 64 with mixed choices
# (S, p) -> how many seeds were passed over: because a Poisson draw of theirs is ambiguous (none so far), or, at S = 3, until one of the
# six samples fails its first infilling attempt and the kernel's retry loop has to take the second (a span of length 0 adds a row,
# longer ones remove rows, so at greater lengths an attempt that overflows is too rare to find; the replay tests make those by hand)
SEED_BUMP = {(3, 0.9): 4, (3, 0.5): 5}


def grid_seed(S, p):
    """The seed of configuration (S, p): both halves of the 64 bits in use."""
    return (0x9E3779B9 << 32) + S * 1000 + round(p * 100) + SEED_BUMP.get((S, p), 0)


_ORACLE = {}


def oracle_corruptor(S, p=0.15):
    from oracle import pianobart_oracle as O
    from tests.golden_util import load_vocab
    if 'pb' not in _ORACLE:
        e2w, w2e = load_vocab()
        _ORACLE['pb'] = O.PianoBart(O.BartConfig(max_position_embeddings=64, d_model=32, encoder_layers=1, decoder_layers=1, encoder_ffn_dim=64,
                                                 decoder_ffn_dim=64, encoder_attention_heads=4, decoder_attention_heads=4), e2w, w2e)
    return O.Corruptor(_ORACLE['pb'], S, p)


def oracle_cases(corr, seqs, seed0, choices=(1, 2, 3, 4, 5)):
    """Every sequence under every choice through the oracle's gen_mask, each under its own seed, with the decisions it drew."""
    import random
    import torch
    S = corr.max_seq_len
    cases = []
    for k, x in enumerate(seqs):
        for choice in choices:
            random.seed(seed0 + 7 * k + choice); np.random.seed(seed0 + 7 * k + choice)
            corr.trace = {}
            masked, pos = corr.gen_mask(torch.from_numpy(x).long(), choice)
            tr = corr.trace
            cases.append(dict(ids=x.astype(np.int64), choice=tr['choice'], dec=tr['dec'], rand_rows=tr.get('rand_rows'),
                              masked=np.asarray(masked).astype(np.int64), pos=np.asarray(pos).astype(np.int64).reshape(S, -1)[:, 0]))
    corr.trace = None
    return cases
