"""Dictionaries for the vocabulary-layout tests and tools, written from the dictionary FORMAT (the reference's class names and key order,
words '<class> <value>', the six specials '<class> <PAD|MASK|SOS|EOS|CLS|SEP>' as the last six ids), and synthetic batches for them. Imports
numpy and torch only, so a measuring tool can use it too.
  D_SMALL  total 249 (odd), table slot 72, every head narrow
  D_WIDE   total 2470; head 0 wide with p = 1 (and the head of the stop / order rules), head 3 wide with p = 0.9 (the ranked nucleus), head 4 =
           300: over the sampler's narrow rows (272), under the score kernel's register form (320)
  D_RANKED the default dictionary with `pos_resolution` doubled (Duration 134 -> 262): every head <= 272, but the heads with p < 1 (3, 4, 7) hold
           262 + 262 + 55 = 579 classes, more than the narrow sampler's 512 rank threads"""
import numpy as np
import torch

CLASSES = ['Bar', 'Position', 'Instrument', 'Pitch', 'Duration', 'Velocity', 'TimeSig', 'Tempo']          # PianoBart.classes: the model's column order
DICT_KEYS = ['Bar', 'Position', 'Pitch', 'Duration', 'Velocity', 'Instrument', 'Tempo', 'TimeSig']       # the key order of a reference dictionary
SPECIALS = ['PAD', 'MASK', 'SOS', 'EOS', 'CLS', 'SEP']
D_DEFAULT = [262, 134, 135, 262, 134, 38, 260, 55]
D_SMALL = [70, 38, 23, 45, 22, 14, 17, 20]
D_WIDE = [1030, 134, 135, 518, 300, 38, 260, 55]
D_RANKED = [262, 134, 135, 262, 262, 38, 260, 55]


def make_dict(sizes):
    """(e2w, w2e) of a dictionary with the given head sizes (CLASSES order): per class the ordinary words '<class> 0' .. and then the six
    specials, ids in that order; keys in the reference's dictionary order."""
    by_class = dict(zip(CLASSES, sizes))
    e2w, w2e = {}, {}
    for name in DICT_KEYS:
        n = by_class[name]
        words = ['%s %d' % (name, v) for v in range(n - 6)] + ['%s <%s>' % (name, tag) for tag in SPECIALS]
        e2w[name] = {w: i for i, w in enumerate(words)}
        w2e[name] = {i: w for i, w in enumerate(words)}
    return e2w, w2e


def synth_batch(sizes, B, S, seed, min_len=None):
    """tests.golden_util.synth_octuple_batch for a dictionary of the given sizes: (enc, dec, loss_mask, emask, dmask, target) with ragged
    lengths, an EOS row, a PAD tail, a TokenMask-style corruption and a Bernoulli(0.15) loss mask. Ordinary ids cover each head's whole
    ordinary range, its last class included."""
    rng = np.random.default_rng(seed)
    n = np.asarray(sizes)
    pad = n - 6
    tgt = np.zeros((B, S, 8), dtype=np.int64)
    for b in range(B):
        L = int(rng.integers(min_len if min_len is not None else S // 2, S + 1)) if b else S        # row 0 fills the window, the others are ragged
        L = max(2, min(L, S))
        rows = np.stack([rng.integers(0, pad[c], size=L - 1) for c in range(8)], axis=1)
        rows[:, 0] = np.sort(rows[:, 0])
        rows[0] = 0
        if L > 2:
            rows[L - 2] = pad - 1                                  # the last ordinary class of every head
        tgt[b, :L - 1] = rows
        tgt[b, L - 1] = pad + 3                                    # EOS row
        tgt[b, L:] = pad
    sel = rng.random((B, S)) < 0.15
    sel[:, 0] |= ~sel.any(axis=1)
    kind = rng.random((B, S))
    enc = tgt.copy()
    for b in range(B):
        for s in np.nonzero(sel[b])[0]:
            if kind[b, s] < 0.8:
                enc[b, s] = pad + 1                                # MASK row
            elif kind[b, s] < 0.9:
                enc[b, s] = [rng.integers(0, n[c]) for c in range(8)]
    dec = np.zeros_like(tgt)
    dec[:, 1:] = tgt[:, :-1]
    dec[:, 0] = pad + 2                                            # SOS row
    loss_mask = np.repeat(sel[:, :, None], 8, axis=2).astype(np.float32)
    t = torch.from_numpy
    return t(enc), t(dec), t(loss_mask), t((enc[:, :, 0] != pad[0]).astype(np.float32)), t((dec[:, :, 0] != pad[0]).astype(np.float32)), t(tgt)
