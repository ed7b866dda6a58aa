"""Host restatement (numpy) of the dropout stream of csrc/pb_common.h: Philox4x32 and drop_mask4.

The round function is checked against the published Random123 known answers at 10 rounds (tests/test_philox_ref_cpu.py); the kernels
draw 7 rounds of the same function over the counter (idx4, site, 0x5EED, 0) under the key (low, high half of the step's seed), and
element 4 * idx4 + e of a dropout site takes word e of that draw. The GPU tests compare every kernel's mask with drop_mask() bit for bit.
"""
import numpy as np

_M32 = np.uint64(0xFFFFFFFF)
_MUL0, _MUL1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_KEY0, _KEY1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)


def _u(x):
    return np.asarray(x, dtype=np.uint64) & _M32


def philox4x32(c0, c1, c2, c3, k0, k1, rounds):
    """Philox4x32 with `rounds` rounds on uint64 arrays (or scalars) that hold 32-bit words; returns the four output words."""
    c0, c1, c2, c3, k0, k1 = (_u(x) for x in (c0, c1, c2, c3, k0, k1))
    for _ in range(rounds):
        p0, p1 = _MUL0 * c0, _MUL1 * c2                          # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + _KEY0) & _M32, (k1 + _KEY1) & _M32
    return c0, c1, c2, c3


def drop_words(seed, site, idx4):
    """(len(idx4), 4) uint32: the four words of every counter idx4 of dropout site `site` under the 64-bit `seed`."""
    idx4 = np.asarray(idx4, dtype=np.uint64)
    seed = int(seed)
    w = philox4x32(idx4, np.uint64(site), np.uint64(0x5EED), np.uint64(0), np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF), 7)
    return np.stack([np.broadcast_to(x, idx4.shape) for x in w], axis=-1).astype(np.uint32)


def drop_consts(p):
    """(thresh, scale) as the kernels compute them, in float32: drop where word < thresh, keep times scale."""
    p32 = np.float32(p)
    assert 0.0 < float(p32) < 1.0
    thresh = np.uint32(p32 * np.float32(4294967296.0))
    scale = np.float32(1.0) / (np.float32(1.0) - p32)
    return thresh, scale


def drop_mask(seed, site, p, n):
    """float32[n]: 0 where the element is dropped, 1 / (1 - p) where it is kept."""
    thresh, scale = drop_consts(p)
    words = drop_words(seed, site, np.arange((n + 3) // 4, dtype=np.uint64)).reshape(-1)[:n]
    return np.where(words < thresh, np.float32(0.0), scale).astype(np.float32)
