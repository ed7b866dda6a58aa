"""CPU: tests/philox_ref.py, the host reference of the dropout stream, against the published Random123 known answers of Philox4x32-10
(the kernels run the same round function 7 times), and the constants the mask is cut with."""
import numpy as np
import pytest

from tests.philox_ref import drop_consts, drop_mask, drop_words, philox4x32

F = 0xFFFFFFFF
KAT = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
       ((F, F, F, F), (F, F), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]


@pytest.mark.parametrize('ctr,key,want', KAT)
def test_philox4x32_10_known_answers(ctr, key, want):
    got = philox4x32(*ctr, *key, rounds=10)
    assert tuple(int(x) for x in got) == want


def test_philox_is_elementwise_over_arrays():
    """A vector of counters gives what the counters give one at a time (the masks are built from one vectorised call)."""
    ctr = np.array([[c[i] for c, _, _ in KAT] for i in range(4)], dtype=np.uint64)
    key = np.array([[k[i] for _, k, _ in KAT] for i in range(2)], dtype=np.uint64)
    got = philox4x32(*ctr, *key, rounds=10)
    for j, (_, _, want) in enumerate(KAT):
        assert tuple(int(x[j]) for x in got) == want
    seven = philox4x32(*ctr, *key, rounds=7)
    assert all(tuple(int(x[j]) for x in seven) != KAT[j][2] for j in range(3))     # the round count matters


def test_drop_constants_are_the_float32_ones():
    thresh, scale = drop_consts(0.1)
    assert int(thresh) == 429496736 and float(scale) == 1.1111111640930176
    thresh, scale = drop_consts(0.5)
    assert int(thresh) == 1 << 31 and float(scale) == 2.0


def test_drop_mask_layout_and_key():
    seed, site = 0x12345679ABCDEF1, 5
    w = drop_words(seed, site, np.arange(3))
    assert w.shape == (3, 4) and w.dtype == np.uint32
    one = philox4x32(2, site, 0x5EED, 0, seed & F, seed >> 32, rounds=7)           # counter (idx4, site, 0x5EED, 0), key (low, high)
    assert [int(x) for x in one] == [int(x) for x in w[2]]
    thresh, scale = drop_consts(0.1)
    m = drop_mask(seed, site, 0.1, 11)                                             # element 4 i + e <- word e of counter i; ragged tail
    assert m.dtype == np.float32 and m.shape == (11,)
    assert np.array_equal(m, np.where(w.reshape(-1)[:11] < thresh, np.float32(0), scale))
    assert set(np.unique(drop_mask(seed, site, 0.1, 4096))) == {np.float32(0), scale}
    assert not np.array_equal(drop_words(seed, site + 1, np.arange(3)), w)         # the site and both halves of the seed enter
    assert not np.array_equal(drop_words(seed ^ (1 << 40), site, np.arange(3)), w)
    assert not np.array_equal(drop_words(seed ^ 1, site, np.arange(3)), w)
    frac = float((drop_mask(seed, site, 0.1, 1 << 18) == 0).mean())
    assert abs(frac - 0.1) < 5 * (0.1 * 0.9 / (1 << 18)) ** 0.5                    # five standard deviations of a Bernoulli(0.1) mean
