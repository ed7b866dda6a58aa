"""GPU: the kernels that decide which rows exist in the packed step (csrc/pb_rowmap.hip, pb_shift_right) against tests/rowmap_ref.py.

They are integer (or exactly summable) kernels: every comparison is np.array_equal on whole buffers. Every output is a view inside a
larger allocation whose guards, like every element the contract leaves alone (the gaps between batches in `off`, the rows a scatter
does not name), hold a sentinel that must survive.
  * rowmap_count / _build / _build_sub at S = 1, 2, 255, 256, 257, 333, 512, 513, 1024, 2049 (a thread of the 256 owns ceil(S / 256)
    consecutive positions: a partly filled last thread on both sides of 1, 2 and 4 positions per thread, and 9 at S = 2049), B = 4:
    masks all visible, none visible, a prefix, a prefix with a hole, a hole at position 0, a hole only at S - 1 (the prefix flag of each
    asserted), with the values 2.0, -1.0 (visible) and -0.0 (not visible); the loss mask set in each single column 0 .. 7, in no column,
    and NULL; len[b] = 0, the live count, live + 1 and S; build_sub with len 0, exactly the loss rows, and all rows of the packing.
  * gather_rows16 / scatter_rows16 at row_bytes 16, 48, 1536, 4096 with the row count that puts n_rows * row_bytes / 16 just below, at
    and above 524 288 (the 2048 x 256 lanes of the full grid: one sweep short, an exact sweep, a second sweep); at 16 bytes these are
    524 287, 524 288 and 524 352 lanes, at the wider rows the nearest row counts (524 288 is no multiple of 3 or 96 words: no exact sweep
    there). Repeated sources, a strict subset of destinations, n_rows = 0, row_bytes 8 and 24 refused.
  * pos_grad_packed in both dtypes at (S, d) = (1, 4), (333, 64), (1024, 768), (2049, 1024) (the last crosses the sweep), B = 1 and 5,
    `inv` with -1 entries, on integers of magnitude <= 8: every sum is exact in float32 and must equal the float64 one.
  * shift_right at (B, S) = (1, 1), (3, 64), (5, 333), (33, 2048) (the last crosses the sweep) against numpy.roll plus the SOS row.

Scratch builds of the library, one change each, and what fails on them of the 32 tests of this file (test_rowmap_kernels_match_numpy
of tests/test_packed_gpu.py, at S = 333 with its loss mask in column 3, fails on both as well):
  (e) rowmap_build_kernel computes `per = S / 256`: 7 fail, test_rowmap_count_build_and_build_sub at every S that is no multiple of 256;
  (f) row_has_loss ignores column 3: 10 fail, test_rowmap_count_build_and_build_sub at every S.
"""
import numpy as np
import pytest
import torch

from tests import rowmap_ref as R
from tests.golden_util import PAD

pytestmark = pytest.mark.gpu
GUARD = 64
SENTINEL = {torch.int32: -7777777, torch.int16: -31111, torch.float32: 1.5 * 2.0 ** -20}
SWEEP = 2048 * 256


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from pianobart_amd import ops as o
    return o


class Guarded:
    """n elements inside an allocation of GUARD + n + GUARD; everything starts as the dtype's sentinel (or `init` inside)."""

    def __init__(self, n, dtype, init=None):
        self.n, self.buf = n, torch.full((GUARD + n + GUARD,), SENTINEL[dtype], dtype=dtype, device='cuda')
        self.inside = self.buf[GUARD:GUARD + n]
        if init is not None:
            self.inside.copy_(torch.as_tensor(init, dtype=dtype).reshape(-1))
        self.start = self.buf.cpu().numpy().copy()

    def host(self):
        """The inside after a call; the guards are asserted untouched."""
        got = self.buf.cpu().numpy()
        assert np.array_equal(got[:GUARD], self.start[:GUARD]) and np.array_equal(got[GUARD + self.n:], self.start[GUARD + self.n:]), 'a guard was written'
        return got[GUARD:GUARD + self.n]

    def initial(self):
        return self.start[GUARD:GUARD + self.n].copy()


def _dev(x, dtype):
    return torch.tensor(np.asarray(x), dtype=dtype, device='cuda')


# ---------------------------------------------------------------- row maps
def _masks(S, rng):
    """name -> (mask row (S,) float32, prefix flag): 0 where invisible (0.0 and -0.0 alternate), 1.0 / 2.0 / -1.0 where visible."""
    def row(vis):
        vis = np.asarray(vis, dtype=bool)
        m = np.where(np.arange(S) % 2 == 0, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
        m[vis] = np.array([1.0, 2.0, -1.0], dtype=np.float32)[np.arange(S) % 3][vis]
        return m
    s = np.arange(S)
    L = S // 2
    hole = min(L // 2, S - 1)
    out = {'all': (row(s >= 0), 1), 'none': (row(s < 0), 1), 'prefix': (row(s < L), 1),
           'prefix, hole inside': (row((s < L) & (s != hole)), int(L <= 1 or hole == L - 1)),
           'hole at 0': (row(s != 0), int(S == 1)), 'hole only at S - 1': (row(s != S - 1), 1),
           'prefix, hole at 0': (row((s < L) & (s != 0)), int(L <= 1)), 'scattered': (row(rng.random(S) < 0.5), None)}
    return out


def _loss_masks(B, S, rng):
    """name -> (B,S,8) float32 or None: a fifth of the positions, and the last one, carry a loss term in one single column."""
    sel = rng.random((B, S)) < 0.2
    sel[:, -1] = True
    sel[0, 0] = True
    out = {'NULL': None, 'no column': np.zeros((B, S, 8), dtype=np.float32)}
    out['no column'][~sel, :] = -0.0                                       # -0.0 is no loss term
    for c in range(8):
        lm = np.zeros((B, S, 8), dtype=np.float32)
        lm[sel, c] = np.where(rng.random(int(sel.sum())) < 0.5, 1.0, -2.0)
        out['column %d' % c] = lm
    return out


@pytest.mark.parametrize('S', [1, 2, 255, 256, 257, 333, 512, 513, 1024, 2049])
def test_rowmap_count_build_and_build_sub(ops, S):
    B = 4
    rng = np.random.default_rng(S)
    masks = _masks(S, rng)
    names = list(masks)
    losses = _loss_masks(B, S, rng)
    emask = np.stack([masks[n][0] for n in ('scattered', 'all', 'none', 'hole at 0')])
    for group in (names[:4], names[4:]):
        dmask = np.stack([masks[n][0] for n in group])
        flags = [masks[n][1] for n in group]
        t_e, t_d = _dev(emask, torch.float32), _dev(dmask, torch.float32)
        for lname, lm in losses.items():
            t_l = None if lm is None else _dev(lm, torch.float32)
            counts = Guarded(B * 8, torch.int32)
            ops.rowmap_count(t_e, t_d, t_l, counts.inside.view(B, 8))
            want = R.count(emask, dmask, lm)
            got = counts.host().reshape(B, 8)
            assert np.array_equal(got, want), (group, lname)
            assert all(f is None or f == w for f, w in zip(flags, want[:, 3])), (group, lname)   # the reference itself has the stated flags
            live = want[:, 2]
            assert (want[:, 1] <= live).all() and (live <= S).all()
            kinds = [np.zeros(B, dtype=np.int64), live, np.minimum(live + 1, S), np.full(B, S)]
            for turn in range(4):
                length = np.array([kinds[(b + turn) % 4][b] for b in range(B)])
                off = np.concatenate([[2], 2 + np.cumsum(length + 3)[:-1]])                       # gaps of 3 rows between the batches, 2 in front
                total = int(off[-1] + length[-1]) + 1
                src, pos, inv = Guarded(total, torch.int32), Guarded(total, torch.int32), Guarded(B * S, torch.int32)
                ops.rowmap_build(t_d, t_l, _dev(off, torch.int32), _dev(length, torch.int32), src.inside, pos.inside, inv.inside)
                w_src, w_pos, w_inv = R.build(dmask, lm, off, length, src.initial(), pos.initial(), inv.initial())
                g_src, g_pos, g_inv = src.host(), pos.host(), inv.host()
                assert np.array_equal(g_src, w_src) and np.array_equal(g_pos, w_pos) and np.array_equal(g_inv, w_inv), (group, lname, turn)
                for b in range(B):
                    if length[b] == 0:
                        assert (g_inv[b * S:(b + 1) * S] == -1).all()
                assert int((g_src != SENTINEL[torch.int32]).sum()) == int(length.sum())           # the gaps keep the sentinel
                if lm is None:
                    continue
                # the sub-packing of this packing: no row, exactly the loss rows, all rows of the packing
                nloss = np.minimum(want[:, 4], length)
                sub_kinds = [np.zeros(B, dtype=np.int64), nloss, length]
                len_s = np.array([sub_kinds[(b + turn) % 3][b] for b in range(B)])
                off_s = np.concatenate([[1], 1 + np.cumsum(len_s + 2)[:-1]])
                total_s = int(off_s[-1] + len_s[-1]) + 1
                s_src, s_idx = Guarded(total_s, torch.int32), Guarded(total_s, torch.int32)
                ops.rowmap_build_sub(t_l, inv.inside, _dev(off_s, torch.int32), _dev(len_s, torch.int32), s_src.inside, s_idx.inside)
                w_ssrc, w_sidx = R.build_sub(lm, w_inv, off_s, len_s, s_src.initial(), s_idx.initial())
                assert np.array_equal(s_src.host(), w_ssrc) and np.array_equal(s_idx.host(), w_sidx), (group, lname, turn, 'sub')
                assert np.array_equal(inv.host(), w_inv)                                          # `present` is read only


# ---------------------------------------------------------------- gather / scatter
def _row_counts(q):
    """Row counts of q 16-byte words whose lane count n * q is the largest below a full sweep, a full sweep (where q divides it), and the
    smallest that reaches 64 lanes into the second sweep."""
    return [(SWEEP - 1) // q] + ([SWEEP // q] if SWEEP % q == 0 else []) + [-(-(SWEEP + 64) // q)]


def test_row_counts_sit_on_the_sweep_edges():
    assert _row_counts(1) == [SWEEP - 1, SWEEP, SWEEP + 64] and _row_counts(256) == [2047, 2048, 2049]
    assert _row_counts(3) == [174762, 174784] and _row_counts(96) == [5461, 5462]
    assert 174762 * 3 == SWEEP - 2 and 174784 * 3 == SWEEP + 64 and 5461 * 96 == SWEEP - 32 and 5462 * 96 == SWEEP + 64


@pytest.mark.parametrize('row_bytes', [16, 48, 1536, 4096])
def test_gather_and_scatter_rows16_across_the_grid_sweep(ops, row_bytes):
    q, w = row_bytes // 16, row_bytes // 4
    rng = np.random.default_rng(row_bytes)
    for n in _row_counts(q):
        # gather: repeated sources out of a table of about half as many rows
        n_src = n // 2 + 3
        table = rng.integers(-2 ** 31, 2 ** 31, size=(n_src, w), dtype=np.int64).astype(np.int32)
        row_src = rng.integers(0, n_src, size=n).astype(np.int32)
        row_src[-1], row_src[0] = n_src - 1, 0
        t_table, t_rows = _dev(table, torch.int32), _dev(row_src, torch.int32)
        dst = Guarded(n * w, torch.int32)
        ops.gather_rows16(t_table, t_rows, dst.inside, n, row_bytes)
        assert np.array_equal(dst.host().reshape(n, w), table[row_src]), ('gather', n)
        assert torch.equal(t_table, _dev(table, torch.int32)) and torch.equal(t_rows, _dev(row_src, torch.int32))
        # scatter: a strict subset of the destination rows, each named once; the others keep the sentinel
        n_dst = n + 65
        row_dst = rng.permutation(n_dst)[:n].astype(np.int32)
        data = rng.integers(-2 ** 31, 2 ** 31, size=(n, w), dtype=np.int64).astype(np.int32)
        big = Guarded(n_dst * w, torch.int32)
        ops.scatter_rows16(_dev(data, torch.int32), _dev(row_dst, torch.int32), big.inside, n, row_bytes)
        want = big.initial().reshape(n_dst, w)
        want[row_dst] = data
        assert np.array_equal(big.host().reshape(n_dst, w), want), ('scatter', n)
        del dst, big, t_table
    # n_rows = 0 writes nothing
    table = _dev(rng.integers(0, 100, size=(4, w)), torch.int32)
    rows = _dev([3, 1], torch.int32)
    dst = Guarded(2 * w, torch.int32)
    ops.gather_rows16(table, rows, dst.inside, 0, row_bytes)
    ops.scatter_rows16(table, rows, dst.inside, 0, row_bytes)
    assert np.array_equal(dst.host(), dst.initial())


@pytest.mark.parametrize('row_bytes', [8, 24, 0, -16])
def test_gather_and_scatter_refuse_rows_that_are_no_multiple_of_16_bytes(ops, row_bytes):
    from pianobart_amd._lib import PBError
    table = _dev(np.arange(64), torch.int32)
    rows = _dev([1, 0], torch.int32)
    dst = Guarded(64, torch.int32)
    with pytest.raises(PBError):
        ops.gather_rows16(table, rows, dst.inside, 2, row_bytes)
    with pytest.raises(PBError):
        ops.scatter_rows16(table, rows, dst.inside, 2, row_bytes)
    assert np.array_equal(dst.host(), dst.initial())


# ---------------------------------------------------------------- position-table gradient
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('S,d', [(1, 4), (333, 64), (1024, 768), (2049, 1024)])
def test_pos_grad_packed_sums_exactly(ops, S, d, dtype):
    rng = np.random.default_rng(S + d)
    for B in (1, 5):
        T = min(B * S, 2048)                                               # packed rows; several positions may name one
        x = rng.integers(-8, 9, size=(T, d)).astype(np.float32)            # integers: exact in bf16, and every sum exact in float32
        inv = rng.integers(0, T, size=(B, S)).astype(np.int32)
        inv[rng.random((B, S)) < 0.3] = -1
        inv[0, 0], inv[B - 1, S - 1] = -1, T - 1
        if S > 1:
            inv[:, 1] = -1                                                 # a position no batch row kept: `out` stays as it is
        start = rng.integers(-4, 5, size=(S, d)).astype(np.float32)
        out = Guarded(S * d, torch.float32, init=start)
        t_x, t_inv = _dev(x, torch.float32).to(dtype), _dev(inv, torch.int32)
        ops.pos_grad_packed(t_x, t_inv, out.inside.view(S, d), B, S)
        want = R.pos_grad(x, inv, start, B, S)
        assert np.abs(want).max() <= 8 * B + 4
        assert np.array_equal(out.host().reshape(S, d).astype(np.float64), want), B
        assert np.array_equal(t_inv.cpu().numpy(), inv) and np.array_equal(t_x.float().cpu().numpy(), x)


def test_pos_grad_packed_refuses_a_width_that_is_no_multiple_of_4(ops):
    from pianobart_amd._lib import PBError
    out = Guarded(3 * 6, torch.float32)
    with pytest.raises(PBError):
        ops.pos_grad_packed(torch.zeros(3, 6, device='cuda'), _dev(np.zeros((1, 3)), torch.int32), out.inside.view(3, 6), 1, 3)
    assert np.array_equal(out.host(), out.initial())


# ---------------------------------------------------------------- shift right
@pytest.mark.parametrize('B,S', [(1, 1), (3, 64), (5, 333), (33, 2048)])
def test_shift_right_is_a_roll_behind_the_sos_row(ops, B, S):
    rng = np.random.default_rng(B * S)
    ids = rng.integers(0, [262, 134, 135, 262, 134, 38, 260, 55], size=(B, S, 8)).astype(np.int16)
    sos = (PAD + 2).astype(np.int16)
    t_ids, t_sos = _dev(ids, torch.int16), _dev(sos, torch.int16)
    out = Guarded(B * S * 8, torch.int16)
    ops.shift_right(t_ids, t_sos, out.inside.view(B, S, 8), B, S)
    assert np.array_equal(out.host().reshape(B, S, 8), R.shift_right(ids, sos))
    assert np.array_equal(t_ids.cpu().numpy(), ids) and np.array_equal(t_sos.cpu().numpy(), sos)
