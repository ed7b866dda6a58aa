"""GPU: the four kernels that read pieces agree on a piece's extent (csrc/pb_pieces.h), and with the host (pieces.live_rows).

For one input, called through ops: piece_features[:, 0] == piece_structure[:, 0] == piece_harmony[:, 0] == the host's count of live rows,
and piece_keys' klen is that count less one (0 for one note or none). Exact integers.

  * shapes: 24 pieces of S = 1, 64, 257 and 1 025 rows: at 257 and 1 025 a stop row lies beyond one stride of the 256-thread (features,
    keys, narrow harmony: S <= 512) and 1 024-thread (structure, wide harmony) searches, and both harmony kernels run;
  * pieces: the special id in each of the eight heads in turn, at row 0, at row S - 1, absent, two special rows (the first one counts), an
    id of 65 535 (the int16 -1: the kernels read ids as unsigned, so it ends the piece), stop rows at 255, 256, 1 023 and 1 024 where S has
    them; the rows behind a stop row hold ordinary ids, not PAD: only the first special row may end the piece;
  * start: None, and one vector that holds 0, a row inside the piece, L - 1, L, L + 1 and S + 3."""
import numpy as np
import pytest
import torch

from tests import metrics_ref as MR
from tests.vocab_layout_util import D_DEFAULT

pytestmark = pytest.mark.gpu

N = 24
PAD8, PITCH_OF, DUR_POS = MR.tables_for(D_DEFAULT, 128)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


def _pieces(S):
    """(ids (N, S, 8) int64 with ordinary ids but for the stop rows, stop (N): each piece's first special row, S if none)."""
    rng = np.random.default_rng(S)
    ids = np.stack([rng.integers(0, PAD8[h], size=(N, S)) for h in range(8)], axis=2)
    ids[:, :, 0] = np.sort(rng.integers(0, 12, size=(N, S)), axis=1)       # bars in time order
    stop = np.full(N, S)

    def put(i, r, h, v):
        ids[i, r, h] = v
        stop[i] = min(stop[i], r)

    for h in range(8):                                                      # every head in turn, spread over the window
        put(h, (h * S) // 9, h, PAD8[h] + h % 6)
    put(8, 0, 0, PAD8[0])
    put(9, S - 1, 7, PAD8[7] + 5)
    # piece 10: no special id
    put(11, S // 2, 3, 65535)
    put(12, S - 1, 0, 65535)
    put(13, (2 * S) // 3, 1, PAD8[1])
    put(13, S // 3, 5, PAD8[5] + 3)
    for i, r in ((14, 255), (15, 256), (16, 1023), (17, 1024)):
        put(i, min(r, S - 1), i % 8, PAD8[i % 8] + 1)
    for i in range(18, N):
        r = int(rng.integers(0, S + 1))
        if r < S:
            put(i, r, int(rng.integers(0, 8)), 65535 if i % 2 else PAD8[0] + 2)
    return ids, stop


@pytest.mark.parametrize('with_start', [False, True], ids=['no_start', 'start'])
@pytest.mark.parametrize('S', [1, 64, 257, 1025])
def test_the_four_kernels_and_the_host_agree_on_a_pieces_extent(S, with_start):
    _need_gpu()
    from pianobart_amd import ops, pieces
    ids, stop = _pieces(S)
    start = None
    if with_start:
        start = np.array([(0, stop[i] // 2, max(stop[i] - 1, 0), stop[i], stop[i] + 1, S + 3)[i % 6] for i in range(N)], dtype=np.int32)
    L, live = pieces.live_rows(ids, start=start)
    n = live.sum(1)
    assert np.array_equal(L, stop) and np.array_equal(n, np.maximum(stop - (0 if start is None else start), 0))
    assert (n == 0).any() and (start is not None or (n == S).any())
    dev = lambda a: torch.from_numpy(a).cuda()
    ids16, pitch_of, d_start = dev(ids.astype(np.int16)), dev(PITCH_OF), None if start is None else dev(start)
    assert int((ids16 == -1).sum()) >= 2
    got = {'features': ops.piece_features(ids16, pitch_of, dev(DUR_POS), start=d_start)[:, 0],
           'structure': ops.piece_structure(ids16, pitch_of, start=d_start)[:, 0],
           'harmony': ops.piece_harmony(ids16, pitch_of, start=d_start)[:, 0]}
    klen = ops.piece_keys(ids16, pitch_of, start=d_start)[1]
    for name, col in got.items():
        assert np.array_equal(col.cpu().numpy().astype(np.int64), n), name
    assert np.array_equal(klen.cpu().numpy().astype(np.int64), np.maximum(n - 1, 0))
