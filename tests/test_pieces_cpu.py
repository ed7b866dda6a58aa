"""CPU: the shared host front end of the evaluation families (pianobart_amd.pieces) against the four independent restatements.

  * pieces.live_rows: on seeded motif pieces (full windows) and synthetic pieces (ragged, an EOS row and a PAD tail) the number of live
    rows equals column 0 of metrics_ref, structure_ref and harmony_ref, and novelty_ref's key count is that number less one (0 for a
    piece of one note or none). start: None, one number, one per piece, == L, > L. The mask is exactly the rows start .. L - 1;
  * metrics.piece_lengths, structure.bar_spans and harmony.kept_pieces, which are built on it, against the same restatements;
  * the one JSON sanitiser of the eval_* tools on a nested value with nan, inf, a tuple and an int64 array."""
import json

import numpy as np
import pytest

from pianobart_amd import eval_metrics, harmony, metrics, pieces, structure
from tests import harmony_ref as HR
from tests import metrics_ref as MR
from tests import novelty_ref as NR
from tests import structure_ref as SR
from tests.vocab_layout_util import D_DEFAULT

PAD8, PITCH_OF, DUR_POS = MR.tables_for(D_DEFAULT, 128)
S = 40
PIECES = np.concatenate([SR.motif_pieces(D_DEFAULT, 4, S, seed=7, mb=(1, 2, 3)), MR.synth_pieces(D_DEFAULT, 8, S, seed=8)])
PIECES[5, 0] = np.asarray(PAD8) + 3                                      # L = 0
PIECES[6, 1, 6] = PAD8[6]                                                # L = 1, the special id in one head only
LENGTHS = np.array([MR.length(p, PAD8) for p in PIECES])
N = len(PIECES)
STARTS = {'none': None, 'scalar': 5, 'per_piece': np.arange(N) * 3, 'at_L': LENGTHS, 'beyond_L': LENGTHS + 2}


def test_the_seeded_pieces_cover_the_cases():
    assert LENGTHS[0] == S and LENGTHS[5] == 0 and LENGTHS[6] == 1 and len(set(LENGTHS)) >= 6


@pytest.mark.parametrize('case', list(STARTS))
def test_live_rows_agree_with_the_four_restatements(case):
    start = STARTS[case]
    L, live = pieces.live_rows(PIECES, start=start)
    n = live.sum(1)
    first = np.zeros(N, dtype=np.int64) if start is None else np.broadcast_to(start, (N,))
    rows = np.arange(S)
    assert np.array_equal(L, LENGTHS) and live.shape == (N, S) and live.dtype == bool
    assert np.array_equal(live, (rows >= first[:, None]) & (rows < LENGTHS[:, None]))
    assert np.array_equal(n, MR.features(PIECES, PAD8, PITCH_OF, DUR_POS, start)[:, 0])
    assert np.array_equal(n, SR.structure(PIECES, PAD8, PITCH_OF, start)[:, 0])
    c = HR.harmony(PIECES, PAD8, PITCH_OF, start)
    assert np.array_equal(n, c[:, 0])
    assert np.array_equal(np.maximum(n - 1, 0), NR.keys_ref(PIECES, PAD8, PITCH_OF, start=start)[1])
    if case in ('at_L', 'beyond_L'):
        assert not live.any()
    # what the families build on it
    assert np.array_equal(metrics.piece_lengths(PIECES, start=start), n)
    assert np.array_equal(structure.bar_spans(PIECES, start=start), c[:, 1])
    assert np.array_equal(harmony.kept_pieces(PIECES, start=start), (c[:, 1] >= 2) & (c[:, 2] >= 1))


def test_the_names_that_moved_stay_reachable():
    assert metrics.tables is pieces.tables and metrics.Tables is pieces.Tables and structure.bar_spans is pieces.bar_spans
    tab = pieces.tables()
    assert pieces.tables(tab) is tab and (tab.pitch_of == PITCH_OF).all() and (tab.dur_pos == DUR_POS).all()


def test_json_sanitiser():
    v = {'a': [float('nan'), (float('inf'), 1.5, -float('inf'))], 'b': np.array([[1, 2], [3, 4]], dtype=np.int64),
         'c': {'d': np.array([float('nan'), 2.0]), 'e': (), 'f': 'x', 'g': 7, 'h': None}}
    want = {'a': [None, [None, 1.5, None]], 'b': [[1, 2], [3, 4]], 'c': {'d': [None, 2.0], 'e': [], 'f': 'x', 'g': 7, 'h': None}}
    got = eval_metrics.json_safe(v)
    assert got == want and list(got) == ['a', 'b', 'c'] and json.loads(json.dumps(got, allow_nan=False)) == want
