"""CPU: the restatement of tests/texture_ref.py on pieces worked out by hand, the identities its columns obey, the bar lengths of
pieces.tables(), the time axis against octuple_midi.encoding_to_midi, texture_groups on hand-made columns and the refusals of
pianobart_amd.texture and eval_texture that need no GPU."""
import json

import numpy as np
import pytest

from tests import metrics_ref as M
from tests import texture_ref as R
from tests.vocab_layout_util import D_DEFAULT, D_SMALL, D_WIDE, SPECIALS, make_dict

PAD = np.asarray(D_DEFAULT) - 6
PAD8, PITCH_OF, DUR_POS = M.tables_for(D_DEFAULT, 128)
BAR_POS = R.bar_pos_default()

# (bar, position, pitch id, duration id, time-signature id); duration ids 0, 4, 5, 16, 17 are 0 (counted as 1), 4, 5, 16, 18 positions
HAND = [(2, 0, 60, 16, 9),        # a: t 0, e 16
        (2, 16, 60, 17, 9),       # b: t 16, e 34: touches a, no collision
        (2, 20, 60, 4, 9),        # c: t 20, e 24: struck inside b, a collision
        (2, 16, 64, 16, 9),       # d: t 16, e 32: a chord with b
        (2, 16, 64, 16, 9),       # e: d once more, a duplicate
        (3, 8, 130, 5, 8),        # f: percussion; bar 3 is 3/4 (48 positions), B = 64
        (3, 40, 67, 16, 8),       # g: t 104, e 120 > 64 + 48: tied
        (5, 50, 72, 0, 8)]        # h: bar 4 is empty and takes 3/4: B(bar 5) = 160; position 50 >= 48: off-bar; t 210, e 211 > 208: tied
HAND_ROW = ([8, 7, 4, 211, 51, 16, 67, 2, 87, 1, 1, 5, 2, 1, 6, 0] + [160, 35, 16] + [0] * 14 + [4, 1] + [0] * 7
            + [0, 0, 1, 0, 1, 0, 2] + [0] * 9 + [0] * 6)


def _one(notes, S=16, start=0, L=None):
    return R.texture_one(R.from_notes(notes, S, PAD, L), PAD8, PITCH_OF, DUR_POS, BAR_POS, start)


def test_the_hand_computed_piece():
    assert [int(DUR_POS[i]) for i in (0, 4, 5, 16, 17, 127)] == [0, 4, 5, 16, 18, 3952]
    assert [int(BAR_POS[i]) for i in (R.TS_44, R.TS_34, R.TS_21, R.TS_164, R.TS_68)] == [64, 48, 128, 1, 48]
    assert len(HAND_ROW) == 64 and _one(HAND) == HAND_ROW
    rng = np.random.default_rng(1)
    for _ in range(3):
        assert _one([HAND[i] for i in rng.permutation(len(HAND))]) == HAND_ROW             # the row order does not matter


def test_small_pieces_by_hand():
    one = [1, 1, 1, 1, 1, 0, 1, 1, 1, 0, 0, 1, 0, 0, 1, 0] + [0, 1] + [0] * 15 + [1] + [0] * 8 + [0] * 16 + [0] * 6
    assert _one([(0, 0, 60, 0, 9)]) == one
    assert _one([(7, 3, 130, 9, 9), (9, 0, 131, 9, 9)]) == [2, 0, 3] + [0] * 61               # percussion only: notes, P = 0, W, then zeros
    assert _one([]) == [0] * 64 and _one(HAND, L=0) == [0] * 64
    assert _one(HAND, start=5)[:3] == [3, 2, 3] and _one(HAND, start=8)[:3] == [0, 0, 0]
    # two time signatures in bar 0, both at position 0: the smaller id (3/4) sets the length; a later row's smaller id does not
    r = _one([(0, 0, 60, 16, 9), (0, 0, 62, 16, 8), (0, 5, 64, 16, 1), (1, 0, 65, 16, 9)])
    assert r[3] == 48 + 16 and r[11] == 3 and r[42 + 2] == 1 and r[42 + 5] == 1               # onsets 0, 5, 48: gaps 5 and 43
    # an overlap of one step, and notes nested in a long one of the same pitch
    r = _one([(0, 0, 60, 17, 9), (0, 17, 60, 16, 9)])                                         # [0, 18) and [17, 33)
    assert (r[9], r[10], r[6], r[8], r[3], r[16]) == (1, 0, 33, 34, 33, 0)
    r = _one([(0, 0, 60, 36, 9), (0, 4, 60, 2, 9), (0, 9, 60, 2, 9), (0, 9, 60, 3, 9)])       # [0, 64), [4, 6), [9, 11), [9, 12)
    assert (r[9], r[10], r[14], r[6], r[8], r[7]) == (2, 1, 3, 64, 64 + 2 + 2 + 3, 1)
    # touching notes of one pitch: no collision, no silence
    r = _one([(0, 0, 60, 16, 9), (0, 16, 60, 16, 9), (0, 32, 60, 16, 9)])
    assert (r[9], r[16], r[17], r[3]) == (0, 0, 48, 48)
    # every note on one (pitch, onset)
    r = _one([(1, 8, 60, 3 + i % 3, 9) for i in range(9)])
    assert (r[10], r[14], r[7], r[11], r[3], r[33]) == (8, 1, 1, 1, 5, 1)


def _random_rows(n, seed):
    return R.from_notes(R.piano_notes(n, seed), n + 1, PAD)


def test_identities():
    ids = np.stack([np.concatenate([_random_rows(n, 10 + n), np.tile(PAD, (400 - n, 1))]) for n in (1, 2, 17, 150, 399)])
    c = R.texture(ids, PAD8, PITCH_OF, DUR_POS, BAR_POS)
    assert (c[:, 0] == [1, 2, 17, 150, 399]).all() and c[:, 1].tolist() == [0, 2, 16, 139, 367]          # the first piece is one percussion row
    assert (c[:, 16:33].sum(1) == c[:, 3]).all() and (c[:, 33:42].sum(1) == c[:, 11]).all()
    assert (c[:, 42:58].sum(1) == np.maximum(c[:, 11] - 1, 0)).all()
    assert (c[:, 6] <= c[:, 8]).all() and (c[:, 14] == c[:, 1] - c[:, 10]).all()
    assert (c[:, 7] <= 15).all() and (c[:, 6] == (c[:, 16:33] * np.arange(17)).sum(1)).all()
    assert (c[:, 4] == c[:, 3] - c[:, 16]).all() and (c[:, 5] == c[:, 4] - c[:, 17]).all()
    assert (c[:, 9] <= c[:, 14]).all() and (c[:, 11] <= c[:, 14]).all() and (c[:, [15] + list(range(58, 64))] == 0).all()
    assert c[4, 9] > 0 and c[4, 10] > 0 and c[4, 12] > 0 and c[4, 13] > 0 and c[4, 5] > 0 and c[4, 16] > 0      # the pieces exercise them


def test_tables_carry_the_bar_lengths():
    from pianobart_amd import octuple_midi, pieces, texture
    tab = pieces.tables()
    assert pieces.Tables._fields[-1] == 'bar_pos' and tab.bar_pos.dtype == np.int32 and len(tab.bar_pos) == tab.layout.pad8[6] == 254
    assert tab.bar_pos.tolist() == [octuple_midi.bar_length(i) for i in range(254)] == R.bar_pos_default().tolist()
    e2w = json.load(open(pieces.VOCAB))['e2w']
    assert [w for w, _ in sorted(e2w['TimeSig'].items(), key=lambda kv: kv[1])][:254] == R.ts_words()
    for sizes in (D_SMALL, D_WIDE):
        plain = pieces.tables(make_dict(sizes)[0])                                           # 'TimeSig 7': no bar length, and no error here
        assert plain.bar_pos.tolist() == [0] * (sizes[6] - 6) and len(plain.pitch_of) == sizes[3] - 6
        with pytest.raises(texture.PBError, match='time-signature id 0 '):
            texture.piece_texture(np.zeros((1, 4, 8), dtype=np.int64), plain)
    e2w, _ = make_dict(D_SMALL)
    words = ['TimeSig 4/4', 'TimeSig 3/4', 'TimeSig 33/1', 'TimeSig 0/4', 'TimeSig 1/128', 'TimeSig 4/0', 'TimeSig 16/1', 'TimeSig x']
    e2w['TimeSig'] = {w: i for i, w in enumerate(words + ['TimeSig %d/4' % i for i in range(8, 11)] + ['TimeSig <%s>' % s for s in SPECIALS])}
    tab = pieces.tables(e2w)
    assert tab.bar_pos.tolist() == [64, 48, 0, 0, 0, 0, 1024, 0, 128, 144, 160]
    with pytest.raises(texture.PBError, match='time-signature id 2 '):
        texture.compare_texture(np.zeros((2, 4, 8), dtype=np.int64), np.zeros((2, 4, 8), dtype=np.int64), tab)


def test_onsets_are_those_of_the_midi_writer():
    from pianobart_amd import octuple_midi
    rng = np.random.default_rng(5)
    bar_ts = [R.TS_44] * 3 + [R.TS_34] * 2 + [R.TS_68, R.TS_21, R.TS_164, R.TS_44]            # one time signature per bar, changes in the middle
    rows = []
    for bar, ts in enumerate(bar_ts):
        if bar == 4:
            continue                                                                         # an empty bar takes the one before
        for _ in range(4):
            rows.append((bar, int(rng.integers(0, BAR_POS[ts])), 0, int(rng.integers(30, 90)), int(rng.integers(0, 60)), 20, ts, 30))
    song = octuple_midi.encoding_to_midi(rows)
    piece = np.asarray(rows + [tuple(PAD + 3)], dtype=np.int64)
    got = R.onsets(piece, PAD8, PITCH_OF, DUR_POS, BAR_POS)
    assert len(got) == len(song.notes) == 32
    assert [t * 480 // 16 for t, _ in got] == [n[0] for n in song.notes]
    assert max(t for t, _ in got) >= 3 * 64 + 2 * 48 + 48 + 128 + 1


def test_texture_groups_on_hand_made_columns():
    from pianobart_amd import texture
    cols = np.zeros((4, 64), dtype=np.int64)
    cols[0] = HAND_ROW
    cols[1, :3] = [5, 0, 2]                                                                  # P = 0: left out
    cols[2, :15] = [1, 1, 1, 1, 1, 0, 1, 1, 1, 0, 0, 1, 0, 0, 1]                             # one note: O - 1 = 0
    cols[2, 17], cols[2, 33] = 1, 1
    cols[3, :3] = [3, 3, 1]                                                                  # every divisor 0
    g, unpitched = texture.texture_groups(cols)
    assert unpitched == 1 and list(g) == list(texture.GROUPS) == list(R.GROUPS) and all(v.dtype == np.float32 for v in g.values())
    want = {'silence_ratio': 160 / 211, 'polyphony_mean': 67 / 51, 'polyphonic_rate': 16 / 51, 'max_polyphony': 2.0, 'overlap_ratio': 20 / 87,
            'collision_rate': 1 / 6, 'duplicate_rate': 1 / 7, 'tie_rate': 2 / 7, 'offbar_rate': 1 / 7, 'chord_size_mean': 6 / 5}
    for k, v in want.items():
        assert g[k].shape == (3,) and g[k][0] == np.float32(v), k
        assert g[k][1] == (1.0 if k in ('polyphony_mean', 'max_polyphony', 'chord_size_mean') else 0.0) and g[k][2] == 0.0, k
    assert g['polyphony_hist'].shape == (3, 17) and g['chord_hist'].shape == (3, 9) and g['ioi_hist'].shape == (3, 16)
    assert g['polyphony_hist'][0, :3].tolist() == [np.float32(160 / 211), np.float32(35 / 211), np.float32(16 / 211)]
    assert g['chord_hist'][0, :2].tolist() == [np.float32(0.8), np.float32(0.2)] and g['ioi_hist'][0, 6] == 0.5
    assert g['ioi_hist'][1].sum() == 0 and g['chord_hist'][1, 0] == 1 and not g['polyphony_hist'][2].any()
    ref, ref_unpitched = R.groups(cols)
    assert ref_unpitched == 1 and all(np.array_equal(g[k], ref[k]) for k in g)
    p = texture.pooled_profiles(cols)
    assert p['polyphony'][:3] == [160 / 212, 36 / 212, 16 / 212] and p['chord'][:2] == [5 / 6, 1 / 6] and p == R.pooled(cols)
    assert all(np.isnan(v) for v in texture.pooled_profiles(cols[1:2])['chord'])
    with pytest.raises(texture.PBError, match='64'):
        texture.texture_groups(np.zeros((2, 63), dtype=np.int64))
    ids = np.stack([R.from_notes(HAND, 12, PAD), R.from_notes([(0, 0, 130, 1, 9)], 12, PAD), R.from_notes(HAND, 12, PAD, L=0)])
    assert texture.kept_pieces(ids).tolist() == [True, False, False] and texture.kept_pieces(ids, start=7).tolist() == [True, False, False]
    assert texture.kept_pieces(ids, start=8).tolist() == [False, False, False]


def test_eval_texture_refusals(tmp_path):
    from pianobart_amd import eval_texture, texture
    ids = np.stack([R.from_notes(HAND, 12, PAD), R.from_notes([(0, 0, 130, 1, 9)], 12, PAD), R.from_notes(HAND, 12, PAD, L=0)])
    gp, bad = str(tmp_path / 'g.npy'), str(tmp_path / 'bad.npy')
    np.save(gp, ids)
    np.save(bad, np.zeros((3, 12, 7)))
    args = eval_texture.get_args(['--generated', gp])
    assert args.output == './texture.json' and args.reference is None and args.grid == 1024 and not hasattr(args, 'lags')
    with pytest.raises(texture.PBError, match='--cpu: the texture columns come from a HIP kernel'):
        eval_texture.main(['--generated', gp, '--cpu'])
    with pytest.raises(texture.PBError, match='no file'):
        eval_texture.main(['--generated', str(tmp_path / 'none.npy')])
    with pytest.raises(texture.PBError, match='shape'):
        eval_texture.main(['--generated', bad])
    with pytest.raises(texture.PBError, match='--dict_file'):
        eval_texture.main(['--generated', gp, '--dict_file', str(tmp_path / 'none.json')])
    with pytest.raises(texture.PBError, match='--generated holds 1 pieces with a pitched note'):
        eval_texture.main(['--generated', gp, '--reference', gp])
    long = str(tmp_path / 'long.npy')
    np.save(long, np.zeros((1, 4097, 8), dtype=np.int16))
    with pytest.raises(texture.PBError, match='4096'):
        eval_texture.main(['--generated', long])
    with pytest.raises(texture.PBError, match='--grid'):
        eval_texture.main(['--generated', gp, '--reference', gp, '--grid', '1'])
