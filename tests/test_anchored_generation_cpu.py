"""CPU: the host half of anchored generation ("Anchored notes") -- anchored_token on a table of cases, every refusal
of check_anchors by name, follows_anchors, anchor_rows, the flags of eval_generation / demo, and the header, binding and library knowing the
four entry points with the ABI version unchanged."""
import ctypes

import numpy as np
import pytest
import torch

from pianobart_amd import _lib
from pianobart_amd import generation as G
from pianobart_amd._lib import PBError
from tests.test_allowed_generation_cpu import _e2w
from tests.test_bar_schedule_cpu import PAD, _NoDevice

PAD_T = torch.as_tensor(PAD)
EOS = [int(v) + 3 for v in PAD]


def _tok(bar, pos, salt=0):
    return [bar, pos] + [(5 * salt + h) % int(PAD[h]) for h in range(2, 8)]


def _anc(*rows):
    return torch.as_tensor(np.asarray(rows, dtype=np.int64).reshape(-1, 8))


# ---------------------------------------------------------------------------------------------------------------- the rule
def test_anchored_token_table():
    A = _anc(_tok(2, 10, 1), _tok(2, 10, 2), _tok(4, 3, 3))
    sv = G.stop_vector(PAD_T, None)
    T = lambda *a: torch.as_tensor(_tok(*a))
    cases = [
        # candidate, k, stop vector -> written, k'
        (T(2, 9), 0, sv, T(2, 9), 0),                                  # in front of the anchor: the candidate
        (T(1, 100), 0, sv, T(1, 100), 0),                              # an earlier bar at a higher position: in front (lexicographic)
        (T(2, 10), 0, sv, A[0], 1),                                    # a tie in time: the anchor goes first
        (T(2, 11), 0, sv, A[0], 1),                                    # behind it
        (T(3, 0), 0, sv, A[0], 1),                                     # a later bar at a lower position: behind it (lexicographic)
        (T(2, 10, 9), 1, sv, A[1], 2),                                 # several anchors at one time: one per position
        (T(2, 10, 9), 2, sv, T(2, 10, 9), 2),                          # ... and then the candidate, in front of (4, 3)
        (T(3, 120), 2, sv, T(3, 120), 2),
        (T(4, 3), 2, sv, A[2], 3),
        (torch.as_tensor(EOS), 0, sv, A[0], 1),                        # an ending candidate with anchors left: the anchor, the row lives
        (torch.as_tensor(EOS), 2, sv, A[2], 3),
        (torch.as_tensor(EOS), 3, sv, torch.as_tensor(EOS), 3),        # ... with none left: the candidate, which ends the row
        (T(9, 9), 3, sv, T(9, 9), 3),
        (T(0, 0)[:3].tolist() + [int(PAD[3]) + 1] + T(0, 0)[4:].tolist(), 0, sv, A[0], 1),    # a special id in another head ends too
        (T(5, 0), 2, G.stop_vector(PAD_T, 5), A[2], 3),                # a stop-bar candidate with an anchor left
        (T(5, 0), 3, G.stop_vector(PAD_T, 5), T(5, 0), 3),             # ... with none left: the caller's stop test ends the row 'bar'
        (T(3, 0), 2, G.stop_vector(PAD_T, 5), T(3, 0), 2),             # below the stop bar and in front of the anchor
    ]
    for cand, k, stop, want, k2 in cases:
        cand = torch.as_tensor(cand)
        tok, kk = G.anchored_token(cand, A, k, stop, PAD_T)
        assert kk == k2 and torch.equal(tok, torch.as_tensor(want)), (cand.tolist(), k, tok.tolist(), kk)
        if kk > k:                                                     # an anchor never trips the caller's stop test
            assert not bool((tok >= stop).any())
    # no anchors: the candidate itself, the same object
    c = T(1, 1)
    assert G.anchored_token(c, None, 0, sv, PAD_T) == (c, 0)
    # a written anchor is a copy: the caller may keep it while the list lives on
    tok, _ = G.anchored_token(T(2, 10), A, 0, sv, PAD_T)
    tok[0] = 99
    assert int(A[0, 0]) == 2


def test_a_whole_row_places_every_anchor_in_order():
    """The consequences of the contract on a random walk: every anchor is written, in order, the output is time-ordered, and the row cannot
    end while anchors remain."""
    rng = np.random.RandomState(5)
    for trial in range(50):
        n = int(rng.randint(1, 9))
        t = np.sort(rng.randint(0, 8 * 128, size=n))
        A = _anc(*[_tok(int(v) // 128, int(v) % 128, i) for i, v in enumerate(t)])
        sv = G.stop_vector(PAD_T, 9)
        prev, k, out = (0, 0), 0, []
        for i in range(64):
            if rng.random_sample() < 0.15:
                cand = torch.as_tensor(EOS)
            else:                                                      # an ordered candidate: never in front of prev
                v = prev[0] * 128 + prev[1] + int(rng.randint(0, 90))
                cand = torch.as_tensor(_tok(min(v // 128, 255), v % 128, 40 + i))
            tok, k = G.anchored_token(cand, A, k, sv, PAD_T)
            if bool((tok >= sv).any()):
                break
            out.append(tok.tolist())
            prev = (int(tok[0]), int(tok[1]))
        assert k == n, (trial, k, n)
        rows = np.asarray(out + [EOS], dtype=np.int64)
        assert G.follows_anchors(rows, A) == (True, n) and G.is_time_ordered(rows)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_check_anchors_refusals_by_name():
    S = 16
    good = np.asarray([_tok(1, 5), _tok(1, 5, 1), _tok(3, 0)], dtype=np.int64)
    chk = lambda a, **kw: G.check_anchors(a, kw.pop('P', 1), S, PAD, **kw)
    out, order = chk(good)
    assert len(out) == 1 and torch.equal(out[0], torch.as_tensor(good)) and order == [0]               # anchors imply order, floor 0
    assert chk(good, order=[2 - 1])[1] == [1] and chk(None) is None and chk([]) is None and chk(np.zeros((0, 8), dtype=np.int64)) is None
    assert chk([None, []], P=2) is None                                                                  # an empty list for every row: the call without
    bad = good.copy(); bad[1, 3] = 256
    with pytest.raises(PBError, match=r'prompt 0, anchor 1, head 3: id 256 is not an ordinary event'):
        chk(bad)
    bad = good.copy(); bad[0, 0] = -1
    with pytest.raises(PBError, match=r'prompt 0, anchor 0, head 0: id -1 is not an ordinary event'):
        chk(bad)
    with pytest.raises(PBError, match=r'prompt 1: anchor 2 at \(bar 1, position 5\) lies in front of anchor 1 at \(3, 0\).*order'):
        chk([None, good[[0, 2, 1]]], P=2)
    with pytest.raises(PBError, match=r'prompt 0: anchor 0 sits in bar 1, outside the bars 2 \.\. 255'):
        chk(good, order=[2])
    with pytest.raises(PBError, match=r'prompt 0: anchor 2 sits in bar 3, outside the bars 0 \.\. 2'):
        chk(good, stop=[3])
    pre = torch.as_tensor(np.asarray([[_tok(0, 0), _tok(1, 6)]], dtype=np.int64))
    with pytest.raises(PBError, match=r'prompt 0: anchor 0 at \(bar 1, position 5\) lies in front of the last row of the prefix at \(1, 6\)'):
        chk(good, ks=[2], rows=pre)
    pre[0, 1, 1] = 5                                                   # a tie with the prefix's last row is legal
    assert chk(good, ks=[2], rows=pre) is not None
    with pytest.raises(PBError, match=r'prompt 0: 3 anchors for the 2 positions left in the window'):
        chk(good, ks=[14], rows=torch.zeros(1, 14, 8, dtype=torch.long))
    with pytest.raises(PBError, match=r'3 anchors for the 2 positions left.*max_new 2'):
        chk(good, max_new=2)
    with pytest.raises(PBError, match=r'forced tokens.*position-indexed and time-indexed givens do not combine'):
        chk(good, forced=np.zeros((1, S, 8), dtype=np.int16))
    with pytest.raises(PBError, match=r'anchors has 1 entries for 2 prompt'):
        chk([good], P=2)
    with pytest.raises(PBError, match=r'anchors\[0\] of shape \(3, 7\)'):
        chk(good[:, :7])
    with pytest.raises(PBError, match=r'must be integers'):
        chk(good.astype(np.float32))
    # per-prompt lists expand to rows under samples_per_prompt; a free prompt's rows stay free and unordered
    out, order = chk([good, None], P=2, owner=[0, 0, 1], order=None)
    assert [o is not None for o in out] == [True, True, False] and order == [0, 0, -1]


def test_generate_refuses_before_any_device_work():
    from pianobart_amd.model import PianoBartLM
    x = torch.zeros(2, 8, 8, dtype=torch.long)
    good = np.asarray([_tok(1, 5), _tok(3, 0)], dtype=np.int64)
    rngs = [np.random.RandomState(0), np.random.RandomState(1)]
    with pytest.raises(PBError, match='anchors of prompt 1: anchor 1 at'):
        G.GenerationMixin.generate_batch(_NoDevice(), x, None, None, rngs, anchors=[None, good[::-1]])
    with pytest.raises(PBError, match='forced tokens'):
        G.GenerationMixin.generate_batch(_NoDevice(), x, None, None, rngs, anchors=[good, None], forced=np.zeros((2, 8, 8), dtype=np.int16))
    with pytest.raises(PBError, match='anchors of prompt 0.*outside the bars 0 .. 0'):
        G.GenerationMixin.generate(_NoDevice(), x[:1], None, None, anchors=good, stop=1)
    with pytest.raises(PBError, match='2 anchors for the 1 positions left'):
        G.GenerationMixin.generate(_NoDevice(), x[:1], None, None, anchors=[good], max_new=1)

    class _M:                                                          # forward()'s own refusal comes before the engine does anything
        def _get_engine(self):
            return None
    with pytest.raises(PBError, match='decoder_anchors.*generate=True'):
        PianoBartLM.forward(_M(), x[:1], x[:1], decoder_anchors=good)


# ---------------------------------------------------------------------------------------------------------------- follows_anchors, anchor_rows
def test_follows_anchors_on_hand_written_rows():
    a, b, c = _tok(0, 4, 1), _tok(0, 4, 2), _tok(2, 0, 3)
    rows = np.asarray([_tok(0, 0, 7), a, b, _tok(1, 9, 8), c, EOS, a, a], dtype=np.int64)
    assert G.follows_anchors(rows, [a, b, c]) == (True, 3)
    assert G.follows_anchors(rows, [a, c]) == (True, 2) and G.follows_anchors(rows, []) == (True, 0) and G.follows_anchors(rows, None) == (True, 0)
    assert G.follows_anchors(rows, [b, a]) == (False, 1)               # out of order: a subsequence match, not a set
    assert G.follows_anchors(rows, [a, b, c], start=2) == (False, 0)   # behind `start` only
    assert G.follows_anchors(rows, [c, a]) == (False, 1)               # rows behind the first special bar id do not count
    wrong = rows.copy(); wrong[2, 5] += 1
    assert G.follows_anchors(wrong, [a, b, c]) == (False, 1)           # all 8 heads, as given: b is missing, and c cannot come before it
    back = rows.copy(); back[3] = _tok(0, 3, 8)
    assert G.follows_anchors(back, [a, b, c]) == (False, 3)            # every anchor there, but a row between them goes back in time
    assert G.follows_anchors(torch.as_tensor(rows), torch.as_tensor(np.asarray([a, b, c]))) == (True, 3)


def test_anchor_rows_skyline_and_bass():
    e2w = _e2w()
    row = lambda bar, pos, pitch, ins=0: [bar, pos, ins, pitch, 3, 10, 5, 20]
    piece = np.asarray([row(0, 0, 60), row(0, 0, 64), row(0, 0, 67),   # a chord: skyline 67, bass 60
                        row(0, 0, 128 + 40, 128),                      # a percussion note at the same time: never kept
                        row(0, 16, 55),
                        row(1, 0, 128 + 36, 128),                      # percussion alone at its time: no anchor there
                        row(1, 8, 72), row(1, 8, 48),
                        [int(v) + 3 for v in PAD], row(5, 0, 1)], dtype=np.int64)     # the EOS row ends the piece
    sky, bass = G.anchor_rows(piece, 'skyline', e2w), G.anchor_rows(piece, 'bass', e2w)
    assert sky[:, [0, 1, 3]].tolist() == [[0, 0, 67], [0, 16, 55], [1, 8, 72]]
    assert bass[:, [0, 1, 3]].tolist() == [[0, 0, 60], [0, 16, 55], [1, 8, 48]]
    assert np.array_equal(G.anchor_rows(piece, 'skyline'), sky) and sky.dtype == np.int64               # the default dictionary without names
    sel = np.zeros(len(piece), dtype=bool); sel[[1, 3, 6]] = True
    assert G.anchor_rows(torch.as_tensor(piece), sel).tolist() == piece[[1, 3, 6]].tolist()             # a row selector keeps what it names
    assert G.anchor_rows(piece[:0], 'bass').shape == (0, 8)
    assert G.check_anchors(sky, 1, 16, PAD) is not None                # what it returns is a legal anchor list
    unsorted = piece[[6, 0, 4]]
    assert G.anchor_rows(unsorted, 'skyline')[:, [0, 1]].tolist() == [[0, 0], [0, 16], [1, 8]]          # in (bar, position) order
    with pytest.raises(PBError, match='neither "skyline", "bass"'):
        G.anchor_rows(piece, 'melody')
    with pytest.raises(PBError, match='bool vector'):
        G.anchor_rows(piece, np.arange(3))
    with pytest.raises(PBError, match=r'expected \(n, 8\)'):
        G.anchor_rows(piece[:, :7], 'bass')


# ---------------------------------------------------------------------------------------------------------------- flags, header, binding
def test_cli_flag_rules():
    from pianobart_amd import demo as D
    from pianobart_amd import eval_generation as EG
    base = ['--nopretrain', '--seed', '0']
    a = EG.get_args(base)
    assert a.accompany is None and G.anchors_from_args(a, np.zeros((4, 8), dtype=np.int64), 2) is None
    for extra in (['--prime', 'half', '--accompany', 'skyline'], ['--prime', '8', '--accompany', 'bass', '--bars', '2'],
                  ['--prime', 'half', '--accompany', 'skyline', '--samples', '3', '--key', 'C:major'],
                  ['--prime', 'half', '--accompany', 'bass', '--refill', '--chords', 'C:maj', '--score']):
        a = EG.get_args(base + extra)
        a.cpu = False
        EG.check_args(a)
    piece = np.asarray([_tok(0, 0), [0, 8, 0, 60, 1, 1, 1, 1], [0, 8, 0, 72, 1, 1, 1, 1], [1, 0, 0, 50, 1, 1, 1, 1]], dtype=np.int64)
    a = EG.get_args(base + ['--prime', '1', '--accompany', 'skyline'])
    assert G.anchors_from_args(a, piece, 1)[:, 3].tolist() == [72, 50]                                  # the rows behind the prime only
    for extra, msg in ((['--accompany', 'skyline'], 'needs --prime'), (['--prime', '4', '--accompany', 'bass', '--keep', 'pitch'], 'combine with --keep'),
                       (['--accompany', 'bass', '--infill', '1:2'], 'needs --prime|combine with --infill'),
                       (['--prime', '4', '--accompany', 'bass', '--score_dataset'], 'no --accompany')):
        a = EG.get_args(base + extra)
        a.cpu = False
        with pytest.raises(PBError, match=msg):
            EG.check_args(a)
    with pytest.raises(SystemExit):
        EG.get_args(base + ['--accompany', 'melody'])
    d = D.get_args(['--prime', '8', '--accompany', 'bass'])
    assert d.accompany == 'bass' and D.Args().accompany is None and D.Args(accompany='skyline').accompany == 'skyline'
    G.check_anchor_flags(d)
    for bad in (D.Args(accompany='bass'), D.Args(accompany='bass', prime='4', keep='pitch'), D.Args(accompany='bass', prime='4', infill='1:2')):
        with pytest.raises(PBError, match='--accompany'):
            G.check_anchor_flags(bad)


def test_header_and_binding_know_the_entry_points():
    decls = _lib.parse_header()
    want = dict(pb_batch_decoder_anchor=[ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p],
                pb_batch_decoder_admit_anchor=[ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32],
                pb_batch_decoder_seek_anchor=[ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32],
                pb_batch_decoder_anchors_placed=[ctypes.c_void_p, ctypes.c_void_p])
    dll = _lib.LIB.load()
    assert dll.pb_abi_version() == 10                                  # additions only
    for name, args in want.items():
        assert decls[name] == (ctypes.c_int, args), name               # declared
        assert getattr(dll, name).argtypes == args                     # exported and bound
    assert dll.pb_batch_decoder_anchor(None, None, 1, None, None) < 0 and b'pb_batch_decoder_anchor: null argument' in dll.pb_last_error()
    assert dll.pb_batch_decoder_admit_anchor(None, 0, 0, 1) < 0 and b'pb_batch_decoder_admit_anchor' in dll.pb_last_error()
    assert dll.pb_batch_decoder_seek_anchor(None, 0, 0) < 0 and b'pb_batch_decoder_seek_anchor' in dll.pb_last_error()
    assert dll.pb_batch_decoder_anchors_placed(None, None) < 0 and b'pb_batch_decoder_anchors_placed: null argument' in dll.pb_last_error()
