"""CPU: bar-bounded generation (Engine.generate / generate_batch(stop=...)) and infilling -- the argument rules (generation.check_stop),
the "n more bars" rule (stop_after_bars), the infilling plan and splice (infill_plan, infill_splice) on hand-made pieces, the
eval_generation / demo flag rules, and the two new entry points in the header and the binding. No device work."""
import os

import numpy as np
import pytest
import torch

from pianobart_amd import _lib
from pianobart_amd import generation as G
from pianobart_amd._lib import PBError

PAD = np.asarray([256, 128, 129, 256, 128, 32, 254, 49])
MASK = PAD + 1
EOS = PAD + 3
PAD0 = 256


# ---------------------------------------------------------------------------------------------------------------- check_stop
def test_check_stop_accepts_and_normalises():
    assert G.check_stop(None, 3, PAD0) is None
    assert G.check_stop([PAD0] * 3, 3, PAD0) is None                   # no real stop: the caller runs what it ran before
    assert G.check_stop(np.full(2, PAD0), 2, PAD0) is None and G.check_stop(torch.full((2,), PAD0), 2, PAD0) is None
    assert G.check_stop([4, PAD0, 0], 3, PAD0) == [4, PAD0, 0]
    assert G.check_stop((4, 5), 2, PAD0) == [4, 5]
    assert G.check_stop(np.asarray([7, 256], dtype=np.int32), 2, PAD0) == [7, 256]
    assert G.check_stop(torch.tensor([7, 9]), 2, PAD0) == [7, 9]
    got = G.check_stop([np.int64(3)], 1, PAD0)
    assert got == [3] and type(got[0]) is int
    assert G.check_stop([], 0, PAD0) is None


def test_check_stop_refusals():
    for bad, P in (([1, 2], 3), ([1, 2, 3], 2), ([], 1), (np.zeros((2, 2), dtype=np.int64), 4)):
        with pytest.raises(PBError, match='entries|integer'):
            G.check_stop(bad, P, PAD0)
    with pytest.raises(PBError, match='sequence'):
        G.check_stop(5, 1, PAD0)
    for bad in ([1.0, 2], [True, 2], ['3', 2], [None, 2], np.asarray([1.5, 2.0]), torch.tensor([1.0, 2.0])):
        with pytest.raises(PBError, match='not an integer'):
            G.check_stop(bad, 2, PAD0)
    for bad in ([-1, 2], [3, 257], [3, 1000]):
        with pytest.raises(PBError, match='outside 0 .. 256'):
            G.check_stop(bad, 2, PAD0)


def test_check_stop_expands_through_owner():
    owner = G.check_samples([3, 1, 2], 3, 6)
    assert G.check_stop([4, PAD0, 9], 3, PAD0, owner) == [4, 4, 4, PAD0, 9, 9]
    assert G.check_stop([PAD0] * 3, 3, PAD0, owner) is None
    with pytest.raises(PBError, match='entries'):                      # `stop` describes the prompts, not the rows
        G.check_stop([4] * 6, 3, PAD0, owner)


def test_stop_vector_is_pad_with_head_0_lowered():
    pad = torch.as_tensor(PAD)
    assert G.stop_vector(pad, None) is pad and G.stop_vector(pad, PAD0) is pad
    v = G.stop_vector(pad, 7)
    assert v.tolist() == [7] + PAD.tolist()[1:] and pad[0] == PAD0     # a copy
    tok = torch.tensor([7, 0, 0, 0, 0, 0, 0, 0])
    assert bool((tok >= v).any()) and not bool((tok >= pad).any()) and G.end_reason(tok, pad) == 'bar'
    assert G.end_reason(torch.as_tensor(EOS), pad) == 'special'


class _NoDevice:
    """An engine stand-in whose every attribute access fails: the calls must refuse before they touch anything but the PAD word."""
    BATCH_MAX = 16

    class pb:
        pad_word_np = PAD

    def __getattr__(self, name):
        raise AssertionError('device work before the argument check: %s' % name)


@pytest.mark.parametrize('stop', [[1], [1, 2, 3], [1, 257], [-1, 2], [1.0, 2.0], 'ab'])
def test_generate_batch_refuses_before_any_device_work(stop):
    x = torch.zeros(2, 8, 8, dtype=torch.long)
    with pytest.raises(PBError, match='stop'):
        G.GenerationMixin.generate_batch(_NoDevice(), x, None, None, [np.random.RandomState(0) for _ in range(2)], stop=stop)


@pytest.mark.parametrize('stop', [257, -1, [1, 2], 1.5])
def test_generate_refuses_before_any_device_work(stop):
    x = torch.zeros(1, 8, 8, dtype=torch.long)
    with pytest.raises(PBError, match='stop'):
        G.GenerationMixin.generate(_NoDevice(), x, None, None, stop=stop)


def test_model_surface_needs_generate():
    from pianobart_amd.model import BartConfig, PianoBart, PianoBartLM
    from tests.golden_util import load_vocab
    e2w, w2e = load_vocab()
    cfg = BartConfig(max_position_embeddings=8, d_model=64, encoder_layers=1, decoder_layers=1, encoder_ffn_dim=64, decoder_ffn_dim=64,
                     encoder_attention_heads=2, decoder_attention_heads=2, dropout=0.0)
    m = PianoBartLM(PianoBart(cfg, e2w, w2e, precision='fp32'))
    x = torch.zeros(1, 8, 8, dtype=torch.long)
    with pytest.raises(PBError, match='decoder_stop.*generate=True'):
        m(x, x, None, None, decoder_stop=4)
    assert np.array_equal(m.pianobart.pad_word_np, PAD) and np.array_equal(m.pianobart.mask_word_np, MASK)


# ---------------------------------------------------------------------------------------------------------------- stop_after_bars
def _rows(bars):
    """Ordinary rows with the given bar ids; the other heads count up so that every row is distinct."""
    x = np.zeros((len(bars), 8), dtype=np.int64)
    x[:, 0] = bars
    for h in range(1, 8):
        x[:, h] = (np.arange(len(bars)) * (h + 1) + h) % (PAD[h] - 1)
    return x


def test_stop_after_bars():
    assert G.stop_after_bars(None, 4, PAD0) == 4                       # unprimed: bars 0 .. 3
    assert G.stop_after_bars(np.zeros((0, 8), dtype=np.int64), 2, PAD0) == 2
    assert G.stop_after_bars(None, 0, PAD0) == 0
    pre = _rows([0, 0, 1, 3, 3])                                       # primed mid-bar: bar 3 is finished, then 4 and 5
    assert G.stop_after_bars(pre, 2, PAD0) == 6
    assert G.stop_after_bars(torch.as_tensor(pre), 0, PAD0) == 4       # n = 0: only the bar it is in
    assert G.stop_after_bars(_rows([250]), 4, PAD0) == 255
    assert G.stop_after_bars(_rows([250]), 5, PAD0) == 256 and G.stop_after_bars(_rows([255]), 9, PAD0) == 256       # the clamp: no stop
    for bad in (-1, 1.5, True, None):
        with pytest.raises(PBError, match='bars'):
            G.stop_after_bars(pre, bad, PAD0)


# ---------------------------------------------------------------------------------------------------------------- infill_plan / infill_splice
def _piece(bars, S, eos=True):
    """(S, 8): ordinary rows with the given bars, the EOS row, PAD behind."""
    x = np.tile(PAD, (S, 1)).astype(np.int64)
    x[:len(bars)] = _rows(bars)
    if eos:
        x[len(bars)] = EOS
    return x


BARS = [0, 0, 1, 2, 2, 2, 3, 4, 4, 6]


def test_infill_plan_rows_mode():
    S = 16
    piece = _piece(BARS, S)
    plan = G.infill_plan(piece, 2, 4, MASK, PAD)
    assert plan['k'] == 3 and plan['stop'] == 4
    assert np.array_equal(plan['prefix'], piece[:3])
    assert np.array_equal(plan['suffix'], piece[7:11]) and np.array_equal(plan['suffix'][-1], EOS)      # the EOS row travels with the suffix
    enc = plan['enc']
    assert enc.shape == (S, 8) and np.array_equal(enc[:3], piece[:3]) and np.array_equal(enc[7:], piece[7:])
    assert (enc[3:7] == MASK).all()                                    # TokenMask: one MASK row per row, the length preserved
    assert np.array_equal(piece, _piece(BARS, S))                      # the piece is not written to
    t = G.infill_plan(torch.as_tensor(piece), 2, 4, torch.as_tensor(MASK), torch.as_tensor(PAD))
    assert all(np.array_equal(t[key], plan[key]) for key in ('prefix', 'suffix', 'enc')) and t['k'] == 3


def test_infill_plan_span_mode():
    S = 16
    piece = _piece(BARS, S)
    plan = G.infill_plan(piece, 2, 4, MASK, PAD, mode='span')
    enc = plan['enc']
    assert enc.shape == (S, 8) and np.array_equal(enc[:3], piece[:3]) and np.array_equal(enc[3], MASK)  # TokenInfilling: ONE MASK row
    assert np.array_equal(enc[4:8], piece[7:11]) and (enc[8:] == PAD).all()                             # the rest moves up, PAD fills the tail
    assert plan['k'] == 3 and np.array_equal(plan['suffix'], piece[7:11])


def test_infill_plan_empty_region():
    S = 12
    piece = _piece(BARS, S)                                            # no row of bar 5
    rows = G.infill_plan(piece, 5, 6, MASK, PAD)
    assert rows['k'] == 9 and np.array_equal(rows['enc'], piece)       # 'rows' masks nothing
    assert np.array_equal(rows['suffix'], piece[9:11])
    span = G.infill_plan(piece, 5, 6, MASK, PAD, mode='span')
    assert np.array_equal(span['enc'][:9], piece[:9]) and np.array_equal(span['enc'][9], MASK) and np.array_equal(span['enc'][10:], piece[9:11])
    full = _piece(BARS, 11)                                            # no PAD row to give way: the inserted row pushes the last one out
    assert np.array_equal(G.infill_plan(full, 5, 6, MASK, PAD, mode='span')['enc'][-1], full[9])


def test_infill_plan_region_at_the_start_and_at_the_end():
    S = 14
    piece = _piece(BARS, S)
    first = G.infill_plan(piece, 0, 2, MASK, PAD)
    assert first['k'] == 0 and first['prefix'].shape == (0, 8) and np.array_equal(first['suffix'], piece[3:11])
    last = G.infill_plan(piece, 4, PAD0, MASK, PAD)
    assert last['k'] == 7 and last['stop'] == PAD0 and np.array_equal(last['suffix'], piece[10:11])     # only the EOS row is left
    bare = _piece(BARS, S, eos=False)                                  # a piece without an EOS row: an empty suffix, no PAD row in it
    assert G.infill_plan(bare, 4, PAD0, MASK, PAD)['suffix'].shape == (0, 8)
    assert (G.infill_plan(bare, 4, PAD0, MASK, PAD)['enc'][7:10] == MASK).all()
    window = _rows(list(range(8)))                                     # a piece that fills the window: no special row at all
    assert np.array_equal(G.infill_plan(window, 2, 4, MASK, PAD)['suffix'], window[4:])


def test_infill_plan_refusals():
    S = 14
    with pytest.raises(ValueError, match='decrease at row 3'):
        G.infill_plan(_piece([0, 1, 2, 1, 3], S), 1, 2, MASK, PAD)     # not sorted: it has no region
    G.infill_plan(_piece([0, 1, 2], S), 1, 2, MASK, PAD)
    piece = _piece(BARS, S)
    for lo, hi in ((2, 2), (3, 2), (-1, 2), (0, 257), (1.0, 2), (True, 2)):
        with pytest.raises(PBError, match='lo < hi'):
            G.infill_plan(piece, lo, hi, MASK, PAD)
    with pytest.raises(PBError, match='mode'):
        G.infill_plan(piece, 1, 2, MASK, PAD, mode='bars')
    with pytest.raises(PBError, match='shape'):
        G.infill_plan(piece[None], 1, 2, MASK, PAD)


def test_infill_splice():
    S = 16
    piece = _piece(BARS, S)
    plan = G.infill_plan(piece, 2, 4, MASK, PAD)
    new = _rows([2, 3])                                                # the model wrote two rows where the piece had four
    out = np.tile(PAD, (S, 1)).astype(np.int64)
    out[:3], out[3:5] = plan['prefix'], new
    row, cut = G.infill_splice(out, plan['suffix'], S, PAD0)
    assert not cut and row.shape == (S, 8)
    assert np.array_equal(row[:3], piece[:3]) and np.array_equal(row[3:5], new) and np.array_equal(row[5:9], piece[7:11]) and (row[9:] == PAD).all()
    row_t, cut_t = G.infill_splice(torch.as_tensor(out), plan['suffix'], S, PAD0)
    assert not cut_t and np.array_equal(row_t, row)
    frow, _ = G.infill_splice(out.astype(np.float32), plan['suffix'], S, PAD0)      # the dtype of the generated row is kept
    assert frow.dtype == np.float32 and np.array_equal(frow, row.astype(np.float32))
    empty, cut = G.infill_splice(np.tile(PAD, (S, 1)), plan['suffix'], S, PAD0)     # nothing emitted: the suffix alone
    assert not cut and np.array_equal(empty[:4], piece[7:11]) and (empty[4:] == PAD).all()


def test_infill_splice_overflow_is_reported():
    S = 16
    piece = _piece(BARS, S)
    plan = G.infill_plan(piece, 2, 4, MASK, PAD)
    out = np.tile(PAD, (S, 1)).astype(np.int64)
    out[:3] = plan['prefix']
    out[3:13] = _rows([2] * 10)                                        # 13 emitted rows + 4 suffix rows > 16
    row, cut = G.infill_splice(out, plan['suffix'], S, PAD0)
    assert cut and row.shape == (S, 8) and np.array_equal(row[:13], out[:13]) and np.array_equal(row[13:], plan['suffix'][:3])
    out[13:] = _rows([3] * 3)                                          # a row that ran to the window's end: no PAD row in it
    row, cut = G.infill_splice(out, plan['suffix'], S, PAD0)
    assert cut and np.array_equal(row, out)
    out[12:] = PAD
    row, cut = G.infill_splice(out, plan['suffix'], S, PAD0)           # 12 + 4 = 16: it just fits
    assert not cut and np.array_equal(row[12:], plan['suffix'])


@pytest.mark.parametrize('mode', ['rows', 'span'])
@pytest.mark.parametrize('lo,hi', [(2, 4), (0, 1), (4, 256), (5, 6), (0, 256)])
def test_plan_then_splice_of_the_original_region_gives_back_the_piece(mode, lo, hi):
    S = 16
    piece = _piece(BARS, S)
    plan = G.infill_plan(piece, lo, hi, MASK, PAD, mode=mode)
    m = int((np.asarray(BARS) < hi).sum())
    out = np.tile(PAD, (S, 1)).astype(np.int64)
    out[:m] = piece[:m]                                                # the prime and the region's own rows, as a generated row holds them
    assert np.array_equal(out[:plan['k']], plan['prefix'])
    row, cut = G.infill_splice(out, plan['suffix'], S, PAD0)
    assert not cut and np.array_equal(row, piece)


# ---------------------------------------------------------------------------------------------------------------- flags
def test_eval_generation_bars_and_infill_rules():
    from pianobart_amd import eval_generation as EG
    a = EG.get_args([])
    assert a.bars is None and a.infill is None and a.infill_mode == 'rows'
    EG.check_args(a)
    assert EG.parse_infill(None) is None and EG.parse_infill('2:4') == (2, 4) and EG.parse_infill('0:256') == (0, 256)
    for bad in ('2', '4:2', '2:2', '-1:3', '2:257', 'a:b', '1:2:3', ''):
        with pytest.raises(PBError, match='--infill takes LO:HI'):
            EG.parse_infill(bad)
    # --bars: with and without --prime, with --keep, --samples, --refill, --score and --pick
    EG.check_args(EG.get_args(['--bars', '4']))
    EG.check_args(EG.get_args(['--bars', '0', '--prime', 'half', '--keep', 'bar', '--seed', '1', '--batch_size', '16']))
    EG.check_args(EG.get_args(['--bars', '2', '--prime', '8', '--seed', '1', '--samples', '3', '--score', '--pick', 'best']))
    EG.check_args(EG.get_args(['--bars', '2', '--seed', '1', '--refill', '4', '--score']))
    with pytest.raises(PBError, match='--bars must be >= 0'):
        EG.check_args(EG.get_args(['--bars', '-1']))
    with pytest.raises(PBError, match='--score_dataset generates nothing: it takes no --bars'):
        EG.check_args(EG.get_args(['--bars', '2', '--prime', 'half', '--score_dataset']))
    # --infill: needs --seed; excludes --prime, --keep, --bars, --score_dataset; combines with --samples, --refill, --score, --pick
    EG.check_args(EG.get_args(['--infill', '2:4', '--seed', '0']))
    EG.check_args(EG.get_args(['--infill', '2:4', '--seed', '0', '--infill_mode', 'span', '--batch_size', '16']))
    EG.check_args(EG.get_args(['--infill', '2:4', '--seed', '0', '--samples', '3', '--score', '--pick', 'best']))
    EG.check_args(EG.get_args(['--infill', '2:4', '--seed', '0', '--refill', '--score']))
    with pytest.raises(PBError, match='--infill needs --seed'):
        EG.check_args(EG.get_args(['--infill', '2:4']))
    with pytest.raises(PBError, match='--infill takes LO:HI'):
        EG.check_args(EG.get_args(['--infill', '4:2', '--seed', '0']))
    for flag, extra in (('prime', ['--prime', 'half']), ('keep', ['--keep', 'bar']), ('bars', ['--bars', '2'])):
        with pytest.raises(PBError, match='--infill does not combine with --%s' % flag):
            EG.check_args(EG.get_args(['--infill', '2:4', '--seed', '0'] + extra))
    with pytest.raises(PBError, match='--infill'):
        EG.check_args(EG.get_args(['--infill', '2:4', '--seed', '0', '--score_dataset']))
    with pytest.raises(PBError, match='--infill_mode span needs --infill'):
        EG.check_args(EG.get_args(['--infill_mode', 'span']))
    with pytest.raises(SystemExit):
        EG.get_args(['--infill_mode', 'bars'])


def test_demo_bars_and_infill_rules():
    from pianobart_amd import demo as D
    a = D.get_args(['--bars', '3'])
    assert a.bars == 3 and a.infill is None and D.Args().bars is None and D.Args(infill='1:2').infill == '1:2' and D.Args().infill_mode == 'rows'
    assert D.check_bar_args(None, None, None, None, None) is None and D.check_bar_args(3, None, 'half', 'bar', None) is None
    assert D.check_bar_args(None, '2:4', None, None, 0) == (2, 4)
    with pytest.raises(PBError, match='--bars must be >= 0'):
        D.check_bar_args(-2, None, None, None, None)
    with pytest.raises(PBError, match='--infill needs --seed'):
        D.check_bar_args(None, '2:4', None, None, None)
    for flag, kw in (('prime', dict(prime='half')), ('keep', dict(keep='bar')), ('bars', dict(bars=1))):
        args = dict(bars=None, infill='2:4', prime=None, keep=None, seed=1)
        args.update(kw)
        with pytest.raises(PBError, match='--infill does not combine with --%s' % flag):
            D.check_bar_args(**args)


# ---------------------------------------------------------------------------------------------------------------- header and binding
def test_header_and_binding_have_the_entry_points():
    decls = _lib.parse_header()
    assert len(decls['pb_batch_decoder_stop'][1]) == 2 and len(decls['pb_batch_decoder_admit_stop'][1]) == 3
    assert len(decls['pb_batch_decoder_admit'][1]) == 11 and len(decls['pb_batch_decoder_sampler_init'][1]) == 11       # no signature changed
    src = ' '.join(open(_lib.HEADER).read().replace('*', ' ').split())          # comment blocks: ' * ' starts every line
    for words in ('pb_batch_decoder_stop', 'pb_batch_decoder_admit_stop', 'Stop at a bar (an addition to ABI 10)',
                  'never inherits its previous occupant', 'same launches per step'):
        assert words in src, words
    if not os.path.exists(_lib.LIB_PATH):
        from pianobart_amd.build import build
        build(verbose=False)
    dll = _lib.LIB.load()
    assert _lib.LIB.query('pb_abi_version') == 10
    for name in ('pb_batch_decoder_stop', 'pb_batch_decoder_admit_stop'):
        assert hasattr(dll, name)
    assert _lib.LIB.query('pb_batch_decoder_stop', None, None) < 0 and b'pb_batch_decoder_stop' in dll.pb_last_error()
    assert _lib.LIB.query('pb_batch_decoder_admit_stop', None, 0, 4) < 0 and b'pb_batch_decoder_admit_stop' in dll.pb_last_error()
