"""CPU: refilled batched generation (Engine.generate_batch(refill=...)) -- the argument rules (generation.check_refill), the slot / slice
bookkeeping (refill.RefillSchedule) on hand-made finish orders, the two new entry points in the header and the binding, and the
eval_generation flag rules. No device work."""
import os

import numpy as np
import pytest
import torch

from pianobart_amd import _lib
from pianobart_amd import generation as G
from pianobart_amd._lib import PBError
from pianobart_amd.refill import RefillSchedule


def test_check_refill_values():
    assert G.check_refill(False) == 0 and G.check_refill(None) == 0
    assert G.check_refill(True) == 16 and G.check_refill(2) == 2 and G.check_refill(16) == 16 and G.check_refill(np.int64(5)) == 5
    assert G.check_refill(False, samples=3) == 0                       # off: samples are today's business
    for bad in ('4', 4.0, [4], (2,), 1.5):
        with pytest.raises(PBError, match='refill must be'):
            G.check_refill(bad)
    for bad in (1, 17, 0, -3):
        with pytest.raises(PBError, match='slot count'):
            G.check_refill(bad)
    for samples in (1, 2, [1, 2]):
        with pytest.raises(PBError, match='samples'):
            G.check_refill(4, samples=samples)
        with pytest.raises(PBError, match='samples'):
            G.check_refill(True, samples=samples)


class _NoDevice:
    """An engine stand-in whose every attribute access fails: generate_batch must refuse before it touches anything."""
    BATCH_MAX = 16

    def __getattr__(self, name):
        raise AssertionError('device work before the argument check: %s' % name)


@pytest.mark.parametrize('refill,samples', [('x', None), (1, None), (17, None), (4, 2), (True, [1, 1])])
def test_generate_batch_refuses_before_any_device_work(refill, samples):
    x = torch.zeros(2, 8, 8, dtype=torch.long)
    with pytest.raises(PBError):
        G.GenerationMixin.generate_batch(_NoDevice(), x, None, None, [np.random.RandomState(0) for _ in range(2)], samples=samples, refill=refill)


def test_model_surface_refuses_before_any_device_work():
    from pianobart_amd.model import BartConfig, PianoBart, PianoBartLM
    from tests.golden_util import load_vocab
    e2w, w2e = load_vocab()
    cfg = BartConfig(max_position_embeddings=8, d_model=64, encoder_layers=1, decoder_layers=1, encoder_ffn_dim=64, decoder_ffn_dim=64,
                     encoder_attention_heads=2, decoder_attention_heads=2, dropout=0.0)
    m = PianoBartLM(PianoBart(cfg, e2w, w2e, precision='fp32'))
    x = torch.zeros(2, 8, 8, dtype=torch.long)
    for kw in (dict(refill=1), dict(refill=17), dict(refill='yes'), dict(refill=4, samples_per_prompt=1)):
        with pytest.raises(PBError, match='refill'):
            m.generate_batch(x, None, seeds=[1, 2], **kw)


def _drive(rows, slots, slices, finish_order):
    """Run a whole schedule: finish_order(live slots, step) picks the slot that stops next. Checks the invariants at every move and
    returns (rows in admission order, the (row, slot, slice) of every admission)."""
    sc = RefillSchedule(rows, slots, slices)
    live_rows, released, log = set(), set(range(slices)), []

    def check():
        owners = [r for r in sc.slot_row if r is not None]
        assert len(owners) == len(set(owners))                         # no row in two slots
        held = [c for c in sc.slot_slice if c is not None]
        assert len(held) == len(set(held))                             # no slice under two live rows
        ready_slices = [c for _, c in sc.ready]
        assert not set(held) & set(ready_slices) and len(ready_slices) == len(set(ready_slices))
        for c, r in enumerate(sc.slice_row):                           # slice_row is the ownership the two lists spell out
            assert (r is not None) == (c in held or c in ready_slices)

    def fill():
        while True:
            got = sc.prepare()
            if got is None:
                break
            r, c = got
            assert c in released, 'slice %d handed out before it was released' % c
            released.discard(c)
            assert c == min(released | {c})                            # the lowest free slice
            check()
        while True:
            got = sc.admit()
            if got is None:
                break
            r, s, c = got
            assert r not in live_rows and sc.slice_row[c] == r
            assert all(sc.slot_row[t] is not None for t in range(s))   # the lowest free slot
            live_rows.add(r)
            log.append((r, s, c))
            check()

    fill()
    step = 0
    while not sc.done():
        live = [s for s, r in enumerate(sc.slot_row) if r is not None]
        assert live, 'rows wait but no slot is live'
        s = finish_order(live, step)
        r, c = sc.finish(s)
        live_rows.discard(r)
        assert c not in released
        released.add(c)
        check()
        fill()                                                         # hand-over first, then the next prompts are prepared ahead
        fill()
        step += 1
    assert sc.free_slot() == 0 and sc.free_slice() == 0 and not sc.ready and not sc.waiting
    return [r for r, _, _ in log], log


@pytest.mark.parametrize('rows,slots,slices', [(12, 4, 8), (11, 4, 5), (19, 16, 19), (5, 2, 2), (3, 3, 6), (0, 2, 4), (7, 3, 4)])
def test_schedule_admits_every_row_once_in_row_order(rows, slots, slices):
    g = np.random.RandomState(rows * 100 + slots)
    orders = [lambda live, k: live[0], lambda live, k: live[-1], lambda live, k: live[k % len(live)], lambda live, k: live[int(g.randint(len(live)))]]
    for order in orders:
        admitted, log = _drive(rows, slots, slices, order)
        assert admitted == list(range(rows))                           # each row exactly once, in row order
        assert [s for _, s, _ in log[:min(rows, slots)]] == list(range(min(rows, slots)))      # the first rows: slot b, slice b
        assert [c for _, _, c in log[:min(rows, slots)]] == list(range(min(rows, slots)))


def test_schedule_prepares_ahead_and_refuses_misuse():
    sc = RefillSchedule(6, 2, 3)
    assert sc.prepare() == (0, 0) and sc.prepare() == (1, 1) and sc.prepare() == (2, 2) and sc.prepare() is None      # every slice owned
    assert sc.admit() == (0, 0, 0) and sc.admit() == (1, 1, 1) and sc.admit() is None          # row 2 is prepared and waits for a slot
    assert sc.finish(1) == (1, 1)
    assert sc.admit() == (2, 1, 2)                                     # the hand-over needs no encoder pass: its slice was ready
    assert sc.prepare() == (3, 1) and sc.prepare() is None             # the released slice goes to the next waiting row
    with pytest.raises(ValueError):
        RefillSchedule(3, 4, 2)
    sc.finish(0)
    with pytest.raises(ValueError):
        sc.finish(0)
    assert not sc.done()


def test_header_and_binding_have_the_entry_points():
    decls = _lib.parse_header()
    assert len(decls['pb_batch_decoder_dynamic'][1]) == 2 and len(decls['pb_batch_decoder_admit'][1]) == 11
    assert len(decls['pb_batch_decoder_fence'][1]) == 2
    src = ' '.join(open(_lib.HEADER).read().replace('*', ' ').split())          # comment blocks: ' * ' starts every line
    for words in ('pb_batch_decoder_dynamic', 'pb_batch_decoder_admit', 'a live row is refused', 'Launches per step do not change'):
        assert words in src, words
    if not os.path.exists(_lib.LIB_PATH):
        from pianobart_amd.build import build
        build(verbose=False)
    dll = _lib.LIB.load()
    assert _lib.LIB.query('pb_abi_version') == 10
    for name in ('pb_batch_decoder_dynamic', 'pb_batch_decoder_admit', 'pb_batch_decoder_fence'):
        assert hasattr(dll, name)
    assert _lib.LIB.query('pb_batch_decoder_dynamic', None, 4) < 0 and b'pb_batch_decoder_dynamic' in dll.pb_last_error()
    assert _lib.LIB.query('pb_batch_decoder_admit', None, 0, 0, 1, -1, None, 1, None, None, None, None) < 0
    assert b'pb_batch_decoder_admit' in dll.pb_last_error()


def test_eval_generation_refill_rules():
    from pianobart_amd import eval_generation as EG
    assert EG.get_args([]).refill is None and EG.get_args(['--refill']).refill == 0 and EG.get_args(['--refill', '4']).refill == 4
    EG.check_args(EG.get_args(['--refill', '--seed', '3']))
    EG.check_args(EG.get_args(['--refill', '4', '--seed', '3', '--batch_size', '8', '--prime', 'half', '--keep', 'bar', '--score']))
    with pytest.raises(PBError, match='--refill needs --seed'):
        EG.check_args(EG.get_args(['--refill']))
    with pytest.raises(PBError, match='--samples 2'):
        EG.check_args(EG.get_args(['--refill', '--seed', '3', '--samples', '2']))
    for bad in ('1', '17'):
        with pytest.raises(PBError, match='slot count'):
            EG.check_args(EG.get_args(['--refill', bad, '--seed', '3']))
