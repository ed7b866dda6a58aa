"""The vocabulary layout is the dictionary's (ops.Layout), not a constant of the package: what needs no GPU.

The dictionaries beside the default one (tests/vocab_layout_util.py writes them from the dictionary FORMAT):
  D_SMALL  = [70, 38, 23, 45, 22, 14, 17, 20]          total 249 (odd), table slot 72, every head narrow
  D_WIDE   = [1030, 134, 135, 518, 300, 38, 260, 55]   total 2470; heads of 1030 (p = 1), 518 (p = 0.9) and 300 classes
  D_RANKED = [262, 134, 135, 262, 262, 38, 260, 55]    pos_resolution doubled: no head over 272, but 579 classes under the heads with p < 1
The oracle sizes itself from e2w, so it is the reference for every dictionary."""
import numpy as np
import pytest
import torch

from oracle import pianobart_oracle as O
from pianobart_amd import generation as G
from pianobart_amd import ops
from pianobart_amd._lib import PBError
from tests.golden_util import load_vocab
from tests.vocab_layout_util import CLASSES, D_DEFAULT, D_RANKED, D_SMALL, D_WIDE, DICT_KEYS, SPECIALS, make_dict, synth_batch  # noqa: F401


def _cfgs(S=16, d=64, L=1, f=64, h=2):
    from pianobart_amd.model import BartConfig
    kw = dict(max_position_embeddings=S, d_model=d, encoder_layers=L, decoder_layers=L, encoder_ffn_dim=f, decoder_ffn_dim=f,
              encoder_attention_heads=h, decoder_attention_heads=h)
    return BartConfig(**kw), O.BartConfig(**kw)


def test_the_helper_writes_the_default_dictionary():
    """make_dict(D_DEFAULT) has the packaged dictionary's classes, key order, sizes and special ids: the helper speaks the format."""
    e2w, _ = load_vocab()
    mine, back = make_dict(D_DEFAULT)
    assert list(mine.keys()) == list(e2w.keys()) == DICT_KEYS
    for k in e2w:
        assert len(mine[k]) == len(e2w[k])
        for tag in SPECIALS:
            assert mine[k]['%s <%s>' % (k, tag)] == e2w[k]['%s <%s>' % (k, tag)]
        assert all(back[k][i] == w for w, i in mine[k].items())


def test_default_dictionary_gives_the_module_globals():
    from pianobart_amd.model import PianoBart
    e2w, w2e = load_vocab()
    lay = PianoBart(_cfgs()[0], e2w, w2e).layout
    assert lay == ops.DEFAULT_LAYOUT and lay == ops.Layout(D_DEFAULT) and hash(lay) == hash(ops.DEFAULT_LAYOUT)
    assert list(lay.sizes) == ops.SEG_SIZES == D_DEFAULT and list(lay.seg_off) == ops.SEG_OFF and lay.vocab == ops.VOCAB == 1280
    assert lay.tab_rows == ops.TAB_ROWS == 264 and list(lay.tab_off) == ops.TAB_OFF and lay.tab_total == ops.TAB_TOTAL == 2112
    assert list(lay.seg9) == ops.SEG_OFF and list(lay.tab9) == ops.TAB_OFF and list(ops._SEG9) == ops.SEG_OFF and list(ops._TAB9) == ops.TAB_OFF
    assert list(lay.pad8) == [256, 128, 129, 256, 128, 32, 254, 49]
    with pytest.raises(AttributeError):
        lay.vocab = 7                                              # immutable
    import copy
    import pickle
    assert copy.deepcopy(lay) == lay and pickle.loads(pickle.dumps(lay)) == lay


@pytest.mark.parametrize('sizes', [D_SMALL, D_WIDE], ids=['small', 'wide'])
def test_model_constructs_and_its_layout_and_state_dict_are_the_oracles(sizes):
    """PianoBart(cfg, e2w, w2e) for another dictionary: refused before this change ('vocabulary sizes ... differ')."""
    from pianobart_amd.model import PianoBart, PianoBartLM
    e2w, w2e = make_dict(sizes)
    c, oc = _cfgs()
    m = PianoBartLM(PianoBart(c, e2w, w2e))
    o = O.PianoBartLM(O.PianoBart(oc, e2w, w2e))
    lay = m.pianobart.layout
    assert m.pianobart.n_tokens == o.pianobart.n_tokens == sizes == list(lay.sizes)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, tuple(v.shape)) for k, v in o.state_dict().items()]
    off = np.concatenate([[0], np.cumsum(sizes)])
    assert list(lay.seg_off) == off.tolist() and lay.vocab == sum(sizes)
    rows = (max(sizes) + 7) // 8 * 8
    assert lay.tab_rows == rows and list(lay.tab_off) == [rows * i for i in range(9)] and lay.tab_total == 8 * rows
    assert lay.tab_rows == (72 if sizes is D_SMALL else 1032) and lay.vocab == (249 if sizes is D_SMALL else 2470)
    assert list(lay.pad8) == o.pianobart.pad_word_np.tolist() == m.pianobart.pad_word_np.tolist() == [n - 6 for n in sizes]
    for name, arr in (('MASK', m.pianobart.mask_word_np), ('SOS', m.pianobart.sos_word_np), ('EOS', m.pianobart.eos_word_np)):
        assert [sp[SPECIALS.index(name)] for sp in lay.specials] == arr.tolist()
    assert list(lay.seg9) == list(lay.seg_off) and list(lay.tab9) == list(lay.tab_off)
    # the flat parameter layout follows the dictionary (no device needed)
    eng = m._get_engine()
    assert eng.lay is lay and eng.slots['head.w'].shape == (sum(sizes), 64) and eng.slots['emb'].shape == (8 * rows, 256)
    # the train branch's split points
    assert m.pianobart.bar_pad_word == sizes[0] - 6


def _break(sizes, fn):
    e2w, w2e = make_dict(sizes)
    fn(e2w)
    return e2w, w2e


@pytest.mark.parametrize('what,match', [
    ('big', r'head 3 \(Pitch\) has 1089 classes.*7 \.\. 1088'),
    ('tiny', r'head 5 \(Velocity\) has 6 classes.*7 \.\. 1088'),
    ('missing', r"head 2 \(Instrument\) has no special word 'Instrument <SOS>'"),
    ('middle', r'head 1 \(Position\).*must be the last six ids'),
    ('order', r'head 0 \(Bar\).*must be the last six ids'),
    ('classes', r'needs exactly'),
])
def test_illegal_dictionaries_are_refused_by_head_and_rule_without_a_device(what, match, monkeypatch):
    from pianobart_amd._lib import LIB
    from pianobart_amd.model import PianoBart
    monkeypatch.setattr(LIB, 'load', lambda: (_ for _ in ()).throw(AssertionError('device library touched')))
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: (_ for _ in ()).throw(AssertionError('device touched')))
    sizes = list(D_SMALL)
    if what == 'big':
        sizes[3] = 1089
        e2w, w2e = make_dict(sizes)
    elif what == 'tiny':
        sizes[5] = 6
        e2w, w2e = make_dict(sizes)
    elif what == 'missing':
        def drop(e2w):
            i = e2w['Instrument'].pop('Instrument <SOS>')
            e2w['Instrument']['Instrument 999'] = i                # the size stays
        e2w, w2e = _break(sizes, drop)
    elif what == 'middle':
        def move(e2w):                                             # the specials first, the ordinary words behind them
            words = sorted(e2w['Position'], key=e2w['Position'].get)
            e2w['Position'] = {w: i for i, w in enumerate(words[-6:] + words[:-6])}
        e2w, w2e = _break(sizes, move)
    elif what == 'order':
        def swap(e2w):                                             # at the end, but <PAD> is not the first of them
            t = e2w['Bar']
            t['Bar <PAD>'], t['Bar <SEP>'] = t['Bar <SEP>'], t['Bar <PAD>']
        e2w, w2e = _break(sizes, swap)
    else:
        def rename(e2w):
            e2w['Chord'] = e2w.pop('Tempo')
        e2w, w2e = _break(sizes, rename)
    with pytest.raises(PBError, match=match):
        PianoBart(_cfgs()[0], e2w, w2e)
    with pytest.raises(PBError, match=match):
        ops.Layout.from_dict(e2w)


def test_layout_limits_are_inclusive():
    assert ops.Layout([7] * 8).tab_rows == 8 and ops.Layout([1088] * 8).vocab == 8704
    for bad in ([6] + [7] * 7, [7] * 7 + [1089]):
        with pytest.raises(PBError, match='classes'):
            ops.Layout(bad)
    with pytest.raises(PBError, match='8'):
        ops.Layout([7] * 7)


def test_sample_row_reproduces_sampling_draw_for_draw_on_the_wide_dictionary():
    """tests/test_model_cpu.py::test_fast_host_sampler_reproduces_sampling_draw_for_draw on D_WIDE's rows: the ids of sampling() / nucleus()
    (model.py:84-107) and the same np.random state afterwards, for flat, peaked and tied logits; the host scratch is as wide as the
    dictionary's largest head."""
    from pianobart_amd.model import PianoBart, PianoBartLM, _sample_tables, sampling
    e2w, w2e = make_dict(D_WIDE)
    m = PianoBartLM(PianoBart(_cfgs()[0], e2w, w2e))
    lay = m.pianobart.layout
    assert _sample_tables(lay)['probs'].shape == (8, 1040) and _sample_tables()['probs'].shape == (8, 272)
    rng = np.random.default_rng(6)
    n_multi = 0
    for trial in range(400):
        scale = [0.05, 1.0, 4.0, 12.0][trial % 4]
        row = rng.normal(scale=scale, size=lay.vocab).astype(np.float32)
        if trial % 7 == 0:
            row = np.round(row)                                    # ties
        np.random.seed(trial)
        ref = [int(sampling(torch.from_numpy(row[lay.seg_off[j]:lay.seg_off[j + 1]].copy()), m.SAMPLE_P[j], m.SAMPLE_T[j])) for j in range(8)]
        st_ref = np.random.get_state()
        np.random.seed(trial)
        got = m.sample_row(torch.from_numpy(row.copy())).tolist()
        st_got = np.random.get_state()
        assert got == ref, (trial, got, ref)
        assert st_ref[2] == st_got[2] and np.array_equal(st_ref[1], st_got[1])
        n_multi += int(ref[3] != int(np.argmax(row[lay.seg_off[3]:lay.seg_off[4]])))
    assert n_multi > 20              # the 518-class p = 0.9 head really sampled in a good share of the trials
    # the ordered sample masks with this dictionary's offsets: bars below 700 are never drawn, specials stay reachable
    row = torch.from_numpy(rng.normal(size=lay.vocab).astype(np.float32))
    for s in range(20):
        tok = m.sample_row(row, rng=np.random.RandomState(s), order=(700, -1, 0, -1))
        assert int(tok[0]) >= 700


def test_stop_and_order_rules_follow_the_dictionary():
    pad0 = D_WIDE[0] - 6                                           # 1024
    assert G.check_stop([1024], 1, pad0) is None and G.check_stop([1000, 1024], 2, pad0) == [1000, 1024]
    with pytest.raises(PBError, match=r'outside 0 \.\. 1024'):
        G.check_stop([1025], 1, pad0)
    assert G.check_order([1023, -1], 2, order_max=pad0 - 1) == [1023, -1]
    with pytest.raises(PBError, match=r'outside -1 \.\. 1023'):
        G.check_order([1024], 1, order_max=pad0 - 1)
    with pytest.raises(PBError, match=r'outside -1 \.\. 255'):
        G.check_order([256], 1)                                    # without the argument: the default dictionary's range, as before
    # the engine hands its own dictionary's range to both (no device: the argument checks come first)
    from pianobart_amd.model import PianoBart, PianoBartLM
    e2w, w2e = make_dict(D_WIDE)
    eng = PianoBartLM(PianoBart(_cfgs()[0], e2w, w2e))._get_engine()
    x = torch.zeros(1, 16, 8, dtype=torch.long)
    with pytest.raises(PBError, match=r'stop\[0\] = 1025 outside 0 \.\. 1024'):
        eng.generate(x, None, None, stop=1025)
    with pytest.raises(PBError, match=r'order\[0\] = 1024 outside -1 \.\. 1023'):
        eng.generate(x, None, None, order=1024)
    with pytest.raises(PBError, match=r'order\[1\] = 1024 outside -1 \.\. 1023'):
        eng.generate_batch(torch.zeros(2, 16, 8, dtype=torch.long), None, None, [np.random.RandomState(0) for _ in range(2)], order=[3, 1024])
    with pytest.raises(IndexError, match='1030, 134, 135, 518'):                      # a forced id is checked against this dictionary's tables
        f = -torch.ones(1, 16, 8, dtype=torch.long)
        f[0, 3, 0] = 1030
        eng.generate(x, None, None, forced=f)
    # keep_mask / infill_plan / parse_infill take the bar PAD id from the caller
    from pianobart_amd import eval_generation as EG
    assert EG.parse_infill('300:1024', pad0) == (300, 1024) and EG.parse_infill('300:1024', None) == (300, 1024)
    with pytest.raises(PBError, match='--infill takes LO:HI'):
        EG.parse_infill('300:1025', pad0)
    with pytest.raises(PBError, match='--infill takes LO:HI'):
        EG.parse_infill('300:1024')                                # the default dictionary's 256
    EG.check_args(EG.get_args(['--infill', '300:1024', '--seed', '0']))               # before the dictionary is read: the form only
    piece = synth_batch(D_WIDE, 1, 16, seed=3)[5][0].numpy()
    piece[:15, 0] = np.arange(15) * 60                              # bars 0, 60, .., 840
    pad_w, mask_w = np.asarray([n - 6 for n in D_WIDE]), np.asarray([n - 5 for n in D_WIDE])
    plan = G.infill_plan(piece, 300, 600, mask_w, pad_w)
    assert plan['stop'] == 600 and plan['k'] == 5
    with pytest.raises(PBError, match='infill_plan'):
        G.infill_plan(piece, 300, 1025, mask_w, pad_w)
    km = G.keep_mask(torch.from_numpy(piece)[None], G.parse_keep('bar'), [2], bar_pad=pad0)
    assert km.shape == (1, 16, 8) and km[0, 2:15, 0].tolist() == piece[2:15, 0].tolist()


def test_every_legal_dictionary_gets_one_of_the_two_device_samplers():
    """generation.sampler_form_for states pb_batch_decoder_sampler_init's rule: narrow while every head has <= 272 classes AND the heads
    with p < 1 hold at most 512 classes together, else wide. No legal dictionary is without a sampler (tests/test_vocab_layout_gpu.py checks
    that the device agrees and generates)."""
    from pianobart_amd.model import PianoBartLM
    P = PianoBartLM.SAMPLE_P
    assert G.sampler_form_for(D_DEFAULT, P) == 'narrow' and G.sampler_form_for(D_SMALL, P) == 'narrow'             # 451 and 87 ranked classes
    assert G.sampler_form_for(D_WIDE, P) == 'wide'                                                                 # heads over 272
    assert sum(D_RANKED[h] for h in (3, 4, 7)) == 579 and max(D_RANKED) <= 272 and G.sampler_form_for(D_RANKED, P) == 'wide'
    assert G.sampler_form_for([262, 134, 135, 272, 185, 38, 260, 55], P) == 'narrow'                               # 272 + 185 + 55 = 512: the last narrow one
    assert G.sampler_form_for([262, 134, 135, 272, 186, 38, 260, 55], P) == 'wide'
    assert G.sampler_form_for([273, 134, 135, 60, 60, 38, 260, 55], P) == 'wide'                                   # a head of 273 with p = 1
    assert G.sampler_form_for([272] * 8, [1.0] * 8) == 'narrow' and G.sampler_form_for([1088] * 8, [0.5] * 8) == 'wide'
    ops.Layout(D_RANKED)                                                                                           # legal


def test_demo_refuses_a_dictionary_its_midi_codec_does_not_speak():
    from pianobart_amd import demo as D
    assert D.check_dictionary(load_vocab()[0]) == ops.DEFAULT_LAYOUT
    assert D.check_dictionary(make_dict(D_DEFAULT)[0]) == ops.DEFAULT_LAYOUT
    with pytest.raises(PBError, match=r'head 0 \(Bar\) has 70 ids.*default dictionary only'):
        D.check_dictionary(make_dict(D_SMALL)[0])
    with pytest.raises(PBError, match=r'head 0 \(Bar\) has 1030 ids'):
        D.check_dictionary(make_dict(D_WIDE)[0])
    # demo() itself: its device check comes first on a machine without a GPU, so drive it past that with the dictionary file of D_SMALL
    import json
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        path = tmp + '/small.json'
        json.dump({'e2w': make_dict(D_SMALL)[0]}, open(path, 'w'))
        args = D.Args(dict_file=path, nopretrain=True)
        orig = torch.cuda.is_available
        torch.cuda.is_available = lambda: True
        try:
            with pytest.raises(PBError, match='default dictionary only'):
                D.demo(args)
        finally:
            torch.cuda.is_available = orig


def test_header_adds_symbols_only():
    from pianobart_amd import _lib
    decls = _lib.parse_header()
    assert decls['pb_colsum_any'] == decls['pb_colsum'] and len(decls['pb_batch_decoder_sampler_form'][1]) == 1
    assert len(decls['pb_token_scores'][1]) == 10 and len(decls['pb_batch_decoder_sampler_init'][1]) == 11 and len(decls['pb_ce_fwd_bwd'][1]) == 13
    if _lib.os.path.exists(_lib.LIB_PATH):
        assert _lib.LIB.query('pb_abi_version') == 10
