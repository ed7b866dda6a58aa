"""CPU: the host half of forced tokens -- generation.check_forced (argument rules), forced_token (the one overwrite-after-sample line every
decode path shares), forced_draws (the draws made ahead), keep_mask / parse_keep, the --keep rules of eval_generation and demo, and the new
entry point in the generated binding.

Contract ("Forced tokens"): `forced` (B, S, 8), -1 = free, v >= 0 = "head h of position i of row b is v"; the reference
loop with the given heads of `current_output` overwritten right after `self.sample(x, i)`. A position with a free head draws its 8 uniforms,
a position with all 8 heads given draws nothing."""
import numpy as np
import pytest
import torch

from pianobart_amd import _lib
from pianobart_amd import generation as G
from pianobart_amd._lib import PBError

SIZES = [262, 134, 135, 262, 134, 38, 260, 55]
PAD = [256, 128, 129, 256, 128, 32, 254, 49]


def _free(P, S):
    return np.full((P, S, 8), -1, dtype=np.int64)


def test_check_forced_shape_dtype_and_range():
    P, S = 2, 6
    assert G.check_forced(None, P, S, SIZES, [0, 0]) is None
    f = _free(P, S)
    f[0, 2, 3] = 60
    f[1, 5] = [1, 2, 3, 4, 5, 6, 7, 8]
    out = G.check_forced(f, P, S, SIZES, [0, 0])
    assert out.dtype == np.int16 and out.shape == (P, S, 8) and out.flags['C_CONTIGUOUS'] and np.array_equal(out, f)
    for dt in (np.int16, np.int32):                                    # any integer type, arrays and tensors
        assert np.array_equal(G.check_forced(f.astype(dt), P, S, SIZES, [0, 0]), out)
    assert np.array_equal(G.check_forced(torch.from_numpy(f), P, S, SIZES, [0, 0]), out)
    for bad in (f[0], f[:, :5], f[:, :, :7], f[:1], np.concatenate([f, f], 1)):
        with pytest.raises(PBError, match='forced of shape'):
            G.check_forced(bad, P, S, SIZES, [0, 0])
    for bad in (f.astype(np.float32), f > 0):
        with pytest.raises(PBError, match='integers'):
            G.check_forced(bad, P, S, SIZES, [0, 0])
    for h in range(8):                                                 # the last id of every table is legal, the next one is not; so is -2
        g = _free(P, S)
        g[1, 3, h] = SIZES[h] - 1
        assert G.check_forced(g, P, S, SIZES, [0, 0])[1, 3, h] == SIZES[h] - 1
        g[1, 3, h] = SIZES[h]
        with pytest.raises(IndexError, match='head %d' % h):
            G.check_forced(g, P, S, SIZES, [0, 0])
        g[1, 3, h] = -2
        with pytest.raises(IndexError):
            G.check_forced(g, P, S, SIZES, [0, 0])


def test_check_forced_allows_specials_and_refuses_a_prefix_conflict():
    P, S = 2, 8
    f = _free(P, S)
    f[0, 4] = [v + 3 for v in PAD]                                     # an EOS-like row: every id special, inside its table
    f[1, 3, 0] = 5
    out = G.check_forced(f, P, S, SIZES, [4, 3])                       # the first position behind each prefix may be given
    assert np.array_equal(out[0, 4], f[0, 4])
    with pytest.raises(PBError, match='prefix'):
        G.check_forced(f, P, S, SIZES, [5, 0])
    with pytest.raises(PBError, match='prompt 1'):
        G.check_forced(f, P, S, SIZES, [0, 4])


def test_check_forced_all_free_is_none_and_rows_follow_the_owner_map():
    P, S = 3, 4
    assert G.check_forced(_free(P, S), P, S, SIZES, [0] * P) is None
    assert G.check_forced(torch.from_numpy(_free(P, S)), P, S, SIZES, [2] * P, owner=[0, 0, 1, 2]) is None
    f = _free(P, S)
    for p in range(P):
        f[p, p + 1, p] = 10 + p
    owner = G.check_samples([2, 1, 3], P, 6)
    rows = G.check_forced(f, P, S, SIZES, [0] * P, owner=owner)
    assert rows.dtype == np.int16 and rows.shape == (6, S, 8) and rows.flags['C_CONTIGUOUS']
    for r, p in enumerate(owner):
        assert np.array_equal(rows[r], f[p])


def test_forced_token_is_the_overwrite_after_sample():
    calls = []

    def sample():
        calls.append(1)
        return torch.arange(8) + 100
    assert torch.equal(G.forced_token(None, sample), torch.arange(8) + 100) and len(calls) == 1
    frow = np.full(8, -1, dtype=np.int16)
    assert torch.equal(G.forced_token(frow, sample), torch.arange(8) + 100) and len(calls) == 2
    frow[[1, 6]] = [7, 0]
    tok = G.forced_token(frow, sample)
    assert tok.dtype == torch.int64 and tok.tolist() == [100, 7, 102, 103, 104, 105, 0, 107] and len(calls) == 3
    frow[:] = np.arange(8)
    tok = G.forced_token(frow, sample)                                 # all 8 given: no sample, hence no draw
    assert tok.dtype == torch.int64 and tok.tolist() == list(range(8)) and len(calls) == 3


@pytest.mark.parametrize('start', [0, 5, 40])
def test_forced_draws_follow_the_position_loop(start):
    S = 40
    g = np.random.RandomState(3)
    frow = np.where(g.random_sample((S, 8)) < 0.6, g.randint(0, 30, size=(S, 8)), -1).astype(np.int16)
    frow[[7, 8, 20, S - 1]] = 4                                        # fully given positions
    frow[[9, 10]] = -1                                                 # fully free ones
    assert 0 < int((frow >= 0).all(1).sum()) < S
    for tab in (frow, None):
        a, b = np.random.RandomState(11), np.random.RandomState(11)
        want = np.zeros((S, 8))
        for i in range(start, S):
            if tab is None or (tab[i] < 0).any():
                want[i] = a.random_sample(8)
        got = G.forced_draws(b, tab, start, S)
        assert got.shape == (S, 8) and got.dtype == np.float64 and np.array_equal(got, want)
        sa, sb = a.get_state(), b.get_state()
        assert sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]


def _piece(S=12, end=8):
    x = np.random.RandomState(1).randint(0, np.asarray(PAD) - 1, size=(2, S, 8)).astype(np.int64)
    x[0, end] = [v + 3 for v in PAD]                                   # the EOS row
    x[0, end + 1:] = PAD
    return x                                                           # row 1: no special row at all


def test_keep_mask_names_eos_row_tail_and_start():
    assert G.parse_keep('Pitch, velocity') == [3, 5] == G.parse_keep(['VELOCITY', 3]) == G.parse_keep(['pitch', 'velocity', 'Pitch'])
    assert G.parse_keep(list(G.KEEP_NAMES)) == list(range(8)) and G.parse_keep('bar,position,duration,timesig') == [0, 1, 4, 6]
    for bad in ('pitch,loudness', ['note'], [8], [-1], '', [], [True]):
        with pytest.raises(PBError, match='keep'):
            G.parse_keep(bad)
    x = _piece()
    S, end = x.shape[1], 8
    f = G.keep_mask(x, ['bar', 'Position', 'duration'])
    assert f.dtype == np.int16 and f.shape == x.shape
    kept, free = [0, 1, 4], [2, 3, 5, 6, 7]
    assert np.array_equal(f[0, :end + 1][:, kept], x[0, :end + 1][:, kept])     # up to and including the EOS row
    assert (f[0, end, kept] >= np.asarray(PAD)[kept]).all()
    assert (f[0, end + 1:] == -1).all() and (f[:, :, free] == -1).all()         # the PAD tail and the other heads are free
    assert np.array_equal(f[1][:, kept], x[1][:, kept])                          # no special row: the whole window
    g = G.keep_mask(torch.from_numpy(x), 'bar,position,duration', start=[3, S])
    assert (g[0, :3] == -1).all() and np.array_equal(g[0, 3:], f[0, 3:]) and (g[1] == -1).all()
    assert np.array_equal(G.keep_mask(x, kept, start=np.asarray([0, 0])), f)
    with pytest.raises(PBError):
        G.keep_mask(x, ['bar'], start=[0])
    with pytest.raises(PBError):
        G.keep_mask(x[0], ['bar'])
    # what keep_mask builds passes the argument rules behind a prime of the same length
    assert np.array_equal(G.check_forced(g, 2, S, SIZES, [3, S]), np.where(np.arange(2)[:, None, None] == 0, g, -1))


def test_eval_generation_and_demo_keep_rules(capsys):
    from pianobart_amd import demo as D
    from pianobart_amd import eval_generation as EG
    a = EG.get_args(['--prime', 'half', '--keep', 'bar,position,duration'])
    assert a.keep == 'bar,position,duration' and EG.get_args([]).keep is None
    EG.check_args(a)
    EG.check_args(EG.get_args(['--prime', '4', '--keep', 'Pitch', '--seed', '1', '--batch_size', '16', '--samples', '2', '--score']))
    with pytest.raises(PBError, match='--keep needs --prime'):
        EG.check_args(EG.get_args(['--keep', 'pitch']))
    with pytest.raises(PBError, match='no Octuple attribute'):
        EG.check_args(EG.get_args(['--prime', 'half', '--keep', 'pitch,loudness']))
    with pytest.raises(PBError, match='--keep'):
        EG.check_args(EG.get_args(['--prime', 'half', '--keep', 'pitch', '--score_dataset']))
    with pytest.raises(SystemExit):
        EG.get_args(['--help'])
    assert 'all 8 heads of a position, kept by --keep or sampled' in ' '.join(capsys.readouterr().out.split())     # --score's help says so
    assert D.get_args(['--prime', '8', '--keep', 'pitch']).keep == 'pitch' and D.Args().keep is None
    assert D.check_keep_args(None, None) is None and D.check_keep_args('velocity,pitch', 'half') == [3, 5]
    with pytest.raises(PBError, match='--keep needs --prime'):
        D.check_keep_args('pitch', None)
    with pytest.raises(PBError, match='no Octuple attribute'):
        D.check_keep_args('pitch,loudness', 8)


def test_binding_declares_the_entry_point_and_the_abi_stays_10():
    decls = _lib.parse_header()
    assert 'pb_batch_decoder_force' in decls
    restype, argtypes = decls['pb_batch_decoder_force']
    assert len(argtypes) == 2
    assert _lib.LIB.query('pb_abi_version') == 10
    assert hasattr(_lib.LIB.load(), 'pb_batch_decoder_force')
    assert _lib.LIB.query('pb_batch_decoder_force', None, None) < 0 and b'pb_batch_decoder_force' in _lib.LIB.load().pb_last_error()


def test_forced_without_generate_is_refused():
    from pianobart_amd.model import BartConfig, PianoBart, PianoBartLM
    from tests.golden_util import load_vocab
    e2w, w2e = load_vocab()
    cfg = BartConfig(max_position_embeddings=8, d_model=64, encoder_layers=1, decoder_layers=1, encoder_ffn_dim=64, decoder_ffn_dim=64,
                     encoder_attention_heads=2, decoder_attention_heads=2, dropout=0.0)
    m = PianoBartLM(PianoBart(cfg, e2w, w2e, precision='fp32'))
    x = torch.zeros(1, 8, 8, dtype=torch.long)
    with pytest.raises(PBError, match='decoder_forced'):
        m(x, x, None, None, decoder_forced=np.full((1, 8, 8), -1))
