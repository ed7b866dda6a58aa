"""CPU: argument rules of primed generation (decoder_prefix / prefix_len), eval_generation's --prime rule against Ablation.py's split,
and the pb_batch_decoder_start ABI entry. No device work."""
import ctypes

import numpy as np
import pytest
import torch

from pianobart_amd import _lib
from pianobart_amd._lib import PBError
from tests.golden_util import load_vocab, synth_octuple_batch

E2W, W2E = load_vocab()
PAD = np.array([256, 128, 129, 256, 128, 32, 254, 49])
S = 16


def _lm():
    from pianobart_amd.model import BartConfig, PianoBart, PianoBartLM
    cfg = BartConfig(max_position_embeddings=S, d_model=64, encoder_layers=1, decoder_layers=1, encoder_ffn_dim=128, decoder_ffn_dim=128,
                     encoder_attention_heads=2, decoder_attention_heads=2)
    return PianoBartLM(PianoBart(cfg, E2W, W2E))


def _rows(B, n, seed=0):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, PAD, size=(B, n, 8)))


def test_check_prefix_rules():
    from pianobart_amd.engine import check_prefix
    assert check_prefix(None, None, 3, S, PAD) == ([0, 0, 0], None)
    k, rows = check_prefix(_rows(2, 5), [0, 5], 2, S, PAD)
    assert k == [0, 5] and rows.shape == (2, 5, 8) and rows.dtype == torch.int64
    assert check_prefix(_rows(2, 5), None, 2, S, PAD)[0] == [5, 5]
    assert check_prefix(_rows(1, S), None, 1, S, PAD)[0] == [S]               # k = S: nothing is sampled
    assert check_prefix(_rows(2, 0), None, 2, S, PAD) == ([0, 0], None)
    bad = [(_rows(2, 5), None, 3),                                          # batch mismatch
           (_rows(2, 5)[:, :, :7], None, 2),                                # not 8 heads
           (_rows(2, 5)[0], None, 2),                                       # not (B, P, 8)
           (_rows(2, 5), [1, 6], 2),                                        # longer than the prefix
           (_rows(2, 5), [1], 2),                                           # one length per prompt
           (_rows(2, 5), [-1, 2], 2),
           (_rows(1, S + 2), None, 1),                                      # beyond the window
           (_rows(2, 5).float(), None, 2)]
    for p, lens, B in bad:
        with pytest.raises(PBError):
            check_prefix(p, lens, B, S, PAD)
    with pytest.raises(PBError):
        check_prefix(None, [1, 0], 2, S, PAD)
    for h in range(8):                                                      # a special id (PAD, SOS, EOS, MASK) in a primed row
        p = _rows(2, 5)
        p[1, 3, h] = int(PAD[h]) + h % 4
        with pytest.raises(PBError, match='ordinary'):
            check_prefix(p, None, 2, S, PAD)
        assert check_prefix(p, [5, 3], 2, S, PAD)[0] == [5, 3]              # ... beyond prefix_len it is not a prefix row
    p = _rows(1, 4)
    p[0, 0, 0] = -1
    with pytest.raises(PBError):
        check_prefix(p, None, 1, S, PAD)


def test_module_surface_refuses_bad_prefixes_before_device_work():
    """The model stays on the CPU: a refusal must come from the argument rules, before the engine binds a device."""
    m = _lm()
    x = torch.zeros(2, S, 8, dtype=torch.long)
    with pytest.raises(PBError):
        m.generate_batch(x, seeds=[1, 2], decoder_prefix=_rows(3, 4))
    with pytest.raises(PBError):
        m.generate_batch(x, seeds=[1, 2], decoder_prefix=_rows(2, 4), prefix_len=[2, 5])
    special = _rows(2, 4)
    special[0, 1, 2] = int(PAD[2]) + 1
    with pytest.raises(PBError, match='ordinary'):
        m.generate_batch(x, seeds=[1, 2], decoder_prefix=special)
    with pytest.raises(PBError):
        m(x[:1], generate=True, decoder_prefix=_rows(2, 4))
    with pytest.raises(PBError, match='ordinary'):
        m(x[:1], generate=True, decoder_prefix=special[:1])
    with pytest.raises(PBError, match='generate=True'):
        m(x, x, decoder_prefix=_rows(2, 4))


def test_prime_flag_and_rule_match_ablation_split():
    from pianobart_amd import eval_generation as EG
    assert EG.get_args([]).prime is None
    assert EG.parse_prime('half') == 'half' and EG.parse_prime('7') == 7 and EG.parse_prime('0') == 0
    for v in ('-1', 'x', '1.5'):
        with pytest.raises(PBError):
            EG.parse_prime(v)
        with pytest.raises(PBError):
            EG.check_args(EG.get_args(['--prime', v]))
    EG.check_args(EG.get_args(['--prime', 'half', '--seed', '1', '--batch_size', '4']))
    tgt = synth_octuple_batch(12, 64, seed=3)[5]                            # ordinary rows, EOS row at L - 1, PAD tail
    length = torch.sum(tgt[:, :, 0] != 256, dim=-1)                          # Ablation.py:134
    ks = EG.prime_lengths(tgt.numpy(), 'half', 256, PAD)
    assert ks == [int(v) // 2 for v in length]
    ks = EG.prime_lengths(tgt.numpy(), 40, 256, PAD)
    assert ks == [min(40, int(v) - 1) for v in length]                      # min(N, L), capped before the EOS row
    odd = tgt.clone()
    odd[0, 3] = torch.from_numpy(PAD) + 1                                   # a MASK row caps the prime at the rows before it
    assert EG.prime_lengths(odd.numpy(), 'half', 256, PAD)[0] == min(3, int(length[0]) // 2)
    enc, prefix = EG.prime_inputs(tgt, ks, PAD)
    assert prefix.shape == (12, max(ks), 8)
    for b, k in enumerate(ks):                                              # Ablation.py:138: rows >= k set to PAD
        assert torch.equal(enc[b, :k], tgt[b, :k]) and torch.equal(prefix[b, :k], tgt[b, :k])
        assert (enc[b, k:] == torch.from_numpy(PAD)).all()


def test_demo_takes_the_prime_flag():
    from pianobart_amd import demo
    assert demo.Args().prime is None and demo.Args(prime='half').prime == 'half'
    assert demo.get_args(['--prime', '64']).prime == '64' and demo.get_args([]).prime is None


def test_batch_decoder_start_is_declared_and_exported():
    decls = _lib.parse_header()
    assert decls['pb_batch_decoder_start'][1] == [ctypes.c_void_p] * 4
    assert _lib.LIB.query('pb_abi_version') == 10
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), 'pb_batch_decoder_start')
