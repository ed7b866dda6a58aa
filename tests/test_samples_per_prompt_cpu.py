"""CPU: the device-free rules of samples-per-prompt generation -- the argument helper next to check_prefix (engine.check_samples), the seed
rule of the command lines (engine.sample_seed), eval_generation's and demo's flag checks, and the native entry point
(pb_batch_decoder_share_cross) in the header and the built library at ABI 9."""
import ctypes
import os

import numpy as np
import pytest

from pianobart_amd import _lib
from pianobart_amd._lib import PBError


def test_check_samples_refuses_bad_counts_before_any_device_work():
    from pianobart_amd.engine import check_samples
    for bad in (0, -1, [2, 0, 1], [1, -3, 1]):
        with pytest.raises(PBError):
            check_samples(bad, 3, 3)
    with pytest.raises(PBError):
        check_samples([1, 2], 3, 3)                  # 2 counts for 3 prompts
    with pytest.raises(PBError):
        check_samples([1, 2, 3, 4], 3, 10)
    with pytest.raises(PBError):
        check_samples(2, 3, 5)                       # 5 generators for 6 rows
    with pytest.raises(PBError):
        check_samples([1, 5, 10], 3, 17)
    with pytest.raises(PBError):
        check_samples([1.5, 1, 1], 3, 3)
    with pytest.raises(PBError):
        check_samples('abc', 3, 3)


def test_check_samples_gives_the_prompt_major_row_map():
    from pianobart_amd.engine import check_samples
    assert check_samples(1, 3, 3) == [0, 1, 2]
    assert check_samples(4, 2, 8) == [0, 0, 0, 0, 1, 1, 1, 1]
    assert check_samples([1, 5, 2], 3, 8) == [0, 1, 1, 1, 1, 1, 2, 2]
    assert check_samples(np.asarray([2, 1]), 2, 3) == [0, 0, 1]
    assert check_samples((np.int64(1), 3), 2, 4) == [0, 1, 1, 1]
    assert check_samples(17, 1, 17) == [0] * 17
    assert check_samples([], 0, 0) == []


def test_model_surface_refuses_a_wrong_generator_count_without_a_device():
    import torch
    from pianobart_amd.model import BartConfig, PianoBart, PianoBartLM
    from tests.golden_util import load_vocab
    e2w, w2e = load_vocab()
    cfg = BartConfig(max_position_embeddings=8, d_model=64, encoder_layers=1, decoder_layers=1, encoder_ffn_dim=64, decoder_ffn_dim=64,
                     encoder_attention_heads=2, decoder_attention_heads=2)
    m = PianoBartLM(PianoBart(cfg, e2w, w2e))
    x = torch.zeros(2, 8, 8, dtype=torch.long)
    with pytest.raises(PBError):
        m.generate_batch(x, seeds=[1, 2, 3], samples_per_prompt=2)
    with pytest.raises(PBError):
        m.generate_batch(x, seeds=[1, 2], samples_per_prompt=[1, 0])
    with pytest.raises(PBError):
        m.generate_batch(x, seeds=[1, 2], samples_per_prompt=[1])
    assert m._engine is None                        # refused before an engine (and with it any device state) exists


def test_sample_seed_rule():
    from pianobart_amd.engine import sample_seed
    N, seed = 5, 3
    assert [sample_seed(seed, 0, i, N) for i in range(N)] == [seed + i for i in range(N)]       # sample 0: the seeds of a run without samples
    assert sample_seed(seed, 2, 4, N) == seed + 2 * N + 4
    all_seeds = [sample_seed(seed, j, i, N) for i in range(N) for j in range(4)]
    assert len(set(all_seeds)) == len(all_seeds)


def test_eval_generation_samples_flag_rules():
    from pianobart_amd import eval_generation as EG
    assert EG.get_args([]).samples == 1
    EG.check_args(EG.get_args(['--samples', '1']))
    EG.check_args(EG.get_args(['--samples', '2', '--seed', '5']))
    EG.check_args(EG.get_args(['--samples', '3', '--seed', '5', '--batch_size', '16']))
    with pytest.raises(PBError):
        EG.check_args(EG.get_args(['--samples', '0']))
    with pytest.raises(PBError):
        EG.check_args(EG.get_args(['--samples', '0', '--seed', '1']))
    with pytest.raises(PBError):
        EG.check_args(EG.get_args(['--samples', '2']))


def test_demo_samples_flag_rules_and_file_names():
    from pianobart_amd import demo as D
    a = D.get_args(['--samples', '3', '--seed', '7', '--output', 'out/piece.mid'])
    assert (a.samples, a.seed) == (3, 7)
    assert D.sample_paths(a.output, 3) == ['out/piece.mid', 'out/piece.1.mid', 'out/piece.2.mid']
    assert D.sample_paths('x.mid', 1) == ['x.mid']
    assert D.sample_paths('noext', 2) == ['noext', 'noext.1']
    assert (D.Args().samples, D.Args().seed) == (1, None)
    D.check_samples_args(1, None)
    D.check_samples_args(4, 0)
    with pytest.raises(PBError):
        D.check_samples_args(0, 1)
    with pytest.raises(PBError):
        D.check_samples_args(2, None)


def test_share_cross_is_declared_and_exported():
    decls = _lib.parse_header()
    assert 'pb_batch_decoder_share_cross' in decls
    restype, argtypes = decls['pb_batch_decoder_share_cross']
    assert restype is ctypes.c_int and argtypes == [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
    if not os.path.exists(_lib.LIB_PATH):
        from pianobart_amd.build import build
        build(verbose=False)
    dll = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(dll, 'pb_batch_decoder_share_cross')
    assert _lib.LIB.query('pb_abi_version') == 10
    # a null decoder or map is refused through pb_last_error, without touching a device
    assert _lib.LIB.query('pb_batch_decoder_share_cross', None, 1, None) < 0
    assert b'share_cross' in _lib.LIB.load().pb_last_error()
