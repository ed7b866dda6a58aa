"""CPU: argument handling of pianobart_amd.eval_generation, PianoBartLM.sample_row's per-prompt generator, the batched decoder's ABI
declarations and PianoBartLM.generate_batch's argument rules. No device work."""
import ctypes

import numpy as np
import pytest
import torch

from pianobart_amd import _lib
from pianobart_amd._lib import PBError
from tests.golden_util import load_vocab

E2W, W2E = load_vocab()


def test_flags_match_the_reference_plus_precision_and_seed():
    from pianobart_amd import eval_generation as EG
    a = EG.get_args([])
    assert (a.ckpt, a.dataset_path, a.dataset_name, a.output) == ('result/pretrain/pianobart/model_best.ckpt',
                                                                  './Data/output_generate/GiantMIDI1k/gen_method', 'GiantMIDI1k_test.npy', './output.npy')
    assert (a.num_workers, a.batch_size, a.max_seq_len, a.hs, a.layers, a.ffn_dims, a.heads) == (5, 1, 1024, 1024, 8, 2048, 8)
    assert (a.nopretrain, a.cpu, a.cuda_devices, a.precision, a.seed) == (False, False, [0], 'bf16', None)
    EG.check_args(a)                                              # batch 1 without --seed: the reference's loop
    EG.check_args(EG.get_args(['--batch_size', '4', '--seed', '3']))


def test_batches_without_seed_are_refused_before_any_device_work():
    from pianobart_amd import eval_generation as EG
    with pytest.raises(PBError, match='--seed'):
        EG.check_args(EG.get_args(['--batch_size', '4']))
    with pytest.raises(PBError, match='--seed'):
        EG.eval_generation(EG.get_args(['--batch_size', '4', '--dataset_path', '/nonexistent']))
    with pytest.raises(PBError, match='ONE device'):
        EG.check_args(EG.get_args(['--cuda_devices', '0', '1']))
    with pytest.raises(PBError):
        EG.check_args(EG.get_args(['--batch_size', '0', '--seed', '1']))


def test_sample_row_draws_from_the_given_generator():
    """sample_row(row, rng) == sample_row(row) with the global stream at rng's state; the global stream is untouched."""
    from pianobart_amd import ops
    from pianobart_amd.model import BartConfig, PianoBart, PianoBartLM
    cfg = BartConfig(max_position_embeddings=16, d_model=64, encoder_layers=1, decoder_layers=1, encoder_ffn_dim=128, decoder_ffn_dim=128,
                     encoder_attention_heads=2, decoder_attention_heads=2)
    m = PianoBartLM(PianoBart(cfg, E2W, W2E))
    g = torch.Generator().manual_seed(0)
    rows = [torch.randn(ops.VOCAB, generator=g) * 3 for _ in range(6)]
    np.random.seed(123)
    want = [m.sample_row(r) for r in rows]
    end = np.random.get_state()
    np.random.seed(9)
    before = np.random.get_state()
    rng = np.random.RandomState(123)
    got = [m.sample_row(r, rng) for r in rows]
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert np.array_equal(rng.get_state()[1], end[1]) and rng.get_state()[2] == end[2]
    assert np.array_equal(np.random.get_state()[1], before[1]) and np.random.get_state()[2] == before[2]


def test_generate_batch_needs_one_generator_per_prompt():
    from pianobart_amd.model import BartConfig, PianoBart, PianoBartLM
    cfg = BartConfig(max_position_embeddings=16, d_model=64, encoder_layers=1, decoder_layers=1, encoder_ffn_dim=128, decoder_ffn_dim=128,
                     encoder_attention_heads=2, decoder_attention_heads=2)
    m = PianoBartLM(PianoBart(cfg, E2W, W2E))
    x = torch.zeros(2, 16, 8, dtype=torch.long)
    with pytest.raises(PBError):
        m.generate_batch(x)                                       # neither seeds nor rngs
    with pytest.raises(PBError):
        m.generate_batch(x, seeds=[1, 2], rngs=[np.random.RandomState(1)] * 2)
    with pytest.raises(PBError):
        m.generate_batch(x, seeds=[1])


def test_batched_decoder_abi_is_declared_and_exported():
    decls = _lib.parse_header()
    names = ['pb_batch_decoder_' + n for n in ('create', 'destroy', 'reset', 'sampler_init', 'launch', 'wait', 'logs', 'seek', 'launches', 'graph')]
    assert all(n in decls for n in names)
    assert decls['pb_batch_decoder_seek'][1] == [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]
    assert len(decls['pb_batch_decoder_sampler_init'][1]) == 11
    # pb_decode_batch = the plan, B, padding, s_enc[16]
    assert ctypes.sizeof(_lib.DecodeBatch) == ctypes.sizeof(_lib.DecodePlan) + 4 + 4 + 16 * 4
    assert _lib.LIB.query('pb_abi_version') == 10
    dll = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(dll, n) for n in names)
