"""CPU: the host-side rules of teacher-forced scoring -- check_score_args, the default length, eval_generation's new flag rules, the
--pick best selection (scoring.pick_best) and the two new symbols of the C ABI. No device work."""
import ctypes
import os

import numpy as np
import pytest
import torch

from pianobart_amd import _lib
from pianobart_amd import eval_generation as EG
from pianobart_amd._lib import PBError
from pianobart_amd.scoring import check_score_args, default_length, pick_best

BAR_PAD = 256
PAD = [256, 128, 129, 256, 128, 32, 254, 49]


def _piece():
    """(2, 6, 8): row 0 = 4 events then PAD, with a live-looking row BEHIND the first PAD row (does not count); row 1 = PAD from the start."""
    t = torch.tensor(PAD).repeat(2, 6, 1)
    t[0, :4] = torch.tensor([1, 2, 3, 4, 5, 6, 7, 8])
    t[0, 5] = torch.tensor([9, 2, 3, 4, 5, 6, 7, 8])
    return t


def test_default_length_counts_leading_rows_before_the_first_bar_pad():
    t = _piece()
    assert default_length(t, BAR_PAD) == [4, 0]
    assert default_length(t.numpy(), BAR_PAD) == [4, 0]
    full = t.clone()
    full[:, :, 0] = 3
    assert default_length(full, BAR_PAD) == [6, 6]
    eos = t.clone()
    eos[0, 4] = torch.tensor(PAD) + 3                  # the EOS row of a dataset piece is a target like any other
    eos[0, 5] = torch.tensor(PAD)
    assert default_length(eos, BAR_PAD) == [5, 0]


def test_check_score_args_accepts_the_legal_cases():
    t = _piece()
    assert check_score_args(t, t, None, None, 6, BAR_PAD) == ([0, 0], [4, 0])
    assert check_score_args(t, t, [2, 0], None, 8, BAR_PAD) == ([2, 0], [4, 0])
    assert check_score_args(t, t, [4, 0], [4, 0], 6, BAR_PAD) == ([4, 0], [4, 0])            # start == length: nothing scored
    assert check_score_args(t, t, np.array([0, 6]), torch.tensor([6, 6]), 6, BAR_PAD) == ([0, 6], [6, 6])
    assert check_score_args(t.int(), t.short().numpy(), [0, 0], [1, 2], None, None) == ([0, 0], [1, 2])


@pytest.mark.parametrize('kw,needle', [
    (dict(enc=torch.zeros(2, 6, 7, dtype=torch.long)), 'input_ids_encoder'),
    (dict(tgt=torch.zeros(2, 6, dtype=torch.long)), 'target_ids'),
    (dict(tgt=torch.zeros(3, 6, 8, dtype=torch.long)), 'same'),
    (dict(tgt=torch.zeros(2, 5, 8, dtype=torch.long)), 'same'),
    (dict(enc=torch.zeros(2, 6, 8)), 'integers'),
    (dict(tgt=torch.zeros(2, 6, 8, dtype=torch.bool)), 'integers'),
    (dict(max_positions=5), 'max_position_embeddings'),
    (dict(start=[0]), 'start has 1 entries'),
    (dict(length=[1, 2, 3]), 'length has 3 entries'),
    (dict(start=[0, 1.5]), 'start[1]'),
    (dict(start=[0, -1], length=[1, 1]), 'row 1'),
    (dict(start=[3, 0], length=[2, 0]), 'row 0'),
    (dict(length=[6, 7]), 'row 1'),
    (dict(start=[0, 1]), 'row 1'),                      # default length of row 1 is 0
])
def test_check_score_args_refuses_each_illegal_case(kw, needle):
    t = _piece()
    args = dict(enc=t, tgt=t, start=None, length=None, max_positions=6)
    args.update(kw)
    with pytest.raises(PBError) as e:
        check_score_args(args['enc'], args['tgt'], args['start'], args['length'], args['max_positions'], BAR_PAD)
    assert needle in str(e.value), str(e.value)


def test_lm_score_checks_its_arguments_before_any_device_work():
    from pianobart_amd.model import BartConfig, PianoBart, PianoBartLM
    from tests.golden_util import load_vocab
    e2w, w2e = load_vocab()
    cfg = BartConfig(max_position_embeddings=4, d_model=64, encoder_layers=1, decoder_layers=1, encoder_ffn_dim=64, decoder_ffn_dim=64,
                     encoder_attention_heads=2, decoder_attention_heads=2)
    m = PianoBartLM(PianoBart(cfg, e2w, w2e, precision='fp32'))
    t = _piece()
    with pytest.raises(PBError, match='max_position_embeddings'):
        m.score(t, t)
    with pytest.raises(PBError, match='row 0'):
        m.score(t[:, :4], t[:, :4], start=[5, 0])
    with pytest.raises(PBError, match='no CPU path'):       # legal arguments, CPU tensors: refused like every op
        m.score(t[:, :4], t[:, :4])


def test_eval_generation_flag_rules():
    base = ['--seed', '0', '--batch_size', '2']
    ok = lambda *extra: EG.check_args(EG.get_args(base + list(extra)))
    ok('--score')
    ok('--score', '--pick', 'best', '--samples', '3')
    ok('--score_dataset', '--prime', 'half')
    ok('--score_dataset', '--prime', '4', '--samples', '1')
    with pytest.raises(PBError, match='--pick'):
        ok('--pick', 'best', '--samples', '3')
    with pytest.raises(PBError, match='--prime'):
        ok('--score_dataset')
    with pytest.raises(PBError, match='--samples'):
        ok('--score_dataset', '--prime', 'half', '--samples', '2')
    a = EG.get_args(['--output', '/x/out.npy', '--score'])
    assert EG.score_path(a) == '/x/out_score.npy'
    assert EG.score_path(EG.get_args(['--output', '/x/out.npy', '--score_output', '/y/s.npy'])) == '/y/s.npy'


def test_pick_best_prefers_mean_logp_ranks_empty_rows_last_and_breaks_ties_low():
    s = np.zeros((5, 3, 9), dtype=np.float32)
    # prompt 0: per-position means -2, -1, -1.5 -> sample 1 (the longer sample 0 has the larger SUM of counts but the worse mean)
    s[0, 0, :8], s[0, 0, 8] = -2.5, 10
    s[0, 1, :8], s[0, 1, 8] = -0.5, 4
    s[0, 2, :8], s[0, 2, 8] = -1.5, 8
    # prompt 1: sample 0 scored nothing (count 0, sums 0): it ranks last although 0 > every log-probability
    s[1, 0] = 0
    s[1, 1, :8], s[1, 1, 8] = -3.0, 2
    s[1, 2, :8], s[1, 2, 8] = -2.0, 2
    # prompt 2: samples 1 and 2 tie exactly -> the lower index
    s[2, 0, :8], s[2, 0, 8] = -4.0, 4
    s[2, 1, :8], s[2, 1, 8] = -1.0, 4
    s[2, 2, :8], s[2, 2, 8] = -2.0, 8
    # prompt 3: nothing scored anywhere -> sample 0
    # prompt 4: the heads differ; the sum over heads decides
    s[4, 0, :8], s[4, 0, 8] = [-1, -1, -1, -1, -1, -1, -1, -9], 4
    s[4, 1, :8], s[4, 1, 8] = [-2, -2, -2, -2, -2, -2, -2, -1], 4
    s[4, 2, :8], s[4, 2, 8] = [-3, -3, -3, -3, -3, -3, -3, -3], 4
    got = pick_best(s)
    assert got.dtype == np.int64 and got.tolist() == [1, 2, 1, 0, 1]
    assert pick_best(s[:, :1]).tolist() == [0] * 5
    with pytest.raises(PBError):
        pick_best(np.zeros((5, 9)))


def test_header_declares_and_library_exports_the_score_symbols():
    decls = _lib.parse_header()
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    assert decls['pb_token_scores'] == (ctypes.c_int, [vp] * 7 + [i32, i32, vp])
    assert decls['pb_seq_scores'] == (ctypes.c_int, [vp] * 5 + [i32, i32, vp])
    if not os.path.exists(_lib.LIB_PATH):
        from pianobart_amd.build import build
        build(verbose=False)
    dll = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(dll, 'pb_token_scores') and hasattr(dll, 'pb_seq_scores')
    assert _lib.LIB.query('pb_abi_version') == 10


def test_score_ops_refuse_cpu_tensors():
    from pianobart_amd import ops
    x = torch.zeros(2, 1280)
    t = torch.zeros(2, 8, dtype=torch.int16)
    m = torch.ones(2)
    o = torch.zeros(2, 8)
    with pytest.raises(PBError):
        ops.token_scores(x, t, m, o)
    with pytest.raises(PBError):
        ops.seq_scores(o, None, None, m.view(1, 2), torch.zeros(1, 4, 8))
