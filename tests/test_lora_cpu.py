"""CPU: the parts of LoRA that need no device -- the flags of finetune_generation, eval_generation and demo, the refusals raised before any
device work (configuration, drivers, and the argument checks of the four pb_lora_* entries, which come before the first HIP call), and the
adapter file's key names and shapes."""
import ctypes

import pytest
import torch

from pianobart_amd import _lib, lora
from pianobart_amd._lib import PBError
from tests.golden_util import load_vocab

E2W, W2E = load_vocab()


def _lm(Le=1, Ld=2, d=64):
    from pianobart_amd.model import BartConfig, PianoBart, PianoBartLM
    cfg = BartConfig(max_position_embeddings=32, d_model=d, encoder_layers=Le, decoder_layers=Ld, encoder_ffn_dim=128, decoder_ffn_dim=128,
                     encoder_attention_heads=2, decoder_attention_heads=2)
    return PianoBartLM(PianoBart(cfg, E2W, W2E, precision='fp32'))


# ---- flags ------------------------------------------------------------------------------------------------------------------------------
def test_finetune_generation_flags():
    from pianobart_amd.finetune_generation import get_args_generation
    a = get_args_generation([])
    assert a.lora_rank == 0 and lora.from_args(a) is None                       # off by default
    a = get_args_generation(['--lora_rank', '16'])
    cfg = lora.from_args(a)
    assert (cfg.rank, cfg.alpha, cfg.targets, a.lora_seed, a.lora_freeze_heads) == (16, 32, ('q', 'v', 'cq', 'cv'), 0, False)
    a = get_args_generation(['--lora_rank', '8', '--lora_alpha', '12', '--lora_targets', 'q,k,cv', '--lora_seed', '7', '--lora_freeze_heads',
                             '--augment_seed', '3', '--label_smoothing', '0.1'])
    cfg = lora.from_args(a)
    assert (cfg.rank, cfg.alpha, cfg.targets, cfg.scale, a.lora_seed, a.lora_freeze_heads) == (8, 12.0, ('q', 'k', 'cv'), 1.5, 7, True)


def test_finetune_generation_refusals_by_name(monkeypatch):
    from pianobart_amd.finetune_generation import get_args_generation
    for argv, word in ((['--lora_rank', '6'], 'multiple of 4'), (['--lora_rank', '128'], 'rank'), (['--lora_rank', '8', '--lora_targets', 'q,fc1'], "'fc1'"),
                       (['--lora_alpha', '4'], '--lora_alpha needs --lora_rank'), (['--lora_freeze_heads'], '--lora_freeze_heads needs --lora_rank'),
                       (['--lora_rank', '8', '--accum_steps', '2'], '--accum_steps 2')):
        with pytest.raises(PBError, match=word):
            lora.from_args(get_args_generation(argv))
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(PBError, match='multi-rank'):
        lora.from_args(get_args_generation(['--lora_rank', '8']))


def test_eval_generation_and_demo_take_an_adapter_file():
    from pianobart_amd import demo, eval_generation
    assert eval_generation.get_args([]).lora is None and demo.get_args([]).lora is None
    assert eval_generation.get_args(['--lora', 'x/a.lora.pt']).lora == 'x/a.lora.pt'
    assert demo.get_args(['--lora', 'a.lora.pt']).lora == 'a.lora.pt'
    assert demo.Args().lora is None and demo.Args(lora='a.lora.pt').lora == 'a.lora.pt'


def test_merge_tool_needs_its_three_paths():
    with pytest.raises(SystemExit):
        lora.main(['--ckpt', 'base.ckpt'])


# ---- configuration and engine refusals (before any device work) -----------------------------------------------------------------------------
@pytest.mark.parametrize('kw,word', [(dict(rank=0), 'rank'), (dict(rank=2), 'rank'), (dict(rank=12.0), 'rank'), (dict(rank=6), 'multiple of 4'),
                                     (dict(rank=68), '4 .. 64'), (dict(targets=('q', 'wo')), "'wo'"), (dict(targets=()), 'empty'),
                                     (dict(targets=('q', 'q')), 'twice'), (dict(alpha=float('nan')), 'alpha'), (dict(alpha='x'), 'alpha')])
def test_config_refusals(kw, word):
    with pytest.raises(PBError, match=word):
        lora.LoraConfig(**kw).check()


def test_defaults():
    c = lora.LoraConfig().check(64)
    assert (c.rank, c.alpha, c.targets, c.scale) == (8, 16, ('q', 'v', 'cq', 'cv'), 2.0)
    assert lora.parse_targets('q, v ,ck') == ('q', 'v', 'ck')


def test_engine_refuses_before_it_needs_a_device(monkeypatch):
    eng = _lm(d=32)._get_engine()
    with pytest.raises(PBError, match='d_model 32'):
        eng.attach_lora(lora.LoraConfig(rank=64))
    with pytest.raises(PBError, match='LoraConfig'):
        eng.attach_lora(dict(rank=8))
    with pytest.raises(PBError, match='unknown LoRA target'):
        eng.attach_lora(lora.LoraConfig(targets=('fc1',)))
    monkeypatch.setenv('WORLD_SIZE', '4')
    with pytest.raises(PBError, match='WORLD_SIZE = 4'):
        eng.attach_lora(lora.LoraConfig())
    monkeypatch.delenv('WORLD_SIZE')
    with pytest.raises(PBError, match='HIP device'):                           # a good request on a CPU model: there is no CPU path
        eng.attach_lora(lora.LoraConfig())
    assert eng.lora is None
    with pytest.raises(PBError, match='no LoRA adapters'):
        eng.merge_lora()
    with pytest.raises(PBError, match='no adapters are attached'):
        lora.save('/nonexistent/a.lora.pt', _lm())


# ---- the adapter file ---------------------------------------------------------------------------------------------------------------------
def test_adapter_keys_of_a_1_plus_2_layer_model():
    m = _lm(1, 2, 64)
    keys = lora.adapter_keys(m, lora.LoraConfig(rank=8, targets=lora.TARGETS), train_heads=True)
    enc, dec = 'pianobart.bart.encoder.layers.%d.', 'pianobart.bart.decoder.layers.%d.'
    mods = [enc % 0 + 'self_attn.%s_proj' % t for t in 'qkv']
    for l in range(2):
        mods += [dec % l + 'self_attn.%s_proj' % t for t in 'qkv'] + [dec % l + 'encoder_attn.%s_proj' % t for t in 'qkv']
    want = {}
    for mod in mods:
        want[mod + '.lora_A'], want[mod + '.lora_B'] = (8, 64), (64, 8)
    heads = {k: tuple(p.shape) for k, p in m.named_parameters() if k.startswith('mask_lm.')}
    assert len(heads) == 16
    want.update(heads)
    assert keys == want
    assert 'pianobart.bart.decoder.layers.0.encoder_attn.v_proj.lora_B' in keys
    # the default targets, frozen heads: q / v of every self-attention, q / v of every cross-attention, nothing else
    keys = lora.adapter_keys(m, lora.LoraConfig(rank=4), train_heads=False)
    assert len(keys) == 2 * (2 * 1 + 4 * 2) and all(k.endswith(('q_proj.lora_A', 'q_proj.lora_B', 'v_proj.lora_A', 'v_proj.lora_B')) for k in keys)
    # no backbone key: nothing in the file is a tensor of the model's own state dict but the heads
    own = set(m.state_dict())
    assert not [k for k in lora.adapter_keys(m, lora.LoraConfig(), train_heads=True) if k in own and not k.startswith('mask_lm.')]


def test_file_checks_name_the_mismatch(tmp_path):
    shape = dict(d_model=64, encoder_layers=1, decoder_layers=2, sizes=[262, 134, 135, 262, 134, 38, 260, 55])
    f = {'model': dict(shape)}
    lora.check_file(f, shape)
    for k, v in (('d_model', 128), ('encoder_layers', 2), ('decoder_layers', 1)):
        with pytest.raises(PBError, match=k):
            lora.check_file({'model': dict(shape, **{k: v})}, shape)
    with pytest.raises(PBError, match='vocabulary layout'):
        lora.check_file({'model': dict(shape, sizes=[262] * 8)}, shape)
    p = tmp_path / 'x.pt'
    torch.save({'state_dict': {}}, str(p))
    with pytest.raises(PBError, match='not an adapter file'):
        lora.read(str(p))


# ---- the C entries: every argument check comes before the first HIP call ---------------------------------------------------------------------
P = 0x10000          # a dummy, 16-byte aligned, non-null address: only good for calls that are refused, or found empty, before any HIP call


def _down(**o):
    a = dict(X=P, ldx=64, x_off=0, dtype=_lib.PB_BF16, W=2 * P, w_kr=0, T=3 * P, M=8, K=64, r=8, alpha=1.0)
    a.update(o)
    return ('pb_lora_down', a['X'], a['ldx'], a['x_off'], a['dtype'], a['W'], a['w_kr'], a['T'], a['M'], a['K'], a['r'], a['alpha'], None)


def _up(**o):
    a = dict(Y=P, ldy=64, y_off=0, dtype=_lib.PB_F32, T=2 * P, W=3 * P, w_nr=0, M=8, N=64, r=8, alpha=1.0)
    a.update(o)
    return ('pb_lora_up', a['Y'], a['ldy'], a['y_off'], a['dtype'], a['T'], a['W'], a['w_nr'], a['M'], a['N'], a['r'], a['alpha'], None)


def _wgrad(**o):
    a = dict(T=P, X=2 * P, ldx=64, x_off=0, dtype=_lib.PB_BF16, G=3 * P, g_cr=0, M=8, C=64, r=8, alpha=1.0, ws=4 * P)
    a.update(o)
    return ('pb_lora_wgrad', a['T'], a['X'], a['ldx'], a['x_off'], a['dtype'], a['G'], a['g_cr'], a['M'], a['C'], a['r'], a['alpha'], a['ws'], None)


def _merge(**o):
    a = dict(W=P, B=2 * P, A=3 * P, N=8, K=64, r=8, alpha=1.0)
    a.update(o)
    return ('pb_lora_merge', a['W'], a['B'], a['A'], a['N'], a['K'], a['r'], a['alpha'], None)


_REFUSED = [
    (_down(dtype=7), 'dtype = 7'), (_down(r=6), 'r = 6'), (_down(r=68), 'r = 68'), (_down(r=0), 'r = 0'), (_down(M=-1), 'M = -1'), (_down(K=0), 'K = 0'),
    (_down(ldx=63), 'ldx = 63'), (_down(x_off=8), 'x_off'), (_down(x_off=-1), 'x_off'), (_down(w_kr=2), 'w_kr = 2'), (_down(X=None), 'X must'),
    (_down(X=P + 1), 'X must'), (_down(W=None), 'W must'), (_down(T=P + 2), 'T must'), (_down(T=P), 'alias'),
    (_up(dtype=2), 'dtype = 2'), (_up(r=10), 'r = 10'), (_up(M=1 << 25), 'M = 33554432'), (_up(N=0), 'N = 0'), (_up(ldy=32), 'ldy = 32'),
    (_up(y_off=1), 'y_off'), (_up(w_nr=-1), 'w_nr = -1'), (_up(Y=None), 'Y must'), (_up(T=None), 'T must'), (_up(W=P + 1), 'W must'), (_up(T=P), 'alias'),
    (_wgrad(dtype=-1), 'dtype = -1'), (_wgrad(r=5), 'r = 5'), (_wgrad(M=-3), 'M = -3'), (_wgrad(C=0), 'C = 0'), (_wgrad(ldx=8), 'ldx = 8'),
    (_wgrad(x_off=60), 'x_off'), (_wgrad(g_cr=3), 'g_cr = 3'), (_wgrad(X=None), 'X must'), (_wgrad(T=None), 'T must'), (_wgrad(G=None), 'G must'),
    (_wgrad(ws=None), 'ws must'), (_wgrad(ws=4 * P + 4), 'ws must'), (_wgrad(G=P), 'distinct'),
    (_merge(r=3), 'r = 3'), (_merge(N=-1), 'N = -1'), (_merge(K=0), 'K = 0'), (_merge(W=None), 'W must'), (_merge(B=None), 'B must'),
    (_merge(A=P + 3), 'A must'), (_merge(B=P), 'alias'),
]


@pytest.mark.parametrize('call,names', _REFUSED, ids=['%s-%s' % (c[0][8:], n.replace(' ', '')) for c, n in _REFUSED])
def test_entries_refuse_bad_arguments_without_a_gpu(call, names):
    with pytest.raises(PBError) as e:
        _lib.LIB.call(*call)
    assert call[0] in str(e.value) and '(-2)' in str(e.value) and names in str(e.value), str(e.value)


@pytest.mark.parametrize('call', [_down(M=0), _up(M=0), _wgrad(M=0), _merge(N=0)], ids=['down', 'up', 'wgrad', 'merge'])
def test_zero_rows_return_ok_without_a_launch(call):
    _lib.LIB.call(*call)                                                      # raises on any non-zero status


def test_queries():
    q = _lib.LIB.query
    assert q('pb_lora_down_rows') >= 16 and q('pb_lora_up_rows') >= 16
    assert q('pb_lora_wgrad_chunk', 32768, 16) % 4 == 0 and q('pb_lora_wgrad_chunk', 1, 4) == 64
    assert q('pb_lora_wgrad_ws_floats', 32768, 16, 768) == -(-32768 // q('pb_lora_wgrad_chunk', 32768, 16)) * 16 * 768
    assert q('pb_lora_wgrad_ws_floats', 32768, 6, 768) == 0 and q('pb_lora_wgrad_chunk', -1, 8) == 0
    assert _lib.LIB.query('pb_abi_version') == 10


def test_wrappers_refuse_cpu_tensors():
    from pianobart_amd import ops
    x, t, w = torch.zeros(4, 8), torch.zeros(4, 4), torch.zeros(4, 8)
    for call in (lambda: ops.lora_down(x, w, t, 4, 8), lambda: ops.lora_up(x, t, w, 4, 8), lambda: ops.lora_wgrad(t, x, w.clone(), 4, 8),
                 lambda: ops.lora_merge(torch.zeros(8, 8), torch.zeros(8, 4), torch.zeros(4, 8), 1.0)):
        with pytest.raises(PBError, match='HIP device tensors'):
            call()
