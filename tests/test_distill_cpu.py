"""CPU: the distillation reference (tests/distill_ref.py) stands without a GPU, and so do the host parts of the feature: the float64
restatement against float64 autograd, its reduction to tests/row_ref.ce_fwd_bwd, the teacher == student fixed point, the new command
line flags of both trainers, distill.load_teacher on the two checkpoint formats it accepts and the one it refuses, and the two new symbols
of the ABI."""
import ctypes
import os

import pytest
import torch

from tests import distill_ref as DR
from tests import row_ref as R
from tests.golden_util import load_vocab

SIZES = [70, 7, 8, 64, 65, 129, 9, 12]
OFF = [0]
for _n in SIZES:
    OFF.append(OFF[-1] + _n)


def _inputs(T=11, seed=0):
    g = torch.Generator().manual_seed(seed)
    z = 2 * torch.randn(T, OFF[8], generator=g, dtype=torch.float64)
    u = 2 * torch.randn(T, OFF[8], generator=g, dtype=torch.float64)
    tgt = torch.stack([torch.randint(0, n, (T,), generator=g) for n in SIZES], 1)
    tgt[0] = 0
    tgt[T - 1] = torch.tensor(SIZES) - 1
    tgt[1, 3] = -1                                  # outside its head: scores a logit of 0, no one-hot column
    tgt[2, 4] = SIZES[4]
    m = (torch.rand(T, 8, generator=g) < 0.7).double()
    m[0] = 1
    coef = torch.rand(8, generator=g, dtype=torch.float64) + 0.1
    return z, u, tgt, m, coef


def _autograd_loss(z, u, tgt, m, coef, alpha, tau, eps):
    """sum_{t,i} coef_i m_ti loss_ti written with torch's own log_softmax / kl formulas, so the comparison is not the restatement against itself."""
    total = z.new_zeros(())
    for i in range(8):
        o, n = OFF[i], SIZES[i]
        lp = torch.log_softmax(z[:, o:o + n], -1)
        ok = (tgt[:, i] >= 0) & (tgt[:, i] < n)
        picked = lp.gather(1, tgt[:, i].clamp(0, n - 1)[:, None])[:, 0]
        # a target outside its head scores a logit of 0: -log p[y] = logsumexp(z) - 0
        hard = torch.where(ok, -picked, torch.logsumexp(z[:, o:o + n], -1))
        hard_e = (1 - eps) * hard - (eps / n) * lp.sum(-1)
        lpt = torch.log_softmax(z[:, o:o + n] / tau, -1)
        lq = torch.log_softmax(u[:, o:o + n] / tau, -1)
        kl = (lq.exp() * (lq - lpt)).sum(-1)
        total = total + (coef[i] * m[:, i] * ((1 - alpha) * hard_e + alpha * tau * tau * kl)).sum()
    return total


@pytest.mark.parametrize('alpha,tau,eps', [(0.0, 1.0, 0.0), (1.0, 1.0, 0.0), (0.5, 2.0, 0.0), (0.3, 0.5, 0.1), (0.0, 1.0, 0.1)])
def test_restatement_matches_float64_autograd(alpha, tau, eps):
    z, u, tgt, m, coef = _inputs()
    r = DR.distill_fwd_bwd(z, u, tgt, m, OFF, coef, alpha, tau, eps)
    zz = z.clone().requires_grad_(True)
    loss = _autograd_loss(zz, u, tgt, m, coef, alpha, tau, eps)
    loss.backward()
    loss = loss.detach()
    assert float((r['dlogits'] - zz.grad).abs().max()) <= 1e-12
    assert float(((r['terms'][0] * coef[None, :]).sum() - loss.detach()).abs()) <= 1e-10 * max(1.0, float(loss.abs()))


def test_out_of_head_target_has_no_onehot_column():
    z, u, tgt, m, coef = _inputs()
    r = DR.distill_fwd_bwd(z, u, tgt, m, OFF, coef, 0.0, 1.0, 0.1)
    o, n = OFF[3], SIZES[3]
    p = torch.softmax(z[1, o:o + n], -1)
    assert torch.allclose(r['dlogits'][1, o:o + n], coef[3] * m[1, 3] * (p - 0.1 / n), atol=1e-14)


def test_alpha0_eps0_is_row_ref_cross_entropy():
    z, u, tgt, m, coef = _inputs(seed=3)
    for teacher in (None, u):
        r = DR.distill_fwd_bwd(z, teacher, tgt, m, OFF, coef, 0.0, 1.0, 0.0)
        k = R.ce_fwd_bwd(z, tgt, m, OFF, coef)
        assert torch.equal(r['hard'], k['ce']) and torch.equal(r['loss'], k['ce']) and torch.equal(r['argmax'], k['argmax'])
        assert torch.equal(r['terms'][:3], k['terms']) and torch.equal(r['terms'][3], k['terms'][0])
        assert torch.equal(r['dlogits'], k['dlogits']) and torch.equal(r['gscale'], k['gscale'])
    assert float(DR.distill_fwd_bwd(z, None, tgt, m, OFF, coef)['kl'].abs().max()) == 0.0


@pytest.mark.parametrize('dt', [torch.float64, torch.float32])
@pytest.mark.parametrize('tau', [1.0, 2.0, 0.5])
def test_teacher_equals_student_has_no_kl_and_no_soft_gradient(dt, tau):
    z, _, tgt, m, coef = _inputs(seed=5)
    z, m, coef = z.to(dt), m.to(dt), coef.to(dt)
    soft = DR.distill_fwd_bwd(z, z.clone(), tgt, m, OFF, coef, 1.0, tau, 0.0)
    assert float(soft['kl'].abs().max()) == 0.0 and float(soft['dlogits'].abs().max()) == 0.0
    half = DR.distill_fwd_bwd(z, z.clone(), tgt, m, OFF, coef, 0.5, tau, 0.0)
    hard = DR.distill_fwd_bwd(z, None, tgt, m, OFF, coef, 0.0, 1.0, 0.0)
    assert torch.equal(half['dlogits'], 0.5 * hard['dlogits'])


def test_row_map_is_a_gather():
    z, u, tgt, m, coef = _inputs(seed=7)
    T = z.shape[0]
    big = torch.full((2 * T, OFF[8]), float('nan'), dtype=torch.float64)
    rows = torch.randperm(2 * T, generator=torch.Generator().manual_seed(1))[:T]
    big[rows] = u
    a = DR.distill_fwd_bwd(z, big, tgt, m, OFF, coef, 0.5, 2.0, 0.0, t_row=rows.int())
    b = DR.distill_fwd_bwd(z, u, tgt, m, OFF, coef, 0.5, 2.0, 0.0)
    assert torch.equal(a['dlogits'], b['dlogits']) and torch.equal(a['terms'], b['terms']) and bool(torch.isfinite(a['terms']).all())


# ---------------------------------------------------------------- command line
def test_flags_of_both_trainers():
    from pianobart_amd.finetune_generation import get_args_generation
    from pianobart_amd.pretrain import get_args_pretrain
    for parse in (get_args_pretrain, get_args_generation):
        a = parse([])
        assert a.distill_from is None and a.distill_alpha == 0.5 and a.distill_temperature == 2.0 and a.label_smoothing == 0.0
        assert a.teacher_precision == 'bf16' and (a.teacher_hs, a.teacher_layers, a.teacher_ffn_dims, a.teacher_heads) == (1024, 8, 2048, 8)
        a = parse(['--distill_from', 'teacher.ckpt', '--teacher_hs', '512', '--teacher_layers', '4', '--teacher_ffn_dims', '1024', '--teacher_heads', '4',
                   '--teacher_precision', 'fp32', '--distill_alpha', '0.3', '--distill_temperature', '4', '--label_smoothing', '0.1', '--accum_steps', '2',
                   '--augment', 'pitch=-2:2'])
        assert a.distill_from == 'teacher.ckpt' and (a.teacher_hs, a.teacher_layers, a.teacher_ffn_dims, a.teacher_heads) == (512, 4, 1024, 4)
        assert a.teacher_precision == 'fp32' and a.distill_alpha == 0.3 and a.distill_temperature == 4.0 and a.label_smoothing == 0.1
        assert a.accum_steps == 2 and a.augment == 'pitch=-2:2'
        with pytest.raises(SystemExit):
            parse(['--teacher_precision', 'fp16'])


def test_from_args_without_a_teacher_and_bad_scalars():
    from pianobart_amd import distill
    from pianobart_amd._lib import PBError
    from pianobart_amd.pretrain import get_args_pretrain
    e2w, w2e = load_vocab()
    assert distill.from_args(get_args_pretrain([]), e2w, w2e) == (None, 0.0)
    plan, eps = distill.from_args(get_args_pretrain(['--label_smoothing', '0.1']), e2w, w2e)
    assert plan is None and eps == 0.1 and distill.step_kwargs(plan, eps) == {'smooth': 0.1} and distill.step_kwargs(None, 0.0) == {}
    for flags, word in ((['--label_smoothing', '1.0'], 'label_smoothing'), (['--distill_from', 'x', '--distill_alpha', '1.5'], 'distill_alpha'),
                        (['--distill_from', 'x', '--distill_temperature', '0'], 'distill_temperature')):
        with pytest.raises(PBError, match=word):
            distill.from_args(get_args_pretrain(flags), e2w, w2e)


# ---------------------------------------------------------------- teacher checkpoints
KW = dict(hs=64, layers=1, ffn_dims=128, heads=2)


def _tiny_lm(seed=0):
    from pianobart_amd.model import BartConfig, PianoBart, PianoBartLM
    e2w, w2e = load_vocab()
    torch.manual_seed(seed)
    cfg = BartConfig(max_position_embeddings=32, d_model=64, encoder_layers=1, decoder_layers=1, encoder_ffn_dim=128, decoder_ffn_dim=128,
                     encoder_attention_heads=2, decoder_attention_heads=2)
    return PianoBartLM(PianoBart(cfg, e2w, w2e, precision='fp32')), e2w, w2e


def _same(model, ref):
    a, b = model.state_dict(), ref.state_dict()
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def test_load_teacher_accepts_a_generation_checkpoint(tmp_path):
    from pianobart_amd import distill
    ref, e2w, w2e = _tiny_lm(1)
    path = str(tmp_path / 'gen.ckpt')
    torch.save({'epoch': 1, 'state_dict': ref.state_dict(), 'optimizer': {'lr': 1e-5}}, path)       # GenerationTrainer.save_checkpoint's keys
    t = distill.load_teacher(path, e2w, w2e, precision='fp32', **KW)
    assert _same(t, ref) and not t.training and not any(p.requires_grad for p in t.parameters())
    assert t.pianobart.bartConfig.max_position_embeddings == 32 and t.pianobart.precision == 'fp32'
    # saved from an nn.DataParallel wrapper: every key carries 'module.'
    torch.save({'state_dict': {'module.' + k: v for k, v in ref.state_dict().items()}}, path)
    assert _same(distill.load_teacher(path, e2w, w2e, precision='fp32', **KW), ref)
    plan = distill.Distill(t, 0.25, 3.0)
    assert plan.teacher is t._get_engine() and plan.teacher.mlm is t.mask_lm and (plan.alpha, plan.tau) == (0.25, 3.0)


def test_load_teacher_accepts_this_projects_pretrain_checkpoint(tmp_path):
    from pianobart_amd import distill
    ref, e2w, w2e = _tiny_lm(2)
    path = str(tmp_path / 'pre.ckpt')
    opt = {'step': 3, 'exp_avg': {}, 'exp_avg_sq': {}, 'lr': 2e-5, 'mask_lm': ref.mask_lm.state_dict()}  # Pretrainer.save_checkpoint: the heads travel here
    torch.save({'epoch': 1, 'state_dict': ref.pianobart.state_dict(), 'best_acc': 0.0, 'optimizer': opt}, path)
    assert _same(distill.load_teacher(path, e2w, w2e, precision='fp32', **KW), ref)


def test_load_teacher_refuses_a_headless_checkpoint_by_name(tmp_path):
    from pianobart_amd import distill
    from pianobart_amd._lib import PBError
    ref, e2w, w2e = _tiny_lm(3)
    path = str(tmp_path / 'reference_pretrain.ckpt')
    torch.save({'epoch': 1, 'state_dict': ref.pianobart.state_dict(), 'optimizer': {'state': {}, 'param_groups': []}}, path)   # torch's optimizer.state_dict()
    with pytest.raises(PBError, match=r'reference_pretrain\.ckpt has no LM heads.*no logits to distill'):
        distill.load_teacher(path, e2w, w2e, precision='fp32', **KW)
    torch.save({'epoch': 1, 'state_dict': ref.state_dict()}, path)
    with pytest.raises(PBError, match='does not fit a teacher of --teacher_hs 128'):
        distill.load_teacher(path, e2w, w2e, precision='fp32', hs=128, layers=1, ffn_dims=128, heads=2)


# ---------------------------------------------------------------- ABI
def test_header_declares_and_library_exports_the_new_symbols():
    from pianobart_amd import _lib
    decls = _lib.parse_header()
    assert len(decls['pb_distill_fwd_bwd'][1]) == 19 and decls['pb_distill_fwd_bwd'][1][15:18] == [ctypes.c_float] * 3
    assert decls['pb_distill_partials_floats'] == (ctypes.c_int64, [])
    if not os.path.exists(_lib.LIB_PATH):
        from pianobart_amd.build import build
        build(verbose=False)
    dll = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(dll, 'pb_distill_fwd_bwd') and hasattr(dll, 'pb_distill_partials_floats')
    assert _lib.LIB.query('pb_abi_version') == 10
    assert _lib.LIB.query('pb_distill_partials_floats') == 2048 * 40
