"""Teacher-forced scoring (pb_token_scores, pb_seq_scores, Engine.score, PianoBartLM.score, eval_generation --score / --pick best).

Bounds and where they come from:
  * kernel against float64 on given logits: 1e-4 absolute on logp and entropy (the project's fp32 bar; an f32 max-subtracted evaluation
    over at most 262 columns with |x - max| <= 160 is off by under 3e-5), rank exact.
  * sequence sums against float64 sums of the per-token outputs: 1e-6 relative.
  * against the pinned loss (pb_ce_fwd_bwd inside loss_and_grads(train=False) on the same decoder inputs): 1e-5 relative per head, hits
    exact. The comparison run hands loss_and_grads an argmax_out buffer: that keeps its forward on the dense rows, the schedule Engine.score
    runs, so both kernels read the same logits.
  * against the oracle: the metric of test_model_gpu.py::test_g1_forward_golden (max|a - b| / max|b|) with twice its bound per
    precision (1e-4 fp32, 2.5e-2 bf16): logp is a difference of two quantities that are each inside the logits bound.
"""
import os

import numpy as np
import pytest
import torch

from tests.golden_util import synth_octuple_batch

SEG = [0, 262, 396, 531, 793, 927, 965, 1225, 1280]
N_SEG = [SEG[i + 1] - SEG[i] for i in range(8)]
G1_LOGITS_TOL = {'fp32': 1e-4, 'bf16': 2.5e-2}            # tests/test_model_gpu.py::test_g1_forward_golden
gpu = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


# ---------------------------------------------------------------------------------------------------- kernel inputs and float64 reference
def _kernel_case(T):
    """T rows of N(0, 4) logits followed by three hand-made rows; targets in range; mask 0 at the first and the last of the T rows, the
    targets under the zeros set to 32767. Returns (logits f32 (T + 3, 1280), target int16 (T + 3, 8), mask f32 (T + 3,))."""
    g = torch.Generator().manual_seed(1000 + T)
    R = T + 3
    x = 2.0 * torch.randn(R, 1280, generator=g)
    tgt = torch.stack([torch.randint(0, n, (R,), generator=g) for n in N_SEG], 1)
    x[T] = 0.0
    for i in range(8):
        x[T, SEG[i]:SEG[i + 1]] = 1.5 + i                   # every logit of a segment equal: all ties
        x[T + 1, SEG[i]:SEG[i + 1]] = -80.0                 # +80 spike at column 0, -80 elsewhere
        x[T + 1, SEG[i]] = 80.0
        tgt[T + 2, i] = N_SEG[i] - 1                        # target = the last column of every segment
    tgt[T + 1, ::2] = 0                                     # the spike itself on the even heads, a -80 column on the odd ones
    tgt[T + 1, 1::2] = torch.tensor([n - 1 for n in N_SEG[1::2]])
    tgt[T, 3] = 0                                           # first of the ties: rank 0
    mask = torch.ones(R)
    mask[0] = 0
    mask[T - 1] = 0
    tgt = tgt.to(torch.int16)
    tgt[mask == 0] = 32767
    return x, tgt, mask


def _reference(x, tgt, mask):
    """float64 logp / entropy and the numpy rank count, (R, 8) each, with 0 / 0 / -1 on masked rows."""
    R = x.shape[0]
    x64 = x.double()
    logp, ent, rank = torch.zeros(R, 8, dtype=torch.double), torch.zeros(R, 8, dtype=torch.double), -np.ones((R, 8), dtype=np.int64)
    xn = x.numpy()
    for i in range(8):
        lsm = torch.log_softmax(x64[:, SEG[i]:SEG[i + 1]], dim=-1)
        p = lsm.exp()
        e = -torch.where(p > 0, p * lsm, torch.zeros_like(p)).sum(-1)
        for r in range(R):
            if mask[r] == 0:
                continue
            t = int(tgt[r, i])
            logp[r, i] = lsm[r, t]
            ent[r, i] = e[r]
            seg = xn[r, SEG[i]:SEG[i + 1]]
            rank[r, i] = int((seg > seg[t]).sum() + (seg[:t] == seg[t]).sum())
    return logp, ent, rank


@pytest.mark.parametrize('T', [1, 5, 67])
def test_float64_reference_is_sound_on_the_hand_made_rows(T):
    """No GPU: the reference of the kernel test is finite everywhere and gives what the hand-made rows must give."""
    x, tgt, mask = _kernel_case(T)
    logp, ent, rank = _reference(x, tgt, mask)
    assert torch.isfinite(logp).all() and torch.isfinite(ent).all()
    for i in range(8):
        assert abs(float(ent[T, i]) - np.log(N_SEG[i])) < 1e-12 and abs(float(logp[T, i]) + np.log(N_SEG[i])) < 1e-12      # uniform
        assert rank[T, i] == int(tgt[T, i])                                                                                # ties: lower indices beat
        assert 0 <= float(ent[T + 1, i]) < 1e-60                                                                           # spike: ~0, not NaN
        assert rank[T + 1, i] == (0 if i % 2 == 0 else N_SEG[i] - 1)
        assert abs(float(logp[T + 1, i]) - (0.0 if i % 2 == 0 else -160.0)) < 1e-12
    assert rank[T, 3] == 0
    live = mask != 0
    assert (rank[live.numpy()] >= 0).all() and (ent[live] >= 0).all() and (logp[live] <= 0).all()


def _run_kernel(x, tgt, mask, with_extras=True):
    from pianobart_amd import ops
    R = x.shape[0]
    xd, td, md = x.cuda(), tgt.cuda(), mask.cuda()
    logp = torch.full((R, 8), 7.0, device='cuda')
    ent = torch.full((R, 8), 7.0, device='cuda') if with_extras else None
    rank = torch.full((R, 8), 7, dtype=torch.int16, device='cuda') if with_extras else None
    ops.token_scores(xd, td, md, logp, ent, rank)
    torch.cuda.synchronize()
    return logp, ent, rank


@gpu
@pytest.mark.parametrize('T', [1, 5, 67])
def test_token_scores_against_float64(T):
    _need_gpu()
    from pianobart_amd import ops
    from pianobart_amd._lib import LIB
    x, tgt, mask = _kernel_case(T)
    ref_lp, ref_en, ref_rk = _reference(x, tgt, mask)
    logp, ent, rank = _run_kernel(x, tgt, mask)
    logp_c, ent_c, rank_c = logp.cpu(), ent.cpu(), rank.cpu()
    dead = mask == 0
    assert int(dead.sum()) == (1 if T == 1 else 2)
    assert (logp_c[dead] == 0).all() and (ent_c[dead] == 0).all() and (rank_c[dead] == -1).all()          # exactly 0 / 0 / -1
    e_lp, e_en = float((logp_c.double() - ref_lp).abs().max()), float((ent_c.double() - ref_en).abs().max())
    print('token_scores T=%d: max |logp - f64| = %.3e, max |entropy - f64| = %.3e' % (T, e_lp, e_en))
    assert e_lp < 1e-4 and e_en < 1e-4
    assert not torch.isnan(ent_c).any()
    assert np.array_equal(rank_c.numpy().astype(np.int64), ref_rk)
    # logp alone (entropy and rank NULL, the kernel's second instantiation): the same values, exact zeros on the masked rows
    lp_only, _, _ = _run_kernel(x, tgt, mask, with_extras=False)
    assert float((lp_only.cpu().double() - ref_lp).abs().max()) < 1e-4 and (lp_only.cpu()[dead] == 0).all()
    # rank == 0 iff the argmax of pb_ce_fwd_bwd on the same inputs is the target
    R = x.shape[0]
    safe = tgt.clone()
    safe[dead] = 0
    am = torch.full((R, 8), -5, dtype=torch.int16, device='cuda')
    sums = torch.zeros(24, device='cuda')
    partials = torch.empty(int(LIB.query('pb_ce_partials_floats')), device='cuda')
    ops.ce_fwd_bwd(x.cuda(), safe.cuda(), mask[:, None].repeat(1, 8).contiguous().cuda(), sums, partials, None, None, am)
    am = am.cpu()
    live = ~dead
    assert torch.equal(rank_c[live] == 0, am[live] == tgt[live])
    assert abs(float(sums[16:24].sum()) - float((rank_c[live] == 0).sum())) == 0


@gpu
def test_token_scores_beyond_one_pass_of_the_grid():
    """More rows than the grid has waves (4 x 4096): the row loop's second trip, against float64 on the device."""
    _need_gpu()
    from pianobart_amd import ops
    R = 4 * 4096 + 9
    g = torch.Generator(device='cuda').manual_seed(5)
    x = 2.0 * torch.randn(R, 1280, generator=g, device='cuda')
    tgt = torch.stack([torch.randint(0, n, (R,), generator=g, device='cuda') for n in N_SEG], 1)
    mask = (torch.rand(R, generator=g, device='cuda') < 0.9).float()
    logp, ent = torch.empty(R, 8, device='cuda'), torch.empty(R, 8, device='cuda')
    rank = torch.empty(R, 8, dtype=torch.int16, device='cuda')
    ops.token_scores(x, tgt.to(torch.int16), mask, logp, ent, rank)
    for i in range(8):
        seg = x[:, SEG[i]:SEG[i + 1]].double()
        lsm = torch.log_softmax(seg, -1)
        want = lsm.gather(1, tgt[:, i:i + 1])[:, 0] * mask
        assert float((logp[:, i].double() - want).abs().max()) < 1e-4
        e = -(lsm.exp() * lsm).sum(-1) * mask
        assert float((ent[:, i].double() - e).abs().max()) < 1e-4
        xt = seg.gather(1, tgt[:, i:i + 1])
        col = torch.arange(seg.shape[1], device='cuda')[None]
        rk = ((seg > xt) | ((seg == xt) & (col < tgt[:, i:i + 1]))).sum(1)
        assert torch.equal(rank[:, i].long(), torch.where(mask != 0, rk, torch.full_like(rk, -1)))


@gpu
def test_seq_scores_sums():
    _need_gpu()
    from pianobart_amd import ops
    B, S = 3, 40
    length, start = [40, 17, 0], [0, 5, 0]
    g = torch.Generator().manual_seed(77)
    x = (2.0 * torch.randn(B * S, 1280, generator=g)).cuda()
    tgt = torch.stack([torch.randint(0, n, (B * S,), generator=g) for n in N_SEG], 1).to(torch.int16).cuda()
    x[3, :262] = 9.0                                       # some certain hits: the target is the first of a tie at the maximum
    tgt[3, 0] = 0
    pos = torch.arange(S)[None]
    mask = ((pos >= torch.tensor(start)[:, None]) & (pos < torch.tensor(length)[:, None])).float().cuda()
    logp, ent = torch.empty(B * S, 8, device='cuda'), torch.empty(B * S, 8, device='cuda')
    rank = torch.empty(B * S, 8, dtype=torch.int16, device='cuda')
    ops.token_scores(x, tgt, mask.view(-1), logp, ent, rank)
    outs = []
    for _ in range(2):
        out = torch.full((B, 4, 8), 3.0, device='cuda')
        ops.seq_scores(logp, ent, rank, mask, out)
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1])                   # two launches: the same bits
    out = outs[0].double()
    m = mask.cpu().double()[:, :, None]
    want = [(m * logp.cpu().double().view(B, S, 8)).sum(1), (m * ent.cpu().double().view(B, S, 8)).sum(1),
            (m * (rank.cpu().view(B, S, 8) == 0).double()).sum(1)]
    for plane, w in enumerate(want):
        err = float(((out[:, plane] - w).abs() / w.abs().clamp(min=1e-30)).max()) if float(w.abs().max()) > 0 else 0.0
        print('seq_scores plane %d: max rel err %.3e' % (plane, err))
        assert torch.allclose(out[:, plane], w, rtol=1e-6, atol=0)
    assert float(want[2].sum()) >= 1
    assert torch.equal(outs[0][:, 3], torch.tensor([40.0, 12.0, 0.0])[:, None].repeat(1, 8))
    assert (outs[0][2] == 0).all()


# ---------------------------------------------------------------------------------------------------- the engine on the small model
_MODELS = {}


def _small(precision):
    """d = 256, 2 layers, 4 heads, S = 40 (the _lm shapes of tests/test_samples_per_prompt_gpu.py), three pieces and their scores, once."""
    if precision not in _MODELS:
        from tests.test_generate_batch_gpu import _lm, _prompts
        S = 40
        m = _lm(S, 256, 2, 512, 4, 51, precision)
        enc, emask = _prompts(3, S, seed=300)
        piece = synth_octuple_batch(3, S, seed=301, min_len=S // 2)[5].cuda()
        start = [0, 5, 0]
        r = m.score(enc, piece, emask, start=start, device_num=0)
        _MODELS[precision] = dict(m=m, enc=enc, emask=emask, piece=piece, start=start, r=r)
    return _MODELS[precision]


@gpu
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_score_against_the_pinned_loss(precision):
    _need_gpu()
    from pianobart_amd import ops
    from pianobart_amd.scoring import default_length
    c = _small(precision)
    m, enc, emask, piece, r = c['m'], c['enc'], c['emask'], c['piece'], c['r']
    B, S = piece.shape[:2]
    length = default_length(piece, 256)
    assert all(S // 2 <= n <= S for n in length)
    pos = torch.arange(S, device='cuda')[None]
    ln, st = torch.tensor(length, device='cuda')[:, None], torch.tensor(c['start'], device='cuda')[:, None]
    mask = ((pos >= st) & (pos < ln)).float()
    assert torch.equal(r.count, mask.sum(1)) and r.logp.shape == (B, S, 8) and r.rank.dtype == torch.int16
    assert (r.logp[mask == 0] == 0).all() and (r.entropy[mask == 0] == 0).all() and (r.rank[mask == 0] == -1).all()
    assert (r.rank[mask != 0] >= 0).all() and (r.logp[mask != 0] < 0).all()
    eng = m._get_engine()
    tgt16 = ops.ids_to_i16(piece)
    dec16 = torch.empty_like(tgt16)
    ops.shift_right(tgt16, eng.sos16, dec16, B, S)
    dmask = (pos < ln.clamp(min=1)).float().contiguous()
    am = torch.empty(B * S, 8, dtype=torch.int16, device='cuda')
    sums = eng.loss_and_grads(ops.ids_to_i16(enc), dec16, tgt16, mask[:, :, None].repeat(1, 1, 8).contiguous(), emask, dmask, train=False,
                              argmax_out=am).double().cpu()
    mine = -r.sum_logp.double().sum(0).cpu()
    rel = ((mine - sums[0:8]).abs() / sums[0:8].abs()).max()
    print('score vs pinned loss (%s): max rel %.3e' % (precision, float(rel)))
    assert float(rel) < 1e-5
    assert torch.equal(r.hits.double().sum(0).cpu(), sums[16:24])
    assert torch.equal(r.count.double().sum().cpu(), sums[8])


@gpu
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_score_against_the_oracle(precision):
    _need_gpu()
    from oracle import pianobart_oracle as O                # checker only
    from pianobart_amd.scoring import default_length
    from tests.test_generate_batch_gpu import E2W, W2E
    c = _small(precision)
    m, enc, emask, piece, r = c['m'], c['enc'].cpu(), c['emask'].cpu(), c['piece'].cpu(), c['r']
    B, S = piece.shape[:2]
    o = O.PianoBartLM(O.PianoBart(O.BartConfig(max_position_embeddings=S, d_model=256, encoder_layers=2, decoder_layers=2, encoder_ffn_dim=512,
                                               decoder_ffn_dim=512, encoder_attention_heads=4, decoder_attention_heads=4, dropout=0.0), E2W, W2E)).eval()
    o.load_state_dict(m.state_dict(), strict=True)
    length = torch.tensor(default_length(piece, 256))[:, None]
    pos = torch.arange(S)[None]
    mask = (pos >= torch.tensor(c['start'])[:, None]) & (pos < length)
    dmask = (pos < length.clamp(min=1)).float()
    with torch.no_grad():
        yo = torch.cat(o(enc, O.shift_right(piece, o.pianobart.sos_word_np), emask, dmask), -1).double()
    ref = torch.zeros(B, S, 8, dtype=torch.double)
    for i in range(8):
        ref[:, :, i] = torch.log_softmax(yo[:, :, SEG[i]:SEG[i + 1]], -1).gather(2, piece[:, :, i:i + 1])[:, :, 0]
    ref = ref * mask[:, :, None]
    err = float((r.logp.double().cpu() - ref).abs().max() / ref.abs().max())
    print('score logp vs oracle (%s): rel %.3e' % (precision, err))
    assert err < 2 * G1_LOGITS_TOL[precision]


@gpu
def test_score_raises_index_error_for_an_id_outside_its_table_only():
    _need_gpu()
    c = _small('bf16')
    piece = c['piece'].clone()
    piece[0, 3] = torch.tensor([256, 128, 129, 256, 128, 32, 254, 49], device='cuda') + 3          # an EOS row is a legal target
    c['m'].score(c['enc'], piece, c['emask'])
    piece[0, 3, 5] = 38                                     # head 5 has 38 classes
    with pytest.raises(IndexError):
        c['m'].score(c['enc'], piece, c['emask'])
    r = c['m'].score(c['enc'], c['piece'], c['emask'], start=c['start'], device_num=0)             # and the engine goes on working
    assert torch.allclose(r.logp, c['r'].logp, rtol=0, atol=1e-2) and torch.equal(r.count, c['r'].count)


# ---------------------------------------------------------------------------------------------------- end to end
@gpu
def test_score_of_generated_rows_counts_the_sampled_positions():
    _need_gpu()
    from pianobart_amd.scoring import default_length
    c = _small('bf16')
    m, enc, emask = c['m'], c['enc'], c['emask']
    counts, ks = [2, 1, 3], [0, 6, 0]
    prefix = synth_octuple_batch(3, 8, seed=11, min_len=8)[5][:, :6]                                # ordinary rows only
    y = m.generate_batch(enc, emask, seeds=list(range(20, 26)), max_new=12, decoder_prefix=prefix, prefix_len=ks, samples_per_prompt=counts,
                         device_num=0)
    own = torch.tensor([p for p, n in enumerate(counts) for _ in range(n)], device='cuda')
    k_rows = [ks[int(p)] for p in own]
    emitted = default_length(y, 256)
    assert all(k <= e <= k + 12 for k, e in zip(k_rows, emitted)) and max(e - k for k, e in zip(k_rows, emitted)) > 0
    r = m.score(enc[own], y, emask[own], start=k_rows)
    assert r.logp.device.type == 'cpu'
    assert r.count.tolist() == [float(e - k) for k, e in zip(k_rows, emitted)]
    for b, (k, e) in enumerate(zip(k_rows, emitted)):
        assert (r.rank[b, :k] == -1).all() and (r.rank[b, k:e] >= 0).all() and (r.rank[b, e:] == -1).all()


@gpu
def test_eval_generation_score_and_pick_best(tmp_path):
    _need_gpu()
    from pianobart_amd import eval_generation as EG
    from pianobart_amd.scoring import pick_best
    S, N, n = 40, 3, 3
    np.save(str(tmp_path / 'prompts.npy'), synth_octuple_batch(N, S, seed=5, min_len=S // 2)[5].numpy())
    base = ['--dataset_path', str(tmp_path), '--dataset_name', 'prompts.npy', '--max_seq_len', str(S), '--hs', '256', '--layers', '2',
            '--ffn_dims', '512', '--heads', '4', '--nopretrain', '--batch_size', '4', '--samples', str(n), '--seed', '0']

    def run(name, *extra):
        torch.manual_seed(0)                     # --nopretrain: the same random initialisation in every run
        out = str(tmp_path / name)
        EG.eval_generation(EG.get_args(base + ['--output', out] + list(extra)))
        return out

    plain = run('plain.npy')
    scored = run('scored.npy', '--score')
    assert open(plain, 'rb').read() == open(scored, 'rb').read()          # the generation file does not change under --score
    picked = run('picked.npy', '--score', '--pick', 'best')
    sc = np.load(str(tmp_path / 'picked_score.npy'))
    assert sc.shape == (N, n, 9) and sc.dtype == np.float32
    assert np.array_equal(sc, np.load(str(tmp_path / 'scored_score.npy')))
    gen = np.load(plain)
    assert gen.shape == (N, n, S, 8)
    emitted = (gen[..., 0] != 256).sum(-1)                                # unprimed rows: every emitted position is scored
    assert np.array_equal(sc[:, :, 8], emitted.astype(np.float32)) and (sc[:, :, :8][emitted > 0] < 0).all()
    best = pick_best(sc)
    y = np.load(picked)
    assert y.shape == (N, S, 8) and y.dtype == np.float32
    for i in range(N):
        assert np.array_equal(y[i], gen[i, best[i]]), i


@gpu
def test_eval_generation_score_dataset(tmp_path, capsys):
    _need_gpu()
    from pianobart_amd import eval_generation as EG
    S, N = 40, 3
    data = synth_octuple_batch(N, S, seed=6, min_len=S // 2)[5].numpy()
    np.save(str(tmp_path / 'pieces.npy'), data)
    out = str(tmp_path / 'unused.npy')
    torch.manual_seed(0)
    sc = EG.eval_generation(EG.get_args(['--dataset_path', str(tmp_path), '--dataset_name', 'pieces.npy', '--max_seq_len', str(S), '--hs', '256',
                                         '--layers', '2', '--ffn_dims', '512', '--heads', '4', '--nopretrain', '--batch_size', '2', '--seed', '0',
                                         '--output', out, '--prime', 'half', '--score_dataset']))
    assert not os.path.exists(out)                                        # only the score file is written
    saved = np.load(str(tmp_path / 'unused_score.npy'))
    assert saved.shape == (N, 9) and saved.dtype == np.float32 and np.array_equal(saved, sc)
    L = (data[:, :, 0] != 256).sum(1)
    assert np.array_equal(saved[:, 8], (L - L // 2).astype(np.float32))   # rows k_b .. L_b - 1 of every piece (its EOS row included)
    assert (saved[:, :8] < 0).all()
    text = capsys.readouterr().out
    assert 'LogP: ' in text and 'Hit: ' in text
