"""GPU: RegMean merging (csrc/pb_regmean.hip, merge.regmean_weights, python -m pianobart_amd.regmean, model_merge --method regmean_merging).

  * pb_gram_accum exactly: integer operands (|x| <= 4, every sum far below 2^24) against the int64 X^T X, both dtypes, at every edge of
    the 128-column tile (K = 128 / 130 / 264: 1, 3 and 6 tiles), the 64 / 32-row stage and the T split (one chunk up to T = 256, two from
    257, four at 1000), dense X and column slices of a wider buffer (16-byte loads and the scalar path); two batches equal their
    concatenation; G bitwise symmetric; guard bands around G and the workspace; two runs give equal bytes.
  * pb_gram_accum with real f32 values inside T 2^-24 sum_t |x_ti x_tj| of float64: what an f32 fma chain of T terms in any order keeps.
  * pb_regmean_scale bit for bit (one multiplication per element).
  * pb_chol_factor + pb_chol_solve: the normwise residual eta = ||S Z - R|| / (||S|| ||Z|| + ||R||) in float64 is at most 4 times the larger
    of the two CPU yardsticks on the same S, R (float32 inverse @ R, and LAPACK's float32 Cholesky): a different blocking and summation
    order at a few units of 2^-24. K on both sides of every 64-column block edge, K = 768 (two 512-column pieces of the trailing update).
  * a zero row and column: info = 1 + j; through merge_state_dicts a PBError that names the weight.
  * the whole merge of a 1 + 1 layer model against tests/regmean_ref.py in float64, held to 4 times the float32 recipe's own error.
  * the pass against float64 forward hooks on the oracle's classifier; the command lines end to end.
  * the reference's own recorded regmean_merging results on a toy classifier (tests/golden/g17_regmean.npz, read through the helpers of
    tests/test_regmean_cpu.py): merge_state_dicts per case and N, every solved weight within 4 times the recorded output's own distance from
    float64 (at least one float32 ulp), every averaged parameter equal to the recording bit for bit; q / k as one shared Gram tensor and as
    two copies; pb_gram_accum over the recorded activations, batch by batch and in one call, f32 and bf16, held to 4 times the recorded
    matrix's own figure; a 2-D-input layer cut to fewer rows than inputs is refused by name. Two deviations from the reference stay as they
    are: a sum that is not positive definite is refused where the reference inverts whatever it is given, and the pass gives
    encoder_linear.weight no Gram matrix (merge.regmean_pass prints it) -- the toy has no such layer, every Linear of it is solved."""
import copy
import os

import pytest
import torch

from tests import regmean_ref as R
from tests.test_regmean_cpu import CASE_IDS, GOLDEN_CASES, MARGIN, ULP, gram_figure, golden, golden_activations, golden_truth, rel_error

gpu = pytest.mark.gpu
TS = [1, 2, 33, 63, 64, 65, 255, 256, 257, 1000]
KS = [1, 7, 8, 31, 32, 33, 64, 65, 96, 128, 130, 264]
GUARD = 7.25


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


def _ints(T, K, g):
    return torch.randint(-4, 5, (T, K), generator=g)


def _place(X, dtype, layout):
    """X on the device as `dtype`: dense, or columns 8 .. of a buffer whose rows keep 16-byte alignment, or columns 3 .. of an odd-width one."""
    T, K = X.shape
    if layout == 'dense':
        return X.to(dtype).cuda()
    off, wide = (8, (K + 7) // 8 * 8 + 16) if layout == 'slice16' else (3, K + 11)
    buf = torch.full((T, wide), 3.0, dtype=dtype, device='cuda')            # what the slice must not read
    buf[:, off:off + K] = X.to(dtype).cuda()
    return buf[:, off:off + K]


def _guarded(rows, cols, pad=5):
    """(a (rows, cols) f32 view with a leading dimension of cols + 2 pad inside a buffer of GUARD, the buffer)."""
    buf = torch.full((rows + 2 * pad, cols + 2 * pad), GUARD, dtype=torch.float32, device='cuda')
    return buf[pad:pad + rows, pad:pad + cols], buf


def _guards_intact(buf, rows, cols, pad=5):
    probe = buf.clone()
    probe[pad:pad + rows, pad:pad + cols] = GUARD
    return bool((probe == GUARD).all())


# ---- pb_gram_accum ------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32], ids=['bf16', 'f32'])
@pytest.mark.parametrize('K', KS)
def test_gram_accum_is_exact_on_integers(K, dtype):
    _need_gpu()
    from pianobart_amd import ops
    from pianobart_amd._lib import LIB
    g = torch.Generator().manual_seed(K)
    G0 = _ints(K, K, g)
    G0 = G0 + G0.t()
    for T in TS:
        X1, X2 = _ints(T, K, g), _ints(T // 2 + 1, K, g)
        want = G0 + X1.t() @ X1
        want2 = want + X2.t() @ X2
        assert torch.equal(want2, G0 + torch.cat([X1, X2]).t() @ torch.cat([X1, X2]))
        first = None
        for layout in ('dense', 'slice16', 'slice3'):
            G, gbuf = _guarded(K, K)
            G.copy_(G0.float().cuda())
            nws = LIB.query('pb_gram_ws_bytes', T, K) // 4
            wbuf = torch.full((nws + 8,), GUARD, dtype=torch.float32, device='cuda')
            ops.gram_accum(G, _place(X1, dtype, layout), wbuf[4:4 + nws])
            got = G.cpu()
            assert torch.equal(got.long(), want), (T, layout)
            assert torch.equal(got, got.t())
            assert _guards_intact(gbuf, K, K) and bool((wbuf[:4] == GUARD).all()) and bool((wbuf[4 + nws:] == GUARD).all()), (T, layout)
            if first is None:
                first = got
            assert got.numpy().tobytes() == first.numpy().tobytes()        # run to run, layout to layout
            ops.gram_accum(G, _place(X2, dtype, layout))                   # a second batch of another T, the wrapper's own workspace
            assert torch.equal(G.cpu().long(), want2), (T, layout)


@gpu
def test_gram_accum_overwrites_the_upper_triangle():
    """The new G[i][j], j <= i, goes to (i, j) and (j, i): what the strict upper triangle held does not matter."""
    _need_gpu()
    from pianobart_amd import ops
    g = torch.Generator().manual_seed(1)
    K, T = 130, 70
    X, L0 = _ints(T, K, g), torch.tril(_ints(K, K, g))
    G = (L0 + torch.triu(torch.full((K, K), 1000), 1)).float().cuda()
    ops.gram_accum(G, X.float().cuda())
    low = L0 + torch.tril(X.t() @ X)
    assert torch.equal(G.cpu().long(), low + torch.tril(low, -1).t())


@gpu
def test_gram_accum_real_values_stay_inside_the_fma_chain_bound():
    _need_gpu()
    from pianobart_amd import ops
    T, K = 257, 65
    X = torch.randn(T, K, generator=torch.Generator().manual_seed(2))
    G = torch.zeros(K, K, device='cuda')
    ops.gram_accum(G, X.cuda())
    Xd = X.double()
    err = (G.cpu().double() - Xd.t() @ Xd).abs()
    bound = T * 2.0 ** -24 * (Xd.abs().t() @ Xd.abs())
    print('largest error over bound: %.3g' % float((err / bound).max()))
    assert bool((err <= bound).all())
    assert torch.equal(G, G.t())


# ---- pb_regmean_scale ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('ratio', [1.0, 0.9, 0.5, 0.0])
def test_scale_equals_the_float32_product(ratio):
    _need_gpu()
    from pianobart_amd import merge as M, ops
    for K in (1, 7, 65, 130):
        Gc = R.gram_inputs(K, 2 * K + 2, 1, K)[0]
        want = R.scale32(Gc, ratio)
        off, diag = M.regmean_factors(ratio)
        G, gbuf = _guarded(K, K)
        G.copy_(Gc.cuda())
        out, obuf = _guarded(K, K, pad=3)
        ops.regmean_scale(G, out, off, diag)
        assert torch.equal(out.cpu(), want) and torch.equal(G.cpu(), Gc) and _guards_intact(obuf, K, K, pad=3)
        ops.regmean_scale(G, G, off, diag)                                 # in place
        assert torch.equal(G.cpu(), want) and _guards_intact(gbuf, K, K)


# ---- factor and solve ---------------------------------------------------------------------------------------------------------------------
def _device_solve(S, Rm):
    """(Z, Z^T by the transpose kernel, info, the factor) with S and R inside guarded buffers (leading dimensions above K and nrhs)."""
    from pianobart_amd import ops
    K, nrhs = Rm.shape
    A, abuf = _guarded(K, K)
    Z, zbuf = _guarded(K, nrhs, pad=3)
    A.copy_(S.cuda())
    Z.copy_(Rm.cuda())
    info = torch.zeros(1, dtype=torch.int32, device='cuda')
    ops.chol_factor(A, info)
    ops.chol_solve(A, Z)
    Zt, tbuf = _guarded(nrhs, K, pad=2)
    ops.transpose_f32(Z, Zt)
    assert _guards_intact(abuf, K, K) and _guards_intact(zbuf, K, nrhs, pad=3) and _guards_intact(tbuf, nrhs, K, pad=2)
    return Z.cpu(), Zt.cpu(), int(info.item()), A.cpu()


def _check_solve(K, nrhs, T, ratio, seed):
    S, Rm = R.solve_case(K, nrhs, T, ratio, seed)
    Z, Zt, info, L = _device_solve(S, Rm)
    assert info == 0 and bool(torch.isfinite(Z).all())
    assert torch.equal(Zt, Z.t().contiguous())
    assert torch.equal(L, torch.tril(L))
    Z2, _, _, L2 = _device_solve(S, Rm)
    assert Z2.numpy().tobytes() == Z.numpy().tobytes() and L2.numpy().tobytes() == L.numpy().tobytes()
    e_dev = R.eta(S, Z, Rm)
    e_inv, e_chol = R.yardsticks(S, Rm)
    ratio_seen = e_dev / max(e_inv, e_chol)
    print('K %4d nrhs %4d ratio %.1f: eta device %.3g, inverse %.3g, LAPACK Cholesky %.3g (device / larger %.2f)' % (K, nrhs, ratio, e_dev, e_inv, e_chol, ratio_seen))
    assert e_dev <= 4 * max(e_inv, e_chol), (K, nrhs, ratio, e_dev, e_inv, e_chol)
    return ratio_seen


@gpu
@pytest.mark.parametrize('K', [1, 2, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 130, 257])
def test_factor_and_solve_match_the_cpu_yardsticks(K):
    _need_gpu()
    for ratio in (1.0, 0.9):
        for nrhs in (1, 7, 64, 65, 192):
            _check_solve(K, nrhs, max(4, 2 * K), ratio, 1000 * K + nrhs)


@gpu
def test_factor_and_solve_at_768():
    _need_gpu()
    _check_solve(768, 768, 2048, 1.0, 7)


@gpu
def test_a_zero_row_and_column_sets_info():
    """An input that is identically 0: row and column j of S are exactly 0, the pivot of column j is exactly 0."""
    _need_gpu()
    from pianobart_amd import ops
    K = 200
    S, _ = R.solve_case(K, 1, 2 * K, 1.0, 3)
    for j in (5, 100, K - 1):                                              # first block, an interior block, the last column
        A = S.clone()
        A[j, :] = 0
        A[:, j] = 0
        A = A.cuda()
        info = torch.zeros(1, dtype=torch.int32, device='cuda')
        ops.chol_factor(A, info)
        assert int(info.item()) == 1 + j
        ops.chol_factor(S.cuda(), info)                                    # a later clean matrix leaves the word alone
        assert int(info.item()) == 1 + j
    info = torch.zeros(1, dtype=torch.int32, device='cuda')
    ops.chol_factor(torch.full((1, 1), -1.0, device='cuda'), info)
    assert int(info.item()) == 1


# ---- the whole merge ------------------------------------------------------------------------------------------------------------------------
def _tiny_backbones(n_models):
    from pianobart_amd.model import BartConfig, PianoBart
    from tests.golden_util import load_vocab, randomize_params
    e2w, w2e = load_vocab()
    cfg = BartConfig(max_position_embeddings=64, d_model=64, encoder_layers=1, decoder_layers=1, encoder_ffn_dim=128, decoder_ffn_dim=128,
                     encoder_attention_heads=4, decoder_attention_heads=4)
    pre = PianoBart(cfg, e2w, w2e)
    randomize_params(pre, 5)
    g = torch.Generator().manual_seed(6)
    fts = []
    for _ in range(n_models):
        m = copy.deepcopy(pre)
        with torch.no_grad():
            for q in m.parameters():
                q.add_(torch.randn(q.shape, generator=g) * 0.01)
        fts.append(m.state_dict())
    return pre.state_dict(), fts


def _constructed_grams(sd, n_models, seed):
    """Per model {Linear weight name: Gram matrix}, shared as the pass shares them: q / k / v of a self-attention block one tensor, the
    decoder's cross-attention k / v one tensor; encoder_linear.weight has none."""
    groups = {}
    for name, t in sd.items():
        if not name.endswith('.weight') or t.dim() != 2 or '.layers.' not in name or 'layer_norm' in name:
            continue
        block, leaf = name.rsplit('.', 2)[0], name.rsplit('.', 2)[1]
        if leaf in ('q_proj', 'k_proj', 'v_proj') and block.endswith('self_attn'):
            key = block + '.qkv'
        elif leaf in ('k_proj', 'v_proj'):
            key = 'cross.kv'
        else:
            key = name
        groups.setdefault(key, []).append(name)
    assert len(groups) == 4 * 1 + 6 * 1 + 1
    out = [dict() for _ in range(n_models)]
    for i, (key, names) in enumerate(sorted(groups.items())):
        K = sd[names[0]].shape[1]
        for m, G in enumerate(R.gram_inputs(K, 2 * K, n_models, seed + 17 * i)):
            for name in names:
                out[m][name] = G
    return out, groups


@gpu
@pytest.mark.parametrize('ratio', [1.0, 0.9])
@pytest.mark.parametrize('N', [2, 3])
def test_merge_matches_the_float64_restatement(N, ratio):
    _need_gpu()
    from pianobart_amd import merge as M
    pre, fts = _tiny_backbones(N)
    grams, groups = _constructed_grams(pre, N, 40 + N)
    exclude = [r'.*layernorm_embedding.*']
    got = M.merge_state_dicts(pre, fts, method='regmean_merging', regmean_weights=grams, reduce_non_diagonal_ratio=ratio, exclude=exclude)
    average = M.merge_state_dicts(pre, fts, method='average_merging', exclude=exclude)
    assert list(got) == list(pre)
    worst = 0.0
    for name in pre:
        if name in grams[0]:
            Ws, Gs = [f[name] for f in fts], [g[name] for g in grams]
            W64 = R.merge64(Ws, Gs, ratio)
            e_ref = float(torch.linalg.norm(R.merge32_recipe(Ws, Gs, ratio).double() - W64) / torch.linalg.norm(W64))
            e_dev = float(torch.linalg.norm(got[name].double() - W64) / torch.linalg.norm(W64))
            print('%-55s device %.3g, float32 recipe %.3g' % (name, e_dev, e_ref))
            assert e_dev <= 4 * e_ref + 8 * 2.0 ** -24, (name, e_dev, e_ref)
            assert not torch.equal(got[name], average[name])
            worst = max(worst, e_dev)
        elif 'layernorm_embedding' in name:
            assert torch.equal(got[name], pre[name])
        else:
            assert torch.equal(got[name], average[name]), name
    assert worst > 0 and not torch.equal(got['encoder_linear.weight'], pre['encoder_linear.weight'])
    _, alias = M.state_dict_layout(pre, exclude)
    tied = [names for names in alias.values() if len(names) > 1]
    assert tied and all(got[n].data_ptr() == got[names[0]].data_ptr() for names in tied for n in names)


@gpu
def test_merge_names_the_weight_whose_gram_sum_is_not_positive_definite():
    _need_gpu()
    from pianobart_amd import merge as M
    from pianobart_amd._lib import PBError
    pre, fts = _tiny_backbones(2)
    grams, _ = _constructed_grams(pre, 2, 50)
    name = 'bart.decoder.layers.0.fc2.weight'
    for m in range(2):
        G = grams[m][name].clone()
        G[77, :] = 0
        G[:, 77] = 0
        grams[m][name] = G
    with pytest.raises(PBError, match=r'bart\.decoder\.layers\.0\.fc2\.weight.*not positive definite.*column 77'):
        M.merge_state_dicts(pre, fts, method='regmean_merging', regmean_weights=grams)


# ---- the pass -----------------------------------------------------------------------------------------------------------------------------
_ORACLE = {}


def _oracle_grams(tag):
    """The reference's loop (merging_methods.py:330-405) on the oracle's classifier in float64: a forward hook on every backbone nn.Linear
    accumulates X^T X over x.reshape(-1, K); the sums are divided by the rows seen."""
    if tag in _ORACLE:
        return _ORACLE[tag]
    from oracle import pianobart_oracle as O
    from tests.test_finetune_heads import _build
    from tests.test_fisher_gpu import BATCH, N_EX, _batches, _data
    m = _build(O, O.BartConfig, O.PianoBart, tag).double()
    pad = m.pianobart.bar_pad_word
    sums, rows, handles = {}, {}, []

    def hook(name):
        def fn(module, inputs, output):
            x = inputs[0].detach().reshape(-1, inputs[0].shape[-1])
            sums[name] = sums.get(name, 0) + x.t() @ x
            rows[name] = rows.get(name, 0) + x.shape[0]
        return fn

    for name, mod in m.pianobart.named_modules():
        if isinstance(mod, torch.nn.Linear):
            handles.append(mod.register_forward_hook(hook(name + '.weight')))
    X, y = _data(tag)
    counted = 0
    with torch.no_grad():
        for x, yb in _batches(X, y):
            if counted >= N_EX:
                break
            attn = (x[:, :, 0] != pad).double()
            if tag == 'seq':
                m(input_ids_encoder=x, encoder_attention_mask=attn)
            else:
                y_shift = torch.zeros_like(yb) + 7
                y_shift[:, 1:] = yb[:, :-1]
                attn_shift = torch.zeros_like(attn)
                attn_shift[:, 1:] = attn[:, :-1]
                attn_shift[:, 0] = attn[:, 0]
                m(input_ids_encoder=x, input_ids_decoder=y_shift, encoder_attention_mask=attn, decoder_attention_mask=attn_shift)
            counted += x.shape[0]
    for h in handles:
        h.remove()
    assert counted == N_EX
    _ORACLE[tag] = ({k: v / rows[k] for k, v in sums.items()}, rows)
    return _ORACLE[tag]


@gpu
@pytest.mark.parametrize('precision,tol_grad', [('fp32', 2e-3), ('bf16x3', 2e-3), ('bf16', 2e-1)])
@pytest.mark.parametrize('tag', ['seq', 'tok8'])
def test_regmean_weights_match_the_oracle(tag, precision, tol_grad):
    """A Gram entry is a sum of products of two activations, and those activations are what the weight gradients dY^T X that
    test_heads_match_reference_golden holds to tol_grad are made of: (x + dx)(y + dy) - x y is held to 2 tol_grad + tol_grad^2 (largest
    error over largest entry, per matrix). A loose bound: it catches a wrong buffer, a wrong row count or a missed layer."""
    _need_gpu()
    from pianobart_amd import merge as MG, model as M
    from tests.test_finetune_heads import L as LAYERS, S, _build
    from tests.test_fisher_gpu import N_EX, _batches, _data
    ref, ref_rows = _oracle_grams(tag)
    m = _build(M, M.BartConfig, M.PianoBart, tag, precision=precision).cuda()
    for x in m.modules():
        if isinstance(x, torch.nn.Dropout):
            x.p = 0.1
    m.eval()
    eng = m.pianobart._get_engine()
    eng.bind(torch.device('cuda', torch.cuda.current_device()))
    eng.p_drop = 0.1
    before = eng.P32.clone()
    heads_before = {k: p.detach().clone() for k, p in m.named_parameters() if not k.startswith('pianobart.')}
    X, y = _data(tag)
    W, num_rows, counted = MG.regmean_pass(m, _batches(X, y), N_EX, tag == 'seq', 'cuda')
    assert counted == N_EX and num_rows == N_EX * S                        # batches of 4, 4 and 2 examples: the actual sizes count (Fisher's pass counts 12)
    assert torch.equal(before, eng.P32) and all(torch.equal(v, dict(m.named_parameters())[k].detach()) for k, v in heads_before.items())
    assert eng.p_drop == 0.1 and not m.training and all(x.p == 0.1 for x in m.modules() if isinstance(x, torch.nn.Dropout))
    assert all(p.grad is None for p in m.parameters())
    distinct = {v.data_ptr() for v in W.values()}
    assert len(distinct) == 4 * LAYERS + 6 * LAYERS + 1 and len(W) == 6 * LAYERS + 10 * LAYERS
    own = m.pianobart.state_dict()
    assert all(k in own and k.endswith('.weight') and own[k].dim() == 2 and v.shape == (own[k].shape[1],) * 2 for k, v in W.items())
    assert 'encoder_linear.weight' not in W and not any(k.startswith(('classifier', 'attention')) or 'decoder_emb' in k or 'decoder_linear' in k for k in W)
    for side in ('encoder', 'decoder'):
        for l in range(LAYERS):
            p = 'bart.%s.layers.%d.self_attn.' % (side, l)
            assert W[p + 'q_proj.weight'] is W[p + 'k_proj.weight'] is W[p + 'v_proj.weight']
    cross = [W['bart.decoder.layers.%d.encoder_attn.%s_proj.weight' % (l, kv)] for l in range(LAYERS) for kv in 'kv']
    assert all(c is cross[0] for c in cross)
    assert W['bart.decoder.layers.0.encoder_attn.q_proj.weight'] is not cross[0]
    bound = 2 * tol_grad + tol_grad ** 2
    for name, G in W.items():
        want = ref[name]
        assert ref_rows[name] == num_rows
        got = G.double().cpu()
        assert torch.equal(G, G.t()) and bool(torch.isfinite(got).all())
        r = float((got - want).abs().max() / want.abs().max())
        print('%s %s %-60s %.3g' % (tag, precision, name, r))
        assert r < bound, (name, r)


# ---- the command lines --------------------------------------------------------------------------------------------------------------------
@gpu
def test_regmean_and_model_merge_command_lines(tmp_path, capsys):
    _need_gpu()
    import pickle
    from pianobart_amd._lib import PBError
    from pianobart_amd.merge import merge_state_dicts
    from pianobart_amd.model import BartConfig, PianoBart, SequenceClassification
    from pianobart_amd.model_merge import model_merge
    from pianobart_amd.regmean import regmean
    from tests.golden_util import load_vocab, randomize_params
    from tests.test_finetune_heads import _write_finetune_sets
    e2w, w2e = load_vocab()
    pickle.dump((e2w, w2e), open(tmp_path / 'dict.pkl', 'wb'))
    root = str(tmp_path / 'data')
    os.makedirs(root)
    _write_finetune_sets(root, 'Pianist8', True)                           # 4 training examples of length 64: 256 rows for K = 64 and 128
    shape = dict(max_seq_len=64, hs=64, layers=1, ffn_dims=128, heads=4)
    cfg = BartConfig(max_position_embeddings=64, d_model=64, encoder_layers=1, decoder_layers=1, encoder_ffn_dim=128, decoder_ffn_dim=128,
                     encoder_attention_heads=4, decoder_attention_heads=4)
    pre = PianoBart(cfg, e2w, w2e)
    randomize_params(pre, 5)
    torch.save({'state_dict': pre.state_dict()}, str(tmp_path / 'pre.ckpt'))
    g = torch.Generator().manual_seed(6)
    fts = []
    for i in range(2):
        m = SequenceClassification(copy.deepcopy(pre), 8, 64)
        randomize_params(m.attention, 7 + i)
        randomize_params(m.classifier, 9 + i)
        with torch.no_grad():
            for q in m.pianobart.parameters():
                q.add_(torch.randn(q.shape, generator=g) * 0.01)
        torch.save({'state_dict': m.state_dict(), 'epoch': 1}, str(tmp_path / ('ft%d.ckpt' % i)))
        fts.append(m)
    flags = [x for k, v in shape.items() for x in ('--' + k, str(v))] + ['--dict_file', str(tmp_path / 'dict.pkl')]
    for i in range(2):
        regmean(flags + ['--ckpt', str(tmp_path / ('ft%d.ckpt' % i)), '--task', 'composer', '--dataset', 'Pianist8', '--dataroot', root, '--num_examples', '3',
                         '--batch_size', '2', '--precision', 'fp32', '--output', str(tmp_path / ('ft%d.regmean.pt' % i))])
    assert 'encoder_linear.weight has no Gram matrix' in capsys.readouterr().out
    files = [torch.load(str(tmp_path / ('ft%d.regmean.pt' % i)), weights_only=False) for i in range(2)]
    assert all(set(f) == {'regmean', 'num_rows', 'num_examples', 'task', 'precision'} and f['num_rows'] == 4 * 64 and f['num_examples'] == 4
               and f['task'] == 'composer' and f['precision'] == 'fp32' for f in files)
    for f in files:
        rw = f['regmean']
        assert len(rw) == 16 and len({v.data_ptr() for v in rw.values()}) == 11 and 'encoder_linear.weight' not in rw
        assert all(v.dtype == torch.float32 and v.device.type == 'cpu' and torch.equal(v, v.t()) and bool((v.diagonal() > 0).all()) for v in rw.values())
    out = str(tmp_path / 'merged.ckpt')
    mflags = flags + ['--pretrain_ckpt', str(tmp_path / 'pre.ckpt'), '--model_path', '%s,%s' % (tmp_path / 'ft0.ckpt', tmp_path / 'ft1.ckpt'), '--output_path', out]
    model_merge(mflags + ['--method', 'regmean_merging', '--regmean', '%s,%s' % (tmp_path / 'ft0.regmean.pt', tmp_path / 'ft1.regmean.pt'),
                          '--reduce_non_diagonal_ratio', '0.9'])
    said = capsys.readouterr().out
    assert 'Gram matrices for 16 weights' in said and 'regmean_merging of 2 models' in said
    merged = torch.load(out, map_location='cpu', weights_only=False)['state_dict']
    sds = [f.pianobart.state_dict() for f in fts]
    want = merge_state_dicts(pre.state_dict(), sds, method='regmean_merging', regmean_weights=[f['regmean'] for f in files], reduce_non_diagonal_ratio=0.9)
    assert list(merged) == list(pre.state_dict())
    for k in want:
        assert merged[k].numpy().tobytes() == want[k].numpy().tobytes(), k
    PianoBart(cfg, e2w, w2e).load_state_dict(merged, strict=True)
    average = merge_state_dicts(pre.state_dict(), sds, method='average_merging')
    assert torch.equal(merged['encoder_linear.weight'], average['encoder_linear.weight'])
    assert not torch.equal(merged['bart.encoder.layers.0.fc1.weight'], average['bart.encoder.layers.0.fc1.weight'])
    assert all(bool(torch.isfinite(v).all()) for v in merged.values() if v.is_floating_point())
    with pytest.raises(PBError, match=r'regmean_merging.*pianobart_amd\.regmean'):
        model_merge(mflags + ['--method', 'regmean_merging'])


# ---- the reference's recorded results ---------------------------------------------------------------------------------------------------------
def _merge_recorded(case, N, grams=None):
    from pianobart_amd import merge as M
    g = golden()
    c = g.cases[(case, N)]
    grams = g.grams[:N] if grams is None else grams
    grams = [{k: v for k, v in G.items() if k in c.kept} for G in grams]   # an excluded weight is not merged: its matrix is not handed over
    return M.merge_state_dicts(g.pre, g.fts[:N], method='regmean_merging', regmean_weights=grams, reduce_non_diagonal_ratio=c.ratio, exclude=c.exclude)


def _check_against_recording(case, N, got, tag='device'):
    g = golden()
    c = g.cases[(case, N)]
    assert list(got) == list(g.pre)
    for name in g.pre:
        if name not in c.kept:
            assert got[name].numpy().tobytes() == g.pre[name].numpy().tobytes(), name
        elif name in g.solved:
            W64, e_rec = golden_truth(case, N, name)
            e_dev = rel_error(got[name], W64)
            print('%-5s N=%d %-12s K %3d: %s %.3g, recorded reference %.3g (bound %.3g)' % (case, N, name, W64.shape[1], tag, e_dev, e_rec, MARGIN * max(e_rec, ULP)))
            assert e_dev <= MARGIN * max(e_rec, ULP), (case, N, name, e_dev, e_rec)
        else:
            assert got[name].numpy().tobytes() == c.out[name].numpy().tobytes(), name


@gpu
@pytest.mark.parametrize('case,N', GOLDEN_CASES, ids=CASE_IDS)
def test_merge_matches_the_recorded_reference(case, N):
    _need_gpu()
    _check_against_recording(case, N, _merge_recorded(case, N))


@gpu
@pytest.mark.parametrize('case,N', [('r1', 2), ('r09', 3), ('r09x', 3)], ids=['r1-2', 'r09-3', 'r09x-3'])
def test_shared_and_copied_gram_matrices_give_the_same_bytes(case, N):
    """q and k read one input. As ONE tensor per model regmean_groups makes them one factorisation with stacked right-hand sides (128 columns;
    with q excluded a group of one); as two equal copies two factorisations."""
    _need_gpu()
    from pianobart_amd import merge as M
    g = golden()
    segs = [s for s in g.segs if s.name in g.cases[(case, N)].kept]
    shared = g.grams[:N]
    copied = [dict(G, **{'k.weight': G['k.weight'].clone()}) for G in shared]
    kept = lambda grams: [{k: v for k, v in G.items() if k in g.cases[(case, N)].kept} for G in grams]
    assert len(M.regmean_groups(kept(copied), segs)) == len(M.regmean_groups(kept(shared), segs)) + ('q.weight' in g.cases[(case, N)].kept) == 5 - (case == 'r09x')
    a, b = _merge_recorded(case, N, shared), _merge_recorded(case, N, copied)
    for name in a:
        assert a[name].numpy().tobytes() == b[name].numpy().tobytes(), name
    _check_against_recording(case, N, a, 'shared')
    _check_against_recording(case, N, b, 'copied')


@gpu
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_gram_accum_on_the_recorded_activations(dtype):
    """G = (sum over the batches of X^T X) / rows as the pass forms it (pb_gram_accum per batch, one pb_fisher_finish), batch by batch as the
    hook saw them (40- and 30-row calls, or 8 and 6) and in one call (350 rows: two chunks of T), against X^T X / rows in float64 of the values
    the kernel was given. The header promises an order that depends on (T, K) alone, not that two batches equal their concatenation for
    real values: both results are held to 4 times the recorded matrix's own figure (at least one float32 ulp)."""
    _need_gpu()
    from pianobart_amd import ops
    for module, G_rec, batches in golden_activations():
        given = [b.to(dtype) for b in batches]
        fig_rec, _ = gram_figure(G_rec, batches)
        bound = MARGIN * max(fig_rec, ULP)
        rows, K = sum(b.shape[0] for b in batches), G_rec.shape[0]
        for how, calls in (('batch-wise', given), ('one call', [torch.cat(given)])):
            G = torch.zeros(K, K, device='cuda')
            for x in calls:
                ops.gram_accum(G, x.cuda())
            flags = torch.zeros(1, dtype=torch.int32, device='cuda')
            ops.fisher_finish(G.view(-1), rows, flags)
            assert int(flags.item()) == 0 and torch.equal(G, G.t())
            fig, _ = gram_figure(G.cpu(), given)
            print('%-5s K %3d %-5s %-10s: device %.3g, recorded reference %.3g (bound %.3g)' % (module, K, str(dtype)[6:], how, fig, fig_rec, bound))
            assert fig <= bound, (module, how, fig, fig_rec)


@gpu
def test_too_few_rows_for_a_2d_input_layer_are_refused_by_name():
    """head sees one row per example. Its Gram matrices cut to 6 rows per model (12 in all for 16 inputs) sum to a singular matrix: the
    reference returns finite garbage, merge_state_dicts a PBError that names the weight."""
    _need_gpu()
    from pianobart_amd._lib import PBError
    g = golden()
    (_, _, batches), = [a for a in golden_activations() if a[0] == 'head']
    X = torch.cat(batches).double()
    assert X.shape[1] == 16
    grams = [dict(G) for G in g.grams[:2]]
    for m in range(2):
        x = X[6 * m:6 * m + 6]
        grams[m]['head.weight'] = (x.t() @ x / 6).float()
    with pytest.raises(PBError, match=r'head\.weight.*not positive definite'):
        _merge_recorded('r1', 2, grams)
