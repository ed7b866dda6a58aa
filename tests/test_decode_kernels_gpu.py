"""GPU: the decode kernels of csrc/pb_decode.hip against float64 references written out here, step by step.

  1. pb_gemv          (gemv_kernel, stand-alone instances): integer inputs whose every partial sum is exact in f32, so the result must
                      EQUAL the float64 one (one dropped or doubled element of K = 8192 shows), random inputs under the bounds
                      test_kernels_gpu.py applies to the same arithmetic, and the host-side refusals.
  2. pb_attn_decode   (attn_decode_kernel, all eight instances): key counts from the kernel's own geometry (KPW = 64 / CPR keys per wave load,
                      128 KPW keys per outer iteration), both cache layouts, five key masks, random and `needle` inputs, refusals.
  3. pb_decode_step   against a float64 decoder step (the only route to attn_split_kernel, the MergeIn prologue and the LayerNorm prologue of
                      the GEMV), key-split and one-workgroup attention forms, four encoder masks, and the self K|V cache it leaves behind.
  4. the fused decoder (pb_batch_decoder_*) against the same float64 decoder: B = 1 as graph replays and as direct launches, and the B = 3 row
                      form under the device sampler, every row teacher-forced on the tokens it accepted.

No reference calls into the engine, the training kernels or the oracle for the operation under test. Every output buffer of parts 1 and 2 is
prefilled with NaN and has guard elements behind its end, which must stay NaN.

The decoder parts use a model of max_position_embeddings 160 (the cross cache must hold S_enc = 150 keys) and decode N = 80 positions: the
self-attention goes from one key split to two at position 64, the cross-attention has splits of 64, 64 and 22 keys. The position row of step
i is dec.pos[i + 2] (BART's offset of 2, applied inside pb_embed_ln_fwd).

Measured on an MI355X (worst over the cases; every test prints its own figures): pb_attn_decode f32 5.1e-7 of the output's maximum (bound 3e-5),
bf16 1.5e-2 absolute (4e-2); pb_decode_step fp32 1.6e-6 (2e-4), bf16 3.0e-2 at head_dim 96 (4e-2; its rounding mirror 3.0e-2) and 1.4e-2 ..
2.1e-2 at the other shapes; the fused decoder 1.3e-2 .. 2.6e-2 (mirror 1.2e-2 .. 2.9e-2). The kernels never exceeded 1.14 x their mirror."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests.golden_util import synth_octuple_batch
from tests.test_kernels_gpu import TOL, _rel
from tests.test_model_gpu import _lm

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
NAN = float('nan')
GUARD = 8


@pytest.fixture(scope='module')
def lib():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from pianobart_amd._lib import LIB
    LIB.load()
    return LIB


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _code(dt):
    return 1 if dt == BF16 else 0


def _epv(dt):
    return 8 if dt == BF16 else 4


def _nan(n, dt):
    return torch.full((n + GUARD,), NAN, device='cuda', dtype=dt)


def _guard_ok(buf, n):
    return bool(torch.isnan(buf[n:]).all())


def _err(lib):
    return lib.load().pb_last_error().decode()


# ================================================================================================================ 1. pb_gemv
VARIANTS = {'f32': (F32, 0), 'bf16': (BF16, 0), 'bf16_yf32': (BF16, 1)}
GEMV_N = [1, 2, 3, 7, 262]                      # odd N: the last workgroup has one row and its second weight pointer aliases row n0


def _gemv_K(dt):
    """One live thread; one thread short of a chunk; NCH = 1 full; NCH = 2 with one live thread in chunk 2; nch = 3 on the NCH = 4 instance
    (chunk 3 one live thread, chunk 4 empty); the maximum."""
    e = _epv(dt)
    c = 256 * e
    return [e, c - e, c, c + e, 2 * c + e, 4 * c]


def _gemv(lib, W, x, bias, y, N, K, dt, y_f32, gelu):
    return int(lib.query('pb_gemv', W.data_ptr(), x.data_ptr(), bias.data_ptr() if bias is not None else None, y.data_ptr(), N, K, _code(dt), y_f32,
                         gelu, _stream()))


@pytest.mark.parametrize('ki', range(6))
@pytest.mark.parametrize('variant', list(VARIANTS))
def test_gemv_integer_inputs_are_exact(lib, variant, ki):
    """W, x in -2..2 and an integer bias: every partial sum, in any order, is an integer below 2^24, so f32 accumulation is exact. The f32
    output equals the float64 result, the bf16 output equals it rounded to bf16. The first and the last EPV columns are made positive, so
    the elements of a lone live thread cannot cancel."""
    dt, y_f32 = VARIANTS[variant]
    K, e = _gemv_K(dt)[ki], _epv(dt)
    odt = F32 if (y_f32 or dt == F32) else BF16
    g = torch.Generator(device='cuda').manual_seed(1000 + K)
    for N in GEMV_N:
        W = torch.randint(-2, 3, (N, K), device='cuda', generator=g).float()
        x = torch.randint(-2, 3, (K,), device='cuda', generator=g).float()
        for t in (W, x):
            t[..., :e] = t[..., :e].abs().clamp_min(1)
            t[..., K - e:] = t[..., K - e:].abs().clamp_min(1)
        bias = torch.randint(-1000, 1001, (N,), device='cuda', generator=g).float()
        Wd, xd = W.to(dt), x.to(dt)
        for b in (None, bias):
            ref = Wd.double() @ xd.double() + (b.double() if b is not None else 0)
            y = _nan(N, odt)
            assert _gemv(lib, Wd, xd, b, y, N, K, dt, y_f32, 0) == 0, _err(lib)
            assert _guard_ok(y, N), (N, K)
            want = ref.float() if odt == F32 else ref.float().to(BF16)
            assert torch.equal(y[:N], want), (variant, N, K, b is not None, (y[:N].double() - ref).abs().max().item())


@pytest.mark.parametrize('gelu', [0, 1])
@pytest.mark.parametrize('ki', range(6))
@pytest.mark.parametrize('variant', list(VARIANTS))
def test_gemv_random_inputs(lib, variant, ki, gelu):
    """randn x, randn / sqrt(K) weights, both rounded to the storage type, a bias, erf-GELU or none: the bounds of test_gemm_layouts (no GELU)
    and test_gemm_epilogues (GELU) for the output's type. bf16 operands with an f32 output are f32 arithmetic on rounded inputs: the f32 bounds."""
    dt, y_f32 = VARIANTS[variant]
    K = _gemv_K(dt)[ki]
    odt = F32 if (y_f32 or dt == F32) else BF16
    tol = TOL[odt] if gelu else (3e-6 if odt == F32 else 8e-3)
    g = torch.Generator(device='cuda').manual_seed(2000 + K + gelu)
    for N in (3, 262):
        W = (torch.randn(N, K, device='cuda', generator=g) / math.sqrt(K)).to(dt)
        x = torch.randn(K, device='cuda', generator=g).to(dt)
        bias = torch.randn(N, device='cuda', generator=g)
        ref = W.double() @ x.double() + bias.double()
        if gelu:
            ref = torch.nn.functional.gelu(ref)
        y = _nan(N, odt)
        assert _gemv(lib, W, x, bias, y, N, K, dt, y_f32, gelu) == 0, _err(lib)
        assert _guard_ok(y, N)
        err = _rel(y[:N], ref)
        print('gemv %s N=%d K=%d gelu=%d: %.2e (bound %.0e)' % (variant, N, K, gelu, err, tol))
        assert err < tol, (variant, N, K, gelu, err)


@pytest.mark.parametrize('variant', list(VARIANTS))
def test_gemv_refusals(lib, variant):
    """K not a multiple of EPV, K one vector above the maximum, N = 0, a misaligned x: refused on the host, the output is never written."""
    dt, y_f32 = VARIANTS[variant]
    e = _epv(dt)
    kmax = 4 * 256 * e
    odt = F32 if (y_f32 or dt == F32) else BF16
    W = torch.ones(4 * (kmax + e), device='cuda', dtype=dt)
    x = torch.ones(kmax + 2 * e, device='cuda', dtype=dt)
    y = _nan(4, odt)
    call = lambda N, K, xp: int(lib.query('pb_gemv', W.data_ptr(), xp, None, y.data_ptr(), N, K, _code(dt), y_f32, 0, _stream()))
    for N, K, xp in ((4, e + 1, x.data_ptr()), (4, kmax + e, x.data_ptr()), (0, e, x.data_ptr()), (4, 4 * e, x.data_ptr() + 4)):
        assert call(N, K, xp) < 0, (N, K)
        assert 'pb_gemv' in _err(lib), _err(lib)
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all())
    assert call(4, 4 * e, x.data_ptr()) == 0                        # the same buffers are fine when the arguments are
    assert bool((y[:4].float() == 4 * e).all()) and _guard_ok(y, 4)


# ================================================================================================================ 2. pb_attn_decode
CPR = {(BF16, 32): 4, (BF16, 64): 8, (BF16, 96): 16, (BF16, 128): 16, (F32, 32): 8, (F32, 64): 16, (F32, 96): 32, (F32, 128): 32}
ATTN_MASKS = ['null', 'random', 'key0', 'last', 'none']


def _attn_sks(dt, hd):
    kpw = 64 // CPR[(dt, hd)]
    sks = [1, 2, kpw - 1, kpw, 16 * kpw + 1, 128 * kpw, 128 * kpw + 1] + ([8192] if hd == 64 else [])
    return sorted(set(s for s in sks if s > 0)), kpw


def _attn_mask(kind, Sk, g):
    """(Sk + GUARD) floats or None; the entries behind Sk do not belong to the mask and say `visible`, so a kernel that read them would
    see a key where there is none."""
    if kind == 'null':
        return None
    m = torch.ones(Sk + GUARD, device='cuda')
    if kind == 'random':
        m[:Sk] = (torch.rand(Sk, device='cuda', generator=g) > 0.3).float()
    elif kind == 'key0':
        m[0] = 0
    elif kind == 'last':
        m[:Sk - 1] = 0
    else:
        m[:Sk] = 0
    return m


def _attn_ref(q, K, V, mask, H, hd, scale):
    """softmax(scale q K^T, masked keys at -inf) V in float64 per head; no visible key -> zeros. q (H hd), K / V (Sk, H hd) as stored."""
    Sk = K.shape[0]
    qh, Kh, Vh = q.double().view(H, hd), K.double().view(Sk, H, hd), V.double().view(Sk, H, hd)
    s = torch.einsum('hc,nhc->hn', qh, Kh) * scale
    if mask is not None:
        vis = mask[:Sk] != 0
        if not bool(vis.any()):
            return torch.zeros(H * hd, dtype=torch.float64, device=q.device)
        s = s.masked_fill(~vis[None], float('-inf'))
    return torch.einsum('hn,nhc->hc', torch.softmax(s, -1), Vh).reshape(H * hd)


def _attn_buffers(Kf, Vf, dt, layout):
    """The caches as the kernel sees them: `kv` = the decoder's (S, 2d) rows, V at +d; `sep` = two tensors with padded, different row strides."""
    Sk, d = Kf.shape
    e = _epv(dt)
    if layout == 'kv':
        kv = torch.cat([Kf, Vf], 1).to(dt).contiguous()
        return kv, kv[:, :d], kv[:, d:], kv.data_ptr(), kv.data_ptr() + d * kv.element_size(), 2 * d, 2 * d
    Kb = torch.full((Sk, d + e), 77.0, device='cuda', dtype=dt)
    Vb = torch.full((Sk, d + 2 * e), -77.0, device='cuda', dtype=dt)
    Kb[:, :d] = Kf.to(dt)
    Vb[:, :d] = Vf.to(dt)
    return (Kb, Vb), Kb[:, :d], Vb[:, :d], Kb.data_ptr(), Vb.data_ptr(), d + e, d + 2 * e


def _attn_call(lib, q, kp, vp, out, mask, H, Sk, hd, kss, vss, scale, dt):
    return int(lib.query('pb_attn_decode', q.data_ptr(), kp, vp, out.data_ptr(), mask.data_ptr() if mask is not None else None, H, Sk, hd, kss, vss,
                         scale, _code(dt), _stream()))


def _attn_check(out, ref, dt, d, what):
    """bf16: the forward bound and measure of test_flash_attention_fwd_bwd (max absolute difference < 4e-2). f32: the forward bound and
    measure of test_flash_attention_x3_fwd_bwd, the project's f32-tensor attention (max difference over max reference < 3e-5); one key of
    8192 dropped moves a random output by ~1e-4 of its maximum. A reference of exact zeros (no visible key) must be met exactly."""
    assert _guard_ok(out, d), what
    diff = float((out[:d].double() - ref).abs().max())
    top = float(ref.abs().max())
    if top == 0.0:
        assert bool((out[:d] == 0).all()), what
        return 0.0
    e = diff if dt == BF16 else diff / top
    assert e < (4e-2 if dt == BF16 else 3e-5), (what, e)
    return e


@pytest.mark.parametrize('layout', ['kv', 'sep'])
@pytest.mark.parametrize('H', [1, 3])
@pytest.mark.parametrize('hd', [32, 64, 96, 128])
@pytest.mark.parametrize('dt', [F32, BF16], ids=['f32', 'bf16'])
def test_attn_decode_random_inputs(lib, dt, hd, H, layout):
    d, scale = H * hd, hd ** -0.5
    sks, _ = _attn_sks(dt, hd)
    g = torch.Generator(device='cuda').manual_seed(hd * 10 + H)
    worst = 0.0
    for Sk in sks:
        if Sk == 8192 and (H, layout) != (3, 'kv'):                # the largest size: one instance per dtype
            continue
        q = (1.5 * torch.randn(d, device='cuda', generator=g)).to(dt)
        keep, Kd, Vd, kp, vp, kss, vss = _attn_buffers(1.5 * torch.randn(Sk, d, device='cuda', generator=g),
                                                       1.5 * torch.randn(Sk, d, device='cuda', generator=g), dt, layout)
        for kind in ATTN_MASKS:
            mask = _attn_mask(kind, Sk, g)
            ref = _attn_ref(q, Kd, Vd, mask, H, hd, scale)
            out = _nan(d, dt)
            assert _attn_call(lib, q, kp, vp, out, mask, H, Sk, hd, kss, vss, scale, dt) == 0, _err(lib)
            if kind == 'none':
                assert float(ref.abs().max()) == 0.0
            worst = max(worst, _attn_check(out, ref, dt, d, (Sk, kind)))
    print('attn_decode random %s hd=%d H=%d %s: worst %.2e' % (dt, hd, H, layout, worst))


@pytest.mark.parametrize('hd', [32, 64, 96, 128])
@pytest.mark.parametrize('dt', [F32, BF16], ids=['f32', 'bf16'])
def test_attn_decode_needle(lib, dt, hd):
    """At large Sk the rounding of a bf16 output hides one key of a random input. Here q = 2 u and K[j*] = 4 u per head (u a random sign
    vector, all exact in bf16), the other keys randn: score j* = 8 sqrt(hd) >= 45 against N(0, 2^2) for the others, so key j* carries all
    but e^-30 of the weight and the output is V[j*]. j* = 0, Sk - 1 and each side of the 16 KPW (one load of all waves) and 128 KPW (one
    outer iteration) boundaries; a key that is skipped, or read from the wrong row, gives another row of V. Also with j* the only key a
    mask leaves, and with key j* masked (the output is then far from V[j*] and must match the reference)."""
    H, scale = 3, hd ** -0.5
    d = H * hd
    _, kpw = _attn_sks(dt, hd)
    g = torch.Generator(device='cuda').manual_seed(hd)
    for Sk in [128 * kpw + 1] + ([8192] if hd == 64 else []):
        u = torch.randint(0, 2, (d,), device='cuda', generator=g).float() * 2 - 1
        Kf = torch.randn(Sk, d, device='cuda', generator=g)
        Vf = 1.5 * torch.randn(Sk, d, device='cuda', generator=g)
        q = (2 * u).to(dt)
        for js in sorted({0, Sk - 1, 16 * kpw - 1, 16 * kpw, 128 * kpw - 1, 128 * kpw, Sk // 2}):
            Kn = Kf.clone()
            Kn[js] = 4 * u
            keep, Kd, Vd, kp, vp, kss, vss = _attn_buffers(Kn, Vf, dt, 'kv')
            for kind in ('null', 'only', 'hidden'):
                mask = None
                if kind != 'null':
                    mask = torch.ones(Sk + GUARD, device='cuda')
                    if kind == 'only':
                        mask[:Sk] = 0
                    mask[js] = 1.0 if kind == 'only' else 0.0
                ref = _attn_ref(q, Kd, Vd, mask, H, hd, scale)
                out = _nan(d, dt)
                assert _attn_call(lib, q, kp, vp, out, mask, H, Sk, hd, kss, vss, scale, dt) == 0, _err(lib)
                _attn_check(out, ref, dt, d, (Sk, js, kind))
                if kind != 'hidden':
                    _attn_check(out, Vd[js].double(), dt, d, (Sk, js, kind, 'V[j*]'))
                else:
                    assert float((ref - Vd[js].double()).abs().max()) > 1.0


@pytest.mark.parametrize('dt', [F32, BF16], ids=['f32', 'bf16'])
def test_attn_decode_refusals(lib, dt):
    e, hd, H = _epv(dt), 64, 2
    d = H * hd
    q = torch.ones(d + 2 * e, device='cuda', dtype=dt)
    kv = torch.ones(16, 2 * d + e, device='cuda', dtype=dt)
    out = _nan(d, dt)
    call = lambda qp, Sk, hd_, kss: int(lib.query('pb_attn_decode', qp, kv.data_ptr(), kv.data_ptr() + d * kv.element_size(), out.data_ptr(), None, H, Sk, hd_,
                                                  kss, 2 * d, hd ** -0.5, _code(dt), _stream()))
    for qp, Sk, hd_, kss in ((q.data_ptr(), 8, 48, 2 * d), (q.data_ptr(), 0, hd, 2 * d), (q.data_ptr(), 8193, hd, 2 * d), (q.data_ptr(), 8, hd, 2 * d + 1),
                             (q.data_ptr() + 4, 8, hd, 2 * d)):
        assert call(qp, Sk, hd_, kss) < 0, (Sk, hd_, kss)
        assert 'pb_attn_decode' in _err(lib), _err(lib)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert call(q.data_ptr(), 8, hd, 2 * d) == 0
    assert bool((out[:d] == 1).all()) and _guard_ok(out, d)


# ================================================================================================================ 3. / 4. the decoder
SMAX, N_STEPS, S_ENC, FFN = 160, 80, 150, 136
SPECIAL = [256, 128, 129, 256, 128, 32, 254, 49]
ENC_MASKS = ['all', 'holes', 'mid', 'none']
_MODELS, _REFS = {}, {}


def _model(d, H, precision):
    """A 2-layer model and its engine with bound weights, the bf16 shadow and the projected embedding table in place. The special ids carry a
    -30 bias, as in the existing decode tests, so a sampled row runs to its limit; such logits are left out of the measure, as there."""
    key = (d, H, precision)
    if key not in _MODELS:
        m = _lm(SMAX, d, 2, FFN, H, 31, precision).eval()
        with torch.no_grad():
            for i, p0 in enumerate(SPECIAL):
                m.mask_lm.proj[i].bias[p0:] = -30.0
        m = m.cuda()
        eng = m._get_engine()
        eng.bind(torch.device('cuda', torch.cuda.current_device()))
        eng.refresh_shadow(force=True)
        eng.build_ptab()
        torch.cuda.synchronize()
        _MODELS[key] = (m, eng)
    return _MODELS[key]


def _enc_mask(kind, s_enc, seed=5):
    """(SMAX) f32 on the CPU: all visible; ~30 % holes; keys 64..127 hidden (the middle split's record has m = -inf); nothing visible."""
    m = torch.ones(SMAX)
    if kind == 'holes':
        m[:s_enc] = (torch.rand(s_enc, generator=torch.Generator().manual_seed(seed)) > 0.3).float()
    elif kind == 'mid':
        m[64:128] = 0
    elif kind == 'none':
        m[:] = 0
    return m


def _cross_values(d, dt, seed):
    """Random cross K|V caches of the two layers, rounded to dt: no encoder pass is involved."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(SMAX, 2 * d, generator=g).to(dt) for _ in range(2)]


def _inputs():
    """The decoder inputs of the N_STEPS positions: SOS, then a fixed synthetic piece."""
    forced = synth_octuple_batch(1, N_STEPS, seed=23, min_len=N_STEPS)[5][0]
    forced[-1] = forced[-2]
    sos = torch.tensor([258, 130, 131, 258, 130, 34, 256, 51])
    return torch.cat([sos[None], forced[:-1]], 0)


class Decoder64:
    """One decoder token at a time in float64 on the CPU, from the engine's weight dictionaries (weights as stored in dt, biases / LayerNorm /
    tables f32). mirror: round to dt wherever the kernels store a row of dt (x, q, the K|V cache row, the merged context, a, y1, yc, g, y2);
    otherwise nothing is rounded."""

    def __init__(self, eng, kvc, mask, s_enc, mirror):
        from pianobart_amd import ops
        dt = eng.xdt
        self.rnd = (lambda t: t.to(dt).double()) if mirror else (lambda t: t)
        self.d, self.H, self.hd = eng.d, eng.H, eng.d // eng.H
        W = lambda n: eng.w[n].detach().double().cpu()
        F = lambda n: eng.wf[n].detach().double().cpu()
        self.ptab, self.off = eng.ptab.double().cpu(), ops.TAB_OFF
        self.lin_b, self.pos, self.lne = F('lin.b'), F('dec.pos'), (F('dec.lne.w'), F('dec.lne.b'))
        self.layers = []
        for l in range(2):
            p = 'dec.%d.' % l
            L = {n: W(p + n) for n in ('wqkv', 'wo', 'wq_c', 'wo_c', 'w1', 'w2')}
            L.update({n: F(p + n) for n in ('bqkv', 'bo', 'bq_c', 'bo_c', 'b1', 'b2', 'ln1.w', 'ln1.b', 'lnc.w', 'lnc.b', 'ln2.w', 'ln2.b')})
            L['kvc'] = kvc[l][:s_enc].double().cpu()
            L['kvs'] = torch.zeros(SMAX, 2 * self.d, dtype=torch.float64)
            self.layers.append(L)
        self.head = (W('head.w'), F('head.b'))
        self.vis = (mask[:s_enc] != 0) if mask is not None else None

    @staticmethod
    def ln(x, w, b):
        mu = x.mean()
        return (x - mu) / torch.sqrt(((x - mu) ** 2).mean() + 1e-5) * w + b

    def attn(self, q, kv, vis):
        n, H, hd, d = kv.shape[0], self.H, self.hd, self.d
        if vis is not None and not bool(vis.any()):
            return torch.zeros(d, dtype=torch.float64)
        s = torch.einsum('hc,nhc->hn', q.view(H, hd), kv[:, :d].reshape(n, H, hd)) / math.sqrt(hd)
        if vis is not None:
            s = s.masked_fill(~vis[None], float('-inf'))
        return torch.einsum('hn,nhc->hc', torch.softmax(s, -1), kv[:, d:].reshape(n, H, hd)).reshape(d)

    def step(self, i, tok):
        r, d = self.rnd, self.d
        x = self.lin_b + self.pos[i + 2]
        for k in range(8):
            x = x + self.ptab[self.off[k] + int(tok[k])]
        h = r(self.ln(x, *self.lne))
        for L in self.layers:
            qkv = r(L['wqkv'] @ h + L['bqkv'])
            L['kvs'][i] = qkv[d:]
            a = r(L['wo'] @ r(self.attn(qkv[:d], L['kvs'][:i + 1], None)) + L['bo'])
            y1 = r(self.ln(h + a, L['ln1.w'], L['ln1.b']))
            q = r(L['wq_c'] @ y1 + L['bq_c'])
            a = r(L['wo_c'] @ r(self.attn(q, L['kvc'], self.vis)) + L['bo_c'])
            yc = r(self.ln(y1 + a, L['lnc.w'], L['lnc.b']))
            g = r(torch.nn.functional.gelu(L['w1'] @ yc + L['b1']))
            a = r(L['w2'] @ g + L['b2'])
            h = r(self.ln(yc + a, L['ln2.w'], L['ln2.b']))
        return self.head[0] @ h + self.head[1]

    def run(self, inputs):
        return torch.stack([self.step(i, inputs[i]) for i in range(len(inputs))])


def _reference(eng, kvc, mask, s_enc, inputs):
    """(exact logits, mirror logits, exact K|V rows per layer) of the float64 decoder teacher-forced on `inputs`."""
    ex = Decoder64(eng, kvc, mask, s_enc, False)
    mi = Decoder64(eng, kvc, mask, s_enc, True)
    return ex.run(inputs), mi.run(inputs), [L['kvs'] for L in ex.layers]


def _shared_reference(d, H, precision, kind):
    """The reference of one (shape, dtype, encoder mask): computed once, shared by parts 3 and 4, never modified."""
    key = (d, H, precision, kind)
    if key not in _REFS:
        m, eng = _model(d, H, precision)
        _REFS[key] = _reference(eng, _cross_values(d, eng.xdt, d + H), _enc_mask(kind, S_ENC), S_ENC, _inputs())
    return _REFS[key]


def _worst(got, ref):
    """The cfg-2 decode test's measure: per step max |difference| over max |reference| of the logits row (without the -30 biased
    special ids); the worst step."""
    got, ref = got.double().cpu(), ref.double()
    worst = 0.0
    for i in range(ref.shape[0]):
        keep = ref[i] > -20
        worst = max(worst, float((got[i][keep] - ref[i][keep]).abs().max() / ref[i][keep].abs().max()))
    return worst


def _check_logits(got, exact, mirror, precision, what):
    """fp32: 2e-4 against the unrounded decoder. bf16: at most twice the error of the float64 decoder that rounds where the kernels store bf16
    rows (f32 accumulation flips individual roundings: noise of the size of the rounding noise itself), and at most the project's 4e-2."""
    assert bool(torch.isfinite(got).all()), what
    e_k = _worst(got, exact)
    if precision == 'fp32':
        print('%s: kernel vs exact %.2e (bound 2e-4)' % (what, e_k))
        assert e_k < 2e-4, (what, e_k)
    else:
        e_m = _worst(mirror, exact)
        print('%s: kernel vs exact %.2e, mirror vs exact %.2e (bounds %.2e and 4e-2)' % (what, e_k, e_m, 2 * e_m))
        assert e_k <= 2 * e_m and e_k <= 4e-2, (what, e_k, e_m)
    return e_k


def _plan(eng, B, s_enc, masks, kvc_rows):
    """eng._decode_plan with its cross caches filled (row b from kvc_rows[b]) and its self caches zeroed. masks: (B, SMAX) CPU or None."""
    dev = torch.device('cuda', torch.cuda.current_device())
    em = masks.to(dev).contiguous() if masks is not None else None
    bp, bufs = eng._decode_plan(B, SMAX, s_enc, em, dev)
    for l in range(2):
        for b in range(B):
            bufs['kvc'][l][b].copy_(kvc_rows[b][l])
        bufs['kvs'][l].zero_()
    bufs['em'] = em
    return bp, bufs


# head_dim 32, 96, 64, 128 with the keys split over workgroups; `one` = plan.attn_part NULL, for one shape per dtype
DEC_SHAPES = [(128, 4, 'split'), (192, 2, 'split'), (256, 4, 'split'), (256, 2, 'split'), (256, 4, 'one')]


@pytest.mark.parametrize('kind', ENC_MASKS)
@pytest.mark.parametrize('d,H,form', DEC_SHAPES)
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_decode_step_against_float64_decoder(lib, precision, d, H, form, kind):
    """pb_decode_step, 80 positions: the logits row of every step and the self K|V cache afterwards. form `one` = the one-workgroup
    attention writing ctx; both forms meet the same bound."""
    m, eng = _model(d, H, precision)
    exact, mirror, kv_ref = _shared_reference(d, H, precision, kind)
    bp, bufs = _plan(eng, 1, [S_ENC], None if kind == 'all' else _enc_mask(kind, S_ENC)[None], [_cross_values(d, eng.xdt, d + H)])
    assert bool(bp.plan.attn_part)
    if form == 'one':
        bp.plan.attn_part = None
    toks = _inputs().to(torch.int16).cuda()
    rows = torch.full((N_STEPS, bufs['logits'].shape[1]), NAN, device='cuda')
    for i in range(N_STEPS):
        bufs['tok16'].copy_(toks[i])
        bufs['logits'].fill_(NAN)
        lib.call('pb_decode_step', ctypes.byref(bp.plan), i, _stream())
        rows[i].copy_(bufs['logits'][0])
    torch.cuda.synchronize()
    _check_logits(rows, exact, mirror, precision, 'pb_decode_step %s d=%d hd=%d %s mask=%s' % (precision, d, d // H, form, kind))
    for l in range(2):
        kvs = bufs['kvs'][l][0]
        assert _rel(kvs[:N_STEPS].cpu(), kv_ref[l][:N_STEPS]) < TOL[eng.xdt], l
        assert bool((kvs[N_STEPS:] == 0).all()), l                  # rows that were never decoded


FUSED_SHAPES = [(256, 4), (256, 2), (512, 4)]                     # head_dim 64, 128, 128


@pytest.mark.parametrize('kind', ENC_MASKS)
@pytest.mark.parametrize('d,H', FUSED_SHAPES)
def test_fused_decoder_one_row_against_float64_decoder(lib, d, H, kind):
    """pb_batch_decoder_step at B = 1, as graph replays and as direct launches: each meets the bf16 bound of part 3 against the float64
    decoder, and the two are equal bit for bit."""
    m, eng = _model(d, H, 'bf16')
    exact, mirror, kv_ref = _shared_reference(d, H, 'bf16', kind)
    toks = _inputs().numpy().astype(np.int16)
    got = {}
    for use_graph in (1, 0):
        bp, bufs = _plan(eng, 1, [S_ENC], None if kind == 'all' else _enc_mask(kind, S_ENC)[None], [_cross_values(d, BF16, d + H)])
        dec = eng._decoder_create(bp)
        assert dec is not None
        try:
            lib.call('pb_batch_decoder_reset', dec, _stream(), use_graph)
            rows = torch.full((N_STEPS, exact.shape[1]), NAN)
            tok = np.zeros(8, dtype=np.int16)
            for i in range(N_STEPS):
                tok[:] = toks[i]
                lib.call('pb_batch_decoder_step', dec, tok.ctypes.data, rows[i].data_ptr())
            assert bool(lib.query('pb_batch_decoder_graph', dec)) == bool(use_graph)
        finally:
            lib.call('pb_batch_decoder_destroy', dec)
        _check_logits(rows, exact, mirror, 'bf16', 'fused B=1 d=%d hd=%d graph=%d mask=%s' % (d, d // H, use_graph, kind))
        for l in range(2):
            kvs = bufs['kvs'][l][0]
            assert _rel(kvs[:N_STEPS].cpu(), kv_ref[l][:N_STEPS]) < TOL[BF16], l
            assert bool((kvs[N_STEPS:] == 0).all()), l
        got[use_graph] = rows
    assert torch.equal(got[1], got[0])


ROW_MASKS = {0: ('holes', 'mid', 'all'), 1: ('none', 'holes', 'mid')}
ROW_S_ENC = [40, 150, SMAX]                                        # one split; 64 + 64 + 22; 64 + 64 + 32


@pytest.mark.parametrize('assign', [0, 1])
@pytest.mark.parametrize('d,H', FUSED_SHAPES)
def test_fused_decoder_rows_against_float64_decoder(lib, d, H, assign):
    """B = 3 rows under the device sampler (GenerationMixin._decode_device_sampled on a decoder built here): rows of 40, 150 and 160 encoder
    keys, each with its own mask and its own random cross K|V, so a row that read another row's cache slice, mask or split geometry cannot
    pass. The host's sampler is handed every logged logits row once; each row's float64 decoder is then teacher-forced on the tokens the row
    accepted, and every logged row must meet the bf16 bound of part 3."""
    m, eng = _model(d, H, 'bf16')
    B = 3
    masks = torch.stack([_enc_mask(k, ROW_S_ENC[b], seed=7 + b) for b, k in enumerate(ROW_MASKS[assign])])
    kvc_rows = [_cross_values(d, BF16, 100 * assign + 10 * b + d) for b in range(B)]
    bp, bufs = _plan(eng, B, ROW_S_ENC, masks, kvc_rows)
    pad_cpu = torch.from_numpy(eng.pb.pad_word_np)
    res_cpu = pad_cpu.repeat(B, SMAX, 1)
    rngs = [np.random.RandomState(300 + 10 * assign + b) for b in range(B)]
    logged = [[] for _ in range(B)]

    def sample(b, row, **kw):
        logged[b].append(row.clone())
        return m.sample_row(row, rngs[b], **kw)

    dec = eng._decoder_create(bp)
    assert dec is not None
    try:
        lib.call('pb_batch_decoder_reset', dec, _stream(), 1)
        torch.cuda.current_stream().synchronize()
        with torch.no_grad():
            info = eng._decode_device_sampled(dec, B, SMAX, sample, [r.get_state() for r in rngs], dict(T=m.SAMPLE_T, P=m.SAMPLE_P), res_cpu, pad_cpu,
                                              N_STEPS, (-1, 0), inline_verify=True)
    finally:
        lib.call('pb_batch_decoder_destroy', dec)
    assert info['ended'] == ['limit'] * B and info['tokens'] == [N_STEPS] * B, info
    sos = torch.tensor([258, 130, 131, 258, 130, 34, 256, 51])
    for b in range(B):
        assert len(logged[b]) == N_STEPS
        assert bool((res_cpu[b, :N_STEPS] < pad_cpu).all()) and bool((res_cpu[b, N_STEPS:] == pad_cpu).all())
        inputs = torch.cat([sos[None], res_cpu[b, :N_STEPS - 1]], 0)
        exact, mirror, kv_ref = _reference(eng, kvc_rows[b], masks[b], ROW_S_ENC[b], inputs)
        _check_logits(torch.stack(logged[b]), exact, mirror, 'bf16',
                      'fused B=3 d=%d hd=%d row %d (s_enc %d, mask %s, %d rewinds)' % (d, d // H, b, ROW_S_ENC[b], ROW_MASKS[assign][b], info['rewinds'][b]))
        for l in range(2):
            kvs = bufs['kvs'][l][b]
            assert _rel(kvs[:N_STEPS].cpu(), kv_ref[l][:N_STEPS]) < TOL[BF16], (b, l)
            assert bool((kvs[N_STEPS:] == 0).all()), (b, l)
