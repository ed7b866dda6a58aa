"""A plain reference of the attention kernels (csrc/pb_flash.hip, pb_flash64.hip, pb_flash1.hip, pb_flash_x3.hip behind pb_attn_fwd /
pb_attn_bwd) and a model of what they store, written from the formulas of include/pianobart_hip.h with torch tensor arithmetic only: no
softmax / scaled_dot_product_attention call, no autograd.

attn() computes in the dtype of its inputs. float64 inputs with the default (identity) `rnd` and plain `mm` give the TRUTH. float32 inputs
with `rnd`, `mm`, `prescale` and `dq_block` set give the STORAGE MODEL: float32 arithmetic with a rounding wherever the ABI or the kernels'
own header comments say that a matrix-core operand or a stored result is narrow. The model is written from the header and those comments
alone and is never tuned to a kernel's output; its own distance from the truth, in the measure of figure() below, is the yardstick the GPU
tests (tests/test_attention_kernels_gpu.py) hold the kernels to. tests/test_attn_ref_cpu.py checks the float64 form against float64
torch.autograd, so the reference stands without a GPU.

Operands are (B, H, S, head_dim); `vis` is a boolean (B, 1 | H, Sq, Sk) visibility, so key masks, kmax, causal and the packed k_vis all
reduce to it (visible()).
"""
import math

import torch

LOG2E = 1.4426950408889634
E8, E9 = 2.0 ** -8, 2.0 ** -9


# ---------------------------------------------------------------- roundings and products of the storage models
def ident(x):
    return x


def bf16(x):
    """x rounded to bfloat16 (nearest even) and back in x's dtype."""
    return x.to(torch.bfloat16).to(x.dtype)


def mm_plain(a, b):
    return a @ b


def mm_split3(a, b):
    """PB_F32X3: a_hi b_hi + a_hi b_lo + a_lo b_hi with hi = bf16(x), lo = bf16(x - hi); the a_lo b_lo term is dropped and the two small
    terms are added first (the header of pb_gemm_x3.hip)."""
    ah, bh = bf16(a), bf16(b)
    al, bl = bf16(a - ah), bf16(b - bh)
    return (ah @ bl + al @ bh) + ah @ bh


MODELS = {
    # the generic kernels (pb_flash.hip): P and dS are bf16 matrix-core operands, O / dQ / dK / dV are stored in bf16, the scores stay f32
    'bf16': dict(mm=mm_plain, rnd=bf16, prescale=False, kv_prescale=False, dq_block=0),
    # the pipelined kernels (pb_flash64.hip): the same, and Q (forward, dQ kernel) or K (dK / dV kernel) is prescaled by scale * log2(e) in bf16
    'prescale': dict(mm=mm_plain, rnd=bf16, prescale=True, kv_prescale=True, dq_block=0),
    # the one-pass backward (pb_flash1.hip): K prescaled, and dQ goes through one bf16 slab per 256-key block, summed in f32, rounded once
    'one_pass': dict(mm=mm_plain, rnd=bf16, prescale=True, kv_prescale=True, dq_block=256),
    # PB_F32X3 (pb_flash_x3.hip): f32 storage, every product a split-bf16 triple (P and dS are cut into hi + lo like any other operand)
    'x3': dict(mm=mm_split3, rnd=ident, prescale=False, kv_prescale=False, dq_block=0),
}


# ---------------------------------------------------------------- visibility
def visible(B, Sq, Sk, device, key_mask=None, causal=False, kmax=None):
    """(B, 1, Sq, Sk) bool: key j is visible to query i of batch b iff key_mask[b, j] != 0 (where given), j < kmax[b] (where given) and,
    causal, j <= i. The packed k_vis is a kmax."""
    vis = torch.ones(B, 1, Sq, Sk, dtype=torch.bool, device=device)
    j = torch.arange(Sk, device=device)
    if key_mask is not None:
        vis = vis & (key_mask != 0)[:, None, None, :]
    if kmax is not None:
        vis = vis & (j[None, :] < torch.as_tensor(kmax, device=device).reshape(B, 1))[:, None, None, :]
    if causal:
        vis = vis & (j[None, :] <= torch.arange(Sq, device=device)[:, None])
    return vis


# ---------------------------------------------------------------- attention, forward and backward
def attn(q, k, v, dout, vis, scale, mm=mm_plain, rnd=ident, prescale=False, kv_prescale=False, dq_block=0):
    """dict with
      o (B,H,Sq,hd)  = P V, P = softmax over the visible keys of scale * Q K^T; a row without a visible key: o = 0
      lse (B,H,Sq)   = log sum_visible exp(scale * q.k), natural units; +inf for a row without a visible key
      delta (B,H,Sq) = sum_c dO_c O_c
      dq, dk, dv     = the gradients of sum(dO * O); dq = 0 for a row without a visible key, dk = dv = 0 for a key no query sees
      p, dP          = the probabilities (exactly 0 where not visible) and dO V^T
      a              = p * (|dP| + sum_c |dO_c O_c|): the magnitude of the two terms dS = p * (dP - delta) is the difference of.
    rnd rounds every narrow operand and stored result, mm is the matrix product, prescale rounds q * scale * log2(e) once before the score
    product, dq_block > 0 rounds the dQ partial of every block of dq_block keys and sums the blocks in the working dtype.
    The backward is the ABI's: it reads the stored lse and recomputes p = exp2(score - lse * log2(e)) (not the forward's e / sum). With
    kv_prescale its dK / dV side takes its scores from q . bf16(k * scale * log2(e)) -- the header comment of fa64_bwd_dkv_kernel: "With K
    prescaled by c" -- while lse comes from the forward's bf16(q * scale * log2(e)) . k: the two roundings differ by 2^-9 |score|, so this
    p is not normalised (one visible key: p != 1). The dQ side keeps the forward's scores, except with dq_block, where one dS (the one-pass
    kernel's, "K fragments (prescaled)" in pb_flash1.hip) serves dQ, dK and dV."""
    kT = k.transpose(-1, -2)
    c = scale * LOG2E
    if prescale:
        s2 = mm(rnd(q * c), kT)                                        # scores in log2 units
    else:
        s2 = mm(q, kT) * c
    vis = vis.expand(s2.shape)
    has = vis.any(-1, keepdim=True)
    mx = torch.where(vis, s2, torch.full_like(s2, float('-inf'))).amax(-1, keepdim=True)
    mx = torch.where(has, mx, torch.zeros_like(mx))
    e = torch.where(vis, torch.exp2(s2 - mx), torch.zeros_like(s2))
    tot = e.sum(-1, keepdim=True)
    safe = torch.where(has, tot, torch.ones_like(tot))
    p = e / safe                                                       # rows without a visible key: 0 / 1
    lse = torch.where(has, (mx + torch.log2(safe)) / LOG2E, torch.full_like(mx, float('inf')))[..., 0]
    pr = rnd(p)
    o = rnd(mm(pr, v))
    dod = dout * o
    delta = dod.sum(-1)
    dP = mm(dout, v.transpose(-1, -2))
    lse2 = (lse * LOG2E)[..., None]                                    # +inf for a row without a visible key: p = exp2(-inf) = 0
    pq = torch.where(vis, torch.exp2(s2 - lse2), torch.zeros_like(s2))
    pk = torch.where(vis, torch.exp2(mm(q, rnd(k * c).transpose(-1, -2)) - lse2), torch.zeros_like(s2)) if kv_prescale else pq
    dSk = rnd(pk * (dP - delta[..., None]))
    if dq_block:
        dq = torch.zeros_like(q)
        for j0 in range(0, k.shape[-2], dq_block):
            dq = dq + rnd(scale * mm(dSk[..., j0:j0 + dq_block], k[..., j0:j0 + dq_block, :]))
        dq = rnd(dq)
    else:
        dq = rnd(scale * mm(rnd(pq * (dP - delta[..., None])), k))
    dk = rnd(scale * mm(dSk.transpose(-1, -2), q))
    dv = rnd(mm(rnd(pk).transpose(-1, -2), dout))
    a = p * (dP.abs() + dod.abs().sum(-1, keepdim=True))
    return dict(o=o, lse=lse, delta=delta, dq=dq, dk=dk, dv=dv, p=p, dP=dP, a=a)


def scales(truth, q, k, v, dout, vis, scale):
    """S of every result, from the truth (float64 operands): the cancellation-free sum of the term magnitudes of the element's contraction.
    The plain |dS| would be the wrong scale of dq / dk: a row with one visible key has dS == 0 exactly while the rounded o moves delta.
    lse: the largest |q|.|k| score bound over the row's visible keys (0 for a row without one, whose lse is +inf)."""
    p, a = truth['p'], truth['a']
    sabs = scale * (q.abs() @ k.abs().transpose(-1, -2))
    s_lse = torch.where(vis.expand(sabs.shape), sabs, torch.zeros_like(sabs)).amax(-1)
    return dict(o=p @ v.abs(), dv=p.transpose(-1, -2) @ dout.abs(), dq=scale * (a @ k.abs()), dk=scale * (a.transpose(-1, -2) @ q.abs()),
                delta=(dout * truth['o']).abs().sum(-1), lse=s_lse)


def colsum(x):
    """(B, H, S, hd) -> (H * hd): the sum over batch and position, columns in the (h, c) order of a (B, S, H * hd) projection output."""
    return x.sum((0, 2)).reshape(-1)


def figure(got, truth, S, stored_bf16):
    """max over ALL elements of (|got - truth| - ulp) / (2^-9 * S), ulp = 2^-8 |truth| for a bf16-stored result and 0 for f32. An element
    with S == 0 must be exactly 0 (and one whose truth is +inf exactly +inf): otherwise the figure is +inf, and so it is for any NaN."""
    got, truth, S = got.double(), truth.double(), S.double()
    if got.numel() == 0:
        return 0.0
    inf = torch.isinf(truth)
    err = torch.where(inf, torch.zeros_like(truth), got - torch.where(inf, torch.zeros_like(truth), truth)).abs()
    if stored_bf16:
        err = (err - E8 * torch.where(inf, torch.zeros_like(truth), truth).abs()).clamp_min(0)
    exact = inf | (S == 0)
    fig = torch.where(exact, torch.zeros_like(err), err / (E9 * torch.where(exact, torch.ones_like(S), S)))
    bad = (exact & (got != truth)) | torch.isnan(got)
    fig = torch.where(bad, torch.full_like(fig, float('inf')), fig)
    return float(fig.max())


# ---------------------------------------------------------------- inputs that move the forward's lazy reference maximum
LAZY_KINDS = ('rise', 'fall', 'edge', 'wide', 'low')


def lazy_inputs(kind, B, H, Sq, Sk, hd, scale, gen, device):
    """float32 (B, H, S, hd) q, k whose log2 scores scale * log2(e) * q.k follow a profile per 64-key tile (pb_flash64.hip keeps a row's
    reference maximum until a tile holds a score more than 8 log2 units above it): q lies along the unit direction u plus noise, key j has
    the projection t[j // 64] on u plus noise, so a score is about |q| * t in natural units.
      rise: + 9.5 log2 units per tile     fall: - 9.5 per tile     edge: steps of +7.6, +8.4, -7.6, -8.4, ... (just under and over 8)
      wide: no direction, randn * 4       low: every score about -100 natural units."""
    f = lambda *s: torch.randn(*s, generator=gen, device=device)
    if kind == 'wide':
        return f(B, H, Sq, hd) * 4, f(B, H, Sk, hd) * 4
    u = torch.zeros(hd, device=device)
    u[::2] = (2.0 / hd) ** 0.5                                          # unit vector
    nt = (Sk + 63) // 64
    amp = 4.0                                                          # |q . u|
    per = 1.0 / (scale * LOG2E * amp)                                  # projection that makes one log2 unit
    if kind == 'rise':
        lv = [9.5 * i for i in range(nt)]
    elif kind == 'fall':
        lv = [-9.5 * i for i in range(nt)]
    elif kind == 'edge':
        steps, lv = [7.6, 8.4, -7.6, -8.4], [0.0]
        for i in range(nt - 1):
            lv.append(lv[-1] + steps[i % 4])
    elif kind == 'low':
        lv = [-100.0 * LOG2E] * nt
    else:
        raise ValueError(kind)
    lv = torch.tensor(lv, device=device)
    t = lv[torch.arange(Sk, device=device) // 64] * per
    nq = f(B, H, Sq, hd)
    nq = nq - (nq @ u)[..., None] * u                                  # noise across u: it moves single scores, not the tiles' levels
    return amp * u + nq, t[:, None] * u + f(B, H, Sk, hd)
