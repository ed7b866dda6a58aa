"""Plain references of the row kernels (csrc/pb_norm.hip, pb_softmax.hip, pb_loss.hip, pb_optim.hip), written from the formulas of
include/pianobart_hip.h with torch tensor arithmetic only: no layer_norm / softmax / cross_entropy call, no autograd. Every function
computes in the dtype of its inputs: float64 inputs give the reference, float32 inputs the "plain float32 evaluation of the same
formula" whose own error sets the bounds of tests/test_row_kernels_gpu.py. tests/test_row_ref_cpu.py checks the float64 forms against
float64 torch.autograd, so the references stand without a GPU.
"""
import numpy as np
import torch

from tests.philox_ref import drop_consts, drop_words


# ---------------------------------------------------------------- dropout masks by row
def drop_mask_rows(seed, site, p, row_ids, d):
    """float32 (len(row_ids), d) on the CPU: element (r, c) of a (rows, d) dropout site takes word c & 3 of the counter
    row_ids[r] * (d / 4) + c // 4 (mod 2^32): what the kernels draw for row row_ids[r] of the padded batch. p == 0 gives ones."""
    rid = np.asarray(row_ids, dtype=np.uint64).reshape(-1)
    if p <= 0:
        return torch.ones(len(rid), d)
    d4 = d // 4
    idx4 = (rid[:, None] * np.uint64(d4) + np.arange(d4, dtype=np.uint64)[None, :]) & np.uint64(0xFFFFFFFF)
    words = drop_words(seed, site, idx4.reshape(-1)).reshape(len(rid), d)
    thresh, scale = drop_consts(p)
    return torch.from_numpy(np.where(words < thresh, np.float32(0.0), scale).astype(np.float32))


# ---------------------------------------------------------------- LayerNorm
def ln_fwd(z, w, b, eps):
    """y = (z - mean) * rstd * w + b with the biased variance; returns y, mean (T), rstd (T)."""
    mean = z.sum(-1, keepdim=True) / z.shape[-1]
    c = z - mean
    rstd = 1.0 / torch.sqrt((c * c).sum(-1, keepdim=True) / z.shape[-1] + eps)
    return c * rstd * w + b, mean[:, 0], rstd[:, 0]


def ln_bwd(dy, z, w, mean, rstd):
    """dz of y = LN(z) for the cotangent dy, from the saved statistics. Returns dz and the pieces the bounds need:
    xhat, g = dy * w, s1 = mean(g), s2 = mean(g * xhat)."""
    xh = (z - mean[:, None]) * rstd[:, None]
    g = dy * w
    s1 = g.sum(-1, keepdim=True) / z.shape[-1]
    s2 = (g * xh).sum(-1, keepdim=True) / z.shape[-1]
    return (g - s1 - xh * s2) * rstd[:, None], xh, g, s1, s2


def add_ln_fwd(res, a, mask, w, b, eps):
    """y = LN(res + a * mask)."""
    return ln_fwd(res + a * mask, w, b, eps)


def add_ln_bwd(dy, res, a, mask, w, mean, rstd):
    """dict: dres = dz, da = dz * mask, the column-sum terms (T, d) of dgamma = dy * xhat, dbeta = dy, dbias_a = da, and the row scale
    of dz (the magnitude of the three terms it is the difference of)."""
    dz, xh, g, s1, s2 = ln_bwd(dy, res + a * mask, w, mean, rstd)
    scale = (g.abs().amax(-1) + s1.abs()[:, 0] + xh.abs().amax(-1) * s2.abs()[:, 0]) * rstd.abs()
    return dict(dres=dz, da=dz * mask, t_dgamma=dy * xh, t_dbeta=dy, t_dbias=dz * mask, scale=scale)


# ---------------------------------------------------------------- Octuple embedding + position + LayerNorm (+ dropout after it)
def embed_z(ids, P, seg_off, lin_bias, pos, pos_idx):
    """z[t] = lin_bias + pos[pos_idx[t] + 2] + sum_i P[seg_off[i] + ids[t, i]]; ids (T, 8) int64, pos_idx (T) int64."""
    off = torch.as_tensor(list(seg_off[:8]), device=ids.device)
    z = lin_bias + pos[pos_idx + 2]
    for i in range(8):                                       # the kernel's order of additions
        z = z + P[off[i] + ids[:, i]]
    return z


def embed_ln_fwd(ids, P, seg_off, lin_bias, pos, pos_idx, w, b, eps, mask):
    y, mean, rstd = ln_fwd(embed_z(ids, P, seg_off, lin_bias, pos, pos_idx), w, b, eps)
    return y * mask, mean, rstd


def embed_ln_bwd(dy, ids, P, seg_off, lin_bias, pos, pos_idx, w, mean, rstd, mask):
    """dict: dz (T, d), dP and dpos (scatter-adds of dz), sP (table rows) and spos (positions) = the row scales of dz scatter-added
    the same way (each addend of a dP / dpos element is a dz element, whose error is measured against its row's scale; 0 where no row with
    a gradient points), the column-sum terms of dgamma, dbeta and dbias, and the row scale of dz."""
    dyv = dy * mask
    dz, xh, g, s1, s2 = ln_bwd(dyv, embed_z(ids, P, seg_off, lin_bias, pos, pos_idx), w, mean, rstd)
    scale = (g.abs().amax(-1) + s1.abs()[:, 0] + xh.abs().amax(-1) * s2.abs()[:, 0]) * rstd.abs()
    off = torch.as_tensor(list(seg_off[:8]), device=ids.device)
    dP, sP = torch.zeros_like(P), torch.zeros_like(P[:, 0])
    for i in range(8):
        dP.index_add_(0, off[i] + ids[:, i], dz)
        sP.index_add_(0, off[i] + ids[:, i], scale)
    dpos, spos = torch.zeros_like(pos), torch.zeros_like(pos[:, 0])
    dpos.index_add_(0, pos_idx + 2, dz)
    spos.index_add_(0, pos_idx + 2, scale)
    return dict(dz=dz, dP=dP, sP=sP, dpos=dpos, spos=spos, t_dgamma=dyv * xh, t_dbeta=dyv, t_dbias=dz, scale=scale)


# ---------------------------------------------------------------- masked softmax over the key axis
def softmax_visible(B, H, Sq, Sk, key_mask, causal, device):
    vis = torch.ones(B, H, Sq, Sk, dtype=torch.bool, device=device)
    if key_mask is not None:
        vis = vis & (key_mask != 0)[:, None, None, :]
    if causal:
        i = torch.arange(Sq, device=device)[:, None]
        j = torch.arange(Sk, device=device)[None, :]
        vis = vis & (j <= i)
    return vis


def softmax_fwd(scores, key_mask, scale, causal):
    """P = softmax(scale * scores) over the visible keys of each (b, h, query) row, the maximum subtracted; masked positions and rows
    without a visible key are exactly 0."""
    B, H, Sq, Sk = scores.shape
    vis = softmax_visible(B, H, Sq, Sk, key_mask, causal, scores.device)
    s = scores * scale
    mx = torch.where(vis, s, torch.full_like(s, float('-inf'))).amax(-1, keepdim=True)
    mx = torch.where(torch.isinf(mx), torch.zeros_like(mx), mx)
    e = torch.where(vis, torch.exp(s - mx), torch.zeros_like(s))
    tot = e.sum(-1, keepdim=True)
    return torch.where(tot > 0, e / torch.where(tot > 0, tot, torch.ones_like(tot)), torch.zeros_like(e))


def softmax_bwd(dP, P, scale):
    """dS = scale * P * (dP - rowsum(dP * P))."""
    return scale * P * (dP - (dP * P).sum(-1, keepdim=True))


# ---------------------------------------------------------------- 8-head cross-entropy
def first_argmax(x):
    """index of the first maximum of each row (np.argmax's rule), without relying on any library's tie rule."""
    n = x.shape[-1]
    idx = torch.arange(n, device=x.device).expand_as(x)
    return torch.where(x == x.amax(-1, keepdim=True), idx, torch.full_like(idx, n)).amin(-1)


def ce_fwd_bwd(logits, target, loss_mask, seg_off, coef=None):
    """dict: ce (T, 8) = logsumexp(head) - x[target] (a target outside its head scores a logit of 0), argmax (T, 8) int64 (first
    maximum), terms (3, T, 8) = {ce * m, m, [argmax == target] * m} whose sums over T are the kernel's `sums`, and, with coef (8),
    dlogits (T, V) = coef[i] * m[t, i] * (softmax - onehot) and gscale (T, 8) = |coef[i] * m[t, i]|."""
    T = logits.shape[0]
    ce = torch.zeros(T, 8, dtype=logits.dtype, device=logits.device)
    am = torch.zeros(T, 8, dtype=torch.int64, device=logits.device)
    dl = torch.zeros_like(logits) if coef is not None else None
    for i in range(8):
        o, n = seg_off[i], seg_off[i + 1] - seg_off[i]
        x = logits[:, o:o + n]
        mx = x.amax(-1, keepdim=True)
        e = torch.exp(x - mx)
        se = e.sum(-1, keepdim=True)
        tgt = target[:, i]
        ok = (tgt >= 0) & (tgt < n)
        xt = torch.where(ok, x.gather(1, tgt.clamp(0, n - 1)[:, None])[:, 0], torch.zeros_like(mx[:, 0]))
        ce[:, i] = torch.log(se[:, 0]) + mx[:, 0] - xt
        am[:, i] = first_argmax(x)
        if coef is not None:
            onehot = (torch.arange(n, device=x.device)[None, :] == tgt[:, None]).to(x.dtype)
            dl[:, o:o + n] = (coef[i] * loss_mask[:, i])[:, None] * (e / se - onehot)
    m = loss_mask.to(logits.dtype)
    terms = torch.stack([ce * m, m, (am == target).to(logits.dtype) * m])
    out = dict(ce=ce, argmax=am, terms=terms, dlogits=dl)
    if coef is not None:
        out['gscale'] = (coef[None, :] * m).abs()
    return out


def loss_coef(counts, w, scale=1.0):
    """coef[i] = scale * w[i] / (sum(w) * counts[i])."""
    return scale * w / (w.sum() * counts)


# ---------------------------------------------------------------- optimizer
def clip_coef(sq, max_norm, gscale):
    """min(1, max_norm / (sqrt(sq) * gscale + 1e-6)) * gscale."""
    r = max_norm / (torch.sqrt(sq) * gscale + 1e-6)
    return torch.clamp(r, max=1.0) * gscale


def adamw_step(p, g, m, v, clip, lr, beta1, beta2, eps, weight_decay, step):
    """One HF-AdamW step (the header of csrc/pb_optim.hip), out of place: returns the new p, m, v. clip: a scalar factor on g or None."""
    if clip is not None:
        g = g * clip
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    step_size = lr * (1.0 - beta2 ** step) ** 0.5 / (1.0 - beta1 ** step)
    p = p - step_size * m / (torch.sqrt(v) + eps)
    p = p - lr * weight_decay * p
    return p, m, v
