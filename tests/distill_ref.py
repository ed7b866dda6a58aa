"""Plain reference of the distillation loss kernel (csrc/pb_distill.hip), written from the formulas of include/pianobart_hip.h with torch
tensor arithmetic only: no softmax / log_softmax / cross_entropy / kl_div call, no autograd. It computes in the dtype of its inputs:
float64 inputs give the reference, float32 inputs the "plain float32 evaluation of the same formula" whose own error sets the bounds of
tests/test_distill_kernels_gpu.py. tests/test_distill_cpu.py checks the float64 form against float64 torch.autograd.
"""
import torch

from tests.row_ref import first_argmax


def _log_softmax(x):
    """(log softmax, softmax) of the last axis, the maximum subtracted."""
    s = x - x.amax(-1, keepdim=True)
    e = torch.exp(s)
    se = e.sum(-1, keepdim=True)
    return s - torch.log(se), e / se


def distill_fwd_bwd(logits, teacher, target, loss_mask, seg_off, coef=None, alpha=0.0, tau=1.0, eps=0.0, t_row=None):
    """Per row t and head i of n classes, z / u the student's / teacher's logits (teacher row t_row[t], or t), y = target, m = loss mask:
      hard   = -log p[y]                        p = softmax(z); a target outside its head scores a logit of 0 and has no one-hot column
      hard_e = (1 - eps) hard - (eps / n) sum_c log p[c]
      kl     = sum_c q[c] (log q[c] - log p_tau[c])        p_tau = softmax(z / tau), q = softmax(u / tau); q == 0 counts as 0
      loss   = (1 - alpha) hard_e + alpha tau^2 kl
      dz[c]  = coef[i] m ((1 - alpha) (p[c] - (1 - eps) [c == y] - eps / n) + alpha tau (p_tau[c] - q[c]))
    teacher None: kl = 0 and no soft gradient (alpha must be 0).
    dict: loss / hard / kl (T, 8), argmax (T, 8) int64 (first maximum), terms (5, T, 8) = {loss m, m, [argmax == y] m, hard m, kl m} whose
    sums over T are the kernel's `sums`, kl_abs (T, 8) = m sum_c q (|log q| + |log p_tau|) (the magnitude of what the KL is the difference
    of), and, with coef (8), dlogits (T, V) and gscale (T, 8) = |coef[i] m|."""
    T = logits.shape[0]
    dt, dev = logits.dtype, logits.device
    z8 = lambda: torch.zeros(T, 8, dtype=dt, device=dev)
    hard, loss, kl, kl_abs = z8(), z8(), z8(), z8()
    am = torch.zeros(T, 8, dtype=torch.int64, device=dev)
    dl = torch.zeros_like(logits) if coef is not None else None
    if teacher is not None and t_row is not None:
        teacher = teacher[t_row.long()]
    if teacher is None and alpha != 0:
        raise ValueError('alpha > 0 needs teacher logits')
    for i in range(8):
        o, n = seg_off[i], seg_off[i + 1] - seg_off[i]
        x = logits[:, o:o + n]
        lp, p = _log_softmax(x)
        tgt = target[:, i]
        ok = (tgt >= 0) & (tgt < n)
        mx = x.amax(-1)
        lse = torch.log(torch.exp(x - mx[:, None]).sum(-1)) + mx
        xt = torch.where(ok, x.gather(1, tgt.clamp(0, n - 1)[:, None])[:, 0], torch.zeros_like(mx))
        hard[:, i] = lse - xt
        hard_e = (1.0 - eps) * hard[:, i] - (eps / n) * lp.sum(-1) if eps != 0 else hard[:, i]
        am[:, i] = first_argmax(x)
        soft = None
        if teacher is not None:
            lpt, pt = _log_softmax(x / tau)
            lq, q = _log_softmax(teacher[:, o:o + n] / tau)
            live = q > 0
            kl[:, i] = torch.where(live, q * (lq - lpt), torch.zeros_like(q)).sum(-1)
            kl_abs[:, i] = torch.where(live, q * (lq.abs() + lpt.abs()), torch.zeros_like(q)).sum(-1)
            soft = pt - q
        loss[:, i] = (1.0 - alpha) * hard_e + (alpha * tau * tau) * kl[:, i]
        if coef is not None:
            onehot = (torch.arange(n, device=dev)[None, :] == tgt[:, None]).to(dt)
            g = (1.0 - alpha) * (p - (1.0 - eps) * onehot - eps / n)
            if soft is not None:
                g = g + (alpha * tau) * soft
            dl[:, o:o + n] = (coef[i] * loss_mask[:, i])[:, None] * g
    m = loss_mask.to(dt)
    terms = torch.stack([loss * m, m, (am == target).to(dt) * m, hard * m, kl * m])
    out = dict(loss=loss, hard=hard, kl=kl, argmax=am, terms=terms, kl_abs=kl_abs * m, dlogits=dl)
    if coef is not None:
        out['gscale'] = (coef[None, :] * m).abs()
    return out
