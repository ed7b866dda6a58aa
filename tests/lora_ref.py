"""References for the LoRA tests: float64 / int64 restatements of the four operations of csrc/pb_lora.hip, their per-element error bounds,
and the oracle (oracle/pianobart_oracle.py, unchanged) evaluated on merged weights W + s B A built from leaf tensors A and B, so that
autograd gives the oracle's dA, dB and head gradients."""
import torch

U = 2.0 ** -24        # the unit of the bounds: (n + 2) U sum |a b| for an f32 accumulation of n terms in any order, one scale and one add


def _wide(t):
    return t.detach().cpu().to(torch.int64 if not t.is_floating_point() else torch.float64)


def _mm(a, b, integer):
    if integer:
        return a.to(torch.int64) @ b.to(torch.int64)
    return a.to(torch.float64) @ b.to(torch.float64)


def down(X, W, alpha, w_kr, integer=False):
    """T = alpha X W^T, W (r, K) or (K, r) with w_kr. X already cut to the (M, K) slice. integer: int64 arithmetic (alpha must be an integer)."""
    X, W = X.detach().cpu(), W.detach().cpu()
    Wt = W if w_kr else W.t()
    out = _mm(X, Wt, integer)
    mag = X.double().abs() @ Wt.double().abs()
    return (out * int(alpha) if integer else out * float(alpha)), mag * abs(float(alpha))


def up_term(T, W, alpha, w_nr, integer=False):
    """alpha T W, W (r, N) or (N, r) with w_nr: the term added to the Y slice."""
    T, W = T.detach().cpu(), W.detach().cpu()
    Wn = W.t() if w_nr else W
    out = _mm(T, Wn, integer)
    mag = T.double().abs() @ Wn.double().abs()
    return (out * int(alpha) if integer else out * float(alpha)), mag * abs(float(alpha))


def wgrad(T, X, alpha, g_cr, integer=False):
    """G = alpha T^T X as (r, C), or its transpose (C, r) with g_cr."""
    T, X = T.detach().cpu(), X.detach().cpu()
    out = _mm(T.t(), X, integer)
    mag = T.double().abs().t() @ X.double().abs()
    out = out * int(alpha) if integer else out * float(alpha)
    mag = mag * abs(float(alpha))
    return (out.t(), mag.t()) if g_cr else (out, mag)


def merge_term(B, A, alpha):
    """alpha B A in float64 and sum |alpha| |B| |A|."""
    B, A = B.detach().cpu().double(), A.detach().cpu().double()
    return (B @ A) * float(alpha), (B.abs() @ A.abs()) * abs(float(alpha))


def bound(n, mag, result=None, bf16=False):
    """(n + 2) 2^-24 sum |a b| per element, plus 2^-8 |result| for the one final rounding of a bf16 read-modify-write."""
    b = (n + 2) * U * mag
    if bf16:
        b = b + 2.0 ** -8 * result.abs()
    return b


# ---- the oracle on merged weights ---------------------------------------------------------------------------------------------------------
def oracle_forward(o, base, adapters, scale, enc, dec, emask, dmask, heads=None):
    """Logits (list of 8) of oracle model `o` with the weights named by `adapters` replaced by base[name] + scale * B @ A.
    base: {parameter name: tensor} of the whole oracle model (detached); adapters: {weight name: (A, B)} with A, B leaf tensors (float32 or
    float64, requires_grad as the caller wants); heads: {name: leaf tensor} replacing mask_lm.* parameters (so that they take a gradient)."""
    from torch.func import functional_call
    params = {}                              # only the adapted weights are replaced (the oracle's tied embedding tables stay the module's own)
    for name, (A, B) in adapters.items():
        params[name] = base[name] + scale * (B @ A).to(base[name].dtype)
    if heads:
        params.update(heads)
    return functional_call(o, params, (enc, dec, emask, dmask))
