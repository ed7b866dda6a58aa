"""RegMean merging restated from its formulas, for tests/test_regmean_*.py:

    W^T = (sum_m G'_m)^-1 sum_m G'_m W_m^T,   G'_m = G_m * F,   F = off off the diagonal and diag on it,
    off = float32(ratio), diag = float32(float32(1 - ratio) + float32(ratio))

once in float64 (the truth the tests measure against) and once as the float32 recipe a CPU framework runs (scale, sum, matmul,
inverse, matmul): the yardstick for how far a correct float32 computation is from that truth."""
import numpy as np
import torch


def factors(ratio):
    """(off, diag) as float32 numbers."""
    off = np.float32(ratio)
    return off, np.float32(np.float32(np.float32(1.0) - off) + off)


def scale32(G, ratio):
    """G * F in float32 (one multiplication per element)."""
    off, diag = factors(ratio)
    K = G.shape[0]
    F = torch.full((K, K), float(off), dtype=torch.float32)
    F.fill_diagonal_(float(diag))
    return G * F


def scale64(G, ratio):
    off, diag = factors(ratio)
    K = G.shape[0]
    F = torch.full((K, K), float(off), dtype=torch.float64)
    F.fill_diagonal_(float(diag))
    return G.double() * F


def merge64(Ws, Gs, ratio=1.0):
    """The merged (out, K) weight in float64 from per-model (out, K) weights and (K, K) Gram matrices."""
    S = sum(scale64(G, ratio) for G in Gs)
    R = sum(scale64(G, ratio) @ W.double().t() for G, W in zip(Gs, Ws))
    return torch.linalg.solve(S, R).t()


def merge32_recipe(Ws, Gs, ratio=1.0):
    """The float32 recipe: scaled matrices summed, products summed, inverse, product, transpose."""
    scaled = [scale32(G, ratio) for G in Gs]
    S = sum(scaled)
    R = sum(torch.matmul(G, W.t()) for G, W in zip(scaled, Ws))
    return torch.matmul(torch.inverse(S), R).t()


def eta(S, Z, R):
    """The normwise residual ||S Z - R||_F / (||S||_F ||Z||_F + ||R||_F) in float64."""
    S, Z, R = S.double(), Z.double(), R.double()
    return float(torch.linalg.norm(S @ Z - R) / (torch.linalg.norm(S) * torch.linalg.norm(Z) + torch.linalg.norm(R)))


def gram_inputs(K, T, n_models, seed):
    """n_models Gram matrices X^T X / T (float32, exactly symmetric) of (T, K) activations ~ N(0.5, 1) rounded to bf16."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n_models):
        X = (torch.randn(T, K, generator=g) + 0.5).bfloat16().double()
        out.append((X.t() @ X / T).float())
    return out


def solve_case(K, nrhs, T, ratio, seed):
    """(S, R) float32: S = sum_{m<3} scale(X_m^T X_m / T), R = sum_m G'_m W_m^T with W_m ~ 0.05 N(0, 1) of shape (nrhs, K)."""
    Gs = [scale32(G, ratio) for G in gram_inputs(K, T, 3, seed)]
    g = torch.Generator().manual_seed(seed + 1)
    Ws = [0.05 * torch.randn(nrhs, K, generator=g) for _ in Gs]
    return sum(Gs), sum(torch.matmul(G, W.t()) for G, W in zip(Gs, Ws))


def yardsticks(S, R):
    """(eta of inverse(S) @ R, eta of LAPACK's float32 Cholesky factor and solve) on the CPU."""
    z_inv = torch.matmul(torch.inverse(S), R)
    z_chol = torch.cholesky_solve(R, torch.linalg.cholesky(S))
    return eta(S, z_inv, R), eta(S, z_chol, R)
