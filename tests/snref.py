"""Spectral normalisation in fp64 (numpy), written from its statement.  For W [R, C] (a weight reshaped so that C = cout) and the
persistent state u [C], one refresh with `iteration` = k is, k times,

    v_ = u W^T      v = v_ / sqrt(max(sum v_^2, 1e-12))
    u_ = v W        u = u_ / sqrt(max(sum u_^2, 1e-12))

then, with the final u, v taken as constants,  sigma = v W u^T,  Wbar = W / sigma,  and u is stored back.  The pull-back of
G = dL/dWbar to dL/dW follows from Wbar_ij = W_ij / sigma and d sigma / d W_ij = v_i u_j:

    dL/dW = G / sigma - <G, W> v^T u / sigma^2 = (G - <G, Wbar> v^T u) / sigma

The a-priori bounds at the end say how far an f32 evaluation of the same sums -- in ANY order -- can be from these values: a sum of
n f32 products carries at most gamma_n * sum |terms|, gamma_n = n eps / (1 - n eps), eps = 2^-24 (Higham, Accuracy and Stability of
Numerical Algorithms, section 3.1); eight further roundings (products, the square root, the quotients, conversions) are allowed for by
n + 8, and the bounds of the sums are carried through the later sums and quotients term by term."""
import numpy as np

CLAMP = 1e-12
EPS32 = 2.0 ** -24


def _normalise(x):
    return x / np.sqrt(max(float(np.sum(x * x)), CLAMP))


def refresh(w, u, iteration=1):
    """w [R, C], u [C] (any float arrays; computed in fp64) -> dict(u, v, sigma, wbar) plus the sums of the LAST iteration:
    t = W u_in^T, s = W^T t, T = sum t^2, S = sum s^2, u_in (the u that iteration started from)."""
    w = np.asarray(w, np.float64)
    u = np.asarray(u, np.float64).reshape(-1)
    assert w.ndim == 2 and u.shape[0] == w.shape[1] and iteration >= 1
    for _ in range(int(iteration)):
        u_in = u
        t = w @ u
        v = _normalise(t)
        u = _normalise(v @ w)
    s = t @ w
    sigma = float(v @ w @ u)
    with np.errstate(divide='ignore', invalid='ignore'):      # (sigma = 0 is not protected against)
        wbar = w / sigma
    return dict(u=u, v=v, sigma=sigma, wbar=wbar, t=t, s=s, T=float(np.sum(t * t)), S=float(np.sum(s * s)), u_in=u_in)


def pullback(g, wbar, u, v, sigma):
    """(G - <G, Wbar> v^T u) / sigma in fp64; g, wbar [R, C], u [C], v [R] (not necessarily normalised)."""
    g, wbar = np.asarray(g, np.float64), np.asarray(wbar, np.float64)
    u, v = np.asarray(u, np.float64).reshape(-1), np.asarray(v, np.float64).reshape(-1)
    return (g - float(np.sum(g * wbar)) * np.outer(v, u)) / float(sigma)


def weight_matrix(w):
    """[..., cout] -> [R, cout], the reference's reshape."""
    w = np.asarray(w)
    return w.reshape(-1, w.shape[-1])


def gamma(n):
    return n * EPS32 / (1.0 - n * EPS32)


def refresh_bounds(w, u):
    """Absolute error bounds (fp64 arrays / floats) of ONE f32 iteration from the f32 values w, u: dict(u, v, sigma, wbar).
    Valid while no clamp engages (T, S far above 1e-12), which the function asserts."""
    w = np.asarray(w, np.float64)
    u = np.asarray(u, np.float64).reshape(-1)
    rows, cols = w.shape
    aw = np.abs(w)
    r = refresh(w, u, 1)
    t, s, T, S = r['t'], r['s'], r['T'], r['S']
    et = gamma(cols + 8) * (aw @ np.abs(u))                                   # t_r = sum_c W_rc u_c
    at = np.abs(t) + et                                                        # what the computed |t_r| can be
    eT = float(np.sum(2 * np.abs(t) * et + et * et) + gamma(rows + 8) * np.sum(at * at))
    es = et @ aw + gamma(rows + 8) * (at @ aw)                                 # s_c = sum_r W_rc t_r, from the computed t
    a_s = np.abs(s) + es
    eS = float(np.sum(2 * np.abs(s) * es + es * es) + gamma(cols + 8) * np.sum(a_s * a_s))
    assert T - eT > 1e-6 and S - eS > 1e-6, 'the bounds assume that no clamp is near'
    rel_t = 0.5 * eT / (T - eT) + gamma(8)                                     # of sqrt(T)
    rel_s = 0.5 * eS / (S - eS) + gamma(8)                                     # of sqrt(S)
    rel_sigma = rel_t + rel_s + gamma(8)                                       # sigma = sqrt(S) / sqrt(T)
    slack = 1.0 + 1e-3                                                         # the second-order terms dropped above
    return dict(v=slack * (et / np.sqrt(T) + np.abs(r['v']) * (rel_t + gamma(8))),
                u=slack * (es / np.sqrt(S) + np.abs(r['u']) * (rel_s + gamma(8))),
                sigma=slack * abs(r['sigma']) * rel_sigma,
                wbar=slack * np.abs(r['wbar']) * (rel_sigma + gamma(8)))


def pullback_bound(g, wbar, u, v, sigma):
    """Absolute error bound of an f32 pull-back from the f32 values it is given."""
    g, wbar = np.asarray(g, np.float64), np.asarray(wbar, np.float64)
    u, v = np.asarray(u, np.float64).reshape(-1), np.asarray(v, np.float64).reshape(-1)
    d = float(np.sum(g * wbar))
    ed = gamma(g.size + 8) * float(np.sum(np.abs(g * wbar)))
    vu = np.abs(np.outer(v, u))
    return (ed * vu + gamma(8) * (np.abs(g) + (abs(d) + ed) * vu)) / abs(float(sigma))
