"""numpy restatement of csrc/et_tsne.hip (sklearn's Barnes-Hut t-SNE pipeline with exact repulsion).

knn / perplexity search / symmetrisation follow sklearn's types and orders (so they can be pinned to G18 bit for bit);
kl_grad sums the repulsion in fp64 over all pairs (a more accurate reference for the kernel's fp32-chunked sums);
update is sklearn's _gradient_descent step with numpy 2 promotion, which the kernel reproduces bit for bit."""
import math

import numpy as np

FLT_MIN = np.float32(np.finfo(np.float32).tiny)


def n_neighbors(n, perplexity=30.0):
    return min(n - 1, int(3.0 * perplexity + 1))


def knn(X, k):
    """-> idx (N,k) int32 and squared distances (N,k) fp32 in column order; neighbours by (fp64 rdist, index)."""
    X = np.asarray(X, np.float32)
    n = X.shape[0]
    r = np.zeros((n, n))
    for c in range(X.shape[1]):
        t = X[:, None, c].astype(np.float64) - X[None, :, c]  # fp64 differences of the fp32 inputs, summed in fp64
        r = r + t * t
    np.fill_diagonal(r, np.inf)
    order = np.lexsort((np.broadcast_to(np.arange(n), (n, n)), r), axis=1)[:, :k]
    idx = np.sort(order, axis=1)
    rd = np.take_along_axis(r, idx, axis=1)
    d = np.sqrt(rd)
    return idx.astype(np.int32), (d * d).astype(np.float32)


def binary_search_perplexity(d32, perplexity=30.0, exp=np.exp):
    """sklearn.manifold._utils._binary_search_perplexity, all rows at once (per-row state, j-ordered sums)."""
    d32 = np.asarray(d32, np.float32)
    n, k = d32.shape
    dd = d32.astype(np.float64)
    desired = math.log(float(np.float32(perplexity)))
    tol, eps = float(np.float32(1e-5)), float(np.float32(1e-8))
    beta = np.ones(n)
    bmin, bmax = np.full(n, -np.inf), np.full(n, np.inf)
    P = np.zeros((n, k))
    act = np.ones(n, bool)
    for _ in range(100):
        a = np.nonzero(act)[0]
        if a.size == 0:
            break
        Pa = exp((-d32[a]).astype(np.float64) * beta[a, None])
        s = np.zeros(a.size)
        for j in range(k):
            s = s + Pa[:, j]
        s[s == 0.0] = eps
        Pa = Pa / s[:, None]
        sd = np.zeros(a.size)
        for j in range(k):
            sd = sd + dd[a, j] * Pa[:, j]
        P[a] = Pa
        ent = np.log(s) + beta[a] * sd
        diff = ent - desired
        done = np.abs(diff) <= tol
        up = ~done & (diff > 0)
        dn = ~done & ~(diff > 0)
        b = beta[a].copy()
        bmin[a[up]] = b[up]
        b[up] = np.where(bmax[a[up]] == np.inf, b[up] * 2.0, (b[up] + bmax[a[up]]) / 2.0)
        bmax[a[dn]] = b[dn]
        b[dn] = np.where(bmin[a[dn]] == -np.inf, b[dn] / 2.0, (b[dn] + bmin[a[dn]]) / 2.0)
        beta[a] = b
        act[a[done]] = False
    return P


def _pairwise_block(a):
    n = len(a)
    if n < 8:
        res = -0.0
        for v in a:
            res = res + v
        return res
    r = [float(v) for v in a[:8]]
    i = 8
    while i < n - (n % 8):
        for u in range(8):
            r[u] = r[u] + float(a[i + u])
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for v in a[i:]:
        res = res + float(v)
    return res


def pairwise_sum(a):
    """numpy's pairwise summation of a contiguous fp64 array, restated."""
    n = len(a)
    if n <= 128:
        return _pairwise_block(a)
    n2 = n // 2
    n2 -= n2 % 8
    return pairwise_sum(a[:n2]) + pairwise_sum(a[n2:])


def symmetrize(idx, pc):
    """P = P_cond + P_cond^T as canonical CSR (zero sums dropped), divided by max(total, eps) as scipy's P /= s does:
    -> indptr, indices, P (fp64), total."""
    n, k = idx.shape
    rows = np.concatenate([np.repeat(np.arange(n), k), idx.ravel()])
    cols = np.concatenate([idx.ravel(), np.repeat(np.arange(n), k)])
    vals = np.concatenate([pc.ravel(), pc.ravel()])
    key = rows.astype(np.int64) * n + cols
    order = np.argsort(key, kind="stable")
    key, vals = key[order], vals[order]
    uk, first = np.unique(key, return_index=True)
    sums = vals[first].copy()
    dup = np.nonzero(np.diff(key) == 0)[0]  # each pair appears at most twice: forward + reverse
    sums[np.searchsorted(uk, key[dup])] = vals[dup] + vals[dup + 1]
    keep = sums != 0.0
    uk, sums = uk[keep], sums[keep]
    r, c = uk // n, (uk % n).astype(np.int32)
    indptr = np.zeros(n + 1, np.int64)
    np.add.at(indptr, r + 1, 1)
    indptr = np.cumsum(indptr)
    rowsum = np.zeros(n)
    lens = np.diff(indptr)
    for t in range(int(lens.max())):
        m = lens > t
        rowsum[m] = rowsum[m] + sums[indptr[:-1][m] + t]
    total = pairwise_sum(rowsum)
    P = sums * (1.0 / max(total, np.finfo(np.float64).eps))
    return indptr.astype(np.int32), c, P, total


def kl_grad(Y, indptr, indices, P32):
    """KL and gradient with exact repulsion: attraction and KL over the CSR entries, repulsion over all j whose fp32
    position differs from i's in at least one coordinate (sklearn's compiled tree leaves out exactly coincident points
    only), in fp64; Z = max(Z, DBL_EPSILON) as sklearn clamps sum_Q."""
    Y = np.asarray(Y, np.float32)
    y = Y.astype(np.float64)
    n = Y.shape[0]
    diff = y[:, None, :] - y[None, :, :]
    q = 1.0 / (1.0 + (diff ** 2).sum(-1))
    q[np.all(diff == 0.0, axis=-1)] = 0.0  # j = i and exactly coincident points
    Z = max(q.sum(), np.finfo(np.float64).eps)
    neg = ((q * q)[:, :, None] * diff).sum(1)
    r = np.repeat(np.arange(n), np.diff(indptr))
    b = y[r] - y[indices]
    qe = 1.0 / (1.0 + (b ** 2).sum(-1))
    p = np.asarray(P32, np.float32).astype(np.float64)
    pos = np.zeros((n, 2))
    np.add.at(pos, r, (p * qe)[:, None] * b)
    kl = float(np.sum(p * np.log(np.maximum(p, FLT_MIN) / np.maximum(qe / Z, FLT_MIN))))
    return kl, (4.0 * (pos - neg / Z)).astype(np.float32)


def edge_embeddings(n, seed):
    """seeded (n,2) fp32 embeddings at the coincidence edges (n even): name -> Y.  `dup`: the second half repeats the
    first exactly; `d1e-7`, `d9e-7`, `d2e-6`: the second half is the first moved by that much in both coordinates (std 0.5,
    so that fp32 keeps the offsets: the tool and the tests assert what the differences are); `pca`: std 1e-4, the scale
    of init="pca"; `eq0`, `eqc`: all points at the origin / at one other point."""
    rng = np.random.default_rng(seed)
    h = n // 2
    base = (rng.standard_normal((n, 2)) * 0.5).astype(np.float32)
    out = {}
    y = base.copy()
    y[h:2 * h] = y[:h]
    out["dup"] = y
    for name, delta in (("d1e-7", 1e-7), ("d9e-7", 9e-7), ("d2e-6", 2e-6)):
        y = base.copy()
        y[h:2 * h] = (y[:h].astype(np.float64) + delta).astype(np.float32)
        out[name] = y
    out["pca"] = (rng.standard_normal((n, 2)) * 1e-4).astype(np.float32)
    out["eq0"] = np.zeros((n, 2), np.float32)
    out["eqc"] = np.tile(np.float32([0.3, -0.7]), (n, 1))
    return out


def pair_offsets(Y):
    """max-norm offsets |y_i - y_{i+n/2}| of the paired halves of an edge embedding (fp32 differences, as the kernel forms)"""
    h = Y.shape[0] // 2
    return np.abs(Y[h:2 * h] - Y[:h]).max(-1), np.abs(Y[h:2 * h] - Y[:h]).min(-1)


def update(p, upd, gains, grad, momentum, lr):
    """sklearn's _gradient_descent step (numpy 2 semantics): returns new (p fp32, update fp64, gains fp32, grad fp32)."""
    p, gains, grad = p.astype(np.float32).copy(), gains.astype(np.float32).copy(), grad.astype(np.float32).copy()
    inc = upd * grad < 0.0
    dec = np.invert(inc)
    gains[inc] += 0.2
    gains[dec] *= 0.8
    np.clip(gains, 0.01, np.inf, out=gains)
    grad *= gains
    upd = momentum * upd - np.float64(lr) * grad
    p += upd
    return p, upd, gains, grad


def phase_p(P64, ee, phase2):
    """the fp32 P of a phase: fp32(P * ee), or fp32((P * ee) / ee) after sklearn's P /= early_exaggeration."""
    x = P64 * ee
    return (x / ee if phase2 else x).astype(np.float32)


def optimize(Y0, indptr, indices, P64, ee=12.0, lr=None, iters=1000, max_iter=1000):
    """sklearn's TSNE._tsne schedule with kl_grad; stops after `iters` iterations (for prefix comparisons)."""
    n = Y0.shape[0]
    lr = np.maximum(n / ee / 4, 50) if lr is None else lr
    p = np.asarray(Y0, np.float32).ravel().copy()
    i = 0
    for ph, (start, end, mom) in enumerate(((0, 250, 0.5), (250, max_iter, 0.8))):
        P32 = phase_p(P64, ee, ph == 1)
        upd, gains = np.zeros(2 * n), np.ones(2 * n, np.float32)
        for i in range(start, min(end, iters)):
            _, g = kl_grad(p.reshape(n, 2), indptr, indices, P32)
            p, upd, gains, _ = update(p, upd, gains, g.ravel(), mom, lr)
    return p.reshape(n, 2)


def pca_init(X):
    """sklearn's init="pca" up to rounding: top-2 principal axes, svd_flip signs, PC1 scaled to std 1e-4."""
    X = np.asarray(X, np.float64)
    Xc = X - X.mean(0)
    w, V = np.linalg.eigh(Xc.T @ Xc)
    V = V[:, ::-1][:, :2]
    s = np.sign(V[np.argmax(np.abs(V), axis=0), range(2)])
    V = V * s
    Y = (Xc @ V).astype(np.float32)
    return Y / np.std(Y[:, 0]) * 1e-4


def trustworthiness(X, Y, k=10):
    """sklearn.manifold.trustworthiness (squared Euclidean ranks in both spaces)."""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    n = X.shape[0]
    dx = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(dx, np.inf)
    ind_x = np.argsort(dx, axis=1)
    dy = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(dy, np.inf)
    ind_y = np.argsort(dy, axis=1)[:, :k]
    ranks = np.zeros((n, n), np.int64)
    ranks[np.arange(n)[:, None], ind_x] = np.arange(1, n + 1)[None, :]
    r = ranks[np.arange(n)[:, None], ind_y] - k
    t = np.sum(r[r > 0])
    return 1.0 - t * (2.0 / (n * k * (2.0 * n - 3.0 * k - 1.0)))


def libm_exp(a):
    """exp through the C library, element by element (sklearn's perplexity search calls libm's exp)."""
    return np.frompyfunc(math.exp, 1, 1)(a).astype(np.float64)


# ---- the coincidence edges (tests/golden/g18c_tsne_edges.npz): case names and the bounds both test modules hold
EDGE_NAMES = ["dup", "d1e-7", "d9e-7", "d2e-6", "pca", "eq0", "eqc"]
N2_P = (np.int32([0, 1, 2]), np.int32([1, 0]), np.float32([0.5, 0.5]))  # the only symmetric P of two points


def check_kl_grad(kl, g, kl_ref, g_ref, all_equal):
    """the project's bounds: 5e-5 of max |grad|, 1e-5 relative KL.  All points equal: the gradient is exactly 0 and the KL
    only not NaN (sklearn's own value there is finite at N = 2 and 300 and -inf at N = 2 000)."""
    if all_equal:
        assert not np.any(g_ref) and not np.any(g) and not np.isnan(kl)
        return
    assert np.abs(g - g_ref).max() <= 5e-5 * np.abs(g_ref).max(), (np.abs(g - g_ref).max(), np.abs(g_ref).max())
    assert abs(kl - kl_ref) <= 1e-5 * abs(kl_ref), (kl, kl_ref)


def check_n2_far(kl, g, Y):
    """two distinct points: P = Q = 1/2 whatever the distance, so KL and gradient are 0 and what any fp32 evaluation
    returns is the rounding of two cancelling forces of size F = 4 p q |y_0 - y_1| (sklearn's record: 2.2e-8 F).  A bound
    relative to max |grad| is a bound relative to noise here; held instead to 2^-22 F (the forces are sums of two
    products rounded to 2^-24 each), and |KL| to 2^-22 (sum p = 1, log of a ratio within 2^-23 of 1)."""
    d = Y[0].astype(np.float64) - Y[1]
    F = 4 * 0.5 / (1.0 + d @ d) * np.abs(d).max()
    assert np.abs(g).max() <= 2.0 ** -22 * F, (np.abs(g).max(), F)
    assert abs(kl) <= 2.0 ** -22, kl
