"""float64 restatement (plain torch on the CPU) of the training form of one wrapper call on one scene --
EigenTrajectory/model.py:73-123 with normalizer.py:17-62 -- the arithmetic csrc/et_train.hip is checked against, plus the
seeded inputs of those checks.  Not a test module itself, and it uses none of the project's kernels or formulas: the
rotation comes from atan2 / cos / sin as in normalizer.py:24-26, the minima and their gradient from ``.min(dim)`` and
torch autograd in float64.

Next to every dot product it returns ``M``, the sum of the absolute values of its terms, the scale of the fp32 error
bound ``(n + 8) * 2**-24 * M`` of an n-term FMA dot product (8: the roundings of normalise / denormalise around it).
"""
import functools
from types import SimpleNamespace as NS

import numpy as np
import torch

F64 = torch.float64
U32 = 2.0 ** -24      # unit roundoff of fp32
TAU = 1e-4            # a row-term is undecided when (second smallest - smallest) < TAU * max(1, smallest)
STATIC_DIST = 0.4
TERMS = ("eigentraj", "ade", "fde")


def _t(a):
    return None if a is None else torch.as_tensor(np.asarray(a)).to(F64)


# ------------------------------------------------------------------------------------------------ normaliser state
def row_state(nrm, mode, static_dist):
    """nrm (4,N) fp32 = (ox, oy, dx, dy) with d = obs[-1] - obs[-3] -> the normaliser of every row (normalizer.py:17-29)
    in float64: ox, oy, c, s, sca (N,), mv (N,) bool, margin (N,) = | ||d/2|| - static_dist |.  mode: 0 static, 1 moving,
    2 split by model.py:73, 3 identity (no normalisation).  The split decision is taken in fp32 like row_norm's."""
    nrm = np.asarray(nrm, np.float32)
    n = nrm.shape[1]
    hx, hy = nrm[2] * np.float32(0.5), nrm[3] * np.float32(0.5)
    half = np.sqrt(hx * hx + hy * hy)                       # fp32, one rounding per operation
    if mode == 2:
        mv = half > np.float32(static_dist)
    else:
        mv = np.full((n,), mode == 1)
    margin = np.abs(half.astype(np.float64) - float(np.float32(static_dist)))
    d = _t(nrm[2:4])
    mvt = torch.from_numpy(mv)
    if mode == 3:
        one, zero = torch.ones(n, dtype=F64), torch.zeros(n, dtype=F64)
        return NS(ox=zero, oy=zero, c=one, s=zero, sca=one, mv=mvt, margin=margin)
    theta = torch.atan2(d[1], d[0])                         # normalizer.py:24
    sca = torch.where(mvt, 1.0 / d.norm(dim=0) * 2, torch.ones(n, dtype=F64))  # normalizer.py:28 (inf: motionless)
    return NS(ox=_t(nrm[0]), oy=_t(nrm[1]), c=theta.cos(), s=theta.sin(), sca=sca, mv=mvt, margin=margin)


def _pick(st, a_m, a_s, like):
    """per row: the moving or the static descriptor's array (None = not given; rows that need it then get zeros)"""
    z = torch.zeros_like(like)
    a_m, a_s = (z if a_m is None else a_m), (z if a_s is None else a_s)
    shape = (-1,) + (1,) * like.dim()
    return torch.where(st.mv.view(shape), a_m[None], a_s[None])  # (N, ...)


def _project(traj, st, U_m, U_s):
    """descriptor.py projection of traj (N,T,2): C (k,N) = U^T vec(normalised traj), and M (k,N)"""
    like = U_m if U_m is not None else U_s
    U = _pick(st, U_m, U_s, like)                            # (N, 2T, k)
    tx, ty = traj[..., 0] - st.ox[:, None], traj[..., 1] - st.oy[:, None]
    c, s, sca = st.c[:, None], st.s[:, None], st.sca[:, None]
    a, b = (tx * c + ty * s) * sca, (tx * -s + ty * c) * sca  # normalizer.py:42-51, R = [[c,-s],[s,c]]
    ma, mb = ((tx * c).abs() + (ty * s).abs()) * sca, ((tx * s).abs() + (ty * c).abs()) * sca
    v = torch.stack([a, b], dim=-1).reshape(traj.shape[0], -1)
    mv_ = torch.stack([ma, mb], dim=-1).reshape(traj.shape[0], -1)
    return torch.einsum("ntj,nt->jn", U, v), torch.einsum("ntj,nt->jn", U.abs(), mv_)


def project_train(obs, pred, U_obs_m, U_obs_s, U_pred_m, U_pred_s, mode, static_dist):
    """model.py:73-90, 113-116 for one scene.  obs (N,T_obs,2), pred (N,T_pred,2) fp32; U_* (2T,k) or None.
    -> C_obs (k,N), nrm (4,N), obs_ori (2,N), C_gt (k,N), flag (N) and the M of C_obs, C_gt, obs_ori."""
    obs32, pred32 = np.asarray(obs, np.float32), np.asarray(pred, np.float32)
    last, d = obs32[:, -1], obs32[:, -1] - obs32[:, -3]       # fp32 like normalizer.py:23 on fp32 tensors
    nrm32 = np.ascontiguousarray(np.stack([last[:, 0], last[:, 1], d[:, 0], d[:, 1]]))
    st = row_state(nrm32, mode, static_dist)
    C_obs, M_obs = _project(_t(obs32), st, _t(U_obs_m), _t(U_obs_s))
    C_gt, M_gt = _project(_t(pred32), st, _t(U_pred_m), _t(U_pred_s))
    ori = _t(nrm32[:2])
    mean = ori.mean(dim=1, keepdim=True)
    return NS(C_obs=C_obs, nrm=_t(nrm32), nrm32=nrm32, obs_ori=ori - mean, C_gt=C_gt, flag=st.mv.numpy().astype(np.uint8),
              M_C_obs=M_obs, M_C_gt=M_gt, M_obs_ori=ori.abs() + ori.abs().mean(dim=1, keepdim=True), margin=st.margin)


# ------------------------------------------------------------------------------------------------ losses
def _forward(C, st, A_m, A_s, U_m, U_s, C_gt, gt):
    """-> cp (k,N,S), recon (S,N,T,2), dist (S,N,T), vals 3 x (N,S), Mx / My (S,N,T), U (N,2T,k)"""
    k, n, S = C.shape
    A = _pick(st, A_m, A_s, torch.zeros(k, S, dtype=F64)).permute(1, 0, 2)   # (k,N,S)
    cp = A + C                                                                 # anchor.py:87
    e = (cp - C_gt[:, :, None]).norm(p=2, dim=0)                               # model.py:119 (N,S)
    U = _pick(st, U_m, U_s, U_m if U_m is not None else U_s)                   # (N,2T,k)
    v = torch.einsum("ntj,jns->snt", U, cp).reshape(S, n, -1, 2)               # descriptor.py:86-88
    c, s, sca = st.c[None, :, None], st.s[None, :, None], st.sca[None, :, None]
    x, y = v[..., 0] / sca, v[..., 1] / sca                                    # normalizer.py:53-62, R^T = [[c,s],[-s,c]]
    recon = torch.stack([x * c - y * s + st.ox[None, :, None], x * s + y * c + st.oy[None, :, None]], dim=-1)
    dist = (recon - gt[None]).norm(p=2, dim=-1)                                # model.py:120 (S,N,T)
    vals = [e, dist.mean(dim=-1).T, dist[:, :, -1].T]                          # 3 x (N,S), separate graphs as in model.py
    with torch.no_grad():
        p = torch.einsum("ntj,jns->snt", U.abs(), cp.abs()).reshape(S, n, -1, 2)
        Mx = (p[..., 0] * c.abs() + p[..., 1] * s.abs()) / sca + st.ox.abs()[None, :, None]
        My = (p[..., 0] * s.abs() + p[..., 1] * c.abs()) / sca + st.oy.abs()[None, :, None]
    return cp, recon, dist, vals, Mx, My, U


def _select(vals, arg):
    if arg is None:
        best, arg = vals.min(dim=-1)                  # first minimum; a NaN takes over (model.py:121-123)
    else:
        arg = torch.as_tensor(np.asarray(arg)).long()
        best = vals.gather(-1, arg[..., None])[..., 0]
    return best, arg


def losses(C, nrm, A_m, A_s, U_m, U_s, mode, static_dist, C_gt, gt, arg=None):
    """model.py:98-123 for one scene, from the predictor's output on.  C (k,N,S), nrm (4,N), A_* (k,S) or None,
    U_* (2T,k) or None (the one the mode does not use), C_gt (k,N), gt (N,T,2): fp32 values, taken as exact.
    -> recon (S,N,T,2), best (3,N), arg (3,N), means (3,), gap (3,N) = second smallest - smallest of every row-term,
    and M_recon (S,N,T,2), M_best (3,N), n_best (3,) for the error bounds.  With ``arg`` the minima are read there."""
    st = row_state(nrm, mode, static_dist)
    C, A_m, A_s, U_m, U_s, C_gt, gt = map(_t, (C, A_m, A_s, U_m, U_s, C_gt, gt))
    with torch.no_grad():
        cp, recon, dist, vals, Mx, My, _ = _forward(C, st, A_m, A_s, U_m, U_s, C_gt, gt)
        vals = torch.stack(vals)
        best, arg = _select(vals, arg)
        k, n, S = C.shape
        T = gt.shape[1]
        if S > 1:
            two = torch.topk(vals, 2, dim=-1, largest=False).values
            gap = two[..., 1] - two[..., 0]
        else:
            gap = torch.full((3, n), float("inf"), dtype=F64)
        # error scales at the selected samples: the rounding of cp = A + C enters e through the difference cp - C_gt
        Md = Mx + My + dist                                                     # (S,N,T)
        rows = torch.arange(n)
        M_best = torch.stack([cp.norm(dim=0)[rows, arg[0]] + best[0], Md.mean(dim=-1)[arg[1], rows], Md[:, :, -1][arg[2], rows]])
    return NS(recon=recon, best=best, arg=arg, means=best.mean(dim=1), gap=gap, vals=vals, dist=dist,
              M_recon=torch.stack([Mx, My], dim=-1), M_best=M_best, n_recon=2 * k, n_best=(k, 2 * k + T, 2 * k))


def grad(C, nrm, A_m, A_s, U_m, U_s, mode, static_dist, C_gt, gt, weights=(1.0, 1.0, 1.0), arg=None, g_recon=None):
    """d(sum_i weights[i] * loss_i)/dC (k,N,S) by autograd in float64 through ``.min(dim)[0]`` (or the gather at a
    forced ``arg``); a weight of None: that term is not differentiated.  Also M (k,N,S) -- the sum of absolute terms of
    the chained dots behind every element: the terms of the selected recon point (and of cp - C_gt) over the distance they
    are divided by, pulled back through |R| / sca and |U| -- its length n, and rel (N,): the largest relative fp32
    error bound of a selected distance of the row (the factor 1 + rel of the division).  ``g_recon`` (S,N,T,2): the
    objective also holds (recon * g_recon).sum(), for callers that differentiate through recon_traj itself."""
    st = row_state(nrm, mode, static_dist)
    C, A_m, A_s, U_m, U_s, C_gt, gt = map(_t, (C, A_m, A_s, U_m, U_s, C_gt, gt))
    C = C.clone().requires_grad_(True)
    cp, recon, dist, vals, Mx, My, U = _forward(C, st, A_m, A_s, U_m, U_s, C_gt, gt)
    arg = None if arg is None else torch.as_tensor(np.asarray(arg)).long()
    picks = [_select(v, None if arg is None else arg[i]) for i, v in enumerate(vals)]
    best, arg = [p[0] for p in picks], torch.stack([p[1] for p in picks])
    k, n, S = C.shape
    T = gt.shape[1]
    # (a term that is not differentiated stays out of the graph, like a loss nobody calls backward on)
    total = sum(float(w) * best[i].mean() for i, w in enumerate(weights) if w is not None)
    best = torch.stack([b.detach() for b in best])
    if g_recon is not None:
        g_recon = _t(g_recon)
        total = total + (recon * g_recon).sum()
    dC = torch.zeros_like(C) if isinstance(total, int) else torch.autograd.grad(total, C)[0]
    with torch.no_grad():
        rows = torch.arange(n)
        w = [0.0 if x is None else abs(float(x)) for x in weights]
        M = torch.zeros(k, n, S, dtype=F64)
        rel = torch.zeros(n, dtype=F64)
        e = best[0]
        me = (cp[:, rows, arg[0]].abs() + C_gt.abs()) / e * (w[0] / n)         # (k,N)
        if w[0]:
            M[:, rows, arg[0]] += torch.where((e == 0)[None], torch.zeros_like(me), me)
        c, s, sca = st.c.abs()[:, None], st.s.abs()[:, None], st.sca[:, None]
        Ue, Uo = U[:, 0::2].abs(), U[:, 1::2].abs()                              # (N,T,k)
        if g_recon is not None:
            gx, gy = g_recon[..., 0].abs(), g_recon[..., 1].abs()                # (S,N,T)
            a, b = (gx * c[None] + gy * s[None]) / sca[None], (gx * s[None] + gy * c[None]) / sca[None]
            M += torch.einsum("ntj,snt->jns", Ue, a) + torch.einsum("ntj,snt->jns", Uo, b)
        for i, tsel, scale in ((1, slice(None), w[1] / n / T), (2, slice(T - 1, T), w[2] / n)):
            sel = arg[i]
            d = dist[sel, rows][:, tsel]                                         # (N,t)
            mx = (Mx[sel, rows][:, tsel] + gt[:, tsel, 0].abs()) / d
            my = (My[sel, rows][:, tsel] + gt[:, tsel, 1].abs()) / d
            a, b = (mx * c + my * s) / sca, (mx * s + my * c) / sca              # (N,t)
            a, b = (torch.where(d == 0, torch.zeros_like(x), x) for x in (a, b))
            M[:, rows, sel] += scale * (torch.einsum("ntj,nt->jn", Ue[:, tsel], a) + torch.einsum("ntj,nt->jn", Uo[:, tsel], b))
            err = (2 * k + 8) * U32 * (Mx[sel, rows][:, tsel] + My[sel, rows][:, tsel] + d) / d
            if w[i]:
                rel = torch.maximum(rel, torch.where(d == 0, torch.zeros_like(err), err).amax(dim=1))
    return NS(dC=dC, M=M, n=2 * k + 2 * T, rel=rel, arg=arg, best=best)


def undecided(gap, best, tau=TAU):
    """(3,N) bool: row-terms whose two smallest values are closer than tau * max(1, smallest)"""
    return gap < tau * torch.clamp(best, min=1.0)


# ------------------------------------------------------------------------------------------------ seeded inputs
BASE = (6, 8, 12, 20)
SHAPES = [(n,) + BASE for n in (1, 2, 63, 64, 65, 255, 256, 257, 513, 700)]
SHAPES += [(n,) + s for s in ((1, 3, 1, 1), (4, 8, 12, 2), (16, 5, 7, 37), (32, 32, 32, 3)) for n in (65, 300)]
SHAPES += [(16384, 2, 3, 2, 2)]                     # ET_SCENE_MAX_N: 64 trips of the row loop
NAN_SEED = 3                                        # seed of nan_case()
SEED = {}                                           # shape -> seed where the default one exceeds the cap of undecided row-terms


def _basis(rng, rows, k):
    a = rng.standard_normal((rows, k))
    if rows >= k:
        a = np.linalg.qr(a)[0]                      # orthonormal columns
    else:
        a /= np.sqrt(rows)
    return np.ascontiguousarray(a.astype(np.float32))


@functools.lru_cache(maxsize=None)
def make_case(n, k, t_obs, t_pred, S, seed=None, moving=0.5):
    """Seeded inputs of one scene: coordinates within +-16, |obs[-1] - obs[-3]| / 2 from {0.05, 0.1} (static) or
    [0.8, 3] (moving, a share ``moving`` of the rows) against static_dist 0.4, so every row is >= 0.3 clear of the
    decision.  nrm and C_gt, the inputs of the loss kernels, are this module's own (rounded to fp32): they are known
    without a GPU."""
    if seed is None:
        seed = SEED.get((n, k, t_obs, t_pred, S), 1000 + n + 7 * k + 11 * t_obs + 13 * t_pred + 17 * S)
    rng = np.random.default_rng(seed)
    last = rng.uniform(-10.0, 10.0, (n, 2))
    moving = rng.random(n) < moving
    half = np.where(moving, rng.uniform(0.8, 3.0, n), rng.choice([0.05, 0.1], n))
    ang = rng.uniform(-np.pi, np.pi, n)
    d = 2.0 * half[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    obs = last[:, None, :] + rng.uniform(-3.0, 3.0, (n, t_obs, 2))
    obs[:, -1], obs[:, -3] = last, last - d
    pred = last[:, None, :] + rng.uniform(-4.0, 4.0, (n, t_pred, 2))
    c = NS(n=n, k=k, t_obs=t_obs, t_pred=t_pred, S=S, seed=seed, static_dist=STATIC_DIST,
           obs=np.ascontiguousarray(obs.astype(np.float32)), pred=np.ascontiguousarray(pred.astype(np.float32)),
           U_obs_m=_basis(rng, 2 * t_obs, k), U_obs_s=_basis(rng, 2 * t_obs, k),
           U_pred_m=_basis(rng, 2 * t_pred, k), U_pred_s=_basis(rng, 2 * t_pred, k),
           A_m=(0.5 * rng.standard_normal((k, S))).astype(np.float32), A_s=(0.5 * rng.standard_normal((k, S))).astype(np.float32),
           C=np.ascontiguousarray(rng.standard_normal((k, n, S)).astype(np.float32)))
    return c


def mode_case(mode):
    """the case of the per-mode tests: two waves; in mode 1 every row walks (a slow row under the moving descriptor is
    scaled by 2 / ||d|| = 20..40 on the way in and shrunk as much on the way out: its samples all but coincide in metres,
    and a fifth of its row-terms would be undecided)"""
    return make_case(65, *BASE, seed=106, moving=1.0 if mode == 1 else 0.5)


def loss_inputs(c, mode):
    """-> (nrm32 (4,N), C_gt32 (k,N)) of a case in a mode: the reference's projection, rounded to fp32"""
    p = project_train(c.obs, c.pred, *u_for(c, mode, obs=True), *u_for(c, mode), mode, c.static_dist)
    return p.nrm32, np.ascontiguousarray(p.C_gt.numpy().astype(np.float32))


def u_for(c, mode, obs=False):
    """(U_m, U_s) of a case with the descriptor the mode does not use as None (mode 3 uses the static one)"""
    m, s = (c.U_obs_m, c.U_obs_s) if obs else (c.U_pred_m, c.U_pred_s)
    return (m if mode in (1, 2) else None), (s if mode != 1 else None)


def a_for(c, mode, anchors=True):
    if not anchors:
        return None, None
    return (c.A_m if mode in (1, 2) else None), (c.A_s if mode != 1 else None)


# ------------------------------------------------------------------------------------------------ inputs of the edge cases
def tie_pairs(n):
    """per row: (lower, higher) index of the duplicated sample -- the first one for even rows, a later pair for odd"""
    lo = np.where(np.arange(n) % 2 == 0, 0, 7)
    hi = np.where(np.arange(n) % 2 == 0, 11, 13)
    return lo, hi


def tie_inputs(c):
    """C and anchors with sample `hi` an exact copy of sample `lo` (anchors are per sample, not per row: columns 11
    and 13 copy 0 and 7), and the copied sample pulled towards the target so that it is the minimum of many rows"""
    lo, hi = tie_pairs(c.n)
    A_m, A_s, C = c.A_m.copy(), c.A_s.copy(), c.C.copy()
    for A in (A_m, A_s):
        A[:, 11], A[:, 13] = A[:, 0], A[:, 7]
    _, C_gt = loss_inputs(c, 2)
    rows = np.arange(c.n)
    flag = row_state(loss_inputs(c, 2)[0], 2, c.static_dist).mv.numpy()
    A_lo = np.where(flag[None], A_m[:, lo], A_s[:, lo])
    C[:, rows, lo] = (C_gt - A_lo + 0.05 * C[:, rows, lo]).astype(np.float32)   # close to the target: the row's minimum
    C[:, rows, hi] = C[:, rows, lo]
    return C, A_m, A_s


def zero_distance_inputs():
    """Row 9: sample 3 has A + C == C_gt bit for bit (dyadic values, so the sum is exact in fp32 and in float64).
    Row 40: a static row at the origin heading along +x, U_s with unit columns, integer coefficients: recon[5, 40, T-1]
    == gt[40, T-1] exactly.  -> case, C, A_m, A_s, C_gt, nrm, gt, U_m, U_s, (9, 40)"""
    c = make_case(70, *BASE)
    nrm, C_gt = loss_inputs(c, 2)
    nrm, C_gt, C, gt = nrm.copy(), C_gt.copy(), c.C.copy(), c.pred.copy()
    A_m, A_s = np.round(c.A_m * 8) / 8, np.round(c.A_s * 8) / 8
    U_s = np.zeros_like(c.U_pred_s)
    for j in range(c.k):                                   # column j = unit vector of row 2T - 1 - j
        U_s[2 * c.t_pred - 1 - j, j] = 1.0
    n_e, n_f = 9, 40
    flag = row_state(nrm, 2, c.static_dist).mv.numpy()
    A = A_m if flag[n_e] else A_s
    C[:, n_e, 3] = np.arange(1, c.k + 1) / 4.0
    C_gt[:, n_e] = A[:, 3] + C[:, n_e, 3]
    nrm[:, n_f] = (0.0, 0.0, 0.125, 0.0)                   # static (||d / 2|| = 0.0625), theta = 0, ori = 0
    C[:, n_f, 5] = np.arange(2, c.k + 2)
    y, x = A_s[1, 5] + C[1, n_f, 5], A_s[0, 5] + C[0, n_f, 5]   # recon[5, n_f, T-1] = (cp[1], cp[0])
    gt[n_f, -1] = (y, x)
    return c, C, A_m.astype(np.float32), A_s.astype(np.float32), C_gt, nrm, gt, c.U_pred_m, U_s, (n_e, n_f)


def nan_case():
    """the scene of the NaN test: two waves, walking rows only (see mode_case), a seed with no undecided row-term"""
    return make_case(70, *BASE, seed=NAN_SEED, moving=1.0)


def nan_inputs(c):
    """mode 1 (every row through the moving descriptor): row 21 motionless (d = 0: sca = inf, its projected ground truth
    and so its coefficient loss are not finite), row 66 with a NaN coefficient in sample 4.  -> C, nrm, C_gt, (21, 66)"""
    still, nanc = 21, 66
    obs = c.obs.copy()
    obs[still, -3] = obs[still, -1]
    p = project_train(obs, c.pred, *u_for(c, 1, obs=True), *u_for(c, 1), 1, c.static_dist)
    C = c.C.copy()
    C[2, nanc, 4] = np.nan
    return C, p.nrm32, np.ascontiguousarray(p.C_gt.numpy().astype(np.float32)), (still, nanc)
