"""float64 numpy restatement of both passes of csrc/et_graphtern_train.hip, independent of torch: Graph-TERN's training-mode
forward (n_epgcn = 1; DropEdge through an explicit keep mask), the backward pass to every parameter, and a running
elementwise bound for what the fp32 kernels may differ by -- the value-and-bound arithmetic ``V`` of
tests/_sgcn_train_np.py (its docstring derives the bound).  The bounds are the only tolerances
tests/test_gpu_graphtern_train.py uses; they are derived here, not tuned.  Not a test module itself.

The graphs.  The distances are taken on the fp32 input (tests/_graphtern_np.distances: the device forms the same fp32
numbers); an inverse is one fp32 quotient (one rounding), 0 where the distance is exactly 0.  A' = A * keep (the mask is
applied to the float tensor, before + I), s = rowsum(A' + I) (n terms, a lane's ascending chain), d = s^-1/2 (the square
root and the quotient are correctly rounded: two roundings on top of s's bound through |d'| = d / (2 s)),
L[w, v] = (d_w (A'[w, v] + [v == w])) d_v (two roundings) and the contracted rows P[r, j, t, w] = sum_v L[w, v] X_j[t, v] with
X_0 = u and X_1 = 1.

Step by step.  With ``device=kept`` (what ``ops.graphtern_train_views`` returns, as numpy) every kept value is formed here
from the DEVICE's kept inputs of its step (exact fp32 numbers, bound 0), compared with the device's within that one step's
bound (``kept_ratio``), and then the device's value goes on.  Every PReLU branch is read from the device's kept word; a
decision that differs from this file's outside the band is counted as a flip.  Without ``device`` the file's own kept
values take that place (bound reset to 0 at every kept value); with ``propagate`` nothing is reset, every value carries the
whole chain's bound and every sum is bounded for ANY order of its true number of terms: loose, but a bound on the distance
to the exact gradient, which is what a comparison with another implementation (the reference's float64 gradients, this
file's own float32 mode) needs.

The transposed convolution under replicate padding.  The gradient with respect to the PADDED input is the ordinary
transposed convolution; the gradient of an input cell is the sum of the padded cells that replicate it (an edge cell: its own
and the pad beside it, a corner cell: four, a plane of one row or column: all three).  The device sums the same terms in one
fmaf chain of 9 C_out terms, so the folded cells' bounds add without a further rounding.

Sums.  Every gradient element is one wavefront's sum (the kernel's header comment): a lane's ascending chain of
ceil(count / 64) terms, then 6 butterfly steps; that depth stands in place of the number of terms.

``plain`` runs the same statements in one numpy dtype (np.float32: what the fp32 arithmetic itself costs) without bounds."""
import numpy as np

from . import _graphtern_np as GN
from ._sgcn_train_np import (U, V, Decisions, add, compare, conv, conv_bwd, ein, gamma, mul, prelu_bwd, prelu_fwd,  # noqa: F401
                             vsum)

H = GN.HIDDEN
REL = GN.REL
UNUSED = "tp_mrgcns.0.prelu.weight"   # in the state_dict, never applied by the forward: no gradient


def depth_of(count):
    return -(-count // 64) + 6


def relations(u, rel):
    """u, rel (T, n) fp32 -> A (4, T, n, n) as V: [A_abs, A_rel, 1 / A_abs, 1 / A_rel]; the inverses are fp32 quotients"""
    A = [GN.distances(u).astype(np.float64), GN.distances(rel).astype(np.float64)]
    val, err = list(A), [np.zeros_like(A[0]), np.zeros_like(A[1])]
    for a in A:
        with np.errstate(divide="ignore"):
            inv = 1.0 / a
        inv[a == 0] = 0.0
        val.append(inv)
        err.append(U * inv)
    return V(np.stack(val), np.stack(err))


def masked(A, keep):
    """A V (4, T, n, n), keep (4, T, n, n) or None -> A' + I as V"""
    n = A.shape[-1]
    m = 1.0 if keep is None else (np.asarray(keep) != 0).astype(np.float64)
    return V(A.val * m + np.eye(n), A.err * m)


def degrees(At):
    """A' + I -> (s, d): the row sums and d = s^-1/2 as V (4, T, n)"""
    s = vsum(At, -1, extra=0)
    dval = s.val ** -0.5
    lo = np.maximum(s.val - s.err, 1e-300)
    return s, V(dval, 0.5 * s.err * lo ** -1.5 + 2 * U * dval)


def normalised(At, d):
    """-> L[r, t, w, v] = (d_w (A' + I)[w, v]) d_v as V"""
    n = At.shape[-1]
    return mul(mul(d.reshape(*d.shape, 1), At), d.reshape(*d.shape[:-1], 1, n))


def patches_rep(x):
    """x V (B, C, P, Q) -> (B, C * 9, P, Q): the replicate-padded neighbours a 3x3 convolution reads, channel-major"""
    B, C, P, Q = x.shape
    pad = ((0, 0), (0, 0), (1, 1), (1, 1))
    xv, xe = np.pad(x.val, pad, mode=GN.PAD_MODE), np.pad(np.ascontiguousarray(x.err), pad, mode=GN.PAD_MODE)
    val = np.stack([xv[:, :, a:a + P, b:b + Q] for a in range(3) for b in range(3)], axis=2)
    err = np.stack([xe[:, :, a:a + P, b:b + Q] for a in range(3) for b in range(3)], axis=2)
    return V(val.reshape(B, C * 9, P, Q), err.reshape(B, C * 9, P, Q))


def conv_rep(x, w, b):
    O, C = w.shape[:2]
    return ein("ok,bkpq->bopq", w.reshape(O, C * 9), patches_rep(x), init=b.reshape(1, O, 1, 1))


def _fold(a):
    """(B, C, P + 2, Q + 2) -> (B, C, P, Q): every padded cell added to the input cell it replicates"""
    a = np.array(a, np.float64)
    a[:, :, 1] += a[:, :, 0]
    a[:, :, -2] += a[:, :, -1]
    a = a[:, :, 1:-1]
    a[:, :, :, 1] += a[:, :, :, 0]
    a[:, :, :, -2] += a[:, :, :, -1]
    return a[:, :, :, 1:-1]


def conv_rep_bwd(dz, x, w, depth=None):
    """-> (d x, d w) of conv_rep(x, w): d w reads x through the clamps; d x is the folded gradient of the padded input, one
    chain of 9 O terms per cell"""
    O, C = w.shape[:2]
    B, _, P, Q = dz.shape
    dw = ein("bopq,bkpq->ok", dz, patches_rep(x), depth=depth).reshape(O, C, 3, 3)
    pad = ((0, 0), (0, 0), (2, 2), (2, 2))
    zv, ze = np.pad(dz.val, pad), np.pad(np.ascontiguousarray(dz.err), pad)
    cut = lambda a: np.stack([a[:, :, 2 - dh:2 - dh + P + 2, 2 - dq:2 - dq + Q + 2] for dh in range(3) for dq in range(3)],
                             axis=2).reshape(B, O * 9, P + 2, Q + 2)
    pz = V(cut(zv), cut(ze))
    wt = V(w.val.transpose(1, 0, 2, 3).reshape(C, O * 9), np.ascontiguousarray(w.err).transpose(1, 0, 2, 3).reshape(C, O * 9))
    g = ein("ck,bkpq->bcpq", wt, pz, extra=0)
    return V(_fold(g.val), _fold(g.err), tm=_fold(g.tm)), dw


def parameter_names(sd):
    return list(sd)


def run(sd, u, rel, d_out, keep=None, device=None, propagate=False):
    """sd: fp32 state dict, u (T, N) fp32, rel (T, N) fp32 as given (None: formed from u as the bridge does), d_out
    (k, N, S), keep (4, T, N, N) or None -> dict: ``out`` V (k, N, S), ``kept`` {name: V or list of V} (the names of
    ops.graphtern_train_views), ``kept_ratio``, ``grads`` {parameter name: V}, ``decisions``."""
    dec = Decisions()
    dv = (lambda q, j=None: None) if device is None else (lambda q, j=None: np.asarray(device[q] if j is None else device[q][j],
                                                                                       np.float64))
    Pm = lambda q: V(np.asarray(sd[q], np.float64))
    dp = (lambda count: None) if propagate else depth_of   # any order under ``propagate``
    u32 = np.asarray(u, np.float32)
    rel32 = GN.rel_of(u32) if rel is None else np.asarray(rel, np.float32)
    uv = V(u32.astype(np.float64))
    T, n = uv.shape
    k = T - 2
    n_gcn, n_cnn = GN.counts(sd)
    assert n_gcn == 1
    pre = "tp_mrgcns.0."
    cnt = T * n
    kept, grads, kept_ratio = {"u": uv}, {}, {}

    def force(name, val, j=None):
        if j is None:
            kept[name] = val
        else:
            kept.setdefault(name, {})[j] = val
        if device is None:
            return val if propagate else V(val.val)
        d = dv(name, j)
        kept_ratio[name] = max(kept_ratio.get(name, 0.0), compare(d, val))
        return V(d.reshape(val.shape))

    def prelu_kept(name, z, slope, j=None):
        """a kept PReLU input: the branch from the device's kept word, the value forced, then PReLU of the forced value"""
        sign = None if device is None else dv(name, j).reshape(z.shape) > 0
        _, keep_ = prelu_fwd(z, slope, dec, sign)
        if device is not None:   # the device's word decides everywhere, not only inside the band
            keep_ = sign
        z = force(name, z, j)
        y, _ = prelu_fwd(z, slope, Decisions(), keep_)
        return z, y, keep_

    # ------------------------------------------------------------------------------------------------ forward
    At = masked(relations(u32, rel32), keep)
    _, d = degrees(At)
    d = force("d", d)
    Lg = normalised(At, d)
    X = V(np.stack([uv.val, np.ones((T, n))]))                                        # (2, T, n): u and the ones row
    P_own = ein("rtwv,jtv->rjtw", Lg, X, extra=0)
    P = force("P", P_own)
    coef = V(np.stack([np.asarray(sd[pre + "gcn.conv.weight"], np.float64).reshape(REL, H),
                       np.asarray(sd[pre + "gcn.conv.bias"], np.float64).reshape(REL, H)], 1))   # (4, 2, 16): channel r 16 + c
    a_tcn = Pm(pre + "tcn.0.weight")
    yp, y, keep_yp = prelu_kept("yp", ein("rjc,rjtw->ctw", coef, P, extra=0), a_tcn)
    tw = Pm(pre + "tcn.1.weight")
    z = conv(y.reshape(1, H, T, n), tw, Pm(pre + "tcn.1.bias")).reshape(H, T, n)
    rw, rb = Pm(pre + "residual.0.weight").reshape(H, 1, 1), Pm(pre + "residual.0.bias").reshape(H, 1, 1)
    res = add(mul(rw, uv.reshape(1, T, n), roundings=0), rb, roundings=1)
    cur = force("x0", add(z, res).t(1, 0, 2))                                         # the permute: (T, 16, n)
    blocks = []
    for j in range(n_cnn):
        ep = f"tpcnns.{j}."
        B = dict(x=cur)
        Rin = cur.shape[0]
        c0, act, B["keep0"] = prelu_kept("c0", conv_rep(cur.reshape(1, Rin, H, n), Pm(ep + "tpcns.0.0.weight"),
                                                        Pm(ep + "tpcns.0.0.bias")).reshape(k, H, n),
                                         Pm(ep + "tpcns.0.1.weight"), j)
        B["c0"], B["y"] = c0, force("y", act, j)
        Wc = Pm(ep + "cpcns.0.0.weight")
        Cout = Wc.shape[0]
        c1 = conv_rep(B["y"].t(1, 0, 2).reshape(1, H, k, n), Wc, Pm(ep + "cpcns.0.0.bias")).reshape(Cout, k, n).t(1, 0, 2)
        c1, act, B["keep1"] = prelu_kept("c1", c1, Pm(ep + "cpcns.0.1.weight"), j)
        B["c1"] = c1
        if ep + "restconv.0.weight" in sd:
            r = ein("ot,tcv->ocv", Pm(ep + "restconv.0.weight").reshape(k, Rin), cur, extra=0,
                    init=Pm(ep + "restconv.0.bias").reshape(k, 1, 1))
        elif ep + "rescconv.0.weight" in sd:
            r = ein("oc,tcv->tov", Pm(ep + "rescconv.0.weight").reshape(Cout, H), cur, extra=0,
                    init=Pm(ep + "rescconv.0.bias").reshape(1, Cout, 1))
        else:
            r = cur
        cur = force("o", add(act, r), j)
        blocks.append(B)
    out = cur.t(0, 2, 1)                                                              # (k, n, S)
    S = out.shape[2]
    if d_out is None:   # the forward alone (the seed search of tests/_graphtern_train_cases.py)
        return dict(out=out, kept=kept, kept_ratio=kept_ratio, grads={}, decisions=dec.figures())

    # ------------------------------------------------------------------------------------------------ backward
    do = V(np.asarray(d_out, np.float64).reshape(k, n, S).transpose(0, 2, 1))         # (k, S, n)
    for j in range(n_cnn - 1, -1, -1):
        ep, B = f"tpcnns.{j}.", blocks[j]
        xin = B["x"]
        Rin, Cout = xin.shape[0], do.shape[1]
        do = force("d_o", do, j)
        dc1, grads[ep + "cpcns.0.1.weight"] = prelu_bwd(do, B["c1"], Pm(ep + "cpcns.0.1.weight"), B["keep1"],
                                                        depth=dp(k * Cout * n))
        grads[ep + "cpcns.0.0.bias"] = vsum(dc1, (0, 2), extra=0, depth=dp(k * n))
        dy, grads[ep + "cpcns.0.0.weight"] = conv_rep_bwd(dc1.t(1, 0, 2).reshape(1, Cout, k, n),
                                                          B["y"].t(1, 0, 2).reshape(1, H, k, n), Pm(ep + "cpcns.0.0.weight"),
                                                          depth=dp(k * n))
        dy = force("d_y", dy.reshape(H, k, n).t(1, 0, 2), j)
        dc0, grads[ep + "tpcns.0.1.weight"] = prelu_bwd(dy, B["c0"], Pm(ep + "tpcns.0.1.weight"), B["keep0"],
                                                        depth=dp(k * H * n))
        grads[ep + "tpcns.0.0.bias"] = vsum(dc0, (1, 2), extra=0, depth=dp(H * n))
        dxc, grads[ep + "tpcns.0.0.weight"] = conv_rep_bwd(dc0.reshape(1, k, H, n), xin.reshape(1, Rin, H, n),
                                                           Pm(ep + "tpcns.0.0.weight"), depth=dp(H * n))
        dxc = dxc.reshape(Rin, H, n)
        if ep + "restconv.0.weight" in sd:
            grads[ep + "restconv.0.weight"] = ein("ocv,tcv->ot", do, xin, extra=0, depth=dp(H * n)).reshape(k, Rin, 1, 1)
            grads[ep + "restconv.0.bias"] = vsum(do, (1, 2), extra=0, depth=dp(H * n))
            dres = ein("ot,ocv->tcv", Pm(ep + "restconv.0.weight").reshape(k, Rin), do, extra=0)
        elif ep + "rescconv.0.weight" in sd:
            grads[ep + "rescconv.0.weight"] = ein("tov,tcv->oc", do, xin, extra=0, depth=dp(k * n)).reshape(Cout, H, 1, 1)
            grads[ep + "rescconv.0.bias"] = vsum(do, (0, 2), extra=0, depth=dp(k * n))
            dres = ein("oc,tov->tcv", Pm(ep + "rescconv.0.weight").reshape(Cout, H), do, extra=0)
        else:
            dres = do
        do = add(dres, dxc)
    dx0 = force("d_x0", do)
    ds = dx0.t(1, 0, 2)                                                               # (16, T, n): no PReLU of the block's own
    dsum, dc = dp(H * T * n), dp(cnt)
    grads[pre + "tcn.1.bias"] = vsum(ds, (1, 2), extra=0, depth=dc)
    dyt, grads[pre + "tcn.1.weight"] = conv_bwd(ds.reshape(1, H, T, n), y.reshape(1, H, T, n), tw, depth=dc)
    dyt = force("d_yt", dyt.reshape(H, T, n))
    grads[pre + "residual.0.weight"] = ein("ctw,tw->c", ds, uv, extra=0, depth=dc).reshape(H, 1, 1, 1)
    grads[pre + "residual.0.bias"] = vsum(ds, (1, 2), extra=0, depth=dc)
    dyp, grads[pre + "tcn.0.weight"] = prelu_bwd(dyt, yp, a_tcn, keep_yp, depth=dsum)
    dcoef = ein("ctw,rjtw->rjc", dyp, P, extra=0, depth=dc)
    # P's u row is a sum of both signs: the terms' magnitudes of a gcn gradient are taken with those of P's own terms
    dcoef.tm = np.einsum("ctw,rjtw->rjc", dyp.mag, P_own.tm)
    for jj, (q, shape) in enumerate((("weight", (REL * H, 1, 1, 1)), ("bias", (REL * H,)))):
        grads[f"{pre}gcn.conv.{q}"] = V(dcoef.val[:, jj].reshape(shape), dcoef.err[:, jj].reshape(shape),
                                        tm=dcoef.tm[:, jj].reshape(shape))
    grads[UNUSED] = V(np.zeros(1))
    for name, gk in grads.items():   # the final rounding of every stored gradient
        gk.err = gk.err + U * np.abs(gk.val)
        shape = np.asarray(sd[name]).shape
        if gk.shape != shape:
            grads[name] = V(np.ascontiguousarray(gk.val).reshape(shape), np.ascontiguousarray(gk.err).reshape(shape),
                            None if gk.tm is None else np.ascontiguousarray(gk.tm).reshape(shape))
    kept = {q: [val[j] for j in sorted(val)] if isinstance(val, dict) else val for q, val in kept.items()}
    return dict(out=out, kept=kept, kept_ratio=kept_ratio, grads={q: grads[q] for q in parameter_names(sd)},
                decisions=dec.figures())


def _conv_rep_plain(x, w, b):
    return GN._conv33_replicate(x, w, b, x.dtype)


def _conv_rep_bwd_plain(dz, x, w):
    """dz (O, P, Q), x (C, P, Q), w (O, C, 3, 3) -> (d x, d w), all in x's dtype"""
    O, C = w.shape[:2]
    _, P, Q = dz.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1)), mode=GN.PAD_MODE)
    dw = np.zeros_like(w)
    g = np.zeros((C, P + 2, Q + 2), x.dtype)
    for dh in range(3):
        for dq in range(3):
            dw[:, :, dh, dq] = np.einsum("opq,cpq->oc", dz, xp[:, dh:dh + P, dq:dq + Q])
            g[:, dh:dh + P, dq:dq + Q] += np.einsum("oc,opq->cpq", w[:, :, dh, dq], dz)
    return _fold(g[None])[0].astype(x.dtype), dw


def plain(sd, u, rel, d_out, keep=None, dtype=np.float64):
    """the same forward and backward in ONE numpy dtype, no bounds -> (out (k, N, S), {parameter name: gradient}, the kept
    PReLU inputs as a flat list).  The distances are fp32 in both modes; np.float32 shows what the fp32 arithmetic itself
    costs on an input"""
    f = lambda q: np.asarray(sd[q], dtype)
    a = lambda q: f(q).reshape(-1)[0]
    prelu = lambda x, s: np.where(x > 0, x, s * x)
    u32 = np.asarray(u, np.float32)
    rel32 = GN.rel_of(u32) if rel is None else np.asarray(rel, np.float32)
    T, n = u32.shape
    k = T - 2
    _, n_cnn = GN.counts(sd)
    pre = "tp_mrgcns.0."
    A = [GN.distances(u32).astype(dtype), GN.distances(rel32).astype(dtype)]
    for q in list(A):
        with np.errstate(divide="ignore"):
            inv = (dtype(1) / q).astype(dtype)
        inv[q == 0] = 0
        A.append(inv)
    A = np.stack(A)
    if keep is not None:
        A = A * (np.asarray(keep) != 0).astype(dtype)
    At = A + np.eye(n, dtype=dtype)
    d = (dtype(1) / np.sqrt(At.sum(-1))).astype(dtype)
    d[np.isinf(d)] = 0
    Lg = (d[..., None] * At) * d[..., None, :]
    ud = u32.astype(dtype)
    X = np.stack([ud, np.ones((T, n), dtype)])
    P = np.einsum("rtwv,jtv->rjtw", Lg, X)
    coef = np.stack([f(pre + "gcn.conv.weight").reshape(REL, H), f(pre + "gcn.conv.bias").reshape(REL, H)], 1)
    yp = np.einsum("rjc,rjtw->ctw", coef, P)
    pre_acts = [yp]
    y = prelu(yp, a(pre + "tcn.0.weight"))
    tw = f(pre + "tcn.1.weight")[:, :, :, 0]
    ypad = np.zeros((H, T + 2, n), dtype)
    ypad[:, 1:-1] = y
    z = f(pre + "tcn.1.bias")[:, None, None] + sum(np.einsum("oc,ctv->otv", tw[:, :, dt], ypad[:, dt:dt + T]) for dt in range(3))
    x0 = z + f(pre + "residual.0.weight").reshape(H, 1, 1) * ud[None] + f(pre + "residual.0.bias").reshape(H, 1, 1)
    cur = np.ascontiguousarray(x0.transpose(1, 0, 2))
    blocks = []
    for j in range(n_cnn):
        ep = f"tpcnns.{j}."
        c0 = _conv_rep_plain(cur, f(ep + "tpcns.0.0.weight"), f(ep + "tpcns.0.0.bias"))
        yj = prelu(c0, a(ep + "tpcns.0.1.weight"))
        c1 = _conv_rep_plain(np.ascontiguousarray(yj.transpose(1, 0, 2)), f(ep + "cpcns.0.0.weight"),
                             f(ep + "cpcns.0.0.bias")).transpose(1, 0, 2)
        pre_acts += [c0, c1]
        if ep + "restconv.0.weight" in sd:
            r = np.einsum("ot,tcv->ocv", f(ep + "restconv.0.weight")[:, :, 0, 0], cur) + f(ep + "restconv.0.bias")[:, None, None]
        elif ep + "rescconv.0.weight" in sd:
            r = np.einsum("oc,tcv->tov", f(ep + "rescconv.0.weight")[:, :, 0, 0], cur) + f(ep + "rescconv.0.bias")[None, :, None]
        else:
            r = cur
        blocks.append((cur, c0, yj, c1))
        cur = prelu(c1, a(ep + "cpcns.0.1.weight")) + r
    out = np.ascontiguousarray(cur.transpose(0, 2, 1))
    S = out.shape[2]
    g = {UNUSED: np.zeros(1, dtype)}
    do = np.asarray(d_out, dtype).reshape(k, n, S).transpose(0, 2, 1)
    for j in range(n_cnn - 1, -1, -1):
        ep = f"tpcnns.{j}."
        xin, c0, yj, c1 = blocks[j]
        s1, s0 = a(ep + "cpcns.0.1.weight"), a(ep + "tpcns.0.1.weight")
        g[ep + "cpcns.0.1.weight"] = np.array([np.where(c1 > 0, 0, do * c1).sum()], dtype)
        dc1 = np.where(c1 > 0, do, s1 * do)
        g[ep + "cpcns.0.0.bias"] = dc1.sum((0, 2))
        dy, g[ep + "cpcns.0.0.weight"] = _conv_rep_bwd_plain(np.ascontiguousarray(dc1.transpose(1, 0, 2)),
                                                              np.ascontiguousarray(yj.transpose(1, 0, 2)), f(ep + "cpcns.0.0.weight"))
        dy = dy.transpose(1, 0, 2)
        g[ep + "tpcns.0.1.weight"] = np.array([np.where(c0 > 0, 0, dy * c0).sum()], dtype)
        dc0 = np.where(c0 > 0, dy, s0 * dy)
        g[ep + "tpcns.0.0.bias"] = dc0.sum((1, 2))
        dxc, g[ep + "tpcns.0.0.weight"] = _conv_rep_bwd_plain(np.ascontiguousarray(dc0), xin, f(ep + "tpcns.0.0.weight"))
        if ep + "restconv.0.weight" in sd:
            g[ep + "restconv.0.weight"] = np.einsum("ocv,tcv->ot", do, xin)[:, :, None, None]
            g[ep + "restconv.0.bias"] = do.sum((1, 2))
            dres = np.einsum("ot,ocv->tcv", f(ep + "restconv.0.weight")[:, :, 0, 0], do)
        elif ep + "rescconv.0.weight" in sd:
            g[ep + "rescconv.0.weight"] = np.einsum("tov,tcv->oc", do, xin)[:, :, None, None]
            g[ep + "rescconv.0.bias"] = do.sum((0, 2))
            dres = np.einsum("oc,tov->tcv", f(ep + "rescconv.0.weight")[:, :, 0, 0], do)
        else:
            dres = do
        do = dres + dxc
    ds = do.transpose(1, 0, 2)
    g[pre + "tcn.1.bias"] = ds.sum((1, 2))
    g[pre + "tcn.1.weight"] = np.stack([np.einsum("otv,ctv->oc", ds, ypad[:, dt:dt + T]) for dt in range(3)], -1)[..., None]
    dpad = np.zeros((H, T + 2, n), dtype)
    dpad[:, 1:-1] = ds
    dyt = sum(np.einsum("oc,otv->ctv", tw[:, :, dt], dpad[:, 2 - dt:2 - dt + T]) for dt in range(3))
    g[pre + "residual.0.weight"] = np.einsum("ctw,tw->c", ds, ud).reshape(H, 1, 1, 1)
    g[pre + "residual.0.bias"] = ds.sum((1, 2))
    g[pre + "tcn.0.weight"] = np.array([np.where(yp > 0, 0, dyt * yp).sum()], dtype)
    dyp = np.where(yp > 0, dyt, a(pre + "tcn.0.weight") * dyt)
    dcoef = np.einsum("ctw,rjtw->rjc", dyp, P)
    g[pre + "gcn.conv.weight"] = dcoef[:, 0].reshape(REL * H, 1, 1, 1)
    g[pre + "gcn.conv.bias"] = dcoef[:, 1].reshape(REL * H)
    return out, {q: np.asarray(g[q], dtype).reshape(np.asarray(sd[q]).shape) for q in sd}, pre_acts


def gcn_names(sd):
    return tuple(q for q in sd if ".gcn.conv." in q)


def vacuous(sd, grads, zero=()):
    """the tensors of more than one element whose bound reaches half their largest entry: a bound below that cannot pass
    zeros, a flipped sign or a wrong scale at that entry.  ``zero``: the analytically zero tensors of the case, excepted; so is
    a one-element tensor (a sum over the whole scene that can cancel)."""
    return [q for q, g in grads.items() if q not in zero and g.val.size > 1 and g.err.max() > 0
            and g.err.max() >= 0.5 * np.abs(g.val).max()]


def device_dict(views):
    """``ops.graphtern_train_views``' result (torch views or numpy copies) -> the ``device=`` argument of :func:`run`"""
    f = lambda t: np.asarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, np.float64)
    return {q: ([f(t) for t in val] if isinstance(val, list) else f(val)) for q, val in views.items()}
