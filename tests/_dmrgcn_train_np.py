"""float64 numpy restatement of both passes of csrc/et_dmrgcn_train.hip, independent of torch: DMRGCN's training-mode forward
(n_stgcn = 1; DropEdge through an explicit keep mask), the backward pass to every parameter, and a running elementwise bound
for what the fp32 kernels may differ by -- the value-and-bound arithmetic ``V`` of tests/_sgcn_train_np.py (its docstring
derives the bound).  The bounds are the only tolerances tests/test_gpu_dmrgcn_train.py uses; they are derived here, not
tuned.  Not a test module itself.

The graphs.  The bins are decided on the fp32 distances with tests/_dmrgcn_np.bins (the device compares the same fp32
numbers), A' = A_b * keep, cnt = the kept entries of a row, d = (1 + cnt)^-1/2 (1 + cnt is exact, sqrt and the quotient are
correctly rounded: two roundings), L[w, v] = [v == w] - (d_w (A'[w, v] + [v == w])) d_v (A' + I is 0, 1 or 2: exact), and the
contraction rows P[r, b, j, t, w] = sum_v L[w, v] X_j[t, v] with X_0 = u and X_1 = 1.

Step by step.  With ``device=kept`` (what ``ops.dmrgcn_train_views`` returns, as numpy) every kept value is formed here from
the DEVICE's kept inputs of its step (exact fp32 numbers, bound 0), compared with the device's within that one step's bound
(``kept_ratio``), and then the device's value goes on.  Every PReLU branch is read from the device's kept word; a decision
that differs from this file's outside the band is counted as a flip.  The gradient at a tpcnn block's output is not kept
between the blocks (it lives in the arena): it carries the bound of the step that formed it into the next block's first
kept value.  Without ``device`` the file's own kept values take that place (bound reset to 0 at every kept value); with
``propagate`` nothing is reset and every value carries the whole chain's bound: loose, but a bound on the distance to the
exact gradient, which is what a comparison with another implementation's float64 gradients needs.

Values.  The forward's float64 VALUES are formed with tests/_dmrgcn_np's own expressions (its _contract on the masked
distances, its einsums and _conv33, term for term), so that with an all-ones mask the forward equals
tests/_dmrgcn_np.forward exactly; the bounds come from the V arithmetic beside them.

Sums.  Every gradient element is one wavefront's sum (the kernel's header comment): a lane's ascending chain of
ceil(count / 64) terms, then 6 butterfly steps; that depth stands in place of the number of terms."""
import numpy as np

from . import _dmrgcn_np as DN
from ._sgcn_train_np import (U, V, Decisions, add, compare, conv, conv_bwd, ein, mul, neg, prelu_bwd, prelu_fwd,  # noqa: F401
                             vsum)

NB = len(DN.SPLIT[0])


def depth_of(count):
    return -(-count // 64) + 6


def kept_adjacency(a, keep=None, split=DN.SPLIT):
    """a (2, K, n, n) fp32, keep (2, 5, K, n, n) or None -> A' (2, 5, K, n, n) float64 0/1: the clipped bins after DropEdge"""
    A = np.stack([DN.bins(a[r], split[r]) for r in range(2)]).astype(np.float64)
    return A if keep is None else A * (np.asarray(keep) != 0)


def apply_keep(a, keep, split=DN.SPLIT):
    """a (2, K, n, n) fp32 -> the same with every dropped entry set to 0.  A pair is in at most one bin of a relation and 0
    is in no bin, so the eval restatement (tests/_dmrgcn_np.forward, which reads ``a`` as it is) on this tensor computes the
    forward on the dropped, asymmetric graphs"""
    a = np.asarray(a, np.float32)
    if keep is None:
        return a
    M = np.stack([DN.bins(a[r], split[r]) for r in range(2)])
    return np.where((M & (np.asarray(keep) == 0)).any(axis=1), np.float32(0), a)


def laplacians(Ak):
    """A' (2, 5, K, n, n) -> L as V, [r, b, t, w, v]"""
    n = Ak.shape[-1]
    eye = np.eye(n)
    cnt = Ak.sum(-1)
    dval = (1.0 + cnt) ** -0.5
    d = V(dval, 2 * U * dval)
    dw, dv = d.reshape(*dval.shape, 1), d.reshape(*dval.shape[:-1], 1, n)
    inner = mul(mul(dw, V(Ak + eye), roundings=0), dv)
    return add(V(np.broadcast_to(eye, Ak.shape)), neg(inner), roundings=1)


def parameter_names(sd):
    return list(sd)


def run(sd, v, a, d_out, keep=None, device=None, propagate=False, split=DN.SPLIT):
    """sd: fp32 state dict, v (K, N) fp32, a (2, K, N, N) fp32 (None: formed from v as the bridge does), d_out (S, k, N),
    keep (2, 5, K, N, N) or None -> dict: ``out`` V (S, k, N), ``kept`` {name: V or list of V} (the names of
    ops.dmrgcn_train_views), ``kept_ratio``, ``grads`` {parameter name: V}, ``decisions``."""
    dec = Decisions()
    dv = (lambda q, j=None: None) if device is None else (lambda q, j=None: np.asarray(device[q] if j is None else device[q][j],
                                                                                       np.float64))
    Pm = lambda q: V(np.asarray(sd[q], np.float64))
    u = V(np.asarray(v, np.float32).astype(np.float64))
    K, n = u.shape
    pre = "st_dmrgcns.0."
    S = np.asarray(sd[pre + "tcn.1.weight"]).shape[0]
    k = K - 2
    cnt = K * n
    n_tp = len([q for q in sd if q.endswith("gtacn.0.1.weight")])
    has_res = pre + "residual.0.weight" in sd
    if a is None:
        a = DN.adjacency(np.asarray(v, np.float32))
    kept, grads, kept_ratio = {"u": u}, {}, {}

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
    f64 = lambda q: np.asarray(sd[q], np.float64)
    like = lambda val, bound: V(val, bound.err)                                       # _dmrgcn_np's value, this file's bound
    Lp = laplacians(kept_adjacency(np.asarray(a, np.float32), keep, split))
    X = V(np.stack([u.val, np.ones((K, n))]))                                         # (2, K, n): u and the ones row
    am = apply_keep(a, keep, split)
    Pval = np.empty((2, NB, 2, K, n))
    for r in range(2):
        for t in range(K):
            Pval[r, :, :, t] = DN._contract(np.concatenate([u.val[None, t], np.ones((1, n))]),
                                            lambda lo, hi, r=r, t=t: am[r][t][lo:hi], split[r], False)
    P_own = ein("rbtwv,jtv->rbjtw", Lp, X)                                            # + the `zero` term: extra = 2
    P = force("P", like(Pval, P_own))
    coef = V(np.stack([np.stack([np.asarray(sd[f"{pre}gcns.{r}.conv.weight"], np.float64).reshape(NB, S),
                                 np.asarray(sd[f"{pre}gcns.{r}.conv.bias"], np.float64).reshape(NB, S)], 1)
                       for r in range(2)]))                                           # (2, 5, 2, S): channel b S + c
    a_tcn, a_blk = Pm(pre + "tcn.0.weight"), Pm(pre + "prelu.weight")
    ypv = np.zeros((S, K, n))
    for r in range(2):
        Wr, Br = f64(f"{pre}gcns.{r}.conv.weight")[:, :, 0, 0].reshape(NB, S, 1), f64(f"{pre}gcns.{r}.conv.bias").reshape(NB, S)
        for t in range(K):
            ypv[:, t] += np.einsum("bsc,bcw->sw", Wr, P.val[r, :, :1, t]) + np.einsum("bs,bw->sw", Br, P.val[r, :, 1, t])
    yp, y, keep_yp = prelu_kept("yp", like(ypv, ein("rbjc,rbjtw->ctw", coef, P)), a_tcn)
    tw = Pm(pre + "tcn.1.weight")
    ypad = np.zeros((S, K + 2, n))
    ypad[:, 1:-1] = y.val
    zv = tw.val[:, :, :, 0], f64(pre + "tcn.1.bias")
    zv = zv[1][:, None, None] + sum(np.einsum("oc,ctv->otv", zv[0][:, :, dt], ypad[:, dt:dt + K]) for dt in range(3))
    z = like(zv, conv(y.reshape(1, S, K, n), tw, Pm(pre + "tcn.1.bias")).reshape(S, K, n))
    if has_res:
        rw, rb = Pm(pre + "residual.0.weight").reshape(S, 1, 1), Pm(pre + "residual.0.bias").reshape(S, 1, 1)
        resv = np.einsum("oc,ctv->otv", rw.val[:, :, 0], u.val[None]) + rb.val
        res = like(resv, add(mul(rw, u.reshape(1, K, n), roundings=0), rb, roundings=1))
    else:
        res = u.reshape(1, K, n)
    s, x, keep_s = prelu_kept("s", add(z, res), a_blk)
    cur = force("x", x.t(1, 0, 2))                                                    # the permute: (K, S, n)
    blocks = []
    for j in range(n_tp):
        tp = f"tpcnns.{j}."
        B = dict(x=cur)
        c33 = lambda x, m: like(DN._conv33(x.val, f64(f"{tp}tpcn.{m}.0.weight"), f64(f"{tp}tpcn.{m}.0.bias")),
                                conv(x.reshape(1, *x.shape), Pm(f"{tp}tpcn.{m}.0.weight"),
                                     Pm(f"{tp}tpcn.{m}.0.bias")).reshape(k, S, n))
        c0, act, B["keep0"] = prelu_kept("c0", c33(cur, 0), Pm(tp + "tpcn.0.1.weight"), j)
        if j == 0:
            r0v = np.einsum("oc,chw->ohw", f64(tp + "residual.0.weight")[:, :, 0, 0], cur.val) + \
                f64(tp + "residual.0.bias")[:, None, None]
            r0 = like(r0v, ein("oc,chw->ohw", Pm(tp + "residual.0.weight").reshape(k, K), cur, extra=0,
                               init=Pm(tp + "residual.0.bias").reshape(k, 1, 1)))
        else:
            r0 = cur
        B["c0"], B["y"] = c0, force("y", add(act, r0), j)
        c1, act, B["keep1"] = prelu_kept("c1", c33(B["y"], 1), Pm(tp + "tpcn.1.1.weight"), j)
        B["c1"], B["q"] = c1, force("q", add(act, B["y"]), j)
        Wg = Pm(tp + "gtacn.0.0.weight").reshape(S, S, k)
        zgv = np.einsum("ost,tsw->ow", Wg.val, B["q"].val) + f64(tp + "gtacn.0.0.bias")[:, None]
        zg, g, B["keepz"] = prelu_kept("z", like(zgv, ein("ost,tsw->ow", Wg, B["q"], extra=0,
                                                          init=Pm(tp + "gtacn.0.0.bias").reshape(S, 1))),
                                       Pm(tp + "gtacn.0.1.weight"), j)
        B["z"] = zg
        cur = force("o", add(g.reshape(1, S, n), B["q"]), j)
        blocks.append(B)
    out = cur.t(1, 0, 2)                                                              # (S, k, n)

    # ------------------------------------------------------------------------------------------------ backward
    dp, dko = depth_of(S * n), depth_of(k * S * n)
    do = V(np.asarray(d_out, np.float64).reshape(S, k, n).transpose(1, 0, 2))         # (k, S, n)
    for j in range(n_tp - 1, -1, -1):
        tp, B = f"tpcnns.{j}.", blocks[j]
        Wg = Pm(tp + "gtacn.0.0.weight").reshape(S, S, k)
        dg = force("d_g", vsum(do, 0, extra=0), j)
        dz, grads[tp + "gtacn.0.1.weight"] = prelu_bwd(dg, B["z"], Pm(tp + "gtacn.0.1.weight"), B["keepz"], depth=dp)
        grads[tp + "gtacn.0.0.bias"] = vsum(dz, 1, extra=0, depth=depth_of(n))
        grads[tp + "gtacn.0.0.weight"] = ein("ow,tsw->ost", dz, B["q"], extra=0, depth=depth_of(n)).reshape(S, S, k, 1)
        dq = force("d_q", ein("ost,ow->tsw", Wg, dz, extra=0, init=do), j)
        dc1, grads[tp + "tpcn.1.1.weight"] = prelu_bwd(dq, B["c1"], Pm(tp + "tpcn.1.1.weight"), B["keep1"], depth=dko)
        grads[tp + "tpcn.1.0.bias"] = vsum(dc1, (1, 2), extra=0, depth=dp)
        dy, grads[tp + "tpcn.1.0.weight"] = conv_bwd(dc1.reshape(1, k, S, n), B["y"].reshape(1, k, S, n),
                                                     Pm(tp + "tpcn.1.0.weight"), init=dq.reshape(1, k, S, n), depth=dp)
        dy = force("d_y", dy.reshape(k, S, n), j)
        dc0, grads[tp + "tpcn.0.1.weight"] = prelu_bwd(dy, B["c0"], Pm(tp + "tpcn.0.1.weight"), B["keep0"], depth=dko)
        grads[tp + "tpcn.0.0.bias"] = vsum(dc0, (1, 2), extra=0, depth=dp)
        xin = B["x"]
        dxc, grads[tp + "tpcn.0.0.weight"] = conv_bwd(dc0.reshape(1, k, S, n), xin.reshape(1, *xin.shape),
                                                      Pm(tp + "tpcn.0.0.weight"), depth=dp)
        dxc = dxc.reshape(xin.shape)
        if j == 0:
            rwm = Pm(tp + "residual.0.weight").reshape(k, K)
            grads[tp + "residual.0.weight"] = ein("ohw,chw->oc", dy, xin, extra=0, depth=dp).reshape(k, K, 1, 1)
            grads[tp + "residual.0.bias"] = vsum(dy, (1, 2), extra=0, depth=dp)
            do = force("d_x", add(ein("oc,ohw->chw", rwm, dy, extra=0), dxc))
        else:
            do = add(dy, dxc)
    dsum, dc = depth_of(S * K * n), depth_of(cnt)
    ds, grads[pre + "prelu.weight"] = prelu_bwd(do.t(1, 0, 2), s, a_blk, keep_s, depth=dsum)
    grads[pre + "tcn.1.bias"] = vsum(ds, (1, 2), extra=0, depth=dc)
    dyt, grads[pre + "tcn.1.weight"] = conv_bwd(ds.reshape(1, S, K, n), y.reshape(1, S, K, n), tw, depth=dc)
    dyt = force("d_yt", dyt.reshape(S, K, n))
    if has_res:
        grads[pre + "residual.0.weight"] = ein("ctw,tw->c", ds, u, extra=0, depth=dc).reshape(S, 1, 1, 1)
        grads[pre + "residual.0.bias"] = vsum(ds, (1, 2), extra=0, depth=dc)
    dyp, grads[pre + "tcn.0.weight"] = prelu_bwd(dyt, yp, a_tcn, keep_yp, depth=dsum)
    dcoef = ein("ctw,rbjtw->rbjc", dyp, P, extra=0, depth=dc)
    # a row of L can sum to zero (two pedestrians, both directions kept): what is left of P's ones row is the rounding of
    # ITS sum, so the terms' magnitudes of a gcn gradient are taken with the magnitudes of P's own terms
    dcoef.tm = np.einsum("ctw,rbjtw->rbjc", dyp.mag, P_own.tm)
    for r in range(2):
        for jj, (q, shape) in enumerate((("weight", (NB * S, 1, 1, 1)), ("bias", (NB * S,)))):
            grads[f"{pre}gcns.{r}.conv.{q}"] = V(dcoef.val[r][:, jj].reshape(shape), dcoef.err[r][:, jj].reshape(shape),
                                                 tm=dcoef.tm[r][:, jj].reshape(shape))
    for name, gk in grads.items():   # the final rounding of every stored gradient
        gk.err = gk.err + U * np.abs(gk.val)
        shape = np.asarray(sd[name]).shape
        if gk.shape != shape:
            grads[name] = V(np.ascontiguousarray(gk.val).reshape(shape), np.ascontiguousarray(gk.err).reshape(shape),
                            None if gk.tm is None else np.ascontiguousarray(gk.tm).reshape(shape))
    kept = {q: [val[j] for j in sorted(val)] if isinstance(val, dict) else val for q, val in kept.items()}
    return dict(out=out, kept=kept, kept_ratio=kept_ratio, grads={q: grads[q] for q in parameter_names(sd)},
                decisions=dec.figures())


def gcn_names(sd):
    return tuple(q for q in sd if ".gcns." in q)


def analytic_zero(sd, n, kind):
    """the tensors whose gradient is analytically zero in the case (n pedestrians, keep mask ``kind``): with one pedestrian,
    or with every edge dropped, every bin is empty, L = 0 and both gcn tensors of both relations get an exact zero (P is an
    exact 0).  With two pedestrians and a symmetric graph (nothing dropped) every L is c [[1, -1], [-1, 1]]: its rows sum
    to zero, the contracted ones row vanishes and the gcn biases' gradients are sums of rounding residues -- nothing a bound
    could be small against, so they are held to their bound around zero"""
    if n == 1 or kind == "zeros":
        return gcn_names(sd)
    if n == 2 and kind in ("null", "ones"):
        return tuple(q for q in gcn_names(sd) if q.endswith("bias"))
    return ()


def vacuous(sd, grads, zero=()):
    """the tensors of more than one element whose bound reaches half their largest entry: a bound below that cannot pass
    zeros, a flipped sign or a wrong scale at that entry.  ``zero``: the analytically zero tensors of the case, excepted; so is
    a one-element tensor (a sum over the whole scene that can cancel)."""
    return [q for q, g in grads.items() if q not in zero and g.val.size > 1 and g.err.max() > 0
            and g.err.max() >= 0.5 * np.abs(g.val).max()]


def device_dict(views):
    """``ops.dmrgcn_train_views``' result (torch views or numpy copies) -> the ``device=`` argument of :func:`run`"""
    f = lambda t: np.asarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, np.float64)
    return {q: ([f(t) for t in val] if isinstance(val, list) else f(val)) for q, val in views.items()}
