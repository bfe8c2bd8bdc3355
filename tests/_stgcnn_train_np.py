"""float64 numpy restatement of both passes of csrc/et_stgcnn_train.hip, independent of torch: Social-STGCNN's training-mode
forward (n_stgcnn = 1; BatchNorm batch statistics, the running-statistics update), the backward pass to every parameter, and
a running elementwise bound for what the fp32 kernels may differ by -- the value-and-bound arithmetic ``V`` of
tests/_sgcn_train_np.py (its docstring derives the bound).  The bounds are the only tolerances
tests/test_gpu_stgcnn_train.py uses; they are derived here, not tuned.  Not a test module itself.

Step by step.  With ``device=kept`` (what ``ops.stgcnn_train_views`` returns, as numpy) every kept value is formed here from
the DEVICE's kept inputs of its step (exact fp32 numbers, bound 0), compared with the device's within that one step's bound
(``kept_ratio``), and then the device's value goes on.  Every PReLU branch is read from the device's kept word; a kept PReLU
input cannot lie inside a band then (its bound is 0), so a decision that differs from this file's is a flip and is counted.
Without ``device`` the file's own kept values take that place (bound reset to 0 at every kept value); with ``propagate``
nothing is reset and every value carries the whole chain's bound: loose, but a bound on the distance to the exact gradient,
which is what a comparison with another implementation's float64 gradients needs.

Sums.  Every per-channel statistic and every gradient element is one wavefront's sum (the kernel's header comment): a lane's
ascending chain of ceil(count / 64) terms, then 6 butterfly steps; that depth stands in place of the number of terms."""
import numpy as np

from ._sgcn_train_np import (U, V, Decisions, add, compare, const, conv, conv_bwd, ein, gamma, mul, neg, prelu_bwd,  # noqa: F401
                             prelu_fwd, vsum)

BN_NAMES = ("st_gcns.0.tcn.0", "st_gcns.0.tcn.3", "st_gcns.0.residual.1")
ZERO_GRADS = ("st_gcns.0.tcn.2.bias", "st_gcns.0.residual.0.bias")


def parameter_names(sd):
    return [k for k in sd if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))]


def unused_names(sd):
    """the tail the forward never reads (n_txpcnn >= 2)"""
    j = len([k for k in sd if k.startswith("prelus.")]) - 1
    return (f"tpcnns.{j}.weight", f"tpcnns.{j}.bias", f"prelus.{j}.weight") if j >= 1 else ()


def depth_of(count):
    return -(-count // 64) + 6


def scale(x, c):
    """x / c for an exact positive float c: one rounding"""
    return V(x.val / c, x.err / c + U * np.abs(x.val / c))


def rsqrt_eps(var, eps):
    """1 / sqrt(var + eps) with var >= 0 on both sides: the derivative's supremum over the interval, three roundings"""
    w = var.val + eps
    werr = var.err + U * np.abs(w)
    lo = np.maximum(w - werr, eps * (1 - 4 * U))
    inv = 1.0 / np.sqrt(w)
    return V(inv, 0.5 * lo ** -1.5 * werr + 2 * U * inv)


def bn_stats(x, cnt, eps):
    """x V (S, K, n) -> mean, biased variance, 1 / sqrt(var + eps): V (S,) each, two passes"""
    d = depth_of(cnt)
    mean = scale(vsum(x, (1, 2), extra=0, depth=d), float(cnt))
    diff = add(x, neg(mean.reshape(-1, 1, 1)))
    var = scale(vsum(mul(diff, diff), (1, 2), extra=0, depth=d), float(cnt))
    return mean, var, rsqrt_eps(var, eps)


def bn_apply(x, mean, inv, w, b):
    xh = mul(add(x, neg(mean.reshape(-1, 1, 1))), inv.reshape(-1, 1, 1))
    return add(mul(xh, w.reshape(-1, 1, 1), roundings=0), b.reshape(-1, 1, 1), roundings=1)


def bn_bwd_sums(dy, x, mean, inv, cnt):
    d = depth_of(cnt)
    xh = mul(add(x, neg(mean.reshape(-1, 1, 1))), inv.reshape(-1, 1, 1))
    db = vsum(dy, (1, 2), extra=0, depth=d)
    dg = vsum(mul(dy, xh), (1, 2), extra=0, depth=d)
    return db, dg, scale(db, float(cnt)), scale(dg, float(cnt)), xh


def bn_bwd_dx(dy, xh, mdy, mdyx, inv, w):
    inner = add(add(dy, neg(mdy.reshape(-1, 1, 1))), neg(mul(xh, mdyx.reshape(-1, 1, 1))))
    return mul(mul(w, inv).reshape(-1, 1, 1), inner)


def stack(*vs):
    return V(np.stack([x.val for x in vs]), np.stack([x.err for x in vs]))


def run(sd, v, a, d_out, momentum=0.1, eps=1e-5, device=None, propagate=False):
    """sd: fp32 state dict (parameters and buffers), v (K, N) fp32, a (K, N, N) fp32 (None: the contraction rows P are the
    device's, unchecked -- the scenes form builds its Laplacian itself), d_out (1, S, k, N) -> dict: ``out`` V (S, k, N),
    ``kept`` {name: V or list of V} (the names of ops.stgcnn_train_views; the statistics as ``stat_fwd`` / ``stat_bwd``
    [3] x (3, S) / (2, S)), ``kept_ratio``, ``grads`` {parameter name: V}, ``buffers`` {buffer name: V; num_batches_tracked: int},
    ``decisions``."""
    dec = Decisions()
    dv = (lambda k, j=None: None) if device is None else (lambda k, j=None: np.asarray(device[k] if j is None else device[k][j],
                                                                                       np.float64))
    P = lambda k: V(np.asarray(sd[k], np.float64))
    u = V(np.asarray(v, np.float64))
    K, n = u.shape
    S = np.asarray(sd["st_gcns.0.tcn.0.weight"]).shape[0]
    k = K - 2
    cnt = K * n
    has_res = "st_gcns.0.residual.0.weight" in sd
    n_tp = len([q for q in sd if q.startswith("prelus.")])
    A = max(1, n_tp - 1)
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
        _, keep = prelu_fwd(z, slope, dec, sign)
        if device is not None:   # the device's word decides everywhere, not only inside the band
            keep = sign
        z = force(name, z, j)
        y, _ = prelu_fwd(z, slope, Decisions(), keep)
        return z, y, keep

    # ------------------------------------------------------------------------------------------------ forward
    pre = "st_gcns.0."
    if a is None:
        Pk = V(dv("P"))
        kept["P"] = Pk
    else:
        X = V(np.concatenate([u.val, np.ones((1, n))]))                                       # (K + 1, n): the ones row last
        Pk = force("P", ein("jv,kvw->kjw", X, V(np.asarray(a, np.float64))))                  # (K, K + 1, n)
    Pp = V(np.stack([Pk.val[:, :K], np.broadcast_to(Pk.val[:, K:], (K, K, n))], 1),           # (K, 2, K, n)
           np.stack([Pk.err[:, :K], np.broadcast_to(Pk.err[:, K:], (K, K, n))], 1))
    coef = V(np.stack([np.asarray(sd[pre + "gcn.conv.weight"], np.float64).reshape(K, S),
                       np.asarray(sd[pre + "gcn.conv.bias"], np.float64).reshape(K, S)], 1))   # (K, 2, S): o = kk S + c
    g = force("g", ein("kjc,kjtw->ctw", coef, Pp))
    st = [None, None, None]
    st[0] = force("stat_fwd", stack(*bn_stats(g, cnt, eps)), 0)
    a1 = bn_apply(g, st[0][0], st[0][2], P(pre + "tcn.0.weight"), P(pre + "tcn.0.bias"))
    a1, y, keep1 = prelu_kept("a1", a1, P(pre + "tcn.1.weight"))
    y = force("y", y)
    tw = P(pre + "tcn.2.weight")
    t1 = force("t", conv(y.reshape(1, S, K, n), tw, P(pre + "tcn.2.bias")).reshape(S, K, n))
    st[1] = force("stat_fwd", stack(*bn_stats(t1, cnt, eps)), 1)
    tb = bn_apply(t1, st[1][0], st[1][2], P(pre + "tcn.3.weight"), P(pre + "tcn.3.bias"))
    if has_res:
        rw, rb = P(pre + "residual.0.weight").reshape(S, 1, 1), P(pre + "residual.0.bias").reshape(S, 1, 1)
        r = force("r", add(mul(rw, u.reshape(1, K, n), roundings=0), rb, roundings=1))
        st[2] = force("stat_fwd", stack(*bn_stats(r, cnt, eps)), 2)
        res = bn_apply(r, st[2][0], st[2][2], P(pre + "residual.1.weight"), P(pre + "residual.1.bias"))
    else:
        res = u.reshape(1, K, n)
    s, x, keep_s = prelu_kept("s", add(tb, res), P(pre + "prelu.weight"))
    x = force("x", x)
    cur = x.reshape(1, K, S, n)                                                              # the reference's view
    ins, pres, keeps = [], [], []
    for j in range(A):
        z = conv(cur, P(f"tpcnns.{j}.weight"), P(f"tpcnns.{j}.bias"))
        z, yj, kp = prelu_kept("tp_pre", z.reshape(k, S, n), P(f"prelus.{j}.weight"), j)
        yj = yj.reshape(1, k, S, n)
        if j:
            yj = add(yj, cur)
        ins.append(cur), pres.append(z), keeps.append(kp)
        cur = force("tp_out", yj.reshape(k, S, n), j).reshape(1, k, S, n)
    ow = P("tpcnn_ouput.weight")
    out = conv(cur, ow, P("tpcnn_ouput.bias")).reshape(S, k, n)

    # the running statistics, from the kept batch statistics
    mom = V(np.float64(momentum), U * abs(momentum))               # the device holds the momentum in fp32 ...
    one_m = V(np.float64(1.0 - momentum), 2 * U)                   # ... and forms 1 - m from that
    buffers = {}
    for b, name in enumerate(BN_NAMES):
        if st[b] is None:
            continue
        unb = mul(st[b][1], const(cnt / (cnt - 1.0)), roundings=3)
        buffers[name + ".running_mean"] = add(mul(one_m, P(name + ".running_mean")), mul(mom, st[b][0]))
        buffers[name + ".running_var"] = add(mul(one_m, P(name + ".running_var")), mul(mom, unb))
        buffers[name + ".num_batches_tracked"] = int(sd[name + ".num_batches_tracked"]) + 1

    # ------------------------------------------------------------------------------------------------ backward
    dp = depth_of(S * n)                                                                     # a 3x3 conv's (S, n) plane
    dfin = V(np.asarray(d_out, np.float64).reshape(1, k, S, n))                             # the same memory, (o, h, w)
    kept["d_fin"] = dfin.reshape(k, S, n)
    grads["tpcnn_ouput.bias"] = vsum(dfin, (0, 2, 3), extra=0, depth=dp)
    gcur, grads["tpcnn_ouput.weight"] = conv_bwd(dfin, cur, ow, depth=dp)
    gcur = force("d_tp_out", gcur.reshape(k, S, n), A - 1)
    for j in range(A - 1, -1, -1):
        dz, grads[f"prelus.{j}.weight"] = prelu_bwd(gcur, pres[j], P(f"prelus.{j}.weight"), keeps[j], depth=depth_of(k * S * n))
        dz = force("d_tp_pre", dz, j)
        dz4 = dz.reshape(1, k, S, n)
        grads[f"tpcnns.{j}.bias"] = vsum(dz4, (0, 2, 3), extra=0, depth=dp)
        din, grads[f"tpcnns.{j}.weight"] = conv_bwd(dz4, ins[j], P(f"tpcnns.{j}.weight"),
                                                    init=gcur.reshape(1, k, S, n) if j else None, depth=dp)
        gcur = force("d_tp_out", din.reshape(k, S, n), j - 1) if j else force("d_x", din.reshape(S, K, n))
    dsum = depth_of(S * K * n)
    ds, grads[pre + "prelu.weight"] = prelu_bwd(gcur, s, P(pre + "prelu.weight"), keep_s, depth=dsum)
    ds = force("d_s", ds)
    sb = [None, None, None]

    def bn_backward(b, dy, xin, wname):
        db, dg, mdy, mdyx, xh = bn_bwd_sums(dy, xin, st[b][0], st[b][2], cnt)
        grads[wname + ".weight"], grads[wname + ".bias"] = dg, db
        sb[b] = force("stat_bwd", stack(mdy, mdyx), b)
        return bn_bwd_dx(dy, xh, sb[b][0], sb[b][1], st[b][2], P(wname + ".weight"))

    dt = force("d_t", bn_backward(1, ds, t1, pre + "tcn.3"))
    if has_res:
        dr = force("d_r", bn_backward(2, ds, r, pre + "residual.1"))
        grads[pre + "residual.0.weight"] = ein("ctw,tw->c", dr, u, extra=0, depth=depth_of(cnt))
        grads[pre + "residual.0.bias"] = V(np.zeros(S))
    dy, dtw = conv_bwd(dt.reshape(1, S, K, n), y.reshape(1, S, K, n), tw, depth=depth_of(cnt))
    grads[pre + "tcn.2.weight"], grads[pre + "tcn.2.bias"] = dtw, V(np.zeros(S))
    dy = force("d_y", dy.reshape(S, K, n))
    da1, grads[pre + "tcn.1.weight"] = prelu_bwd(dy, a1, P(pre + "tcn.1.weight"), keep1, depth=dsum)
    da1 = force("d_a1", da1)
    dg = force("d_g", bn_backward(0, da1, g, pre + "tcn.0"))
    dcoef = ein("ctw,kjtw->kjc", dg, Pp, extra=0, depth=depth_of(cnt))
    grads[pre + "gcn.conv.weight"], grads[pre + "gcn.conv.bias"] = dcoef[:, 0], dcoef[:, 1]
    for name in unused_names(sd):
        grads[name] = V(np.zeros(np.asarray(sd[name]).shape))
    for name, gk in grads.items():   # the final rounding of every stored gradient
        gk.err = gk.err + U * np.abs(gk.val)
        shape = np.asarray(sd[name]).shape
        if gk.shape != shape:
            grads[name] = V(np.ascontiguousarray(gk.val).reshape(shape), np.ascontiguousarray(gk.err).reshape(shape))
    kept = {q: [val[j] for j in sorted(val)] if isinstance(val, dict) else val for q, val in kept.items()}
    return dict(out=out, kept=kept, kept_ratio=kept_ratio, grads={q: grads[q] for q in parameter_names(sd)}, buffers=buffers,
                decisions=dec.figures())


GROUPS = ("gcn", "tcn", "residual", "prelu", "tpcnns", "tpcnn_ouput", "prelus")


def group_of(key):
    """st_gcns.0.<group>.* -> gcn / tcn / residual / prelu; else the key's first component"""
    part = key.split(".")
    g = part[2] if part[0] == "st_gcns" else part[0]
    if g not in GROUPS:
        raise KeyError(key)
    return g


def exact_zero_names(sd):
    return tuple(q for q in ZERO_GRADS if q in sd) + tuple(unused_names(sd))


def vacuous(sd, grads, n):
    """the tensors of more than one element whose bound reaches half their largest entry: a bound below that cannot pass
    zeros, a flipped sign or a wrong scale at that entry.  The exact-zero tensors are excepted; so is a one-element tensor, a
    sum over the whole scene that can cancel, and a tensor that is exactly zero with bound 0 (a scene of one pedestrian has
    L = 0: the gcn output, its gradients and tcn.0's weight gradient are exact zeros)."""
    skip = exact_zero_names(sd)
    if n <= 2:
        # two pedestrians: L[kk] = c_kk [[1, -1], [-1, 1]], so the contraction rows are rank one, P[kk, t, :] = c_kk (u[t, 0] -
        # u[t, 1]) [1, -1], and the ones row vanishes: the gcn output of every channel is a multiple of ONE pattern whatever the
        # weights, tcn.0's BatchNorm divides the multiple out, and the gcn gradients are analytically zero (what is left is
        # rounding: nothing a bound could be small against).  One pedestrian: L = 0.
        skip += ("st_gcns.0.gcn.conv.weight", "st_gcns.0.gcn.conv.bias")
    return [q for q, g in grads.items() if q not in skip and g.val.size > 1 and g.err.max() > 0
            and g.err.max() >= 0.5 * np.abs(g.val).max()]


def device_dict(views, n_bn=3):
    """``ops.stgcnn_train_views``' result (torch views or numpy copies) -> the ``device=`` argument of :func:`run`"""
    f = lambda t: np.asarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, np.float64)
    out = {q: ([f(t) for t in val] if isinstance(val, list) else f(val)) for q, val in views.items()}
    out["stat_fwd"] = [out["stats"][b, :3] for b in range(n_bn)]
    out["stat_bwd"] = [out["stats"][b, 3:] for b in range(n_bn)]
    return out
