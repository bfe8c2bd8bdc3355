"""float64 numpy restatement of the training pass of csrc/et_sgcn_train.inl, independent of torch: SGCN's forward
(tests/_sgcn_np.py's, in the kernels' collapsed-attention form, every kept value returned), the backward pass to all
parameters, and a running elementwise bound for what the fp32 kernels may differ by.  The bounds are the only tolerances
tests/test_gpu_sgcn_train.py uses; they are derived here, not tuned.  Not a test module itself.

The bound.  u = 2^-24, gamma_K = K u / (1 - K u).  Every value is a :class:`V`: the float64 value and a bound ``err`` of the
kernel's fp32 value of it.  A sum of K products of computed operands (|x^ - x| <= ex, |y^ - y| <= ey) obeys, for ANY order
of summation and with or without contraction (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., eq. 3.5 and
section 4.2),

    |fl(s^) - s|  <=  gamma_(K+R) sum (|x| + ex)(|y| + ey)  +  sum ex (|y| + ey) + |x| ey          (:func:`ein`)

with K the TRUE number of terms of the element (all pedestrians, rows or positions of the scene for a weight gradient: the
per-workgroup partials and their fixed-order sum are one such sum in some order) and R the roundings around the chain.
Products, quotients and differences carry one rounding each; expf is taken as correct to 2 ulp; exp, the sigmoid and the
quotient propagate their operands' bounds through their derivatives' suprema over the operand's interval.  The float64
arithmetic of this file has its own rounding, bounded the same way with 2^-53; U below is 2^-24 + 2^-50, which covers both.
Where the kernel regroups a formula to avoid a cancellation (the ZeroSoftmax backward around the row's first entry), this
file follows the kernel's grouping, because the bound of a difference is the sum of its parts' bounds.

Hard decisions.  ``sigmoid(logit) > 0.5`` and the sign of every PReLU argument.  An argument inside its band -- DELTA of
tests/_sgcn_np.py for a logit, its own bound for a PReLU argument -- is UNDECIDED: there the decision is the device's, read
from the kept forward values (``device=``: what ``ops.sgcn_train_views`` returns, as numpy); outside the band it is this
file's own, and a device decision that differs is counted as a flip.  Without ``device`` every decision is this file's.

Layer by layer.  A worst-case bound carried through seven asymmetric layers grows by the layers' absolute row sums (about
4.6 each for the test weights) and says nothing at the end.  The training forward keeps every layer's input, so the forward
is checked LAYER-LOCALLY: each kept value is formed here from the DEVICE's kept inputs of its layer (exact fp32 numbers, bound
0) and compared with the device's within the bound of that one layer (``kept_ratio``); then the device's value goes on to the
next layer.  A PReLU argument's band is therefore its own layer's bound, and a device decision outside it is an error, not a
tolerance.  The backward pass starts from these forward values, which are also what the device's backward reads, and
is checked the same way: the device keeps d ts, d f1, d f2, the tail's part of d A_t, d (A_s f2), the gradient of every kept
stack, the direct parts of d dense and d dense_s, each is formed here from the device's values of the step before and compared
within that one step's bound, and a weight gradient's bound is that of its own sum over the scene.  Only the tail's chain
(output layer, tcns, fusion_, gcn 1: one kernel, its intermediate gradients live in LDS) is carried from d out to d ts, d f1
and d A_t in one piece.  Without ``device`` the file's own kept values take that place (bound reset to 0 at every kept value),
so the bands of a CPU-only run are the same layer-local ones."""
import numpy as np

from . import _sgcn_np as SN

U = 2.0 ** -24 + 2.0 ** -50
H, D = SN.H, SN.D
SWA = SN.SWA


def gamma(k):
    return k * U / (1.0 - k * U)


class V:
    """a float64 array, the elementwise bound of the kernel's fp32 value of it and, for a sum, ``tm``: the sum of its terms'
    magnitudes (what a different order of summation is bounded by)"""

    def __init__(self, val, err=None, tm=None):
        self.val = np.asarray(val, np.float64)
        self.err = np.zeros_like(self.val) if err is None else np.broadcast_to(np.asarray(err, np.float64), self.val.shape)
        self.tm = tm

    def __getitem__(self, idx):
        return V(self.val[idx], self.err[idx])

    @property
    def mag(self):
        return np.abs(self.val) + self.err

    @property
    def shape(self):
        return self.val.shape

    def t(self, *axes):
        return V(self.val.transpose(*axes), self.err.transpose(*axes))

    def reshape(self, *shape):
        tm = None if self.tm is None else np.asarray(self.tm).reshape(*shape)
        return V(self.val.reshape(*shape), np.ascontiguousarray(self.err).reshape(*shape), tm)


def _terms(spec, shapes):
    ins, out = spec.split("->")
    size = {}
    for names, shape in zip(ins.split(","), shapes):
        for c, s in zip(names, shape):
            size[c] = s
    k = 1
    for c, s in size.items():
        if c not in out:
            k *= s
    return max(k, 1)


def ein(spec, x, y, extra=2, init=None, depth=None):
    """einsum(spec, x, y) (+ init, the chain's first accumulator: it meets every rounding of the chain) as a sum of its
    TRUE number of products per element in any order, ``extra`` more roundings.  ``depth``: the sum is a tree (a lane's
    ascending chain, the butterfly over the lanes, the wavefronts, the per-workgroup partials): no term meets more than
    ``depth`` additions, which then stands in place of the number of terms (Higham, section 4.2: gamma of the tree's depth)"""
    val = np.einsum(spec, x.val, y.val)
    mag = np.einsum(spec, x.mag, y.mag)
    err = np.einsum(spec, x.err, y.mag) + np.einsum(spec, np.abs(x.val), y.err)
    if init is not None:
        val, mag, err = val + init.val, mag + init.mag, err + init.err
    k = _terms(spec, (x.shape, y.shape))
    return V(val, gamma((k if depth is None else min(k, depth)) + extra) * mag + err, tm=mag)


def mul(x, y, roundings=1):
    val = x.val * y.val
    return V(val, x.err * y.mag + np.abs(x.val) * y.err + gamma(roundings) * x.mag * y.mag)


def add(*parts, roundings=None):
    r = len(parts) - 1 if roundings is None else roundings
    val = sum(p.val for p in parts)
    return V(val, sum(p.err for p in parts) + gamma(r) * sum(p.mag for p in parts))


def neg(x):
    return V(-x.val, x.err)


def div(x, y):
    val = x.val / y.val
    lo = np.maximum(np.abs(y.val) - y.err, 1e-300)
    return V(val, (x.err + np.abs(val) * y.err) / lo + U * (np.abs(val) + x.err / lo))


def vexp(x):
    val = np.exp(x.val)
    exact = (x.val == 0) & (x.err == 0)   # expf(0) = 1
    return V(val, np.where(exact, 0.0, val * np.expm1(x.err) + 4 * U * val * np.exp(x.err)))


def vsum(x, axis, keepdims=False, extra=1, depth=None):
    k = int(np.prod([x.shape[a] for a in (axis if isinstance(axis, tuple) else (axis,))]))
    k = k if depth is None else min(k, depth)
    mag = x.mag.sum(axis=axis, keepdims=keepdims)
    return V(x.val.sum(axis=axis, keepdims=keepdims), x.err.sum(axis=axis, keepdims=keepdims) + gamma(k + extra) * mag, tm=mag)


def const(a):
    return V(np.asarray(a, np.float64))


class Decisions:
    """the bookkeeping of the hard decisions: per kind ("mask" / "prelu") the entries, those inside the band and the device's
    flips outside it"""

    def __init__(self):
        self.count = {"mask": [0, 0, 0], "prelu": [0, 0, 0]}

    def take(self, kind, own, band, dev):
        c = self.count[kind]
        c[0] += own.size
        c[1] += int(band.sum())
        if dev is None:
            return own
        dev = np.asarray(dev, bool)
        c[2] += int(((dev != own) & ~band).sum())
        return np.where(band, dev, own)

    def figures(self):
        return {k: dict(entries=c[0], undecided=c[1], flips_outside_band=c[2]) for k, c in self.count.items()}


def prelu_fwd(z, a, dec, dev_sign=None):
    """PReLU of V z with slope V a (scalar) -> (out, keep): keep = z > 0, the device's inside the band |z| <= err"""
    own = z.val > 0
    band = (np.abs(z.val) <= z.err) & (z.err > 0)
    keep = dec.take("prelu", own, band, dev_sign)
    neg_ = mul(a, z)
    return V(np.where(keep, z.val, neg_.val), np.where(keep, z.err, neg_.err)), keep


def prelu_bwd(g, z, a, keep, depth=None):
    """-> (d z, d a): d z = g where kept else a g; d a = sum g z over the others (``depth``: of that sum, as :func:`ein`)"""
    ag = mul(a, g)
    dz = V(np.where(keep, g.val, ag.val), np.where(keep, g.err, ag.err))
    gz = mul(g, z)
    gz = V(np.where(keep, 0.0, gz.val), np.where(keep, 0.0, gz.err))
    return dz, vsum(gz, tuple(range(gz.val.ndim)), depth=depth).reshape(1)


def patches(x, kp, kq):
    """x (B, C, P, Q) -> (B, C * kp * kq, P, Q): the zero-padded neighbours a kp x kq convolution reads, channel-major"""
    B, C, P, Q = x.shape
    pp, pq = kp // 2, kq // 2
    pad = ((0, 0), (0, 0), (pp, pp), (pq, pq))
    xv, xe = np.pad(x.val, pad), np.pad(x.err, pad)
    val = np.stack([xv[:, :, a:a + P, b:b + Q] for a in range(kp) for b in range(kq)], axis=2)
    err = np.stack([xe[:, :, a:a + P, b:b + Q] for a in range(kp) for b in range(kq)], axis=2)
    return V(val.reshape(B, C * kp * kq, P, Q), err.reshape(B, C * kp * kq, P, Q))


def conv(x, w, b=None):
    """w (O, C, kp, kq) on x (B, C, P, Q), padded to the same size (+ b)"""
    O, C, kp, kq = w.shape
    return ein("ok,bkpq->bopq", w.reshape(O, C * kp * kq), patches(x, kp, kq), init=None if b is None else b.reshape(1, O, 1, 1))


def conv_bwd(dz, x, w, init=None, depth=None):
    """-> (d x (+ init, the chain's first accumulator), d w) of conv(x, w); ``depth``: of d w's sum, as :func:`ein`"""
    O, C, kp, kq = w.shape
    dw = ein("bopq,bkpq->ok", dz, patches(x, kp, kq), depth=depth).reshape(O, C, kp, kq)
    wt = V(w.val[:, :, ::-1, ::-1].transpose(1, 0, 2, 3).reshape(C, O * kp * kq),
           w.err[:, :, ::-1, ::-1].transpose(1, 0, 2, 3).reshape(C, O * kp * kq))
    return ein("ck,bkpq->bcpq", wt, patches(dz, kp, kq), init=init), dw


def prep(sd, a):
    """the collapsed attention of attention ``a`` (0 spatial, 1 temporal) -> dict of float64 arrays and alpha, beta as V"""
    p = SWA + ("spatial_attention." if a == 0 else "temporal_attention.")
    f = lambda k: np.asarray(sd[p + k], np.float64)
    we, be, Wq, bq, Wk = f("embedding.weight")[:, 0], f("embedding.bias"), f("query.weight"), f("query.bias"), f("key.weight")
    aq, cq, ak = Wq @ we, Wq @ be + bq, Wk @ we
    alpha = (aq * ak).reshape(H, D).sum(1) / 8.0
    beta = (cq * ak).reshape(H, D).sum(1) / 8.0
    return dict(we=we, be=be, Wq=Wq, Wk=Wk, aq=aq, cq=cq, ak=ak, alpha=V(alpha, U * np.abs(alpha)), beta=V(beta, U * np.abs(beta)))


def prep_bwd(pr, dalpha, dbeta, names):
    """step 7: d alpha, d beta (V (4,)) -> {name: V} of the six tensors of one attention (fp64 on the device, one rounding
    to fp32 at the end)"""
    rep = lambda x: V(np.repeat(x.val, D), np.repeat(x.err, D))
    da, db = rep(dalpha), rep(dbeta)
    c = lambda x: V(np.asarray(x, np.float64))
    daq = mul(da, c(pr["ak"] / 8.0))
    dcq = mul(db, c(pr["ak"] / 8.0))
    dak = add(mul(da, c(pr["aq"] / 8.0)), mul(db, c(pr["cq"] / 8.0)))
    dWq = add(ein("c,e->ce", daq, c(pr["we"])), ein("c,e->ce", dcq, c(pr["be"])))
    dWk = ein("c,e->ce", dak, c(pr["we"]))
    dwe = add(ein("ce,c->e", c(pr["Wq"]), daq), ein("ce,c->e", c(pr["Wk"]), dak))
    dbe = ein("ce,c->e", c(pr["Wq"]), dcq)
    return {names + "embedding.weight": dwe.reshape(64, 1), names + "embedding.bias": dbe, names + "query.weight": dWq,
            names + "query.bias": dcq, names + "key.weight": dWk, names + "key.bias": V(np.zeros(64))}


def _softmax_rows(score, force):
    """score V (..., L) -> dense V as the kernels form it, exp(score - max) / sum, from the kept (max, sum) records"""
    m = score.val.max(axis=-1)
    m_err = score.err.max(axis=-1)
    sc = V(score.val - m[..., None], score.err + m_err[..., None] + U * np.abs(score.val - m[..., None]))
    s = vsum(vexp(sc), -1, extra=0)
    rec = force(V(np.stack([m, s.val], -1), np.stack([m_err, s.err], -1)))
    m, s = rec.val[..., :1], V(rec.val[..., 1:], rec.err[..., 1:])
    return div(vexp(V(score.val - m, score.err + U * np.abs(score.val - m))), s)


def _sigmoid(l):
    s = 1.0 / (1.0 + np.exp(-l.val))
    return V(s, 0.25 * l.err + 8 * U * s)   # |sigma'| <= 1/4; exp, the sum and the quotient: a few roundings


def _zsm_fwd(dn, mk):
    x = mul(dn, mk)
    ex = vexp(x)
    em1 = V(ex.val - 1.0, ex.err + U * np.abs(ex.val - 1.0))
    e = mul(em1, em1)
    ssum = vsum(e, -1, keepdims=True, extra=0)
    den = V(ssum.val + 1e-5, ssum.err + U * (ssum.val + 1e-5))
    return x, ex, em1, e, den


def _zsm_bwd(dA, e, den, ex, em1, dn, mk, keep, sg):
    """ZeroSoftmax, mask and sigmoid backward of rows (..., L), the kernels' grouping around the row's first entry ->
    (direct part of d dense, d logit)"""
    c0 = V(dA.val[..., :1], dA.err[..., :1])
    dd = add(dA, neg(c0))
    y = div(e, den)
    sdy = vsum(mul(dd, y, roundings=2), -1, keepdims=True, extra=0)
    tail0 = mul(c0, div(const(1e-5), den))
    de = div(add(add(dd, neg(sdy)), tail0), den)
    fac = mul(mul(const(2.0), em1, roundings=0), ex)
    dx = mul(de, fac)
    direct = mul(mk, dx)
    s1 = V(1.0 - sg.val, sg.err + U)
    dl = mul(mul(dn, dx), mul(sg, s1))
    return direct, V(np.where(keep, dl.val, 0.0), np.where(keep, dl.err, 0.0))


def _mask(logit, identity, dec, dev_logit):
    own = logit.val > 0
    band = np.abs(logit.val) < SN.DELTA
    keep = dec.take("mask", own, band, None if dev_logit is None else SN.decisions_fp32(dev_logit))
    sg = _sigmoid(logit)
    ident = np.broadcast_to(np.asarray(identity, np.float64), logit.shape)
    mk = V(np.where(keep, sg.val, 0.0) + ident, np.where(keep, sg.err, 0.0) + U * (1.0 + ident))
    return mk, keep, sg


def run(sd, v, identity_s, identity_t, d_out, device=None, propagate=False):
    """sd: fp32 state dict, v (T, N) fp32, the identities as tests/_sgcn_np.forward takes them, d_out (pred_len, N, S) ->
    dict: ``out`` V, ``kept`` {name: V or list of V} (the names of ops.sgcn_train_views), ``grads`` {state_dict name: V},
    ``decisions`` (:meth:`Decisions.figures`).  ``device``: the kept values of the device run (numpy), for the decisions
    inside the bands.  ``propagate`` (without ``device``): no bound is reset, every value carries the worst case of the whole
    chain before it -- loose behind many layers, but a bound on the distance to the exact gradient, which is what a comparison
    with another implementation's float64 gradients needs."""
    dec = Decisions()
    dv = (lambda k, j=None: None) if device is None else (lambda k, j=None: np.asarray(device[k] if j is None else device[k][j],
                                                                                       np.float64))
    P = lambda k: V(np.asarray(sd[k], np.float64))
    x = V(np.asarray(v, np.float64))
    T, N = x.shape
    na, nt = SN.n_layers(sd)
    ids = np.asarray(identity_s, np.float64)[:, None]                       # (1 or T, 1, N, N)
    idt = np.asarray(identity_t, np.float64)[:, None]                       # (N, 1, 1 or T, 1 or T)
    kept, grads, kept_ratio = {"v": x}, {}, {}

    def force(name, val, j=None, to_dev=lambda a: a, from_dev=lambda a: a):
        """a kept value: recorded (device layout), compared with the device's, and replaced by it (or by itself, bound 0)"""
        rec = V(to_dev(val.val), to_dev(val.err))
        if j is None:
            kept[name] = rec
        else:
            kept.setdefault(name, []).append(rec)
        if device is None:
            return val if propagate else V(val.val)
        d = dv(name, j)
        kept_ratio[name] = max(kept_ratio.get(name, 0.0), compare(d, rec))
        return V(from_dev(d.reshape(rec.shape)))

    # ------------------------------------------------------------------------------------------------ forward
    pr = [prep(sd, 0), prep(sd, 1)]
    xe = V(x.val[:, None, :], x.err[:, None, :])                            # (T, 1, N)
    ti_s = add(mul(xe, pr[0]["alpha"].reshape(1, H, 1), roundings=0), pr[0]["beta"].reshape(1, H, 1), roundings=1)   # (T,H,N)
    score_s = mul(V(ti_s.val[..., None], ti_s.err[..., None]), V(x.val[:, None, None, :]))              # (T,H,N,N)
    dense_s = _softmax_rows(score_s, lambda r: force("rows_s", r))
    xn = V(x.val.T[:, None, :])                                                                          # (N, 1, T)
    ti_t = add(mul(xn, pr[1]["alpha"].reshape(1, H, 1), roundings=0), pr[1]["beta"].reshape(1, H, 1), roundings=1)   # (N,H,T)
    score_t = mul(V(ti_t.val[..., None], ti_t.err[..., None]), V(x.val.T[:, None, None, :]))            # (N,H,T,T)
    dense_t = _softmax_rows(score_t, lambda r: force("rows_t", r))
    fw, fb, fa = P(SWA + "spa_fusion.conv.0.weight").reshape(T, T), P(SWA + "spa_fusion.conv.0.bias"), P(SWA + "spa_fusion.conv.1.weight")
    facc = ein("ut,thij->uhij", fw, dense_s, init=fb.reshape(T, 1, 1, 1))
    dev0 = None if device is None else (dv("stack_s", 0) - dense_s.val) > 0
    fpre, keep_f = prelu_fwd(facc, fa, dec, dev0)
    stack_s, stack_t = [force("stack_s", add(fpre, dense_s), 0)], [force("stack_t", dense_t, 0)]
    dense_t = stack_t[0]   # the kept temporal attention is what the backward reads
    keep_as, keep_at, z_as, z_at = [], [], [], []

    def asym_fwd(xin, p, dev_next, dev_in):
        w1, w2, b2, a = P(p + "conv1.weight"), P(p + "conv2.weight"), P(p + "conv2.bias"), P(p + "activation.weight")
        z = add(conv(xin, w2, b2), conv(xin, w1))
        dev_sign = None if dev_next is None else (dev_next - dev_in) > 0
        y, keep = prelu_fwd(z, a, dec, dev_sign)
        return add(y, xin), z, keep

    for j in range(na):
        o, z, kp = asym_fwd(stack_s[j], f"{SWA}interaction_mask.spatial_asymmetric_convolutions.{j}.", dv("stack_s", j + 1), dv("stack_s", j))
        stack_s.append(force("stack_s", o, j + 1)), z_as.append(z), keep_as.append(kp)
        o, z, kp = asym_fwd(stack_t[j], f"{SWA}interaction_mask.temporal_asymmetric_convolutions.{j}.", dv("stack_t", j + 1), dv("stack_t", j))
        stack_t.append(force("stack_t", o, j + 1)), z_at.append(z), keep_at.append(kp)
    mk_s, keep_ms, sg_s = _mask(stack_s[-1], ids, dec, dv("stack_s", na))
    mk_t, keep_mt, sg_t = _mask(stack_t[-1], idt, dec, dv("stack_t", na))
    _, ex_s, em1_s, e_s, den_s = _zsm_fwd(dense_s, mk_s)
    _, ex_t, em1_t, e_t, den_t = _zsm_fwd(dense_t, mk_t)
    gw = [P(f"stsgcn.{nm}_sparse_gcn.{i}.embedding.weight") for nm in ("spatial_temporal", "temporal_spatial") for i in (0, 1)]
    ga = [P(f"stsgcn.{nm}_sparse_gcn.{i}.activation.weight") for nm in ("spatial_temporal", "temporal_spatial") for i in (0, 1)]
    A_t = force("at", div(e_t, den_t))                                                                  # (N,H,T,T)
    acc_t = ein("nhtu,un->nht", A_t, x, extra=1)
    z2 = mul(V(acc_t.val[..., None], acc_t.err[..., None]), gw[2].reshape(1, 1, 1, D))
    f2, keep2 = prelu_fwd(z2, ga[2], dec, None if device is None else dv("f2") > 0)
    f2 = force("f2", f2)
    den3 = V(den_s.val[..., 0], den_s.err[..., 0])                                                      # (T,H,N)
    ax = div(ein("thij,tj->thi", e_s, x, extra=1), den3)
    z0 = mul(V(ax.val[..., None], ax.err[..., None]), gw[0].reshape(1, 1, 1, D))
    f1, keep0 = prelu_fwd(z0, ga[0], dec, None if device is None else dv("f1") > 0)
    f1 = force("f1", f1)
    accn = div(ein("thij,jhtd->thid", e_s, f2, extra=1), V(den_s.val, den_s.err))
    o3 = ein("dq,thiq->thid", gw[3], accn, extra=1)
    ts_thid, keep3 = prelu_fwd(o3, ga[3], dec, None if device is None else dv("ts").transpose(2, 1, 0, 3) > 0)
    ts = force("ts", ts_thid.t(2, 1, 0, 3))                                                             # (N,H,T,D)
    Gm = ein("nhtu,uhnd->nhtd", A_t, f1, extra=1)
    z1 = ein("dq,nhtq->nhtd", gw[1], Gm, extra=1)
    to_keep = lambda a: np.ascontiguousarray(a.transpose(0, 2, 1, 3)).reshape(N, T, H * D)              # (N,H,T,D) -> (N,T,64)
    from_keep = lambda a: a.reshape(N, T, H, D).transpose(0, 2, 1, 3)
    _, keep1 = prelu_fwd(z1, ga[1], dec, None if device is None else from_keep(dv("st_pre")) > 0)
    z1 = force("st_pre", z1, None, to_keep, from_keep)
    st, _ = prelu_fwd(z1, ga[1], Decisions(), keep1)
    fus = P("fusion_.weight").reshape(H, H)
    rep = force("rep", add(ein("hg,ngtd->nhtd", fus, st, extra=1), ts), None, to_keep, from_keep)
    xs = [rep.t(0, 2, 1, 3)]                                                                            # (N, C, H, D)
    keep_tc, z_tc = [], []
    flat = (lambda a: a.reshape(N, -1, H * D)), (lambda a: a.reshape(N, -1, H, D))
    for j in range(nt):
        z = conv(xs[j], P(f"tcns.{j}.0.weight"), P(f"tcns.{j}.0.bias"))
        _, kp = prelu_fwd(z, P(f"tcns.{j}.1.weight"), dec, None if device is None else flat[1](dv("tcn_pre", j)) > 0)
        z = force("tcn_pre", z, j, *flat)
        y, _ = prelu_fwd(z, P(f"tcns.{j}.1.weight"), Decisions(), kp)
        if j:
            y = add(y, xs[j])
        xs.append(force("tcn_out", y, j, *flat)), z_tc.append(z), keep_tc.append(kp)
    ow, ob = P("output.weight"), P("output.bias")
    lin = ein("sq,nthq->nths", ow, xs[-1], init=ob)
    out = vsum(lin, 2, extra=0)
    out = V(0.25 * out.val, 0.25 * out.err).t(1, 0, 2)
    # ------------------------------------------------------------------------------------------------ backward
    # the depth of every weight gradient's summation tree (csrc/et_sgcn_train.inl): a lane's own chain, 6 butterfly steps, 4
    # wavefronts, the scene's per-workgroup partials (chunks of ET_SGCN_BWD_CHUNK pedestrians / _ROWS rows / _ITEMS positions)
    from eigentrajectory_amd import _lib as L
    cd = lambda a, b: -(-a // b)
    tree = lambda lane, slots: lane + 6 + 4 + slots
    k_ = xs[-1].shape[1]
    s_tail = L.SGCN_BWD_CHUNK + cd(N, L.SGCN_BWD_CHUNK)                     # a chunk's pedestrians, then the chunks
    s_rows, s_rows2 = cd(4 * T * N, L.SGCN_BWD_ROWS), cd(8 * T * N, L.SGCN_BWD_ROWS)
    s_stack = {"spatial": cd(T * N * N, L.SGCN_BWD_ITEMS), "temporal": cd(N * T * T, L.SGCN_BWD_ITEMS)}
    s_fuse = cd(4 * N * N, L.SGCN_BWD_ITEMS)
    per_lane = cd(L.SGCN_BWD_ITEMS, 256)
    g = V(0.25 * np.asarray(d_out, np.float64))                                                         # (k, N, S)
    go = V(np.asarray(d_out, np.float64))
    grads["output.bias"] = vsum(go, (0, 1), depth=k_ + s_tail)
    xh = vsum(xs[-1], 2, extra=0)                                                                       # (N, k, D): heads summed
    grads["output.weight"] = ein("tns,ntq->sq", g, xh, extra=2 + H, depth=H * k_ + s_tail)
    gx = ein("tns,sq->ntq", g, ow)
    gx = V(np.repeat(gx.val[:, :, None, :], H, 2), np.repeat(gx.err[:, :, None, :], H, 2))              # (N, k, H, D)
    for j in range(nt - 1, -1, -1):
        a = P(f"tcns.{j}.1.weight")
        dz, da = prelu_bwd(gx, z_tc[j], a, keep_tc[j], depth=tree(cd(k_ * 64, 256), s_tail))
        grads[f"tcns.{j}.1.weight"] = da
        grads[f"tcns.{j}.0.bias"] = vsum(dz, (0, 2, 3), depth=64 + s_tail)
        gx, grads[f"tcns.{j}.0.weight"] = conv_bwd(dz, xs[j], P(f"tcns.{j}.0.weight"), init=gx if j else None, depth=64 + s_tail)
    drep = force("d_ts", gx.t(0, 2, 1, 3))                                                              # (N,H,T,D)
    grads["fusion_.weight"] = ein("nhtd,ngtd->hg", drep, st, depth=T * D + s_tail).reshape(H, H, 1, 1)
    dst = ein("hg,nhtd->ngtd", fus, drep)
    dz1, grads["stsgcn.spatial_temporal_sparse_gcn.1.activation.weight"] = prelu_bwd(dst, z1, ga[1], keep1,
                                                                                         depth=tree(cd(T * 64, 256), s_tail))
    grads["stsgcn.spatial_temporal_sparse_gcn.1.embedding.weight"] = ein("nhtd,nhtq->dq", dz1, Gm, depth=T * H + s_tail)
    dGm = ein("dq,nhtd->nhtq", gw[1], dz1)
    dat = force("d_at", ein("nhtd,uhnd->nhtu", dGm, f1))
    df1 = force("d_f1", ein("nhtu,nhtd->uhnd", A_t, dGm))
    # sadj
    dz0, grads["stsgcn.spatial_temporal_sparse_gcn.0.activation.weight"] = prelu_bwd(df1, z0, ga[0], keep0,
                                                                                         depth=tree(4 * D, s_rows))
    grads["stsgcn.spatial_temporal_sparse_gcn.0.embedding.weight"] = ein("thid,thi->d", dz0, ax, depth=tree(4, s_rows)).reshape(D, 1)
    dax = ein("thid,d->thi", dz0, gw[0].reshape(D))
    dzo, grads["stsgcn.temporal_spatial_sparse_gcn.1.activation.weight"] = prelu_bwd(drep.t(2, 1, 0, 3), o3, ga[3], keep3,
                                                                                         depth=tree(4 * D, s_rows))
    grads["stsgcn.temporal_spatial_sparse_gcn.1.embedding.weight"] = ein("thid,thiq->dq", dzo, accn,
                                                                         depth=L.SGCN_BWD_ROWS + s_rows)   # one lane per (d, q)
    daccn = force("d_accn", ein("dq,thid->thiq", gw[3], dzo))
    dA_s = ein("thiq,jhtq->thij", daccn, f2, init=mul(V(dax.val[..., None], dax.err[..., None]), V(x.val[:, None, None, :])))
    A_s = div(e_s, den_s)
    df2 = force("d_f2", ein("thij,thiq->jhtq", A_s, daccn))
    dir_s, dl_s = _zsm_bwd(dA_s, e_s, den_s, ex_s, em1_s, dense_s, mk_s, keep_ms, sg_s)
    dir_s, dl_s = force("dir_s", dir_s), force("g_s", dl_s, na)
    # tadj
    dz2, grads["stsgcn.temporal_spatial_sparse_gcn.0.activation.weight"] = prelu_bwd(df2, z2, ga[2], keep2,
                                                                                         depth=tree(4 * D, s_rows))
    grads["stsgcn.temporal_spatial_sparse_gcn.0.embedding.weight"] = ein("nhtd,nht->d", dz2, acc_t, depth=tree(4, s_rows)).reshape(D, 1)
    dacc = ein("nhtd,d->nht", dz2, gw[2].reshape(D))
    dA_t = add(mul(V(dacc.val[..., None], dacc.err[..., None]), V(x.val.T[:, None, None, :]), roundings=0), dat, roundings=1)
    dir_t, dl_t = _zsm_bwd(dA_t, e_t, den_t, ex_t, em1_t, dense_t, mk_t, keep_mt, sg_t)
    dir_t, dl_t = force("dir_t", dir_t), force("g_t", dl_t, na)
    # asym, last layer to first
    for name, stack, zs, keeps, gcur in (("spatial", stack_s, z_as, keep_as, dl_s), ("temporal", stack_t, z_at, keep_at, dl_t)):
        for j in range(na - 1, -1, -1):
            p = f"{SWA}interaction_mask.{name}_asymmetric_convolutions.{j}."
            dp = tree(per_lane, s_stack[name])
            dz, grads[p + "activation.weight"] = prelu_bwd(gcur, zs[j], P(p + "activation.weight"), keeps[j], depth=dp + 3 * per_lane)
            grads[p + "conv2.bias"] = vsum(dz, (0, 2, 3), depth=dp)
            d2, grads[p + "conv2.weight"] = conv_bwd(dz, stack[j], P(p + "conv2.weight"), depth=dp)
            d1, grads[p + "conv1.weight"] = conv_bwd(dz, stack[j], P(p + "conv1.weight"), depth=dp)
            gcur = force("g_s" if name == "spatial" else "g_t", add(gcur, d2, d1, roundings=24), j)   # one chain of 24
        if name == "spatial":
            g_s0 = gcur
        else:
            g_t0 = gcur
    # fuse
    dfacc, grads[SWA + "spa_fusion.conv.1.weight"] = prelu_bwd(g_s0, facc, fa, keep_f, depth=tree(cd(L.SGCN_BWD_ITEMS, 128) * T, s_fuse))
    grads[SWA + "spa_fusion.conv.0.bias"] = vsum(dfacc, (1, 2, 3), depth=L.SGCN_BWD_ITEMS + s_fuse)   # one lane per u / per (u, t)
    grads[SWA + "spa_fusion.conv.0.weight"] = ein("uhij,thij->ut", dfacc, dense_s, depth=L.SGCN_BWD_ITEMS + s_fuse).reshape(T, T, 1, 1)
    dd_s = force("dd_s", add(ein("ut,uhij->thij", fw, dfacc, init=g_s0), dir_s))
    dd_t = add(g_t0, dir_t)
    # softmax rows and the collapsed attention
    dab = []
    for a, (dn, dd, xrow, xcol) in enumerate(((dense_s, dd_s, x.val[:, None, None, :], x.val[:, None, :]),
                                              (dense_t, dd_t, x.val.T[:, None, None, :], x.val.T[:, None, :]))):
        s = vsum(mul(dn, dd, roundings=0), -1, keepdims=True, extra=1)
        dscore = mul(dn, add(dd, neg(s)))
        dti = vsum(mul(dscore, V(xrow), roundings=0), -1, extra=1)                                       # (T,H,N) / (N,H,T)
        dalpha = vsum(mul(dti, V(np.broadcast_to(xcol, dti.shape)), roundings=0), (0, 2), extra=1, depth=tree(4, s_rows2))
        dbeta = vsum(dti, (0, 2), depth=tree(4, s_rows2))
        dab.append((dalpha, dbeta))
        grads.update(prep_bwd(pr[a], dalpha, dbeta, SWA + ("spatial_attention." if a == 0 else "temporal_attention.")))
    for k, gk in grads.items():   # the final rounding of every stored gradient
        gk.err = gk.err + U * np.abs(gk.val)
        shape = np.asarray(sd[k]).shape
        if gk.shape != shape:
            grads[k] = gk.reshape(*shape)
    return dict(out=out, kept=kept, kept_ratio=kept_ratio, grads={k: grads[k] for k in sd}, decisions=dec.figures(), dab=dab,
                prep=pr)


def compare(dev, ref, what=""):
    """device value(s) against V(s) -> the largest |device - value| / bound (0 / 0 = 0; anything / 0 = inf)"""
    if isinstance(ref, (list, tuple)):
        return max((compare(d, r, what) for d, r in zip(dev, ref)), default=0.0)
    d = np.abs(np.asarray(dev, np.float64).reshape(ref.shape) - ref.val)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(d == 0, 0.0, d / ref.err)
    return float(ratio.max()) if ratio.size else 0.0


GROUPS = ("attention", "spa_fusion", "interaction_mask", "stsgcn", "fusion_", "tcns", "output")


def group_of(key):
    for g in GROUPS:
        if g in key:
            return g
    raise KeyError(key)


def vacuous(grads, n):
    """the tensors of more than one element whose bound reaches half their largest entry: a bound below that cannot pass
    zeros, a flipped sign or a wrong scale at that entry.  (A one-element tensor, a PReLU slope's gradient, is a sum over the
    whole scene that can cancel; its bound is that of the sum, whatever is left of it.)"""
    return [k for k, g in grads.items() if "key.bias" not in k and g.val.size > 1 and g.err.max() >= 0.5 * np.abs(g.val).max()
            and not (n == 1 and "spatial_attention" in k)]   # a scene of ``n`` = 1: a softmax row of one entry has no gradient
