"""float64 numpy restatement of the training pass of csrc/et_gpgraph_train.inl (on csrc/et_sgcn_train.inl's GP = true
kernels), independent of torch: GP-Graph-SGCN's forward (tests/_gpgraph_np.py's, every kept value returned), the backward
pass to all parameters, and a running elementwise bound for what the fp32 kernels may differ by.  The bounds are the only
tolerances tests/test_gpu_gpgraph_train.py uses; they are derived here, not tuned.  Not a test module itself.

Built on tests/_sgcn_train_np.py: its :class:`V` (value and bound), :func:`ein`, :func:`gamma` (Higham's bound of a sum of
products in any order, the depth of a summation tree in place of the number of terms), its :class:`Decisions` and its
layer-local scheme -- every kept value is re-formed here from the DEVICE's own kept inputs of that step (exact fp32 numbers,
bound 0), compared within that one step's bound and replaced by the device's; a weight gradient is within the bound of its
own summation tree.  :func:`base_run` is that file's ``run`` for the two-channel base: the temporal attention reads the
position and the coefficient channel (six collapsed numbers per head, a (64, 2) embedding), the identities are eye(n) and
eye(T), the spatial mask of the intra-group pass is multiplied by the same-group matrix, a pass has n_m nodes, and the input
gradient of both channels is formed -- from the spatial attention as query and as key, the temporal attention, A_s x and A_t x.
:func:`run` is the wrapper around three such passes: distance, soft assignment, straight-through, pool, mix and their
backward steps 1-7 (include/eigentraj.h).

Hard decisions.  The masks' and PReLUs' as in tests/_sgcn_train_np.py (per pass).  The pair decisions d <= th make the group
index: with ``device`` the index is the device's, and a pair with |d - th| <= BAND_D th (tests/_gpgraph_np.py) is counted as
undecided; the test inputs have none.  The mix's PReLU reads the three kept pass outputs, exact numbers: no band.  The
distance's backward is 0 where the norm is 0 (the diagonal and coincident pedestrians: torch's norm backward, which
tests/test_gpgraph_train_cpu.py confirms on the twin); the norm is formed from the kept f, so 0 is decided exactly.

A weight gradient of the base is the sum over the three passes: the device adds the passes' per-workgroup partials in one
ascending chain, so the bound is the passes' bounds plus gamma(slots of all passes) x the sum of their terms' magnitudes; the
attention tensors follow from the summed collapsed gradients through the (fp64) prep backward."""
import numpy as np

from . import _gpgraph_np as GN
from . import _sgcn_np as SN
from . import _sgcn_train_np as TN
from ._sgcn_train_np import (U, V, add, const, conv, conv_bwd, div, ein, gamma, mul, neg, prelu_bwd, prelu_fwd, vexp,  # noqa: F401
                             vsum)

H, D, SWA = TN.H, TN.D, TN.SWA
BASE = "baseline_model."


def scale(x, c, roundings=1):
    """x * c for an exact constant c (a division by T, by a group size, by tau: one rounding)"""
    val = x.val * c
    return V(val, x.err * abs(c) + gamma(roundings) * np.abs(val))


def where(cond, a, b):
    return V(np.where(cond, a.val, b.val), np.where(cond, a.err, b.err))


def prep_t(sd):
    """the collapsed two-channel temporal attention: hdr[8 + 4 q + h] of sgcn_prep<true>, q = 0..5 -> dict, ``h`` [6] V (4,)"""
    p = SWA + "temporal_attention."
    f = lambda k: np.asarray(sd[p + k], np.float64)
    W, be, Wq, bq, Wk = f("embedding.weight"), f("embedding.bias"), f("query.weight"), f("query.bias"), f("key.weight")
    wp, wc = W[:, 0], W[:, 1]
    aq_p, aq_c, cq, ak_p, ak_c = Wq @ wp, Wq @ wc, Wq @ be + bq, Wk @ wp, Wk @ wc
    dot = lambda a, b: (a * b).reshape(H, D).sum(1) / 8.0
    hs = [dot(aq_p, ak_p), dot(aq_c, ak_p), dot(cq, ak_p), dot(aq_p, ak_c), dot(aq_c, ak_c), dot(cq, ak_c)]
    return dict(wp=wp, wc=wc, be=be, Wq=Wq, Wk=Wk, aq_p=aq_p, aq_c=aq_c, cq=cq, ak_p=ak_p, ak_c=ak_c,
                h=[V(x, U * np.abs(x)) for x in hs])


def prep_t_bwd(pr, dh, names):
    """d h_q (V (4,), q = 0..5) -> {name: V} of the six tensors of the temporal attention (fp64 on the device)"""
    rep = lambda x: V(np.repeat(x.val, D), np.repeat(x.err, D))
    d = [rep(x) for x in dh]
    c = lambda x: V(np.asarray(x, np.float64) / 8.0)
    k = lambda x: V(np.asarray(x, np.float64))
    daq_p = add(mul(d[0], c(pr["ak_p"])), mul(d[3], c(pr["ak_c"])))
    daq_c = add(mul(d[1], c(pr["ak_p"])), mul(d[4], c(pr["ak_c"])))
    dcq = add(mul(d[2], c(pr["ak_p"])), mul(d[5], c(pr["ak_c"])))
    dak_p = add(mul(d[0], c(pr["aq_p"])), mul(d[1], c(pr["aq_c"])), mul(d[2], c(pr["cq"])))
    dak_c = add(mul(d[3], c(pr["aq_p"])), mul(d[4], c(pr["aq_c"])), mul(d[5], c(pr["cq"])))
    dWq = add(ein("c,e->ce", daq_p, k(pr["wp"])), ein("c,e->ce", daq_c, k(pr["wc"])), ein("c,e->ce", dcq, k(pr["be"])))
    dWk = add(ein("c,e->ce", dak_p, k(pr["wp"])), ein("c,e->ce", dak_c, k(pr["wc"])))
    dwp = add(ein("ce,c->e", k(pr["Wq"]), daq_p), ein("ce,c->e", k(pr["Wk"]), dak_p))
    dwc = add(ein("ce,c->e", k(pr["Wq"]), daq_c), ein("ce,c->e", k(pr["Wk"]), dak_c))
    dbe = ein("ce,c->e", k(pr["Wq"]), dcq)
    dwe = V(np.stack([dwp.val, dwc.val], 1), np.stack([dwp.err, dwc.err], 1))
    return {names + "embedding.weight": dwe, names + "embedding.bias": dbe, names + "query.weight": dWq,
            names + "query.bias": dcq, names + "key.weight": dWk, names + "key.bias": V(np.zeros(64))}


def slots_of(T, n):
    """upper count of the per-workgroup partials of one virtual scene of n nodes, over all the base's kernels"""
    from eigentrajectory_amd import _lib as L
    cd = lambda a, b: -(-a // b)
    return cd(T * n * n, L.SGCN_BWD_ITEMS) + cd(n * T * T, L.SGCN_BWD_ITEMS) + cd(n, L.SGCN_BWD_CHUNK) + cd(8 * T * n, L.SGCN_BWD_ROWS) + 2


def base_run(sd, g, same, d_out, device=None, want_dx=True, propagate=False):
    """one pass of the two-channel base.  sd: the base's fp32 state dict (no prefix), g (2, T, n) = [position; coefficients]
    fp32, ``same`` the (n, n) same-group matrix or None, d_out (k, n, S) -> dict: ``out`` V (k, n, S), ``kept``, ``kept_ratio``,
    ``grads`` {name: V with ``tm``} of every tensor but the attentions', ``dab`` (d alpha, d beta) of the spatial and ``dh`` [6]
    of the temporal attention (V (4,) with ``tm``), ``dx`` V (2, T, n) (``want_dx``), ``decisions``.  ``device``: this pass's
    kept values (``ops.gpgraph_sgcn_train_views(...)["passes"][m]`` as numpy)."""
    dec = TN.Decisions()
    dv = (lambda k, j=None: None) if device is None else (lambda k, j=None: np.asarray(device[k] if j is None else device[k][j],
                                                                                       np.float64))
    P = lambda k: V(np.asarray(sd[k], np.float64))
    if not isinstance(g, V):
        g = V(np.asarray(g, np.float64))
    xp, x = g[0], g[1]
    E = lambda a, idx: V(a.val[idx], a.err[idx])
    xT, xpT = x.t(1, 0), xp.t(1, 0)
    T, N = x.shape
    na, nt = SN.n_layers(sd)
    ids = np.eye(N)[None, None]                                             # (1, 1, N, N)
    idt = np.eye(T)[None, None]                                             # (1, 1, T, T)
    kept, grads, kept_ratio = {"v": x, "vp": xp}, {}, {}

    def force(name, val, j=None, to_dev=lambda a: a, from_dev=lambda a: a):
        rec = V(to_dev(val.val), to_dev(val.err))
        if j is None:
            kept[name] = rec
        else:
            kept.setdefault(name, []).append(rec)
        if device is None:
            return val if propagate else V(val.val)
        d = dv(name, j)
        kept_ratio[name] = max(kept_ratio.get(name, 0.0), TN.compare(d, rec))
        return V(from_dev(d.reshape(rec.shape)))

    # ------------------------------------------------------------------------------------------------ forward
    pr_s, pr_t = TN.prep(sd, 0), prep_t(sd)
    hq = [h.reshape(1, H, 1) for h in pr_t["h"]]
    xe = V(x.val[:, None, :], x.err[:, None, :])
    ti_s = add(mul(xe, pr_s["alpha"].reshape(1, H, 1), roundings=0), pr_s["beta"].reshape(1, H, 1), roundings=1)   # (T,H,N)
    xrow = E(x, (slice(None), None, None, slice(None)))                                                  # (T,1,1,N)
    score_s = mul(V(ti_s.val[..., None], ti_s.err[..., None]), xrow)                                     # (T,H,N,N)
    dense_s = TN._softmax_rows(score_s, lambda r: force("rows_s", r))
    pn, cn = E(xpT, (slice(None), None, slice(None))), E(xT, (slice(None), None, slice(None)))           # (N, 1, T)
    fma2 = lambda p_, c_, h0, h1, h2: add(mul(p_, h0, roundings=0), add(mul(c_, h1, roundings=0), h2, roundings=1), roundings=1)
    ta, tb = fma2(pn, cn, hq[0], hq[1], hq[2]), fma2(pn, cn, hq[3], hq[4], hq[5])                        # (N, H, T)
    pu, cu = E(xpT, (slice(None), None, None, slice(None))), E(xT, (slice(None), None, None, slice(None)))   # (N, 1, 1, T)
    ex4 = lambda a: V(a.val[..., None], a.err[..., None])
    score_t = add(mul(pu, ex4(ta), roundings=0), mul(cu, ex4(tb)), roundings=1)                          # (N,H,T,T)
    dense_t = TN._softmax_rows(score_t, lambda r: force("rows_t", r))
    fw, fb, fa = P(SWA + "spa_fusion.conv.0.weight").reshape(T, T), P(SWA + "spa_fusion.conv.0.bias"), P(SWA + "spa_fusion.conv.1.weight")
    facc = ein("ut,thij->uhij", fw, dense_s, init=fb.reshape(T, 1, 1, 1))
    dev0 = None if device is None else (dv("stack_s", 0) - dense_s.val) > 0
    fpre, keep_f = prelu_fwd(facc, fa, dec, dev0)
    stack_s, stack_t = [force("stack_s", add(fpre, dense_s), 0)], [force("stack_t", dense_t, 0)]
    dense_t = stack_t[0]
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
    mk_s, keep_ms, sg_s = TN._mask(stack_s[-1], ids, dec, dv("stack_s", na))
    if same is not None:   # the intra-group pass: the mask, identity added, times the same-group matrix (0 / 1: exact)
        sm = np.asarray(same, np.float64)[None, None]
        mk_s = V(mk_s.val * sm, mk_s.err * sm)
    mk_t, keep_mt, sg_t = TN._mask(stack_t[-1], idt, dec, dv("stack_t", na))
    _, ex_s, em1_s, e_s, den_s = TN._zsm_fwd(dense_s, mk_s)
    _, ex_t, em1_t, e_t, den_t = TN._zsm_fwd(dense_t, mk_t)
    gw = [P(f"stsgcn.{nm}_sparse_gcn.{i}.embedding.weight") for nm in ("spatial_temporal", "temporal_spatial") for i in (0, 1)]
    ga = [P(f"stsgcn.{nm}_sparse_gcn.{i}.activation.weight") for nm in ("spatial_temporal", "temporal_spatial") for i in (0, 1)]
    A_t = force("at", div(e_t, den_t))
    acc_t = ein("nhtu,un->nht", A_t, x, extra=1)
    z2 = mul(V(acc_t.val[..., None], acc_t.err[..., None]), gw[2].reshape(1, 1, 1, D))
    f2, keep2 = prelu_fwd(z2, ga[2], dec, None if device is None else dv("f2") > 0)
    f2 = force("f2", f2)
    den3 = V(den_s.val[..., 0], den_s.err[..., 0])
    ax = div(ein("thij,tj->thi", e_s, x, extra=1), den3)
    z0 = mul(V(ax.val[..., None], ax.err[..., None]), gw[0].reshape(1, 1, 1, D))
    f1, keep0 = prelu_fwd(z0, ga[0], dec, None if device is None else dv("f1") > 0)
    f1 = force("f1", f1)
    accn = div(ein("thij,jhtd->thid", e_s, f2, extra=1), V(den_s.val, den_s.err))
    o3 = ein("dq,thiq->thid", gw[3], accn, extra=1)
    ts_thid, keep3 = prelu_fwd(o3, ga[3], dec, None if device is None else dv("ts").transpose(2, 1, 0, 3) > 0)
    ts = force("ts", ts_thid.t(2, 1, 0, 3))
    Gm = ein("nhtu,uhnd->nhtd", A_t, f1, extra=1)
    z1 = ein("dq,nhtq->nhtd", gw[1], Gm, extra=1)
    to_keep = lambda a: np.ascontiguousarray(a.transpose(0, 2, 1, 3)).reshape(N, T, H * D)
    from_keep = lambda a: a.reshape(N, T, H, D).transpose(0, 2, 1, 3)
    _, keep1 = prelu_fwd(z1, ga[1], dec, None if device is None else from_keep(dv("st_pre")) > 0)
    z1 = force("st_pre", z1, None, to_keep, from_keep)
    st, _ = prelu_fwd(z1, ga[1], TN.Decisions(), keep1)
    fus = P("fusion_.weight").reshape(H, H)
    rep = force("rep", add(ein("hg,ngtd->nhtd", fus, st, extra=1), ts), None, to_keep, from_keep)
    xs = [rep.t(0, 2, 1, 3)]
    keep_tc, z_tc = [], []
    flat = (lambda a: a.reshape(N, -1, H * D)), (lambda a: a.reshape(N, -1, H, D))
    for j in range(nt):
        z = conv(xs[j], P(f"tcns.{j}.0.weight"), P(f"tcns.{j}.0.bias"))
        _, kp = prelu_fwd(z, P(f"tcns.{j}.1.weight"), dec, None if device is None else flat[1](dv("tcn_pre", j)) > 0)
        z = force("tcn_pre", z, j, *flat)
        y, _ = prelu_fwd(z, P(f"tcns.{j}.1.weight"), TN.Decisions(), kp)
        if j:
            y = add(y, xs[j])
        xs.append(force("tcn_out", y, j, *flat)), z_tc.append(z), keep_tc.append(kp)
    ow, ob = P("output.weight"), P("output.bias")
    lin = ein("sq,nthq->nths", ow, xs[-1], init=ob)
    out = vsum(lin, 2, extra=0)
    out = force("out", V(0.25 * out.val, 0.25 * out.err).t(1, 0, 2))
    if d_out is None:
        return dict(out=out, kept=kept, kept_ratio=kept_ratio, decisions=dec.figures())
    # ------------------------------------------------------------------------------------------------ backward
    from eigentrajectory_amd import _lib as L
    cd = lambda a, b: -(-a // b)
    tree = lambda lane, slots: lane + 6 + 4 + slots
    k_ = xs[-1].shape[1]
    s_tail = L.SGCN_BWD_CHUNK + cd(N, L.SGCN_BWD_CHUNK)
    s_rows, s_rows2 = cd(4 * T * N, L.SGCN_BWD_ROWS), cd(8 * T * N, L.SGCN_BWD_ROWS)
    s_stack = {"spatial": cd(T * N * N, L.SGCN_BWD_ITEMS), "temporal": cd(N * T * T, L.SGCN_BWD_ITEMS)}
    s_fuse = cd(4 * N * N, L.SGCN_BWD_ITEMS)
    per_lane = cd(L.SGCN_BWD_ITEMS, 256)
    go = d_out if isinstance(d_out, V) else V(np.asarray(d_out, np.float64))
    gq = V(0.25 * go.val, 0.25 * go.err)
    grads["output.bias"] = vsum(go, (0, 1), depth=k_ + s_tail)
    xh = vsum(xs[-1], 2, extra=0)
    grads["output.weight"] = ein("tns,ntq->sq", gq, xh, extra=2 + H, depth=H * k_ + s_tail)
    gx = ein("tns,sq->ntq", gq, ow)
    gx = V(np.repeat(gx.val[:, :, None, :], H, 2), np.repeat(gx.err[:, :, None, :], H, 2))
    for j in range(nt - 1, -1, -1):
        a = P(f"tcns.{j}.1.weight")
        dz, da = prelu_bwd(gx, z_tc[j], a, keep_tc[j], depth=tree(cd(k_ * 64, 256), s_tail))
        grads[f"tcns.{j}.1.weight"] = da
        grads[f"tcns.{j}.0.bias"] = vsum(dz, (0, 2, 3), depth=64 + s_tail)
        gx, grads[f"tcns.{j}.0.weight"] = conv_bwd(dz, xs[j], P(f"tcns.{j}.0.weight"), init=gx if j else None, depth=64 + s_tail)
    drep = force("d_ts", gx.t(0, 2, 1, 3))
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
    if want_dx:
        dax = force("d_ax", dax)
    dzo, grads["stsgcn.temporal_spatial_sparse_gcn.1.activation.weight"] = prelu_bwd(drep.t(2, 1, 0, 3), o3, ga[3], keep3,
                                                                                         depth=tree(4 * D, s_rows))
    grads["stsgcn.temporal_spatial_sparse_gcn.1.embedding.weight"] = ein("thid,thiq->dq", dzo, accn, depth=L.SGCN_BWD_ROWS + s_rows)
    daccn = force("d_accn", ein("dq,thid->thiq", gw[3], dzo))
    dA_s = ein("thiq,jhtq->thij", daccn, f2, init=mul(V(dax.val[..., None], dax.err[..., None]), xrow))
    A_s = div(e_s, den_s)
    df2 = force("d_f2", ein("thij,thiq->jhtq", A_s, daccn))
    dir_s, dl_s = TN._zsm_bwd(dA_s, e_s, den_s, ex_s, em1_s, dense_s, mk_s, keep_ms, sg_s)
    dir_s, dl_s = force("dir_s", dir_s), force("g_s", dl_s, na)
    # tadj
    dz2, grads["stsgcn.temporal_spatial_sparse_gcn.0.activation.weight"] = prelu_bwd(df2, z2, ga[2], keep2,
                                                                                         depth=tree(4 * D, s_rows))
    grads["stsgcn.temporal_spatial_sparse_gcn.0.embedding.weight"] = ein("nhtd,nht->d", dz2, acc_t, depth=tree(4, s_rows)).reshape(D, 1)
    dacc = ein("nhtd,d->nht", dz2, gw[2].reshape(D))
    if want_dx:
        dacc = force("d_acc_t", dacc)
    dA_t = add(mul(V(dacc.val[..., None], dacc.err[..., None]), cu, roundings=0), dat, roundings=1)
    dir_t, dl_t = TN._zsm_bwd(dA_t, e_t, den_t, ex_t, em1_t, dense_t, mk_t, keep_mt, sg_t)
    dir_t, dl_t = force("dir_t", dir_t), force("g_t", dl_t, na)
    for name, stack, zs, keeps, gcur in (("spatial", stack_s, z_as, keep_as, dl_s), ("temporal", stack_t, z_at, keep_at, dl_t)):
        for j in range(na - 1, -1, -1):
            p = f"{SWA}interaction_mask.{name}_asymmetric_convolutions.{j}."
            dp = tree(per_lane, s_stack[name])
            dz, grads[p + "activation.weight"] = prelu_bwd(gcur, zs[j], P(p + "activation.weight"), keeps[j], depth=dp + 3 * per_lane)
            grads[p + "conv2.bias"] = vsum(dz, (0, 2, 3), depth=dp)
            d2, grads[p + "conv2.weight"] = conv_bwd(dz, stack[j], P(p + "conv2.weight"), depth=dp)
            d1, grads[p + "conv1.weight"] = conv_bwd(dz, stack[j], P(p + "conv1.weight"), depth=dp)
            gcur = force("g_s" if name == "spatial" else "g_t", add(gcur, d2, d1, roundings=24), j)
        if name == "spatial":
            g_s0 = gcur
        else:
            g_t0 = gcur
    dfacc, grads[SWA + "spa_fusion.conv.1.weight"] = prelu_bwd(g_s0, facc, fa, keep_f, depth=tree(cd(L.SGCN_BWD_ITEMS, 128) * T, s_fuse))
    grads[SWA + "spa_fusion.conv.0.bias"] = vsum(dfacc, (1, 2, 3), depth=L.SGCN_BWD_ITEMS + s_fuse)
    grads[SWA + "spa_fusion.conv.0.weight"] = ein("uhij,thij->ut", dfacc, dense_s, depth=L.SGCN_BWD_ITEMS + s_fuse).reshape(T, T, 1, 1)
    dd_s = force("dd_s", add(ein("ut,uhij->thij", fw, dfacc, init=g_s0), dir_s))
    dd_t = add(g_t0, dir_t)
    # softmax rows: d score = dense (d dense - sum dense d dense)
    dr = tree(4, s_rows2)
    s_s = vsum(mul(dense_s, dd_s, roundings=0), -1, keepdims=True, extra=1)
    dsc_s = mul(dense_s, add(dd_s, neg(s_s)))                                                            # (T,H,N,N)
    dti_s = vsum(mul(dsc_s, xrow, roundings=0), -1, extra=1)                                             # (T,H,N)
    s_t = vsum(mul(dense_t, dd_t, roundings=0), -1, keepdims=True, extra=1)
    dsc_t = mul(dense_t, add(dd_t, neg(s_t), roundings=2))                                               # (N,H,T,T)
    da_t = vsum(mul(dsc_t, pu, roundings=0), -1, extra=1)                                                # (N,H,T)
    db_t = vsum(mul(dsc_t, cu, roundings=0), -1, extra=1)
    if want_dx:   # the row records the input gradient reads
        rec = force("srec", V(np.stack([s_s.val[..., 0], dti_s.val], -1), np.stack([s_s.err[..., 0], dti_s.err], -1)))
        s_s, dti_s = V(rec.val[..., :1], rec.err[..., :1]), V(rec.val[..., 1], rec.err[..., 1])
        rec = force("trec", V(np.stack([s_t.val[..., 0], da_t.val, db_t.val], -1), np.stack([s_t.err[..., 0], da_t.err, db_t.err], -1)))
        s_t, da_t, db_t = V(rec.val[..., :1], rec.err[..., :1]), V(rec.val[..., 1], rec.err[..., 1]), V(rec.val[..., 2], rec.err[..., 2])
    xcol = V(np.broadcast_to(x.val[:, None, :], dti_s.shape), np.broadcast_to(x.err[:, None, :], dti_s.shape))
    dalpha = vsum(mul(dti_s, xcol, roundings=0), (0, 2), extra=1, depth=dr)
    dbeta = vsum(dti_s, (0, 2), depth=dr)
    pt_ = V(np.broadcast_to(pn.val, da_t.shape), np.broadcast_to(pn.err, da_t.shape))
    ct_ = V(np.broadcast_to(cn.val, da_t.shape), np.broadcast_to(cn.err, da_t.shape))
    dh = [vsum(mul(da_t, pt_, roundings=0), (0, 2), extra=1, depth=dr), vsum(mul(da_t, ct_, roundings=0), (0, 2), extra=1, depth=dr),
          vsum(da_t, (0, 2), depth=dr),
          vsum(mul(db_t, pt_, roundings=0), (0, 2), extra=1, depth=dr), vsum(mul(db_t, ct_, roundings=0), (0, 2), extra=1, depth=dr),
          vsum(db_t, (0, 2), depth=dr)]
    res = dict(out=out, kept=kept, kept_ratio=kept_ratio, decisions=dec.figures(), dab=(dalpha, dbeta), dh=dh)
    if want_dx:
        # channel 1 (coefficients) and channel 0 (position), item (t, i): csrc/et_gpgraph_train.inl gp_dx
        dsc_s = mul(dense_s, add(dd_s, neg(s_s)))                    # from the kept row sums, as the kernel forms it
        dsc_t = mul(dense_t, add(dd_t, neg(s_t), roundings=2))
        dx_as = force("dx_as", ein("thij,thi->jht", A_s, dax, extra=1))                                  # (N,H,T)
        al, h_ = pr_s["alpha"], pr_t["h"]
        parts_c = [ein("thi,h->ti", dti_s, al), ein("thji,thj->ti", dsc_s, ti_s), vsum(dx_as, 1).t(1, 0),
                   ein("iht,h->ti", da_t, h_[1]), ein("iht,h->ti", db_t, h_[4]), ein("ihut,ihu->ti", dsc_t, tb),
                   ein("ihut,ihu->ti", A_t, dacc)]
        parts_p = [ein("iht,h->ti", da_t, h_[0]), ein("iht,h->ti", db_t, h_[3]), ein("ihut,ihu->ti", dsc_t, ta)]
        dxc, dxp = add(*parts_c, roundings=8 * H), add(*parts_p, roundings=4 * H)
        res["dx"] = force("dx", V(np.stack([dxp.val, dxc.val]), np.stack([dxp.err, dxc.err])))
    for k, gk in grads.items():
        if gk.tm is None:
            gk.tm = gk.mag
        tm = np.asarray(gk.tm)
        gk.err = gk.err + U * np.abs(gk.val)
        shape = np.asarray(sd[k]).shape
        if gk.shape != shape:
            tmr = tm.reshape(shape) if tm.size == int(np.prod(shape)) else np.broadcast_to(tm.max(), shape)
            grads[k] = V(gk.val.reshape(shape), np.ascontiguousarray(gk.err).reshape(shape), tmr)
    res["grads"] = grads
    res["prep"] = (pr_s, pr_t)
    return res


def _sqrt(ss):
    val = np.sqrt(ss.val)
    lo = np.sqrt(np.maximum(ss.val - ss.err, 0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.where(ss.val == 0, np.sqrt(ss.err), np.where(lo > 0, ss.err / (val + lo), np.sqrt(ss.err)))
    return V(val, err + U * val)


def _norms(f):
    """f V (8, T, n) -> (diff V (8, T, n, n), norm V (T, n, n)) as the kernels form them: one fma chain over the channels"""
    d = f.val[..., :, None] - f.val[..., None, :]   # of two fp32 numbers (the kept f: exact): one rounding
    diff = V(d, U * np.abs(d) + np.where(d == 0, 0.0, f.err[..., :, None] + f.err[..., None, :]))
    return diff, _sqrt(ein("ctij,ctij->tij", diff, diff, extra=0))


def run(sd, v_abs, v_rel, d_out, device=None, tau=0.1, propagate=False):
    """sd: the whole GPGraph's fp32 state dict, v_abs (T, n), v_rel (2, T, n) fp32, d_out (S, k, n) -> dict: ``out`` V (S, k, n),
    ``indices``, ``kept_ratio`` {step: largest error / bound}, ``grads`` {state_dict name: V}, ``decisions`` [3] per pass,
    ``pairs`` dict(entries, undecided, near: within 3 tau of th), ``passes`` (the three :func:`base_run` results).
    ``device``: ``ops.gpgraph_sgcn_train_views`` of the device run, as numpy (its ``group_index`` is then the index).
    ``propagate`` (without ``device``): no bound is reset, every value carries the worst case of the whole chain before it,
    as in tests/_sgcn_train_np.run -- a bound on the distance to the EXACT gradient, which is what a comparison with another
    implementation's float64 gradients needs.  Carried through three passes and back through the input gradient it is very
    loose (it exceeds many of the gradients themselves, and where a worst-case denominator reaches zero it is infinite: such
    an entry says nothing and is reported as infinite, never as NaN); ``loose`` in the result is bound / largest entry per
    tensor, so that a reader sees what a comparison under it is worth."""
    from eigentrajectory_amd import _lib as L
    base, rest = GN.split_state(sd)
    P = lambda k: V(np.asarray(sd[k], np.float64))
    va = V(np.asarray(v_abs, np.float64))
    vr = V(np.asarray(v_rel, np.float64))
    T, n = va.shape
    kept_ratio = {}
    dv = (lambda k: None) if device is None else (lambda k: np.asarray(device[k], np.float64))

    def force(name, val, dev=None):
        if device is None:
            return val if propagate else V(val.val)
        d = dv(name) if dev is None else np.asarray(dev, np.float64)
        kept_ratio[name] = max(kept_ratio.get(name, 0.0), TN.compare(d, val))
        return V(d.reshape(val.shape))

    # ------------------------------------------------------------------------------------------------ forward
    gwt, gb = P("group_gen.group_cnn.0.weight").reshape(8, 3), P("group_gen.group_cnn.0.bias")
    xpad = np.pad(va.val, ((1, 1), (0, 0)))
    taps = V(np.stack([xpad[d:d + T] for d in range(3)]))                                                # (3, T, n)
    f = force("f", ein("cd,dti->cti", gwt, taps, init=gb.reshape(8, 1, 1), extra=1))
    diff, nrm = _norms(f)
    dist = force("dist", scale(vsum(nrm, 0, extra=0), 1.0 / T))
    th = float(np.asarray(sd["group_gen.th"], np.float32).reshape(-1)[0])
    low = np.tril(np.ones((n, n), bool), -1)
    pairs = dict(entries=int(low.sum()), undecided=int((np.abs(dist.val - th)[low] <= GN.BAND_D * th).sum()),
                 near=int((np.abs(dist.val - th)[low] <= 3 * tau).sum()))
    own_idx = GN.compact(GN.merge_literal(dist.val <= th))
    idx = own_idx if device is None else np.asarray(device["group_index"]).astype(np.int64)
    G = int(idx.max()) + 1
    cnt = np.bincount(idx, minlength=G).astype(np.float64)
    onehot = (idx[:, None] == np.arange(G)[None]).astype(np.float64)                                    # (n, G)
    dmt = V(dist.val - th, dist.err + U * np.abs(dist.val - th))
    u = scale(neg(dmt), 1.0 / tau)
    sig = force("sig", TN._sigmoid(u))
    cs = force("colsum", vsum(sig, 0, extra=0))
    sn = force("sn", div(sig, V(cs.val[None], cs.err[None])))
    soft = ein("cti,ij->ctj", vr, sn, extra=0)
    v2 = add(add(vr, neg(soft)), soft)
    v2 = force("v2", v2, None if device is None else np.stack([device["passes"][2]["vp"], device["passes"][2]["v"]]))
    pool_sum = V(np.einsum("cti,ig->ctg", v2.val, onehot), gamma(int(cnt.max())) * np.einsum("cti,ig->ctg", v2.mag, onehot)
                 + np.einsum("cti,ig->ctg", v2.err, onehot))
    pooled = div(pool_sum, V(cnt[None, None]))
    pooled = force("pooled", pooled, None if device is None else np.stack([device["passes"][1]["vp"], device["passes"][1]["v"]]))
    same = idx[:, None] == idx[None, :]
    S, k = np.asarray(d_out).shape[:2]
    Sk = S * k
    dp = (lambda m: None) if device is None else (lambda m: device["passes"][m])
    inputs = [vr, pooled, v2] if propagate else [vr.val, pooled.val, v2.val]
    sames = [None, None, same]
    if device is None:
        o = [base_run(base, inputs[m], sames[m], None, propagate=propagate)["out"] for m in range(3)]    # (k, n_m, S)
    else:   # the kept pass outputs (each is compared within its pass, below)
        o = [V(np.asarray(device["passes"][m]["out"], np.float64)) for m in range(3)]
    o[1] = V(o[1].val[:, idx], o[1].err[:, idx])                                                         # unpool by gather
    z = V(np.concatenate([x.val.transpose(2, 0, 1).reshape(Sk, n) for x in o]),
          np.concatenate([x.err.transpose(2, 0, 1).reshape(Sk, n) for x in o]))                          # (3 S k, n)
    a, W, b = P("group_mix.st_gcns_mix.0.weight"), P("group_mix.st_gcns_mix.1.weight").reshape(Sk, 3 * Sk), P("group_mix.st_gcns_mix.1.bias")
    pos = z.val > 0
    act = where(pos, z, mul(a, z))
    y = ein("oq,qi->oi", W, act, init=b.reshape(Sk, 1), extra=1)
    zz = [V(z.val[m * Sk:(m + 1) * Sk], z.err[m * Sk:(m + 1) * Sk]) for m in range(3)]
    mean3 = scale(add(add(zz[0], zz[1]), zz[2]), 1.0 / 3.0)
    out = add(mean3, y).reshape(S, k, n)
    if device is not None and "out" in device:
        kept_ratio["out"] = TN.compare(device["out"], out)
    # ------------------------------------------------------------------------------------------------ backward
    cd = lambda a_, b_: -(-a_ // b_)
    n_mix = cd(n, L.GPGRAPH_BWD_ROWS)
    d_rows = min(n, L.GPGRAPH_BWD_ROWS) + n_mix
    g = V(np.asarray(d_out, np.float64).reshape(Sk, n))
    grads = {}
    grads["group_mix.st_gcns_mix.1.bias"] = vsum(g, 1, depth=d_rows)
    grads["group_mix.st_gcns_mix.1.weight"] = ein("oi,qi->oq", g, act, depth=d_rows).reshape(Sk, 3 * Sk, 1, 1)
    wtg = ein("oq,oi->qi", W, g, extra=0)
    wz = mul(wtg, z)
    grads["group_mix.st_gcns_mix.0.weight"] = vsum(where(pos, const(np.zeros_like(z.val)), wz), (0, 1),
                                                    depth=cd(3 * Sk, 128) + 6 + 2 + d_rows).reshape(1)
    g3 = scale(g, 1.0 / 3.0)
    dz = add(V(np.tile(g3.val, (3, 1)), np.tile(g3.err, (3, 1))), where(pos, wtg, mul(a, wtg)))
    to_kns = lambda x: V(x.val.reshape(S, k, n).transpose(1, 2, 0), x.err.reshape(S, k, n).transpose(1, 2, 0))
    d_o = []
    for m in range(3):
        piece = to_kns(V(dz.val[m * Sk:(m + 1) * Sk], dz.err[m * Sk:(m + 1) * Sk]))
        d_o.append(force(f"d_o{m}", piece, None if device is None else device["d_o"][m]))
    up = V(np.einsum("kns,ng->kgs", d_o[1].val, onehot), gamma(int(cnt.max())) * np.einsum("kns,ng->kgs", d_o[1].mag, onehot)
           + np.einsum("kns,ng->kgs", d_o[1].err, onehot))
    up = force("d_pooled_out", up, None if device is None else device["passes"][1]["d_out"])
    if device is not None:   # passes 0 and 2: copies
        for m in (0, 2):
            assert np.array_equal(np.asarray(device["passes"][m]["d_out"]), np.asarray(device["d_o"][m])), m
    ups = [d_o[0], up, d_o[2]] if propagate else [d_o[0].val, up.val, d_o[2].val]
    R = [base_run(base, inputs[m], sames[m], ups[m], device=dp(m), want_dx=m > 0, propagate=propagate) for m in range(3)]
    for m in range(3):
        for key, r in R[m]["kept_ratio"].items():
            kept_ratio[f"pass{m}.{key}"] = max(kept_ratio.get(f"pass{m}.{key}", 0.0), r)
    # the base's gradients: the three passes' partials in one ascending chain
    n_slots = sum(slots_of(T, m_) for m_ in (n, G, n)) + 3
    for key in R[0]["grads"]:
        val = sum(R[m]["grads"][key].val for m in range(3))
        err = sum(R[m]["grads"][key].err for m in range(3))
        tm = sum(np.asarray(R[m]["grads"][key].tm) + R[m]["grads"][key].err for m in range(3))
        grads[BASE + key] = V(val, err + gamma(n_slots) * tm + U * np.abs(val), tm=tm)
    comb = lambda vs: V(sum(x.val for x in vs), sum(x.err for x in vs) + gamma(n_slots) * sum(np.asarray(x.tm) + x.err for x in vs))
    dalpha, dbeta = comb([R[m]["dab"][0] for m in range(3)]), comb([R[m]["dab"][1] for m in range(3)])
    dh = [comb([R[m]["dh"][q] for m in range(3)]) for q in range(6)]
    pr_s, pr_t = R[0]["prep"]
    att = TN.prep_bwd(pr_s, dalpha, dbeta, SWA + "spatial_attention.")
    att.update(prep_t_bwd(pr_t, dh, SWA + "temporal_attention."))
    for key, gk in att.items():
        shape = np.asarray(base[key]).shape
        grads[BASE + key] = V(gk.val.reshape(shape), (gk.err + U * np.abs(gk.val)).reshape(shape))
    # pool and straight-through
    dx1, dx2 = R[1]["dx"], R[2]["dx"]                                                                    # (2, T, G), (2, T, n)
    dvp = force("d_vp", add(dx2, div(V(dx1.val[:, :, idx], dx1.err[:, :, idx]), V(cnt[idx][None, None]))))
    dP = force("d_P", ein("cti,ctj->ij", vr, dvp, extra=0))
    cols = ein("ij,ij->j", sn, dP, extra=0)
    dsig = force("d_sig", div(add(dP, neg(V(cols.val[None], cols.err[None]))), V(cs.val[None], cs.err[None])))
    one_m = V(1.0 - sig.val, sig.err + U * np.abs(1.0 - sig.val))
    du = mul(dsig, mul(sig, one_m))
    dd = force("d_d", scale(neg(du), 1.0 / tau))
    lane = cd(n * n, 256)
    grads["group_gen.th"] = vsum(scale(du, 1.0 / tau), (0, 1), depth=lane + 6 + 4).reshape(1)
    # the learned distance
    wsum = scale(add(dd, dd.t(1, 0)), 1.0 / T)
    nz = nrm.val > 0
    wq = div(V(np.broadcast_to(wsum.val[None], nrm.shape), np.broadcast_to(wsum.err[None], nrm.shape)),
             V(np.where(nz, nrm.val, 1.0), np.where(nz, nrm.err, 0.0)))
    wq = V(np.where(nz, wq.val, 0.0), np.where(nz, wq.err, 0.0))
    df_own = ein("tij,ctij->cti", wq, diff, extra=0)
    df = force("d_f", df_own)
    lane = cd(T * n, 256)
    grads["group_gen.group_cnn.0.weight"] = ein("cti,dti->cd", df, taps, depth=lane + 6 + 4).reshape(8, 1, 3, 1)
    grads["group_gen.group_cnn.0.bias"] = vsum(df, (1, 2), depth=lane + 6 + 4)
    for key in ("group_gen.th", "group_gen.group_cnn.0.weight", "group_gen.group_cnn.0.bias", "group_mix.st_gcns_mix.0.weight",
                "group_mix.st_gcns_mix.1.weight", "group_mix.st_gcns_mix.1.bias"):
        grads[key].err = grads[key].err + U * np.abs(grads[key].val)
    if propagate:   # an overflowed worst case (a denominator whose bound reaches zero) says nothing: infinite, not NaN
        for gk in grads.values():
            gk.err = np.where(np.isfinite(gk.err), gk.err, np.inf)
    loose = {k_: float(np.max(g_.err) / max(float(np.abs(g_.val).max()), 1e-300)) for k_, g_ in grads.items() if k_ in sd}
    # group_cnn's bias: the exact sum of the exact d f is 0 (w is symmetric, f_i - f_j antisymmetric), so the kernel's value lies
    # within the bound of its own sum plus the sum of d f's step bounds around 0
    bias_zero_bound = grads["group_gen.group_cnn.0.bias"].err + df_own.err.sum(axis=(1, 2)) + 1e-12 * df_own.mag.sum(axis=(1, 2))
    return dict(bias_zero_bound=bias_zero_bound, loose=loose, out=out, indices=idx, own_indices=own_idx, n_groups=G, kept_ratio=kept_ratio, grads={k_: grads[k_] for k_ in sd},
                decisions=[R[m]["decisions"] for m in range(3)], pairs=pairs, passes=R, dist=dist.val, th=th)


GROUPS = TN.GROUPS + ("group_gen", "group_mix")


def group_of(key):
    for g in ("group_gen", "group_mix"):
        if key.startswith(g):
            return g
    return TN.group_of(key)


def vacuous(grads, n, n_groups):
    """the multi-element tensors whose bound reaches half their largest entry (tests/_sgcn_train_np.vacuous).  With one
    pedestrian P = [[1]] and every gradient of group_gen is an exact zero; a softmax row of one entry (n = 1; the pooled pass
    when there is one group) has no gradient.  group_cnn's BIAS is left out for every n: the distance reads f_i - f_j, in which
    the bias cancels, so its exact gradient is zero (sum_i d f_i = 0: every pair's two terms are opposite) and what the device,
    autograd and this file give is rounding noise around it -- the bound of that sum is all there is to compare with."""
    out = []
    for k, g in grads.items():
        if "key.bias" in k or g.val.size <= 1 or k == "group_gen.group_cnn.0.bias":
            continue
        if n == 1 and ("spatial_attention" in k or k.startswith("group_gen")):
            continue
        if g.err.max() >= 0.5 * np.abs(g.val).max():
            out.append(k)
    return out
