"""float64 numpy restatement of the PECNet half of csrc/et_mlp_train.hip, independent of torch: the forward of ``predict``
(six chains, ``pools`` rounds of non-local social pooling with the same theta / phi / g weights) with every kept value, its
backward pass, and a running elementwise error bound for what the fp32 kernels may differ by.  The chains, their ``_dot``
inequality, U and gamma are tests/_mlp_train_np.py's (imported, not copied); this file adds the pooling step.

One round, feat (N, F) -> out (N, F), n = N columns per row:
    f = theta phi^T;  e_j = exp(f_j - max_k f_k);  s = e / sum e;  w = s * mask;  l1 = sum |w|;  den = max(l1, EPS);
    p = w / den;  out = p g + feat
backward from G, the gradient at out (include/eigentraj.h, "PECNet predictor, training"):
    dp = G g^T;  r1_i = sum_k dp_ik p_ik;  dw = (dp - sign(w) r1) / den where l1 > EPS, else dp / EPS;  ds = dw * mask (exactly
    0 under a zero of the mask);  r2_i = sum_k ds_ik s_ik;  df = s (ds - r2);  d theta = df phi;  d phi = df^T theta;
    d g = p^T G;  the gradient at feat = ((G + theta's input gradient) + phi's) + g's, in this order.
A dW / db of theta / phi / g is ONE dot product over the rows of all rounds, round 0's first (``_dot`` over pools N rows);
``round_terms`` also gives each round's own product, whose sum is the same number in exact arithmetic.

The bound through the pooling, to first order in the operands' bounds (products of two bounds are kept where they come for
free), every fp32 operation adding U times the magnitude of its result:
  * the logits: ``_dot`` over the D columns of theta and phi;
  * the softmax is invariant under a common shift of a row's logits, so the kernel's own row maximum may stand for the
    exact one: x^_j = fl(f^_j - m^) differs from f_j - m^ by at most ef_j + U |x^_j|, and expf(x^_j) from exp(f_j - m^) by
    the relative amount expm1(that) + EXPF_REL.  EXPF_REL = 3 ulp = 3 * 2^-23: the OpenCL C specification's bound for the
    single-precision exp (section "Relative Error as ULPs": exp <= 3 ulp), which the ROCm device library's expf is written
    to (the HIP math API table documents 1 ulp for expf; the larger figure is taken).  A result below the smallest normal
    number may be flushed: TINY = 2^-126 absolute;
  * z = sum e^: a sum of n terms in any order, gamma(n); s = e^ / z^: the two relative bounds and the division's rounding;
  * w = s mask, l1 = sum |w| (gamma(n), any order: the kernel sums lane-strided, then a butterfly), den, p = w / den:
    |w^ / d^ - w / d| <= (ew + |p| eden) / (den - eden), plus the division's rounding.  EPS is the kernel's constant, the
    float32 nearest to 1e-12.  A row whose l1 is within its bound of EPS, or a w within its bound of 0 where the mask is not
    0 (an exp the kernel may have flushed), makes the branch / the sign ambiguous: ``unsure`` marks the row, its p gets the
    bound 2 (p and p^ lie in [-1, 1]; likewise s and s^ in [0, 1]: no bound exceeds these) and its dw the bound BIG = 1e30,
    "nothing is known".  The bound never fails for want of precision; it turns vacuous, which the tests that use it report;
  * out = p g + feat: ``_dot`` over the n rows of g, one more addition;
  * backward: dp ``_dot`` over F; r1, r2 row dot products over n (gamma(n + 1), any order); the subtractions, the divisions
    and the products one rounding each on top of their operands' bounds; d theta, d phi, d g ``_dot`` over n; the sum of four
    terms at the features three additions.
Behind the 16-fold scaled last layers of theta and phi of the test configurations the running bound grows fast: 3e-6 of the
features' scale before the first round, 7e-3 after it, past the values themselves after the second (the worst case of every
|W| sum, of a 1 % logit error under exp; an fp32 evaluation is within 1e-7).  :func:`pool_stage` restarts it at a round's kept
inputs.
The ReLU masks are an ARGUMENT as in tests/_mlp_train_np.py: {chain: [mask of a_1 .. a_{L-1}]}, for theta / phi / g with the
rounds stacked along the rows (pools N, width), as `saved` holds them.
"""
import numpy as np

from . import _mlp_train_np as TN
from ._mlp_train_np import U, _dot, gamma

CHAINS = ("encoder_past", "encoder_dest", "non_local_theta", "non_local_phi", "non_local_g", "predictor")
POOLED = ("non_local_theta", "non_local_phi", "non_local_g")
EPS = float(np.float32(1e-12))
EXPF_REL = 3 * 2.0 ** -23
TINY = 2.0 ** -126
BIG = 1e30


def _rowdot(x, ex, y, ey):
    """sum_k x_ik y_ik per row, n terms in any order -> (N, 1) value and bound"""
    n = x.shape[1]
    ax, ay = np.abs(x), np.abs(y)
    val = (x * y).sum(axis=1, keepdims=True)
    err = (gamma(n + 1) * ((ax + ex) * (ay + ey)).sum(axis=1, keepdims=True) + (ex * (ay + ey)).sum(axis=1, keepdims=True)
           + (ax * ey).sum(axis=1, keepdims=True))
    return val, err


def _quot(a, ea, b, eb):
    """a / b with b > eb >= 0, one rounding"""
    q = a / b
    e = (ea + np.abs(q) * eb) / (b - eb)
    return q, e + U * (np.abs(q) + e) + TINY


def pool_forward(theta, eth, phi, eph, g, eg, feat, efeat, mask):
    """one round -> dict of every value of the docstring with its bound (``x`` / ``ex``)"""
    n = theta.shape[0]
    mk = np.ones((n, n)) if mask is None else np.asarray(mask, np.float64)
    f, ef = _dot(theta, eth, phi.T, eph.T)
    x = f - f.max(axis=1, keepdims=True)
    dx = np.minimum(ef + U * (np.abs(x) + ef + ef.max(axis=1, keepdims=True)), 50.0)
    e = np.exp(x)
    rel_e = np.expm1(dx) + EXPF_REL
    z = e.sum(axis=1, keepdims=True)
    rel_z = (gamma(n) * (e * (1 + rel_e)).sum(axis=1, keepdims=True) + (e * rel_e).sum(axis=1, keepdims=True)) / z
    s = e / z
    with np.errstate(divide="ignore", invalid="ignore"):
        es = np.where(rel_z < 0.5, s * ((1 + rel_e) * (1 + U) / (1 - rel_z) - 1), 1.0)
    es = np.minimum(es, 1.0) + U + TINY  # s and the kernel's s^ both lie in [0, 1 + U]
    w = s * mk
    ew = es * np.abs(mk) * (1 + U) + U * np.abs(w)
    l1 = np.abs(w).sum(axis=1, keepdims=True)
    el1 = gamma(n) * (np.abs(w) + ew).sum(axis=1, keepdims=True) + ew.sum(axis=1, keepdims=True)
    clamped = ~(l1 > EPS)
    # the kernel may take the other branch of the clamp, or see a weight of 0 (its exp flushed) where w is not
    unsure = ((l1 != 0) & (np.abs(l1 - EPS) <= el1)) | ((mk != 0) & (x - dx < -85.0)).any(axis=1, keepdims=True)
    den, eden = np.where(clamped, EPS, l1), np.where(clamped, 0.0, el1)
    with np.errstate(divide="ignore", invalid="ignore"):
        p, ep = _quot(w, ew, den, np.minimum(eden, den))
    ep = np.where(unsure | ~np.isfinite(ep), 2.0, np.minimum(ep, 2.0))  # p and the kernel's p^ both lie in [-1, 1]
    ep = np.where(mk == 0, 0.0, ep)  # 0 / den is 0 exactly
    val, e_val = _dot(p, ep, g, eg)
    out = val + feat
    eout = e_val + efeat
    eout = eout + U * (np.abs(out) + eout)
    return dict(f=f, ef=ef, s=s, es=es, w=w, ew=ew, l1=l1, den=den, eden=eden, clamped=clamped, unsure=unsure, p=p, ep=ep, mask=mk,
                out=out, eout=eout)


def forward(sd, past, dest, pos, mask, pools):
    """-> dict: ``out`` / ``out_err``; ``acts`` / ``acts_err`` / ``z`` / ``z_err`` per chain as tests/_mlp_train_np.py (for
    theta / phi / g a LIST over the rounds of those lists); ``feat`` / ``feat_err``: the features entering round 0 ..
    pools-1 and the predictor; ``rounds``: :func:`pool_forward`'s dict per round"""
    past, dest, pos = (np.asarray(a, np.float64) for a in (past, dest, pos))
    r = {"acts": {}, "acts_err": {}, "z": {}, "z_err": {}, "rounds": []}

    def run(chain, a0, e0):
        return TN._chain_forward(sd, chain, a0, e0)
    for chain, a0 in (("encoder_past", past), ("encoder_dest", dest)):
        r["acts"][chain], r["acts_err"][chain], r["z"][chain], r["z_err"][chain] = run(chain, a0, np.zeros_like(a0))
    feat = np.concatenate([r["z"]["encoder_past"][-1], r["z"]["encoder_dest"][-1], pos], axis=1)
    efeat = np.concatenate([r["z_err"]["encoder_past"][-1], r["z_err"]["encoder_dest"][-1], np.zeros_like(pos)], axis=1)
    r["feat"], r["feat_err"] = [feat], [efeat]
    for c in POOLED:
        r["acts"][c], r["acts_err"][c], r["z"][c], r["z_err"][c] = [], [], [], []
    for _ in range(pools):
        for c in POOLED:
            a, ea, z, ez = run(c, feat, efeat)
            r["acts"][c].append(a), r["acts_err"][c].append(ea), r["z"][c].append(z), r["z_err"][c].append(ez)
        zs = [(r["z"][c][-1][-1], r["z_err"][c][-1][-1]) for c in POOLED]
        rd = pool_forward(*zs[0], *zs[1], *zs[2], feat, efeat, mask)
        r["rounds"].append(rd)
        feat, efeat = rd["out"], rd["eout"]
        r["feat"].append(feat), r["feat_err"].append(efeat)
    c = "predictor"
    r["acts"][c], r["acts_err"][c], r["z"][c], r["z_err"][c] = run(c, feat, efeat)
    r["out"], r["out_err"] = r["z"][c][-1], r["z_err"][c][-1]
    return r


def pool_backward(rd, theta, eth, phi, eph, g, eg, G, eG):
    """-> dict: d theta, d phi, d g (``dtheta`` / ``edtheta`` ...), ``df`` / ``edf``, ``dp``, ``ds``"""
    s, es, w, p, ep, mk, den, eden = (rd[k] for k in ("s", "es", "w", "p", "ep", "mask", "den", "eden"))
    dp, edp = _dot(G, eG, g.T, eg.T)
    r1, er1 = _rowdot(dp, edp, p, ep)
    sg = np.sign(w)
    t = dp - sg * r1
    et = edp + np.abs(sg) * er1
    et = et + U * (np.abs(t) + et)
    with np.errstate(divide="ignore", invalid="ignore"):
        dw_n, edw_n = _quot(t, et, den, np.minimum(eden, den))
    dw_c, edw_c = _quot(dp, edp, np.full_like(den, EPS), np.zeros_like(den))
    dw, edw = np.where(rd["clamped"], dw_c, dw_n), np.where(rd["clamped"], edw_c, edw_n)
    edw = np.where(rd["unsure"] | ~np.isfinite(edw), BIG, np.minimum(edw, BIG))  # nothing is known there
    ds = np.where(mk == 0, 0.0, dw * mk)
    eds = np.where(mk == 0, 0.0, edw * np.abs(mk) * (1 + U) + U * np.abs(ds))
    r2, er2 = _rowdot(ds, eds, s, es)
    t2 = ds - r2
    et2 = eds + er2
    et2 = et2 + U * (np.abs(t2) + et2)
    df = s * t2
    edf = es * (np.abs(t2) + et2) + np.abs(s) * et2
    edf = edf + U * (np.abs(df) + edf) + TINY
    dth, edth = _dot(df, edf, phi, eph)
    dph, edph = _dot(df.T, edf.T, theta, eth)
    dg, edg = _dot(p.T, ep.T, G, eG)
    return dict(dp=dp, edp=edp, ds=ds, eds=eds, df=df, edf=edf, dtheta=dth, edtheta=edth, dphi=dph, edphi=edph, dg=dg,
                edg=edg)


def pool_stage(theta, phi, g, feat, mask, G=None, eG=None):
    """one round on GIVEN float32 inputs (the values a forward under test kept), taken as exact -> :func:`pool_forward`'s
    dict and, with G, :func:`pool_backward`'s: the bound is then this step's own rounding only, a few ulp of its values --
    the check that stays sharp where the running bound has grown past the values.  ``eG``: the bound of a G that was itself
    restated (default: G is a kept value, exact)"""
    theta, phi, g, feat = (np.asarray(a, np.float64) for a in (theta, phi, g, feat))
    zero = np.zeros_like
    rd = pool_forward(theta, zero(theta), phi, zero(phi), g, zero(g), feat, zero(feat), mask)
    if G is None:
        return rd, None
    G = np.asarray(G, np.float64)
    return rd, pool_backward(rd, theta, zero(theta), phi, zero(phi), g, zero(g), G, zero(G) if eG is None else eG)


def backward(sd, acts_mask, past, dest, pos, mask, pools, g_out):
    """``acts_mask`` as the docstring says (the masks the forward under test produced) -> dict: ``grads`` / ``grads_err``
    keyed by parameter name plus ``past``, ``dest`` and ``pos``; ``gz`` / ``gz_err`` per chain [g_z(1) .. g_z(L)] (theta /
    phi / g: stacked over the rounds); ``gfeat`` / ``gfeat_err``: the gradient at the features entering round 0 .. pools-1
    and the predictor; ``pool``: :func:`pool_backward`'s dict per round; ``round_terms``: {parameter name: [each round's own
    dW / db]} for theta / phi / g"""
    f = forward(sd, past, dest, pos, mask, pools)
    n, fdim = f["feat"][0].shape[0], f["z"]["encoder_past"][-1].shape[1]
    grads, gerrs, gz, gzerr = {}, {}, {}, {}
    g = np.asarray(g_out, np.float64)
    G, eG = TN._chain_backward(sd, "predictor", f["acts"]["predictor"], f["acts_err"]["predictor"], acts_mask["predictor"],
                               g, np.zeros_like(g), grads, gerrs, gz, gzerr)
    gfeat, gfeat_err, pool = [None] * (pools + 1), [None] * (pools + 1), [None] * pools
    gfeat[pools], gfeat_err[pools] = G, eG
    per_round = {c: [None] * pools for c in POOLED}  # (gz list, gz_err list) of the round
    terms = {}
    for r in range(pools - 1, -1, -1):
        zs = [(f["z"][c][r][-1], f["z_err"][c][r][-1]) for c in POOLED]
        pb = pool_backward(f["rounds"][r], *zs[0], *zs[1], *zs[2], G, eG)
        pool[r] = pb
        parts = []
        for c, key in zip(POOLED, ("dtheta", "dphi", "dg")):
            gr, ge, z_, ze_ = {}, {}, {}, {}
            m = [np.asarray(a)[r * n:(r + 1) * n] for a in acts_mask[c]]
            parts.append(TN._chain_backward(sd, c, f["acts"][c][r], f["acts_err"][c][r], m, pb[key], pb["e" + key], gr, ge,
                                            z_, ze_))
            per_round[c][r] = (z_[c], ze_[c])
            for name in gr:
                terms.setdefault(name, [None] * pools)[r] = gr[name]
        val, mag, err = G, np.abs(G) + eG, eG
        for a, ea in parts:  # ((G + theta's) + phi's) + g's
            val, mag, err = val + a, mag + np.abs(a) + ea, err + ea
        G, eG = val, err + gamma(3) * mag
        gfeat[r], gfeat_err[r] = G, eG
    # the shared weights: one dot product over the rows of all rounds
    for c in POOLED if pools else ():
        nl = TN.n_layers(sd, c)
        gz[c] = [np.concatenate([per_round[c][r][0][i] for r in range(pools)]) for i in range(nl)]
        gzerr[c] = [np.concatenate([per_round[c][r][1][i] for r in range(pools)]) for i in range(nl)]
        for i in range(nl):
            a = np.concatenate([f["acts"][c][r][i] for r in range(pools)])
            ea = np.concatenate([f["acts_err"][c][r][i] for r in range(pools)])
            grads[f"{c}.layers.{i}.weight"], gerrs[f"{c}.layers.{i}.weight"] = _dot(gz[c][i].T, gzerr[c][i].T, a, ea)
            ones = np.ones((a.shape[0], 1))
            db, edb = _dot(gz[c][i].T, gzerr[c][i].T, ones, np.zeros_like(ones))
            grads[f"{c}.layers.{i}.bias"], gerrs[f"{c}.layers.{i}.bias"] = db[:, 0], edb[:, 0]
    for chain, key, sl in (("encoder_past", "past", slice(0, fdim)), ("encoder_dest", "dest", slice(fdim, 2 * fdim))):
        grads[key], gerrs[key] = TN._chain_backward(sd, chain, f["acts"][chain], f["acts_err"][chain], acts_mask[chain],
                                                    G[:, sl], eG[:, sl], grads, gerrs, gz, gzerr)
    grads["pos"], gerrs["pos"] = G[:, 2 * fdim:], eG[:, 2 * fdim:]
    return {"grads": grads, "grads_err": gerrs, "gz": gz, "gz_err": gzerr, "gfeat": gfeat, "gfeat_err": gfeat_err,
            "pool": pool, "round_terms": terms, "forward": f}
