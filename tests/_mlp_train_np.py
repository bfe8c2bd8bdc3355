"""float64 numpy restatement of csrc/et_mlp_train.hip, independent of torch: the forward of the three chains ``predict`` of
LBEBM runs (with every activation), their backward pass, and a running elementwise error bound for what the fp32 kernels
may differ by.  The bounds are the only tolerances tests/test_gpu_mlp_train.py uses; they are derived here, not tuned.

Notation for a chain of L layers: a_0 the input, z_i = a_{i-1} W_i^T + b_i, a_i = relu(z_i) for i < L, output z_L;
backward g_z(L) = g_out, g_a(i-1) = g_z(i) W_i, g_z(i-1) = g_a(i-1) * mask(i-1), dW_i = g_z(i)^T a_{i-1}, db_i = the
column sums of g_z(i).  The predictor's a_0 is [encoder_past's output | encoder_dest's output]; its g_a(0) splits at
column fdim into the two encoders' g_out.

The bound.  u = 2^-24 is the unit roundoff of fp32 and gamma_K = K u / (1 - K u).  Every value the kernels form is a dot
product s = sum_k x_k y_k of K terms evaluated as a chain of K fp32 fmaf from a zero accumulator (the f32-input MFMA),
possibly followed by one more fp32 addition (the bias), on operands x^, y^ that are themselves computed: |x^ - x| <= ex,
|y^ - y| <= ey elementwise (0 for an input, a weight or g_out).  Then (Higham, Accuracy and Stability of Numerical
Algorithms, 2nd ed., eq. 3.5, K + 1 roundings at the most, in ANY order of summation)

    |fl(s^) - s|  <=  gamma_(K+1) * sum_k |x^_k||y^_k|  +  |s^ - s|
                  <=  gamma_(K+1) * (sum_k (|x_k| + ex_k)(|y_k| + ey_k) + |b|)
                      + sum_k ex_k (|y_k| + ey_k) + sum_k |x_k| ey_k

which is what :func:`_dot` returns next to the float64 value: the first term is the rounding of this dot product on the
operands as the kernel has them, the others carry the operands' own bounds through |y|, |x| (for the layers: through |W|,
|a| or |g|).  The zero padding of a chain (up to a multiple of 4 or 16) adds exact zeros and no rounding.  relu is
1-Lipschitz, so an activation inherits its pre-activation's bound.  The backward takes the ReLU masks as an ARGUMENT (the
masks the native forward produced, a > 0): restatement and kernel then zero the same elements exactly, the bound of a masked
element is 0 and that of a passed one is its g_a's; whether the native masks are right is the forward test's business (an
activation of 0 needs z <= its bound, a positive one z > -bound).  The float64 arithmetic of this file has its own rounding,
bounded the same way with 2^-53 in place of 2^-24; U below is 2^-24 + 2^-50, which covers both for every K used here
(K < 2^20).
"""
import numpy as np

CHAINS = ("encoder_past", "encoder_dest", "predictor")
U = 2.0 ** -24 + 2.0 ** -50


def gamma(k):
    return k * U / (1.0 - k * U)


def n_layers(sd, chain):
    return 1 + max(int(k.split(".")[2]) for k in sd if k.startswith(chain + ".layers."))


def _w(sd, chain, i, kind):
    return np.asarray(sd[f"{chain}.layers.{i}.{kind}"], np.float64)


def _dot(x, ex, y, ey, bias=None):
    """x (M, K) +- ex times y (K, P) +- ey (+ bias (P,)) -> (value, bound), the docstring's inequality"""
    k = x.shape[1]
    ax, ay = np.abs(x), np.abs(y)
    val = x @ y
    mag = (ax + ex) @ (ay + ey)
    if bias is not None:
        val = val + bias
        mag = mag + np.abs(bias)
    return val, gamma(k + 1) * mag + ex @ (ay + ey) + ax @ ey


def _chain_forward(sd, chain, a0, e0):
    """-> acts [a_0 .. a_{L-1}], their bounds, z [z_1 .. z_L], their bounds"""
    acts, errs, zs, zerrs = [a0], [e0], [], []
    nl = n_layers(sd, chain)
    for i in range(nl):
        w = _w(sd, chain, i, "weight")
        z, ez = _dot(acts[-1], errs[-1], w.T, np.zeros_like(w.T), _w(sd, chain, i, "bias"))
        zs.append(z)
        zerrs.append(ez)
        if i + 1 < nl:
            acts.append(np.maximum(z, 0.0))
            errs.append(ez)
    return acts, errs, zs, zerrs


def forward(sd, past, dest):
    """-> dict: ``out`` (N, out_width) and ``out_err``; per chain name ``acts`` [a_0 .. a_{L-1}] / ``acts_err`` and ``z``
    [z_1 .. z_L] / ``z_err`` (a_i = relu(z_i); the list index of z_i is i - 1), everything float64"""
    past, dest = np.asarray(past, np.float64), np.asarray(dest, np.float64)
    r = {"acts": {}, "acts_err": {}, "z": {}, "z_err": {}}
    for chain, a0 in (("encoder_past", past), ("encoder_dest", dest)):
        r["acts"][chain], r["acts_err"][chain], r["z"][chain], r["z_err"][chain] = _chain_forward(
            sd, chain, a0, np.zeros_like(a0))
    feat = np.concatenate([r["z"]["encoder_past"][-1], r["z"]["encoder_dest"][-1]], axis=1)
    efeat = np.concatenate([r["z_err"]["encoder_past"][-1], r["z_err"]["encoder_dest"][-1]], axis=1)
    r["acts"]["predictor"], r["acts_err"]["predictor"], r["z"]["predictor"], r["z_err"]["predictor"] = _chain_forward(
        sd, "predictor", feat, efeat)
    r["out"], r["out_err"] = r["z"]["predictor"][-1], r["z_err"]["predictor"][-1]
    return r


def masks_of(acts):
    """{chain: [a_1 > 0 .. a_{L-1} > 0]} from {chain: [a_1 .. a_{L-1}]} (hidden activations only, any array type)"""
    return {chain: [np.asarray(a) > 0 for a in acts[chain]] for chain in acts}


def _chain_backward(sd, chain, acts, acts_err, masks, g, eg, grads, gerrs, gz, gzerr):
    """g = g_z(L) +- eg; fills the chain's dW / db and g_z lists; -> g_a(0) and its bound"""
    nl = n_layers(sd, chain)
    gz[chain], gzerr[chain] = [None] * nl, [None] * nl  # index i - 1 holds g_z(i)
    for i in range(nl - 1, -1, -1):
        gz[chain][i], gzerr[chain][i] = g, eg
        w = _w(sd, chain, i, "weight")
        grads[f"{chain}.layers.{i}.weight"], gerrs[f"{chain}.layers.{i}.weight"] = _dot(g.T, eg.T, acts[i], acts_err[i])
        ones = np.ones((g.shape[0], 1))
        db, edb = _dot(g.T, eg.T, ones, np.zeros_like(ones))
        grads[f"{chain}.layers.{i}.bias"], gerrs[f"{chain}.layers.{i}.bias"] = db[:, 0], edb[:, 0]
        g, eg = _dot(g, eg, w, np.zeros_like(w))
        if i > 0:
            m = np.asarray(masks[i - 1], bool)
            g, eg = np.where(m, g, 0.0), np.where(m, eg, 0.0)
    return g, eg


def backward(sd, acts_mask, past, dest, g_out):
    """``acts_mask`` {chain: [mask of a_1 .. mask of a_{L-1}]} (bool, a > 0 as the forward under test produced them) ->
    dict: ``grads`` / ``grads_err`` keyed by parameter name plus ``past`` and ``dest`` (the input gradients), ``gz`` /
    ``gz_err`` per chain [g_z(1) .. g_z(L)]"""
    f = forward(sd, past, dest)
    fdim = f["z"]["encoder_past"][-1].shape[1]
    grads, gerrs, gz, gzerr = {}, {}, {}, {}
    g = np.asarray(g_out, np.float64)
    gf, egf = _chain_backward(sd, "predictor", f["acts"]["predictor"], f["acts_err"]["predictor"], acts_mask["predictor"],
                              g, np.zeros_like(g), grads, gerrs, gz, gzerr)
    for chain, key, sl in (("encoder_past", "past", slice(0, fdim)), ("encoder_dest", "dest", slice(fdim, 2 * fdim))):
        grads[key], gerrs[key] = _chain_backward(sd, chain, f["acts"][chain], f["acts_err"][chain], acts_mask[chain],
                                                 gf[:, sl], egf[:, sl], grads, gerrs, gz, gzerr)
    return {"grads": grads, "grads_err": gerrs, "gz": gz, "gz_err": gzerr}
