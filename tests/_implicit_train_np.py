"""float64 numpy restatement of the training pass of csrc/et_implicit.hip, independent of torch: SocialImplicitLight's
forward (tests/_implicit_np.py's, every intermediate kept), the backward pass to the 18 tensors of every cell that the
forward reads, and a running elementwise bound for what the fp32 kernels may differ by.  The bounds are the only tolerances
tests/test_gpu_implicit_train.py uses; they are derived here, not tuned.

One zone's cell on its n pedestrians COMPACTED in scene order, x (T, n), G (S, T_out, n) the upstream gradient:

    pre  = feat(x)                        (S, T, n)    3x3 over the (T, n) plane, zero-padded
    u    = relu(pre) + highway_input(x)   (S, T, n)
    g    = tpcnn(u) + highway(u)          (T_out, S, n) T as channels, 3x3 over the (S, n) plane, zero-padding u
    prel, ul, l                           the same per pedestrian with 1-d convolutions; l (T_out, S, n)
    out  = global_w g^T + local_w reshape(l)           reshape: the (T_out, S) block READ AS (S, T_out) by flat index

    dg[o, s] = global_w G[s, o]           dl.flat = local_w G.flat      (the inverse of that reshape: the same flat index)
    d global_w = sum G g^T,  d local_w = sum G reshape(l)
    d tpcnn.weight[o, t, ds, dj] = sum_{s, j} dg[o, s, j] u_pad[t, s + ds - 1, j + dj - 1],  d highway.weight = sum dg u, biases: sum dg
    du = tpcnn^T dg + highway^T dg,   dpre = du where pre > 0 (a NaN pre passes, as torch's relu backward), else 0
    d feat.weight[s, dt, dj] = sum_{t, j} dpre[s, t, j] x_pad[t + dt - 1, j + dj - 1],  d highway_input.weight = sum du x, ...

The kernel groups the same terms BY THE PEDESTRIAN WHOSE OUTPUT READ THEM: pedestrian j forms u at the compacted positions
j - 1, j, j + 1 (q = 0, 1, 2) and the du of those three planes through its own dg alone; the dense du at a position is the
sum of the three readers' parts.  This file follows that grouping (shifts along the compacted axis, no neighbour table),
because the bound of a sum is the sum of its parts' bounds; tests/test_implicit_train_cpu.py shows it equal to torch's
autograd of the dense form above.

The bound.  u = 2^-24, gamma_K = K u / (1 - K u).  Every value the kernel forms is a sum of K products, an fmaf chain
from an accumulator, on operands x^, y^ that are themselves computed, |x^ - x| <= ex, |y^ - y| <= ey.  A term of such a
chain meets at most K roundings when every step is one fmaf and at most K + 1 when the product is rounded on its own
before the addition, so for ANY order of summation, with or without contraction of a*b + c (Higham, Accuracy and Stability
of Numerical Algorithms, 2nd ed., eq. 3.5; tests/_mlp_train_np.py's ``_dot`` is the same formula)

    |fl(s^) - s|  <=  gamma_(K+R) sum (|x| + ex)(|y| + ey)  +  sum ex (|y| + ey) + |x| ey

with R = 1 plus the roundings that follow the chain.  K is the TRUE length of the accumulator's chain.  A gradient element
is ONE accumulator over the terms of all the zone's pedestrians of a chunk, and the chunks' partial sums are added after:
K counts the terms of all n pedestrians (S n; S T_out n for the two scalars; T n for the local feat stream; 3 T n for the
global feat stream, whose accumulator runs over the three positions too) and R = n + 1, n being at least the number of
chunk additions.  Where the kernel multiplies once more before a chain (dg = global_w G) the product's own rounding is
carried as that operand's bound.  The float64 arithmetic of this file has its own rounding, bounded the same way with
2^-53; U below is 2^-24 + 2^-50, which covers both.

ReLU.  The mask is decided on the float64 pre; an element with |pre| <= its bound is UNDECIDED (the kernel may have decided
otherwise) and is counted: the tests' inputs are chosen so that there is none.  NaN: the arithmetic is dense, a NaN operand
makes NaN values and bounds; comparisons with a NaN bound are the caller's business (see :func:`compare`)."""
import numpy as np

from . import _implicit_np as IN

U = 2.0 ** -24 + 2.0 ** -50
GLOBAL = ("feat", "highway_input", "highway", "tpcnn")
KINDS = [f"{p}{n}.{k}" for p in ("", "ped.") for n in GLOBAL for k in ("weight", "bias")] + ["global_w", "local_w"]


def gamma(k):
    return k * U / (1.0 - k * U)


class V:
    """a float64 array and the elementwise bound of the kernel's fp32 value of it"""

    def __init__(self, val, err=None):
        self.val = np.asarray(val, np.float64)
        self.err = np.zeros_like(self.val) if err is None else np.asarray(err, np.float64)

    def __getitem__(self, idx):
        return V(self.val[idx], self.err[idx])

    @property
    def mag(self):
        return np.abs(self.val) + self.err


def dot(spec, x, y, k, extra=0, init=None):
    """einsum(spec, x, y) (+ init) as a chain of ``k`` products per element and ``extra`` more roundings (1 for a chain
    alone: its initial accumulator, or a product rounded on its own) -> V with gamma_(k + extra), the docstring's bound"""
    with np.errstate(invalid="ignore"):
        val = np.einsum(spec, x.val, y.val)
        mag = np.einsum(spec, x.mag, y.mag)
        err = np.einsum(spec, x.err, y.mag) + np.einsum(spec, np.abs(x.val), y.err)
        if init is not None:
            val, mag, err = val + init.val, mag + init.mag, err + init.err
        return V(val, gamma(k + extra) * mag + err)


def add(*parts, roundings):
    """the sum of V's with ``roundings`` roundings on the way"""
    with np.errstate(invalid="ignore"):
        val = sum(p.val for p in parts)
        return V(val, sum(p.err for p in parts) + gamma(roundings) * sum(p.mag for p in parts))


def _shift(a, k, axis):
    """b[..., i, ...] = a[..., i + k, ...], zero where i + k is outside"""
    out = np.zeros_like(a)
    n = a.shape[axis]
    src = [slice(None)] * a.ndim
    dst = [slice(None)] * a.ndim
    lo, hi = max(0, -k), min(n, n - k)
    if lo < hi:
        dst[axis], src[axis] = slice(lo, hi), slice(lo + k, hi + k)
        out[tuple(dst)] = a[tuple(src)]
    return out


def shift(v, k, axis):
    return V(_shift(v.val, k, axis), _shift(v.err, k, axis))


def _relu(pre):
    """relu of a V (1-Lipschitz: the bound passes), the pass mask (pre > 0 or NaN) and the number of undecided elements"""
    with np.errstate(invalid="ignore"):
        mask = ~(pre.val <= 0)
        undecided = int(((np.abs(pre.val) <= pre.err) & (pre.err > 0)).sum())  # bound 0: every term is an exact zero
        return V(np.where(pre.val < 0, 0.0, pre.val), pre.err), mask, undecided


def cell(sd, pre, x, G, transpose=False, n_sum=None):
    """One zone's cell on its compacted pedestrians: x (T, n) fp32 values, G (S, T_out, n) -> dict: ``out`` V (S, T_out, n),
    ``grads`` {kind: V}, ``undecided`` (ReLU elements within their bound of 0), ``parts`` the intermediates.  ``n_sum``: the
    number of pedestrians whose terms share the kernel's accumulators (more than n when the scenes of a batch are summed)."""
    w = lambda name: V(np.asarray(sd[pre + name], np.float64))
    x = V(x)
    T, n = x.val.shape
    ns = n if n_sum is None else n_sum
    G = V(G)
    S, To = G.val.shape[:2]
    und = 0
    # ---- forward, global stream: position q in 0..2 is the compacted neighbour j + q - 1 of reader j
    fw, fb, hiw, hib = w("feat.weight"), w("feat.bias"), w("highway_input.weight"), w("highway_input.bias")
    hw, hb, tw, tb = w("highway.weight"), w("highway.bias"), w("tpcnn.weight"), w("tpcnn.bias")
    # x at (t + dt - 1, j + dj - 1): xs[dt][dj]
    xs = [[shift(shift(x, dt - 1, 0), dj - 1, 1) for dj in range(3)] for dt in range(3)]
    pre_v = V(fb.val[:, None, None] + np.zeros((S, T, n)))
    terms, mags = pre_v.val.copy(), np.abs(pre_v.val)
    with np.errstate(invalid="ignore"):
        for dt in range(3):
            for dj in range(3):
                terms = terms + fw.val[:, 0, dt, dj][:, None, None] * xs[dt][dj].val[None]
                mags = mags + np.abs(fw.val[:, 0, dt, dj])[:, None, None] * np.abs(xs[dt][dj].val)[None]
    pre_v = V(terms, gamma(9 + 1) * mags)
    r, mask, k = _relu(pre_v)
    und += k
    with np.errstate(invalid="ignore"):
        hwy = V(hiw.val[:, 0, 0, 0][:, None, None] * x.val[None] + hib.val[:, None, None])
        hwy.err = gamma(2) * (np.abs(hiw.val[:, 0, 0, 0])[:, None, None] * np.abs(x.val)[None] + np.abs(hib.val)[:, None, None])
    u = add(r, hwy, roundings=1)                                   # (S, T, n), u of pedestrian j at its own position
    exists = [np.arange(n) + q - 1 for q in range(3)]
    exists = [(e >= 0) & (e < n) for e in exists]                  # reader j has a neighbour at position q
    uq = [shift(u, q - 1, 2) for q in range(3)]                    # u at position q of reader j (0 where there is none)
    # g[o, s, j] = tb[o] + sum_{t, ds, dj} tw[o, t, ds, dj] uq[dj][t, s + ds - 1, j]  +  hb[o] + sum_t hw[o, t] u[t, s, j]
    acc_val = tb.val[:, None, None] + np.zeros((To, S, n))
    acc_mag, acc_err = np.abs(acc_val), np.zeros_like(acc_val)
    with np.errstate(invalid="ignore"):
        for ds in range(3):
            for dj in range(3):
                us = shift(uq[dj], ds - 1, 0)                      # (S, T, n) at s + ds - 1
                acc_val = acc_val + np.einsum("ot,stn->osn", tw.val[:, :, ds, dj], us.val)
                acc_mag = acc_mag + np.einsum("ot,stn->osn", np.abs(tw.val[:, :, ds, dj]), us.mag)
                acc_err = acc_err + np.einsum("ot,stn->osn", np.abs(tw.val[:, :, ds, dj]), us.err)
    conv = V(acc_val, gamma(9 * T + 1) * acc_mag + acc_err)
    res = dot("ot,stn->osn", V(hw.val[:, :, 0, 0]), u, T, 1, init=V(hb.val[:, None, None] + np.zeros((To, S, n))))
    g = add(conv, res, roundings=1)                                # (T_out, S, n)
    # ---- forward, local stream
    lfw, lfb, lhiw, lhib = w("ped.feat.weight"), w("ped.feat.bias"), w("ped.highway_input.weight"), w("ped.highway_input.bias")
    lhw, lhb, ltw, ltb = w("ped.highway.weight"), w("ped.highway.bias"), w("ped.tpcnn.weight"), w("ped.tpcnn.bias")
    with np.errstate(invalid="ignore"):
        terms = lfb.val[:, None, None] + np.zeros((S, T, n))
        mags = np.abs(terms)
        for dt in range(3):
            terms = terms + lfw.val[:, 0, dt][:, None, None] * xs[dt][1].val[None]
            mags = mags + np.abs(lfw.val[:, 0, dt])[:, None, None] * np.abs(xs[dt][1].val)[None]
        prel = V(terms, gamma(3 + 1) * mags)
        rl, maskl, k = _relu(prel)
        und += k
        hwyl = V(lhiw.val[:, 0, 0][:, None, None] * x.val[None] + lhib.val[:, None, None])
        hwyl.err = gamma(2) * (np.abs(lhiw.val[:, 0, 0])[:, None, None] * np.abs(x.val)[None] + np.abs(lhib.val)[:, None, None])
    ul = add(rl, hwyl, roundings=1)                                # (S, T, n)
    acc_val = ltb.val[:, None, None] + np.zeros((To, S, n))
    acc_mag, acc_err = np.abs(acc_val), np.zeros_like(acc_val)
    with np.errstate(invalid="ignore"):
        for ds in range(3):
            us = shift(ul, ds - 1, 0)
            acc_val = acc_val + np.einsum("ot,stn->osn", ltw.val[:, :, ds], us.val)
            acc_mag = acc_mag + np.einsum("ot,stn->osn", np.abs(ltw.val[:, :, ds]), us.mag)
            acc_err = acc_err + np.einsum("ot,stn->osn", np.abs(ltw.val[:, :, ds]), us.err)
    convl = V(acc_val, gamma(3 * T + 1) * acc_mag + acc_err)
    resl = dot("ot,stn->osn", V(lhw.val[:, :, 0]), ul, T, 1, init=V(lhb.val[:, None, None] + np.zeros((To, S, n))))
    l = add(convl, resl, roundings=1)                              # (T_out, S, n)
    gt = V(np.transpose(g.val, (1, 0, 2)), np.transpose(g.err, (1, 0, 2)))  # (S, T_out, n)
    if transpose:
        lr = V(np.transpose(l.val, (1, 0, 2)), np.transpose(l.err, (1, 0, 2)))
    else:
        lr = V(l.val.reshape(S, To, n), l.err.reshape(S, To, n))   # flat (T_out, S) read as (S, T_out)
    gw, lw = float(w("global_w").val[0]), float(w("local_w").val[0])
    with np.errstate(invalid="ignore"):
        a, b = V(gw * gt.val, abs(gw) * gt.err), V(lw * lr.val, abs(lw) * lr.err)
        out = add(a, b, roundings=3)

    # ---- backward.  rounds: the pedestrians, each of whose terms continue one accumulator, and the chunks after them
    grads = {}
    grads["global_w"] = dot("son,son->", G, gt, S * To * ns, ns + 1)
    grads["local_w"] = dot("son,son->", G, lr, S * To * ns, ns + 1)
    for key in ("global_w", "local_w"):
        grads[key] = V(grads[key].val.reshape(1), grads[key].err.reshape(1))
    with np.errstate(invalid="ignore"):
        dg = V(gw * np.transpose(G.val, (1, 0, 2)))                # (T_out, S, n)
        dg.err = U * np.abs(dg.val)
        Gl = G.val.reshape(S * To, n).reshape(To, S, n) if not transpose else np.transpose(G.val, (1, 0, 2))
        dl = V(lw * Gl)
        dl.err = U * np.abs(dl.val)
    ones = V(np.ones((S, n)))
    # global temporal section
    grads["tpcnn.bias"] = dot("osn,sn->o", dg, ones, S * ns, ns + 1)
    grads["highway.bias"] = dot("osn,sn->o", dg, ones, S * ns, ns + 1)
    hwg = dot("osn,stn->ot", dg, u, S * ns, ns + 1)
    grads["highway.weight"] = V(hwg.val[:, :, None, None], hwg.err[:, :, None, None])
    tg_val, tg_err = np.zeros((To, T, 3, 3)), np.zeros((To, T, 3, 3))
    for ds in range(3):
        for dj in range(3):
            part = dot("osn,stn->ot", dg, shift(uq[dj], ds - 1, 0), S * ns, ns + 1)
            tg_val[:, :, ds, dj], tg_err[:, :, ds, dj] = part.val, part.err
    grads["tpcnn.weight"] = V(tg_val, tg_err)
    # du of reader j at its position q, (S, T, n): sum_{o, ds} tw[o, t, ds, q] dg[o, s - ds + 1, j] (+ highway at q = 1)
    feat_w = [[None] * 3 for _ in range(3)]
    fb_parts, hiw_parts, hib_parts = [], [], []
    for q in range(3):
        val, mag, err = np.zeros((S, T, n)), np.zeros((S, T, n)), np.zeros((S, T, n))
        with np.errstate(invalid="ignore"):
            for ds in range(3):
                d = shift(dg, 1 - ds, 1)                            # dg[o, s - ds + 1, j]
                val = val + np.einsum("ot,osn->stn", tw.val[:, :, ds, q], d.val)
                mag = mag + np.einsum("ot,osn->stn", np.abs(tw.val[:, :, ds, q]), d.mag)
                err = err + np.einsum("ot,osn->stn", np.abs(tw.val[:, :, ds, q]), d.err)
            k = 3 * To
            if q == 1:
                val = val + np.einsum("ot,osn->stn", hw.val[:, :, 0, 0], dg.val)
                mag = mag + np.einsum("ot,osn->stn", np.abs(hw.val[:, :, 0, 0]), dg.mag)
                err = err + np.einsum("ot,osn->stn", np.abs(hw.val[:, :, 0, 0]), dg.err)
                k += To
            du = V(val, gamma(k + 1) * mag + err)
            e = exists[q][None, None, :]
            du = V(np.where(e, du.val, 0.0), np.where(e, du.err, 0.0))   # a missing neighbour carries no gradient
            mq = _shift(mask.astype(np.float64), q - 1, 2) > 0           # the ReLU mask at position q of reader j
            dp = V(np.where(mq & e, du.val, 0.0), np.where(mq & e, du.err, 0.0))
        xq = shift(x, q - 1, 1)                                     # the column at position q of reader j
        hiw_parts.append(dot("stn,tn->s", du, xq, 3 * T * ns, ns + 1))
        hib_parts.append(dot("stn,tn->s", du, V(np.ones((T, n))), 3 * T * ns, ns + 1))
        fb_parts.append(dot("stn,tn->s", dp, V(np.ones((T, n))), 3 * T * ns, ns + 1))
        for dt in range(3):
            for dj in range(3):
                # x at (t + dt - 1, position q + dj - 1 of reader j) = compacted j + q + dj - 2
                feat_w[dt][dj] = (feat_w[dt][dj] or []) + [dot("stn,tn->s", dp, shift(shift(x, dt - 1, 0), q + dj - 2, 1),
                                                               3 * T * ns, ns + 1)]
    # the three positions' terms continue ONE accumulator: each part above carries gamma of the whole chain (3 T n terms),
    # so the parts' bounds add up to the chain's
    tot = lambda parts: V(sum(p.val for p in parts), sum(p.err for p in parts))
    grads["feat.bias"], grads["highway_input.bias"] = tot(fb_parts), tot(hib_parts)
    h = tot(hiw_parts)
    grads["highway_input.weight"] = V(h.val[:, None, None, None], h.err[:, None, None, None])
    fw_val, fw_err = np.zeros((S, 1, 3, 3)), np.zeros((S, 1, 3, 3))
    for dt in range(3):
        for dj in range(3):
            p = tot(feat_w[dt][dj])
            fw_val[:, 0, dt, dj], fw_err[:, 0, dt, dj] = p.val, p.err
    grads["feat.weight"] = V(fw_val, fw_err)
    # local stream
    grads["ped.tpcnn.bias"] = dot("osn,sn->o", dl, ones, S * ns, ns + 1)
    grads["ped.highway.bias"] = dot("osn,sn->o", dl, ones, S * ns, ns + 1)
    p = dot("osn,stn->ot", dl, ul, S * ns, ns + 1)
    grads["ped.highway.weight"] = V(p.val[:, :, None], p.err[:, :, None])
    tg_val, tg_err = np.zeros((To, T, 3)), np.zeros((To, T, 3))
    for ds in range(3):
        part = dot("osn,stn->ot", dl, shift(ul, ds - 1, 0), S * ns, ns + 1)
        tg_val[:, :, ds], tg_err[:, :, ds] = part.val, part.err
    grads["ped.tpcnn.weight"] = V(tg_val, tg_err)
    val, mag, err = np.zeros((S, T, n)), np.zeros((S, T, n)), np.zeros((S, T, n))
    with np.errstate(invalid="ignore"):
        for ds in range(3):
            d = shift(dl, 1 - ds, 1)
            val = val + np.einsum("ot,osn->stn", ltw.val[:, :, ds], d.val)
            mag = mag + np.einsum("ot,osn->stn", np.abs(ltw.val[:, :, ds]), d.mag)
            err = err + np.einsum("ot,osn->stn", np.abs(ltw.val[:, :, ds]), d.err)
        val = val + np.einsum("ot,osn->stn", lhw.val[:, :, 0], dl.val)
        mag = mag + np.einsum("ot,osn->stn", np.abs(lhw.val[:, :, 0]), dl.mag)
        err = err + np.einsum("ot,osn->stn", np.abs(lhw.val[:, :, 0]), dl.err)
        dul = V(val, gamma(4 * To + 1) * mag + err)
        dpl = V(np.where(maskl, dul.val, 0.0), np.where(maskl, dul.err, 0.0))
    grads["ped.feat.bias"] = dot("stn,tn->s", dpl, V(np.ones((T, n))), T * ns, ns + 1)
    grads["ped.highway_input.bias"] = dot("stn,tn->s", dul, V(np.ones((T, n))), T * ns, ns + 1)
    p = dot("stn,tn->s", dul, x, T * ns, ns + 1)
    grads["ped.highway_input.weight"] = V(p.val[:, None, None], p.err[:, None, None])
    fw_val, fw_err = np.zeros((S, 1, 3)), np.zeros((S, 1, 3))
    for dt in range(3):
        p = dot("stn,tn->s", dpl, shift(x, dt - 1, 0), T * ns, ns + 1)
        fw_val[:, 0, dt], fw_err[:, 0, dt] = p.val, p.err
    grads["ped.feat.weight"] = V(fw_val, fw_err)
    return {"out": out, "grads": grads, "undecided": und,
            "parts": {"pre": pre_v, "u": u, "g": g, "prel": prel, "ul": ul, "l": l, "dg": dg, "dl": dl}}


def shapes(sd, prefix="implicit_cells.0."):
    return {kind: np.asarray(sd[prefix + kind]).shape for kind in KINDS}


def run(sd, v, G, bins=IN.BINS, transpose=False, n_sum=None):
    """sd: state_dict (numpy), v (T, N) fp32 of ONE scene, G (S, T_out, N) the upstream gradient of the raw output -> dict:
    ``out`` / ``out_err`` (S, T_out, N); ``grads`` / ``grads_err`` {state_dict key: array} for the 18 tensors of every cell
    (zeros, bound 0, for a cell without pedestrians); ``visited`` (n_bins,) bool; ``undecided`` the ReLU elements that lie
    within their bound of 0.  ``n_sum``: see :func:`cell`."""
    v32 = np.asarray(v, np.float32)
    G = np.asarray(G, np.float64)
    z = IN.zones(v32, bins)
    S, To = G.shape[:2]
    res = {"out": np.zeros((S, To, v32.shape[1])), "out_err": np.zeros((S, To, v32.shape[1])), "grads": {}, "grads_err": {},
           "visited": np.zeros(len(bins), bool), "undecided": 0, "zone": z}
    for i in range(len(bins)):
        sel = z == i
        pre = f"implicit_cells.{i}."
        if sel.any():
            c = cell(sd, pre, v32[:, sel].astype(np.float64), G[:, :, sel], transpose, n_sum)
            res["out"][:, :, sel], res["out_err"][:, :, sel] = c["out"].val, c["out"].err
            res["visited"][i] = True
            res["undecided"] += c["undecided"]
            for kind in KINDS:
                res["grads"][pre + kind], res["grads_err"][pre + kind] = c["grads"][kind].val, c["grads"][kind].err
        else:
            for kind, shape in shapes(sd, pre).items():
                res["grads"][pre + kind], res["grads_err"][pre + kind] = np.zeros(shape), np.zeros(shape)
    return res


def block(sd, grads, n_bins):
    """{state_dict key: array} -> (n_bins, G) in et_implicit_cell's field order, the layout of the native gradient block"""
    return np.stack([np.concatenate([np.asarray(grads[f"implicit_cells.{i}.{kind}"], np.float64).ravel() for kind in KINDS])
                     for i in range(n_bins)])


def kind_of_column(sd):
    """(G,) the index into KINDS of every column of the gradient block"""
    return np.concatenate([np.full(int(np.prod(shape)), k) for k, shape in enumerate(shapes(sd).values())])


def compare(got, want, bound):
    """-> (ok, worst error / bound, NaN pattern equal): every finite element of ``want`` within its bound (an exact zero
    bound asks for equality), the NaNs in the same places"""
    got, want, bound = (np.asarray(a, np.float64) for a in (got, want, bound))
    nan = np.isnan(want) | np.isnan(bound)
    same_nan = bool(np.array_equal(np.isnan(got), nan))
    fin = ~nan & ~np.isnan(got)
    err = np.abs(got - want)[fin]
    ok = bool((err <= bound[fin]).all())
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bound[fin])
    return ok and same_nan, float(ratio.max()) if ratio.size else 0.0, same_nan
