"""The three single-workgroup kernels of the training form (csrc/et_train.hip: et_scene_project_train,
et_wrapper_losses_fwd, et_wrapper_losses_bwd), called through the C ABI the way model.py calls them, against the float64
restatement of the reference (tests/_train_np.py): every floating-point output element-wise within the fp32 bound of its
dot product, (n + 8) * 2**-24 * M, `flag` and `arg` exactly.  tests/test_train_cpu.py proves what this relies on: the
restatement itself, and that the seeded inputs keep the hard decisions clear (undecided row-terms <= 1 %, tau = 1e-4)."""
import math
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from . import _train_np as R
from ._gpu_common import N_, T, dev, ops  # noqa: F401  (dev, ops: fixtures)

pytestmark = pytest.mark.gpu

IDS = dict(ids=lambda s: "-".join(map(str, s)) if isinstance(s, tuple) else str(s))
WEIGHTS = (0.3, 1.7, -2.0)


# ------------------------------------------------------------------------------------------------ calling the ABI
def _p(t):
    return None if t is None else t.data_ptr()


def _d(a, dev, dtype=np.float32):
    return None if a is None else T(np.asarray(a, dtype), dev)


def _nan(shape, dev):
    return torch.full(shape, float("nan"), device=dev)


def call_project(ops, dev, c, mode, want_flag=True):
    """et_scene_project_train on a case -> C_obs, nrm, obs_ori, C_gt, flag (None if not asked for); outputs start as NaN"""
    obs, pred = T(c.obs, dev), T(c.pred, dev)
    U = [_d(u, dev) for u in (*R.u_for(c, mode, obs=True), *R.u_for(c, mode))]
    out = NS(C_obs=_nan((c.k, c.n), dev), nrm=_nan((4, c.n), dev), obs_ori=_nan((2, c.n), dev), C_gt=_nan((c.k, c.n), dev),
             flag=torch.full((c.n,), 255, device=dev, dtype=torch.uint8) if want_flag else None)
    rc = ops.L.lib().et_scene_project_train(obs.data_ptr(), pred.data_ptr(), c.n, c.t_obs, c.t_pred, c.k, *map(_p, U), mode,
                                            c.static_dist, out.C_obs.data_ptr(), out.nrm.data_ptr(), out.obs_ori.data_ptr(),
                                            out.C_gt.data_ptr(), _p(out.flag), ops.L.raw_stream(dev.index))
    assert rc == 0
    torch.cuda.synchronize()
    return out


def inputs(c, mode, anchors=True, **over):
    """the arguments of the loss kernels and of R.losses / R.grad for a case (numpy, None = NULL)"""
    nrm, C_gt = R.loss_inputs(c, mode)
    A_m, A_s = R.a_for(c, mode, anchors)
    U_m, U_s = R.u_for(c, mode)
    i = NS(C=c.C, nrm=nrm, A_m=A_m, A_s=A_s, U_m=U_m, U_s=U_s, mode=mode, sd=c.static_dist, C_gt=C_gt, gt=c.pred)
    i.__dict__.update(over)
    return i


def ref_args(i):
    return (i.C, i.nrm, i.A_m, i.A_s, i.U_m, i.U_s, i.mode, i.sd, i.C_gt, i.gt)


class Device:
    """the inputs of one scene on the device, and the two loss launches on them"""

    def __init__(self, ops, dev, i):
        self.ops, self.dev, self.i = ops, dev, i
        self.k, self.n, self.S = i.C.shape
        self.T = i.gt.shape[1]
        self.t = {name: _d(getattr(i, name), dev) for name in ("C", "nrm", "A_m", "A_s", "U_m", "U_s", "C_gt", "gt")}

    def fwd(self):
        t, dev = self.t, self.dev
        self.recon = _nan((self.S, self.n, self.T, 2), dev)
        self.best, self.losses = _nan((3, self.n), dev), _nan((3,), dev)
        self.arg = torch.full((3, self.n), -1, device=dev, dtype=torch.int32)
        rc = self.ops.L.lib().et_wrapper_losses_fwd(
            _p(t["C"]), self.n, self.S, self.k, self.T, _p(t["nrm"]), _p(t["A_m"]), _p(t["A_s"]), _p(t["U_m"]), _p(t["U_s"]),
            self.i.mode, self.i.sd, _p(t["C_gt"]), _p(t["gt"]), self.recon.data_ptr(), self.best.data_ptr(), self.arg.data_ptr(),
            self.losses.data_ptr(), self.ops.L.raw_stream(dev.index))
        assert rc == 0
        torch.cuda.synchronize()
        return self

    def bwd(self, weights):
        """-> dC written into a buffer that held NaN everywhere; weights: three floats or None (NULL)"""
        t, dev = self.t, self.dev
        g = [None if w is None else torch.tensor(float(w), device=dev) for w in weights]
        dC = _nan((self.k, self.n, self.S), dev)
        rc = self.ops.L.lib().et_wrapper_losses_bwd(
            *map(_p, g), _p(t["C"]), self.n, self.S, self.k, self.T, _p(t["nrm"]), _p(t["A_m"]), _p(t["A_s"]), _p(t["U_m"]),
            _p(t["U_s"]), self.i.mode, self.i.sd, _p(t["C_gt"]), _p(t["gt"]), self.recon.data_ptr(), self.arg.data_ptr(),
            dC.data_ptr(), self.ops.L.raw_stream(dev.index))
        assert rc == 0
        torch.cuda.synchronize()
        return dC


# ------------------------------------------------------------------------------------------------ comparing
def within(name, got, ref, n=0, M=0.0, factor=1.0, rows=None, bound=None):
    """|got - ref| <= (n + 8) * 2**-24 * M * factor (or a bound worked out by the caller) element-wise; prints the
    largest err / bound (pytest -s shows it)"""
    got = N_(got).astype(np.float64) if torch.is_tensor(got) else np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    if bound is None:
        bound = (n + 8) * R.U32 * np.asarray(M, np.float64) * factor
    if rows is not None:
        got, ref, bound = got[rows], ref[rows], np.broadcast_to(bound, ref.shape)[rows]
    assert np.isfinite(got).all(), f"{name}: elements that are not finite (or were never written)"
    err = np.abs(got - ref)
    bound = np.broadcast_to(bound, err.shape)
    ratio = float(np.max(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300)))) if err.size else 0.0
    print(f"RATIO {name} {ratio:.3f} largest |err| {float(err.max()) if err.size else 0.0:.2e}")
    assert ratio <= 1.0, f"{name}: err / bound = {ratio:.3f} at {np.unravel_index(np.argmax(err / np.maximum(bound, 1e-300)), err.shape)}"
    return ratio


def check_forward(name, d, skip_rows=()):
    """recon, best, arg and the three means of a forward launch against the reference -> (reference at the kernel's arg,
    kernel's arg).  arg: exact on decided row-terms; on undecided ones one of the samples within tau of the minimum, and
    the reference is then read at that sample.  skip_rows: rows that hold NaN on purpose (checked by the caller)."""
    i = d.i
    free = R.losses(*ref_args(i))
    karg = N_(d.arg).astype(np.int64)
    assert ((karg >= 0) & (karg < d.S)).all()
    keep = np.ones(d.n, bool)
    keep[list(skip_rows)] = False
    und = R.undecided(free.gap, free.best).numpy()
    exact = ~und & keep[None]
    assert np.array_equal(karg[exact], free.arg.numpy()[exact]), "arg differs on a decided row-term"
    at = np.take_along_axis(free.vals.numpy(), karg[..., None], axis=-1)[..., 0]
    b = free.best.numpy()
    loose = und & keep[None]
    assert (at[loose] - b[loose] <= R.TAU * np.maximum(1.0, b[loose])).all(), "arg outside the margin of the minimum"
    print(f"UNDECIDED {name} {int(loose.sum())} of {3 * int(keep.sum())}")
    ref = R.losses(*ref_args(i), arg=karg)
    within(f"{name}.recon", d.recon, ref.recon, ref.n_recon, ref.M_recon, rows=(slice(None), keep))
    bounds = []
    for t, term in enumerate(R.TERMS):
        within(f"{name}.best_{term}", d.best[t], ref.best[t], ref.n_best[t], ref.M_best[t], rows=keep)
        bounds.append((ref.n_best[t] + 8) * R.U32 * ref.M_best[t].numpy())
    if keep.all():  # the means: positive summands in a fixed-order tree on top of the rows' own bounds
        means, got = ref.means.numpy(), N_(d.losses).astype(np.float64)
        tol = np.array([bb.mean() for bb in bounds]) + (math.ceil(d.n / 256) + 12) * R.U32 * np.abs(means)
        ratio = float(np.max(np.abs(got - means) / tol))
        print(f"RATIO {name}.means {ratio:.3f}")
        assert ratio <= 1.0, (got, means)
    return ref, karg


def check_backward(name, d, karg, weights, skip_rows=()):
    g = R.grad(*ref_args(d.i), weights=weights, arg=karg)
    dC = d.bwd(weights)
    keep = np.ones(d.n, bool)
    keep[list(skip_rows)] = False
    factor = (1.0 + g.rel.numpy())[None, :, None]
    within(f"{name}.dC", dC, g.dC, g.n, g.M, factor=np.broadcast_to(factor, g.dC.shape), rows=(slice(None), keep))
    return dC, g


# ------------------------------------------------------------------------------------------------ projection
def check_project(name, ops, dev, c, mode):
    ref = R.project_train(c.obs, c.pred, *R.u_for(c, mode, obs=True), *R.u_for(c, mode), mode, c.static_dist)
    for want_flag in (True, False):
        out = call_project(ops, dev, c, mode, want_flag)
        if want_flag:
            assert np.array_equal(N_(out.flag), ref.flag)          # exact: no row is within 0.1 of the decision
        assert np.array_equal(N_(out.nrm), ref.nrm32)                # last point and an fp32 difference: exact
        within(f"{name}.C_obs", out.C_obs, ref.C_obs, 2 * c.t_obs, ref.M_C_obs)
        within(f"{name}.C_gt", out.C_gt, ref.C_gt, 2 * c.t_pred, ref.M_C_gt)
        within(f"{name}.obs_ori", out.obs_ori, ref.obs_ori, math.ceil(c.n / 256) + 12, ref.M_obs_ori)


@pytest.mark.parametrize("shape", R.SHAPES, **IDS)
def test_project_train_shapes(ops, dev, shape):
    """Every row count around the wavefront and workgroup sizes, the small / odd / largest (k, T_obs, T_pred), and
    ET_SCENE_MAX_N rows, in ET_MODE_SPLIT, with and without `flag`."""
    check_project("project[%s]" % "-".join(map(str, shape)), ops, dev, R.make_case(*shape), 2)


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_project_train_modes(ops, dev, mode):
    """static, moving, split and identity; the descriptor a mode does not use is passed as NULL"""
    check_project(f"project[mode{mode}]", ops, dev, R.mode_case(min(mode, 2)), mode)


# ------------------------------------------------------------------------------------------------ losses
@pytest.mark.parametrize("shape", R.SHAPES, **IDS)
def test_losses_forward_backward_shapes(ops, dev, shape):
    """forward + backward (all three terms, unequal weights, dC pre-filled with NaN) over the same matrix of shapes"""
    name = "losses[%s]" % "-".join(map(str, shape))
    d = Device(ops, dev, inputs(R.make_case(*shape), 2)).fwd()
    _, karg = check_forward(name, d)
    check_backward(name, d, karg, WEIGHTS)


@pytest.mark.parametrize("anchors", [True, False], ids=["anchors", "bare"])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_losses_modes(ops, dev, mode, anchors):
    """modes 0, 1, 2 with the unused descriptor's U and A as NULL, and A_m = A_s = NULL (bare coefficients)"""
    name = f"losses[mode{mode}-{'anchors' if anchors else 'bare'}]"
    d = Device(ops, dev, inputs(R.mode_case(mode), mode, anchors)).fwd()
    _, karg = check_forward(name, d)
    check_backward(name, d, karg, WEIGHTS)


def test_backward_weight_subsets(ops, dev):
    """all 7 non-empty subsets of {g_e, g_ade, g_fde} (the others NULL), and all three NULL: dC exactly 0 everywhere"""
    d = Device(ops, dev, inputs(R.make_case(257, *R.BASE), 2)).fwd()
    _, karg = check_forward("subsets", d)
    for mask in range(1, 8):
        w = tuple(WEIGHTS[t] if mask >> t & 1 else None for t in range(3))
        check_backward(f"subsets[{mask:03b}]", d, karg, w)
    dC = d.bwd((None, None, None))
    assert bool((dC == 0).all())


# ------------------------------------------------------------------------------------------------ edge cases
def _wrapper_grads(dev, i, weights):
    """the same scene through EigenTrajectory.forward (fused) and ._forward_composite (general kernels + torch autograd)
    with a predictor that returns C -> d(sum_t w_t loss_t)/dC of the two forms, and the wrapper's own C_gt"""
    from eigentrajectory_amd import EigenTrajectory
    from eigentrajectory_amd.utils import DotDict, default_hyper_params

    class Const(torch.nn.Module):
        def __init__(self, C):
            super().__init__()
            self.C = torch.nn.Parameter(C)

        def forward(self, x):
            return self.C

    hooks = DotDict(model_forward_pre_hook=lambda c, o, a=None: (c, o), model_forward=lambda x, m: m(x),
                    model_forward_post_hook=lambda y, a=None: y)
    model = EigenTrajectory(Const(torch.from_numpy(i.C.copy())), hooks, default_hyper_params(static_dist=i.sd))
    sd = model.state_dict()
    for key, v in (("ET_m_descriptor.U_obs_trunc", i.U_obs_m), ("ET_s_descriptor.U_obs_trunc", i.U_obs_s),
                   ("ET_m_descriptor.U_pred_trunc", i.U_m), ("ET_s_descriptor.U_pred_trunc", i.U_s),
                   ("ET_m_anchor.C_anchor", i.A_m), ("ET_s_anchor.C_anchor", i.A_s)):
        sd[key] = torch.from_numpy(np.ascontiguousarray(v))
    model.load_state_dict(sd)
    model = model.to(dev)
    obs, gt = T(i.obs, dev), T(i.gt, dev)
    grads = []
    for fn in (model, model._forward_composite):
        model.zero_grad(set_to_none=True)
        out = fn(obs, gt)
        sum(w * out[key] for w, key in zip(weights, ("loss_eigentraj", "loss_euclidean_ade", "loss_euclidean_fde"))).backward()
        grads.append(N_(model.baseline_model.C.grad).astype(np.float64))
    return grads[0], grads[1], N_(model._scene_project_train(obs, gt)[3]).copy()


def _check_wrapper_ties(tag, dev, i, w, tied, karg):
    """The tie scene through the fused and the composite wrapper call under the loss weights ``w`` (0: term not in use):
    both gradients equal the reference's, and on rows where every term in use ties the copy gets exactly nothing.
    ``tied`` (3,N): the row-terms whose minimum is the duplicated sample; ``karg``: the loss kernel's arg."""
    lo, hi = R.tie_pairs(i.C.shape[1])
    rows = np.arange(i.C.shape[1])
    used = np.array([x != 0.0 for x in w])
    # 1. Both forms project the ground truth themselves, so the reference takes the wrapper's own C_gt (the fused
    #    form's; the composite form's comes from another kernel and may differ in the last bit, far inside the bound
    #    of dC).  The duplicated samples are bit for bit the same whatever C_gt is: the ties stay where they were.
    fused, composite, i.C_gt = _wrapper_grads(dev, i, w)
    mine = R.losses(*ref_args(i))
    assert np.array_equal(mine.arg.numpy() == lo[None], tied)
    # 2. The samples the reference reads: the lower index on a tie, its own arg-min for the coefficient term, the
    #    loss kernel's choice for the two displacement terms (recon does not depend on C_gt).
    arg = np.where(tied, lo[None], mine.arg.numpy())
    arg[1:] = karg[1:]
    g = R.grad(*ref_args(i), weights=tuple(x if x != 0.0 else None for x in w), arg=arg)
    factor = np.broadcast_to((1.0 + g.rel.numpy())[None, :, None], g.dC.shape)
    # 3. Rows to compare: a row-term in use that is undecided without being a tie is left out (torch's arg-min on the
    #    composite form's own fp32 values may settle it the other way).  Rows where every term in use ties: `sure`.
    settled = ~((R.undecided(mine.gap, mine.best).numpy() & ~tied)[used]).any(axis=0)
    sure = tied[used].all(axis=0)
    assert sure.sum() >= 10
    for name, got in (("fused", fused), ("composite", composite)):
        within(f"ties.{name}{tag}", got, g.dC, g.n, g.M, factor=factor, rows=(slice(None), settled))
        assert (got[:, rows[sure], hi[sure]] == 0).all(), name       # nothing split off to the copy
        assert (np.abs(got[:, rows[sure], lo[sure]]).sum(axis=0) > 0).all(), name


def test_exact_ties_send_the_gradient_to_the_lower_index(ops, dev):
    """A duplicated sample (the first one for even rows, a later pair for odd rows) that is the minimum of most rows: arg
    is the lower index for all three terms, the copy gets exactly no gradient, dC equals the reference's -- through the
    kernels, through the fused wrapper call and through the composite one (.min(dim)[0] like the reference, not amin,
    which would hand half of every tied term's gradient to the copy)."""
    c = R.make_case(70, *R.BASE)
    C, A_m, A_s = R.tie_inputs(c)
    i = inputs(c, 2, C=C, A_m=A_m, A_s=A_s)
    d = Device(ops, dev, i).fwd()
    free = R.losses(*ref_args(i))
    lo, hi = R.tie_pairs(c.n)
    karg, rarg = N_(d.arg).astype(np.int64), free.arg.numpy()
    tied = rarg == lo[None]
    odd = (np.arange(c.n) % 2 == 1)[None]
    assert tied.sum(axis=1).min() >= 10 and (tied & odd).sum(axis=1).min() >= 5   # every term, both kinds of pair
    assert np.array_equal(karg[tied], rarg[tied]) and not (karg == hi[None]).any()
    ref, karg = check_forward("ties", d)                       # (a tied row-term counts as undecided there: gap 0)
    rows = np.arange(c.n)
    for t in range(3):
        w = tuple(WEIGHTS[j] if j == t else None for j in range(3))
        dC, g = check_backward(f"ties[{R.TERMS[t]}]", d, karg, w)
        dC = N_(dC)
        assert (dC[:, rows[tied[t]], hi[tied[t]]] == 0).all()
        assert (np.abs(dC[:, rows[tied[t]], lo[tied[t]]]).sum(axis=0) > 0).all()
    # the wrapper's two forms on the same scene, term by term and all three together
    i.obs, i.U_obs_m, i.U_obs_s = c.obs, c.U_obs_m, c.U_obs_s
    for t, w in enumerate([(WEIGHTS[0], 0.0, 0.0), (0.0, WEIGHTS[1], 0.0), (0.0, 0.0, WEIGHTS[2]), WEIGHTS]):
        _check_wrapper_ties(f"[{t}]", dev, i, w, tied, karg)


def test_zero_distance_gives_zero_finite_gradient(ops, dev):
    """One row whose sample 3 has A + C == C_gt bit for bit, one whose recon[5, n, T-1] == gt[n, T-1] bit for bit:
    best is 0 there, dC is finite and that term contributes nothing."""
    c, C, A_m, A_s, C_gt, nrm, gt, U_m, U_s, (n_e, n_f) = R.zero_distance_inputs()
    i = NS(C=C, nrm=nrm, A_m=A_m, A_s=A_s, U_m=U_m, U_s=U_s, mode=2, sd=c.static_dist, C_gt=C_gt, gt=gt)
    d = Device(ops, dev, i).fwd()
    ref, karg = check_forward("zero", d)
    best = N_(d.best)
    assert best[0, n_e] == 0.0 and karg[0, n_e] == 3 and best[2, n_f] == 0.0 and karg[2, n_f] == 5
    assert np.array_equal(N_(d.recon)[5, n_f, -1], gt[n_f, -1])
    for t, n in ((0, n_e), (2, n_f)):
        w = tuple(WEIGHTS[j] if j == t else None for j in range(3))
        dC, _ = check_backward(f"zero[{R.TERMS[t]}]", d, karg, w)
        assert bool(torch.isfinite(dC).all()) and bool((dC[:, n] == 0).all())
    check_backward("zero[all]", d, karg, WEIGHTS)


def test_nan_rows_poison_their_own_gradient_only(ops, dev):
    """mode 1 with a motionless row (its projected ground truth is not finite) and a row with a NaN coefficient: the
    three means are NaN, arg of the NaN row is its first NaN sample, every other row is bit for bit what it is without
    them, and the two rows' dC is NaN at their selected samples, as the reference's autograd gives it."""
    c = R.nan_case()
    clean = inputs(c, 1)
    C, nrm, C_gt, (still, nanc) = R.nan_inputs(c)
    dirty = inputs(c, 1, C=C, nrm=nrm, C_gt=C_gt)
    d0 = Device(ops, dev, clean).fwd()
    d = Device(ops, dev, dirty).fwd()
    assert bool(torch.isnan(d.losses).all())
    _, karg = check_forward("nan", d, skip_rows=(still, nanc))
    assert (karg[:, nanc] == 4).all() and karg[0, still] == 0
    assert bool(torch.isnan(d.best[:, nanc]).all()) and bool(torch.isnan(d.best[0, still]))
    keep = np.ones(c.n, bool)
    keep[[still, nanc]] = False
    for a, b in ((d.best, d0.best), (d.arg, d0.arg)):
        assert np.array_equal(N_(a)[:, keep], N_(b)[:, keep])
    assert np.array_equal(N_(d.recon)[:, keep], N_(d0.recon)[:, keep])
    dC, g = check_backward("nan", d, karg, WEIGHTS, skip_rows=(still, nanc))
    dC0 = d0.bwd(WEIGHTS)
    assert np.array_equal(N_(dC)[:, keep], N_(dC0)[:, keep])
    dC = N_(dC)
    assert np.isnan(dC[:, nanc, 4]).all() and np.isnan(dC[:, still, karg[0, still]]).all()
    for t in range(3):   # term by term: NaN at its selected sample where the reference's is, and its value where both are finite
        w = tuple(WEIGHTS[j] if j == t else None for j in range(3))
        got, g = N_(d.bwd(w)), R.grad(*ref_args(dirty), weights=w, arg=karg)
        ref = g.dC.numpy()
        assert np.isnan(got[:, nanc, 4]).all()
        for n in (still, nanc):
            s = karg[t, n]
            assert np.array_equal(np.isnan(got[:, n, s]), np.isnan(ref[:, n, s])), (n, t)
        if t:  # the motionless row's displacement terms are finite on both sides (1 / sca = 0 shrinks them to 0)
            assert np.isfinite(ref[:, still]).all()
            within(f"nan.still[{R.TERMS[t]}]", got[:, still], ref[:, still], g.n, g.M.numpy()[:, still],
                   factor=1.0 + float(g.rel[still]))


def test_autograd_wiring_through_the_wrapper(ops, dev):
    """EigenTrajectory.forward at N = 300 with a predictor that has parameters, one loss used (the other two reach
    _SceneLosses.backward as None) and recon_traj differentiated too (its g_recon branch): the parameter gradients
    against the reference's dC pushed through the predictor in float64."""
    from eigentrajectory_amd import EigenTrajectory
    from eigentrajectory_amd.utils import DotDict, default_hyper_params
    c = R.make_case(300, *R.BASE)

    class Net(torch.nn.Module):  # (k+2, N) -> (k, N, S), the predictor of test_scene_training_form_fused_equals_composite
        def __init__(self):
            super().__init__()
            torch.manual_seed(5)
            self.w = torch.nn.Parameter(torch.randn(6, 8, 20) * 0.3)
            self.b = torch.nn.Parameter(torch.randn(6, 1, 20) * 0.5)

        def forward(self, x):
            self.x = x.detach()
            self.out = torch.einsum("jis,in->jns", self.w, x) + self.b
            return self.out

    hooks = DotDict(model_forward_pre_hook=lambda co, o, a=None: torch.cat([co, o], dim=0),
                    model_forward=lambda x, m: m(x), model_forward_post_hook=lambda y, a=None: y)
    model = EigenTrajectory(Net(), hooks, default_hyper_params(static_dist=c.static_dist))
    sd = model.state_dict()
    for key, v in (("ET_m_descriptor.U_obs_trunc", c.U_obs_m), ("ET_s_descriptor.U_obs_trunc", c.U_obs_s),
                   ("ET_m_descriptor.U_pred_trunc", c.U_pred_m), ("ET_s_descriptor.U_pred_trunc", c.U_pred_s),
                   ("ET_m_anchor.C_anchor", c.A_m), ("ET_s_anchor.C_anchor", c.A_s)):
        sd[key] = torch.from_numpy(v)
    model.load_state_dict(sd)
    model = model.to(dev)
    G = np.random.default_rng(9).standard_normal((c.S, c.n, c.t_pred, 2)).astype(np.float32) * 1e-3
    out = model(T(c.obs, dev), T(c.pred, dev))
    assert out["loss_euclidean_ade"].grad_fn is not None and type(out["loss_euclidean_ade"].grad_fn).__name__.startswith("_SceneLosses")
    (WEIGHTS[1] * out["loss_euclidean_ade"] + (out["recon_traj"] * T(G, dev)).sum()).backward()
    net = model.baseline_model
    C32, x = N_(net.out), N_(net.x).astype(np.float64)
    nrm, C_gt = R.loss_inputs(c, 2)
    i = NS(C=C32, nrm=nrm, A_m=c.A_m, A_s=c.A_s, U_m=c.U_pred_m, U_s=c.U_pred_s, mode=2, sd=c.static_dist, C_gt=C_gt, gt=c.pred)
    free = R.losses(*ref_args(i))
    # the wrapper does not hand out arg: read the ADE's choice off its fp32 recon_traj; it must be the reference's on
    # every decided row, and is taken as it is on an undecided one
    und = R.undecided(free.gap, free.best)[1].numpy()
    rec = N_(out["recon_traj"]).astype(np.float64)
    karg = free.arg.numpy().copy()
    picked = np.linalg.norm(rec - c.pred[None].astype(np.float64), axis=-1).mean(axis=-1).argmin(axis=0)
    assert np.array_equal(picked[~und], karg[1][~und])
    karg[1] = picked
    within("wiring.recon", rec, free.recon, free.n_recon, free.M_recon)
    within("wiring.ade", float(out["loss_euclidean_ade"].detach()), float(R.losses(*ref_args(i), arg=karg).means[1]), free.n_best[1] + math.ceil(c.n / 256) + 12,
           float(free.M_best[1].mean()))
    g = R.grad(*ref_args(i), weights=(None, WEIGHTS[1], None), g_recon=G, arg=karg)
    dC, bound = g.dC.numpy(), (g.n + 8) * R.U32 * g.M.numpy() * (1.0 + g.rel.numpy())[None, :, None]
    ax = np.abs(x)
    # dw[j,i,s] = sum_n dC[j,n,s] x[i,n]; db[j,0,s] = sum_n dC[j,n,s]: the rows' own bounds, plus an N-term fp32 sum
    dw, db = np.einsum("jns,in->jis", dC, x), dC.sum(axis=1, keepdims=True)
    tw = np.einsum("jns,in->jis", bound, ax) + (c.n + 8) * R.U32 * np.einsum("jns,in->jis", np.abs(dC), ax)
    tb = bound.sum(axis=1, keepdims=True) + (c.n + 8) * R.U32 * np.abs(dC).sum(axis=1, keepdims=True)
    within("wiring.dw", net.w.grad, dw, bound=tw)
    within("wiring.db", net.b.grad, db, bound=tb)
