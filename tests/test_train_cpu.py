"""CPU-side checks of the scene training kernels' yardstick (tests/_train_np.py): the float64 reference against the
numpy oracle of the wrapper and against finite differences, its tie / zero-distance / NaN semantics (the reference's
``.min(dim)[0]`` and norm gradients), the conditions on the seeded inputs that tests/test_gpu_train.py relies on, and the
host-side argument validation of the three entry points of csrc/et_train.hip.  Nothing here launches a kernel."""
import ctypes

import numpy as np
import pytest
import torch

from . import _golden as G
from . import _train_np as R
from ._gpu_common import FP

needs_no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="asserts the behaviour on a box without a GPU")

MODES = (0, 1, 2)


def _grad_args(c, mode, anchors=True, C=None):
    nrm, C_gt = R.loss_inputs(c, mode)
    return (c.C if C is None else C, nrm, *R.a_for(c, mode, anchors), *R.u_for(c, mode), mode, c.static_dist, C_gt, c.pred)


# ------------------------------------------------------------------------------------------------ the reference, pinned
@pytest.mark.parametrize("scene", ["eth", "univ"])
def test_reference_matches_the_wrapper_oracle(oracle, scene):
    """Projection, reconstruction and the three losses of one test scene through the G6 linear stub: the float64
    restatement against oracle.wrapper_ref.forward (fp32 numpy on the C oracle, itself pinned to the reference's G6)."""
    from oracle import wrapper_ref as W
    g2 = G.load("g2_fit_all_scenes.npz")
    p = {key[len(scene) + 1:]: g2[key] for key in g2.files if key.startswith(scene + ".ET_")}
    predictor = W.linear_stub(G.load("g6_wrapper_stub_predictors.npz")["linear_stub_w"])
    obs, pred, sse = G.dataset(scene, "test")
    sd = G.static_dist(scene)
    s, e = max(sse, key=lambda se: se[1] - se[0]) if scene == "eth" else sse[0]
    obs, pred = obs[s:e], pred[s:e]
    out = W.forward(p, obs, pred, predictor, sd)
    U = [p[f"ET_{d}_descriptor.U_{w}_trunc"] for w in ("obs", "pred") for d in ("m", "s")]
    pr = R.project_train(obs, pred, *U, 2, sd)
    np.testing.assert_allclose(pr.C_obs.numpy(), out["C_obs"], **FP)
    np.testing.assert_allclose(pr.obs_ori.numpy(), out["obs_ori"], **FP)
    assert np.array_equal(pr.flag.astype(bool), oracle.moving_flags(obs, sd))
    c_refine = predictor(np.concatenate([out["C_obs"], out["obs_ori"]], axis=0))
    ls = R.losses(c_refine, pr.nrm32, p["ET_m_anchor.C_anchor"], p["ET_s_anchor.C_anchor"], U[2], U[3], 2, sd, pr.C_gt, pred)
    np.testing.assert_allclose(ls.recon.numpy(), out["recon_traj"], **FP)
    ref = [out["loss_eigentraj"], out["loss_euclidean_ade"], out["loss_euclidean_fde"]]
    np.testing.assert_allclose(ls.means.numpy(), ref, **FP)


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_grad_matches_central_differences(shape):
    """The autograd gradient at every shape of the GPU matrix against central differences (step 1e-6, rtol 1e-6) of
    sum_i w_i * best_i[n] / N, on decided rows: at the three selected samples and at one that no term selects."""
    c = R.make_case(*shape)
    weights = (0.3, 1.7, -2.0)
    args = _grad_args(c, 2)
    ls, g = R.losses(*args), R.grad(*args, weights=weights)
    decided = (~(ls.gap < 1e-3 * torch.clamp(ls.best, min=1.0)).any(dim=0)).nonzero()[:, 0].tolist()
    assert decided
    rng = np.random.default_rng(3)
    rows = [decided[i] for i in rng.choice(len(decided), size=min(4, len(decided)), replace=False)]
    nrm, C_gt = args[1], args[8]
    h, checked = 1e-6, 0
    for n in rows:
        sub = (nrm[:, n:n + 1], *args[2:8], C_gt[:, n:n + 1], c.pred[n:n + 1])

        def f(Cn):
            return float(sum(w * b for w, b in zip(weights, R.losses(Cn, *sub).best[:, 0]))) / c.n

        samples = sorted(set(ls.arg[:, n].tolist()) | {int(rng.integers(c.S))})
        for s in samples:
            for j in sorted({0, c.k - 1, int(rng.integers(c.k))}):
                Cn = torch.from_numpy(c.C[:, n:n + 1]).double()
                up, dn = Cn.clone(), Cn.clone()
                up[j, 0, s] += h
                dn[j, 0, s] -= h
                fd = (f(up) - f(dn)) / (2 * h)
                got = float(g.dC[j, n, s])
                assert abs(got - fd) <= 1e-6 * max(abs(fd), abs(got)) + 1e-9 / c.n, (n, j, s, got, fd)
                checked += 1
    assert checked >= 3


# ------------------------------------------------------------------------------------------------ semantics
def test_exact_tie_sends_the_whole_gradient_to_the_lower_index():
    c = R.make_case(70, *R.BASE)
    C, A_m, A_s = R.tie_inputs(c)
    args = list(_grad_args(c, 2, C=C))
    args[2], args[3] = A_m, A_s
    ls = R.losses(*args)
    lo, hi = R.tie_pairs(c.n)
    for i in range(3):
        g = R.grad(*args, weights=tuple(1.0 if j == i else None for j in range(3)))
        tied = (ls.arg[i] == torch.from_numpy(lo))          # rows whose minimum of term i is the duplicated sample
        assert tied.sum() >= 2 and not (ls.arg[i] == torch.from_numpy(hi)).any()
        rows = tied.nonzero()[:, 0]
        assert (g.dC[:, rows, torch.from_numpy(hi)[rows]] == 0).all()           # nothing is split off to the copy
        assert (g.dC[:, rows, torch.from_numpy(lo)[rows]].abs().sum(dim=0) > 0).all()


def test_exactly_hit_target_has_a_zero_finite_gradient():
    c, C, A_m, A_s, C_gt, nrm, gt, U_m, U_s, rows = R.zero_distance_inputs()
    args = (C, nrm, A_m, A_s, U_m, U_s, 2, c.static_dist, C_gt, gt)
    ls = R.losses(*args)
    n_e, n_f = rows
    assert float(ls.best[0, n_e]) == 0.0 and int(ls.arg[0, n_e]) == 3
    assert float(ls.best[2, n_f]) == 0.0 and int(ls.arg[2, n_f]) == 5
    g_e = R.grad(*args, weights=(1.0, None, None)).dC
    g_f = R.grad(*args, weights=(None, None, 1.0)).dC
    assert torch.isfinite(g_e).all() and torch.isfinite(g_f).all()
    assert (g_e[:, n_e] == 0).all() and (g_f[:, n_f] == 0).all()


def test_nan_rows_poison_their_own_gradient_only():
    c = R.nan_case()
    clean = _grad_args(c, 1)
    C, nrm, C_gt, bad = R.nan_inputs(c)
    args = (C, nrm, *clean[2:8], C_gt, c.pred)
    ls, g = R.losses(*args), R.grad(*args)
    ls0, g0 = R.losses(*clean), R.grad(*clean)
    still, nanc = bad
    assert torch.isnan(ls.means).all()
    assert int(ls.arg[0, nanc]) == int(ls.arg[1, nanc]) == int(ls.arg[2, nanc]) == 4          # the first NaN sample
    assert torch.isnan(g.dC[:, nanc, 4]).all() and torch.isnan(g.dC[:, still, ls.arg[0, still]]).all()
    keep = torch.ones(c.n, dtype=torch.bool)
    keep[list(bad)] = False
    assert torch.equal(ls.arg[:, keep], ls0.arg[:, keep]) and torch.equal(ls.best[:, keep], ls0.best[:, keep])
    assert torch.equal(ls.recon[:, keep], ls0.recon[:, keep])
    assert torch.equal(g.dC[:, keep], g0.dC[:, keep])


# ------------------------------------------------------------------------------------------------ input conditions
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_seeded_inputs_keep_hard_decisions_clear(shape):
    """What lets the GPU tests compare `flag` and `arg` exactly: every row is >= 0.1 away from static_dist, at most 1 % of
    the row-terms of a case are undecided (tau = 1e-4), and every selected distance is >= 1e-3 (the bound of dC divides by
    it).  Checked in every mode the case is used in."""
    _check_conditions(R.make_case(*shape), 2, True)
    flags = R.row_state(_grad_args(R.make_case(*shape), 2)[1], 2, R.STATIC_DIST).mv
    if shape[0] >= 63:
        assert 0.3 < float(flags.double().mean()) < 0.7               # about half the rows are moving


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("anchors", [True, False])
def test_seeded_inputs_of_the_mode_cases(mode, anchors):
    _check_conditions(R.mode_case(mode), mode, anchors)


def _check_conditions(c, mode, anchors):
    _check_args(c, _grad_args(c, mode, anchors))


def _check_args(c, args, skip_rows=(), skip_terms=None, zero_ok=False):
    """margin, cap and smallest selected distance of one set of loss inputs; skip_rows: rows that hold NaN on purpose,
    skip_terms (3,N) bool: row-terms that are exact ties on purpose, zero_ok: distances that are exactly 0 on purpose"""
    ls = R.losses(*args)
    keep = torch.ones(c.n, dtype=torch.bool)
    keep[list(skip_rows)] = False
    assert R.row_state(args[1], 2, c.static_dist).margin[keep.numpy()].min() >= 0.1
    und = R.undecided(ls.gap, ls.best) & keep[None]
    if skip_terms is not None:
        und &= ~torch.as_tensor(skip_terms)
    share = float(und.double().sum()) / (3 * int(keep.sum()))
    assert share <= 0.01, share
    rows = torch.arange(c.n)
    sel = torch.cat([ls.best[:, keep].reshape(-1), ls.dist[ls.arg[1], rows][keep].reshape(-1)])  # + every step of the ADE's sample
    if zero_ok:
        sel = sel[sel != 0]
    assert float(sel.min()) >= 1e-3
    return int(und.sum())


def test_inputs_of_the_edge_cases():
    """The same conditions on the modified inputs of the tie, zero-distance and NaN tests, leaving out what they break
    on purpose: the tied row-terms, the two exact zeros, the two NaN rows.  The NaN scene's seed leaves headroom: no
    undecided row-term with or without the NaN rows."""
    c = R.make_case(70, *R.BASE)
    C, A_m, A_s = R.tie_inputs(c)
    args = list(_grad_args(c, 2, C=C))
    args[2], args[3] = A_m, A_s
    lo, _ = R.tie_pairs(c.n)
    assert _check_args(c, args, skip_terms=R.losses(*args).arg.numpy() == lo[None]) <= 1
    c, C, A_m, A_s, C_gt, nrm, gt, U_m, U_s, _ = R.zero_distance_inputs()
    # (row 40's nrm is set by hand to a static row: ||d / 2|| = 0.0625, further than 0.1 from static_dist as well)
    _check_args(c, (C, nrm, A_m, A_s, U_m, U_s, 2, c.static_dist, C_gt, gt), zero_ok=True)
    c = R.nan_case()
    clean = _grad_args(c, 1)
    C, nrm, C_gt, bad = R.nan_inputs(c)
    assert _check_args(c, clean) == 0
    assert _check_args(c, (C, nrm, *clean[2:8], C_gt, c.pred), skip_rows=bad) == 0


# ------------------------------------------------------------------------------------------------ host validation
def _abi():
    from eigentrajectory_amd import _lib
    return _lib, _lib.lib(), ctypes.c_void_p(0)


def test_training_entry_points_validate_arguments_on_the_host():
    """Out-of-range dimensions and modes return ET_ERR_INVALID_ARG before any pointer is looked at or anything is
    launched; an empty scene is a no-op for the projection and an error for the losses (a mean over no rows)."""
    L, lib, null = _abi()
    f = ctypes.c_float(0.4)

    def project(N=5, T_obs=8, T_pred=12, k=6, mode=2):
        return lib.et_scene_project_train(null, null, N, T_obs, T_pred, k, null, null, null, null, mode, f, null, null, null,
                                          null, null, null)

    def fwd(N=5, S=20, k=6, T=12, mode=2):
        return lib.et_wrapper_losses_fwd(null, N, S, k, T, null, null, null, null, null, mode, f, null, null, null, null, null,
                                         null, null)

    def bwd(N=5, S=20, k=6, T=12, mode=2):
        return lib.et_wrapper_losses_bwd(null, null, null, null, N, S, k, T, null, null, null, null, null, mode, f, null, null,
                                         null, null, null, null)

    assert project(N=0) == 0 and fwd(N=0) == 1 and bwd(N=0) == 1
    assert project(N=0, mode=3) == 0 and project(N=0, mode=4) == 1 and project(N=0, mode=-1) == 1
    assert project(N=0, T_obs=2) == 1 and project(N=0, T_obs=3) == 0 and project(N=0, T_obs=33) == 1
    assert project(N=0, T_pred=0) == 1 and project(N=0, T_pred=33) == 1 and project(N=0, k=33) == 1 and project(N=0, k=0) == 1
    assert project(N=-1) == 1 and project(N=L.SCENE_MAX_N + 1) == 1
    assert project() == 1                                    # rows but no tensors
    for call in (fwd, bwd):
        assert call(N=L.SCENE_MAX_N + 1) == 1 and call(N=-1) == 1
        assert call(k=33) == 1 and call(k=0) == 1 and call(T=33) == 1 and call(T=0) == 1 and call(S=0) == 1
        assert call(mode=3) == 1 and call(mode=-1) == 1     # no identity mode for the losses
        assert call() == 1                                   # in range, but no tensors


@needs_no_gpu
def test_losses_bwd_refuses_a_missing_basis_before_the_launch():
    """et_wrapper_losses_bwd without the U_pred of a descriptor its mode uses returns ET_ERR_INVALID_ARG like
    et_wrapper_losses_fwd (the return precedes the launch in csrc/et_train.hip; the pointers are never read)."""
    _, lib, null = _abi()
    fake = ctypes.c_void_p(4096)
    f = ctypes.c_float(0.4)
    for mode, U_m, U_s in ((0, fake, null), (1, null, fake), (2, null, fake), (2, fake, null), (2, null, null)):
        assert lib.et_wrapper_losses_fwd(fake, 5, 20, 6, 12, fake, null, null, U_m, U_s, mode, f, fake, fake, fake, fake, fake,
                                         fake, null) == 1
        assert lib.et_wrapper_losses_bwd(null, null, null, fake, 5, 20, 6, 12, fake, null, null, U_m, U_s, mode, f, fake, fake,
                                         fake, fake, fake, null) == 1
