"""CPU checks of the curve-fitting baselines (CurveModel/, script/descriptor_evaluation.py:38-85): the bases of
eigentrajectory_amd.curve and the numpy restatement of csrc/et_curve.hip (tests/_curve_fit_np.py) against the reference's
own outputs (tests/golden/g17_curve_fit.npz, tools/make_golden_curves.py), the C ABI's host-side argument checks, and the
script's --curves arguments."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from . import _golden as G
from ._curve_fit_np import curve_fit_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = G.load("g17_curve_fit.npz")


def _name(kind, prm):
    return "linear" if kind == "linear" else (f"bezier{prm[0]}" if kind == "bezier" else f"bspline_c{prm[0]}_d{prm[1]}")


def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("T", [3, 5, 8, 12, 20])
def test_bases_match_the_reference(T):
    """Linear and B-spline bases are bit-equal to the reference's; the Bezier bases are within 4 ulp (2.5e-7), the
    reference's binomials coming from lgamma / exp in fp32 where ours are exact."""
    from eigentrajectory_amd import curve
    bases = curve.table_bases(T)
    assert [(k, p) for k, p, _ in bases] == [("linear", ())] + [("bezier", (d,)) for d in range(2, 6)] + [
        ("bspline", (c, d)) for d in range(1, 4) for c in range(2, 6) if c > d]
    for kind, prm, b in bases:
        ref, got = Z[f"a.T{T}.{_name(kind, prm)}"], b.numpy()
        assert got.dtype == np.float32 and got.shape == ref.shape
        if kind == "bezier":
            assert _ulps(got, ref).max() <= 4 and np.abs(got - ref).max() <= 2.5e-7
        else:
            assert np.array_equal(got, ref), (kind, prm)


def test_bspline_last_row_and_signatures():
    from eigentrajectory_amd import curve
    b = curve.bspline_basis(cpoint=4, degree=2, step=12).numpy()
    assert b.shape == (12, 5) and np.array_equal(b[-1], [0, 0, 0, 0, 1]) and np.array_equal(b[0], [1, 0, 0, 0, 0])
    assert curve.bezier_basis(degree=3, step=13).shape == (13, 4)
    assert curve.linear_basis(8).shape == (8, 2)
    np.testing.assert_allclose(curve.bspline_basis(4, 2, 12).numpy().sum(1), 1.0, rtol=0, atol=1e-6)


@pytest.mark.parametrize("part", ["obs", "pred"])
def test_restatement_against_the_reference_short_runs(part):
    """The restatement against the reference's own curve_fitting cut to 1 and 10 steps, every basis: at 1 step within
    4e-6 (2x the reference's 1-ulp spread); at 10 steps median within 1e-6 and maximum within 2e-3 (Adam steps are
    ~lr sign(g), so a gradient sign decided by rounding moves a point by 1e-4 a step)."""
    from eigentrajectory_amd import curve
    traj = Z[f"in.{part}"]
    for kind, prm, b in curve.table_bases(traj.shape[1]):
        for steps in (1, 10):
            got = curve_fit_np(traj, b.numpy(), steps)
            ref = Z[f"b.s{steps}.{part}.{_name(kind, prm)}"]
            d = np.abs(got["recon"] - ref)
            if steps == 1:
                assert got["best"] == 0 and d.max() <= 4e-6, (kind, prm, d.max())
            else:
                assert np.median(d) <= 1e-6 and d.max() <= 2e-3, (kind, prm, np.median(d), d.max())


def test_restatement_best_step_rule():
    """The loss is a fixed-point sum; the recon returned is that of the FIRST step of minimum loss, and the loss curve
    is that sum over N T."""
    rng = np.random.default_rng(3)
    traj = np.cumsum(rng.normal(0, 0.3, (40, 8, 2)), axis=1).astype(np.float32)
    from eigentrajectory_amd import curve
    r = curve_fit_np(traj, curve.bezier_basis(3, 8).numpy(), 50)
    assert r["best"] == int(np.argmin(r["fixed"])) and r["fixed"][r["best"]] < r["fixed"][:r["best"]].min(initial=2 ** 62)
    nn = np.linalg.norm(r["recon"].astype(np.float64) - traj, axis=-1).mean()
    assert abs(nn - r["loss"][r["best"]]) < 1e-6


def test_abi_rejects_bad_arguments_on_the_host():
    """et_curve_fit_batch validates everything before it touches the device; the two symbols are exported."""
    from eigentrajectory_amd import _lib
    assert {"et_curve_fit_batch", "et_curve_fit_batch_workspace_bytes"} <= set(_lib.SYMBOLS)
    lib = _lib.lib()
    ws = lib.et_curve_fit_batch_workspace_bytes
    assert ws(28, 100000) >= 28 * 100000 * 8
    assert ws(0, 10) == 0 and ws(65, 10) == 0 and ws(1, 0) == 0 and ws(1, 2 ** 31) == 0
    fake = C.c_void_p(4096)  # never dereferenced: every case fails validation first

    def call(rows, n_fits=None, steps=10, lr=1e-4, b1=0.9, b2=0.999, traj=fake, recon=fake, wsb=1 << 30):
        rows = [list(r) for r in rows]
        tab = (C.c_int64 * max(1, 6 * len(rows)))(*[v for r in rows for v in r])
        return lib.et_curve_fit_batch(traj, fake, tab, len(rows) if n_fits is None else n_fits, C.c_int64(steps),
                                      C.c_double(lr), C.c_double(b1), C.c_double(b2), C.c_double(1e-8), recon, None,
                                      None, None, None, C.c_size_t(wsb), None)

    good = (10, 8, 4, 0, 0, 0)
    for rows, kw in [([good], dict(traj=None)), ([good], dict(recon=None)), ([good], dict(n_fits=0)),
                     ([good] * 65, {}), ([good], dict(steps=0)), ([good], dict(lr=0.0)), ([good], dict(b1=1.0)),
                     ([(0, 8, 4, 0, 0, 0)], {}), ([(10, 1, 4, 0, 0, 0)], {}), ([(10, 33, 4, 0, 0, 0)], {}),
                     ([(10, 8, 1, 0, 0, 0)], {}), ([(10, 8, 9, 0, 0, 0)], {}), ([(10, 8, 4, -1, 0, 0)], {})]:
        assert call(rows, **kw) == 1, (rows[0], kw)
    assert call([good]) == 4  # no workspace given: ET_ERR_WORKSPACE


def _script():
    spec = importlib.util.spec_from_file_location("descriptor_evaluation", os.path.join(ROOT, "scripts",
                                                                                         "descriptor_evaluation.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_script_curve_arguments():
    m = _script()
    a = m.parse_args([])
    assert not a.curves and a.steps == 100000
    a = m.parse_args(["--curves", "--steps", "200"])
    assert a.curves and a.steps == 200
    with pytest.raises(SystemExit):
        m.parse_args(["--curves", "--steps", "0"])
    assert callable(m.curve_table) and callable(m.svd_table)
