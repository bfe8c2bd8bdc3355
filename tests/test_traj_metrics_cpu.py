"""CPU pin of the numpy restatement of the reference's TCC / COL (tests/_traj_metrics_np.py) to tests/golden/g16 (a):
the reference's utils/metrics.py run on G9's seeded data and on crafted scenes for each quirk of the metrics."""
import numpy as np
import pytest

from . import _golden as G
from . import _traj_metrics_np as R

Z = G.load("g16_tcc_col.npz")
CASES = [str(c) for c in Z["cases"]]


@pytest.mark.parametrize("case", CASES)
def test_restatement_matches_reference_g16a(case):
    pred, gt = Z[f"a.{case}.pred"], Z[f"a.{case}.gt"]
    m = R.metrics(pred, gt)
    ref_tcc, noise = Z[f"a.{case}.tcc"], Z[f"a.{case}.noise"]
    assert np.array_equal(m["col_bits"], Z[f"a.{case}.col_bits"].astype(bool))
    assert np.array_equal(m["COL"], Z[f"a.{case}.col"])
    np.testing.assert_allclose(m["TCC"][~noise], ref_tcc[~noise], rtol=0, atol=1e-6)
    assert np.all(m["TCC"][ref_tcc == 0] == 0)  # the 0/0 rows of a motionless coordinate: exactly 0
    assert np.array_equal(m["best"], Z[f"a.{case}.best"])
    np.testing.assert_allclose(m["ADE"], Z[f"a.{case}.ade"], rtol=1e-6, atol=0)
    np.testing.assert_allclose(m["FDE"], Z[f"a.{case}.fde"], rtol=1e-6, atol=0)
    finite = np.isfinite(Z[f"a.{case}.min_dist"])
    np.testing.assert_allclose(m["min_dist"][finite], Z[f"a.{case}.min_dist"][finite], rtol=1e-6, atol=0)


def test_g16a_covers_each_quirk():
    """The crafted scenes do what their names promise (a fixture that lost its edge cases would pin nothing)."""
    assert np.all(Z["a.cross13.col"] == 50) and np.all(Z["a.cross14.col"] == 0)  # the window ends at dense instant 13
    assert np.all(Z["a.twins.col"][:2] == 100)                                    # identical pedestrians collide
    assert np.all(Z["a.single.col"] == 0)
    assert (Z["a.motionless.tcc"] == 0).sum() >= 3 and Z["a.motionless.noise"].any()
    assert Z["a.t3.gt"].shape[1] == 3 and np.isnan(Z["a.nan.pred"]).any()
    assert Z["a.nan.col_bits"][:, 3].sum() == 0 and np.isfinite(Z["a.nan.tcc"]).all()  # NaN rows: no collision, NaN -> 0
    assert Z["a.ties.best"].min() >= 0


def test_tcc_tree_mean_of_a_motionless_series_is_exact_where_atens_is():
    """For a constant series the binary-counter tree / T equals ATen's mean bit for bit (G16's noise flags are exactly
    the rows where neither is the value)."""
    for case in CASES:
        gt = Z[f"a.{case}.gt"]
        T = gt.shape[1]
        const = (gt == gt[:, :1]).all(axis=1)
        inexact = (R.tree_sum(np.moveaxis(gt, 1, -1)) / np.float32(T)) != gt[:, 0]
        assert np.array_equal((const & inexact).any(axis=1), Z[f"a.{case}.noise"]), case
