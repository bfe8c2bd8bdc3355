"""CPU checks of the t-SNE of descriptor coefficients (script/plot_coeff_tsne.py): the C ABI's new names, the TSNE
class's argument checks (made before any device is touched), and the numpy restatement of csrc/et_tsne.hip
(tests/_tsne_np.py) against sklearn's own outputs (tests/golden/g18_tsne.npz, tools/make_golden_tsne.py)."""
import os
import re
import zlib

import numpy as np
import pytest

from . import _abi_header as H
from . import _golden as G
from . import _tsne_np as T

Z = G.load("g18_tsne.npz")
NAMES = ["et_tsne_neighbors", "et_tsne_affinities_workspace_bytes", "et_tsne_affinities",
         "et_tsne_kl_grad_workspace_bytes", "et_tsne_kl_grad", "et_tsne_update", "et_tsne_optimize_workspace_bytes",
         "et_tsne_optimize", "et_tsne_pca_init_workspace_bytes", "et_tsne_pca_init"]


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def test_tsne_abi_names_declared_listed_and_exported():
    from eigentrajectory_amd import _lib
    header = H.text()
    for name in NAMES:
        assert re.search(rf"\b{name}\(", header), name
        assert name in _lib.SYMBOLS, name
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.lib()
        assert all(hasattr(lib, n) for n in NAMES)
        assert lib.et_tsne_neighbors(_lib.i64(29809), _lib.C.c_double(30.0)) == 91
        assert lib.et_tsne_neighbors(_lib.i64(50), _lib.C.c_double(30.0)) == 49
        assert lib.et_tsne_neighbors(_lib.i64(1), _lib.C.c_double(30.0)) == 0


def test_tsne_rejects_bad_arguments_before_the_device():
    from eigentrajectory_amd.tsne import TSNE
    with pytest.raises(ValueError):
        TSNE(n_components=3)
    with pytest.raises(ValueError):
        TSNE(init="random")
    with pytest.raises(ValueError):
        TSNE(max_iter=100)
    with pytest.raises(ValueError):
        TSNE(learning_rate=-1.0)
    X = np.random.default_rng(0).standard_normal((30, 6)).astype(np.float32)
    with pytest.raises(ValueError, match="perplexity"):
        TSNE(perplexity=30).fit_transform(X)
    with pytest.raises(ValueError):
        TSNE(perplexity=5).fit_transform(np.zeros((1, 6), np.float32))
    with pytest.raises(ValueError):
        TSNE(perplexity=5).fit_transform(np.zeros((40, 33), np.float32))
    with pytest.raises(ValueError, match="features"):
        TSNE(perplexity=5).fit_transform(np.zeros((40, 1), np.float32))
    with pytest.raises(ValueError):
        TSNE(perplexity=5, init=np.zeros((39, 2), np.float32)).fit_transform(X[:20].repeat(2, 0))


@pytest.fixture(scope="module")
def sub_aff():
    X = Z["sub.X"]
    idx, d = T.knn(X, T.n_neighbors(X.shape[0]))
    pc = T.binary_search_perplexity(d, 30.0, exp=T.libm_exp)
    return idx, d, pc


def test_np_knn_matches_sklearn(sub_aff):
    idx, d, _ = sub_aff
    assert [crc(np.sort(r)) for r in d] == list(Z["sub.knn_dcrc"])
    icrc = np.array([crc(np.sort(r)) for r in idx], np.uint32)
    tie = Z["sub.knn_tie"]
    assert np.array_equal(icrc[~tie], Z["sub.knn_icrc"][~tie])
    rows = Z["sub.s_rows"]
    assert np.array_equal(d[rows], Z["sub.s_knn_d"])


def test_np_conditional_p_matches_sklearn(sub_aff):
    """bit for bit on >= 99.9 % of the entries, within one fp32 ulp on all"""
    _, _, pc = sub_aff
    rows = Z["sub.s_rows"]
    ref = Z["sub.s_pcond"]
    got = pc[rows]
    assert np.mean(got == ref) >= 0.999
    assert np.all(np.abs(got - ref) <= np.spacing(ref.astype(np.float32)).astype(np.float64))
    assert np.mean(np.array([crc(r) for r in pc], np.uint32) == Z["sub.pcond_crc"]) >= 0.99


def test_np_symmetric_p_matches_sklearn(sub_aff):
    idx, _, pc = sub_aff
    indptr, indices, P, total = T.symmetrize(idx, pc)
    assert total == Z["sub.P_total"]
    assert np.array_equal(indptr, Z["sub.P_indptr"])
    assert [crc(indices[indptr[i]:indptr[i + 1]]) for i in range(len(indptr) - 1)] == list(Z["sub.P_icrc"])
    rs = np.add.reduceat(P, indptr[:-1])
    np.testing.assert_allclose(rs, Z["sub.P_rowsum"], rtol=1e-12)
    off = Z["sub.s_P_off"]
    for t, r in enumerate(Z["sub.s_rows"]):
        assert np.array_equal(indices[indptr[r]:indptr[r + 1]], Z["sub.s_P_idx"][off[t]:off[t + 1]])
        np.testing.assert_allclose(P[indptr[r]:indptr[r + 1]], Z["sub.s_P_val"][off[t]:off[t + 1]], rtol=1e-15)


@pytest.mark.parametrize("name", ["y50", "y400", "yrand"])
def test_np_gradient_and_kl_match_sklearn_theta0(sub_aff, name):
    idx, _, pc = sub_aff
    indptr, indices, P, _ = T.symmetrize(idx, pc)
    kl, g = T.kl_grad(Z[f"emb.{name}"], indptr, indices, P.astype(np.float32))
    ref = Z[f"grad.{name}"]
    # sklearn sums the forces in fp32 (2 000 terms a row): near convergence (y400) pos - neg / Z cancels to 2.8e-5 of max
    assert np.abs(g - ref).max() <= 5e-5 * np.abs(ref).max()
    assert abs(kl - Z[f"kl.{name}"]) <= 1e-5 * abs(Z[f"kl.{name}"])


def test_np_update_is_sklearns_step():
    """the restated step against sklearn's own _gradient_descent, four iterations on a stub objective with recorded
    gradients (the update becomes fp64 after the first step; gains rise and fall)"""
    _t_sne = pytest.importorskip("sklearn.manifold._t_sne")
    rng = np.random.default_rng(3)
    n = 1000
    p0 = rng.standard_normal(n).astype(np.float32)
    grads = [(rng.standard_normal(n) * 1e-3).astype(np.float32) for _ in range(4)]
    calls = []

    def objective(p, compute_error=True):
        calls.append(len(calls))
        return 1.0, grads[len(calls) - 1].copy()

    lr = np.maximum(29809 / 12.0 / 4, 50)
    for mom in (0.5, 0.8):
        calls.clear()
        ref, _, it = _t_sne._gradient_descent(objective, p0, 0, 4, n_iter_check=100, momentum=mom, learning_rate=lr)
        assert it == 3
        p, upd, gains = p0.copy(), np.zeros(n), np.ones(n, np.float32)
        for g in grads:
            p, upd, gains, gg = T.update(p, upd, gains, g, mom, lr)
            assert p.dtype == np.float32 and upd.dtype == np.float64 and gains.dtype == np.float32
        assert np.array_equal(p, ref)


def test_fixture_records():
    assert Z["sub.X"].shape == (2000, 6) and len(np.unique(Z["sub.X"], axis=0)) == 2000
    assert np.all(Z["run.n_iter"] == 999)
    assert abs(float(Z["default.eth.kl"]) - 1.4434) < 2e-3
    for name in ("y50", "y400", "yrand"):
        assert Z[f"emb.mind.{name}"] > 1e-6


# ------------------------------------------------------------ coincident and nearly coincident embedding points (g18c)
ZE = G.load("g18c_tsne_edges.npz")
@pytest.fixture(scope="module")
def edge_csr():
    X = ZE["X"]
    idx, d = T.knn(X, T.n_neighbors(X.shape[0]))
    indptr, indices, P, _ = T.symmetrize(idx, T.binary_search_perplexity(d, 30.0, exp=T.libm_exp))
    return indptr, indices, P


def test_edge_fixture_records(edge_csr):
    """the recorded cases are what their names say, and the restated P is the P sklearn's records were computed on"""
    indptr, indices, P = edge_csr
    assert P.size == int(ZE["P_nnz"]) and crc(P) == int(ZE["P_crc"])
    embs = T.edge_embeddings(ZE["X"].shape[0], int(ZE["seed"]) + 1)
    for name in T.EDGE_NAMES:
        assert np.array_equal(embs[name], ZE[f"emb.{name}"]), name
    for name, lo_min, hi_max in (("d1e-7", 0.0, 1e-6), ("d9e-7", 0.0, 1e-6), ("d2e-6", 1e-6, 3e-6)):
        hi, lo = T.pair_offsets(embs[name])
        assert np.all(lo > lo_min) and np.all(hi <= hi_max), name
    hi, _ = T.pair_offsets(embs["dup"])
    assert not np.any(hi)
    y = embs["pca"].astype(np.float64)
    near = np.all(np.abs(y[:, None] - y[None]) <= 1e-6, axis=-1).sum() - len(y)
    assert near > 0 and len(np.unique(embs["pca"], axis=0)) == len(y)  # pairs within 1e-6, none equal
    assert ZE["zero.n_iter"] == 99 and not np.any(ZE["zero.embedding"])
    m = G.manifest()["g18c_tsne_edges"]
    assert m["sklearn"] == "1.7.2" and float(m["kl"]["d9e-7"]) == float(ZE["kl.d9e-7"])


@pytest.mark.parametrize("name", T.EDGE_NAMES)
def test_np_edge_gradient_matches_sklearn_records(edge_csr, name):
    """sklearn as compiled leaves out exactly coincident points only (d1e-7 and d9e-7 have the KL of d2e-6, not of dup)
    and clamps Z to DBL_EPSILON (eq0, eqc: gradient exactly 0)"""
    indptr, indices, P = edge_csr
    kl, g = T.kl_grad(ZE[f"emb.{name}"], indptr, indices, P.astype(np.float32))
    T.check_kl_grad(kl, g, float(ZE[f"kl.{name}"]), ZE[f"grad.{name}"], name.startswith("eq"))


def test_np_edge_gradient_two_points_match_sklearn_records():
    kl, g = T.kl_grad(ZE["n2.emb.eq"], *T.N2_P)
    T.check_kl_grad(kl, g, float(ZE["n2.kl.eq"]), ZE["n2.grad.eq"], True)
    Y = ZE["n2.emb.far"]
    T.check_n2_far(float(ZE["n2.kl.far"]), ZE["n2.grad.far"], Y)  # sklearn's own record
    T.check_n2_far(*T.kl_grad(Y, *T.N2_P), Y)


def test_np_edge_gradient_matches_live_sklearn():
    """the same cases at another size and seed against the installed sklearn's theta = 0 gradient"""
    _t_sne = pytest.importorskip("sklearn.manifold._t_sne")
    from scipy.sparse import csr_matrix
    from sklearn.neighbors import NearestNeighbors
    n = 120
    X = np.random.default_rng(7).standard_normal((n, 3)).astype(np.float32)
    g = NearestNeighbors(n_neighbors=T.n_neighbors(n, 10.0)).fit(X).kneighbors_graph(mode="distance")
    g.data **= 2
    P = _t_sne._joint_probabilities_nn(g, 10.0, 0)
    kw = dict(angle=0.0, skip_num_points=0, verbose=0, num_threads=1, compute_error=True)
    for name, Y in T.edge_embeddings(n, 8).items():
        err, grad = _t_sne._kl_divergence_bh(Y.ravel().copy(), P, 1, n, 2, **kw)
        kl, gn = T.kl_grad(Y, P.indptr, P.indices, P.data.astype(np.float32))
        T.check_kl_grad(kl, gn, float(err), grad.reshape(n, 2).astype(np.float32), name.startswith("eq"))
    P2 = csr_matrix(np.array([[0.0, 0.5], [0.5, 0.0]]))
    for key, all_equal in (("eq", True), ("far", False)):
        Y = ZE[f"n2.emb.{key}"]
        err, grad = _t_sne._kl_divergence_bh(Y.ravel().copy(), P2, 1, 2, 2, **kw)
        grad = grad.reshape(2, 2).astype(np.float32)
        if all_equal:
            T.check_kl_grad(*T.kl_grad(Y, *T.N2_P), float(err), grad, True)
        else:
            T.check_n2_far(float(err), grad, Y)
