"""csrc/et_tsne.hip away from the one input the G18 tests run (N = 2 000, d = 6, perplexity 30, k = 91, all rows distinct):
N below / at / one past the block constants (64 kNN rows and LDS tile, 256 rows a block, 1 024 columns a chunk and scan
slices), d in both kNN template instances, k = N - 1, other perplexities, distance ties and zero distances, dropped zero
sums, coincident and nearly coincident embedding points, both parities of the optimiser's copy-back.  Every stage against
the numpy restatement (tests/_tsne_np.py) on seeded inputs, and against sklearn's records at the coincidence edges
(tests/golden/g18c_tsne_edges.npz, tools/make_golden_tsne.py --edges)."""
import numpy as np
import pytest
import torch

from . import _golden as G
from . import _tsne_np as TN
from ._gpu_common import *  # noqa: F401,F403 -- fixtures (dev, ops) and helpers

pytestmark = pytest.mark.gpu
ZE = G.load("g18c_tsne_edges.npz")
INT32_MAX = 2 ** 31 - 1


def _id(case):
    return "-".join(str(c) for c in case)


# ------------------------------------------------------------------------------------------------------- affinities
def make_x(n, d, family, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    if family == "x1e4":
        x = x * np.float32(1e4)
    elif family == "x1e-4":
        x = x * np.float32(1e-4)
    elif family == "lattice":  # massive ties at every distance
        x = rng.integers(0, 3, size=(n, d)).astype(np.float32)
    elif family == "dup":  # the second half repeats the first: zero distances
        x[n // 2:2 * (n // 2)] = x[:n // 2]
    elif family == "equal":
        x[:] = x[0]
    else:
        assert family == "normal"
    return np.ascontiguousarray(x)


# (N, d, perplexity, family).  k = min(N - 1, 3 perplexity + 1): 16, 31, 91, 151.  d <= 8 runs knn_kernel<8>, d > 8
# knn_kernel<32>.  The large N take perplexity 5 to keep the restatement's libm exp loop short.
AFF_CASES = [
    (2, 2, 5, "normal"), (2, 1, 30, "equal"), (3, 1, 5, "normal"), (3, 6, 30, "dup"),
    (63, 6, 30, "normal"), (63, 32, 50, "lattice"), (64, 8, 30, "lattice"), (64, 6, 5, "equal"),
    (65, 9, 30, "normal"), (65, 2, 5, "equal"),
    (200, 2, 10, "lattice"),
    (255, 6, 50, "normal"), (255, 9, 5, "x1e-4"), (256, 32, 30, "x1e4"), (256, 1, 30, "lattice"),
    (257, 32, 5, "dup"), (257, 2, 30, "x1e-4"), (257, 6, 30, "equal"),
    (1023, 6, 30, "normal"), (1023, 1, 5, "normal"), (1024, 9, 5, "lattice"), (1024, 6, 30, "dup"),
    (1025, 8, 50, "normal"), (1025, 2, 5, "dup"),
    (2049, 6, 5, "normal"), (2049, 32, 5, "x1e4"),
]


def test_affinity_cases_cover_the_sizes():
    assert {2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049} <= {c[0] for c in AFF_CASES}
    assert {1, 2, 6, 8, 9, 32} <= {c[1] for c in AFF_CASES} and {5, 30, 50} <= {c[2] for c in AFF_CASES}
    assert {"normal", "x1e4", "x1e-4", "lattice", "dup", "equal"} == {c[3] for c in AFF_CASES}


@pytest.mark.parametrize("case", AFF_CASES, ids=_id)
def test_affinities_match_restatement(dev, ops, case):
    n, d, perp, family = case
    X = make_x(n, d, family, 1000 + n + d)
    aff = ops.tsne_affinities(T(X, dev), float(perp))
    got = {k: N_(v) for k, v in aff.items()}
    k = TN.n_neighbors(n, perp)
    assert got["knn_idx"].shape == (n, k)
    idx, dist = TN.knn(X, k)
    if family in ("dup", "equal"):
        assert (dist == 0).any() and (got["knn_dist"] == 0).any()
    if family == "x1e4":  # at beta = 1 every exp underflows: the search starts through the sum_p == 0 clamp
        assert not np.exp(-dist.astype(np.float64)).any()
    assert np.array_equal(got["knn_idx"], idx)
    assert np.array_equal(got["knn_dist"], dist)
    pc = TN.binary_search_perplexity(dist, float(perp), exp=TN.libm_exp)
    assert np.all(np.isfinite(pc)) and np.all(np.isfinite(got["p_cond"]))
    # within one fp32 ulp (test_gpu_tsne._check_pcond's rule; the device's fp64 exp / log against libm's)
    assert np.all(np.abs(got["p_cond"] - pc) <= np.spacing(pc.astype(np.float32)).astype(np.float64))
    # the CSR against the restated symmetrisation of the kernel's own conditional P: same pattern, same bits
    indptr, indices, P, total = TN.symmetrize(got["knn_idx"], got["p_cond"])
    assert np.array_equal(got["indptr"], indptr) and np.array_equal(got["indices"], indices)
    assert np.array_equal(got["P"], P) and got["total"].item() == total
    assert np.all(np.isfinite(got["P"]))
    if case == (200, 2, 10, "lattice"):  # the dropped-zero path of merge_kernel: zero sums leave the pattern
        rows = np.repeat(np.arange(n), k)
        pairs = np.unique(np.concatenate([rows * n + idx.ravel(), idx.ravel().astype(np.int64) * n + rows]))
        assert (got["p_cond"] == 0).any() and P.size < 2 * n * k and P.size < pairs.size
    again = ops.tsne_affinities(T(X, dev), float(perp))
    for key, v in aff.items():
        assert torch.equal(v, again[key]), key


# --------------------------------------------------------------------------------------------------------- gradient
@pytest.fixture(scope="module")
def csr_of(dev, ops):
    """N -> (indptr, indices, P fp64) on the device: the affinities of a seeded normal X (N, 6), perplexity 30"""
    cache = {}

    def get(n):
        if n not in cache:
            aff = ops.tsne_affinities(T(make_x(n, 6, "normal", 2000 + n), dev))
            cache[n] = (aff["indptr"], aff["indices"], aff["P"])
        return cache[n]
    return get


def embedding(n, name):
    if name == "unit":
        return np.random.default_rng(3000 + n).standard_normal((n, 2)).astype(np.float32)
    return TN.edge_embeddings(n, 3000 + n)[name]


# N = 2 and 3 have k = N - 1 below the perplexity: the search cannot reach it and P is uniform.  Two distinct points then
# have gradient 0 whatever their distance (check_n2_far), and three points at std 1e-4 have Q uniform to 1e-8, below what
# fp32 forces resolve (measured: a gradient of 1e-8 of the forces, pure rounding): no (3, "pca") case, a bound relative
# to max |grad| says nothing there.  At unit scale the three distances differ and the gradient is an ordinary one.
GRAD_CASES = [
    (2, "unit"), (2, "eq0"), (2, "dup"),
    (3, "unit"), (3, "dup"), (3, "d9e-7"),
    (255, "unit"), (255, "d9e-7"),
    (256, "pca"), (256, "dup"), (256, "eqc"),
    (257, "unit"), (257, "d1e-7"), (257, "d2e-6"),
    (1023, "pca"), (1023, "d9e-7"),
    (1024, "unit"), (1024, "dup"), (1024, "eq0"),
    (1025, "pca"), (1025, "d1e-7"), (1025, "d2e-6"), (1025, "eqc"),
    (2049, "unit"), (2049, "d9e-7"), (2049, "eq0"),
    (3000, "pca"), (3000, "d1e-7"),
]


def _kernel_kl_grad(ops, dev, Y, indptr, indices, P32):
    kl, g = ops.tsne_kl_grad(T(Y, dev), indptr, indices, P32)
    kl2, g2 = ops.tsne_kl_grad(T(Y, dev), indptr, indices, P32)
    assert torch.equal(g, g2) and N_(kl).tobytes() == N_(kl2).tobytes()  # bit-equal, a NaN included
    return kl.item(), N_(g)


@pytest.mark.parametrize("case", GRAD_CASES, ids=_id)
def test_kl_grad_matches_restatement(dev, ops, csr_of, case):
    n, name = case
    indptr, indices, P = csr_of(n)
    P32 = P.float()
    Y = embedding(n, name)
    if name.startswith("d"):
        hi, lo = TN.pair_offsets(Y)
        assert (not hi.any()) if name == "dup" else (lo.min() > (1e-6 if name == "d2e-6" else 0.0))
        assert name in ("dup", "d2e-6") or hi.max() <= 1e-6
    kl, g = _kernel_kl_grad(ops, dev, Y, indptr, indices, P32)
    all_equal = len(np.unique(Y, axis=0)) == 1
    if n == 2 and not all_equal:
        TN.check_n2_far(kl, g, Y)
        return
    with np.errstate(all="ignore"):
        kln, gn = TN.kl_grad(Y, N_(indptr), N_(indices), N_(P32))
    print(f"N {n} {name}: KL {kl!r} (restatement {kln!r}) max |grad - restatement| / max |grad| "
          f"{float(np.abs(g - gn).max()) / max(float(np.abs(gn).max()), 1e-300):.3g}")
    TN.check_kl_grad(kl, g, kln, gn, all_equal)


@pytest.fixture(scope="module")
def edge_csr():
    X = ZE["X"]
    idx, d = TN.knn(X, TN.n_neighbors(X.shape[0]))
    return TN.symmetrize(idx, TN.binary_search_perplexity(d, 30.0, exp=TN.libm_exp))[:3]


@pytest.mark.parametrize("name", TN.EDGE_NAMES)
def test_kl_grad_matches_sklearn_edge_records(dev, ops, edge_csr, name):
    indptr, indices, P = edge_csr
    kl, g = _kernel_kl_grad(ops, dev, ZE[f"emb.{name}"], T(indptr, dev), T(indices, dev), T(P.astype(np.float32), dev))
    print(f"{name}: KL {kl!r} (sklearn {float(ZE[f'kl.{name}'])!r}) max |grad - sklearn| / max |grad| "
          f"{float(np.abs(g - ZE[f'grad.{name}']).max()) / max(float(np.abs(ZE[f'grad.{name}']).max()), 1e-300):.3g}")
    TN.check_kl_grad(kl, g, float(ZE[f"kl.{name}"]), ZE[f"grad.{name}"], name.startswith("eq"))


def test_kl_grad_two_points_match_sklearn_records(dev, ops):
    csr = [T(a, dev) for a in TN.N2_P]
    kl, g = _kernel_kl_grad(ops, dev, ZE["n2.emb.eq"], *csr)
    TN.check_kl_grad(kl, g, float(ZE["n2.kl.eq"]), ZE["n2.grad.eq"], True)
    TN.check_n2_far(*_kernel_kl_grad(ops, dev, ZE["n2.emb.far"], *csr), ZE["n2.emb.far"])


# -------------------------------------------------------------------------------------------------- fused optimiser
@pytest.mark.parametrize("m", [1, 2, 3])
@pytest.mark.parametrize("n", [257, 1025])
def test_optimize_prefix_bit_equal_to_standalone_steps(dev, ops, csr_of, n, m):
    """max_iter = m inside et_tsne_optimize against m standalone rounds of gradient + update: both parities of the
    copy-back of the alternating position buffers, and the tail blocks of N = 257 and 1 025"""
    indptr, indices, P = csr_of(n)
    lr = float(np.maximum(n / 12.0 / 4, 50))
    Y0 = T(embedding(n, "pca"), dev)
    y, _, it = ops.tsne_optimize(Y0, indptr, indices, P, 12.0, lr, m)
    assert it == m
    p1 = T(TN.phase_p(N_(P), 12.0, False), dev)
    p = Y0.clone().reshape(-1)
    upd = torch.zeros(2 * n, device=dev, dtype=torch.float64)
    gains = torch.ones(2 * n, device=dev)
    for _ in range(m):
        _, g = ops.tsne_kl_grad(p.reshape(n, 2), indptr, indices, p1)
        ops.tsne_update(p, upd, gains, g.reshape(-1).contiguous(), 0.5, lr)
    assert torch.equal(p.reshape(n, 2), y)
    assert not torch.equal(y, Y0)


def test_whole_run_from_all_zero_init_matches_sklearn(dev):
    """all points coincident: sklearn clamps Z, returns a gradient of exactly 0 and stops at the first checks of the
    two phases (recorded: the zero embedding, n_iter_ 99)"""
    from eigentrajectory_amd.tsne import TSNE
    X = ZE["X"]
    ts = TSNE(n_components=2, random_state=42, init=np.zeros((X.shape[0], 2), np.float32))
    emb = ts.fit_transform(X)
    assert np.all(np.isfinite(emb)) and not np.isnan(ts.kl_divergence_)
    assert np.array_equal(emb, ZE["zero.embedding"]) and ts.n_iter_ == int(ZE["zero.n_iter"])


# --------------------------------------------------------------------------------------------------------- PCA init
def pca_x(n, d, seed):
    """columns scaled 3, 2, 1, 1/2, 1/3, ...: the two top eigenvalues well apart from each other and the rest"""
    scale = np.array([3.0, 2.0] + [1.0 / c for c in range(1, d - 1)])
    return (np.random.default_rng(seed).standard_normal((n, d)) * scale).astype(np.float32)


PCA_CASES = [(3, 2), (3, 6), (255, 3), (255, 32), (257, 2), (257, 9), (257, 32), (5000, 6), (5000, 32)]


@pytest.mark.parametrize("case", PCA_CASES, ids=_id)
def test_pca_init_matches_restatement(dev, ops, case):
    """the bound is the reference's own sensitivity: TN.pca_init on X against X moved by one fp32 ulp (seeded signs),
    times 4 (the kernel rounds the centred rows, the eigenvectors and the d-term projection to fp32, each about one
    input ulp), with the floor of 1e-6 of max |Y0| that the subset holds against sklearn.  The reference's spread,
    measured as a fraction of max |Y0|: (3, 2) 7.9e-8, (3, 6) 1.1e-7, (255, 3) 1.9e-7, (255, 32) 1.7e-7, (257, 2) 9.9e-8,
    (257, 9) 2.0e-7, (257, 32) 2.2e-7, (5000, 6) 2.5e-7, (5000, 32) 1.5e-7 -- 4 x the spread is below the floor at
    every case, so the floor decides."""
    n, d = case
    X = pca_x(n, d, 4000 + n + d)
    ref = TN.pca_init(X)
    sign = np.random.default_rng(5000 + n + d).integers(0, 2, X.shape).astype(bool)
    moved = np.where(sign, np.nextafter(X, np.float32(np.inf)), np.nextafter(X, np.float32(-np.inf)))
    scale = np.abs(ref).max()
    spread = np.abs(TN.pca_init(moved) - ref).max() / scale
    got = N_(ops.tsne_pca_init(T(X, dev)))
    err = np.abs(got - ref).max() / scale
    print(f"pca_init N {n} d {d}: reference moves {spread:.3g} of max |Y0| under 1 ulp of X, kernel differs {err:.3g}")
    assert np.all(np.isfinite(got)) and err <= max(4 * spread, 1e-6)
    assert abs(np.std(got[:, 0].astype(np.float64)) - 1e-4) <= 1e-10


# -------------------------------------------------------------------------------------------------- argument edges
def _allocations(dev):
    return torch.cuda.memory_stats(dev)["allocation.all.allocated"]


def test_rejected_shapes_allocate_and_launch_nothing(dev, ops):
    """N = 1, d = 0 and d = 33 are turned away by the host-side size functions, before any buffer is made"""
    from eigentrajectory_amd import _lib as L
    lib = L.lib()
    xs = [torch.zeros((1, 6), device=dev), torch.zeros((40, 0), device=dev), torch.zeros((40, 33), device=dev)]
    torch.cuda.synchronize(dev)
    before = _allocations(dev)
    for x in xs:
        with pytest.raises(ValueError):
            ops.tsne_affinities(x, 5.0)
    assert _allocations(dev) == before
    assert lib.et_tsne_neighbors(L.i64(1), L.C.c_double(5.0)) == 0
    for n, d, k in ((1, 6, 1), (40, 0, 16), (40, 33, 16), (40, 6, 40), (40, 6, 0)):
        assert lib.et_tsne_affinities_workspace_bytes(L.i64(n), d, k) == 0, (n, d, k)
    assert lib.et_tsne_affinities_workspace_bytes(L.i64(40), 6, 39) > 0
    assert lib.et_tsne_affinities_workspace_bytes(L.i64(40), 32, 16) > 0
    assert lib.et_tsne_kl_grad_workspace_bytes(L.i64(1)) == 0 and lib.et_tsne_optimize_workspace_bytes(L.i64(1), L.i64(0)) == 0
    for n, d in ((1, 6), (40, 1), (40, 33)):
        assert lib.et_tsne_pca_init_workspace_bytes(L.i64(n), d) == 0
    # 2 N k is the CSR's capacity, indexed in int32
    k = 91
    n_over = INT32_MAX // (2 * k) + 1
    assert 2 * n_over * k > INT32_MAX >= 2 * (n_over - 1) * k
    assert lib.et_tsne_affinities_workspace_bytes(L.i64(n_over), 6, k) == 0
    assert lib.et_tsne_affinities_workspace_bytes(L.i64(n_over - 1), 6, k) > 0
    with pytest.raises(ValueError):
        ops.tsne_kl_grad(torch.zeros((1, 2), device=dev), *[T(a, dev) for a in TN.N2_P])
    with pytest.raises(ValueError):
        ops.tsne_pca_init(torch.zeros((1, 6), device=dev))


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_non_finite_embedding_at_a_ragged_size_is_bad_data(dev, ops, csr_of, bad):
    """the last row of N = 257 is the only live lane of its block"""
    n = 257
    indptr, indices, P = csr_of(n)
    Y = T(embedding(n, "unit"), dev)
    Y[n - 1, 1] = bad
    with pytest.raises(ValueError):
        ops.tsne_kl_grad(Y, indptr, indices, P.float())
    with pytest.raises(ValueError):
        ops.tsne_optimize(Y, indptr, indices, P, 12.0, 50.0, 3)
