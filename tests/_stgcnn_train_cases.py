"""Shared inputs of tests/test_stgcnn_train_cpu.py and tests/test_gpu_stgcnn_train.py: the configurations, scenes and
upstream gradients of the STGCNN training tests, all seeded.  Not a test module itself.

A scene's seed is the first for which the float64 restatement ALONE (tests/_stgcnn_train_np.py, no device) leaves no kept
PReLU input within its own step's fp32 bound of 0; tests/test_stgcnn_train_cpu.py asserts it, no scene is filtered out."""
import numpy as np

from . import _stgcnn_np as SN

# name -> (n_txpcnn, S, k): the smallest shapes at which each code path can go wrong
CONFIGS = {"et": (5, 20, 6),     # the ET configuration
           "s1": (3, 1, 1),      # identity residual, no residual.*; K = 3: 3 values per channel at n = 1
           "tp1": (1, 3, 2),     # output conv straight on prelus[0]; nothing unused
           "tp2": (2, 3, 2),     # empty loop; tpcnns[1] and prelus[1] unused
           "tp3": (3, 2, 4),     # one loop pass; ping-pong
           "smax": (2, 64, 1),   # widest
           "kmax": (2, 2, 32)}   # deepest rank
EXACT_N = (1, 2, 3, 5)
RAGGED_N = (63, 64, 65, 257)     # et only: the wavefront and workgroup edges (the training body has no placement switch:
BEYOND_N = 512                   # every scene lives in the workspace)
LAYOUTS = {"one": [1], "mixed": [3, 1, 5], "empty": [3, 0, 2], "many": [2] * 40}
MOMENTUM, EPS = 0.1, 1e-5
SEED = {("et", 257): 3}          # (config, n) -> seed of the scene; default 1


def module_kw(name):
    n_tp, S, k = CONFIGS[name]
    return SN.module_kw(1, n_tp, S, k)


def module(name, device=None, seed=7):
    """a SocialSTGCNN of configuration ``name`` with seeded non-default values in every tensor (buffers included)"""
    import eigentrajectory_amd as ET
    m = ET.SocialSTGCNN(**module_kw(name))
    SN.random_state(m, seed)
    return m if device is None else m.to(device)


def state(m):
    """-> the module's state_dict as numpy arrays"""
    return {k: t.detach().cpu().numpy().copy() for k, t in m.state_dict().items()}


def scene(name, n):
    """-> v (K, n) fp32 and a (K, n, n) fp32 (the bridge's Laplacian, rounded once from float64) of the case (name, n)"""
    k = CONFIGS[name][2]
    rng = np.random.default_rng([SEED.get((name, n), 1), n, k])
    v = np.concatenate([rng.normal(0, 1, (k, n)), rng.normal(0, 2, (2, n))]).astype(np.float32)
    v[-2:] -= v[-2:].mean(axis=1, keepdims=True, dtype=np.float32)
    return v, SN.adjacency(v).astype(np.float32)


def d_out(name, n, seed=0):
    """the upstream gradient (1, S, k, n), N(0, 1) in fp32"""
    _, S, k = CONFIGS[name]
    return np.random.default_rng([seed, n, k, S]).normal(0, 1, (1, S, k, n)).astype(np.float32)


def split(sizes, name="et", seed=3):
    """-> C_obs (k, N), nrm (4, N) of a scenes-form layout (tests/_stgcnn_np.exact_split: the scene means are exact)"""
    return SN.exact_split(sizes, CONFIGS[name][2], seed)


def kernel_laplacian(u):
    """u (K, n) fp32 -> (d (K, n), L (K, n, n)) in float32 with the scene kernel's own statements and orders: a row's degree
    is added over w ascending, one term (a_inv + eye) at a time; d = 1 / sqrt(deg); L[v, w] = eye - (d_v (a_inv + eye)) d_w --
    every operation a single correctly rounded float32 one, so the graph form fed with (u, L) computes what the scenes form
    computes from u"""
    u = np.asarray(u, np.float32)
    f = np.float32
    K, n = u.shape
    eye = np.eye(n, dtype=f)
    dist = np.abs(u[:, :, None] - u[:, None, :])
    with np.errstate(divide="ignore"):
        ainv = np.where(dist == 0, f(0), f(1) / dist).astype(f)
    a_hat = (ainv + eye).astype(f)
    deg = np.add.accumulate(a_hat, axis=2, dtype=f)[:, :, -1]   # sequential, ascending
    d = (f(1) / np.sqrt(deg, dtype=f)).astype(f)
    L = eye - ((d[:, :, None] * a_hat).astype(f) * d[:, None, :]).astype(f)
    return d, L.astype(f)
