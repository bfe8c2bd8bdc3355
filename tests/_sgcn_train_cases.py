"""Shared inputs of tests/test_sgcn_train_cpu.py and tests/test_gpu_sgcn_train.py: the configurations, scenes and upstream
gradients of the SGCN training tests, all seeded.  Not a test module itself.

The scenes are tests/_sgcn_np.py's synthetic ones.  A seed is the first for which the float64 restatement ALONE
(tests/_sgcn_train_np.py, no device) keeps the undecided decisions -- mask logits within DELTA of 0, PReLU arguments within
their own layer's bound of 0 -- within CAP_SCENE of the scene's decisions of each kind, and, for the exact cases, leaves the
band EMPTY; tests/test_sgcn_train_cpu.py asserts both, no scene is filtered out."""
import numpy as np

from . import _sgcn_np as SN

EXACT_N = (1, 2, 3, 5)
EXACT_CONFIGS = ("k1", "k2_wide", "et")
RAGGED = [("et", n) for n in (17, 63, 64, 65, 130)] + [("deep", 65), ("kmax", 3), ("kmax", 65)]
BEYOND = (257, 512)                       # with k1: no float64 comparison (tests/_sgcn_np.py: ZeroSoftmax cancels in fp32)
LAYOUTS = {"edge": "et", "many": "k1"}    # scenes form: layout of tests/_sgcn_np.LAYOUTS -> configuration
SEED = {}                                 # (config, n) -> seed of the scene; default 1
LAYOUT_SEED = {"edge": 1, "many": 3}


def seed_of(name, n):
    return SEED.get((name, n), 1)


def scene(name, n):
    """-> v (T, n) fp32 of the single-scene case (name, n)"""
    C_obs, nrm = SN.synthetic_split([n], seed_of(name, n) + 1000 * n, SN.CONFIGS[name]["k"])
    return SN.scene_input(C_obs, nrm, 0, n)


def layout(which):
    """-> (config, sizes, C_obs (k, N), nrm (4, N)) of a scenes-form layout"""
    name = LAYOUTS[which]
    sizes = SN.LAYOUTS[which]
    C_obs, nrm = SN.synthetic_split(sizes, LAYOUT_SEED[which], SN.CONFIGS[name]["k"])
    return name, sizes, C_obs, nrm


def d_out(name, n, seed=0):
    """the upstream gradient (pred_len, n, out_dims), N(0, 1) in fp32"""
    c = SN.CONFIGS[name]
    return np.random.default_rng([seed, n, c["k"]]).normal(0, 1, (c["k"], n, c["S"])).astype(np.float32)


def module(name, device=None):
    import torch

    import eigentrajectory_amd as ET
    m = ET.SGCN(**SN.module_cfg(name))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in SN.random_state(name).items()})
    return m if device is None else m.to(device)


def within_caps(fig, exact=False):
    """the seed conditions on :meth:`tests._sgcn_train_np.Decisions.figures`"""
    for kind in ("mask", "prelu"):
        f = fig[kind]
        if exact and f["undecided"]:
            return False
        if f["undecided"] > SN.CAP_SCENE * f["entries"]:
            return False
    return True


def _basis(sd, key):
    p = key.rsplit(".", 2)[0] + ".embedding."
    return np.stack([np.asarray(sd[p + "weight"], np.float64)[:, 0], np.asarray(sd[p + "bias"], np.float64)], 1)   # (64, 2)


def pack(sd, key, M):
    """fixture G29: the (64, 64) gradient of a query.weight / key.weight, M = F [we be]^T -> (F (64, 2), residual / |M|)"""
    B = _basis(sd, key)
    M = np.asarray(M, np.float64)
    F = M @ B @ np.linalg.inv(B.T @ B)
    return F, float(np.abs(M - F @ B.T).max() / max(np.abs(M).max(), 1e-300))


def unpack(sd, key, F):
    return np.asarray(F, np.float64) @ _basis(sd, key).T


def g29_gradients(z, case, sd, tag="grad64"):
    """the gradients of a case of fixture G29 (an open npz) -> {state_dict key: array}, the rank-two ones rebuilt"""
    flat, at, out = z[f"{case}.{tag}"], 0, {}
    for key, w in sd.items():
        shape = np.asarray(w).shape
        if key.endswith(("query.weight", "key.weight")):
            out[key] = unpack(sd, key, flat[at:at + 128].reshape(64, 2))
            at += 128
        else:
            cnt = int(np.prod(shape))
            out[key] = np.asarray(flat[at:at + cnt], np.float64).reshape(shape)
            at += cnt
    assert at == flat.size
    return out
