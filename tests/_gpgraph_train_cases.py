"""Shared inputs of tests/test_gpgraph_train_cpu.py and tests/test_gpu_gpgraph_train.py: the configurations, weights, scenes
and upstream gradients of the GP-Graph-SGCN training tests, all seeded.  Not a test module itself.

The base's weights are tests/_sgcn_np.random_state's with the temporal embedding widened to (64, 2): column 1 (coefficients)
is that state's column, column 0 (position, values 1..T) a seeded draw divided by T, so that the temporal scores stay of the
size they have with one channel.  The wrapper's: group_cnn ~ N(0, GROUP_SPREAD) (distances of order 1: with tau = 0.1 a fair
share of the pairs then lies within a few tau of the threshold, where the soft assignment has a gradient), the mix as torch
would initialise it plus noise, its PReLU slope not 0.25.

The threshold belongs to the CASE: ``th`` lies between the m-th and the (m + 1)-th smallest pair distance of the float64
restatement (tests/_gpgraph_np.distances), m = max(1, n // 2) -- about n / 2 close pairs, which leaves 1 < G < n for every
n >= 3 (asserted in tests/test_gpgraph_train_cpu.py): at their midpoint, the largest margin a threshold between the two can
have, but no further than 1.5 tau above the m-th, so that even a scene of two has a pair where the sigmoid is not saturated
(sigmoid(1.5) = 0.82).  No pair is undecided (the margin is of order tau, the band 1e-5 th).  A layout of several scenes takes the same rule on all its scenes' pairs together.  The
scenes are tests/_sgcn_np.py's synthetic ones; a seed is the first for which the float64 restatement alone keeps the undecided
mask and PReLU decisions within CAP_SCENE of each pass (the exact cases: none)."""
import numpy as np

from . import _gpgraph_np as GN
from . import _sgcn_np as SN

EXACT_N = (1, 2, 3, 5)
EXACT_CONFIGS = ("k1", "k2_wide", "et")
RAGGED = [("et", n) for n in (17, 63, 64, 65, 130)] + [("deep", 65), ("kmax", 65)]
LAYOUTS = {"edge": "et", "many": "k1"}
SEED = {}                                 # (config, n) -> seed of the scene; default 1
LAYOUT_SEED = {"edge": 1, "many": 3}
GROUP_SPREAD = 0.1
TAU = 0.1
BASE = "baseline_model."


def seed_of(name, n):
    return SEED.get((name, n), 1)


def scene(name, n):
    """-> (v_abs (T, n), v_rel (2, T, n)) fp32 of the single-scene case (name, n), as the gpgraphsgcn bridge builds them"""
    C_obs, nrm = SN.synthetic_split([n], seed_of(name, n) + 1000 * n, SN.CONFIGS[name]["k"])
    return GN.bridge_input(SN.scene_input(C_obs, nrm, 0, n))


def layout(which):
    """-> (config, sizes, C_obs (k, N), nrm (4, N)) of a scenes-form layout"""
    name = LAYOUTS[which]
    sizes = SN.LAYOUTS[which]
    C_obs, nrm = SN.synthetic_split(sizes, LAYOUT_SEED[which], SN.CONFIGS[name]["k"])
    return name, sizes, C_obs, nrm


def d_out(name, n, seed=0):
    """the upstream gradient (out_dims, pred_len, n), N(0, 1) in fp32: the layout of the graph form's output"""
    c = SN.CONFIGS[name]
    return np.random.default_rng([seed, n, c["k"], 30]).normal(0, 1, (c["S"], c["k"], n)).astype(np.float32)


def state(name, th=1.0):
    """the whole GPGraph's fp32 state dict of CONFIGS[name], in the module's order"""
    c = SN.CONFIGS[name]
    k, S, T = c["k"], c["S"], c["k"] + 2
    rng = np.random.default_rng([SN.STATE_SEED, c["seed"], sorted(SN.CONFIGS).index(name), 30])
    sd = {}
    for key, w in SN.random_state(name).items():
        if key == SN.SWA + "temporal_attention.embedding.weight":
            pos = (rng.uniform(-1, 1, (64, 1)) / np.sqrt(2) + rng.normal(0, c["spread"], (64, 1))) / T
            w = np.concatenate([pos, w], axis=1).astype(np.float32)
        sd[BASE + key] = w
    Sk = S * k
    sd["group_gen.th"] = np.array([th], np.float32)
    sd["group_gen.group_cnn.0.weight"] = rng.normal(0, GROUP_SPREAD, (8, 1, 3, 1)).astype(np.float32)
    sd["group_gen.group_cnn.0.bias"] = rng.normal(0, GROUP_SPREAD, (8,)).astype(np.float32)
    sd["group_mix.st_gcns_mix.0.weight"] = np.array([0.31], np.float32)
    sd["group_mix.st_gcns_mix.1.weight"] = (rng.uniform(-1, 1, (Sk, 3 * Sk, 1, 1)) / np.sqrt(3 * Sk)
                                            + rng.normal(0, 0.02, (Sk, 3 * Sk, 1, 1))).astype(np.float32)
    b = rng.uniform(-1, 1, (Sk,)) / np.sqrt(3 * Sk)
    sd["group_mix.st_gcns_mix.1.bias"] = np.where(np.abs(b) < 1e-3, 1e-3, b).astype(np.float32)
    return sd


def threshold_of(dists):
    """``dists``: the (n, n) float64 distance matrices of a case's scenes -> th (fp32) by the rule above (1.0 without a pair)"""
    d = np.sort(np.concatenate([x[np.tril(np.ones(x.shape, bool), -1)] for x in dists]))
    if d.size == 0:
        return np.float32(1.0)
    m = max(1, sum(x.shape[0] for x in dists) // 2)
    if m >= d.size:
        return np.float32(d[-1] + 1.5 * TAU)
    return np.float32(min(0.5 * (d[m - 1] + d[m]), d[m - 1] + 1.5 * TAU))


def case_state(name, v_abs_list):
    """the state of configuration ``name`` with the threshold of the scenes ``v_abs_list`` ((T, n) each)"""
    sd = state(name)
    _, rest = GN.split_state(sd)
    sd["group_gen.th"] = np.array([threshold_of([GN.distances(rest, v) for v in v_abs_list])], np.float32)
    return sd


def module(name, device=None):
    import torch

    from eigentrajectory_amd.gpgraph import GPGraph
    from eigentrajectory_amd.sgcn import SGCN
    c = SN.CONFIGS[name]
    base = SGCN(position_channel=True, **SN.module_cfg(name))
    m = GPGraph(base, in_channels=1, out_channels=c["S"], obs_seq_len=c["k"] + 2, pred_seq_len=c["k"])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state(name).items()})
    return m if device is None else m.to(device)


def set_threshold(m, sd):
    """write a case's threshold into the module (the kernels read it in place)"""
    import torch
    with torch.no_grad():
        m.group_gen.th.fill_(float(sd["group_gen.th"][0]))
    return m


def within_caps(figs, pairs, exact=False):
    """the seed conditions on :func:`tests._gpgraph_train_np.run`'s ``decisions`` (per pass) and ``pairs``"""
    if pairs["undecided"]:
        return False
    for fig in figs:
        for kind in ("mask", "prelu"):
            f = fig[kind]
            if exact and f["undecided"]:
                return False
            if f["undecided"] > SN.CAP_SCENE * f["entries"]:
                return False
    return True


def _basis(sd, key):
    p = key.rsplit(".", 2)[0] + ".embedding."
    w = np.asarray(sd[p + "weight"], np.float64)
    return np.concatenate([w, np.asarray(sd[p + "bias"], np.float64)[:, None]], 1)   # (64, 2) spatial, (64, 3) temporal


def pack(sd, key, M):
    """fixture G30: the (64, 64) gradient of a query.weight / key.weight, M = F B^T with B the embedding's columns and bias
    -> (F (64, 2 or 3), residual / |M|)"""
    B = _basis(sd, key)
    M = np.asarray(M, np.float64)
    F = M @ B @ np.linalg.inv(B.T @ B)
    return F, float(np.abs(M - F @ B.T).max() / max(np.abs(M).max(), 1e-300))


def unpack(sd, key, F):
    return np.asarray(F, np.float64) @ _basis(sd, key).T


def pack_mix(d_out, M):
    """fixture G30: the gradient of group_mix.st_gcns_mix.1.weight, M (S k, 3 S k) = G A^T with G = d_out as (S k, n) -> (A
    (3 S k, n), residual / |M|)"""
    G = np.asarray(d_out, np.float64).reshape(-1, np.asarray(d_out).shape[-1])
    M = np.asarray(M, np.float64).reshape(G.shape[0], -1)
    A = (np.linalg.pinv(G) @ M).T
    return A, float(np.abs(M - G @ A.T).max() / max(np.abs(M).max(), 1e-300))


def g30_gradients(z, case, sd, tag="grad64"):
    """the gradients of a case of fixture G30 (an open npz) -> {state_dict key: array}, the low-rank ones rebuilt"""
    flat, at, out = z[f"{case}.{tag}"], 0, {}
    G = np.asarray(z[f"{case}.d_out"], np.float64).reshape(-1, z[f"{case}.d_out"].shape[-1])
    for key, w in sd.items():
        shape = np.asarray(w).shape
        if key.endswith(("query.weight", "key.weight")):
            r = _basis(sd, key).shape[1]
            out[key] = unpack(sd, key, flat[at:at + 64 * r].reshape(64, r))
            at += 64 * r
        elif key == "group_mix.st_gcns_mix.1.weight":
            cnt = 3 * G.shape[0] * G.shape[1]
            out[key] = (G @ np.asarray(flat[at:at + cnt], np.float64).reshape(3 * G.shape[0], G.shape[1]).T).reshape(shape)
            at += cnt
        else:
            cnt = int(np.prod(shape))
            out[key] = np.asarray(flat[at:at + cnt], np.float64).reshape(shape)
            at += cnt
    assert at == flat.size
    return out
