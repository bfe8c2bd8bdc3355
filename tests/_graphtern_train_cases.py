"""Shared inputs of tests/test_graphtern_train_cpu.py and tests/test_gpu_graphtern_train.py: the configurations, scenes, keep
masks and upstream gradients of the Graph-TERN training tests, all seeded.  Not a test module itself.

A scene's coefficient rows are ~ N(0, 1) and its two position rows ~ N(0, 2), centred over the scene, as the bridge forms
them.  A scene's seed is the first for which the float64 restatement ALONE (tests/_graphtern_train_np.py, no device, under
every mask the case runs) leaves no kept PReLU input within its own step's fp32 bound of 0 and no multi-element gradient
bound at half the tensor's largest entry; tests/test_graphtern_train_cpu.py asserts it, no scene is filtered out."""
import numpy as np

from . import _graphtern_np as GN

# name -> (k, S, n_epcnn): the smallest shapes at which each code path can go wrong
CONFIGS = {"et": (6, 20, 6),     # the ET shape
           "k1": (1, 1, 2),      # one cpcn row: all three row taps clamp; the restconv block straight into the rescconv block
           "s16": (2, 16, 3),    # identity residual in the last block and a middle identity block
           "e8": (2, 3, 8)}      # the most blocks
EXACT_N = (1, 2, 3, 5)
RAGGED_N = (64, 65, 257)         # et only: the wavefront and workgroup edges, all beyond the LDS arena
BEYOND_N = 513                   # above the training cap
LAYOUTS = {"one": [1], "mixed": [3, 1, 5], "empty": [3, 0, 2], "many": [2] * 40}
MASKS = ("null", "ones", "draw", "zeros", "triu")
EDGE_MASKS = ("null", "draw")    # at the arena's edge and at the ragged sizes
PERCENT = 0.8
STATE_SEED = 35
# (config, n[, mask kind]) -> seed of the scene; default 1.  About 1300 n PReLU inputs of O(1) against step bounds of about
# 1e-5: from n = 35 on most seeds leave one inside its band, and at n = 257 (eight on average) each mask has its own scene
SEED = {("et", 5): 3, ("et", 35): 5, ("et", 36): 18, ("et", 64): 52, ("et", 65): 131, ("et", 257, "null"): 589,
        ("et", 257, "draw"): 12329}
LDS_BYTES = GN.LDS_BYTES


def module_kw(name):
    k, S, n_cnn = CONFIGS[name]
    return dict(n_epgcn=1, n_epcnn=n_cnn, input_feat=1, seq_len=k + 2, pred_seq_len=k, n_smpl=S)


def train_arena_limit(name):
    """the largest scene whose training arena (gt_arena_per_ped: the eval arena serves both passes) fits LDS"""
    k, S, _ = CONFIGS[name]
    return GN.dims(k, S, 1)[3]


def sizes_of(name):
    """the scene sizes configuration ``name`` runs, with the masks of each"""
    out = [(n, MASKS) for n in EXACT_N]
    if name == "et":
        lim = train_arena_limit(name)
        out += [(n, EDGE_MASKS) for n in (lim, lim + 1) + RAGGED_N]
    return out


def state_shapes(name):
    """-> {state_dict name: shape} of GraphTERNLight(**module_kw(name)), in the module's order"""
    import eigentrajectory_amd as ET
    return {q: tuple(t.shape) for q, t in ET.GraphTERNLight(**module_kw(name)).state_dict().items()}


def random_state(name):
    """a seeded fp32 state dict of configuration ``name`` that leaves nothing at its default (tests/_graphtern_np.random_state's
    recipe on this file's shapes): weights and biases uniform in +-1/sqrt(fan_in) plus N(0, 0.05) noise, every bias
    non-zero, every PReLU slope different and none 0.25 -- the slope the network never applies too"""
    shapes = state_shapes(name)
    rng = np.random.default_rng([STATE_SEED, sorted(CONFIGS).index(name)])
    n_slopes = sum(1 for key in shapes if GN.is_slope(key))
    slopes = 0.05 + 0.17 * (rng.permutation(n_slopes) + rng.uniform(0.2, 0.8, n_slopes)) / n_slopes
    sd, q = {}, 0
    for key, shape in shapes.items():
        if GN.is_slope(key):
            sd[key] = np.array([slopes[q]], np.float32)
            q += 1
            continue
        fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else int(np.prod(shapes[key[:-4] + "weight"][1:]))
        w = rng.uniform(-1, 1, shape) / np.sqrt(fan_in) + rng.normal(0, 0.05, shape)
        if key.endswith("bias"):
            w = np.where(np.abs(w) < 1e-3, 1e-3, w)
        sd[key] = w.astype(np.float32)
    return sd


def module(name, device=None):
    """a GraphTERNLight of configuration ``name`` holding :func:`random_state`"""
    import torch

    import eigentrajectory_amd as ET
    m = ET.GraphTERNLight(**module_kw(name))
    m.load_state_dict({q: torch.from_numpy(t) for q, t in random_state(name).items()}, strict=True)
    return m if device is None else m.to(device)


def scene(name, n, kind=None):
    """-> u (T, n) fp32 of the case (name, n[, mask kind]): [coefficients; centred last positions], what
    S_obs[0, 0, :, :, 0] holds"""
    k = CONFIGS[name][0]
    rng = np.random.default_rng([SEED.get((name, n, kind), SEED.get((name, n), 1)), n, k])
    u = np.concatenate([rng.normal(0, 1, (k, n)), rng.normal(0, 2, (2, n))]).astype(np.float32)
    u[-2:] -= u[-2:].mean(axis=1, keepdims=True, dtype=np.float32)
    return u


def keep_mask(kind, T, n, seed=5):
    """-> uint8 (4, T, n, n) indexed [r, t, w, v], or None for "null": all ones, a seeded draw that keeps an entry with
    probability 0.8, all zeros (every L = I exactly), or strictly upper triangular (kept where w < v: tells [w, v] from [v, w])"""
    shape = (GN.REL, T, n, n)
    if kind == "null":
        return None
    if kind == "ones":
        return np.ones(shape, np.uint8)
    if kind == "zeros":
        return np.zeros(shape, np.uint8)
    if kind == "triu":
        return np.ascontiguousarray(np.broadcast_to(np.triu(np.ones((n, n), np.uint8), 1), shape))
    if kind == "draw":
        return (~(np.random.default_rng([seed, T, n]).random(shape) > PERCENT)).astype(np.uint8)
    raise KeyError(kind)


def d_out(name, n, seed=0):
    """the upstream gradient (1, k, n, S), N(0, 1) in fp32"""
    k, S, _ = CONFIGS[name]
    return np.random.default_rng([seed, n, k, S]).normal(0, 1, (1, k, n, S)).astype(np.float32)


def split(sizes, name="et", seed=3):
    """-> C_obs (k, N), nrm (4, N) of a scenes-form layout: coefficients ~ N(0, 1), positions ~ N(0, 5), no ties"""
    n = int(np.sum(sizes))
    rng = np.random.default_rng([seed, n, CONFIGS[name][0]])
    return rng.normal(0, 1, (CONFIGS[name][0], n)).astype(np.float32), rng.normal(0, 5, (4, n)).astype(np.float32)


def pack_bits(keep):
    """uint8 0/1 mask -> its bits, packed (fixtures)"""
    return np.packbits(np.asarray(keep, np.uint8).reshape(-1))


def unpack_bits(bits, shape):
    return np.unpackbits(np.asarray(bits, np.uint8))[:int(np.prod(shape))].reshape(shape)


def host_params(S=20, k=6, n_cnn=6, **kw):
    """et_graphtern_params whose every pointer is a (never dereferenced) non-NULL host address"""
    from eigentrajectory_amd import _lib
    p = _lib.GraphTERNParams()
    p.n_epgcn, p.n_epcnn, p.input_feat, p.hidden_feat, p.seq_len, p.pred_seq_len, p.n_smpl = 1, n_cnn, 1, 16, k + 2, k, S
    ly = p.tp_mrgcns[0]
    ly.gcn_w = ly.gcn_b = ly.tcn_prelu = ly.tcn_w = ly.tcn_b = ly.res_w = ly.res_b = ly.prelu = 8
    for j in range(min(n_cnn, _lib.GRAPHTERN_MAX_EPCNN)):
        t = p.tpcnns[j]
        t.tpcn_w = t.tpcn_b = t.tpcn_a = t.cpcn_w = t.cpcn_b = t.cpcn_a = 8
        if j == 0:
            t.rest_w = t.rest_b = 8
        if j + 1 == n_cnn and S != 16:
            t.resc_w = t.resc_b = 8
    for key, val in kw.items():
        setattr(p, key, val)
    return p
