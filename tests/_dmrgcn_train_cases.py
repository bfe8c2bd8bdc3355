"""Shared inputs of tests/test_dmrgcn_train_cpu.py and tests/test_gpu_dmrgcn_train.py: the configurations, scenes, keep
masks and upstream gradients of the DMRGCN training tests, all seeded.  Not a test module itself.

A scene's pair distances straddle the split values of both relations (coefficient rows ~ N(0, 1), so |v_i - v_j| spreads
over 0 .. 4 and the displacement differences over 0 .. 3, around 0.25 .. 1 and 0.5 .. 4).  A scene's seed is the first for
which the float64 restatement ALONE (tests/_dmrgcn_train_np.py, no device, the seeded 0.8 draw) leaves no kept PReLU input
within its own step's fp32 bound of 0; tests/test_dmrgcn_train_cpu.py asserts it, no scene is filtered out."""
import numpy as np

from . import _dmrgcn_np as DN

# name -> (n_tpcnn, S, k): the smallest shapes at which each code path can go wrong
CONFIGS = {"et": (4, 20, 6),     # the ET configuration
           "s1": (2, 1, 1),      # identity residual in the st block, qpp at its floor, the contraction chunked row by row
           "tp1": (1, 3, 2),     # one tpcnn block: the residual block is also the last
           "tp8": (8, 2, 2)}     # the most blocks
EXACT_N = (1, 2, 3, 5)
RAGGED_N = (64, 65, 257)         # et only: the wavefront and workgroup edges, all beyond the LDS arena
BEYOND_N = 513                   # above the training cap
LAYOUTS = {"one": [1], "mixed": [3, 1, 5], "empty": [3, 0, 2], "many": [2] * 40}
MASKS = ("null", "ones", "draw", "zeros", "triu")
PERCENT = 0.8
STATE_SEED = 29
EDGE_MASKS = ("null", "draw")    # at the arena's edge and at the ragged sizes
SEED = {("et", 24): 5, ("et", 25): 5}   # (config, n) -> seed of the scene; default 1
LDS_BYTES = DN.LDS_BYTES


def module_kw(name):
    n_tp, S, k = CONFIGS[name]
    return dict(n_stgcn=1, n_tpcnn=n_tp, input_feat=1, output_feat=S, seq_len=k + 2, pred_seq_len=k, kernel_size=3)


def train_arena_limit(name):
    """the largest scene whose training arena (dt_arena_per_ped: the eval arena + 2 S floats per pedestrian) fits LDS"""
    _, S, k = CONFIGS[name]
    per = DN.dims(k, S, 1)[2] + 2 * S
    return LDS_BYTES // 4 // per


def random_state(name):
    """a seeded fp32 state dict of configuration ``name`` that leaves nothing at its default (tests/_dmrgcn_np.random_state's
    recipe on this file's shapes): weights and biases uniform in +-1/sqrt(fan_in) plus N(0, 0.05) noise, every bias
    non-zero, every PReLU slope different and none 0.25"""
    import eigentrajectory_amd as ET
    shapes = {q: tuple(t.shape) for q, t in ET.SocialDMRGCN(**module_kw(name)).state_dict().items()}
    rng = np.random.default_rng([STATE_SEED, sorted(CONFIGS).index(name)])
    n_slopes = sum(1 for key in shapes if DN.is_slope(key))
    slopes = 0.05 + 0.17 * (rng.permutation(n_slopes) + rng.uniform(0.2, 0.8, n_slopes)) / n_slopes
    sd, q = {}, 0
    for key, shape in shapes.items():
        if DN.is_slope(key):
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
    """a SocialDMRGCN of configuration ``name`` holding :func:`random_state`"""
    import torch

    import eigentrajectory_amd as ET
    m = ET.SocialDMRGCN(**module_kw(name))
    m.load_state_dict({q: torch.from_numpy(t) for q, t in random_state(name).items()}, strict=True)
    return m if device is None else m.to(device)


def scene(name, n):
    """-> v (K, n) fp32 and a (2, K, n, n) fp32 = [A_disp, A_dist] as the bridge forms them, of the case (name, n)"""
    k = CONFIGS[name][2]
    rng = np.random.default_rng([SEED.get((name, n), 1), n, k])
    v = np.concatenate([rng.normal(0, 1, (k, n)), rng.normal(0, 2, (2, n))]).astype(np.float32)
    v[-2:] -= v[-2:].mean(axis=1, keepdims=True, dtype=np.float32)
    return v, DN.adjacency(v)


def keep_mask(kind, K, n, seed=5):
    """-> uint8 (2, 5, K, n, n) indexed [r, b, t, w, v], or None for "null": all ones, a seeded draw that keeps an entry
    with probability 0.8, all zeros (every L = 0), or strictly upper triangular (kept where w < v: tells [w, v] from [v, w])"""
    shape = (2, DN.RB // 2, K, n, n)
    if kind == "null":
        return None
    if kind == "ones":
        return np.ones(shape, np.uint8)
    if kind == "zeros":
        return np.zeros(shape, np.uint8)
    if kind == "triu":
        return np.ascontiguousarray(np.broadcast_to(np.triu(np.ones((n, n), np.uint8), 1), shape))
    if kind == "draw":
        return (~(np.random.default_rng([seed, K, n]).random(shape) > PERCENT)).astype(np.uint8)
    raise KeyError(kind)


def d_out(name, n, seed=0):
    """the upstream gradient (1, S, k, n), N(0, 1) in fp32"""
    _, S, k = CONFIGS[name]
    return np.random.default_rng([seed, n, k, S]).normal(0, 1, (1, S, k, n)).astype(np.float32)


def split(sizes, name="et", seed=3):
    """-> C_obs (k, N), nrm (4, N) of a scenes-form layout (tests/_dmrgcn_np.synthetic_split)"""
    return DN.synthetic_split(sizes, seed, CONFIGS[name][2])


def pack_bits(keep):
    """uint8 0/1 mask -> its bits, packed (fixtures)"""
    return np.packbits(np.asarray(keep, np.uint8).reshape(-1))


def unpack_bits(bits, shape):
    return np.unpackbits(np.asarray(bits, np.uint8))[:int(np.prod(shape))].reshape(shape)


def host_params(S=20, k=6, n_tp=4, **kw):
    """et_dmrgcn_params whose every pointer is a (never dereferenced) non-NULL host address"""
    from eigentrajectory_amd import _lib
    p = _lib.DMRGCNParams()
    p.n_stgcn, p.n_tpcnn, p.input_feat, p.output_feat, p.seq_len, p.pred_seq_len, p.kernel_size = 1, n_tp, 1, S, k + 2, k, 3
    for r in range(2):
        for b, val in enumerate(DN.SPLIT[r]):
            p.split[r][b] = val
    ly = p.st_dmrgcns[0]
    for r in range(2):
        ly.gcn_w[r] = ly.gcn_b[r] = 8
    ly.tcn_prelu = ly.tcn_w = ly.tcn_b = ly.prelu = 8
    if S != 1:
        ly.res_w = ly.res_b = 8
    for j in range(min(n_tp, _lib.DMRGCN_MAX_TPCNN)):
        t = p.tpcnns[j]
        for m in range(2):
            t.conv_w[m] = t.conv_b[m] = t.conv_a[m] = 8
        t.gta_w = t.gta_b = t.gta_a = 8
        if j == 0:
            t.res_w = t.res_b = 8
    for key, val in kw.items():
        setattr(p, key, val)
    return p
