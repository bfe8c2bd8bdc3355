"""fp64 numpy restatement of GP-Graph-STGCNN's eval-mode forward (baseline/gpgraphstgcnn: model_groupwrapper.py
GPGraph.forward around model_baseline.py's social_stgcnn), the arithmetic csrc/et_gpgraph_stgcnn.hip is checked against, and
the shared inputs of the tests that run the kernels across their family (tests/test_gpgraph_stgcnn_cpu.py,
tests/test_gpu_gpgraph_stgcnn_shapes.py).  Not a test module itself.  The grouping (distances, merge, compact) is
tests/_gpgraph_np.py's, the network's pieces (BatchNorm, PReLU, the 3x3 convolutions) are tests/_stgcnn_np.py's.

The base is the ORIGINAL Social-STGCNN: its gcn convolves to S channels and contracts time row t with its own Laplacian
(``einsum('nctv,tvw->nctw')``), where ET-STGCNN's (baseline/stgcnn/model.py, tests/_stgcnn_np.forward) convolves to S K
channels and contracts over all rows -- so :func:`base_forward` restates the st_gcn block itself and shares the rest.

``GPGraph.forward(v_abs, v_rel)`` takes two graphs: the distances and the decisions come from v_abs; pass 0, the soft
assignment v' = (v_rel - v_soft) + v_soft and the group means come from v_rel.  The bridge hands over one tensor for both;
:func:`grouping` and :func:`forward` take them separately (``v_rel`` defaults to ``v_abs``).

Three kinds of hard decision are taken: ``d <= th`` on every pair (handled as in tests/_gpgraph_np.py: BAND_D, TOL_D),
``a == 0`` in the inverse-distance kernel, and the conditioning of ``1 / |u_i - u_j|``.  For the last two, :func:`forward`
can be fed the fp32 inputs of passes 1 and 2 an implementation used (``inputs=``), which are checked on their own by
:func:`check_inputs` against bounds that follow from fp32 arithmetic.  ``dtype=np.float32`` runs the same statements of the
three passes and the mix with every array and accumulator in fp32: the restatement's own arithmetic error, the evidence for
the tolerance and nothing else.

Across the family (the second half of the file): CONFIGS (n_stgcnn, n_txpcnn, S, k), the per-time-row arena
(:func:`arena_per_ped`, :func:`lds_max_n`) and the workspace (:func:`workspace_floats`) restated from the header comments
of csrc/et_stgcnn_core.inl and csrc/et_gpgraph_stgcnn.hip, the seeded weights (:func:`random_state`, :func:`module`), the
scene layouts (LAYOUTS, USED, :func:`layout_case`), the single graph-form scenes with the bridge's and with an odd v_rel
(:func:`graph_case`), the two extreme thresholds (:func:`extreme_case`) and the case thresholds (:func:`threshold_of`)."""
import functools

import numpy as np

from . import _gpgraph_np as GN
from . import _sgcn_np as SN
from . import _stgcnn_np as ST

TOL = 1e-5             # outputs: of the largest entry
TOL_D = GN.TOL_D
BAND_D = GN.BAND_D
COND = 1e-6            # a scene whose reference fp32 run is within this of its fp64 run is *well conditioned*
_f = GN._f


def laplacian_row(u, same=None, dtype=np.float64):
    """u (N,) one time row -> L (N, N) = I - D a_hat D, a_hat = (1/|u_i - u_j|, 0 where equal) * same + I: the mask
    multiplies a_inv BEFORE + I, so it enters the degree as well"""
    u = np.asarray(u, dtype)
    one, eye = dtype(1), np.eye(len(u), dtype=dtype)
    dist = np.abs(u[:, None] - u[None, :])
    with np.errstate(divide="ignore"):
        a_hat = np.where(dist == 0, dtype(0), one / dist)
    if same is not None:
        a_hat = a_hat * np.asarray(same, dtype)
    a_hat += eye
    deg = a_hat.sum(axis=1, dtype=dtype)
    # float32: two correctly rounded operations (what the kernel does); float64: the reference's pow
    d = deg ** -0.5 if dtype is np.float64 else one / np.sqrt(deg)
    return eye - d[:, None] * a_hat * d[None, :]


def n_layers(sd):
    n_st = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("st_gcns."))
    n_tp = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("tpcnns."))
    return n_st, n_tp


def base_forward(sd, v, same=None, dtype=np.float64, variant=()):
    """model_baseline.py's social_stgcnn.forward on v (K, N) with a = laplacian(v, mask = same) -> (S, k, N).  ``variant``:
    deliberately wrong statements, for the checks that the seeded weights would show them (tests/test_gpgraph_stgcnn_cpu.py):
    "no_identity" drops the identity residual of a block, "first_row" contracts every time row with L[0]"""
    sd = {k: np.asarray(val, dtype) for k, val in sd.items()}
    n_st, n_tp = n_layers(sd)
    x = np.asarray(v, dtype)[None]                                         # (C = 1, K, N)
    K, N = x.shape[1], x.shape[2]
    L = np.stack([laplacian_row(r, same, dtype) for r in np.asarray(v, dtype)])   # (K, N, N)
    if "first_row" in variant:
        L = np.broadcast_to(L[:1], L.shape)
    for i in range(n_st):
        pre = f"st_gcns.{i}"
        W = sd[f"{pre}.gcn.conv.weight"][:, :, 0, 0]                       # (S, Cin)
        x1 = np.einsum("oc,ctv->otv", W, x) + sd[f"{pre}.gcn.conv.bias"][:, None, None]
        y = np.einsum("ctv,tvw->ctw", x1, L)
        S = y.shape[0]
        y = ST._prelu(ST._bn(y, sd, f"{pre}.tcn.0", (-1, 1, 1)), sd[f"{pre}.tcn.1.weight"])
        tw, tb = sd[f"{pre}.tcn.2.weight"][:, :, :, 0], sd[f"{pre}.tcn.2.bias"]
        yp = np.zeros((S, K + 2, N), dtype)
        yp[:, 1:-1] = y
        z = tb[:, None, None] + sum(np.einsum("oc,ctv->otv", tw[:, :, dt], yp[:, dt:dt + K]) for dt in range(3))
        z = ST._bn(z, sd, f"{pre}.tcn.3", (-1, 1, 1))
        if f"{pre}.residual.0.weight" in sd:
            r = np.einsum("oc,ctv->otv", sd[f"{pre}.residual.0.weight"][:, :, 0, 0], x) + \
                sd[f"{pre}.residual.0.bias"][:, None, None]
            r = ST._bn(r, sd, f"{pre}.residual.1", (-1, 1, 1))
        else:
            r = np.zeros_like(x) if "no_identity" in variant else x
        x = ST._prelu(z + r, sd[f"{pre}.prelu.weight"])
    S = x.shape[0]
    t = x.reshape(K, S, N)                                                 # the reference's view, not a permute
    t = ST._prelu(ST._conv33(t, sd["tpcnns.0.weight"], sd["tpcnns.0.bias"]), sd["prelus.0.weight"])
    for j in range(1, n_tp - 1):
        t = ST._prelu(ST._conv33(t, sd[f"tpcnns.{j}.weight"], sd[f"tpcnns.{j}.bias"]), sd[f"prelus.{j}.weight"]) + t
    t = ST._conv33(t, sd["tpcnn_ouput.weight"], sd["tpcnn_ouput.bias"])  # (k, S, N)
    assert t.dtype == dtype
    return t.reshape(S, t.shape[0], N)


def grouping(rest, v_abs, close=None, v_rel=None):
    """v_abs, v_rel (T, N) -> (dist, indices, v' (T, N), group means (T, G)) in fp64: the distances and the decisions from
    v_abs, v' and the means from v_rel (default: v_abs); ``close`` overrides the decisions d <= th"""
    v_abs = _f(v_abs)
    v = v_abs if v_rel is None else _f(v_rel)
    d = GN.distances(rest, v_abs)
    th = GN.threshold(rest)
    indices = GN.compact(GN.merge_rows(d <= th if close is None else np.asarray(close, bool)))
    sig = 1.0 / (1.0 + np.exp((d - th) / 0.1))
    v_soft = v @ (sig / sig.sum(axis=0, keepdims=True))
    v2 = (v - v_soft) + v_soft
    return d, indices, v2, group_means(v2, indices)


def group_means(v2, indices):
    G = int(indices.max()) + 1
    onehot = (np.asarray(indices)[:, None] == np.arange(G)[None]).astype(np.float64)
    return (_f(v2) @ onehot) / onehot.sum(axis=0)


def mix(rest, stack, dtype=np.float64):
    S, k, N = stack[0].shape
    x = np.concatenate(stack, axis=0).reshape(3 * S * k, N).astype(dtype)
    w = np.asarray(rest["group_mix.st_gcns_mix.1.weight"], dtype)[:, :, 0, 0]
    a = dtype(np.asarray(rest["group_mix.st_gcns_mix.0.weight"]).reshape(-1)[0])
    y = w @ np.where(x > 0, x, a * x) + np.asarray(rest["group_mix.st_gcns_mix.1.bias"], dtype)[:, None]
    out = (stack[0] + stack[1] + stack[2]) / dtype(3) + y.reshape(S, k, N)
    assert out.dtype == dtype
    return out


def forward(sd, v, inputs=None, indices=None, v_rel=None, dtype=np.float64, variant=()):
    """v = v_abs (T, N), ``v_rel`` (T, N) or None: v_abs -> dict: out (S, k, N), outs [(S, k, n_m)] * 3 (pass 1 on the G
    group means, before the unpooling), indices, dist, inputs (the group means and v' of this run).  ``inputs`` = (group
    means (T, G), v' (T, N)) with ``indices``: passes 1 and 2 run on THESE values (an implementation's own fp32 ones)
    instead of this module's.  ``dtype``: of the three passes and the mix (the grouping stays fp64)."""
    base, rest = GN.split_state(sd)
    rel = v if v_rel is None else v_rel
    d, own_idx, v2, means = grouping(rest, v, v_rel=v_rel)
    if inputs is not None:
        means, v2 = _f(inputs[0]), _f(inputs[1])
        own_idx = np.asarray(indices)
    same = own_idx[:, None] == own_idx[None, :]
    outs = [base_forward(base, rel, None, dtype, variant), base_forward(base, means, None, dtype, variant),
            base_forward(base, v2, same, dtype, variant)]
    out = mix(rest, [outs[0], outs[1][:, :, own_idx], outs[2]], dtype)
    return {"out": out, "outs": outs, "indices": own_idx, "dist": d, "n_groups": int(own_idx.max()) + 1,
            "inputs": (means, v2)}


# ---------------------------------------------------------------------------------------------- ties and input bounds
def ties(x):
    """x (T, n) fp32 -> (T, n, n) bool: the exact off-diagonal ties of every row (where a == 0 makes a_inv 0)"""
    x = np.asarray(x, np.float32)
    return (x[:, :, None] == x[:, None, :]) & ~np.eye(x.shape[1], dtype=bool)[None]


def ties_robust(v, v_group, v_intra):
    """every exact off-diagonal tie of the three graph inputs is at value 0.0 ((0 - s) + s == 0 for any s) -- or, in v and v',
    between two pedestrians whose whole columns of v are identical (their distances, sig_norm columns and v' columns are then
    computed from identical values by identical operations)"""
    v = np.asarray(v, np.float32)
    twins = (v[:, :, None] == v[:, None, :]).all(axis=0)
    for x, allowed in ((v, twins), (v_group, None), (v_intra, twins)):
        x = np.asarray(x, np.float32)
        t = ties(x) & (np.broadcast_to(x[:, :, None], (x.shape[0], x.shape[1], x.shape[1])) != 0)
        if allowed is not None:
            t &= ~allowed[None]
        if t.any():
            return False
    return True


def check_inputs(v, v2, means, indices):
    """the bounds that fp32 arithmetic gives the inputs of passes 1 and 2 (v' and the group means as an implementation
    computed them, fp32; v: the graph they are formed from, v_rel) -> the two largest ratios error / bound (both must be <= 1):
      |v'[t,j] - v[t,j]| <= 3 * 2^-23 * max_i |v[t,i]|        (v_soft is a convex combination of the row)
      |mean_g - fp64 mean of THE GIVEN v' over THE GIVEN indices| <= (count_g + 1) * 2^-24 * max |v'[t,.]|"""
    v, v2, means, indices = _f(v), _f(v2), _f(means), np.asarray(indices)
    b1 = 3 * 2.0 ** -23 * np.abs(v).max(axis=1, keepdims=True)
    r1 = float((np.abs(v2 - v) / np.maximum(b1, 1e-300)).max())
    counts = np.bincount(indices)
    b2 = (counts[None, :] + 1) * 2.0 ** -24 * np.abs(v2).max(axis=1, keepdims=True)
    r2 = float((np.abs(means - group_means(v2, indices)) / np.maximum(b2, 1e-300)).max())
    return r1, r2


def rel_err(got, ref):
    ref = _f(ref)
    return float(np.abs(_f(got) - ref).max() / max(np.abs(ref).max(), 1e-30))


# ------------------------------------------------------------------------------------------------- across the family
# (n_stgcnn, n_txpcnn, S, k); T = k + 2.  What each is there for: tests/test_gpu_gpgraph_stgcnn_shapes.py's docstring
CONFIGS = {"et": (1, 5, 20, 6), "tp1": (1, 1, 20, 6), "s1": (1, 2, 1, 1), "j17": (2, 3, 16, 4), "deep": (8, 8, 7, 3),
           "wide": (2, 5, 64, 6), "max": (2, 4, 64, 32)}
ARENA = {"et": (456, 33), "tp1": (352, 43), "s1": (18, 853), "j17": (306, 50), "deep": (120, 128), "wide": (1560, 9),
         "max": (6630, 2)}   # floats per pedestrian, LDS limit: computed by hand, asserted against arena_per_ped / lds_max_n
STATE_SEED = 34
GROUP_SPREAD, TAU = 0.1, 0.1
MAX_N = 512            # ET_SGCN_MAX_N
LDS_FLOATS = 60 * 1024 // 4
MAX_SCENE = {"max": 17}  # the fp64 restatement of S k = 2048 stays quick on scenes of at most 17


def arena_per_ped(n_st, n_tp, S, k):
    """floats per pedestrian of a virtual scene's arena with the per-time-row gcn (csrc/et_stgcnn_core.inl: dims_of(p, true),
    arena_per_ped): u and d (K each), x and y (S K each) and q, K rows of C_in + 1 contracted rows each (C_in = S for a
    second st_gcn, else 1), raised to k S by the tpcnn residual loop's pong buffer (n_txpcnn >= 3)"""
    K = k + 2
    q = K * ((S if n_st > 1 else 1) + 1)
    if n_tp >= 3:
        q = max(q, k * S)
    return 2 * K + 2 * S * K + q


def lds_max_n(n_st, n_tp, S, k):
    """the largest virtual scene whose arena fits the 60 KB of LDS a workgroup of gps_passes takes"""
    return LDS_FLOATS // arena_per_ped(n_st, n_tp, S, k)


def _up4(x):
    return (x + 3) // 4 * 4


def workspace_offsets(config, N, sum_n2, n_scenes):
    """the workspace of csrc/et_gpgraph_stgcnn.hip (gslay_of), in floats, every block rounded up to 4: the stack offsets
    (int64 [3 S]), the node counts (int32 [3 S]), the group indices (int32 [N]), v_abs (T, N), group_cnn's features (8, T, N),
    dist and sig_norm (sum n^2 each), the passes' inputs (3, T N), their outputs (k, 3 N, S), and -- only when the largest
    scene the caller may have (at most N rows, MAX_N, n^2 <= sum n^2) does not fit LDS -- per * 3 N floats of arenas
    -> ({block: offset}, total)"""
    n_st, n_tp, S, k = config
    T = k + 2
    cap = min(N, MAX_N)
    while cap > 0 and cap * cap > sum_n2:
        cap -= 1
    per = arena_per_ped(*config)
    arena = 0 if per * cap <= LDS_FLOATS else per * 3 * N
    at, where = 0, {}
    for block, size in (("sq", 2 * 3 * n_scenes), ("vn", 3 * n_scenes), ("gidx", N), ("va", T * N), ("feat", 8 * T * N),
                        ("dist", sum_n2), ("sn", sum_n2), ("in", 3 * T * N), ("po", k * 3 * N * S), ("arena", arena)):
        where[block] = at
        at = _up4(at + size)
    return where, at


def workspace_floats(config, N, sum_n2, n_scenes):
    return workspace_offsets(config, N, sum_n2, n_scenes)[1]


def module(name, device=None, load=True):
    """GPGraph around the per-time-row SocialSTGCNN of CONFIGS[name], with :func:`random_state`'s weights"""
    import torch

    from eigentrajectory_amd.gpgraph import GPGraph
    from eigentrajectory_amd.stgcnn import SocialSTGCNN
    n_st, n_tp, S, k = CONFIGS[name]
    base = SocialSTGCNN(graph_per_time_row=True, **ST.module_kw(n_st, n_tp, S, k))
    m = GPGraph(base, in_channels=1, out_channels=S, obs_seq_len=k + 2, pred_seq_len=k)
    if load:
        m.load_state_dict({key: torch.from_numpy(v) for key, v in random_state(name).items()}, strict=True)
    return m if device is None else m.to(device)


@functools.lru_cache(maxsize=None)
def random_state(name):
    """the whole GPGraph's fp32 state dict of CONFIGS[name], in the module's order, a function of the name alone: the base's
    tensors through tests/_stgcnn_np.random_state (nothing at a default), the wrapper's as tests/_gpgraph_train_cases.state
    draws them (group_cnn ~ N(0, GROUP_SPREAD), the mix at torch's initial scale plus noise, its slope 0.31), th = 1 (the
    threshold belongs to the case: :func:`with_threshold`).  Nothing may edit the result."""
    idx = sorted(CONFIGS).index(name)
    n_st, n_tp, S, k = CONFIGS[name]
    m = module(name, load=False)
    base = ST.random_state(m.baseline_model, [STATE_SEED, idx])
    rng = np.random.default_rng([STATE_SEED, idx, 30])
    Sk = S * k
    rest = {"group_gen.th": np.array([1.0], np.float32),
            "group_gen.group_cnn.0.weight": rng.normal(0, GROUP_SPREAD, (8, 1, 3, 1)).astype(np.float32),
            "group_gen.group_cnn.0.bias": rng.normal(0, GROUP_SPREAD, (8,)).astype(np.float32),
            "group_mix.st_gcns_mix.0.weight": np.array([0.31], np.float32),
            "group_mix.st_gcns_mix.1.weight": (rng.uniform(-1, 1, (Sk, 3 * Sk, 1, 1)).astype(np.float32) / np.float32(np.sqrt(3 * Sk))
                                               + rng.normal(0, 0.02, (Sk, 3 * Sk, 1, 1)).astype(np.float32))}
    b = rng.uniform(-1, 1, (Sk,)) / np.sqrt(3 * Sk)
    rest["group_mix.st_gcns_mix.1.bias"] = np.where(np.abs(b) < 1e-3, 1e-3, b).astype(np.float32)
    sd = {}
    for key in m.state_dict():
        sd[key] = base[key[len("baseline_model."):]] if key.startswith("baseline_model.") else rest[key]
    return sd


def with_threshold(name, th):
    sd = dict(random_state(name))
    sd["group_gen.th"] = np.array([th], np.float32)
    return sd


def set_threshold(m, th):
    """write a case's threshold into the module in place (the kernels read it on the device)"""
    import torch
    with torch.no_grad():
        m.group_gen.th.fill_(float(th))
    return m


def threshold_of(dists):
    """the rule of tests/_gpgraph_train_cases.threshold_of on ONE scene's (n, n) fp64 distances: between the m-th and the
    (m + 1)-th smallest pair distance, m = max(1, n // 2), at their midpoint but no further than 1.5 tau above the m-th"""
    from ._gpgraph_train_cases import threshold_of as rule
    return rule([dists])


def _rest(name):
    return GN.split_state(random_state(name))[1]


def rescaled(name, sizes, C_obs, nrm):
    """one threshold for a layout of several scenes: th is the rule's of the LARGEST scene, and every other scene with a
    pair is scaled about its first pedestrian (C_obs columns and the two position rows of nrm alike) by th / (its own
    rule's threshold) -- the distances depend on differences of columns only and are 1-homogeneous in them, so the rule
    then holds on every scene of the layout for the one th the kernels read.  -> (C_obs, nrm, th) fp32"""
    rest = _rest(name)
    C_obs, nrm = C_obs.copy(), nrm.copy()
    k = C_obs.shape[0]
    scenes = list(SN.scenes_of(sizes, C_obs, nrm))
    own = {}
    for s, lo, n, v in scenes:
        if n >= 2:
            own[s] = float(threshold_of(GN.distances(rest, v)))
    if not own:
        return C_obs, nrm, np.float32(1.0)
    big = max(own, key=lambda s: (sizes[s], -s))
    th = np.float32(own[big])
    for s, lo, n, v in scenes:
        if s in own and s != big:
            f = float(th) / own[s]
            for a in (C_obs, nrm[:2]):
                c = a[:, lo:lo + 1].astype(np.float64)
                a[:, lo:lo + n] = (c + f * (a[:, lo:lo + n].astype(np.float64) - c)).astype(np.float32)
    return C_obs, nrm, th


def layout_sizes(name, layout):
    L = lds_max_n(*CONFIGS[name])
    if layout == "edge":
        return (1, 2, 3, 0, 63, 64, 65, 2) if L > MAX_N else (1, 2, 3, 0, L - 1, L, L + 1, 2)
    return {"big": (257,), "limit": (MAX_N,), "many": tuple((1, 2, 3)[i % 3] for i in range(300)), "nan": (9, 20, 5)}[layout]


LAYOUTS = ("edge", "big", "limit", "many")
USED = {"et": ("edge", "big", "many"), "tp1": ("edge",), "s1": ("edge", "big", "limit", "many"), "j17": ("edge", "big"),
        "deep": ("edge", "limit"), "wide": ("edge",), "max": ("edge",)}
GRAPH_SIZES = ("g3", "g13", "gL1")   # graph-form scenes of 3, 13 and L + 1 (s1: L + 1 is above MAX_N; max: 3 is L + 1)
ODD = ("g3", "g13")                  # ... also run with a v_rel that no bridge builds
EXTREMES = {"s1": 300, "j17": 51}
# the first seed that meets every condition of tests/test_gpgraph_stgcnn_cpu.py, per (configuration, layout or graph scene)
# (et on 257: with seed 1 pedestrian 256, the only one above 255, is merged into a group that straddles index 256 -- as it is
# at s1 and j17; seed 2 leaves it alone, so that a label >= 256 survives in one scene of 257 as well)
SEEDS = {("et", "big"): 2}


def seed_of(name, which):
    return SEEDS.get((name, which), 1)


def graph_n(name, which):
    L = lds_max_n(*CONFIGS[name])
    n = {"g3": 3, "g13": 13, "gL1": L + 1}[which]
    return n if n <= min(MAX_N, MAX_SCENE.get(name, MAX_N)) else None


def graph_cases(name):
    """-> [(which, odd)] of the graph-form cases of a configuration"""
    res = []
    for which in GRAPH_SIZES:
        n = graph_n(name, which)
        if n is None or (which == "gL1" and n == 3):
            continue
        res.append((which, False))
        if which in ODD:
            res.append((which, True))
    return res


@functools.lru_cache(maxsize=None)
def layout_case(name, layout):
    """-> (sizes, C_obs (k, N), nrm (4, N), th) of a scenes-form layout of configuration ``name``"""
    k = CONFIGS[name][3]
    sizes = layout_sizes(name, layout)
    C_obs, nrm = SN.synthetic_split(sizes, [seed_of(name, layout), sorted(CONFIGS).index(name), len(sizes), sum(sizes)], k)
    C_obs, nrm, th = rescaled(name, sizes, C_obs, nrm)
    return sizes, C_obs, nrm, th


@functools.lru_cache(maxsize=None)
def graph_case(name, which, odd=False):
    """-> (v_abs (T, n), v_rel (T, n), th) of a single graph-form scene: v_abs as the bridge builds it, v_rel the same
    tensor (``odd`` False) or a seeded draw of its own, N(0, 1) per entry, that no bridge builds"""
    k = CONFIGS[name][3]
    n = graph_n(name, which)
    idx = sorted(CONFIGS).index(name)
    C_obs, nrm = SN.synthetic_split([n], [seed_of(name, which), idx, n], k)
    v_abs = SN.scene_input(C_obs, nrm, 0, n)
    th = threshold_of(GN.distances(_rest(name), v_abs))
    v_rel = v_abs
    if odd:
        v_rel = np.random.default_rng([seed_of(name, which), idx, n, 7]).normal(0, 1, v_abs.shape).astype(np.float32)
    return v_abs, v_rel, th


@functools.lru_cache(maxsize=None)
def extreme_case(name, above):
    """one scene of EXTREMES[name] pedestrians with th below every pair distance (G = n: the same-group matrix is I and the
    intra-group Laplacian I - I = 0) or above every one (G = 1: pass 1 runs on a single node) -> (sizes, C_obs, nrm, th)"""
    k = CONFIGS[name][3]
    n = EXTREMES[name]
    C_obs, nrm = SN.synthetic_split([n], [seed_of(name, "extreme"), sorted(CONFIGS).index(name), n], k)
    d = GN.distances(_rest(name), SN.scene_input(C_obs, nrm, 0, n))
    low = d[np.tril(np.ones((n, n), bool), -1)]
    return (n,), C_obs, nrm, np.float32(2.0 * low.max() if above else 0.5 * low.min())


@functools.lru_cache(maxsize=None)
def around_case(name):
    """(3, 512, 4): the scene of layout ``limit``, bit for bit and under its threshold, between two small scenes scaled to
    that threshold -> (sizes, C_obs, nrm, th)"""
    k = CONFIGS[name][3]
    (n,), C_big, nrm_big, th_big = layout_case(name, "limit")
    C_s, nrm_s = SN.synthetic_split([3, 4], [seed_of(name, "around"), sorted(CONFIGS).index(name), 7], k)
    C_obs = np.concatenate([C_s[:, :3], C_big, C_s[:, 3:]], axis=1)
    nrm = np.concatenate([nrm_s[:, :3], nrm_big, nrm_s[:, 3:]], axis=1)
    C_obs, nrm, th = rescaled(name, (3, n, 4), C_obs, nrm)
    assert th == th_big and np.array_equal(C_obs[:, 3:3 + n], C_big) and np.array_equal(nrm[:, 3:3 + n], nrm_big)
    return (3, n, 4), C_obs, nrm, th


def scenes_of(sizes, C_obs, nrm):
    """-> [(scene, first row, n, v (T, n))] of the non-empty scenes, v as tests/_sgcn_np.scene_input forms it"""
    return [(s, lo, n, v) for s, lo, n, v in SN.scenes_of(sizes, C_obs, nrm) if n > 0]


def unpack(sizes, T, dist, gin, gidx, n_groups):
    """the documented packing of the scenes form's details (include/eigentraj.h), with the configuration's own T: scene s's
    (n, n) distances at n_0^2 + .. + n_{s-1}^2, pass m's (T, n_m) input block at T (m N + off[s]) of graph_inputs (3, T N)
    -> {scene: dict(dist, gin [3], indices)}"""
    N = int(sum(sizes))
    gin = np.asarray(gin).reshape(3, T * N)
    assert np.asarray(dist).size == sum(n * n for n in sizes) and np.asarray(gidx).shape == (N,)
    res, lo, sq = {}, 0, 0
    for s, n in enumerate(sizes):
        if n:
            g = int(n_groups[s])
            res[s] = {"dist": np.asarray(dist)[sq:sq + n * n].reshape(n, n), "indices": np.asarray(gidx)[lo:lo + n],
                      "gin": [gin[m, T * lo:T * lo + T * nm].reshape(T, nm) for m, nm in enumerate((n, g, n))]}
        lo, sq = lo + n, sq + n * n
    return res
