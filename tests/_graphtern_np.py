"""numpy restatement of csrc/et_graphtern.hip: the graphtern bridge's S_obs = [abs, rel] (baseline/graphtern/bridge.py:4-14),
generate_adjacency_matrix's four relations (model.py:7-15), graph_tern_light's eval-mode forward (model.py:243-264 with the
blocks of stmrgcn.py and normalizer.py) and the post-hook's squeeze, in fp64 from a state_dict of numpy arrays.

The distances are taken ON THE fp32 INPUT: |x_i - x_j| is formed in numpy fp32 as the reference (and the device) forms it,
and ``A == 0 -> A_inv = 0`` is decided on that fp32 number; the inverse, the degrees and everything after them are fp64.
The number of st_mrgcn and epcnn blocks is read off the state_dict's keys, so the same code runs the ET configuration
(1 + 6) and any other member of the family.  ``dtype=np.float32`` runs the same statements in numpy fp32 (what the fp32
arithmetic itself costs on an input); the members of the family the shapes tests run, their seeded weights, their scene
layouts and the kernel's arena figures restated are in the second half of this module."""
import numpy as np

HIDDEN = 16      # model.py:229
PAD_MODE = "edge"  # replicate padding; "constant" is NOT the reference's, kept to show that the fixtures tell them apart


def rel_of(u):
    """u (T, N) fp32 -> the displacement rows (bridge.py:9-10), fp32: rel[0] = 0, rel[t] = u[t] - u[t-1]"""
    u = np.asarray(u, np.float32)
    rel = np.zeros_like(u)
    rel[1:] = u[1:] - u[:-1]
    return rel


def s_obs_of(u):
    """u (T, N) -> S_obs (1, 2, T, N, 1) fp32 = [abs, rel], what the bridge's pre-hook hands the network"""
    u = np.asarray(u, np.float32)
    return np.stack([u, rel_of(u)])[None, :, :, :, None]


def distances(x):
    """x (T, N) fp32 -> (T, N, N) fp32 |x_i - x_j| (the reference's norm over a dimension of size 1)"""
    x = np.asarray(x, np.float32)
    return np.abs(x[:, :, None] - x[:, None, :])


def _prelu(x, a):
    return np.where(x > 0, x, float(np.asarray(a).reshape(-1)[0]) * x)


def _conv33_replicate(x, w, b, dtype=np.float64):
    """x (Cin, H, W), w (Cout, Cin, 3, 3): 'same' convolution, replicate padding (stmrgcn.py:70, 80)"""
    cin, h, wd = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1)), mode=PAD_MODE)
    out = np.zeros((w.shape[0], h, wd), dtype) + np.asarray(b, dtype)[:, None, None]
    for dh in range(3):
        for dw in range(3):
            out += np.einsum("oi,ihw->ohw", w[:, :, dh, dw], xp[:, dh:dh + h, dw:dw + wd])
    return out


def _normalised(A, dtype=np.float64):
    """A (n, n) ``dtype`` -> D^-1/2 (A + I) D^-1/2, D the row sums of A + I, an infinite D^-1/2 set to 0 (normalizer.py:7-21)"""
    At = A + np.eye(A.shape[0], dtype=dtype)
    with np.errstate(divide="ignore"):
        d = At.sum(axis=1) ** -0.5
    d[np.isinf(d)] = 0.0
    return (d[:, None] * At) * d[None, :]


def graphs(u, rel, dtype=np.float64):
    """u, rel (T, N) fp32 -> (4, T, N, N) ``dtype`` normalised graphs of [A_abs, A_rel, 1 / A_abs, 1 / A_rel]"""
    out = []
    for src in (u, rel):
        A32 = distances(src)
        out.append(A32.astype(dtype))
    for A in list(out):
        with np.errstate(divide="ignore"):
            inv = 1.0 / A
        inv[A == 0] = 0.0
        out.append(inv)
    return np.stack([np.stack([_normalised(A[t], dtype) for t in range(A.shape[0])]) for A in out])


def counts(sd):
    """-> (n_epgcn, n_epcnn) of a state_dict"""
    n_gcn = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("tp_mrgcns."))
    n_cnn = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("tpcnns."))
    return n_gcn, n_cnn


def forward(sd, u, rel=None, dtype=np.float64):
    """sd: state_dict (numpy), u (T, N) fp32 (S_obs[0, 0, :, :, 0]), rel (T, N) fp32 as given (S_obs[0, 1, :, :, 0]) or None
    (formed from u in fp32) -> (k, N, S) ``dtype``: the network's (1, k, N, S) without the batch axis, which is also what
    the post-hook's squeeze returns (C_pred_refine).  ``dtype``: np.float64, or np.float32 for the same statements in numpy
    fp32 after the fp32 distances (the inverses, the degrees, the normalisation, every contraction): the arithmetic's own
    error."""
    sd = {k: np.asarray(v, dtype) for k, v in sd.items()}
    u32 = np.asarray(u, np.float32)
    rel32 = rel_of(u32) if rel is None else np.asarray(rel, np.float32)
    n_gcn, n_cnn = counts(sd)
    L = graphs(u32, rel32, dtype)                                            # (4, T, N, N)
    x = u32.astype(dtype)[None]                                              # (C = 1, T, N): V_obs_abs
    for i in range(n_gcn):
        pre = f"tp_mrgcns.{i}"
        W, B = sd[f"{pre}.gcn.conv.weight"][:, :, 0, 0], sd[f"{pre}.gcn.conv.bias"]
        xr = (np.einsum("oc,ctv->otv", W, x) + B[:, None, None]).reshape(4, HIDDEN, x.shape[1], x.shape[2])
        y = np.einsum("rtwv,rctv->ctw", L, xr)
        y = _prelu(y, sd[f"{pre}.tcn.0.weight"])
        tw, tb = sd[f"{pre}.tcn.1.weight"][:, :, :, 0], sd[f"{pre}.tcn.1.bias"]
        T = y.shape[1]
        yp = np.zeros((HIDDEN, T + 2, y.shape[2]), dtype)
        yp[:, 1:-1] = y
        z = tb[:, None, None] + sum(np.einsum("oc,ctv->otv", tw[:, :, dt], yp[:, dt:dt + T]) for dt in range(3))
        if f"{pre}.residual.0.weight" in sd:
            res = np.einsum("oc,ctv->otv", sd[f"{pre}.residual.0.weight"][:, :, 0, 0], x) + \
                sd[f"{pre}.residual.0.bias"][:, None, None]
        else:
            res = x
        x = z + res                                                          # use_mdn: the block's own prelu is NOT applied
    t = np.transpose(x, (1, 0, 2))                                           # (T, 16, N)
    for j in range(n_cnn):
        pre = f"tpcnns.{j}"
        res = t
        if f"{pre}.restconv.0.weight" in sd:
            res = np.einsum("ot,tcv->ocv", sd[f"{pre}.restconv.0.weight"][:, :, 0, 0], res) + \
                sd[f"{pre}.restconv.0.bias"][:, None, None]
        if f"{pre}.rescconv.0.weight" in sd:
            res = np.einsum("oc,tcv->tov", sd[f"{pre}.rescconv.0.weight"][:, :, 0, 0], res) + \
                sd[f"{pre}.rescconv.0.bias"][None, :, None]
        t = _prelu(_conv33_replicate(t, sd[f"{pre}.tpcns.0.0.weight"], sd[f"{pre}.tpcns.0.0.bias"], dtype),
                   sd[f"{pre}.tpcns.0.1.weight"])                            # (k, 16, N): time rows as channels
        c = np.transpose(t, (1, 0, 2))                                       # (16, k, N)
        c = _prelu(_conv33_replicate(c, sd[f"{pre}.cpcns.0.0.weight"], sd[f"{pre}.cpcns.0.0.bias"], dtype),
                   sd[f"{pre}.cpcns.0.1.weight"])                            # (C_out, k, N)
        t = np.transpose(c, (1, 0, 2)) + res                                 # (k, C_out, N)
    return np.ascontiguousarray(np.transpose(t, (0, 2, 1)))                  # (k, N, S)


def scene_input(C_obs, nrm, lo, hi):
    """u (k+2, n) of the rows [lo, hi) of a split: [C_obs; last observed position - its mean over the scene]"""
    ori = np.asarray(nrm[:2, lo:hi], np.float32)
    ori = ori - ori.mean(axis=1, keepdims=True, dtype=np.float32)
    return np.concatenate([np.asarray(C_obs[:, lo:hi], np.float32), ori]).astype(np.float32)


# ------------------------------------------------------------------------- members of the supported family, by path
# (tests/test_gpu_graphtern_shapes.py, tests/test_graphtern_cpu.py).  k = pred_seq_len, T = seq_len = k + 2, S = n_smpl,
# st / epcnn: the numbers of st_mrgcn / epcnn blocks; spread: the sigma of the normal noise random_state adds to every
# parameter
TOL = 1e-5  # outputs: of the largest entry (tests/test_gpu_graphtern.py)
CONFIGS = {
    "k1":    dict(k=1, S=1, st=2, epcnn=2, spread=0.05, seed=0),    # qpp at its floor, one cpcn row, S = 1, first block into last
    "k2s16": dict(k=2, S=16, st=3, epcnn=2, spread=0.05, seed=0),   # identity residual in the last block, odd block count > 1
    "deep":  dict(k=6, S=9, st=4, epcnn=8, spread=0.05, seed=0),    # both layer limits, four rotations of x / y / q
    "wide":  dict(k=6, S=64, st=2, epcnn=3, spread=0.05, seed=0),   # qpp = k S, later block in chunks 5,3 (ragged), S = 64
    "kmax":  dict(k=32, S=64, st=2, epcnn=2, spread=0.05, seed=0),  # T = 34, chunks 30,4, the workspace from n = 3 on
    "tall":  dict(k=32, S=1, st=3, epcnn=2, spread=0.05, seed=0),   # chunks 8,8,8,8,2: many chunks, a ragged rest of 2
    "et":    dict(k=6, S=20, st=1, epcnn=6, spread=0.05, seed=0),   # the ET shape with seeded weights, as control
}
STATE_SEED = 33
LDS_BYTES = 60 * 1024  # kSgLdsBytes
REL = 4                # kGtRel: relations per time row


def module_cfg(name):
    """the GraphTERNLight(...) / graph_tern_light(...) arguments of CONFIGS[name]"""
    c = CONFIGS[name]
    return dict(n_epgcn=c["st"], n_epcnn=c["epcnn"], input_feat=1, seq_len=c["k"] + 2, pred_seq_len=c["k"], n_smpl=c["S"])


def chunks(T, nt):
    """the time rows of each chunk of q: [nt, nt, ..., the ragged rest]"""
    return [min(nt, T - t0) for t0 in range(0, T, nt)]


def dims(k, S, n_st):
    """gt_dims_of, gt_arena_per_ped and the chunking of gt_run_scene restated -> (T, qpp, floats per pedestrian, the largest
    scene whose arena fits LDS, the chunks of a later st_mrgcn block (C_in = 16, J = 17; None without one)).  The first block
    (J = 2) is always one chunk: qpp >= 16 T"""
    T = k + 2
    q = max(HIDDEN * T, k * S)
    if n_st > 1:
        q = max(q, REL * (HIDDEN + 1))
    per = (2 + REL) * T + 3 * q
    assert min(T, q // (REL * 2)) == T
    return T, q, per, LDS_BYTES // 4 // per, chunks(T, min(T, q // (REL * (HIDDEN + 1)))) if n_st > 1 else None


def config_dims(name):
    c = CONFIGS[name]
    return dims(c["k"], c["S"], c["st"])


def workspace_bytes(per, N, max_scene_n):
    """arena_workspace_bytes: none while the largest scene fits LDS, else every scene's rows"""
    return 0 if per * max_scene_n * 4 <= LDS_BYTES else per * N * 4


def state_shapes(name):
    """-> {state_dict name: shape} of GraphTERNLight(**module_cfg(name)), in the module's order"""
    c = CONFIGS[name]
    k, T, S, H = c["k"], c["k"] + 2, c["S"], HIDDEN
    sh = {}
    for i in range(c["st"]):
        p, Cin = f"tp_mrgcns.{i}.", 1 if i == 0 else H
        sh[p + "prelu.weight"] = (1,)
        sh[p + "gcn.conv.weight"], sh[p + "gcn.conv.bias"] = (REL * H, Cin, 1, 1), (REL * H,)
        sh[p + "tcn.0.weight"], sh[p + "tcn.1.weight"], sh[p + "tcn.1.bias"] = (1,), (H, H, 3, 1), (H,)
        if Cin != H:
            sh[p + "residual.0.weight"], sh[p + "residual.0.bias"] = (H, Cin, 1, 1), (H,)
    for j in range(c["epcnn"]):
        p, Rin, Cout = f"tpcnns.{j}.", T if j == 0 else k, S if j + 1 == c["epcnn"] else H
        sh[p + "tpcns.0.0.weight"], sh[p + "tpcns.0.0.bias"], sh[p + "tpcns.0.1.weight"] = (k, Rin, 3, 3), (k,), (1,)
        sh[p + "cpcns.0.0.weight"], sh[p + "cpcns.0.0.bias"], sh[p + "cpcns.0.1.weight"] = (Cout, H, 3, 3), (Cout,), (1,)
        if Cout != H:
            sh[p + "rescconv.0.weight"], sh[p + "rescconv.0.bias"] = (Cout, H, 1, 1), (Cout,)
        if Rin != k:
            sh[p + "restconv.0.weight"], sh[p + "restconv.0.bias"] = (k, Rin, 1, 1), (k,)
    return sh


def is_slope(key):
    """a PReLU's weight among the state dict's names (tp_mrgcns.{i}.prelu, which the network never applies, included)"""
    return key.endswith(("prelu.weight", "tcn.0.weight", "tpcns.0.1.weight", "cpcns.0.1.weight"))


def random_state(name):
    """a seeded fp32 state dict of CONFIGS[name] that leaves nothing at its default: weights and biases uniform in
    +-1/sqrt(fan_in) (torch's default range) plus N(0, spread) noise, every bias non-zero, every PReLU slope different and
    none 0.25 -- the slope the network never applies too, so a kernel that applied it would be noticed"""
    c = CONFIGS[name]
    rng = np.random.default_rng([STATE_SEED, c["seed"], sorted(CONFIGS).index(name)])
    shapes = state_shapes(name)
    n_slopes = sum(1 for key in shapes if is_slope(key))
    slopes = 0.05 + 0.17 * (rng.permutation(n_slopes) + rng.uniform(0.2, 0.8, n_slopes)) / n_slopes  # distinct, in (0.05, 0.22)
    sd, q = {}, 0
    for key, shape in shapes.items():
        if is_slope(key):
            sd[key] = np.array([slopes[q]], np.float32)
            q += 1
            continue
        fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else int(np.prod(shapes[key[:-4] + "weight"][1:]))
        w = rng.uniform(-1, 1, shape) / np.sqrt(fan_in) + rng.normal(0, c["spread"], shape)
        if key.endswith("bias"):
            w = np.where(np.abs(w) < 1e-3, 1e-3, w)
        sd[key] = w.astype(np.float32)
    return sd


def synthetic_split(sizes, seed, k=6):
    """C_obs (k, N), nrm (4, N) of a made-up split of ``sizes`` (or of N) pedestrians: coefficients ~ N(0, 1) with equal
    (rounded) values in every row of the first quarter, every fifth column repeated in the next one (the same pedestrian
    twice) and a few all-zero columns (static pedestrians), positions ~ N(0, 5) around the origin: exact zeros occur off the
    diagonal in both relations"""
    n = int(np.sum(sizes))
    rng = np.random.default_rng(seed)
    C_obs = rng.normal(0, 1, (k, n)).astype(np.float32)
    C_obs[:, : max(n // 4, 1)] = np.round(C_obs[:, : max(n // 4, 1)], 1)
    nrm = rng.normal(0, 5, (4, n)).astype(np.float32)
    for i in range(0, n - 1, 5):  # coincident columns: the same pedestrian twice
        C_obs[:, i + 1], nrm[:, i + 1] = C_obs[:, i], nrm[:, i]
    C_obs[:, 3::11] = 0.0
    return C_obs, nrm


# scene layouts of the shapes tests; "edge" ends with the configuration's own LDS / workspace switch
EDGE_SIZES = (1, 2, 3, 0, 63, 64, 65)
BIG = (257, 512)
MANY = tuple(i % 6 for i in range(300))  # 300 scenes of 0 .. 5 pedestrians
NAN_SIZES = (4, 70, 40, 3, 9)
FIXTURE_SIZES = (3, 13)                  # the scenes of tests/golden/g33_graphtern_family.npz, from the edge generator
USED = {  # the layouts each configuration runs on the GPU; big stays off kmax and tall (O(T n^2) loops of ONE workgroup)
    "k1": ("edge", "g3", "g65", "big", "many"),
    "k2s16": ("edge", "g3", "g65"),
    "deep": ("edge", "g3", "g65", "nan"),
    "wide": ("edge", "g3", "g65", "big", "nan"),
    "kmax": ("edge", "g3", "g65"),
    "tall": ("edge", "g3", "g65"),
    "et": ("edge", "g3", "g65", "many"),
}
SEEDS = {(name, layout): 1 for name, used in USED.items() for layout in used}
# k1 has ONE output number per pedestrian, and a scene of one or two can leave it near zero by cancellation, where the fp32
# arithmetic itself misses TOL / 4 of it (float32 mode against fp64 over the seeds 1 .. 9: 9.2e-6, 4.7e-6, 3.6e-6, 1.3e-6,
# 4.7e-6, 3.6e-6, 1.5e-5, 2.5e-6, 5.0e-6; the smallest scene maximum 1.7e-2, 2.0e-2, 5.5e-2, 8.7e-2, ...): the seed with
# the smallest ratio.  No scene is dropped
SEEDS["k1", "many"] = 4


def layout_sizes(name, layout):
    lim = config_dims(name)[3]
    return {"edge": EDGE_SIZES + (lim, lim + 1), "big": BIG, "many": MANY, "nan": NAN_SIZES, "g3": (3,), "g65": (65,)}[layout]


def layout_inputs(name, layout):
    """-> (sizes, C_obs (k, N), nrm (4, N)) of configuration ``name`` on ``layout``"""
    sizes = layout_sizes(name, layout)
    C_obs, nrm = synthetic_split(sizes, SEEDS[name, layout], CONFIGS[name]["k"])
    return sizes, C_obs, nrm


def fixture_inputs(name):
    """-> (FIXTURE_SIZES, C_obs, nrm): the two scenes of g33, drawn with the edge layout's seed"""
    C_obs, nrm = synthetic_split(FIXTURE_SIZES, SEEDS[name, "edge"], CONFIGS[name]["k"])
    return FIXTURE_SIZES, C_obs, nrm


def scenes_of(sizes, C_obs, nrm):
    """yields (index, lo, n, u (T, n)) for the non-empty scenes of a layout"""
    lo = 0
    for s, n in enumerate(sizes):
        if n:
            yield s, lo, n, scene_input(C_obs, nrm, lo, lo + n)
        lo += n


def odd_rel(u):
    """a ``rel`` (T, n) fp32 that no bridge builds, from u: a non-zero first row, not the difference of u (a quarter of the
    row above is added instead of the whole being subtracted, the rows cycled by one), and, from n = 4 on, exact ties
    between pedestrians that u does not tie: column 3 repeats column 2, the last column repeats column 0 in the odd rows"""
    u = np.asarray(u, np.float32)
    rel = (np.float32(0.5) * np.roll(u, 1, axis=0) + np.float32(0.25) * u).astype(np.float32)
    if u.shape[1] >= 4:
        rel[:, 3] = rel[:, 2]
        rel[1::2, -1] = rel[1::2, 0]
    return np.ascontiguousarray(rel)
