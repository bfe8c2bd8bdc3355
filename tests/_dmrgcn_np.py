"""numpy restatement of csrc/et_dmrgcn.hip: the dmrgcn bridge's adjacency (baseline/dmrgcn/bridge.py:4-19), the disentangled
bins (dmrgcn.py:12-35), social_dmrgcn's eval-mode forward (dmrgcn.py, predictor.py) and the post-hook's permute, in fp64 from
a state_dict of numpy arrays.

The bins are taken ON THE fp32 DISTANCES: v_rel and |.| are formed in numpy fp32 as the bridge (and the device) forms them
and then compared with the split values; everything after the decision is fp64.  A time row's (n, n) distances are
handled in blocks of rows, and a bin's Laplacian is never formed (its action on the rows is a masked sum), so synthetic
scenes of thousands of pedestrians -- which no fixture can hold -- have something to compare with."""
import numpy as np

SPLIT = ((0.0, 0.25, 0.5, 0.75, 1.0), (0.0, 0.5, 1.0, 2.0, 4.0))  # predictor.py:68-69: [A_disp, A_dist]
LAST = 1e10                                                        # dmrgcn.py:29
ROWS = 512                                                         # rows of a time row's (n, n) block handled at once


def v_rel(v):
    """v (K, N) fp32 -> the displacement rows (bridge.py:8-9), fp32"""
    v = np.asarray(v, np.float32)
    rel = np.zeros_like(v)
    rel[1:] = v[1:] - v[:-1]
    return rel


def adjacency(v):
    """v (K, N) -> a (2, K, N, N) fp32 = [A_disp, A_dist], what the bridge's pre-hook hands the network (small scenes)"""
    v = np.asarray(v, np.float32)
    rel = v_rel(v)
    return np.stack([np.abs(rel[:, :, None] - rel[:, None, :]), np.abs(v[:, :, None] - v[:, None, :])])


def bins(dist, split, closed=False):
    """dist (..., fp32), split (5,) -> (5, ...) bool: bin b is lo < dist < hi (``closed``: lo <= dist <= hi -- NOT the
    reference's semantics, kept to show that the fixtures tell the two apart); the comparison is made in fp32."""
    dist = np.asarray(dist, np.float32)
    edges = np.asarray(list(split) + [LAST], np.float32)
    if closed:
        return np.stack([(dist >= edges[b]) & (dist <= edges[b + 1]) & (dist > 0) for b in range(len(split))])
    return np.stack([(dist > edges[b]) & (dist < edges[b + 1]) & (dist > 0) for b in range(len(split))])


def _prelu(x, a):
    return np.where(x > 0, x, float(np.asarray(a).reshape(-1)[0]) * x)


def _conv33(x, w, b, dtype=np.float64):
    """x (Cin, H, W), w (Cout, Cin, 3, 3) zero-padded 'same' convolution"""
    cin, h, wd = x.shape
    xp = np.zeros((cin, h + 2, wd + 2), dtype)
    xp[:, 1:-1, 1:-1] = x
    out = np.zeros((w.shape[0], h, wd), dtype) + np.asarray(b, dtype)[:, None, None]
    for dh in range(3):
        for dw in range(3):
            out += np.einsum("oi,ihw->ohw", w[:, :, dh, dw], xp[:, dh:dh + h, dw:dw + wd])
    return out


def _contract(X, dist_rows, split, closed, dtype=np.float64):
    """One relation, one time row.  X (J, n) rows to contract, dist_rows(lo, hi) -> (hi - lo, n) fp32 distances of
    rows [lo, hi) -> P (5, J, n): P[b, j, w] = sum_v L_b[w, v] X[j, v], L_b = I - D^-1/2 (A_b + I) D^-1/2."""
    J, n = X.shape
    nb = len(split)
    cnt = np.zeros((nb, n), dtype)
    for lo in range(0, n, ROWS):
        cnt[:, lo:lo + ROWS] = bins(dist_rows(lo, min(n, lo + ROWS)), split, closed).sum(axis=2)
    dinv = (1.0 + cnt) ** -0.5                      # A_b + I: every degree is >= 1
    P = np.empty((nb, J, n), dtype)
    for lo in range(0, n, ROWS):
        hi = min(n, lo + ROWS)
        M = bins(dist_rows(lo, hi), split, closed)  # (5, rows, n); the diagonal (distance 0) is in no bin
        for b in range(nb):
            # (D (A + I) D X)[w] = d_w (sum_v A[w,v] d_v X[v] + d_w X[w])
            ax = (X * dinv[b]) @ M[b].T.astype(dtype)
            P[b, :, lo:hi] = X[:, lo:hi] - dinv[b, lo:hi] * (ax + dinv[b, lo:hi] * X[:, lo:hi])
    return P


def gcn(sd, pre, x, rel32, v32, a=None, split=SPLIT, closed=False, dtype=np.float64):
    """the two MultiRelationalGCNs of block ``pre`` summed: x (Cin, K, N) ``dtype``, the bins from the fp32 rows rel32 / v32
    (K, N) or from a given a (2, K, N, N), read as it is -> y (S, K, N) before the tcn's PReLU.  sd: arrays of ``dtype``"""
    Cin, K, N = x.shape
    S = sd[f"{pre}.tcn.1.weight"].shape[0]
    ones = np.ones((1, N), dtype)
    y = np.zeros((S, K, N), dtype)
    for r, src in enumerate((rel32, v32)):
        W = sd[f"{pre}.gcns.{r}.conv.weight"][:, :, 0, 0].reshape(len(split[r]), S, Cin)   # channel b S + c
        B = sd[f"{pre}.gcns.{r}.conv.bias"].reshape(len(split[r]), S)
        for t in range(K):
            if a is not None:
                rows = lambda lo, hi, r=r, t=t: np.asarray(a[r][t][lo:hi], np.float32)
            else:
                rows = lambda lo, hi, s=src[t]: np.abs(s[lo:hi, None] - s[None, :])
            P = _contract(np.concatenate([x[:, t], ones]), rows, split[r], closed, dtype)       # (5, Cin + 1, N)
            y[:, t] += np.einsum("bsc,bcw->sw", W, P[:, :Cin]) + np.einsum("bs,bw->sw", B, P[:, Cin])
    return y


def forward(sd, v, a=None, n_stgcn=1, n_tpcnn=4, split=SPLIT, closed=False, dtype=np.float64):
    """sd: state_dict (numpy), v (K, N) fp32 -> raw output (S, k, N) (the network's (1, S, k, N) without the batch axis).
    a (2, K, N, N) given (read as it is) or None (formed from v in fp32, block by block).  ``dtype``: np.float64, or
    np.float32 for the same statements in fp32 after the bin decision (the arithmetic's own error)."""
    sd = {k: np.asarray(val, dtype) for k, val in sd.items()}
    v32 = np.asarray(v, np.float32)
    rel32 = v_rel(v32)
    x = v32.astype(dtype)[None]  # (C = 1, K, N)
    K, N = x.shape[1], x.shape[2]
    for i in range(n_stgcn):
        pre = f"st_dmrgcns.{i}"
        S = sd[f"{pre}.tcn.1.weight"].shape[0]
        y = gcn(sd, pre, x, rel32, v32, a, split, closed, dtype)
        y = _prelu(y, sd[f"{pre}.tcn.0.weight"])
        tw, tb = sd[f"{pre}.tcn.1.weight"][:, :, :, 0], sd[f"{pre}.tcn.1.bias"]
        yp = np.zeros((S, K + 2, N), dtype)
        yp[:, 1:-1] = y
        z = tb[:, None, None] + sum(np.einsum("oc,ctv->otv", tw[:, :, dt], yp[:, dt:dt + K]) for dt in range(3))
        if f"{pre}.residual.0.weight" in sd:
            res = np.einsum("oc,ctv->otv", sd[f"{pre}.residual.0.weight"][:, :, 0, 0], x) + \
                sd[f"{pre}.residual.0.bias"][:, None, None]
        else:
            res = x
        x = _prelu(z + res, sd[f"{pre}.prelu.weight"])
    t = np.transpose(x, (1, 0, 2))                                         # a real permute: (K, S, N)
    for j in range(n_tpcnn):
        pre = f"tpcnns.{j}"
        if f"{pre}.residual.0.weight" in sd:
            res = np.einsum("oc,chw->ohw", sd[f"{pre}.residual.0.weight"][:, :, 0, 0], t) + \
                sd[f"{pre}.residual.0.bias"][:, None, None]
        else:
            res = t
        t = _prelu(_conv33(t, sd[f"{pre}.tpcn.0.0.weight"], sd[f"{pre}.tpcn.0.0.bias"], dtype), sd[f"{pre}.tpcn.0.1.weight"]) + res
        t = _prelu(_conv33(t, sd[f"{pre}.tpcn.1.0.weight"], sd[f"{pre}.tpcn.1.0.bias"], dtype), sd[f"{pre}.tpcn.1.1.weight"]) + t
        g = np.einsum("ost,tsw->ow", sd[f"{pre}.gtacn.0.0.weight"][:, :, :, 0], t) + sd[f"{pre}.gtacn.0.0.bias"][:, None]
        t = _prelu(g, sd[f"{pre}.gtacn.0.1.weight"])[None] + t              # the one row broadcast over the k rows
    return np.ascontiguousarray(np.transpose(t, (1, 0, 2)))                # (S, k, N)


def c_pred_refine(raw):
    """raw (S, k, N) -> (k, N, S) (bridge.py:40)"""
    return np.ascontiguousarray(np.transpose(raw, (1, 2, 0)))


def scene_input(C_obs, nrm, lo, hi):
    """v (k+2, n) of the rows [lo, hi) of a split: [C_obs; last observed position - its mean over the scene]"""
    ori = np.asarray(nrm[:2, lo:hi], np.float32)
    ori = ori - ori.mean(axis=1, keepdims=True, dtype=np.float32)
    return np.concatenate([np.asarray(C_obs[:, lo:hi], np.float32), ori]).astype(np.float32)


# ------------------------------------------------------------------------- members of the supported family, by path
# (tests/test_gpu_dmrgcn_shapes.py, tests/test_dmrgcn_cpu.py).  k = pred_seq_len, K = seq_len = k + 2, S = output_feat;
# spread: the sigma of the normal noise random_state adds to every parameter
TOL = 1e-5  # outputs: of the largest entry (tests/test_gpu_dmrgcn.py)
CONFIGS = {
    "k1":     dict(k=1, S=1, st=1, tp=1, spread=0.05, seed=0),    # qpp floor, first-block nt = 1, S = 1 in conv33, one tpcnn block
    "narrow": dict(k=7, S=5, st=1, tp=2, spread=0.05, seed=0),    # first block chunked 2,2,2,2,1; the switch at 63 / 64
    "deep":   dict(k=6, S=9, st=4, tp=8, spread=0.05, seed=0),    # both limits, even J = 10, chunks 5,3 then nt = 1, four rotations
    "wide3":  dict(k=2, S=64, st=3, tp=2, spread=0.05, seed=0),   # S = 64, J = 65, an odd block count above 1, K = 4
    "kmax":   dict(k=32, S=64, st=2, tp=1, spread=0.05, seed=0),  # K = 34, later block nt = 3: chunks 3 x 11 then 1
    "et":     dict(k=6, S=20, st=1, tp=4, spread=0.05, seed=0),   # the ET shape as control
}
STATE_SEED = 23
LDS_BYTES = 60 * 1024  # kSgLdsBytes
RB = 2 * len(SPLIT[0])  # kDmRB: (relation, bin) graphs per time row


def module_cfg(name):
    """the SocialDMRGCN(...) arguments of CONFIGS[name]"""
    c = CONFIGS[name]
    return dict(n_stgcn=c["st"], n_tpcnn=c["tp"], input_feat=1, output_feat=c["S"], seq_len=c["k"] + 2, pred_seq_len=c["k"],
                kernel_size=3)


def dims(k, S, n_st, n_tp=1):
    """dm_dims_of, dm_arena_per_ped and the chunking of dm_run_scene restated -> (K, qpp, floats per pedestrian, the
    largest scene whose arena fits LDS, time rows per chunk of the first block, of a later block (None without one))"""
    K = k + 2
    q = max(S * K, 2 * RB)
    if n_st > 1:
        q = max(q, RB * (S + 1))
    per = (2 + RB) * K + 3 * q
    return K, q, per, LDS_BYTES // 4 // per, min(K, q // (RB * 2)), min(K, q // (RB * (S + 1))) if n_st > 1 else None


def config_dims(name):
    c = CONFIGS[name]
    return dims(c["k"], c["S"], c["st"], c["tp"])


def workspace_bytes(per, N, max_scene_n):
    """arena_workspace_bytes: none while the largest scene fits LDS, else every scene's rows"""
    return 0 if per * max_scene_n * 4 <= LDS_BYTES else per * N * 4


def chunks(K, nt):
    """the time rows of each chunk of q: [nt, nt, ..., the ragged rest]"""
    return [min(nt, K - t0) for t0 in range(0, K, nt)]


def state_shapes(name):
    """-> {state_dict name: shape} of SocialDMRGCN(**module_cfg(name)), in the module's order"""
    c = CONFIGS[name]
    k, K, S = c["k"], c["k"] + 2, c["S"]
    nb = len(SPLIT[0])
    sh = {}
    for i in range(c["st"]):
        p, Cin = f"st_dmrgcns.{i}.", 1 if i == 0 else S
        for r in range(2):
            sh[f"{p}gcns.{r}.conv.weight"], sh[f"{p}gcns.{r}.conv.bias"] = (nb * S, Cin, 1, 1), (nb * S,)
        sh[p + "tcn.0.weight"], sh[p + "tcn.1.weight"], sh[p + "tcn.1.bias"] = (1,), (S, S, 3, 1), (S,)
        if Cin != S:
            sh[p + "residual.0.weight"], sh[p + "residual.0.bias"] = (S, Cin, 1, 1), (S,)
        sh[p + "prelu.weight"] = (1,)
    for j in range(c["tp"]):
        p, Cin = f"tpcnns.{j}.", K if j == 0 else k
        for m in range(2):
            sh[f"{p}tpcn.{m}.0.weight"], sh[f"{p}tpcn.{m}.0.bias"] = (k, Cin if m == 0 else k, 3, 3), (k,)
            sh[f"{p}tpcn.{m}.1.weight"] = (1,)
        sh[p + "gtacn.0.0.weight"], sh[p + "gtacn.0.0.bias"], sh[p + "gtacn.0.1.weight"] = (S, S, k, 1), (S,), (1,)
        if Cin != k:
            sh[p + "residual.0.weight"], sh[p + "residual.0.bias"] = (k, Cin, 1, 1), (k,)
    return sh


def is_slope(key):
    """a PReLU's weight among the state dict's names"""
    return key.endswith(("tcn.0.weight", "prelu.weight", "tpcn.0.1.weight", "tpcn.1.1.weight", "gtacn.0.1.weight"))


def random_state(name):
    """a seeded fp32 state dict of CONFIGS[name] that leaves nothing at its default: weights and biases uniform in
    +-1/sqrt(fan_in) (torch's default range) plus N(0, spread) noise, every bias non-zero, every PReLU slope different and
    none 0.25; the two relations' gcn weights are separate draws"""
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
    """C_obs (k, N), nrm (4, N) of a made-up split, as tests/test_gpu_dmrgcn.py's _synthetic: coefficients ~ N(0, 1), the
    first eighth rounded to 0.1 (equal values in every row), every fifth column repeated in the next one (the same
    pedestrian twice: distances of exactly 0), last observed positions ~ N(0, 5)"""
    rng = np.random.default_rng(seed)
    n = int(sum(sizes))
    C_obs = rng.normal(0, 1, (k, n)).astype(np.float32)
    C_obs[:, : n // 8] = np.round(C_obs[:, : n // 8], 1)
    nrm = rng.normal(0, 5, (4, n)).astype(np.float32)
    for i in range(0, n - 1, 5):
        C_obs[:, i + 1], nrm[:, i + 1] = C_obs[:, i], nrm[:, i]
    return C_obs, nrm


# scene layouts of the shapes tests; "edge" ends with the configuration's own LDS / workspace switch
EDGE_SIZES = (1, 2, 3, 0, 63, 64, 65)
BIG = (257, 512)
MANY = tuple(i % 6 for i in range(300))  # 300 scenes of 0 .. 5 pedestrians
NAN_SIZES = (4, 70, 40, 3, 9)
USED = {  # the layouts each configuration runs on the GPU
    "k1": ("edge", "g3", "g65", "big", "many"),
    "narrow": ("edge", "g3", "g65", "nan"),
    "deep": ("edge", "g3", "g65", "nan"),
    "wide3": ("edge", "g3", "g65", "big"),
    "kmax": ("edge", "g3", "g65"),
    "et": ("edge", "g3", "g65", "many"),
}
SEEDS = {(name, layout): 1 for name, used in USED.items() for layout in used}
# k1 has ONE output number per pedestrian, and a scene of one or two can leave it near zero by cancellation, where the fp32
# arithmetic itself misses TOL / 4 of it (float32 mode against fp64 over the seeds 1 .. 7: 4.6e-6, 1.0e-6, 6.7e-7, 1.0e-5,
# 8.2e-7, 1.5e-6, 1.1e-6; the smallest scene maximum 7.0e-3, 5.3e-3, 2.8e-2, 3.1e-3, ...): the seed with the smallest ratio
SEEDS["k1", "many"] = 3


def layout_sizes(name, layout):
    lim = config_dims(name)[3]
    return {"edge": EDGE_SIZES + (lim, lim + 1), "big": BIG, "many": MANY, "nan": NAN_SIZES, "g3": (3,), "g65": (65,)}[layout]


def layout_inputs(name, layout):
    """-> (sizes, C_obs (k, N), nrm (4, N)) of configuration ``name`` on ``layout``"""
    sizes = layout_sizes(name, layout)
    C_obs, nrm = synthetic_split(sizes, SEEDS[name, layout], CONFIGS[name]["k"])
    return sizes, C_obs, nrm


def scenes_of(sizes, C_obs, nrm):
    """yields (index, lo, n, v (K, n)) for the non-empty scenes of a layout"""
    lo = 0
    for s, n in enumerate(sizes):
        if n:
            yield s, lo, n, scene_input(C_obs, nrm, lo, lo + n)
        lo += n


def odd_adjacency(v, split=SPLIT):
    """an ``a`` (2, K, n, n) that no bridge builds, from the bridge's own: asymmetric (what lies above the diagonal is
    multiplied by 1.5, so a pair's two directions fall into different bins), every third pedestrian with a diagonal entry
    inside a bin (0.375 / 0.75: bin 1 of either relation), entries exactly on split values (row w, column w + 2 of every
    fourth row: split[r][1 + w % 4]), and row 1 with no neighbour in any bin (all zeros, its diagonal included)"""
    a = adjacency(v).copy()
    n = a.shape[-1]
    iu = np.triu_indices(n, 1)
    a[:, :, iu[0], iu[1]] *= np.float32(1.5)
    for r in range(2):
        for w in range(0, n, 3):
            a[r, :, w, w] = np.float32((0.375, 0.75)[r])
        for w in range(0, n - 2, 4):
            a[r, :, w, w + 2] = np.float32(split[r][1 + (w // 4) % 4])
    if n > 1:
        a[:, :, 1, :] = 0
    return np.ascontiguousarray(a)
