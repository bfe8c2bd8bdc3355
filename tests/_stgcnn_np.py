"""numpy restatement of csrc/et_stgcnn.hip: the stgcnn bridge's adjacency (baseline/stgcnn/bridge.py:4-21), social_stgcnn's
eval-mode forward (model.py) and the post-hook's permute, in fp64 from a state_dict of numpy arrays.

The Laplacian of a time row is formed from v one row at a time (never (K, N, N) at once), so synthetic scenes of thousands
of pedestrians -- which no fixture can hold -- have something to compare with."""
import numpy as np


def laplacian_row(u, dtype=np.float64):
    """u (N,) one time row of v -> L (N, N) = I - D a_hat D, a_hat = 1/|u_i - u_j| (0 where equal) + I"""
    u = np.asarray(u, dtype)
    one, eye = dtype(1), np.eye(len(u), dtype=dtype)  # (dtype: np.float64 or np.float32, the scalar types)
    dist = np.abs(u[:, None] - u[None, :])
    with np.errstate(divide="ignore", invalid="ignore"):
        a_hat = np.where(dist == 0, dtype(0), one / dist)
    a_hat += eye
    deg = a_hat.sum(axis=1, dtype=dtype)
    # float32: two correctly rounded operations (what the kernel does), the same on every libm; float64: the reference's pow
    d = deg ** -0.5 if dtype is np.float64 else one / np.sqrt(deg)
    return eye - d[:, None] * a_hat * d[None, :]


def adjacency(v):
    """v (K, N) -> (K, N, N), what the bridge's pre-hook hands the network (for small scenes)"""
    return np.stack([laplacian_row(r) for r in np.asarray(v, np.float64)])


def _bn(x, sd, pre, axis_shape, eps=1e-5):
    w, b, m, var = (np.asarray(sd[f"{pre}.{n}"], x.dtype).reshape(axis_shape)
                    for n in ("weight", "bias", "running_mean", "running_var"))
    return (x - m) / np.sqrt(var + x.dtype.type(eps)) * w + b


def _prelu(x, a):
    return np.where(x > 0, x, x.dtype.type(np.asarray(a).reshape(-1)[0]) * x)


def _conv33(x, w, b):
    """x (Cin, H, W), w (Cout, Cin, 3, 3) zero-padded 'same' convolution"""
    cin, h, wd = x.shape
    xp = np.zeros((cin, h + 2, wd + 2), x.dtype)
    xp[:, 1:-1, 1:-1] = x
    out = np.zeros((w.shape[0], h, wd), x.dtype) + np.asarray(b, x.dtype)[:, None, None]
    for dh in range(3):
        for dw in range(3):
            out += np.einsum("oi,ihw->ohw", w[:, :, dh, dw], xp[:, dh:dh + h, dw:dw + wd])
    return out


def forward(sd, v, a=None, n_stgcnn=1, n_txpcnn=5, eps=1e-5, dtype=np.float64):
    """sd: state_dict (numpy), v (K, N) -> raw output (S, k, N) (the network's (1, S, k, N) without the batch axis).
    a (K, N, N) given or None (formed from v row by row).  eps: the BatchNorms' eps.  dtype: np.float64, the restatement
    the kernels are compared with; np.float32 makes every array and accumulator float32 -- the reference arithmetic's own
    rounding error, the evidence for the tests' tolerance and nothing else."""
    sd = {k: np.asarray(val, dtype) for k, val in sd.items()}
    x = np.asarray(v, dtype)[None]  # (C=1, K, N)
    K, N = x.shape[1], x.shape[2]
    for i in range(n_stgcnn):
        pre = f"st_gcns.{i}"
        W = sd[f"{pre}.gcn.conv.weight"][:, :, 0, 0]                   # (S K, Cin)
        S = W.shape[0] // K
        x1 = np.einsum("oc,ctv->otv", W, x) + sd[f"{pre}.gcn.conv.bias"][:, None, None]
        x1 = x1.reshape(K, S, K, N)                                       # (kk, c, t, v)
        y = np.zeros((S, K, N), dtype)
        for kk in range(K):
            L = np.asarray(a[kk], dtype) if a is not None else laplacian_row(v[kk], dtype)
            y += np.einsum("ctv,vw->ctw", x1[kk], L)
        y = _prelu(_bn(y, sd, f"{pre}.tcn.0", (-1, 1, 1), eps), sd[f"{pre}.tcn.1.weight"])
        tw, tb = sd[f"{pre}.tcn.2.weight"][:, :, :, 0], sd[f"{pre}.tcn.2.bias"]
        yp = np.zeros((S, K + 2, N), dtype)
        yp[:, 1:-1] = y
        z = tb[:, None, None] + sum(np.einsum("oc,ctv->otv", tw[:, :, dt], yp[:, dt:dt + K]) for dt in range(3))
        z = _bn(z, sd, f"{pre}.tcn.3", (-1, 1, 1), eps)
        if f"{pre}.residual.0.weight" in sd:
            r = np.einsum("oc,ctv->otv", sd[f"{pre}.residual.0.weight"][:, :, 0, 0], x) + \
                sd[f"{pre}.residual.0.bias"][:, None, None]
            r = _bn(r, sd, f"{pre}.residual.1", (-1, 1, 1), eps)
        else:
            r = x
        x = _prelu(z + r, sd[f"{pre}.prelu.weight"])
    S = x.shape[0]
    t = x.reshape(K, S, N)                                                 # the reference's view, not a permute
    t = _prelu(_conv33(t, sd["tpcnns.0.weight"], sd["tpcnns.0.bias"]), sd["prelus.0.weight"])
    for j in range(1, n_txpcnn - 1):
        t = _prelu(_conv33(t, sd[f"tpcnns.{j}.weight"], sd[f"tpcnns.{j}.bias"]), sd[f"prelus.{j}.weight"]) + t
    t = _conv33(t, sd["tpcnn_ouput.weight"], sd["tpcnn_ouput.bias"])      # (k, S, N)
    assert t.dtype == dtype
    k = t.shape[0]
    return t.reshape(S, k, N)


def c_pred_refine(raw):
    """raw (S, k, N) -> (k, N, S) (bridge.py:42)"""
    return np.ascontiguousarray(np.transpose(raw, (1, 2, 0)))


def scene_input(C_obs, nrm, lo, hi):
    """v (k+2, n) of the rows [lo, hi) of a split: [C_obs; last observed position - its mean over the scene]"""
    ori = np.asarray(nrm[:2, lo:hi], np.float32)
    ori = ori - ori.mean(axis=1, keepdims=True, dtype=np.float32)
    return np.concatenate([np.asarray(C_obs[:, lo:hi], np.float32), ori]).astype(np.float32)


# (n_stgcnn, n_txpcnn, S, k) of the configurations the tests run; floats per pedestrian and LDS limit in the comment
CONFIGS = {"et": (1, 5, 20, 6),        # 456, 33
           "tp1": (1, 1, 20, 6),       # 345, 44
           "tiny": (1, 2, 5, 1),       # 40, 384
           "gen": (2, 3, 12, 6),       # 305, 50
           "deep_tp": (3, 8, 20, 4),   # 373, 41
           "deep_st": (8, 5, 7, 3),    # 116, 132
           "wide": (1, 5, 64, 6),      # 1424, 10
           "max": (2, 4, 64, 32)}      # 6597, 2
ARENA = {"et": (456, 33), "tp1": (345, 44), "tiny": (40, 384), "gen": (305, 50), "deep_tp": (373, 41),
         "deep_st": (116, 132), "wide": (1424, 10), "max": (6597, 2)}


def split_sizes(name):
    """scene sizes around the LDS limit L of a configuration (0: an empty scene); `max` stops at 17 pedestrians"""
    L = lds_max_n(*CONFIGS[name])
    return [1, 2, 3, 0, 17, 2] if name == "max" else [1, 2, 3, L - 1, L, L + 1, 0, 2 * L + 5, 2]


def module_kw(n_stgcnn, n_txpcnn, S, k):
    """constructor arguments of SocialSTGCNN for a configuration"""
    return dict(n_stgcnn=n_stgcnn, n_txpcnn=n_txpcnn, input_feat=1, output_feat=S, seq_len=k + 2, pred_seq_len=k,
                kernel_size=3)


def arena_per_ped(n_stgcnn, n_txpcnn, S, k):
    """floats per pedestrian of a scene's arena, restated from the header comment of csrc/et_stgcnn.hip (not imported from
    the library; the GPU tests cross-check it against et_stgcnn_workspace_bytes): u and d (K each), x and y (S K each) and
    q = K + 1, raised to S K + 1 by a second st_gcn layer and to k S by a tpcnn residual loop (n_txpcnn >= 3)"""
    K = k + 2
    q = K + 1
    if n_stgcnn > 1:
        q = max(q, S * K + 1)
    if n_txpcnn >= 3:
        q = max(q, k * S)
    return 2 * K + 2 * S * K + q


def lds_max_n(n_stgcnn, n_txpcnn, S, k):
    """the largest scene whose arena fits the 60 KB of LDS a workgroup takes"""
    return (60 * 1024 // 4) // arena_per_ped(n_stgcnn, n_txpcnn, S, k)


def exact_split(sizes, k, seed):
    """-> C_obs (k, N) random float32, nrm (4, N) float32 whose rows 0-1 make every scene's mean, and the positions minus
    that mean, EXACT in float32 in any summation order: multiples of 2^-6 with |value| <= 64, drawn inside a scene as pairs
    (x, 2c - x) plus one c when n is odd, c a multiple of 2^-6 that differs per scene and per row.  Every partial sum of up
    to 4096 such values is a multiple of 2^-6 below 2^18 (24 bits), the sum is n c and the mean c.  So the scene form reads
    exactly what scene_input() hands the restatement.  Ties: every fifth column of a scene equals its right neighbour in
    every row (in rows 0-1 of nrm the x are tied before they are paired, so the mirrored values tie as well and the mean
    stays c), and in the largest scene all pedestrians coincide in one C_obs row."""
    rng = np.random.default_rng(seed)
    N = int(sum(sizes))
    assert max(sizes, default=0) <= 4096
    C_obs = rng.normal(0, 1, (k, N)).astype(np.float32)
    nrm = rng.normal(0, 5, (4, N)).astype(np.float32)
    cs = rng.choice(np.arange(-1000, 1001), size=2 * len(sizes), replace=False)  # in units of 2^-6: |c| <= 15.7
    lo = 0
    for s, n in enumerate(sizes):
        half = n // 2
        tied = np.arange(0, n - 1, 5)
        C_obs[:, lo + tied + 1] = C_obs[:, lo + tied]
        for r in range(2):
            c = int(cs[2 * s + r])
            x = rng.integers(-2048, 2049, size=half)  # |x| <= 32, |2c - x| <= 63.3
            t = np.arange(0, half - 1, 5)
            x[t + 1] = x[t]
            row = np.concatenate([x, 2 * c - x, [c] * (n - 2 * half)])
            assert np.abs(row).max(initial=0) <= 4096
            nrm[r, lo:lo + n] = (row / 64.0).astype(np.float32)
        lo += n
    if N:
        big = int(np.argmax(sizes))
        lo = int(sum(sizes[:big]))
        C_obs[1 % k, lo:lo + sizes[big]] = C_obs[1 % k, lo]
    return C_obs, nrm


def random_state(module, seed):
    """Seeded non-default values for EVERY tensor of a SocialSTGCNN's state_dict, written into the module (a function of
    the seed and the shapes alone): convolution weights at their initial scale plus a normal perturbation, biases normal,
    BatchNorm weight in [0.6, 1.4], bias and running_mean normal (non-zero), running_var in [0.5, 2], every PReLU slope
    different and not 0.25.  -> the state_dict as float32 numpy arrays."""
    import torch
    rng = np.random.default_rng(seed)
    sd = module.state_dict()
    slopes = iter(0.05 + 0.4 * (rng.permutation(64) + rng.uniform(0.1, 0.9, 64)) / 64)
    bn = {name for name, m in module.named_modules() if isinstance(m, torch.nn.BatchNorm2d)}
    pr = {name for name, m in module.named_modules() if isinstance(m, torch.nn.PReLU)}
    new = {}
    for key, val in sd.items():
        owner, leaf = key.rsplit(".", 1)
        shape = tuple(val.shape)
        if leaf == "num_batches_tracked":
            new[key] = val.clone()
            continue
        if owner in pr:
            arr = np.full(shape, next(slopes))
            assert abs(arr.flat[0] - 0.25) > 5e-4
        elif owner in bn:
            arr = {"weight": lambda: rng.uniform(0.6, 1.4, shape), "bias": lambda: rng.normal(0, 0.2, shape),
                   "running_mean": lambda: rng.normal(0, 0.3, shape) + 0.05,
                   "running_var": lambda: rng.uniform(0.5, 2.0, shape)}[leaf]()
        else:
            # not the module's own (unseeded) initial values: the same seed gives the same state in every module
            fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else 1
            arr = (rng.uniform(-1, 1, shape) / np.sqrt(fan_in) if len(shape) > 1 else rng.normal(0, 0.2, shape)) + \
                rng.normal(0, 0.1, shape)
        new[key] = torch.from_numpy(np.asarray(arr, np.float32)).to(val.device)
    module.load_state_dict(new)
    return {key: val.detach().cpu().numpy() for key, val in new.items()}
