"""numpy restatement of the reference's per-pedestrian test metrics (utils/metrics.py:30-155) in the arithmetic the HIP
kernel (eigentrajectory_amd/csrc/et_metrics.hip) uses: the CPU pin of tests/golden/g16 and the GPU tests' yardstick.

pred (S,N,T,2), gt (N,T,2) float32; scene_sizes: pedestrians per scene in row order (None: one scene).
"""
import numpy as np

F32 = np.float32


def _fma32(a, b, c):
    """fp32 fused multiply-add through fp64 (a * b is exact there)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def pair_norm(dx, dy):
    """ATen's CPU 2-norm of a pair: sqrt(fma(dy, dy, dx * dx)) in fp32 (utils/metrics.py:84, :151)."""
    return np.sqrt(_fma32(dy, dy, (dx * dx).astype(F32)))


def tree_sum(x):
    """Pairwise sum over the last axis as a binary counter (12 terms: (0..7) + (8..11), every block by halves): for a
    constant series this is ATen's mean's sum bit for bit (utils/metrics.py:119)."""
    T = x.shape[-1]
    stack = {}
    for t in range(T):
        c, l = x[..., t], 0
        while (t >> l) & 1:
            c = (stack[l] + c).astype(F32)
            l += 1
        stack[l] = c
    acc = None
    for l in range(T.bit_length()):
        if (T >> l) & 1:
            acc = stack[l] if acc is None else (stack[l] + acc).astype(F32)
    return acc


def ade_fde_best(pred, gt):
    """utils/metrics.py:73-102 and :114: best-of-S ADE / FDE and the arg-min sample of the final error (first NaN wins)."""
    d = pair_norm(pred[..., 0] - gt[None, ..., 0], pred[..., 1] - gt[None, ..., 1])  # (S,N,T)
    ade = (d.astype(np.float64).sum(axis=-1) / d.shape[-1]).astype(F32).min(axis=0)
    fde = d[..., -1].min(axis=0)
    best = np.argmin(d[..., -1], axis=0).astype(np.int32)
    return ade, fde, best


def tcc(pred, gt, best):
    """utils/metrics.py:105-130 for the sample ``best`` of each row."""
    T = gt.shape[1]
    pb = pred[best, np.arange(gt.shape[0])]  # (N,T,2)
    factor = F32(1.0 / (T - 1))
    out = []
    for c in range(2):
        p, g = pb[..., c], gt[..., c]
        a = (p - (tree_sum(p) / F32(T))[:, None]).astype(F32)
        b = (g - (tree_sum(g) / F32(T))[:, None]).astype(F32)
        fa, fb = (factor * a).astype(F32), (factor * b).astype(F32)
        pg = pp = gg = np.zeros(gt.shape[0], F32)
        for t in range(T):
            pg, pp, gg = _fma32(fa[:, t], b[:, t], pg), _fma32(fa[:, t], a[:, t], pp), _fma32(fb[:, t], b[:, t], gg)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = ((pg / np.sqrt(pp)).astype(F32) / np.sqrt(gg)).astype(F32)
        out.append(np.where(np.isnan(r), F32(0), np.clip(r, F32(-1), F32(1))).astype(F32))
    return ((out[0] + out[1]) / F32(2)).astype(F32)


def dense_path(pred):
    """utils/metrics.py:140-150: (S,N,T,2) -> (S,N,M,2), M = min(14, 1 + 4 (T-1)); fp64 running sum, fp32 instants."""
    T = pred.shape[2]
    M = min(14, 1 + 4 * (T - 1))
    steps = pred[:, :, :min(T, 5)]
    rel = ((steps[:, :, 1:] - steps[:, :, :-1]).astype(F32) / F32(4)).astype(F32)
    seq = np.concatenate([steps[:, :, :1], np.repeat(rel, 4, axis=2)], axis=2)[:, :, :M]
    return np.cumsum(seq.astype(np.float64), axis=2).astype(F32)


def collisions(pred, scene_sizes=None, chunk=256):
    """utils/metrics.py:133-155 within each scene -> collision bits (S,N) bool and, per (sample, pedestrian), the minimum
    over the other pedestrians of the pair's window minimum (S,N) float32 (NaN pairs left out, +inf without a partner)."""
    S, N = pred.shape[:2]
    sizes = [N] if scene_sizes is None else [int(v) for v in scene_sizes]
    dense = dense_path(pred)
    bits = np.zeros((S, N), bool)
    mind = np.full((S, N), np.inf, F32)
    at = 0
    for n in sizes:
        d_sc = dense[:, at:at + n]
        for i0 in range(0, n, chunk):
            di = d_sc[:, i0:i0 + chunk]                        # (S,b,M,2)
            dx = di[:, :, None, :, 0] - d_sc[:, None, :, :, 0]  # (S,b,n,M)
            dy = di[:, :, None, :, 1] - d_sc[:, None, :, :, 1]
            m = pair_norm(dx, dy).min(axis=-1)                  # NaN propagates (:152)
            b = np.arange(di.shape[1])
            m[:, b, i0 + b] = np.inf                            # the +eye: never with itself
            bits[:, at + i0:at + i0 + di.shape[1]] = (m < F32(0.2)).any(axis=-1)
            mind[:, at + i0:at + i0 + di.shape[1]] = np.where(np.isnan(m), np.inf, m).min(axis=-1)
        at += n
    return bits, mind


def metrics(pred, gt, scene_sizes=None):
    """-> dict ADE, FDE, TCC, COL (N,) float32, best (N,) int32, col_bits (S,N) bool, min_dist (S,N)."""
    pred, gt = np.asarray(pred, F32), np.asarray(gt, F32)
    ade, fde, best = ade_fde_best(pred, gt)
    bits, mind = collisions(pred, scene_sizes)
    col = ((bits.sum(axis=0).astype(F32) / F32(pred.shape[0])) * F32(100)).astype(F32)
    return dict(ADE=ade, FDE=fde, TCC=tcc(pred, gt, best), COL=col, best=best, col_bits=bits, min_dist=mind)
