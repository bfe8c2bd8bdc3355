"""numpy restatement of csrc/et_curve.hip (et_curve_fit_batch) for one fit: the same fp32 operations in the same order
(unfused, correctly rounded sqrt and division), the same fp64 bias corrections and fixed-point loss, the same best-step
rule.  The GPU tests compare the kernel with it bit for bit."""
import math

import numpy as np

FIX = 2.0 ** 28        # loss units
FIX_CLAMP = 2.0 ** 26  # per-pedestrian clamp


def curve_fit_np(traj, basis, steps, lr=1e-4, betas=(0.9, 0.999), eps=1e-8):
    """traj (N,T,2), basis (T,ncp) -> dict recon (N,T,2) f32, cp (N,ncp,2) f32, loss (steps,) f64, best int,
    fixed (steps,) int64 (the per-step fixed-point sums)."""
    f32 = np.float32
    traj = np.ascontiguousarray(traj, dtype=f32)
    B = np.ascontiguousarray(basis, dtype=f32)
    n, T, _ = traj.shape
    C = B.shape[1]
    x, y = traj[:, :, 0], traj[:, :, 1]
    sx = (x[:, T - 1] - x[:, 0]) / f32(C - 1)
    sy = (y[:, T - 1] - y[:, 0]) / f32(C - 1)
    cx, cy = np.empty((n, C), f32), np.empty((n, C), f32)
    cx[:, 0], cy[:, 0] = x[:, 0], y[:, 0]
    for i in range(1, C):
        cx[:, i] = cx[:, i - 1] + sx
        cy[:, i] = cy[:, i - 1] + sy
    mx, my, vx, vy, ax, ay = (np.zeros((n, C), f32) for _ in range(6))
    b1, b2 = float(betas[0]), float(betas[1])
    w1, b2f, c2f, epsf = f32(1.0 - b1), f32(b2), f32(1.0 - b2), f32(eps)
    scale = f32(1.0) / f32(n * T)
    p1 = p2 = 1.0

    def forward(cx, cy):
        rx = B[None, :, 0] * cx[:, 0:1]
        ry = B[None, :, 0] * cy[:, 0:1]
        for i in range(1, C):
            rx = rx + B[None, :, i] * cx[:, i:i + 1]
            ry = ry + B[None, :, i] * cy[:, i:i + 1]
        return rx, ry

    fixed = np.zeros(steps, np.int64)
    best, best_v, best_cp = -1, None, None
    with np.errstate(divide="ignore", invalid="ignore"):
        for st in range(steps):
            rx, ry = forward(cx, cy)
            rx, ry = rx - x, ry - y
            nn = np.sqrt(rx * rx + ry * ry)
            a = np.zeros(n, np.float64)
            for t in range(T):
                a = a + nn[:, t].astype(np.float64)
            q = np.rint(np.fmin(a, FIX_CLAMP) * FIX).astype(np.int64)
            fixed[st] = q.sum()
            if best_v is None or fixed[st] < best_v:
                best, best_v, best_cp = st, fixed[st], (cx.copy(), cy.copy())
            sc = np.where(nn == 0, f32(0), scale / nn).astype(f32)
            grx, gry = rx * sc, ry * sc
            gx = B[None, 0, :] * grx[:, 0:1]
            gy = B[None, 0, :] * gry[:, 0:1]
            for t in range(1, T):
                gx = gx + B[None, t, :] * grx[:, t:t + 1]
                gy = gy + B[None, t, :] * gry[:, t:t + 1]
            ax, ay = ax + gx, ay + gy  # the reference never zeroes the gradient: .grad accumulates over the steps
            gx, gy = ax, ay
            p1 = p1 * b1
            p2 = p2 * b2
            nss = f32(-(lr / (1.0 - p1)))
            bc2s = f32(math.sqrt(1.0 - p2))
            mx = mx + w1 * (gx - mx)
            my = my + w1 * (gy - my)
            vx = vx * b2f + (c2f * gx) * gx
            vy = vy * b2f + (c2f * gy) * gy
            ex = np.sqrt(vx) / bc2s + epsf
            ey = np.sqrt(vy) / bc2s + epsf
            cx = cx + (nss * mx) / ex
            cy = cy + (nss * my) / ey
    bx, by = best_cp
    rx, ry = forward(bx, by)
    loss = np.asarray([(float(v) * (1.0 / FIX)) / float(n * T) for v in fixed])
    return dict(recon=np.stack([rx, ry], axis=-1), cp=np.stack([bx, by], axis=-1), loss=loss, best=best, fixed=fixed)
