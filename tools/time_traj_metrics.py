#!/usr/bin/env python3
"""Launch time of the scene-batched test metrics (et_traj_metrics / et_anchor_reconstruct_metrics_scenes), HIP events,
warmed: univ-all's shape (24 334 pedestrians in the test split's 947 scenes, S = 20) and a synthetic 1e6 rows in scenes of
32.  Synthetic trajectories (the time does not depend on the values beyond the collision pass's early exits).
    python tools/time_traj_metrics.py [--reps 20]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for _ in range(reps):
        ev[0].record()
        fn()
        ev[1].record()
        ev[1].synchronize()
        ms.append(ev[0].elapsed_time(ev[1]))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    from eigentrajectory_amd import ops
    from tests import _golden as G
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    _, _, sse = G.dataset("univ", "test")
    shapes = {"univ_all": [int(e - s) for s, e in sse], "synthetic_1e6_scenes_of_32": [32] * (1_000_000 // 32)}
    res = {}
    for name, sizes in shapes.items():
        n, S, k = sum(sizes), 20, 6
        gt = torch.from_numpy(np.cumsum(rng.normal(0, 0.3, (n, 12, 2)), axis=1).astype(np.float32)
                              + rng.uniform(-4, 4, (n, 1, 2)).astype(np.float32)).to(dev)
        pred = gt[None] + 0.3 * torch.randn((S, n, 12, 2), device=dev)
        U = [torch.from_numpy(np.linalg.qr(rng.normal(size=(24, k)))[0].astype(np.float32)).to(dev) for _ in range(2)]
        C = 0.5 * torch.randn((k, n, S), device=dev)
        nrm = torch.cat([gt[:, 0].T, 0.3 * torch.randn((2, n), device=dev)]).contiguous()
        off = ops.scene_offsets(sizes, n, dev)
        outs = [torch.empty((n,), device=dev) for _ in range(4)] + [torch.empty((n,), device=dev, dtype=torch.int32)]
        P = [o.data_ptr() for o in outs]
        L = ops.L

        def tensor_form(col=True):
            L.call("et_traj_metrics", L.ptr(pred), n, S, 12, L.ptr(gt), L.ptr(off), len(sizes), *map(L.ptr, outs[:3]),
                   L.ptr(outs[3] if col else None), L.ptr(outs[4]), L.stream(dev))

        def fused():
            L.call("et_anchor_reconstruct_metrics_scenes", L.ptr(C), n, S, k, 8, 12, None, L.ptr(nrm), None, None, None,
                   L.ptr(U[0]), L.ptr(U[1]), ops.MODE_SPLIT, 0.3, L.ptr(gt), L.ptr(off), len(sizes), *map(L.ptr, outs),
                   L.stream(dev))
        res[name] = dict(rows=n, scenes=len(sizes), S=S, tensor_ms=timed(tensor_form, args.reps),
                         tensor_no_col_ms=timed(lambda: tensor_form(False), args.reps), fused_ms=timed(fused, args.reps))
        print(json.dumps({name: res[name]}), flush=True)
    return res


if __name__ == "__main__":
    main()
