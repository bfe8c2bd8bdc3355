"""The inputs of the Social-Implicit training tests that are not in a fixture, built without a GPU: seeded weights for the
shapes G25 has none for, and scenes v (T, N) whose first row puts every pedestrian in a chosen zone.  Shared by
tests/test_implicit_train_cpu.py (which asserts that the restatement leaves no ReLU of any of them undecided) and
tests/test_gpu_implicit_train.py, so the GPU comparison can never hide behind an undecided element."""
import numpy as np
import torch

from . import _golden as G

Z = G.load("g25_implicit.npz")
ET = dict(spatial_input=1, spatial_output=20, temporal_input=8, temporal_output=6, bins=[0, 0.01, 0.1, 1.2],
          noise_weight=[0.05, 1, 4, 8])
GEN = dict(spatial_input=1, spatial_output=12, temporal_input=10, temporal_output=5, bins=[0, 0.5, 2],
           noise_weight=[0.05, 1, 4])
BIG_BINS = [0, 0.1, 0.3, 0.6, 1.0, 1.5, 2.0, 2.5]
CONFIGS = {
    "et": ET,
    "gen": GEN,
    "s1": dict(ET, spatial_output=1),                                     # S = 1: every S tap but the middle one is padding
    "t1": dict(ET, spatial_output=5, temporal_input=1, temporal_output=1),  # T = T_out = 1
    "big": dict(spatial_input=1, spatial_output=64, temporal_input=16, temporal_output=16, bins=BIG_BINS,
                noise_weight=[1.0] * 8),                                  # the weights do not fit LDS: read in place
}
ZONE_RANGE = {"et": ((0.001, 0.009), (0.02, 0.09), (0.2, 1.1), (1.3, 3.0)), "gen": ((0.1, 0.4), (0.6, 1.9), (2.1, 4.0)),
              "big": tuple((lo + 0.02, hi - 0.02) for lo, hi in zip(BIG_BINS, BIG_BINS[1:] + [3.5]))}
ZONE_RANGE["s1"] = ZONE_RANGE["t1"] = ZONE_RANGE["et"]


def g25_state(prefix):
    return {k[len(prefix):]: np.array(Z[k]) for k in Z.files if k.startswith(prefix + "implicit_cells.")}


def module(config):
    """the library's module of ``config`` on the CPU: G25's weights for ``et`` and ``gen``, else the seeded default
    initialisation with every cell's global_w / local_w its own non-zero value (they initialise to 0)"""
    from eigentrajectory_amd.implicit import SocialImplicitLight
    torch.manual_seed(2800 + sorted(CONFIGS).index(config))
    m = SocialImplicitLight(**CONFIGS[config])
    if config in ("et", "gen"):
        m.load_state_dict({k: torch.from_numpy(v) for k, v in g25_state("net." if config == "et" else "gen.").items()},
                          strict=True)
    else:
        with torch.no_grad():
            for cell in m.implicit_cells:
                cell.global_w.fill_(0.5 + float(torch.rand(1)))
                cell.local_w.fill_(-0.5 - float(torch.rand(1)))
    return m


def state(m):
    return {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}


def scene(config, zone, seed, below=()):
    """v (T, N) float32: normal rows, the first row inside ``zone[i]``'s range with either sign; pedestrians listed in
    ``below`` get a first coefficient under bins[0] (only where bins[0] > 0)"""
    rng = np.random.default_rng(seed)
    n = len(zone)
    v = rng.normal(0, 1, (CONFIGS[config]["temporal_input"], n)).astype(np.float32)
    lo, hi = np.asarray(ZONE_RANGE[config], np.float64)[np.asarray(zone, np.int64)].T.reshape(2, n)
    v[0] = (rng.uniform(lo, hi) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    for i in below:
        v[0, i] = np.float32(0.01)
    return v


def grad_out(config, n, seed):
    c = CONFIGS[config]
    return np.random.default_rng(seed).normal(0, 1, (c["spatial_output"], c["temporal_output"], n)).astype(np.float32)


def chunk_zones(n, chunk, seed):
    """random zones 0..3, the two pedestrians either side of every chunk edge in ONE zone (3), so that zone's compacted
    neighbours straddle the edge"""
    zone = np.random.default_rng(seed).integers(0, 4, size=n)
    for edge in range(chunk, n, chunk):
        zone[max(edge - 2, 0):edge + 2] = 3
    return zone


MOVED_BINS = [0.25, 0.75, 1.5, 2.5]  # a first coefficient below 0.25 is in no zone


def synthetic_cases(chunk):
    """name -> (config, v, G, bins | None): the graph-form cases that no fixture holds"""
    cases = {}
    for n in (2, 3, 5):  # neighbour edges +-1, +-2 inside one zone
        cases[f"onezone{n}"] = ("et", scene("et", [2] * n, 10 + n), grad_out("et", n, 20 + n), None)
    cases["nozone3"] = ("et", scene("et", [0, 1, 0, 2, 1, 0, 2], 31), grad_out("et", 7, 32), None)  # zone 3 has no member
    # moved bins: |first| in (0.2, 1.1) or (1.3, 3.0); below 0.25 -> in no zone (pedestrians 1 and 4 are put there)
    v = scene("et", [2, 2, 3, 2, 2, 3, 3, 2], 33)
    v[0, [1, 4]] = np.asarray([0.125, -0.2], np.float32)
    cases["movedbins"] = ("et", v, grad_out("et", 8, 34), MOVED_BINS)
    cases["s1"] = ("s1", scene("s1", [3, 3, 1, 3, 0, 3, 1], 35), grad_out("s1", 7, 36), None)
    cases["t1"] = ("t1", scene("t1", [2, 2, 1, 2, 2, 0, 2], 37), grad_out("t1", 7, 38), None)
    cases["big"] = ("big", scene("big", [3, 4, 3, 3, 7, 4, 3, 0, 3], 39), grad_out("big", 9, 40), None)
    for n in (chunk - 1, chunk, chunk + 1, 2 * chunk + 1):
        cases[f"chunk{n}"] = ("et", scene("et", chunk_zones(n, chunk, 41 + n), 42 + n), grad_out("et", n, 43 + n), None)
    return cases
