"""The scene preamble every ``ops.*_forward_scenes`` wrapper starts with, on CPU tensors (``scene_offsets`` takes any
device): what it returns for ``scene_sizes`` given as None, a list or a tensor, and what it refuses.  No library call."""
import pytest
import torch

from eigentrajectory_amd import ops

CPU = torch.device("cpu")
K = 6


def batch(n, scene_sizes, k=K, C_obs=None, nrm=None):
    C_obs = torch.arange(K * n, dtype=torch.float64).reshape(K, n) if C_obs is None else C_obs
    nrm = torch.ones(4, n) if nrm is None else nrm
    return ops._scene_batch("some_forward_scenes", CPU, C_obs, nrm, k, scene_sizes)


def test_no_scene_sizes_is_one_scene_of_all_rows():
    b = batch(7, None)
    assert (b.n, b.sizes, b.off, b.n_scenes, b.max_n) == (7, [7], None, 0, 7)
    assert b.C_obs.dtype == torch.float32 and b.C_obs.shape == (K, 7) and b.C_obs.is_contiguous()
    assert b.nrm.shape == (4, 7) and b.C_obs.device == b.nrm.device == CPU
    b = batch(0, None)
    assert (b.n, b.sizes, b.off, b.n_scenes, b.max_n) == (0, [0], None, 0, 0)


@pytest.mark.parametrize("as_tensor", [False, True])
def test_listed_scenes(as_tensor):
    sizes = [0, 3, 0, 4, 0]
    b = batch(7, torch.tensor(sizes, dtype=torch.int64) if as_tensor else sizes)
    assert (b.n, b.sizes, b.n_scenes, b.max_n) == (7, sizes, 5, 4)
    assert all(type(s) is int for s in b.sizes)
    assert b.off.dtype == torch.int32 and b.off.device == CPU and b.off.tolist() == [0, 0, 3, 3, 7, 7]
    b = batch(7, torch.tensor([7]) if as_tensor else [7])  # one listed scene is still listed: offsets, one scene
    assert (b.sizes, b.n_scenes, b.max_n, b.off.tolist()) == ([7], 1, 7, [0, 7])


def test_an_empty_list_takes_no_rows():
    b = batch(0, [])
    assert (b.n, b.sizes, b.n_scenes, b.max_n) == (0, [], 0, 0)
    assert b.off.dtype == torch.int32 and b.off.tolist() == [0]
    with pytest.raises(ValueError, match="some_forward_scenes: no scenes for 3 rows"):
        batch(3, [])
    with pytest.raises(ValueError, match="no scenes for 3 rows"):
        batch(3, torch.zeros((0,), dtype=torch.int64))


@pytest.mark.parametrize("sizes", [[3, 3], [3, 5], [8, -1], [-7]])
def test_sizes_must_be_non_negative_and_sum_to_the_rows(sizes):
    with pytest.raises(ValueError):
        batch(7, sizes)


def test_shapes_are_checked_against_k():
    with pytest.raises(ValueError):
        batch(7, None, C_obs=torch.zeros(K))                     # 1-D C_obs
    with pytest.raises(ValueError, match="some_forward_scenes") as e:
        batch(7, None, k=K + 1)                                  # K rows where K + 1 are expected
    assert "(6, 7)" in str(e.value) and "(4, 7)" in str(e.value) and "7" in str(e.value).split("k =")[-1]
    with pytest.raises(ValueError, match="some_forward_scenes"):
        batch(7, None, nrm=torch.ones(1, 7))                     # fewer than the two rows that hold the positions
    with pytest.raises(ValueError, match="some_forward_scenes"):
        batch(7, None, nrm=torch.ones(4, 8))                     # n + 1 columns
    with pytest.raises(ValueError):
        batch(7, None, nrm=torch.ones(7))                        # 1-D nrm
    assert batch(7, [7], nrm=torch.ones(2, 7)).nrm.shape == (2, 7)  # two rows are enough
