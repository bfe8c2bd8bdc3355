"""What the five scene-graph predictors' training wrappers share in eigentrajectory_amd/ops.py, on the host: the flat
gradient buffer's views, the scene-size preamble, the workspace layouts by name and the packed keep mask's offsets."""
import ctypes as C

import pytest
import torch

from eigentrajectory_amd import _lib, ops

from . import _dmrgcn_train_cases as DC
from . import _gpgraph_train_cases as GC
from . import _graphtern_train_cases as RC
from . import _sgcn_train_cases as SC
from . import _stgcnn_train_cases as TC

FAMILIES = {"stgcnn": TC, "sgcn": SC, "gpgraph_sgcn": GC, "dmrgcn": DC, "graphtern": RC}


@pytest.mark.parametrize("family", FAMILIES)
def test_grad_views_name_every_parameter(family):
    model = FAMILIES[family].module("et")
    grad_views = getattr(ops, f"{family}_grad_views")
    named = list(model.named_parameters())
    numel = sum(p.numel() for _, p in named)
    flat = torch.zeros(numel)
    views = grad_views(model, flat)
    assert list(views) == [name for name, _ in named]
    assert [v.shape for v in views.values()] == [p.shape for _, p in named]
    at = 0
    for v in views.values():   # consecutive views of the buffer itself
        assert v.data_ptr() == flat.data_ptr() + 4 * at
        at += v.numel()
    with pytest.raises(ValueError, match=f"{family}_grad_views: {numel - 1} floats for parameters of {numel}"):
        grad_views(model, torch.zeros(numel - 1))


def test_scene_sizes_of_a_list_a_tensor_and_none():
    dev = torch.device("cpu")
    sizes = [3, 0, 1, 5]
    for given in (sizes, torch.tensor(sizes, dtype=torch.int64)):
        got, off, n_scenes = ops._scene_sizes(given, 9, dev)
        assert got == sizes and all(type(s) is int for s in got) and n_scenes == 4
        assert off.dtype == torch.int32 and off.tolist() == [0, 3, 3, 4, 9]
    assert ops._scene_sizes(None, 9, dev) == ([9], None, 0)   # one scene of every row: no offsets
    got, off, n_scenes = ops._scene_sizes([], 0, dev)
    assert got == [] and n_scenes == 0 and off.dtype == torch.int32 and off.tolist() == [0]
    with pytest.raises(ValueError, match="sum to the 9 rows"):
        ops._scene_sizes([3, 5], 9, dev)
    b = ops._scene_batch("some_forward_scenes", dev, torch.zeros((6, 9)), torch.zeros((4, 9)), 6, sizes)
    assert (b.sizes, b.n_scenes, b.max_n, b.off.tolist()) == (sizes, 4, 5, [0, 3, 3, 4, 9])


@pytest.mark.parametrize("family", FAMILIES)
def test_layout_names_cover_the_fields(family):
    names = getattr(_lib, f"{family.upper()}_TRAIN_LAYOUT_NAMES")
    assert len(names) == getattr(_lib, f"{family.upper()}_TRAIN_LAYOUT_FIELDS") == len(set(names))
    assert names[-1] == "total"


@pytest.mark.parametrize("family", ["dmrgcn", "graphtern"])
def test_layout_tail_by_name(family):
    """the tail the scene training units share, from the library's own answers: N = 3 pedestrians in one scene"""
    params = FAMILIES[family].host_params()   # a host struct: no launch, no device
    lay = ops._layout(f"et_{family}_train_layout", getattr(_lib, f"{family.upper()}_TRAIN_LAYOUT_NAMES"), params, 3, 1)
    assert lay.per > 0 and lay.grads > 0
    assert lay.partials == 3 * lay.per
    assert lay.total == lay.partials + lay.grads
    assert lay.total * 4 == getattr(_lib.lib(), f"et_{family}_train_workspace_bytes")(C.byref(params), 3, 1)


def test_keep_offsets_agree():
    """the 513 scene is over both training caps and takes no room in the packed mask"""
    for keep_offsets in (ops.dmrgcn_keep_offsets, ops.graphtern_keep_offsets):
        off, total = keep_offsets([3, 0, 1, 5, 513])
        assert off.dtype == torch.int64 and off.tolist() == [0, 9, 9, 10, 35, 35] and total == 35
