"""The shared training autograd Function (eigentrajectory_amd/_native_train.py) is differentiable once, for each of the five
predictors that run through it: the gradients of a first ``torch.autograd.grad(..., create_graph=True)`` cannot be
differentiated again."""
import pytest
import torch

from . import _dmrgcn_train_cases as DC
from . import _gpgraph_train_cases as GC
from . import _implicit_train_cases as IC
from . import _sgcn_np as SN
from . import _sgcn_train_cases as SC
from . import _stgcnn_train_cases as TC
from ._gpu_common import *  # noqa: F401,F403 -- fixtures (dev, ops) and helpers

pytestmark = pytest.mark.gpu
N = 3


def _stgcnn(dev):
    v, a = TC.scene("et", N)
    return TC.module("et", dev), (T(v[None, None], dev), T(a, dev))


def _sgcn(dev):
    ids, idt = SN.bridge_identities(SN.CONFIGS["et"]["k"] + 2, N)
    return SC.module("et", dev), (T(SC.scene("et", N)[None, :, :, None], dev), [T(ids, dev), T(idt, dev)])


def _gpgraph(dev):
    va, vr = GC.scene("et", N)
    m = GC.set_threshold(GC.module("et", dev), GC.case_state("et", [va]))
    return m, (T(va[None, None], dev), T(vr[None], dev))


def _dmrgcn(dev):
    v, a = DC.scene("et", N)
    return DC.module("et", dev), (T(v[None, None], dev), T(a[None], dev))


def _implicit(dev):
    return IC.module("et").to(dev), (T(IC.scene("et", [0, 1, 3], 11)[None, None], dev),)


@pytest.mark.parametrize("family", [_stgcnn, _sgcn, _gpgraph, _dmrgcn, _implicit], ids=lambda f: f.__name__[1:])
def test_the_backward_is_differentiable_once(dev, family):
    import eigentrajectory_amd as ET
    m, inputs = family(dev)
    m = ET.enable_native_training(m.train())
    params = list(m.native_parameters())
    for square in (False, True):   # d (sum out^2) = 2 out carries a graph into the backward, d (sum out) does not
        out = m(*inputs)
        out = out[0] if isinstance(out, tuple) else out
        assert out.requires_grad
        loss = (out * out).sum() if square else out.sum()
        grads = torch.autograd.grad(loss, params, create_graph=True, allow_unused=True)
        used = [g for g in grads if g is not None]
        assert len(used) >= len(params) - 3 and all(bool(torch.isfinite(g).all()) for g in used)
        with pytest.raises(RuntimeError, match="once_differentiable" if square else None):
            sum(g.sum() for g in used).backward()
