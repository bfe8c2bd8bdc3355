"""The training-mode autograd Function of the six predictors whose kernels build no input gradient -- the five scene-graph
ones (SocialSTGCNN, SGCN, GPGraph, SocialDMRGCN, GraphTERNLight) and SocialImplicitLight: one skeleton, three hooks on the
model.

``native_parameters()``
    the parameters the kernels differentiate, in the order of the gradients
``native_forward(et, *inputs) -> (out, kept)``
    run the training forward on ``et`` (what ``et_params()`` returned); ``out`` is the output tensor, or a tuple whose
    further items are not differentiable; ``kept`` is a tuple of the tensors the backward needs (no None among them)
``native_backward(et, kept, g_out) -> gradients``
    one per parameter in ``native_parameters()`` order; None where the forward never reads the parameter
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable


def family_name(model):
    """the class that defines the hooks, as the messages name it (``GPGraph`` for a ``GPGraphSGCN``)"""
    return next(c.__name__ for c in type(model).__mro__ if "native_backward" in vars(c))


class TrainForward(torch.autograd.Function):
    """``forward(model, n_inputs, *inputs, *parameters)``.  Every parameter is an input, so autograd routes the gradients into
    ``.grad``; they are saved through ``save_for_backward`` with what the model keeps: the kernels read the weights in
    place, and an in-place change between forward and backward (an optimiser step) is caught by autograd's version
    counters.  No input gradient is built and the backward is differentiable once."""

    @staticmethod
    def forward(ctx, model, n_inputs, *args):
        et = model.et_params()  # the pointer table once: forward and backward see the same tensors
        out, kept = model.native_forward(et, *args[:n_inputs])
        ctx.model, ctx.et, ctx.n_kept = model, et, len(kept)
        ctx.save_for_backward(*kept, *args[n_inputs:])
        ctx.set_materialize_grads(False)
        if isinstance(out, tuple):
            ctx.mark_non_differentiable(*out[1:])
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, *_):
        need = ctx.needs_input_grad
        if g_out is None:
            return (None,) * len(need)
        model = ctx.model
        kept, params = ctx.saved_tensors[:ctx.n_kept], ctx.saved_tensors[ctx.n_kept:]
        if any(p.data_ptr() != q.data_ptr() for p, q in zip(params, model.native_parameters())):
            raise RuntimeError(f"{family_name(model)}: a parameter tensor was replaced between forward and backward")
        grads = model.native_backward(ctx.et, kept, g_out)
        lead = len(need) - len(params)
        return (None,) * lead + tuple(g if wanted else None for g, wanted in zip(grads, need[lead:]))


def train_forward(model, *inputs):
    """``model``'s training-mode forward on ``inputs`` (tensors on its device that require no gradient)"""
    return TrainForward.apply(model, len(inputs), *inputs, *model.native_parameters())
