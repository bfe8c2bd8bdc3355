"""Social-STGCNN's forward (n_stgcnn = 1, input_feat = 1) in stock torch functions over a module's own tensors,
``F.batch_norm(training=True)`` included, differentiable by autograd: our own restatement of what
csrc/et_stgcnn_train.hip computes (tests/_stgcnn_train_np.py is the numpy form).  Used by tests/test_stgcnn_train_cpu.py as
the autograd reference, by tests/test_gpu_stgcnn_train.py as the fp32 network and by tools/time_train.py --predictor stgcnn as the
stock-torch network.  Not a test module itself."""
import copy

import torch
import torch.nn.functional as F


def clone(module, dtype=torch.float64, device="cpu"):
    """a deep copy of a SocialSTGCNN in ``dtype`` on ``device`` (its own parameters and buffers)"""
    return copy.deepcopy(module).to(device=device, dtype=dtype)


def _bn(x, m, training):
    y = F.batch_norm(x, m.running_mean, m.running_var, m.weight, m.bias, training, m.momentum, m.eps)
    if training:
        m.num_batches_tracked += 1   # (nn.BatchNorm2d.forward does this; F.batch_norm does not)
    return y


def forward(m, v, a, training=True):
    """m: a SocialSTGCNN (any dtype / device), v (1, 1, K, N), a (K, N, N) -> (1, S, k, N).  With ``training`` the three
    BatchNorms use batch statistics and update the module's buffers, as the reference in training mode does."""
    p = next(m.parameters())
    v = torch.as_tensor(v).to(device=p.device, dtype=p.dtype)
    a = torch.as_tensor(a).to(device=p.device, dtype=p.dtype)
    blk = m.st_gcns[0]
    K, S = m.seq_len, m.output_feat
    res = v if blk.residual is None else _bn(F.conv2d(v, blk.residual[0].weight, blk.residual[0].bias), blk.residual[1],
                                             training)
    x = F.conv2d(v, blk.gcn.conv.weight, blk.gcn.conv.bias)
    n, kc, t, w = x.shape
    x = torch.einsum("nkctv,kvw->nctw", x.view(n, K, kc // K, t, w), a).contiguous()
    x = F.prelu(_bn(x, blk.tcn[0], training), blk.tcn[1].weight)
    x = _bn(F.conv2d(x, blk.tcn[2].weight, blk.tcn[2].bias, padding=(1, 0)), blk.tcn[3], training)
    x = F.prelu(x + res, blk.prelu.weight)
    x = x.view(x.shape[0], x.shape[2], x.shape[1], x.shape[3])
    x = F.prelu(F.conv2d(x, m.tpcnns[0].weight, m.tpcnns[0].bias, padding=1), m.prelus[0].weight)
    for j in range(1, m.n_txpcnn - 1):
        x = F.prelu(F.conv2d(x, m.tpcnns[j].weight, m.tpcnns[j].bias, padding=1), m.prelus[j].weight) + x
    x = F.conv2d(x, m.tpcnn_ouput.weight, m.tpcnn_ouput.bias, padding=1)
    return x.view(x.shape[0], x.shape[2], x.shape[1], x.shape[3])


class Twin(torch.nn.Module):
    """a SocialSTGCNN's own tensors behind :func:`forward`: the stock-torch network as a predictor module (training mode
    follows ``.train()`` / ``.eval()``)"""

    def __init__(self, base):
        super().__init__()
        self.base = base

    def forward(self, v, a):
        return forward(self.base, v, a, self.training)


def grads(m, v, a, d_out):
    """one training-mode forward and backward -> (out, {parameter name: gradient, zeros where .grad is None}); the module's
    buffers are updated"""
    for q in m.parameters():
        q.grad = None
    out = forward(m, v, a)
    out.backward(torch.as_tensor(d_out).to(out))
    return out.detach(), {k: (torch.zeros_like(q) if q.grad is None else q.grad.detach().clone())
                          for k, q in m.named_parameters()}


def buffers(m):
    """{buffer name: numpy array} of the module's BatchNorm buffers"""
    return {k: b.detach().cpu().numpy().copy() for k, b in m.named_buffers()}
