"""t-SNE of descriptor coefficients on the GPU: the subset of sklearn.manifold.TSNE that the reference's
script/plot_coeff_tsne.py uses (Barnes-Hut pipeline, n_components=2), with the repulsive term summed exactly instead of
through a quadtree.  Every stage is a HIP kernel (csrc/et_tsne.hip); there is no CPU path."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from . import ops


class TSNE:
    """``TSNE(perplexity=30, early_exaggeration=12, learning_rate="auto", max_iter=1000, init="pca", random_state=None)``.

    ``fit_transform(X)`` sets ``embedding_`` (N,2) float32 numpy, ``kl_divergence_``, ``n_iter_`` and
    ``learning_rate_`` as sklearn does.  ``init`` is "pca" or an (N,2) array.  ``random_state`` is accepted for the
    signature: the PCA initialisation here is an exact eigen-decomposition and uses no random numbers."""

    def __init__(self, n_components=2, *, perplexity=30.0, early_exaggeration=12.0, learning_rate="auto",
                 max_iter=1000, init="pca", random_state=None, device=None):
        if n_components != 2:
            raise ValueError(f"TSNE: n_components={n_components} not supported (2 only)")
        if not perplexity > 0:
            raise ValueError(f"TSNE: perplexity={perplexity} must be > 0")
        if not early_exaggeration >= 1:
            raise ValueError(f"TSNE: early_exaggeration={early_exaggeration} must be >= 1")
        if not (learning_rate == "auto" or (not isinstance(learning_rate, str) and learning_rate > 0)):
            raise ValueError(f"TSNE: learning_rate={learning_rate!r} must be 'auto' or > 0")
        if int(max_iter) < 250:
            raise ValueError(f"TSNE: max_iter={max_iter} must be >= 250")
        if isinstance(init, str) and init != "pca":
            raise ValueError(f"TSNE: init={init!r} not supported ('pca' or an array)")
        self.n_components = n_components
        self.perplexity = float(perplexity)
        self.early_exaggeration = float(early_exaggeration)
        self.learning_rate = learning_rate
        self.max_iter = int(max_iter)
        self.init = init
        self.random_state = random_state
        self.device = device

    def _check(self, X):
        X = torch.as_tensor(np.asarray(X, dtype=np.float32) if not torch.is_tensor(X) else X)
        if X.dim() != 2:
            raise ValueError(f"TSNE: X must be 2-D, got {tuple(X.shape)}")
        n, d = X.shape
        if n < 2:
            raise ValueError(f"TSNE: {n} samples, at least 2 needed")
        if d > 32:
            raise ValueError(f"TSNE: {d} features, at most 32 supported")
        if isinstance(self.init, str) and d < 2:
            raise ValueError(f"TSNE: init='pca' needs at least 2 features, got {d}")
        if self.perplexity >= n:
            raise ValueError(f"TSNE: perplexity ({self.perplexity}) must be less than n_samples ({n})")
        if not isinstance(self.init, str):
            init = np.asarray(self.init)
            if init.shape != (n, 2):
                raise ValueError(f"TSNE: init has shape {init.shape}, expected {(n, 2)}")
        return X

    def fit_transform(self, X, y=None):
        X = self._check(X)
        n = X.shape[0]
        dev = torch.device(self.device) if self.device is not None else L.require_device(X)
        X = X.to(dev, torch.float32).contiguous()
        if self.learning_rate == "auto":  # numpy 2: an np.float64, the update runs in fp64
            self.learning_rate_ = np.maximum(n / self.early_exaggeration / 4, 50)
        else:
            self.learning_rate_ = self.learning_rate
        aff = ops.tsne_affinities(X, self.perplexity)
        if isinstance(self.init, str):
            Y0 = ops.tsne_pca_init(X)
        else:
            Y0 = torch.as_tensor(np.asarray(self.init, dtype=np.float32)).to(X.device)
        Y, kl, it = ops.tsne_optimize(Y0, aff["indptr"], aff["indices"], aff["P"], self.early_exaggeration,
                                      float(self.learning_rate_), self.max_iter)
        self.embedding_ = Y.cpu().numpy()
        self.kl_divergence_ = kl
        self.n_iter_ = it
        return self.embedding_

    def fit(self, X, y=None):
        self.fit_transform(X)
        return self
