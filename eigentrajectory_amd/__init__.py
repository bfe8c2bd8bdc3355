"""eigentrajectory_amd -- MI355X-native (gfx950) EigenTrajectory SVD-descriptor path.

Same public surface as the reference package (EigenTrajectory/__init__.py:1-2
exports ``EigenTrajectory`` and ``TrajNorm``); the descriptor / anchor / k-means
modules are importable for the callers that use them directly.  All compute goes
through the C ABI of ``libetamd.so`` (include/eigentraj.h).
"""
from .model import EigenTrajectory
from .normalizer import TrajNorm
from .descriptor import ETDescriptor
from .anchor import ETAnchor
from .kmeans import BatchKMeans
from .stgcnn import SocialSTGCNN
from .sgcn import SGCN
from .dmrgcn import SocialDMRGCN
from .pecnet import PECNet, enable_native_training
from .lbebm import LBEBM
from .implicit import SocialImplicitLight
from .agentformer import AgentFormerLight
from .graphtern import GraphTERNLight
from .gpgraph import GPGraph, GPGraphSGCN, GPGraphSTGCNN, get_GPGraph_SGCN_model, get_GPGraph_STGCNN_model

__all__ = ["EigenTrajectory", "TrajNorm", "ETDescriptor", "ETAnchor", "BatchKMeans", "SocialSTGCNN", "SGCN", "GPGraph",
           "GPGraphSGCN", "get_GPGraph_SGCN_model", "GPGraphSTGCNN", "get_GPGraph_STGCNN_model", "SocialDMRGCN", "PECNet",
           "LBEBM", "SocialImplicitLight", "AgentFormerLight", "GraphTERNLight", "enable_native_training"]
