from .ann_index import ANNIndex
from .forest import CompiledForest, LeafFeatures
from .knn import FlatIndex, PQIndex
from .predictor import BatchPredictor

__all__ = ["ANNIndex", "BatchPredictor", "CompiledForest", "FlatIndex",
           "LeafFeatures", "PQIndex"]
