from .ann_index import ANNIndex
from .forest import CompiledForest, LeafFeatures
from .knn import FlatIndex, PQIndex
from .predictor import BatchPredictor
from .rp_forest import ForestIndex

__all__ = ["ANNIndex", "BatchPredictor", "CompiledForest", "FlatIndex",
           "ForestIndex", "LeafFeatures", "PQIndex"]
