from .ann_index import ANNIndex
from .forest import CompiledForest, LeafFeatures
from .predictor import BatchPredictor

__all__ = ["ANNIndex", "BatchPredictor", "CompiledForest", "LeafFeatures"]
