from .sharded_fm import ShardedFMModel
from .ring import RingDataParallel, broadcast_params, allreduce_gradients
from .sharded_widedeep import ShardedWideDeepModel
from .sharded_ffm import ShardedFFMModel
from .ps import PSConfig, PSShard, PSWorker, ps_train_fm, setup_pair_groups
from .ps_dense import (DenseTable, dense_offsets, dense_range,
                       mlp_dense_spec)
from .ps_widedeep import (ps_train_widedeep, widedeep_dense_spec,
                          widedeep_grads)

__all__ = ["ShardedFMModel", "ShardedWideDeepModel", "ShardedFFMModel", "RingDataParallel", "broadcast_params",
           "allreduce_gradients", "PSConfig", "PSShard", "PSWorker",
           "ps_train_fm", "setup_pair_groups", "DenseTable",
           "dense_offsets", "dense_range", "mlp_dense_spec",
           "ps_train_widedeep", "widedeep_dense_spec", "widedeep_grads"]
