"""sparsepoly_amd -- MI355X-native proximal coordinate-descent core for sparse
factorization machines; drop-in for the pcd / pbcd path of neonnnnn/sparsepoly
(reference ``sparsepoly/__init__.py:1-19`` exports the same estimator and
regularizer names)."""
from .bank import ModelBank
from .model_selection import CVResult, cross_validate_path, fold_ids
from .pairwise import (SparseFactorizationMachineRanker, draw_u64, restate_sample,
                       sample_triples)
from .regularizer import L1, L21, OmegaCS, OmegaTI, SquaredL12, SquaredL21
from .sparse_all_subsets import SparseAllSubsetsClassifier, SparseAllSubsetsRegressor
from .sparse_factorization_machines import (
    SparseFactorizationMachineClassifier,
    SparseFactorizationMachineRegressor,
)

__all__ = [
    "CVResult",
    "L1",
    "L21",
    "ModelBank",
    "OmegaCS",
    "OmegaTI",
    "SquaredL12",
    "SquaredL21",
    "SparseAllSubsetsClassifier",
    "SparseAllSubsetsRegressor",
    "SparseFactorizationMachineClassifier",
    "SparseFactorizationMachineRanker",
    "SparseFactorizationMachineRegressor",
    "sample_triples",
    "draw_u64",
    "restate_sample",
    "cross_validate_path",
    "fold_ids",
]
