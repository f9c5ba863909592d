"""spconv.pytorch: SparseConvTensor, SparseModule, SubMConv3d (gaussiancity_amd.sparse) and `modules`."""
from gaussiancity_amd.sparse import SparseConvTensor, SparseModule, SubMConv3d  # noqa: F401

from . import modules  # noqa: F401
