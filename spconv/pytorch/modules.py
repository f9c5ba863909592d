"""spconv.pytorch.modules: the module base class and its test."""
from gaussiancity_amd.sparse import SparseModule, is_spconv_module  # noqa: F401
