"""Drop-in for torch_scatter on the MI355X: segment_csr with a 1-D indptr (gaussiancity_amd.sparse, libgcs_hip.so),
the one function models/pt_v3.py uses.  Nothing else of torch_scatter is provided."""
from gaussiancity_amd.sparse import segment_csr  # noqa: F401
