"""Drop-in for flash_attn on the MI355X: flash_attn_varlen_qkvpacked_func, the one function models/pt_v3.py uses,
backed by libgca_hip.so (gaussiancity_amd.attention).  Nothing else of flash_attn is provided."""
from .flash_attn_interface import flash_attn_varlen_qkvpacked_func  # noqa: F401

__version__ = "2.6.3+gca1"
