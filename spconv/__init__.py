"""Drop-in for spconv 2.x on the MI355X: `import spconv.pytorch as spconv` gives the submanifold convolution that
models/pt_v3.py uses, backed by libgcs_hip.so (gaussiancity_amd.sparse).  Nothing else of spconv is provided."""
