"""The one loader behind the six ctypes bindings (_native*.py): each binding declares its library -- symbol prefix,
file name, ABI number, one signature table -- and gets lib(), check() and, where the library has them, set_option() and
stage_ms() from here.

The libraries are the product: there is NO Python/CPU fallback.  A missing library or a failing call raises
RuntimeError.  No torch import at module level: the bindings load without it.
"""
import ctypes as C
import os

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")


class Library:
    """`signatures`: name -> (restype, argtypes) for every function the library's header declares.  It is the only list:
    `exported_symbols` is its keys, and every one of them gets its prototype bound when the library is loaded.
    `path_env`: environment variable that overrides the path, read here (that is, when the binding is imported).
    `after_load`: called once with the CDLL, before the ABI check."""

    def __init__(self, prefix, file_name, abi_version, signatures, stage_names=(), path_env=None, after_load=None):
        self.prefix, self.file_name, self.abi_version, self.stage_names = prefix, file_name, abi_version, tuple(stage_names)
        self.signatures, self.after_load = signatures, after_load
        self.exported_symbols = tuple(signatures)
        self.path = (os.environ.get(path_env) if path_env else None) or os.path.join(CSRC, file_name)
        loaded = None

        def lib():  # per frame in ext.py: one cell read and one comparison once loaded
            nonlocal loaded
            if loaded is not None:
                return loaded
            loaded = self._load()
            return loaded
        self.lib = lib

    def _load(self):
        if not os.path.exists(self.path):
            raise RuntimeError("%s is not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "or `make -C gaussiancity_amd/csrc`. There is no CPU fallback." % (self.file_name, self.path))
        L = C.CDLL(self.path)
        for name, (restype, argtypes) in self.signatures.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, list(argtypes)
        if self.after_load is not None:
            self.after_load(L)
        if self._fn(L, "abi_version")() != self.abi_version:
            raise RuntimeError("%s ABI version mismatch" % self.file_name)
        return L

    def _fn(self, L, name):
        return getattr(L, "%s_%s" % (self.prefix, name))

    def check(self, rc, what):
        if rc < 0:
            msg = self._fn(self.lib(), "last_error")().decode("utf-8", "replace")
            raise RuntimeError("%s failed (%s_status %d): %s" % (what, self.prefix, rc, msg))
        return rc

    def set_option(self, name, value):
        return self._fn(self.lib(), "set_option")(name.encode(), int(value))

    def stage_ms(self):
        buf = (C.c_float * len(self.stage_names))()
        n = self._fn(self.lib(), "get_stage_ms")(buf, len(self.stage_names))
        return {self.stage_names[i]: float(buf[i]) for i in range(n)}


def fresh(t):
    """A new tensor of t's values with dense strides, at the allocator's alignment."""
    import torch
    out = torch.empty(t.shape, dtype=t.dtype, device=t.device)
    return out.copy_(t) if out.numel() else out


def dense(t, align=16):
    """t as a library takes a dense operand: t itself when it is contiguous and its first byte `align`-byte aligned, else a
    fresh copy.  Tensor.contiguous() does not serve: a contiguous view at a storage offset (a parameter inside a flat
    buffer, `buf[1:].view(N, C)`) is returned as it is, misaligned pointer included."""
    return t if t.is_contiguous() and t.data_ptr() % align == 0 else fresh(t)


def current_stream():
    """The current torch stream as the `void* hip_stream` argument of the libraries' entry points."""
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
