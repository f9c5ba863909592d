"""The stage-seam operator through the C ABI, as tests/test_seam_gpu.py and tests/test_seam_plans_gpu.py call it: one problem
on the device and the library's three calls on it, with chosen fills of the outputs and the workspace and chosen output
subsets, and the comparison of two such calls bit for bit."""
import torch

import seam_ref as R


def _ptr(t):
    return None if t is None else t.data_ptr()


class Direct:
    """One problem on the device and the library's three calls on it, with chosen fills and output subsets."""
    def __init__(self, dev, N, I, O, seed, product=True, act=True, pad=0):
        from gaussiancity_amd import _native_m as M
        self.M, self.L = M, M.lib()
        inp = R.make_inputs(N, I, O, seed, product)
        self.N, self.I, self.O, self.act, self.product, self.pad = N, inp["x"].shape[1], O, act, product, pad
        self.t = {k: None if v is None else v.to(dev).contiguous() for k, v in inp.items()}
        self.dev = dev

    def rows(self, value, fill):
        """value as a view of rows `pad` elements further apart, the padding filled."""
        wide = torch.full((value.shape[0], value.shape[1] + self.pad), fill, device=self.dev)
        wide[:, :value.shape[1]] = value
        return wide, wide[:, :value.shape[1]]

    def forward(self, training, fill):
        t, N, I, O = self.t, self.N, self.I, self.O
        full = lambda *s: torch.full(s, fill, device=self.dev)  # noqa: E731
        out = {"y_wide": full(N, O + self.pad), "z": full(N, O) if self.product else None, "mean": full(O), "rstd": full(O)}
        out["y"] = out["y_wide"][:, :O]
        x = self.rows(t["x"], 5.0)[1]
        buf = {k: t[k].clone() for k in ("running_mean", "running_var", "tracked")}
        if training:
            nbytes = self.L.gcm_seam_forward_workspace_bytes(N, O)
            ws = torch.full((nbytes // 4,), fill, device=self.dev)
            rc = self.L.gcm_seam_forward_train(x.data_ptr(), x.stride(0), _ptr(t["w"]), _ptr(t["b"]), R.EPS, R.MOMENTUM,
                                               t["g"].data_ptr(), t["h"].data_ptr(), int(self.act), N, I, O, _ptr(out["z"]),
                                               out["y"].data_ptr(), out["y"].stride(0), out["mean"].data_ptr(),
                                               out["rstd"].data_ptr(), buf["running_mean"].data_ptr(),
                                               buf["running_var"].data_ptr(), buf["tracked"].data_ptr(), ws.data_ptr(), nbytes,
                                               None)
        else:
            out["mean"] = buf["running_mean"]
            rc = self.L.gcm_seam_forward_eval(x.data_ptr(), x.stride(0), _ptr(t["w"]), _ptr(t["b"]),
                                              buf["running_mean"].data_ptr(), buf["running_var"].data_ptr(), R.EPS,
                                              t["g"].data_ptr(), t["h"].data_ptr(), int(self.act), N, I, O, out["y"].data_ptr(),
                                              out["y"].stride(0), _ptr(out["z"]), out["rstd"].data_ptr(), None)
        self.M.check(rc, "forward")
        out.update(buf)
        out["x"] = x
        return out

    def backward(self, fwd, training, fill, want=R.GRADS):
        t, N, I, O = self.t, self.N, self.I, self.O
        full = lambda *s: torch.full(s, fill, device=self.dev)  # noqa: E731
        names = [k for k in want if self.product or k not in ("dw", "db")]
        out = {"dx_wide": full(N, I + self.pad) if "dx" in names else None, "dw": full(O, I) if "dw" in names else None,
               "db": full(O) if "db" in names else None, "dg": full(O) if "dg" in names else None,
               "dh": full(O) if "dh" in names else None}
        out["dx"] = None if out["dx_wide"] is None else out["dx_wide"][:, :I]
        dy = self.rows(t["dy"], 7.0)[1]
        x = fwd["x"]
        z = fwd["z"] if self.product else x
        nbytes = self.L.gcm_seam_backward_workspace_bytes(N, I, O)
        ws = torch.full((nbytes // 4,), fill, device=self.dev)
        dx = out["dx"]
        self.M.check(self.L.gcm_seam_backward(x.data_ptr(), x.stride(0), z.data_ptr(), z.stride(0), fwd["mean"].data_ptr(),
                                              fwd["rstd"].data_ptr(), dy.data_ptr(), dy.stride(0), _ptr(t["w"]),
                                              t["g"].data_ptr(), t["h"].data_ptr(), int(self.act), int(training), N, I, O,
                                              _ptr(dx), 0 if dx is None else dx.stride(0), _ptr(out["dw"]), _ptr(out["db"]),
                                              _ptr(out["dg"]), _ptr(out["dh"]), ws.data_ptr(), nbytes, None), "backward")
        return out


def differing(a, b, names):
    """The names whose tensors differ in presence or in any bit."""
    return [k for k in names if (a.get(k) is None) != (b.get(k) is None)
            or (a.get(k) is not None and not torch.equal(R.bits(a[k]) if a[k].dtype == torch.float32 else a[k],
                                                         R.bits(b[k]) if b[k].dtype == torch.float32 else b[k]))]


FORWARD = ("y", "y_wide", "z", "mean", "rstd", "running_mean", "running_var", "tracked")
BACKWARD = ("dx", "dx_wide", "dw", "db", "dg", "dh")
