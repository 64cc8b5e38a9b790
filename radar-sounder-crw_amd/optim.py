"""The reference's optimizer -- ``torch.optim.Adam(model.parameters(), lr)`` with its defaults (scripts/train.py:54,69) -- as ONE
launch per step: the parameters become views of one flat fp32 buffer (like their gradients in ``dist.FlatGradBucket``) and
``crw_adam_step`` updates the whole buffer.  Same arithmetic as torch's default implementation, operation for operation
(``tests/test_hip_parity.py::test_flat_adam_matches_torch_adam``); ``state_dict`` keys / values of the module are unchanged (the
parameters keep their names and shapes, only their storage moves).

Opt-in, a GUARDED step (``max_grad_norm=`` / ``skip_nonfinite=``, include/crw_hip_guard.h): ``crw_adam_step_guarded`` takes the
gradient's norm in fp64 on the device, refuses the step when the gradient holds a NaN or an infinity, scales the gradient when the
norm exceeds the bound, and counts both in a 64-byte control block on the device -- no synchronisation, nothing read back."""
import torch

import crw_hip


class FlatAdam:
    """``FlatAdam(bucket, lr)``: bucket is the ``dist.FlatGradBucket`` that owns the flat gradient of the same parameters.

    max_grad_norm (None: no bound): the gradient is scaled by min(1, max_grad_norm / (norm + 1e-6)) before the update, the
    coefficient of ``torch.nn.utils.clip_grad_norm_`` on an fp64 norm.  skip_nonfinite: a step whose gradient holds a NaN or an
    infinity leaves the parameters and both moments as they are, and does not count towards the bias corrections.  With both off
    ``step()`` is ``crw_adam_step`` exactly as before.  With either set ``step()`` is the guarded entry point, which always does
    both: A CLIP THEREFORE IMPLIES THE SKIP (a norm that is not finite cannot scale anything)."""

    def __init__(self, bucket, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None, skip_nonfinite=False):
        self.bucket, self.lr, self.betas, self.eps = bucket, float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.max_grad_norm = None if max_grad_norm is None else crw_hip.check_max_norm(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.guarded = self.max_grad_norm is not None or self.skip_nonfinite
        params = bucket.params
        if not params or any(p.dtype != torch.float32 or not p.is_cuda for p in params):
            raise ValueError("FlatAdam needs fp32 parameters on the GPU (the HIP path); use torch.optim.Adam elsewhere")
        self.flat = torch.cat([p.data.reshape(-1) for p in params])
        o = 0
        for p in params:  # the module's parameters become views of the flat buffer (same order as the flat gradient)
            p.data = self.flat[o:o + p.numel()].view_as(p)
            o += p.numel()
        self.m, self.v, self.t = torch.zeros_like(self.flat), torch.zeros_like(self.flat), 0
        self.ctl = self.ws = None
        if self.guarded:  # both allocated once: the control block (zeroed once, the device owns it from here) and the workspace
            self.ctl = torch.zeros(crw_hip.GUARD_CTL_BYTES, dtype=torch.uint8, device=self.flat.device)
            self.ws = torch.empty(crw_hip.adam_guard_ws_bytes(self.flat.numel()), dtype=torch.uint8, device=self.flat.device)

    def _check_views(self):
        """the parameters must still be the views of ``self.flat`` made at construction: ``module.to()/.float()/.cuda()`` or
        ``load_state_dict(assign=True)`` re-bind ``p.data`` and the step would then update a dead buffer without an error"""
        params = self.bucket.params
        first, last = params[0], params[-1]
        end = self.flat.data_ptr() + 4 * (self.flat.numel() - last.numel())
        if first.data_ptr() != self.flat.data_ptr() or last.data_ptr() != end or sum(p.numel() for p in params) != self.flat.numel():
            raise RuntimeError("FlatAdam: the module's parameters no longer alias the optimizer's flat buffer (moved / re-assigned "
                               "after FlatAdam was built?) -- rebuild the FlatGradBucket and FlatAdam")

    def step(self):
        """after ``bucket.all_reduce_mean()``: the flat gradient is complete.  ``self.t`` counts the calls; a guarded optimizer
        keeps how many of them were applied on the device (``stats()``)."""
        self._check_views()
        self.t += 1
        if self.guarded:
            crw_hip.adam_step_guarded(self.flat, self.bucket.flat, self.m, self.v, self.t, self.lr, self.ctl, self.ws, self.betas[0],
                                      self.betas[1], self.eps, max_norm=self.max_grad_norm)
        else:
            crw_hip.adam_step(self.flat, self.bucket.flat, self.m, self.v, self.t, self.lr, self.betas[0], self.betas[1], self.eps)

    def stats(self):
        """{'applied', 'skipped', 'last_norm', 'last_scale', 'last_applied'} of a guarded optimizer: ONE 64-byte copy from the device
        (it waits for the steps issued so far), made only when asked."""
        if not self.guarded:
            raise RuntimeError("FlatAdam.stats(): this optimizer is not guarded (max_grad_norm / skip_nonfinite)")
        c = crw_hip.guard_ctl_unpack(self.ctl)
        return {"applied": c["applied"], "skipped": c["skipped"], "last_norm": c["norm"], "last_scale": c["scale"],
                "last_applied": c["last_applied"]}

    def state_dict(self):
        """moments, step count and hyper-parameters (checkpoint / resume, like ``torch.optim.Adam.state_dict``); a guarded optimizer
        adds its control block, so that a resumed one continues bit for bit"""
        sd = {"m": self.m.clone(), "v": self.v.clone(), "t": self.t, "lr": self.lr, "betas": self.betas, "eps": self.eps}
        if self.guarded:
            sd.update(ctl=self.ctl.clone(), max_grad_norm=self.max_grad_norm, skip_nonfinite=self.skip_nonfinite)
        return sd

    def load_state_dict(self, sd):
        if sd["m"].numel() != self.flat.numel():
            raise ValueError("FlatAdam.load_state_dict: moment buffers of another parameter set")
        self.m.copy_(sd["m"])
        self.v.copy_(sd["v"])
        self.t, self.lr, self.betas, self.eps = int(sd["t"]), float(sd["lr"]), tuple(sd["betas"]), float(sd["eps"])
        if self.guarded:
            if sd.get("ctl") is not None:
                self.ctl.copy_(sd["ctl"])
            else:  # the state of an unguarded optimizer: every one of its t steps was applied
                import struct
                raw = struct.pack(crw_hip.GUARD_CTL_FORMAT, self.t, 0, 0.0, 0.0, 1 if self.t else 0).ljust(crw_hip.GUARD_CTL_BYTES, b"\0")
                self.ctl.copy_(torch.tensor(list(raw), dtype=torch.uint8))
        elif sd.get("ctl") is not None and crw_hip.guard_ctl_unpack(sd["ctl"])["skipped"]:
            raise ValueError("FlatAdam.load_state_dict: the state holds skipped steps; build the optimizer with skip_nonfinite=True "
                             "(or max_grad_norm) to continue it")
