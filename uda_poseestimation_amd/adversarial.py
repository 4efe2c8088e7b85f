"""Adversarial views: gradient-direction perturbations of an image batch inside an l2 / linf ball.

`perturb` is the functional form of csrc/perturb.hip (udapose_perturb): normalise a gradient per sample and apply it as a bounded step.
`adversarial_view` runs probe passes of a PoseResNet (PoseResNet.input_grad_only: forward, loss, backward to the input only - no trace on
the module) and perturbs the input against the loss: the one-step form (FGSM in linf, its l2 twin) or a few projected steps (PGD).  The
mean-teacher step uses it for the student's target view (MeanTeacherTrainer.adv_eps).  There is no CPU path.
"""
import torch

from . import _hip
from ._hip import check, lib, ptr

NORMS = {"l2": 0, "linf": 1}        # include/udapose.h: UDAPOSE_PERTURB_L2, UDAPOSE_PERTURB_LINF
MAX_STEPS = 4


def _dev_scalar(v, dev, what):
    """A float or a 0-d / one-element fp32 device tensor -> the device scalar the launches read.  (A float becomes a fill launch: fine in
    eager code and under capture, where it is baked into the graph; hand in a device tensor for a value that changes between replays.)"""
    if torch.is_tensor(v):
        if not v.is_cuda or v.dtype != torch.float32 or v.numel() != 1:
            raise ValueError(f"{what} as a tensor must be one float32 element on the device")
        return v
    v = float(v)
    if not v >= 0.0:
        raise ValueError(f"{what} must be >= 0, got {v}")
    return torch.full((), v, dtype=torch.float32, device=dev)


def _per_channel(v, C, dev, what):
    t = torch.as_tensor(v, dtype=torch.float32).detach().reshape(-1)
    if t.numel() != C:
        raise ValueError(f"{what} must have one value per channel ({C}), got {t.numel()}")
    return t.to(dev).contiguous()


def perturb(x, grad, eps, norm="l2", x0=None, step=None, clamp=None, out=None, want_norm=False):
    """x moved along `grad` inside the eps-ball around x0 (fp32 [N, C, ...] device tensors of one shape; x0 None: the ball is centred on x).
      norm "l2":   per sample, u = grad / ||grad||_2; d = (x - x0) + step * u; d is scaled back onto the ball where ||d||_2 > eps
      norm "linf": per element, d = clip((x - x0) + step * sign(grad), -eps, eps)
    and the result is clamp(x0 + d).  step None: step = eps (with x0 None the one-step form x + eps * u, which needs no second norm).
    eps / step: floats, or 0-d fp32 DEVICE tensors that the launches read (a captured call follows their values).  clamp = (lo[C], hi[C]),
    the form of MeanTeacherTrainer(recover=...).  A sample whose gradient is all zero or holds a non-finite element comes back as clamp(x)
    (udapose.h: per sample in l2 and whenever want_norm is set, per element in the one-launch linf form).  The gradient's scale does not
    matter: grad * 2^k gives the same bits (csrc/perturb.hip), so a loss scale needs no division.  out: may be x itself, never grad.
    want_norm: also return ||grad[n]||_2 as fp32 [N] (0 for a degenerate sample) -> (out, gnorm)."""
    _hip.require_cuda(x, grad, x0, out)
    if norm not in NORMS:
        raise ValueError(f"norm {norm!r}: one of {tuple(NORMS)}")
    if x.dim() < 2:
        raise ValueError("x must be [N, C, ...]")
    for t, what in ((x, "x"), (grad, "grad"), (x0, "x0"), (out, "out")):
        if t is not None and (t.dtype != torch.float32 or t.shape != x.shape or not t.is_contiguous()):
            raise ValueError(f"{what} must be a contiguous float32 tensor of x's shape {tuple(x.shape)}")
    N, C = x.shape[0], x.shape[1]
    HW = x[0, 0].numel()
    dev = x.device
    eps_t = _dev_scalar(eps, dev, "eps")
    step_t = None if step is None else _dev_scalar(step, dev, "step")
    lo = hi = None
    if clamp is not None:
        lo, hi = _per_channel(clamp[0], C, dev, "clamp[0]"), _per_channel(clamp[1], C, dev, "clamp[1]")
    if out is None:
        out = torch.empty_like(x)
    L = lib()
    nbytes = L.udapose_perturb_ws_bytes(N, C, HW)
    if nbytes < 0:
        check(int(nbytes), "perturb_ws_bytes")
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    gnorm = torch.empty(N, dtype=torch.float32, device=dev) if want_norm else None
    check(L.udapose_perturb(_hip.stream(), ptr(x), ptr(grad), ptr(x0), N, C, HW, NORMS[norm], ptr(eps_t), ptr(step_t), ptr(lo), ptr(hi),
                            ptr(ws), ptr(out), ptr(gnorm)), "perturb")
    return (out, gnorm) if want_norm else out


def default_step(eps, steps):
    """The step of `steps` projected iterations: eps for one (None: the kernel's one-step form), 2.5 * eps / steps otherwise (the usual
    PGD choice); for a device eps a device product, so a captured view follows eps."""
    if steps == 1:
        return None
    return eps * (2.5 / steps)


def adversarial_view(model, x, loss_fn, eps, norm="l2", steps=1, step=None, clamp=None, grad_scale=None):
    """The input x (fp32 [N, 3, H, W] on the device) moved, inside the eps-ball around it, in the direction that increases loss_fn(model(x)):
    -> (x_adv, gnorm [N], the norm of the last probe's input gradient per sample, 0 where the sample was left alone).
    `steps` (1 .. 4) probe passes of a PoseResNet: each is the training-mode forward of the current iterate, loss_fn(y), the backward to the
    input only (PoseResNet.input_grad_only) and one perturb() around x.  A probe leaves no trace on the model: no BatchNorm running update, no
    p.grad, no pending step state.  step: None = eps for one step, 2.5 * eps / steps otherwise.  clamp = (lo[C], hi[C]).
    grad_scale (the optimizer's current loss scale: a float or a 0-d device tensor; None = 1): multiplies the probe's loss so that an fp16
    gradient chain ('fp16' / 'strict') does not underflow; the normalisation removes it again, gnorm is divided by it, and a probe that
    overflows (inf / nan in the input gradient) perturbs nothing for that sample.  The scaler's state is never touched."""
    steps = int(steps)
    if not 1 <= steps <= MAX_STEPS:
        raise ValueError(f"steps must be in 1 .. {MAX_STEPS}, got {steps}")
    if norm not in NORMS:
        raise ValueError(f"norm {norm!r}: one of {tuple(NORMS)}")
    x = x.detach()
    if x.dtype != torch.float32 or not x.is_contiguous():
        x = x.float().contiguous()
    eps_t = _dev_scalar(eps, x.device, "eps")
    step_t = default_step(eps_t, steps) if step is None else _dev_scalar(step, x.device, "step")
    probe_loss = loss_fn if grad_scale is None else (lambda y: loss_fn(y) * grad_scale)
    xk, gnorm = x, None
    for _ in range(steps):
        g, _ = model.input_grad_only(xk, probe_loss)
        with torch.no_grad():
            xk, gnorm = perturb(xk, g, eps_t, norm, x0=None if steps == 1 else x, step=step_t, clamp=clamp, want_norm=True)
    if grad_scale is not None:
        with torch.no_grad():
            gnorm = gnorm / grad_scale
    return xk, gnorm
