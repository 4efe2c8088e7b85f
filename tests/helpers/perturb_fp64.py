"""Float64 restatement of csrc/perturb.hip (udapose_perturb): the gradient-direction perturbation inside an l2 / linf ball.  Plain torch on
whatever device the operands live on; the operands are taken as given (fp32 values widened), every operation is float64."""
import torch


def _clamp(v, clamp):
    if clamp is None:
        return v
    C = v.shape[1]
    shape = (1, C) + (1,) * (v.dim() - 2)
    lo = torch.as_tensor(clamp[0], dtype=torch.float64, device=v.device).reshape(shape)
    hi = torch.as_tensor(clamp[1], dtype=torch.float64, device=v.device).reshape(shape)
    return torch.minimum(torch.maximum(v, lo), hi)


def degenerate(g):
    """[N] bool: the sample's gradient holds a non-finite element or is all zero."""
    flat = g.reshape(g.shape[0], -1).double()
    return ~torch.isfinite(flat).all(dim=1) | ((flat * flat).sum(dim=1) == 0)


def perturb(x, g, eps, norm="l2", x0=None, step=None, clamp=None, per_sample_rule=True):
    """-> (out, gnorm) in float64.  x, g, x0: [N, C, ...]; eps, step: floats (step None: eps); clamp = (lo[C], hi[C]).
    per_sample_rule False: the one-launch linf form, which treats a non-finite g element by element (sign(nan) = 0)."""
    x64, g64 = x.double(), g.double()
    z64 = x64 if x0 is None else x0.double()
    eps, step = float(eps), float(eps if step is None else step)
    N = x.shape[0]
    bshape = (N,) + (1,) * (x.dim() - 1)
    bad = degenerate(g)
    gs = torch.where(bad.reshape(bshape), torch.zeros_like(g64), g64)
    gn = gs.reshape(N, -1).norm(dim=1)
    if norm == "l2":
        u = gs / torch.where(bad, torch.ones_like(gn), gn).reshape(bshape)
        d = (x64 - z64) + step * u
        dn = d.reshape(N, -1).norm(dim=1)
        f = torch.where(dn > eps, eps / torch.where(dn > 0, dn, torch.ones_like(dn)), torch.ones_like(dn))
        out = z64 + d * f.reshape(bshape)
    elif norm == "linf":
        sg = torch.sign(torch.nan_to_num(g64, nan=0.0)) if not per_sample_rule else torch.sign(gs)
        out = z64 + ((x64 - z64) + step * sg).clamp(-eps, eps)
    else:
        raise ValueError(norm)
    if per_sample_rule:
        out = torch.where(bad.reshape(bshape), x64, out)
    return _clamp(out, clamp), gn
