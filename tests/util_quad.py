"""A CPU restatement of the quadcopter baseline's objective (baselineQuad.py:44-70, compute_loss), batched, in fp32 or fp64, with its
gradient by autograd.  The tests compare the kernels against it and against the fixture tests/golden/baseline_quad.npz."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "baseline_quad.npz")
XTARGET = [2., 2., 2., 0., 0., 0., 0., 0., 0., 0., 0., 0.]
XINIT = [-1.5, -1.5, -1.5, 0., 0., 0., 0., 0., 0., 0., 0., 0.]
ALPHG = 5000.
NT_LIST = (1, 7, 20, 50)


def load_golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def rollout(z0, U, mass=1.0, grav=9.81, dtype=torch.float64):
    """z0 [B, 12], U [B, nt, 4] -> (running cost L [B], trajectory [B, 12, nt+1]) in `dtype`, the reference's op order"""
    z0 = torch.as_tensor(z0).to(dtype)
    U = torch.as_tensor(U).to(dtype)
    nt = U.shape[1]
    h = 1.0 / nt
    x = z0
    L = torch.zeros(z0.shape[0], dtype=dtype)
    traj = [x]
    for i in range(nt):
        u = U[:, i, :]
        a = x[:, 3:6]
        sp, st, sf = torch.sin(a[:, 0]), torch.sin(a[:, 1]), torch.sin(a[:, 2])
        cp, ct, cf = torch.cos(a[:, 0]), torch.cos(a[:, 1]), torch.cos(a[:, 2])
        f7 = sp * sf + cp * st * cf
        f8 = -cp * sf + sp * st * cf
        f9 = ct * cf
        tmp = u[:, 0] / mass
        dx = torch.cat([x[:, 6:], (tmp * f7)[:, None], (tmp * f8)[:, None], (tmp * f9 - grav)[:, None], u[:, 1:4]], dim=1)
        x = x + h * dx
        L = L + h * (2 + torch.norm(u, p=2, dim=1) ** 2)
        traj.append(x)
    return L, torch.stack(traj, dim=2)


def objective(z0, U, alphG=ALPHG, mass=1.0, grav=9.81, xtarget=XTARGET, dtype=torch.float64, grad=False):
    """-> J [B] (and dJ/dU [B, nt, 4] with grad=True), CPU tensors of `dtype`"""
    U = torch.as_tensor(U).to(dtype).detach().clone().requires_grad_(grad)
    L, traj = rollout(z0, U, mass, grav, dtype)
    xt = torch.as_tensor(xtarget, dtype=dtype)
    G = alphG * 0.5 * torch.norm(traj[:, :, -1] - xt, p=2, dim=1) ** 2
    J = L + G
    if not grad:
        return J.detach()
    (g,) = torch.autograd.grad(J.sum(), U)
    return J.detach(), g


def report(z0, U, alphG=ALPHG, mass=1.0, grav=9.81, xtarget=XTARGET, dtype=torch.float64):
    """-> (rows [B, 3] = L+G, L, G;  trajectory [B, 12, nt+1])"""
    L, traj = rollout(z0, U, mass, grav, dtype)
    xt = torch.as_tensor(xtarget, dtype=dtype)
    G = alphG * 0.5 * torch.norm(traj[:, :, -1] - xt, p=2, dim=1) ** 2
    return torch.stack([L + G, L, G], dim=1), traj


def compare(got, want64, ref32, factor=4.0, floor=1e-6):
    """util_oracle's rule over the whole tensor: |got - fp64| <= factor x the fp32 restatement's own max error against fp64, at least
    floor x max|fp64| -> (ok, err, tol)"""
    want64 = torch.as_tensor(want64).double()
    e32 = float((torch.as_tensor(ref32).double() - want64).abs().max())
    tol = max(factor * e32, floor * float(want64.abs().max()))
    err = float((torch.as_tensor(got).detach().double().cpu() - want64).abs().max())
    return err <= tol, err, tol
