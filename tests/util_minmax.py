"""oracle-side helpers of min-max training's tests (CPU only: nothing here touches a GPU)

neuraloc_amd.minmax_ocflow_train returns three kinds of gradient from one adjoint launch; their yardsticks exist already and are used
unchanged: util_disturb_train.case_grads (fp64 autograd of the restated oracle) for the parameters and x, util_adversary.case_grads(...,
"Jc") for W.  references() puts both into one {name: gradient} dict, compare() applies util_oracle.compare's rule (four times the fp32
restatement's own error, floor 1e-6 of the scale) to every entry.  Cases, screened starts and disturbances are util_disturb's."""
import torch

import util_adversary as ua
import util_disturb_train as ut
import util_oracle as uo

JOINT_KERNEL = {"lane": "rollout_lane_bwd_kernel<joint>", "mono": "rollout_mono_bwd_kernel<joint>", "tile": "rollout_bwd_kernel<joint>",
                "tile-fixed": "rollout_bwd_kernel<joint>"}
FULL_KERNEL = {"lane": "rollout_lane_bwd_kernel", "mono": "rollout_mono_bwd_kernel", "tile": "rollout_bwd_kernel",
               "tile-fixed": "rollout_bwd_kernel"}


def references(case, dtype, n_total=None, rows=None, mutation=None):
    """{parameter name: dJc/dtheta, "x": dJc/dx, "W": dJc/dW} of the restated oracle in `dtype` on the case's screened starts and
    disturbances (rows: a slice of them; n_total: the batch the mean runs over).  The two helpers' results are cached there."""
    out = ut.with_x(ut.case_grads(case, dtype, n_total=n_total, rows=rows, mutation=mutation))
    a = ua.case_grads(case, dtype, "Jc", n_total=n_total, rows=rows, mutation=mutation)
    assert torch.equal(a["dx"], out["x"])                           # (the two references are one)
    out["W"] = a["dW"]
    return out


def compare(got, w64, w32):
    """{name: (ok, err, tol, err32)} over every entry of the fp64 reference; a parameter Jc does not reach has no autograd gradient: zero"""
    res = {}
    for k in w64:
        r64 = torch.zeros_like(got[k], dtype=torch.float64) if w64[k] is None else w64[k]
        r32 = torch.zeros_like(got[k], dtype=torch.float32) if w32[k] is None else w32[k]
        res[k] = uo.compare(got[k], r64, r32)
    return res


def shifted(g):
    """dJ/dW one step late: what a lamW store in front of the wrong stage would give"""
    return torch.roll(g, 1, 0)


def failures(res):
    return {k: v for k, v in res.items() if not v[0]}


def row_objective(tab, alph):
    """[n] per-row training objective L + a0 G + a3 HJt + a4 HJfin + a5 HJgrad from a persample table"""
    a = [float(v) for v in alph[:6]]
    return tab[:, 0] + a[0] * tab[:, 1] + a[3] * tab[:, 2] + a[4] * tab[:, 3] + a[5] * tab[:, 4]
