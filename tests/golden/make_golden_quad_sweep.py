"""Writes tests/golden/quad_sweep.npz: near-optimal controls from xInit at the two horizons where the sweep compares exit reasons
(util_quad_sweep.REASON_HORIZONS), as float32.  The exit "loss change < tolerance_change" is met only near the optimum, 150 iterations
from the reference's guess; started from these controls it ends the first iteration.  They are the result of torch.optim.LBFGS at the
reference's settings on the fp64 restatement (util_quad_sweep.objective64), on the CPU: a start, not something a test compares with.

    python tests/golden/make_golden_quad_sweep.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import util_quad_sweep as qs  # noqa: E402


def main():
    out = {}
    for nt in qs.REASON_HORIZONS:
        z0, U0 = qs.start(nt, torch.float64)
        sol = qs.torch_lbfgs(qs.objective64(z0), U0, **qs.REF_SETTINGS)
        print(f"nt = {nt}: {sol.n_iter} iterations, {sol.n_evals} evaluations, exit {sol.reason}")
        out[f"warm/nt{nt}"] = sol.U.float().numpy()
    np.savez(os.path.join(HERE, "quad_sweep.npz"), **out)


if __name__ == "__main__":
    main()
