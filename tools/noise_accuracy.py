#!/usr/bin/env python3
"""The accuracy of the counter-based disturbance generator on the MI355X: nocf_noise_fill_f32 on the grid
nt, n, d = 64, 1024, 64 at seed 12345 with scale 1 against the float64 restatement (tests/util_noise.py).  Writes the largest error
relative to max(|g|, 1e-3) and the (row, k, i) where it occurs; tests/test_noise_gpu.py's tolerance is four times that figure.

    python tools/noise_accuracy.py [--out profiles/noise]
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def main(argv=None):
    import numpy as np
    import torch
    import neuraloc_amd as na
    import util_noise as un
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "noise"))
    args = p.parse_args(argv)
    nt, n, d, seed = 64, 1024, 64, 12345
    # sigma = sqrt(nt) on tspan [0, 1]: scale = fp32(sqrt(nt) sqrt(1 / nt)) = 1, so the tensor is g itself
    W = na.counter_disturbances(nt, n, d, float(np.sqrt(nt)), seed, device="cuda:0")
    na.check_errors(sync=True)
    got = W.cpu().numpy().astype(np.float64)
    assert float(un.scale_of(np.sqrt(nt), d, nt)[0]) == 1.0
    g = un.gauss_grid(seed, nt, n, d)
    rel = np.abs(got - g) / np.maximum(np.abs(g), 1e-3)
    k, row, i = np.unravel_index(int(np.argmax(rel)), rel.shape)
    worst = float(rel[k, row, i])
    lines = ["nocf_noise_fill_f32 against the float64 restatement, grid nt x n x d = %d x %d x %d, seed %d, scale 1" % (nt, n, d, seed),
             "largest |got - g| / max(|g|, 1e-3) = %.6e = %.3f * 2^-23   (bound of the specification: 2^-20 = %.6e)" % (
                 worst, worst * 2.0 ** 23, 2.0 ** -20),
             "at row %d, k %d, i %d: got %.9e, g %.17e" % (row, k, i, got[k, row, i], g[k, row, i]),
             "mean relative error %.3e; entries above 2^-23: %d of %d" % (float(rel.mean()), int((rel > 2.0 ** -23).sum()), rel.size),
             "largest |g| on the grid %.6f" % float(np.abs(g).max())]
    text = "\n".join(lines)
    print(text)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "noise_accuracy.txt"), "w") as f:
        f.write(text + "\n")
    if not worst < 2.0 ** -20:
        raise SystemExit("the measured error is not below 2^-20: a fast intrinsic or a contraction got in")


if __name__ == "__main__":
    main()
