#!/usr/bin/env python3
"""Time the adversarial ensembles (neuraloc_amd/ensemble_minmax.py) on the MI355X.  Modelled on
tools/ensemble_risk_time.py (one child process per workload and E, the fixtures' ensembles, the sequential yardstick).

Workloads: softcorridor (family "lane") and singlequad (family "mid", the one-CU kernels), n = 1024 rows per member (shared starts), nt = 50,
E in {1, 4, 8}, member e at the budget eps_e = 0.05 e (member 0 undisturbed), K = 4 (step length 2.5 eps_e / 4), W [E, nt, n, d] of
0.02-sized normal draws for the legs that do not move it.
  (a) ms per free adversarial Adam iteration, training mode:
        ens_adv    zero_grad, ensemble_adversarial_step (forward, joint ensemble adjoint, ascent: three launches), one optimiser step
        seq_adv    E sequential adversarial_step iterations on the members (the parent's single-network code), E optimisers
      seq_adv / ens_adv is what one launch saves; at E = 1 it is the cost of the ensemble's host path against the single-network one.
  (b) the joint adjoint against the full one, each as recording forward + backward on the same W (the forward is the same launch in both):
        ens_joint  ensemble_minmax_ocflow_train (W requires a gradient) + backward      ens_full  ensemble_disturbed_ocflow_train + backward
        one_joint  minmax_ocflow_train + backward on member 0                           one_full  disturbed_ocflow_train + backward
  (c) the disturbed forward against the undisturbed one (evaluations):
        ens_dist   ensemble_disturbed_rollout      ens_plain  ensemble_rollout
        one_dist   disturbed_rollout on member 0   one_plain  OCflow on member 0
      The single-network pairs of (b) and (c) are measured in the same process: the ensemble ratios are to lie within their spread.
A repeat is --warmup calls and then --iters calls inside one HIP event pair; the legs alternate within a repeat and there are --repeats of
them; every ratio is formed per repeat, its spread the largest minus the smallest.  Each (workload, E) runs in a child process of its own.

    python tools/ensemble_minmax_time.py [--iters 10] [--warmup 3] [--repeats 5] [--out profiles/ensemble_minmax]
"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tools.ensemble_noise_time import load                            # noqa: E402  (the fixture's network and E - 1 perturbed copies)
from tools.minmax_time import _ratio, _timed                          # noqa: E402

# (fixture, family, nt, n)
SHAPES = [("softcorridor", "lane", 50, 1024), ("singlequad", "mid", 50, 1024)]
MEMBERS = [1, 4, 8]
ITER_LEGS = ("ens_adv", "seq_adv")
BWD_LEGS = ("ens_joint", "ens_full", "one_joint", "one_full")
FWD_LEGS = ("ens_dist", "ens_plain", "one_dist", "one_plain")
K = 4


def child(name, family, nt, n, E, iters, warmup, repeats):
    import torch
    import neuraloc_amd as na
    from neuraloc_amd import _lib
    dev = torch.device("cuda:0")
    nets, rows, prob, x, meta = load(name, n, E, dev)
    ens = na.PhiEnsemble.from_members(nets, alph=rows)
    ts, d, m = [0.0, 1.0], x.shape[1], meta["m"]
    eps = [0.05 * e for e in range(E)]
    step = [2.5 * v / K for v in eps]
    prob.train()
    L = _lib.lib()
    kern = lambda: L.nocf_last_rollout_kernel().decode()              # noqa: E731
    g = torch.Generator().manual_seed(5)
    W = (0.02 * torch.randn(E, nt, n, d, generator=g)).to(dev).contiguous()
    Wg = W.clone().requires_grad_(True)
    W0, W0g = W[0].contiguous(), W[0].clone().requires_grad_(True)
    kernels = {}

    # ---- (a) the free adversarial iteration
    opt = torch.optim.Adam(ens.parameters(), lr=1e-5)
    opts = [torch.optim.Adam(q.parameters(), lr=1e-5) for q in nets]
    Wa = torch.zeros(E, nt, n, d, device=dev, requires_grad=True)
    Ws = [torch.zeros(nt, n, d, device=dev, requires_grad=True) for _ in range(E)]

    def ens_adv():
        opt.zero_grad()
        na.ensemble_adversarial_step(x, ens, prob, ts, nt, Wa, eps, step, family=family)
        opt.step()

    def seq_adv():
        for e in range(E):
            opts[e].zero_grad()
            na.adversarial_step(x, nets[e], prob, ts, nt, Ws[e], eps[e], step[e], alph=rows[e])
            opts[e].step()
    ens_adv()
    seq_adv()
    ms_it = _timed({"ens_adv": ens_adv, "seq_adv": seq_adv}, ITER_LEGS, iters, warmup, repeats, na)

    # ---- (b) recording forward + joint / full adjoint
    def ens_joint():
        ens.zero_grad()
        Wg.grad = None
        na.ensemble_minmax_ocflow_train(x, ens, prob, ts, nt, Wg, family=family)[0].sum().backward()

    def ens_full():
        ens.zero_grad()
        na.ensemble_disturbed_ocflow_train(x, ens, prob, ts, nt, W, family=family)[0].sum().backward()

    def one_joint():
        nets[0].zero_grad()
        W0g.grad = None
        na.minmax_ocflow_train(x, nets[0], prob, ts, nt, W0g, "rk4", rows[0])[0].backward()

    def one_full():
        nets[0].zero_grad()
        na.disturbed_ocflow_train(x, nets[0], prob, ts, nt, W0, "rk4", rows[0])[0].backward()
    for leg, fn in (("ens_joint", ens_joint), ("ens_full", ens_full), ("one_joint", one_joint), ("one_full", one_full)):
        fn()
        kernels[leg] = kern()
    ms_bwd = _timed({"ens_joint": ens_joint, "ens_full": ens_full, "one_joint": one_joint, "one_full": one_full}, BWD_LEGS, iters, warmup,
                    repeats, na)

    # ---- (c) disturbed / undisturbed forward
    fwd = {"ens_dist": lambda: na.ensemble_disturbed_rollout(x, ens, prob, ts, nt, W, family=family),
           "ens_plain": lambda: na.ensemble_rollout(x, ens, prob, ts, nt, family=family),
           "one_dist": lambda: na.disturbed_rollout(x, nets[0], prob, nt, W0, tspan=ts, alph=rows[0]),
           "one_plain": lambda: na.OCflow(x, nets[0], prob, ts, nt, "rk4", rows[0])}
    with torch.no_grad():
        for leg in FWD_LEGS:
            fwd[leg]()
            kernels[leg] = kern()
        ms_fwd = _timed(fwd, FWD_LEGS, iters, warmup, repeats, na)
    res = {"name": name, "family": family, "nt": nt, "n": n, "E": E, "d": d, "m": m, "eps": eps, "K": K, "iters": iters, "warmup": warmup,
           "ms_per_iteration": ms_it, "ms_forward_backward": ms_bwd, "ms_forward": ms_fwd, "kernels": kernels}
    print("RESULT " + json.dumps(res), flush=True)


def run_child(args, name, family, nt, n, E):
    env = dict(os.environ, NOCF_JIT="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--iters", str(args.iters), "--warmup", str(args.warmup), "--repeats",
                        str(args.repeats), "--child", name, family, str(nt), str(n), str(E)], env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"{name} E={E} failed with exit status {r.returncode}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "ensemble_minmax"))
    p.add_argument("--child", nargs=5, default=None, help=argparse.SUPPRESS)
    args = p.parse_args(argv)
    if args.child:
        c = args.child
        return child(c[0], c[1], int(c[2]), int(c[3]), int(c[4]), args.iters, args.warmup, args.repeats)
    rows = []
    for name, family, nt, n in SHAPES:
        for E in MEMBERS:
            row = run_child(args, name, family, nt, n, E)
            for key, num, den, src in (("seq_over_ens", "seq_adv", "ens_adv", "ms_per_iteration"),
                                       ("ens_joint_over_full", "ens_joint", "ens_full", "ms_forward_backward"),
                                       ("one_joint_over_full", "one_joint", "one_full", "ms_forward_backward"),
                                       ("ens_dist_over_plain", "ens_dist", "ens_plain", "ms_forward"),
                                       ("one_dist_over_plain", "one_dist", "one_plain", "ms_forward")):
                row[key], row[key + "_spread"] = _ratio(row[src][num], row[src][den])
            # the ensemble ratio lies within the spread of the single-network ratio measured beside it
            for key in ("joint_over_full", "dist_over_plain"):
                slack = row["ens_" + key + "_spread"] + row["one_" + key + "_spread"]
                row[key + "_within_spread"] = bool(row["ens_" + key] <= row["one_" + key] + slack)
            rows.append(row)
            print("%s E=%d: sequential / ensemble %.2f +- %.2f, joint / full %.3f (one network %.3f), disturbed / plain %.3f (one network %.3f)" % (
                name, E, row["seq_over_ens"], row["seq_over_ens_spread"], row["ens_joint_over_full"], row["one_joint_over_full"],
                row["ens_dist_over_plain"], row["one_dist_over_plain"]), flush=True)

    def cell(v):
        return " ".join("%.3f" % t for t in v)
    lines = ["measured on the MI355X; n = %d rows per member, nt = %d; every figure is ms per call over %d calls after %d warm-ups, one per repeat; "
             "ratios per repeat: median +- spread (largest - smallest)" % (SHAPES[0][3], SHAPES[0][2], args.iters, args.warmup),
             "%-12s %-4s %2s  %-36s %-36s %-13s" % ("workload", "fam", "E", "ensemble adversarial step ms (repeats)", "E sequential adversarial steps ms",
                                                   "seq/ens")]
    for r in rows:
        it, fb, fw = r["ms_per_iteration"], r["ms_forward_backward"], r["ms_forward"]
        lines.append("%-12s %-4s %2d  %-36s %-36s %5.2f+-%.2f" % (r["name"], r["family"], r["E"], cell(it["ens_adv"]), cell(it["seq_adv"]),
                                                                   r["seq_over_ens"], r["seq_over_ens_spread"]))
        lines.append("    (b) forward + joint adjoint %s | forward + full adjoint %s | joint / full %.3f+-%.3f  [%s, %s]" % (
            cell(fb["ens_joint"]), cell(fb["ens_full"]), r["ens_joint_over_full"], r["ens_joint_over_full_spread"], r["kernels"]["ens_joint"],
            r["kernels"]["ens_full"]))
        lines.append("        one network: %s | %s | joint / full %.3f+-%.3f  [%s, %s]; ensemble ratio within the spreads of it: %s" % (
            cell(fb["one_joint"]), cell(fb["one_full"]), r["one_joint_over_full"], r["one_joint_over_full_spread"], r["kernels"]["one_joint"],
            r["kernels"]["one_full"], "yes" if r["joint_over_full_within_spread"] else "NO"))
        lines.append("    (c) disturbed forward %s | undisturbed %s | disturbed / undisturbed %.3f+-%.3f  [%s, %s]" % (
            cell(fw["ens_dist"]), cell(fw["ens_plain"]), r["ens_dist_over_plain"], r["ens_dist_over_plain_spread"], r["kernels"]["ens_dist"],
            r["kernels"]["ens_plain"]))
        lines.append("        one network: %s | %s | disturbed / undisturbed %.3f+-%.3f  [%s, %s]; ensemble ratio within the spreads of it: %s" % (
            cell(fw["one_dist"]), cell(fw["one_plain"]), r["one_dist_over_plain"], r["one_dist_over_plain_spread"], r["kernels"]["one_dist"],
            r["kernels"]["one_plain"], "yes" if r["dist_over_plain_within_spread"] else "NO"))
    text = "\n".join(lines)
    print(text)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "ensemble_minmax_time.txt"), "w") as f:
        f.write(text + "\n")
    with open(os.path.join(args.out, "ensemble_minmax_time.json"), "w") as f:
        json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
