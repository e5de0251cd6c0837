#!/usr/bin/env python3
"""Time the weighted ensemble adjoints (nocf_rollout_bwd_small_ensemble_rw_f32 / nocf_rollout_bwd_mid_ensemble_rw_f32) and a risk-sensitive
ensemble Adam iteration (neuraloc_amd.ensemble_risk_ocflow_train) on the MI355X.  Modelled on tools/risk_time.py (the legs at the C entries,
one child process per workload) and tools/ensemble_noise_time.py (the fixtures' ensembles, the sequential yardstick).

Workloads: softcorridor (family "lane") and singlequad (family "mid", the one-CU kernels), n = 1024 rows per member (128 starts x 8 noise
paths, shared by the members), nt = 50, E in {1, 4, 8}, member e at sigma = 0.05 (e + 1), one seed for all members.
  (a) at the C entries, on ONE recorded noisy forward and the same preallocated outputs:
        weighted   the weighted ensemble adjoint under non-uniform weights (both signs, a zero, a range of 100, different per member)
        full       the unweighted ensemble adjoint (nocf_rollout_bwd_small_ensemble_f32 / nocf_rollout_bwd_mid_ensemble_f32)
        uniform    the weighted entry at w = 1 / n: the unweighted entry's arithmetic and bits from the weighted code
      The expectation is one more load per row, i.e. weighted / full = 1 within the repeats' spread.
  (b) ms per Adam iteration (zero_grad, call, backward, step), training mode, CVaR 0.8 over groups of 8 consecutive rows:
        ens_risk   ensemble_risk_ocflow_train, one optimiser over the ensemble
        seq_risk   E sequential risk_ocflow_train iterations on the members, E optimisers, in the same process
        ens_noisy  ensemble_noisy_ocflow_train at the same E on the same rows (the mean instead of the risk)
      seq_risk / ens_risk is what one launch saves (its yardstick: column (b) of profiles/ensemble_noise/ensemble_noise_time.txt for the same
      workload); ens_risk / ens_noisy is what the risk costs over the mean.
A repeat is --warmup calls and then --iters calls inside one HIP event pair; the legs alternate within a repeat and there are --repeats of
them; every ratio is formed per repeat, its spread the largest minus the smallest.  Each workload runs in a child process of its own.

    python tools/ensemble_risk_time.py [--iters 10] [--warmup 3] [--repeats 5] [--out profiles/ensemble_risk]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tools.ensemble_noise_time import SEED, load                      # noqa: E402  (the fixture's network and E - 1 perturbed copies)
from tools.minmax_time import _ratio, _timed                          # noqa: E402

# (fixture, family, nt, n)
SHAPES = [("softcorridor", "lane", 50, 1024), ("singlequad", "mid", 50, 1024)]
MEMBERS = [1, 4, 8]
ENTRY_LEGS = ("weighted", "full", "uniform")
ITER_LEGS = ("ens_risk", "seq_risk", "ens_noisy")
PATHS, LEVEL = 8, 0.8


def child(name, family, nt, n, E, iters, warmup, repeats):
    import torch
    import neuraloc_amd as na
    from neuraloc_amd import _lib, ensemble, ensemble_noise
    from neuraloc_amd.train import _STEPPERS, _step_sizes
    dev = torch.device("cuda:0")
    nets, rows, prob, x0, meta = load(name, n // PATHS, E, dev)
    x = x0.repeat_interleave(PATHS, 0).contiguous()                    # rows [i R, (i + 1) R): the R noise paths of start i
    ens = na.PhiEnsemble.from_members(nets, alph=rows)
    ts, d, m = [0.0, 1.0], x.shape[1], meta["m"]
    levels = [0.05 * (e + 1) for e in range(E)]
    sigma = [[s_] for s_ in levels]
    prob.train()
    L = _lib.lib()
    kern = lambda: L.nocf_last_rollout_kernel().decode()              # noqa: E731
    g = torch.Generator().manual_seed(5)
    wrow = (10.0 ** (2.0 * torch.rand(E, n, generator=g) - 2.0)) * torch.where(torch.rand(E, n, generator=g) < 0.3, -1.0, 1.0) / n
    wrow[:, n // 2] = 0.0
    wrow = wrow.to(dev).contiguous()
    uni = torch.full((E, n), 1.0 / n, device=dev)
    with torch.no_grad():
        nz = ensemble_noise._Noise(ensemble_noise.scale_table(sigma, E, nt, d, ts), ensemble_noise.seed_list(SEED, E), 0)
        launch = ensemble._launch_mid if family == "mid" else ensemble._launch
        b = launch(x, ens, prob, ts, nt, "rk4", None, record=True, noise=nz)           # the recorded inputs of all three legs
        torch.cuda.synchronize()
        kernels = {"forward": kern()}
        phi_st, keep1 = ens._c_struct()
        prob_st, keep2 = prob._c_struct(dev)
        hs = _step_sizes(ts, nt).to(dev)
        P = int(L.nocf_small_grad_floats(d, m))
        head = (C.byref(phi_st), C.byref(prob_st), n, E, nt, _STEPPERS["rk4"], 1.0, _lib.ptr(b["table"]))
        mid3 = (_lib.ptr(b["s_all"]), _lib.ptr(b["z_out"]), _lib.ptr(hs))
        f_w = ensemble.weighted_entry(L, family)
        if family == "lane":
            f_full = ensemble._shipped()[1][2]
            out, lam0 = torch.empty(E * n, P, device=dev), torch.empty(E * n, d, device=dev)
            tail = (_lib.ptr(out), _lib.ptr(lam0), _lib.stream_ptr(dev))
        else:
            f_full = ensemble._shipped_mid()[1][2]
            grows = int(L.nocf_mid_grad_rows(d, m, ens.nTh, ens.r, int(prob_st.n_agents), n))
            ws = ens.mid_workspace(L, dev)
            out, lam0 = torch.empty(E, grows, P, device=dev), torch.empty(E, n, d, device=dev)
            tail = (_lib.ptr(b["act"]), _lib.ptr(out), grows, _lib.ptr(lam0), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev))

        def full():
            _lib.check(f_full(*head, 1.0 / n, *mid3, *tail), "the unweighted ensemble adjoint")

        def weighted(w=wrow):
            _lib.check(f_w(*head, _lib.ptr(w), *mid3, *tail), "the weighted ensemble adjoint")
        full()
        torch.cuda.synchronize()
        kernels["full"] = kern()
        ref = (out.clone(), lam0.clone())
        weighted(uni)
        torch.cuda.synchronize()
        kernels["weighted"] = kern()
        same = bool(torch.equal(out, ref[0]) and torch.equal(lam0, ref[1]))
        ms = _timed({"weighted": weighted, "full": full, "uniform": lambda: weighted(uni)}, ENTRY_LEGS, iters, warmup, repeats, na)

    opt = torch.optim.Adam(ens.parameters(), lr=1e-5)
    opts = [torch.optim.Adam(q.parameters(), lr=1e-5) for q in nets]

    def ens_risk():
        opt.zero_grad()
        Jr, _, _ = na.ensemble_risk_ocflow_train(x, ens, prob, ts, nt, "cvar", LEVEL, paths=PATHS, sigma=sigma, seed=SEED, family=family)
        Jr.sum().backward()
        opt.step()

    def seq_risk():
        for e in range(E):
            opts[e].zero_grad()
            J1, _, _ = na.risk_ocflow_train(x, nets[e], prob, ts, nt, "cvar", LEVEL, paths=PATHS, sigma=levels[e], seed=SEED, stepper="rk4",
                                            alph=rows[e])
            J1.backward()
            opts[e].step()

    def ens_noisy():
        opt.zero_grad()
        Jc, _ = na.ensemble_noisy_ocflow_train(x, ens, prob, ts, nt, sigma, SEED, "rk4", family=family)
        Jc.sum().backward()
        opt.step()
    ens_risk()
    kernels["ens_risk"] = kern()
    seq_risk()
    kernels["seq_risk"] = kern()
    ms_it = _timed({"ens_risk": ens_risk, "seq_risk": seq_risk, "ens_noisy": ens_noisy}, ITER_LEGS, iters, warmup, repeats, na)
    res = {"name": name, "family": family, "nt": nt, "n": n, "E": E, "d": d, "m": m, "sigma": levels, "iters": iters, "warmup": warmup,
           "ms": ms, "ms_per_iteration": ms_it, "kernels": kernels, "uniform_weights_same_bits": same}
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
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "ensemble_risk"))
    p.add_argument("--child", nargs=5, default=None, help=argparse.SUPPRESS)
    args = p.parse_args(argv)
    if args.child:
        c = args.child
        return child(c[0], c[1], int(c[2]), int(c[3]), int(c[4]), args.iters, args.warmup, args.repeats)
    rows = []
    for name, family, nt, n in SHAPES:
        for E in MEMBERS:
            row = run_child(args, name, family, nt, n, E)
            for key, num, den, src in (("weighted_over_full", "weighted", "full", "ms"), ("uniform_over_full", "uniform", "full", "ms"),
                                       ("seq_over_ens", "seq_risk", "ens_risk", "ms_per_iteration"),
                                       ("risk_over_noisy", "ens_risk", "ens_noisy", "ms_per_iteration")):
                row[key], row[key + "_spread"] = _ratio(row[src][num], row[src][den])
            row["within_spread"] = bool(row["weighted_over_full"] <= 1.0 + row["weighted_over_full_spread"])
            rows.append(row)
            print("%s E=%d: weighted / full %.3f +- %.3f, sequential / ensemble %.2f +- %.2f" % (
                name, E, row["weighted_over_full"], row["weighted_over_full_spread"], row["seq_over_ens"], row["seq_over_ens_spread"]), flush=True)

    def cell(v):
        return " ".join("%.3f" % t for t in v)
    lines = ["measured on the MI355X; n = %d rows per member, nt = %d; every figure is ms per call over %d calls after %d warm-ups, one per repeat; "
             "ratios per repeat: median +- spread (largest - smallest)" % (SHAPES[0][3], SHAPES[0][2], args.iters, args.warmup),
             "%-12s %-4s %2s  %-36s %-36s %-13s" % ("workload", "fam", "E", "weighted ms (repeats)", "full ms (repeats)", "weighted/full")]
    for r in rows:
        lines.append("%-12s %-4s %2d  %-36s %-36s %5.3f+-%.3f" % (
            r["name"], r["family"], r["E"], cell(r["ms"]["weighted"]), cell(r["ms"]["full"]), r["weighted_over_full"], r["weighted_over_full_spread"]))
        lines.append("    forward %s; adjoints %s, %s; ratio above 1 by no more than the spread: %s; w = 1/n gives the unweighted entry's bits: %s" % (
            r["kernels"]["forward"], r["kernels"]["weighted"], r["kernels"]["full"], "yes" if r["within_spread"] else "NO",
            "yes" if r["uniform_weights_same_bits"] else "NO"))
        lines.append("    weighted entry at w = 1/n: %s ms | over full %.3f+-%.3f" % (cell(r["ms"]["uniform"]), r["uniform_over_full"], r["uniform_over_full_spread"]))
        it = r["ms_per_iteration"]
        lines.append("    ms per Adam iteration (CVaR %.1f, %d paths): ensemble risk %s | %d sequential risk %s | noisy ensemble %s" % (
            LEVEL, PATHS, cell(it["ens_risk"]), r["E"], cell(it["seq_risk"]), cell(it["ens_noisy"])))
        lines.append("    sequential / ensemble %.2f+-%.2f | ensemble risk / noisy ensemble %.3f+-%.3f | adjoints %s, %s" % (
            r["seq_over_ens"], r["seq_over_ens_spread"], r["risk_over_noisy"], r["risk_over_noisy_spread"], r["kernels"]["ens_risk"],
            r["kernels"]["seq_risk"]))
    text = "\n".join(lines)
    print(text)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "ensemble_risk_time.txt"), "w") as f:
        f.write(text + "\n")
    with open(os.path.join(args.out, "ensemble_risk_time.json"), "w") as f:
        json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
