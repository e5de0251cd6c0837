#!/usr/bin/env python3
"""Time ensembles on the one-CU kernels (neuraloc_amd.ensemble with family="mid": E networks, one launch per rollout / adjoint, member e on
its own workgroups) on the MI355X against what a user does without them: E single-network calls one after the other in the same process, on
the unchanged single-network code paths.  tools/ensemble_time.py is the same measurement for the lane family.

Workloads: singlequad at its BASELINE shape (m = 128, nt = 50) and swap12 with a 128-wide network (nt = 20), n = 1024 starts shared by the
members (64 tiles per member on 256 CUs), E in {1, 2, 4, 8, 16}.
  eval   one ensemble_rollout                                        against  E sequential OCflow calls
  adam   one Adam iteration over the ensemble (zero_grad, ensemble_ocflow_train, backward, step)
                                                                     against  E sequential single-network iterations with E optimisers
Both legs are the public calls, allocations included; networks, problems, starts and optimisers are made outside the HIP event pair.  The
two legs alternate within each repetition; median of --reps after --warmup, with the smallest and the largest repetition.  The ratio
sequential / ensemble is formed per repetition; its spread (largest minus smallest) is what a difference is judged against.

    python tools/ensemble_mid_time.py [--reps 5] [--warmup 2] [--out profiles/ensemble_mid]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# (fixture, width: None = the fixture's own network, nt, n)
SHAPES = [("singlequad", None, 50, 1024), ("swap12", 128, 20, 1024)]
MEMBERS = [1, 2, 4, 8, 16]


def load(name, width, n, E, dev):
    """E networks (the fixture's and perturbed copies of it; with `width`: fresh networks of that width), the fixture's problem, n starts"""
    import numpy as np
    import torch
    import neuraloc_amd as na
    z = np.load(os.path.join(REPO, "tests", "golden", name + ".npz"))
    meta = json.loads(str(z["meta"]))
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}
    g = torch.Generator().manual_seed(1)
    m = meta["m"] if width is None else width
    nets = []
    for e in range(E):
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(100 + e)
            net = na.Phi(nTh=meta["nTh"], m=m, d=meta["d"], alph=meta["alph"])
        if width is None:
            net.load_state_dict({k: v + (0.01 * e) * torch.randn(v.shape, generator=g) for k, v in sd.items()})
        nets.append(net.to(dev))
    rows = [[float(meta["alph"][0]), float(meta["alph_Q"]), float(meta["alph_W"])] + [float(v) for v in meta["alph"][3:6]]] * E
    cls = na.Quadcopter if meta["prob_class"] == "Quadcopter" else na.Cross2D
    prob = cls(torch.from_numpy(z["xtarget"]).to(dev), obstacle=meta["obstacle"], alph_Q=meta["alph_Q"], alph_W=meta["alph_W"], r=meta["r"])
    xb = torch.from_numpy(z["x"])
    x = xb[torch.arange(n) % xb.shape[0]] + 0.01 * torch.randn(n, xb.shape[1], generator=g)
    return nets, rows, prob, x.to(dev).contiguous(), dict(meta, m=m)


def timed(fns, reps, warmup):
    """all ms per function; the functions alternate within every repetition, so drift of the machine hits all of them alike"""
    import torch
    ms = [[] for _ in fns]
    for r in range(warmup + reps):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= warmup:
                ms[i].append(e0.elapsed_time(e1))
    return ms


def measure(name, width, nt, n, E, reps, warmup):
    import torch
    import neuraloc_amd as na
    from neuraloc_amd import _lib
    dev = torch.device("cuda:0")
    nets, rows, prob, x, meta = load(name, width, n, E, dev)
    ens = na.PhiEnsemble.from_members(nets, alph=rows)
    ts = [0.0, 1.0]
    out = {"name": name, "nt": nt, "n": n, "E": E, "m": meta["m"], "d": meta["d"]}
    kern = lambda: _lib.lib().nocf_last_rollout_kernel().decode()      # noqa: E731

    prob.eval()

    def ens_eval():
        with torch.no_grad():
            na.ensemble_rollout(x, ens, prob, ts, nt, "rk4", family="mid")

    def seq_eval():
        with torch.no_grad():
            for e in range(E):
                na.OCflow(x, nets[e], prob, ts, nt, "rk4", rows[e])

    ens_eval()
    out["ens_kernel"] = kern()
    seq_eval()
    out["seq_kernel"] = kern()
    with torch.no_grad():
        Jc, _ = na.ensemble_rollout(x, ens, prob, ts, nt, "rk4", family="mid")
        if not all(torch.equal(Jc[e], na.OCflow(x, nets[e], prob, ts, nt, "rk4", rows[e])[0]) for e in range(E)):
            raise SystemExit("the ensemble and the sequential calls disagree")
    out["eval_ens"], out["eval_seq"] = timed([ens_eval, seq_eval], reps, warmup)

    prob.train()
    opt = torch.optim.Adam(ens.parameters(), lr=1e-4)
    opts = [torch.optim.Adam(q.parameters(), lr=1e-4) for q in nets]

    def ens_adam():
        opt.zero_grad()
        Jc, _ = na.ensemble_ocflow_train(x, ens, prob, ts, nt, "rk4", family="mid")
        Jc.sum().backward()
        opt.step()

    def seq_adam():
        for e in range(E):
            opts[e].zero_grad()
            J1, _ = na.OCflow(x, nets[e], prob, ts, nt, "rk4", rows[e])
            J1.backward()
            opts[e].step()

    ens_adam()
    out["ens_bwd_kernel"] = kern()
    seq_adam()
    out["seq_bwd_kernel"] = kern()
    out["adam_ens"], out["adam_seq"] = timed([ens_adam, seq_adam], reps, warmup)
    na.check_errors(sync=True)
    return out


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "ensemble_mid"))
    args = p.parse_args(argv)
    os.environ.setdefault("NOCF_JIT", "0")
    rows = [measure(name, width, nt, n, E, args.reps, args.warmup) for name, width, nt, n in SHAPES for E in MEMBERS]
    lines = ["measured on the MI355X; ms = median [smallest, largest] of %d repetitions after %d warm-ups; ratio = sequential / ensemble per "
             "repetition: median [smallest, largest], spread = largest - smallest" % (args.reps, args.warmup),
             "%-11s %4s %5s %3s %3s %-5s %24s %24s %22s %7s" % ("shape", "m", "n", "nt", "E", "what", "ensemble ms", "E sequential ms", "ratio",
                                                              "spread")]

    def cell(v):
        return "%8.3f [%.3f,%.3f]" % (statistics.median(v), min(v), max(v))
    for r in rows:
        for what in ("eval", "adam"):
            en, sq = r[what + "_ens"], r[what + "_seq"]
            ratio = [s_ / e_ for s_, e_ in zip(sq, en)]
            r[what + "_ratio"], r[what + "_spread"] = statistics.median(ratio), max(ratio) - min(ratio)
            lines.append("%-11s %4d %5d %3d %3d %-5s %24s %24s %22s %7.3f" % (r["name"], r["m"], r["n"], r["nt"], r["E"], what, cell(en), cell(sq),
                                                                             "%6.2f [%.2f,%.2f]" % (r[what + "_ratio"], min(ratio), max(ratio)),
                                                                             r[what + "_spread"]))
    lines.append("")
    for name, _w, _nt, _n in SHAPES:
        r0 = next(r for r in rows if r["name"] == name)
        lines.append("kernels %-11s: ensemble %s / %s, sequential %s / %s" % (name, r0["ens_kernel"], r0["ens_bwd_kernel"], r0["seq_kernel"],
                                                                             r0["seq_bwd_kernel"]))
    # conditions, each against the sequential leg of the same run: at E = 1 the ensemble call is not slower than the plain call by more than the
    # spread; at E = 4 the rollout and the Adam iteration are faster than four sequential ones by more than the spread
    for r in rows:
        if r["E"] == 1:
            ok = r["eval_ratio"] >= 1.0 - r["eval_spread"]
            lines.append("condition %-11s E=1 eval: ratio %.3f, spread %.3f (not slower) -> %s" % (r["name"], r["eval_ratio"], r["eval_spread"],
                                                                                                 "met" if ok else "NOT met"))
        if r["E"] == 4:
            for what in ("eval", "adam"):
                ok = r[what + "_ratio"] > 1.0 + r[what + "_spread"]
                lines.append("condition %-11s E=4 %-4s: ratio %.3f, spread %.3f (faster) -> %s" % (r["name"], what, r[what + "_ratio"],
                                                                                                 r[what + "_spread"], "met" if ok else "NOT met"))
    for name, _w, _nt, _n in SHAPES:
        mine = [r for r in rows if r["name"] == name]
        for what in ("eval", "adam"):
            base = statistics.median(mine[0][what + "_ens"])
            twice = next((r["E"] for r in mine if statistics.median(r[what + "_ens"]) >= 2.0 * base), None)
            lines.append("%-11s %-4s: one ensemble call costs twice its E = 1 time (%.3f ms) from E = %s" % (
                name, what, base, twice if twice is not None else "> %d" % MEMBERS[-1]))
    text = "\n".join(lines)
    print(text)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "ensemble_mid_time.txt"), "w") as f:
        f.write(text + "\n")
    with open(os.path.join(args.out, "ensemble_mid_time.json"), "w") as f:
        json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
