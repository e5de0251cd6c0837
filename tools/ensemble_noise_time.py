#!/usr/bin/env python3
"""Time ensembles under in-kernel Brownian noise (neuraloc_amd.ensemble_noise: E networks, every member at its own noise level, one launch
per rollout / adjoint) on the MI355X.  Modelled on tools/ensemble_time.py / tools/ensemble_mid_time.py (the legs, the alternation) and on
tools/noise_time.py (the noisy / undisturbed yardstick).

Workloads: softcorridor (family "lane", the fixture's network, nt = 50) and singlequad (family "mid", m = 128, nt = 50), n = 1024 starts
shared by the members, E in {1, 4, 8}, member e at sigma = 0.05 (e + 1), one seed for all members.
  eval   one rollout;   adam   one Adam iteration (zero_grad, forward, backward, step)
Five legs alternate within each repetition, all public calls, allocations included:
  ens_noisy   ensemble_noisy_rollout / ensemble_noisy_ocflow_train
  ens_plain   ensemble_rollout / ensemble_ocflow_train                      (the same E, undisturbed)
  seq_noisy   E sequential noisy_rollout / noisy_ocflow_train calls, E optimisers
  one_noisy   noisy_rollout / noisy_ocflow_train on member 0                (the single-network yardstick ...)
  one_plain   OCflow on member 0                                            (... against its undisturbed call)
Ratios, each formed per repetition (median [smallest, largest], spread = largest - smallest: what a difference is judged against):
  (a)  ens_noisy / ens_plain    what the noise costs an ensemble; its yardstick is one_noisy / one_plain of the same run
  (b)  seq_noisy / ens_noisy    what one launch saves over E sequential noisy calls (the figure of profiles/ensemble*/, under noise)

The call times hold the host's work in front of the launch (the scale table and seeds are formed and copied in every call).  To split it
from the kernels, the same run also reads the library's own event pairs around the rollout kernel (nocf_profile_begin / nocf_profile_end,
bench.py's hook) for the four evaluation legs at E = 1 and E = 8: ensemble_noise_kernels.txt, ms per launch, median [smallest, largest]
of 5 batches of 10 launches.

    python tools/ensemble_noise_time.py [--reps 5] [--warmup 2] [--out profiles/ensemble_noise]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# (fixture, family, nt, n)
SHAPES = [("softcorridor", "lane", 50, 1024), ("singlequad", "mid", 50, 1024)]
MEMBERS = [1, 4, 8]
SEED = 20240607
LEGS = ("ens_noisy", "ens_plain", "seq_noisy", "one_noisy", "one_plain")


def load(name, n, E, dev):
    """the fixture's network and E - 1 perturbed copies of it, the fixture's problem, n starts"""
    import numpy as np
    import torch
    import neuraloc_amd as na
    z = np.load(os.path.join(REPO, "tests", "golden", name + ".npz"))
    meta = json.loads(str(z["meta"]))
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}
    g = torch.Generator().manual_seed(1)
    nets = []
    for e in range(E):
        net = na.Phi(nTh=meta["nTh"], m=meta["m"], d=meta["d"], alph=meta["alph"])
        net.load_state_dict({k: v + (0.01 * e) * torch.randn(v.shape, generator=g) for k, v in sd.items()})
        nets.append(net.to(dev))
    rows = [[float(meta["alph"][0]), float(meta["alph_Q"]), float(meta["alph_W"])] + [float(v) for v in meta["alph"][3:6]]] * E
    cls = na.Quadcopter if meta.get("prob_class") == "Quadcopter" else na.Cross2D
    prob = cls(torch.from_numpy(z["xtarget"]).to(dev), obstacle=meta["obstacle"], alph_Q=meta["alph_Q"], alph_W=meta["alph_W"], r=meta["r"])
    xb = torch.from_numpy(z["x"])
    x = xb[torch.arange(n) % xb.shape[0]] + 0.01 * torch.randn(n, xb.shape[1], generator=g)
    return nets, rows, prob, x.to(dev).contiguous(), meta


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


def measure(name, family, nt, n, E, reps, warmup):
    import torch
    import neuraloc_amd as na
    from neuraloc_amd import _lib
    dev = torch.device("cuda:0")
    nets, rows, prob, x, meta = load(name, n, E, dev)
    ens = na.PhiEnsemble.from_members(nets, alph=rows)
    ts = [0.0, 1.0]
    levels = [0.05 * (e + 1) for e in range(E)]
    sigma = [[s_] for s_ in levels]
    out = {"name": name, "family": family, "nt": nt, "n": n, "E": E, "m": meta["m"], "d": meta["d"], "sigma": levels}
    kern = lambda: _lib.lib().nocf_last_rollout_kernel().decode()      # noqa: E731

    prob.eval()

    def ens_noisy():
        with torch.no_grad():
            na.ensemble_noisy_rollout(x, ens, prob, ts, nt, sigma, SEED, "rk4", family=family)

    def ens_plain():
        with torch.no_grad():
            na.ensemble_rollout(x, ens, prob, ts, nt, "rk4", family=family)

    def seq_noisy():
        with torch.no_grad():
            for e in range(E):
                na.noisy_rollout(x, nets[e], prob, nt, levels[e], SEED, tspan=ts, alph=rows[e], stepper="rk4")

    def one_noisy():
        with torch.no_grad():
            na.noisy_rollout(x, nets[0], prob, nt, levels[0], SEED, tspan=ts, alph=rows[0], stepper="rk4")

    def one_plain():
        with torch.no_grad():
            na.OCflow(x, nets[0], prob, ts, nt, "rk4", rows[0])

    ens_noisy()
    out["ens_kernel"] = kern()
    seq_noisy()
    out["seq_kernel"] = kern()
    with torch.no_grad():
        Jc, _ = na.ensemble_noisy_rollout(x, ens, prob, ts, nt, sigma, SEED, "rk4", family=family)
        ref = [na.noisy_rollout(x, nets[e], prob, nt, levels[e], SEED, tspan=ts, alph=rows[e], stepper="rk4")["Jc"] for e in range(E)]
        if not all(torch.equal(Jc[e], ref[e]) for e in range(E)):
            raise SystemExit("the noisy ensemble and the sequential noisy calls disagree")
    for leg, ms in zip(LEGS, timed([ens_noisy, ens_plain, seq_noisy, one_noisy, one_plain], reps, warmup)):
        out["eval_" + leg] = ms

    prob.train()
    opt = torch.optim.Adam(ens.parameters(), lr=1e-4)
    opts = [torch.optim.Adam(q.parameters(), lr=1e-4) for q in nets]

    def ens_noisy_adam():
        opt.zero_grad()
        Jc, _ = na.ensemble_noisy_ocflow_train(x, ens, prob, ts, nt, sigma, SEED, "rk4", family=family)
        Jc.sum().backward()
        opt.step()

    def ens_plain_adam():
        opt.zero_grad()
        Jc, _ = na.ensemble_ocflow_train(x, ens, prob, ts, nt, "rk4", family=family)
        Jc.sum().backward()
        opt.step()

    def seq_noisy_adam(members=None):
        for e in range(E) if members is None else members:
            opts[e].zero_grad()
            J1, _ = na.noisy_ocflow_train(x, nets[e], prob, ts, nt, levels[e], SEED, "rk4", rows[e])
            J1.backward()
            opts[e].step()

    def one_plain_adam():
        opts[0].zero_grad()
        J1, _ = na.OCflow(x, nets[0], prob, ts, nt, "rk4", rows[0])
        J1.backward()
        opts[0].step()

    ens_noisy_adam()
    out["ens_bwd_kernel"] = kern()
    seq_noisy_adam()
    out["seq_bwd_kernel"] = kern()
    for leg, ms in zip(LEGS, timed([ens_noisy_adam, ens_plain_adam, seq_noisy_adam, lambda: seq_noisy_adam([0]), one_plain_adam], reps, warmup)):
        out["adam_" + leg] = ms
    na.check_errors(sync=True)
    return out


def kernel_times(name, family, nt, n, E):
    """kernel-only ms per launch of the four evaluation legs (the library's event pairs around the rollout kernel)"""
    import ctypes as C
    import torch
    import neuraloc_amd as na
    from neuraloc_amd import _lib
    dev = torch.device("cuda:0")
    L = _lib.lib()
    nets, rows, prob, x, _meta = load(name, n, E, dev)
    ens = na.PhiEnsemble.from_members(nets, alph=rows)
    ts = [0.0, 1.0]
    levels = [0.05 * (e + 1) for e in range(E)]
    sigma = [[s_] for s_ in levels]
    prob.eval()
    legs = {
        "ens_noisy": lambda: na.ensemble_noisy_rollout(x, ens, prob, ts, nt, sigma, SEED, "rk4", family=family),
        "ens_plain": lambda: na.ensemble_rollout(x, ens, prob, ts, nt, "rk4", family=family),
        "one_noisy": lambda: na.noisy_rollout(x, nets[0], prob, nt, levels[0], SEED, tspan=ts, alph=rows[0], stepper="rk4"),
        "one_plain": lambda: na.OCflow(x, nets[0], prob, ts, nt, "rk4", rows[0]),
    }
    out = {"name": name, "family": family, "E": E}
    with torch.no_grad():
        for leg, fn in legs.items():
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            per = []
            for _ in range(5):
                L.nocf_profile_begin()
                for _ in range(10):
                    fn()
                ms, cnt = C.c_double(0), C.c_int32(0)
                L.nocf_profile_end(C.byref(ms), C.byref(cnt))
                per.append(ms.value / max(1, cnt.value))
            out[leg] = per
    return out


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "ensemble_noise"))
    args = p.parse_args(argv)
    os.environ.setdefault("NOCF_JIT", "0")
    rows = [measure(name, family, nt, n, E, args.reps, args.warmup) for name, family, nt, n in SHAPES for E in MEMBERS]
    lines = ["measured on the MI355X; ms = median [smallest, largest] of %d repetitions after %d warm-ups; ratios per repetition: median "
             "[smallest, largest] +- spread (largest - smallest)" % (args.reps, args.warmup),
             "(a) noisy ensemble / undisturbed ensemble;  single: noisy / undisturbed single-network call, the yardstick of (a);  "
             "(b) E sequential noisy calls / noisy ensemble",
             "%-12s %-4s %2s %-4s %22s %22s %22s   %-24s %-24s %-24s" % ("shape", "fam", "E", "what", "noisy ensemble ms", "undisturbed ens. ms",
                                                                      "E sequential noisy ms", "(a)", "single", "(b)")]

    def cell(v):
        return "%8.3f [%.3f,%.3f]" % (statistics.median(v), min(v), max(v))

    def ratio(r, key, num, den):
        q = [a / b for a, b in zip(r[num], r[den])]
        r[key], r[key + "_spread"] = statistics.median(q), max(q) - min(q)
        return "%5.2f [%.2f,%.2f] +-%.2f" % (r[key], min(q), max(q), r[key + "_spread"])
    for r in rows:
        for what in ("eval", "adam"):
            a = ratio(r, what + "_a", what + "_ens_noisy", what + "_ens_plain")
            one = ratio(r, what + "_single", what + "_one_noisy", what + "_one_plain")
            b = ratio(r, what + "_b", what + "_seq_noisy", what + "_ens_noisy")
            lines.append("%-12s %-4s %2d %-4s %22s %22s %22s   %-24s %-24s %-24s" % (
                r["name"], r["family"], r["E"], what, cell(r[what + "_ens_noisy"]), cell(r[what + "_ens_plain"]), cell(r[what + "_seq_noisy"]),
                a, one, b))
    lines.append("")
    for name, _f, _nt, _n in SHAPES:
        r0 = next(r for r in rows if r["name"] == name)
        lines.append("kernels %-12s: noisy ensemble %s / %s, sequential %s / %s" % (name, r0["ens_kernel"], r0["ens_bwd_kernel"], r0["seq_kernel"],
                                                                                    r0["seq_bwd_kernel"]))
    # (a) at E = 1 against the single-network yardstick of the same run: above it by more than the spreads, or not
    for r in rows:
        if r["E"] == 1:
            for what in ("eval", "adam"):
                over = r[what + "_a"] - r[what + "_single"]
                slack = max(r[what + "_a_spread"], r[what + "_single_spread"])
                lines.append("%-12s E=1 %-4s: (a) %.3f against the single-network %.3f: %s the spread %.3f" % (
                    r["name"], what, r[what + "_a"], r[what + "_single"], "ABOVE it by more than" if over > slack else "within", slack))
    text = "\n".join(lines)
    print(text)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "ensemble_noise_time.txt"), "w") as f:
        f.write(text + "\n")
    with open(os.path.join(args.out, "ensemble_noise_time.json"), "w") as f:
        json.dump(rows, f, indent=1)
    krows = [kernel_times(name, family, nt, n, E) for name, family, nt, n in SHAPES for E in (1, 8)]
    klines = ["measured on the MI355X; rollout-kernel ms per launch between the library's own event pairs (nocf_profile_begin / nocf_profile_end), "
              "median [smallest, largest] of 5 batches of 10 launches; evaluation, n = 1024",
              "%-12s %-4s %2s %26s %26s %26s %26s %8s %8s" % ("shape", "fam", "E", "noisy ensemble", "undisturbed ensemble", "single noisy",
                                                          "single undisturbed", "(a)", "single")]
    for r in krows:
        med = {leg: statistics.median(r[leg]) for leg in LEGS if leg in r}
        klines.append("%-12s %-4s %2d %26s %26s %26s %26s %8.3f %8.3f" % (
            r["name"], r["family"], r["E"], *["%.4f [%.4f,%.4f]" % (med[leg], min(r[leg]), max(r[leg]))
                                              for leg in ("ens_noisy", "ens_plain", "one_noisy", "one_plain")],
            med["ens_noisy"] / med["ens_plain"], med["one_noisy"] / med["one_plain"]))
    ktext = "\n".join(klines)
    print()
    print(ktext)
    with open(os.path.join(args.out, "ensemble_noise_kernels.txt"), "w") as f:
        f.write(ktext + "\n")


if __name__ == "__main__":
    main()
