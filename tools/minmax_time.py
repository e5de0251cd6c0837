#!/usr/bin/env python3
"""Time the joint adjoint (nocf_rollout_bwd_small_w_f32 / _mid_w_f32 / _act_w_f32) on the MI355X against the two calls that give the same
outputs without it -- the full adjoint entry followed by the state-only entry -- and a "free" adversarial Adam iteration against a disturbed
and a one-step PGD iteration, for one workload per kernel family, all at n = 1024 (profiles/adversary/adversary_time.txt's workloads):
  * softcorridor nt = 50 (lane), singlequad nt = 50 (one-CU), swarm50 nt = 80 with NOCF_DUO=0 (per-tile and its nine row streams);
  * (a) "joint" against "two" (full, then states) and against "full" alone: all at the C entry points, on ONE recorded forward (a disturbed
    recording forward, made once) and preallocated outputs -- the ratios are per repeat, their spread the largest ratio minus the smallest;
    the condition is joint / two < 1 - spread;
  * (b) ms per Adam iteration (zero_grad, call, backward, step), networks and problems in training mode: "free" (neuraloc_amd.adversarial_step),
    "disturbed" (disturbed_ocflow_train at a fixed W) and "pgd1" (pgd_ocflow_train with one inner step).
A repeat is --warmup calls and then --iters calls inside one HIP event pair; the legs alternate within a repeat and there are --repeats of
them.  Each workload runs in a child process of its own, because the library reads its NOCF_* knobs once.

    python tools/minmax_time.py [--iters 10] [--warmup 3] [--repeats 3] [--out profiles/minmax]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tools.disturb_time import load                                   # noqa: E402  (the fixtures' networks, problems and batches)

# (fixture, nt, n, family, NOCF_DUO)
WORKLOADS = [("softcorridor", 50, 1024, "lane", None), ("singlequad", 50, 1024, "one-CU", None), ("swarm50", 80, 1024, "per-tile", "0")]
ENTRY_LEGS = ("joint", "two", "full")
ITER_LEGS = ("free", "disturbed", "pgd1")


def _timed(fns, legs, iters, warmup, repeats, na):
    import torch
    ms = {leg: [] for leg in legs}
    for _ in range(repeats):
        for leg in legs:
            for _ in range(warmup):
                fns[leg]()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fns[leg]()
            e1.record()
            e1.synchronize()
            na.check_errors(sync=True)
            ms[leg].append(e0.elapsed_time(e1) / iters)
    return ms


def child(name, nt, n, family, iters, warmup, repeats):
    import torch
    import neuraloc_amd as na
    from neuraloc_amd import _lib, adversary, train
    from neuraloc_amd.train import _STEPPERS
    dev = torch.device("cuda:0")
    net, prob, x, meta = load(name, n, dev)
    net.eval()
    prob.eval()
    alph, d, m = meta["alph"], x.shape[1], meta["m"]
    W = na.brownian_disturbances(nt, n, d, 0.05 * float(meta["r"]), generator=torch.Generator(device=dev).manual_seed(2), device=dev)
    eps = float(W.pow(2).sum((0, 2)).sqrt().median())
    with torch.no_grad():
        s = adversary._Search(x, net, prob, nt, (0.0, 1.0), alph, "rk4", "Jc", 1.0 / n, True, "minmax_time")
        s.gradient(W)                                                    # the recorded inputs of every adjoint leg
        torch.cuda.synchronize()
        L, st = s.L, _STEPPERS["rk4"]
        f_small, f_mid, f_act = train._joint_entries(L)
        common = (C.byref(s.phi_st), C.byref(s.prob_st), n, nt, st, 1.0, s.alph_fwd, 1.0 / n, _lib.ptr(s.s_all), _lib.ptr(s.z_out), _lib.ptr(s.hs))
        wsargs = (_lib.ptr(s.ws), s.ws.numel(), _lib.stream_ptr(dev))
        act = s.act                                                      # (the one-CU forward's record; None elsewhere)
        lam0, lamW = torch.empty(n, d, device=dev), torch.empty(nt, n, d, device=dev)
        lam0j = torch.empty(n, d, device=dev)
        P = int(L.nocf_small_grad_floats(d, m))

        def states():
            _lib.check(s.f_states(*common, _lib.ptr(act), _lib.ptr(s.dx), _lib.ptr(s.dW), *wsargs), "nocf_rollout_bwd_states_f32")
        if family == "lane":
            gpart = torch.empty(n, P, device=dev)

            def full():
                _lib.check(L.nocf_rollout_bwd_small_f32(*common, _lib.ptr(gpart), _lib.ptr(lam0), _lib.stream_ptr(dev)), "nocf_rollout_bwd_small_f32")

            def joint():
                _lib.check(f_small(*common, _lib.ptr(gpart), _lib.ptr(lam0j), _lib.ptr(lamW), _lib.stream_ptr(dev)), "nocf_rollout_bwd_small_w_f32")
        elif family == "one-CU":
            rows = int(L.nocf_mid_grad_rows(d, m, net.nTh, s.phi_st.r, s.prob_st.n_agents, n))
            gmid = torch.empty(rows, P, device=dev)

            def full():
                _lib.check(L.nocf_rollout_bwd_mid_f32(*common, _lib.ptr(act), _lib.ptr(gmid), rows, _lib.ptr(lam0), *wsargs), "nocf_rollout_bwd_mid_f32")

            def joint():
                _lib.check(f_mid(*common, _lib.ptr(act), _lib.ptr(gmid), rows, _lib.ptr(lam0j), _lib.ptr(lamW), *wsargs), "nocf_rollout_bwd_mid_w_f32")
        else:
            R, D1, Lr = (nt * 4 + 2) * n, d + 1, net.nTh - 1
            Y, Ob, Wb = (torch.empty(R, m, device=dev) for _ in range(3))
            V, Ab, Qb, U0 = (torch.empty(Lr, R, m, device=dev) for _ in range(4))
            Gb, Sx, PHIb = torch.empty(R, D1, device=dev), torch.empty(R, D1, device=dev), torch.zeros(n, device=dev)
            streams = [_lib.ptr(t) for t in (Y, Ob, V, Ab, Qb, U0, Wb, Gb, Sx, PHIb)]

            def full():
                _lib.check(L.nocf_rollout_bwd_act_f32(*common, *streams, _lib.ptr(lam0), None, *wsargs), "nocf_rollout_bwd_act_f32")

            def joint():
                _lib.check(f_act(*common, *streams, _lib.ptr(lam0j), _lib.ptr(lamW), None, *wsargs), "nocf_rollout_bwd_act_w_f32")

        def two():
            full()
            states()
        kernels = {"forward": s.forward_kernel}
        for leg, fn in (("states", states), ("full", full), ("joint", joint)):
            fn()
            torch.cuda.synchronize()
            kernels[leg] = L.nocf_last_rollout_kernel().decode()
        # the joint call's outputs against the two calls': dJ/dW and dJ/dx0, largest difference and scale
        agree = {"lamW": (float((lamW - s.dW).abs().max()), float(s.dW.abs().max())),
                 "lam0": (float((lam0j - lam0).abs().max()), float(lam0.abs().max()))}
        ms = _timed({"joint": joint, "two": two, "full": full}, ENTRY_LEGS, iters, warmup, repeats, na)
    net.train()
    prob.train()
    optim = torch.optim.Adam(net.parameters(), lr=1e-5)
    Wfree = torch.zeros(nt, n, d, device=dev, requires_grad=True)
    ts = [0.0, 1.0]

    def free():
        optim.zero_grad()
        na.adversarial_step(x, net, prob, ts, nt, Wfree, eps, 2.5 * eps / 20, stepper="rk4", alph=alph)
        optim.step()

    def disturbed():
        optim.zero_grad()
        Jc, _ = na.disturbed_ocflow_train(x, net, prob, ts, nt, W, "rk4", alph)
        Jc.backward()
        optim.step()

    def pgd1():
        optim.zero_grad()
        Jc, _, _ = na.pgd_ocflow_train(x, net, prob, ts, nt, eps, 1, objective="Jc", stepper="rk4", alph=alph)
        Jc.backward()
        optim.step()
    ms_it = _timed({"free": free, "disturbed": disturbed, "pgd1": pgd1}, ITER_LEGS, iters, warmup, repeats, na)
    out = {"name": name, "family": family, "nt": nt, "n": n, "d": d, "m": m, "NOCF_DUO": os.environ.get("NOCF_DUO"), "iters": iters,
           "warmup": warmup, "ms": ms, "ms_per_iteration": ms_it, "kernels": kernels, "agree": agree}
    print("RESULT " + json.dumps(out), flush=True)


def run_child(args, name, nt, n, family, duo):
    env = dict(os.environ, NOCF_JIT="0")
    if duo is not None:
        env["NOCF_DUO"] = duo
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--iters", str(args.iters), "--warmup", str(args.warmup), "--repeats",
                        str(args.repeats), "--child", name, str(nt), str(n), family], env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"{name} (NOCF_DUO={duo}) failed with exit status {r.returncode}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def _ratio(a, b):
    rs = [u / v for u, v in zip(a, b)]
    return statistics.median(rs), max(rs) - min(rs)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "minmax"))
    p.add_argument("--child", nargs=4, default=None, help=argparse.SUPPRESS)
    args = p.parse_args(argv)
    if args.child:
        return child(args.child[0], int(args.child[1]), int(args.child[2]), args.child[3], args.iters, args.warmup, args.repeats)
    rows = []
    for name, nt, n, family, duo in WORKLOADS:
        row = run_child(args, name, nt, n, family, duo)
        row["joint_over_two"], row["joint_over_two_spread"] = _ratio(row["ms"]["joint"], row["ms"]["two"])
        row["joint_over_full"], row["joint_over_full_spread"] = _ratio(row["ms"]["joint"], row["ms"]["full"])
        row["faster"] = bool(row["joint_over_two"] < 1.0 - row["joint_over_two_spread"])
        it = row["ms_per_iteration"]
        row["free_over_disturbed"], row["free_over_disturbed_spread"] = _ratio(it["free"], it["disturbed"])
        row["free_over_pgd1"], row["free_over_pgd1_spread"] = _ratio(it["free"], it["pgd1"])
        rows.append(row)
        print("%s: joint / (full + states) %.3f +- %.3f" % (name, row["joint_over_two"], row["joint_over_two_spread"]), flush=True)

    def cell(v):
        return " ".join("%.3f" % t for t in v)
    lines = ["%-13s %-8s %5s %3s  %-24s %-24s %-24s %-13s %-13s" % (
        "workload", "family", "n", "nt", "joint ms (repeats)", "full+states ms (repeats)", "full ms (repeats)", "joint/two", "joint/full")]
    for r in rows:
        lines.append("%-13s %-8s %5d %3d  %-24s %-24s %-24s %5.3f+-%.3f %5.3f+-%.3f" % (
            r["name"], r["family"], r["n"], r["nt"], cell(r["ms"]["joint"]), cell(r["ms"]["two"]), cell(r["ms"]["full"]),
            r["joint_over_two"], r["joint_over_two_spread"], r["joint_over_full"], r["joint_over_full_spread"]))
        lines.append("    forward %s; adjoints %s, %s, %s; joint faster than the two calls by more than the spread: %s" % (
            r["kernels"]["forward"], r["kernels"]["joint"], r["kernels"]["full"], r["kernels"]["states"], "yes" if r["faster"] else "NO"))
        lines.append("    joint against the two calls: dJ/dW max |diff| %.3e of %.3e, dJ/dx0 %.3e of %.3e" % (*r["agree"]["lamW"], *r["agree"]["lam0"]))
        it = r["ms_per_iteration"]
        lines.append("    ms per Adam iteration: free %s | disturbed %s | pgd (1 step) %s | free/disturbed %.3f+-%.3f, free/pgd1 %.3f+-%.3f" % (
            cell(it["free"]), cell(it["disturbed"]), cell(it["pgd1"]), r["free_over_disturbed"], r["free_over_disturbed_spread"],
            r["free_over_pgd1"], r["free_over_pgd1_spread"]))
    text = "\n".join(lines)
    print(text)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "minmax_time.txt"), "w") as f:
        f.write(text + "\n")
    with open(os.path.join(args.out, "minmax_time.json"), "w") as f:
        json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
