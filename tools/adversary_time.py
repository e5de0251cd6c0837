#!/usr/bin/env python3
"""Time the state-only adjoint (nocf_rollout_bwd_states_f32) on the MI355X against the full adjoint entry of the same kernel family, and
one iteration of the worst-case disturbance search, for one workload per family, all at n = 1024:
  * softcorridor nt = 50 (lane kernels: nocf_rollout_bwd_small_f32), singlequad nt = 50 (one-CU kernels: nocf_rollout_bwd_mid_f32),
    swarm50 nt = 80 with NOCF_DUO=0 (per-tile kernels: nocf_rollout_bwd_act_f32 and its nine row streams);
  * (a) "states" against "full": both at the C entry points, on the same recorded inputs (one disturbed recording forward, made once) and
    preallocated outputs -- the ratio is states / full per repeat, its spread the largest ratio minus the smallest;
  * (b) "iteration": recording forward + state-only adjoint + ascent step (neuraloc_amd.adversary's three launches);
  * (c) peak device memory of (a)'s two legs above what the inputs hold (torch.cuda.max_memory_allocated), outputs included.
A repeat is --warmup calls and then --iters calls inside one HIP event pair; the legs alternate within a repeat and there are --repeats of
them.  Each workload runs in a child process of its own, because the library reads its NOCF_* knobs once.

    python tools/adversary_time.py [--iters 10] [--warmup 3] [--repeats 3] [--out profiles/adversary]
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
LEGS = ("states", "full", "iteration")


def child(name, nt, n, family, iters, warmup, repeats):
    import torch
    import neuraloc_amd as na
    from neuraloc_amd import _lib, adversary
    from neuraloc_amd.train import _STEPPERS
    dev = torch.device("cuda:0")
    net, prob, x, meta = load(name, n, dev)
    net.eval()
    prob.eval()
    alph, d, m = meta["alph"], x.shape[1], meta["m"]
    W = na.brownian_disturbances(nt, n, d, 0.05 * float(meta["r"]), generator=torch.Generator(device=dev).manual_seed(2), device=dev)
    eps = float(W.pow(2).sum((0, 2)).sqrt().median())
    with torch.no_grad():
        s = adversary._Search(x, net, prob, nt, (0.0, 1.0), alph, "rk4", "Jc", 1.0 / n, True, "adversary_time")
        s.gradient(W)                                                    # the recorded inputs of both adjoint legs
        torch.cuda.synchronize()
        L, st = s.L, _STEPPERS["rk4"]
        common = (C.byref(s.phi_st), C.byref(s.prob_st), n, nt, st, 1.0, s.alph_fwd, 1.0 / n, _lib.ptr(s.s_all), _lib.ptr(s.z_out), _lib.ptr(s.hs))
        wsargs = (_lib.ptr(s.ws), s.ws.numel(), _lib.stream_ptr(dev))
        act = s.act                                                      # (the one-CU forward's record; None elsewhere)
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)

        def states():
            _lib.check(s.f_states(*common, _lib.ptr(act), _lib.ptr(s.dx), _lib.ptr(s.dW), *wsargs), "nocf_rollout_bwd_states_f32")
        states()
        torch.cuda.synchronize()
        kernels = {"forward": s.forward_kernel, "states": L.nocf_last_rollout_kernel().decode()}
        # (dW and dx were allocated with the inputs: count them with the states leg)
        mem = {"states": torch.cuda.max_memory_allocated(dev) - base + 4 * (s.dW.numel() + s.dx.numel())}
        lam0 = torch.empty(n, d, device=dev)
        P = int(L.nocf_small_grad_floats(d, m))
        if family == "lane":
            gpart = torch.empty(n, P, device=dev)

            def full():
                _lib.check(L.nocf_rollout_bwd_small_f32(*common, _lib.ptr(gpart), _lib.ptr(lam0), _lib.stream_ptr(dev)), "nocf_rollout_bwd_small_f32")
        elif family == "one-CU":
            rows = int(L.nocf_mid_grad_rows(d, m, net.nTh, s.phi_st.r, s.prob_st.n_agents, n))
            gmid = torch.empty(rows, P, device=dev)

            def full():
                _lib.check(L.nocf_rollout_bwd_mid_f32(*common, _lib.ptr(act), _lib.ptr(gmid), rows, _lib.ptr(lam0), *wsargs), "nocf_rollout_bwd_mid_f32")
        else:
            R, D1, Lr = (nt * 4 + 2) * n, d + 1, net.nTh - 1
            Y, Ob, Wb = (torch.empty(R, m, device=dev) for _ in range(3))
            V, Ab, Qb, U0 = (torch.empty(Lr, R, m, device=dev) for _ in range(4))
            Gb, Sx, PHIb = torch.empty(R, D1, device=dev), torch.empty(R, D1, device=dev), torch.zeros(n, device=dev)

            def full():
                _lib.check(L.nocf_rollout_bwd_act_f32(*common, *[_lib.ptr(t) for t in (Y, Ob, V, Ab, Qb, U0, Wb, Gb, Sx, PHIb, lam0)], None, *wsargs),
                           "nocf_rollout_bwd_act_f32")
        full()
        torch.cuda.synchronize()
        kernels["full"] = L.nocf_last_rollout_kernel().decode()
        mem["full"] = torch.cuda.max_memory_allocated(dev) - base
        agree = float((lam0 - s.dx).abs().max()), float(lam0.abs().max())   # dJ/dx0 of the two legs on the same inputs
        Wit = torch.zeros_like(W)

        def iteration():
            s.gradient(Wit)
            s.ascent(Wit, None, 2.5 * eps / 20, eps)
        fns = {"states": states, "full": full, "iteration": iteration}
        ms = {leg: [] for leg in LEGS}
        for _ in range(repeats):
            for leg in LEGS:
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
    out = {"name": name, "family": family, "nt": nt, "n": n, "d": d, "m": m, "NOCF_DUO": os.environ.get("NOCF_DUO", "1"), "iters": iters,
           "warmup": warmup, "ms": ms, "kernels": kernels, "peak_bytes": mem, "lam0_max_abs_diff": agree[0], "lam0_max_abs": agree[1]}
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


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "adversary"))
    p.add_argument("--child", nargs=4, default=None, help=argparse.SUPPRESS)
    args = p.parse_args(argv)
    if args.child:
        return child(args.child[0], int(args.child[1]), int(args.child[2]), args.child[3], args.iters, args.warmup, args.repeats)
    rows = []
    for name, nt, n, family, duo in WORKLOADS:
        row = run_child(args, name, nt, n, family, duo)
        rs = [a / b for a, b in zip(row["ms"]["states"], row["ms"]["full"])]
        row["ratio"], row["ratio_spread"] = statistics.median(rs), max(rs) - min(rs)
        row["not_slower"] = bool(row["ratio"] <= 1.0 + row["ratio_spread"])
        rows.append(row)
        print("%s: states / full %.3f +- %.3f" % (name, row["ratio"], row["ratio_spread"]), flush=True)

    def cell(v):
        return " ".join("%.3f" % t for t in v)
    lines = ["%-13s %-8s %5s %3s  %-24s %-24s %-13s %-24s %10s %10s" % (
        "workload", "family", "n", "nt", "states ms (repeats)", "full ms (repeats)", "states/full", "iteration ms (repeats)", "states MB", "full MB")]
    for r in rows:
        lines.append("%-13s %-8s %5d %3d  %-24s %-24s %5.3f+-%.3f %-24s %10.1f %10.1f" % (
            r["name"], r["family"], r["n"], r["nt"], cell(r["ms"]["states"]), cell(r["ms"]["full"]), r["ratio"], r["ratio_spread"],
            cell(r["ms"]["iteration"]), r["peak_bytes"]["states"] / 2 ** 20, r["peak_bytes"]["full"] / 2 ** 20))
        lines.append("    forward %s; adjoints %s, %s; states not slower than full by more than the spread: %s; dJ/dx0 of the two: max |diff| %.3e of %.3e" % (
            r["kernels"]["forward"], r["kernels"]["states"], r["kernels"]["full"], "yes" if r["not_slower"] else "NO",
            r["lam0_max_abs_diff"], r["lam0_max_abs"]))
    text = "\n".join(lines)
    print(text)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "adversary_time.txt"), "w") as f:
        f.write(text + "\n")
    with open(os.path.join(args.out, "adversary_time.json"), "w") as f:
        json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
