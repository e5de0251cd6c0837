#!/usr/bin/env python3
"""Time the weighted adjoint (nocf_rollout_bwd_small_rw_f32 / _mid_rw_f32 / _act_rw_f32) on the MI355X against the unweighted entry of the same
family, and a risk-sensitive Adam iteration against a noisy one, for one workload per kernel family, all at n = 1024 and nt = 80:
  * softcorridor (lane), singlequad (one-CU), swarm50 with NOCF_DUO=0 (per-tile and its nine row streams);
  * (a) "weighted" against "full": both at the C entry points, on ONE recorded forward (a disturbed recording forward, made once), the same
    preallocated outputs and, in the weighted leg, non-uniform weights (both signs, a zero, a range of 100) -- the ratio is per repeat, its
    spread the largest ratio minus the smallest.  The yardstick is the unweighted entry: the expectation is one more load per row and launch,
    i.e. a ratio of 1 within the spread.  A third leg, "uniform", is the weighted entry at w = 1/n: the unweighted entry's arithmetic and
    bits from the weighted code, which tells the code's cost from that of the values it is given;
  * (b) ms per Adam iteration (zero_grad, call, backward, step), network and problem in training mode, on the same rows: "risk"
    (neuraloc_amd.risk_ocflow_train, CVaR 0.8 over groups of 8 consecutive rows) against "noisy" (noisy_ocflow_train), both under the same
    in-kernel noise.
A repeat is --warmup calls and then --iters calls inside one HIP event pair; the legs alternate within a repeat and there are --repeats of
them.  Each workload runs in a child process of its own, because the library reads its NOCF_* knobs once.

    python tools/risk_time.py [--iters 10] [--warmup 3] [--repeats 5] [--out profiles/risk]
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
from tools.minmax_time import _ratio, _timed                          # noqa: E402

# (fixture, nt, n, family, NOCF_DUO)
WORKLOADS = [("softcorridor", 80, 1024, "lane", None), ("singlequad", 80, 1024, "one-CU", None), ("swarm50", 80, 1024, "per-tile", "0")]
ENTRY_LEGS = ("weighted", "full", "uniform")
ITER_LEGS = ("risk", "noisy")
PATHS, LEVEL = 8, 0.8


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
    sigma = 0.05 * float(meta["r"])
    W = na.brownian_disturbances(nt, n, d, sigma, generator=torch.Generator(device=dev).manual_seed(2), device=dev)
    g = torch.Generator().manual_seed(5)
    wrow = (10.0 ** (2.0 * torch.rand(n, generator=g) - 2.0)) * torch.where(torch.rand(n, generator=g) < 0.3, -1.0, 1.0) / n
    wrow[n // 2] = 0.0
    wrow = wrow.to(dev).contiguous()
    uni = torch.full((n,), 1.0 / n, device=dev)
    with torch.no_grad():
        s = adversary._Search(x, net, prob, nt, (0.0, 1.0), alph, "rk4", "Jc", 1.0 / n, True, "risk_time")
        s.gradient(W)                                                    # the recorded inputs of both legs
        torch.cuda.synchronize()
        L, st = s.L, _STEPPERS["rk4"]
        f_small, f_mid, f_act = train._weighted_entries(L)
        head = (C.byref(s.phi_st), C.byref(s.prob_st), n, nt, st, 1.0, s.alph_fwd)
        tail = (_lib.ptr(s.s_all), _lib.ptr(s.z_out), _lib.ptr(s.hs))
        wsargs = (_lib.ptr(s.ws), s.ws.numel(), _lib.stream_ptr(dev))
        act = s.act                                                      # (the one-CU forward's record; None elsewhere)
        lam0 = torch.empty(n, d, device=dev)
        P = int(L.nocf_small_grad_floats(d, m))
        if family == "lane":
            out = torch.empty(n, P, device=dev)

            def full():
                _lib.check(L.nocf_rollout_bwd_small_f32(*head, 1.0 / n, *tail, _lib.ptr(out), _lib.ptr(lam0), _lib.stream_ptr(dev)), "nocf_rollout_bwd_small_f32")

            def weighted(w=wrow):
                _lib.check(f_small(*head, _lib.ptr(w), *tail, _lib.ptr(out), _lib.ptr(lam0), _lib.stream_ptr(dev)), "nocf_rollout_bwd_small_rw_f32")
        elif family == "one-CU":
            rows = int(L.nocf_mid_grad_rows(d, m, net.nTh, s.phi_st.r, s.prob_st.n_agents, n))
            out = torch.empty(rows, P, device=dev)

            def full():
                _lib.check(L.nocf_rollout_bwd_mid_f32(*head, 1.0 / n, *tail, _lib.ptr(act), _lib.ptr(out), rows, _lib.ptr(lam0), *wsargs), "nocf_rollout_bwd_mid_f32")

            def weighted(w=wrow):
                _lib.check(f_mid(*head, _lib.ptr(w), *tail, _lib.ptr(act), _lib.ptr(out), rows, _lib.ptr(lam0), *wsargs), "nocf_rollout_bwd_mid_rw_f32")
        else:
            R, D1, Lr = (nt * 4 + 2) * n, d + 1, net.nTh - 1
            Y, Ob, Wb = (torch.empty(R, m, device=dev) for _ in range(3))
            V, Ab, Qb, U0 = (torch.empty(Lr, R, m, device=dev) for _ in range(4))
            Gb, Sx, PHIb = torch.empty(R, D1, device=dev), torch.empty(R, D1, device=dev), torch.zeros(n, device=dev)
            out = Ob
            streams = [_lib.ptr(t) for t in (Y, Ob, V, Ab, Qb, U0, Wb, Gb, Sx, PHIb)]

            def full():
                _lib.check(L.nocf_rollout_bwd_act_f32(*head, 1.0 / n, *tail, *streams, _lib.ptr(lam0), None, *wsargs), "nocf_rollout_bwd_act_f32")

            def weighted(w=wrow):
                _lib.check(f_act(*head, _lib.ptr(w), *tail, *streams, _lib.ptr(lam0), None, *wsargs), "nocf_rollout_bwd_act_rw_f32")
        kernels = {"forward": s.forward_kernel}
        # the weighted entry at w = 1/n against the unweighted one: the outputs' bits
        full()
        torch.cuda.synchronize()
        kernels["full"] = L.nocf_last_rollout_kernel().decode()
        ref = (out.clone(), lam0.clone())
        weighted(uni)
        torch.cuda.synchronize()
        kernels["weighted"] = L.nocf_last_rollout_kernel().decode()
        same = bool(torch.equal(out, ref[0]) and torch.equal(lam0, ref[1]))
        ms = _timed({"weighted": weighted, "full": full, "uniform": lambda: weighted(uni)}, ENTRY_LEGS, iters, warmup, repeats, na)
    net.train()
    prob.train()
    optim = torch.optim.Adam(net.parameters(), lr=1e-5)
    ts = [0.0, 1.0]

    def risk():
        optim.zero_grad()
        Jr, _, _ = na.risk_ocflow_train(x, net, prob, ts, nt, "cvar", LEVEL, paths=PATHS, sigma=sigma, seed=11, stepper="rk4", alph=alph)
        Jr.backward()
        optim.step()

    def noisy():
        optim.zero_grad()
        Jc, _ = na.noisy_ocflow_train(x, net, prob, ts, nt, sigma, 11, "rk4", alph)
        Jc.backward()
        optim.step()
    ms_it = _timed({"risk": risk, "noisy": noisy}, ITER_LEGS, iters, warmup, repeats, na)
    res = {"name": name, "family": family, "nt": nt, "n": n, "d": d, "m": m, "NOCF_DUO": os.environ.get("NOCF_DUO"), "iters": iters,
           "warmup": warmup, "ms": ms, "ms_per_iteration": ms_it, "kernels": kernels, "uniform_weights_same_bits": same}
    print("RESULT " + json.dumps(res), flush=True)


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
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "risk"))
    p.add_argument("--child", nargs=4, default=None, help=argparse.SUPPRESS)
    args = p.parse_args(argv)
    if args.child:
        return child(args.child[0], int(args.child[1]), int(args.child[2]), args.child[3], args.iters, args.warmup, args.repeats)
    rows = []
    for name, nt, n, family, duo in WORKLOADS:
        row = run_child(args, name, nt, n, family, duo)
        row["weighted_over_full"], row["weighted_over_full_spread"] = _ratio(row["ms"]["weighted"], row["ms"]["full"])
        row["within_spread"] = bool(row["weighted_over_full"] <= 1.0 + row["weighted_over_full_spread"])
        row["uniform_over_full"], row["uniform_over_full_spread"] = _ratio(row["ms"]["uniform"], row["ms"]["full"])
        it = row["ms_per_iteration"]
        row["risk_over_noisy"], row["risk_over_noisy_spread"] = _ratio(it["risk"], it["noisy"])
        rows.append(row)
        print("%s: weighted / full %.3f +- %.3f" % (name, row["weighted_over_full"], row["weighted_over_full_spread"]), flush=True)

    def cell(v):
        return " ".join("%.3f" % t for t in v)
    lines = ["%-13s %-8s %5s %3s  %-36s %-36s %-13s" % ("workload", "family", "n", "nt", "weighted ms (repeats)", "full ms (repeats)", "weighted/full")]
    for r in rows:
        lines.append("%-13s %-8s %5d %3d  %-36s %-36s %5.3f+-%.3f" % (
            r["name"], r["family"], r["n"], r["nt"], cell(r["ms"]["weighted"]), cell(r["ms"]["full"]),
            r["weighted_over_full"], r["weighted_over_full_spread"]))
        lines.append("    forward %s; adjoints %s, %s; ratio above 1 by no more than the spread: %s; w = 1/n gives the unweighted entry's bits: %s" % (
            r["kernels"]["forward"], r["kernels"]["weighted"], r["kernels"]["full"], "yes" if r["within_spread"] else "NO",
            "yes" if r["uniform_weights_same_bits"] else "NO"))
        it = r["ms_per_iteration"]
        lines.append("    weighted entry at w = 1/n: %s ms | over full %.3f+-%.3f" % (cell(r["ms"]["uniform"]), r["uniform_over_full"], r["uniform_over_full_spread"]))
        lines.append("    ms per Adam iteration: risk (CVaR %.1f, %d paths) %s | noisy %s | risk/noisy %.3f+-%.3f" % (
            LEVEL, PATHS, cell(it["risk"]), cell(it["noisy"]), r["risk_over_noisy"], r["risk_over_noisy_spread"]))
    text = "\n".join(lines)
    print(text)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "risk_time.txt"), "w") as f:
        f.write(text + "\n")
    with open(os.path.join(args.out, "risk_time.json"), "w") as f:
        json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
