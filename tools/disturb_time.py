#!/usr/bin/env python3
"""Time the disturbed rollout (neuraloc_amd.disturbed_rollout: one launch per rollout) on the MI355X at the five BASELINE shapes, against
  * the undisturbed OCflow(noMean=True) on the SAME kernel (NOCF_DUO=0 for swarm50: disturbed rollouts never take the split-role kernel),
  * nt chained one-step OCflow(intermediates=True) calls with the displacement added by torch in between: the only way without it,
  * for swarm50 also the undisturbed call on the split-role kernel (what a disturbed m = 512 rollout gives up).
The disturbed and the undisturbed rollout are timed at the C entry points (nocf_rollout_disturbed_f32, nocf_rollout_means_f32) with the
structs, the workspace and every output buffer made once outside the HIP event pair, so their ratio compares the kernels and not Python's
allocations; the chained leg is timed as a user has to write it today: nt OCflow calls, their allocations and the torch additions
included.  Median of --reps after --warmup, the disturbed and the undisturbed call alternating;
the table also gives each leg's smallest and largest repetition.  Each kernel choice runs in a child process of its own, because the library reads its
NOCF_* knobs once.

    python tools/disturb_time.py [--reps 5] [--warmup 2] [--out profiles/disturb]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# (fixture, nt, n): BASELINE.md's table
SHAPES = [("swap2", 20, 1024), ("softcorridor", 50, 1024), ("swap12", 20, 2048), ("swarm50", 80, 1024), ("singlequad", 50, 4096)]


def load(name, n, dev):
    import numpy as np
    import torch
    import neuraloc_amd as na
    z = np.load(os.path.join(REPO, "tests", "golden", name + ".npz"))
    meta = json.loads(str(z["meta"]))
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}
    net = na.Phi(nTh=meta["nTh"], m=meta["m"], d=meta["d"], alph=meta["alph"])
    net.load_state_dict(sd)
    net = net.to(dev).eval()
    cls = {"Cross2D": na.Cross2D, "SwarmTraj": na.SwarmTraj, "Quadcopter": na.Quadcopter}[meta["prob_class"]]
    prob = cls(torch.from_numpy(z["xtarget"]).to(dev), obstacle=meta["obstacle"], alph_Q=meta["alph_Q"], alph_W=meta["alph_W"], r=meta["r"])
    prob.eval()
    xb = torch.from_numpy(z["x"])
    g = torch.Generator().manual_seed(1)
    x = xb[torch.arange(n) % xb.shape[0]] + 0.01 * torch.randn(n, xb.shape[1], generator=g)
    return net, prob, x.to(dev).contiguous(), meta


def timed(fns, reps, warmup):
    """[(median ms, all ms)] per function; the functions alternate within every repetition, so drift of the machine hits all of them alike"""
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
    return [(statistics.median(m), m) for m in ms]


def child(name, nt, n, reps, warmup):
    import ctypes as C
    import torch
    import neuraloc_amd as na
    from neuraloc_amd import _lib, disturb
    from neuraloc_amd.OCflow import _STEPPERS
    dev = torch.device("cuda:0")
    net, prob, x, meta = load(name, n, dev)
    alph = meta["alph"]
    d = x.shape[1]
    sigma = 0.05 * float(meta["r"])
    W = na.brownian_disturbances(nt, n, d, sigma, generator=torch.Generator(device=dev).manual_seed(2), device=dev)
    h = 1.0 / nt
    out = {"name": name, "nt": nt, "n": n, "d": d, "m": meta["m"], "NOCF_DUO": os.environ.get("NOCF_DUO", "1")}
    with torch.no_grad(), torch.cuda.device(dev):
        phi_st, keep1, ws = net._c_struct(n)
        prob_st, keep2 = prob._c_struct(dev)
        L = _lib.lib_for(net.d, net.m, net.nTh, phi_st.r, prob_st.n_agents, fwd=prob_st.kind != _lib.PROB_QUADCOPTER)
        f_dist = disturb._entry(L)
        if f_dist is None:
            L = _lib.lib()
            f_dist = disturb._entry(L)
        persample = torch.empty(n, 7, dtype=torch.float32, device=dev)
        sums = torch.empty(8, dtype=torch.float32, device=dev)
        means = torch.empty(8, dtype=torch.float32, device=dev)
        z_final = torch.empty(n, d + 4, dtype=torch.float32, device=dev)
        alph_c = (C.c_float * 6)(*[float(a) for a in alph[:6]])
        head = (C.byref(phi_st), C.byref(prob_st), _lib.ptr(x))
        tail = (n, 0.0, 1.0, nt, _STEPPERS["rk4"], alph_c, _lib.ptr(z_final), _lib.ptr(persample), _lib.ptr(sums), _lib.ptr(means),
                None, None, _lib.ptr(ws), ws.numel() * ws.element_size(), _lib.stream_ptr(dev))

        def disturbed():
            _lib.check(f_dist(*head, _lib.ptr(W), *tail), "nocf_rollout_disturbed_f32")

        def undisturbed():
            _lib.check(L.nocf_rollout_means_f32(*head, *tail), "nocf_rollout_means_f32")

        disturbed()
        out["disturbed_kernel"] = L.nocf_last_rollout_kernel().decode()
        _lib.track_rollout_status(L, dev, "disturb_time")
        na.check_errors(sync=True)
        ref = na.disturbed_rollout(x, net, prob, nt, W, alph=alph)
        if not (torch.equal(ref["persample"], persample) and torch.equal(ref["z_final"], z_final)):
            raise SystemExit("the timed call and neuraloc_amd.disturbed_rollout disagree")
        undisturbed()
        out["undisturbed_kernel"] = L.nocf_last_rollout_kernel().decode()
        _lib.track_rollout_status(L, dev, "disturb_time")
        na.check_errors(sync=True)
        (out["disturbed_ms"], out["disturbed_all"]), (out["undisturbed_ms"], out["undisturbed_all"]) = timed([disturbed, undisturbed], reps, warmup)
        _lib.track_rollout_status(L, dev, "disturb_time")
        na.check_errors(sync=True)

        def chained():
            xs = x
            for k in range(nt):
                zF, _ = na.OCflow(xs, net, prob, [k * h, (k + 1) * h], 1, "rk4", alph, intermediates=True)
                xs = (zF[:, :d, 1] + W[k]).contiguous()
        (out["chained_ms"], out["chained_all"]), = timed([chained], reps, warmup)
    na.check_errors(sync=True)
    print("RESULT " + json.dumps(out), flush=True)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "disturb"))
    p.add_argument("--child", nargs=3, default=None, help=argparse.SUPPRESS)
    args = p.parse_args(argv)
    if args.child:
        return child(args.child[0], int(args.child[1]), int(args.child[2]), args.reps, args.warmup)
    rows = []
    for name, nt, n in SHAPES:
        for duo in (("0", "1") if name == "swarm50" else ("1",)):
            env = dict(os.environ, NOCF_DUO=duo, NOCF_JIT="0")
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--warmup", str(args.warmup),
                                "--child", name, str(nt), str(n)], env=env, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit(f"{name} (NOCF_DUO={duo}) failed with exit status {r.returncode}")
            rows.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    lines = ["%-13s %5s %3s %3s  %-40s %-40s %22s %22s %22s %8s %10s" % (
        "shape", "n", "nt", "DUO", "disturbed kernel", "undisturbed kernel", "disturbed ms [min,max]", "undisturbed ms", "chained ms", "dist/und", "chain/dist")]

    def cell(r, k):
        return "%8.3f [%.3f,%.3f]" % (r[k + "_ms"], min(r[k + "_all"]), max(r[k + "_all"]))
    for r in rows:
        lines.append("%-13s %5d %3d %3s  %-40s %-40s %22s %22s %22s %8.3f %10.1f" % (
            r["name"], r["n"], r["nt"], r["NOCF_DUO"], r["disturbed_kernel"], r["undisturbed_kernel"], cell(r, "disturbed"),
            cell(r, "undisturbed"), cell(r, "chained"), r["disturbed_ms"] / r["undisturbed_ms"], r["chained_ms"] / r["disturbed_ms"]))
    text = "\n".join(lines)
    print(text)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "disturb_time.txt"), "w") as f:
        f.write(text + "\n")
    with open(os.path.join(args.out, "disturb_time.json"), "w") as f:
        json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
