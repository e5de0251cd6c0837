#!/usr/bin/env python3
"""Time the rollout under counter-based noise (nocf_rollout_noisy_f32: the disturbances are drawn inside the kernels, DESIGN.md section
3.10) on the MI355X at the five BASELINE shapes of tools/disturb_time.py, against what it replaces.  Four legs:
  (a) nocf_rollout_noisy_f32;
  (b) nocf_rollout_disturbed_f32 on a W that is already there;
  (c) neuraloc_amd.brownian_disturbances (torch.randn, scaled) + (b): drawing the tensor and reading it back -- what (a) replaces;
  (d) nocf_noise_fill_f32 alone: the same values as a tensor.
tools/disturb_time.py's protocol: the C entry points, with the structs, the workspace and every output buffer made once outside the HIP
event pair ((c) allocates its W inside: that allocation is part of what it costs); the legs alternate within a repetition; median of
--reps after --warmup, with each leg's smallest and largest repetition.  One child process per shape (NOCF_JIT=0: the shipped library).

    python tools/noise_time.py [--reps 5] [--warmup 2] [--out profiles/noise]
"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from disturb_time import SHAPES, load, timed                # noqa: E402

LEGS = ("noisy", "disturbed", "drawn", "fill")


def child(name, nt, n, reps, warmup):
    import ctypes as C
    import torch
    import neuraloc_amd as na
    from neuraloc_amd import _lib, disturb, noise
    from neuraloc_amd.OCflow import _STEPPERS
    dev = torch.device("cuda:0")
    net, prob, x, meta = load(name, n, dev)
    alph = meta["alph"]
    d = x.shape[1]
    sigma = 0.05 * float(meta["r"])
    seed = 0x1234567887654321
    gen = torch.Generator(device=dev).manual_seed(2)
    out = {"name": name, "nt": nt, "n": n, "d": d, "m": meta["m"], "W_bytes": 4 * nt * n * d}
    with torch.no_grad(), torch.cuda.device(dev):
        phi_st, keep1, ws = net._c_struct(n)
        prob_st, keep2 = prob._c_struct(dev)
        L = _lib.lib_for(net.d, net.m, net.nTh, phi_st.r, prob_st.n_agents, fwd=prob_st.kind != _lib.PROB_QUADCOPTER)
        L, f_noisy = noise._entry_for(L, "nocf_rollout_noisy_f32", "noise_time")
        f_dist = disturb._entry(L)
        _, f_fill = noise._entry_for(L, "nocf_noise_fill_f32", "noise_time")
        scale = noise.noise_scale(sigma, nt, d).to(dev)
        W = na.counter_disturbances(nt, n, d, sigma, seed, device=dev)
        Wf = torch.empty_like(W)
        persample = torch.empty(n, 7, dtype=torch.float32, device=dev)
        sums = torch.empty(8, dtype=torch.float32, device=dev)
        means = torch.empty(8, dtype=torch.float32, device=dev)
        z_final = torch.empty(n, d + 4, dtype=torch.float32, device=dev)
        alph_c = (C.c_float * 6)(*[float(a) for a in alph[:6]])
        head = (C.byref(phi_st), C.byref(prob_st), _lib.ptr(x))
        tail = (n, 0.0, 1.0, nt, _STEPPERS["rk4"], alph_c, _lib.ptr(z_final), _lib.ptr(persample), _lib.ptr(sums), _lib.ptr(means),
                None, None, _lib.ptr(ws), ws.numel() * ws.element_size(), _lib.stream_ptr(dev))

        def noisy():
            _lib.check(f_noisy(*head, _lib.ptr(scale), seed, 0, *tail), "nocf_rollout_noisy_f32")

        def disturbed():
            _lib.check(f_dist(*head, _lib.ptr(W), *tail), "nocf_rollout_disturbed_f32")

        def drawn():
            Wd = na.brownian_disturbances(nt, n, d, sigma, generator=gen, device=dev)
            _lib.check(f_dist(*head, _lib.ptr(Wd), *tail), "nocf_rollout_disturbed_f32")

        def fill():
            _lib.check(f_fill(_lib.ptr(Wf), n, nt, d, _lib.ptr(scale), seed, 0, _lib.stream_ptr(dev)), "nocf_noise_fill_f32")

        disturbed()
        out["disturbed_kernel"] = L.nocf_last_rollout_kernel().decode()
        _lib.track_rollout_status(L, dev, "noise_time")
        na.check_errors(sync=True)
        tab, zf = persample.clone(), z_final.clone()
        noisy()
        out["noisy_kernel"] = L.nocf_last_rollout_kernel().decode()
        _lib.track_rollout_status(L, dev, "noise_time")
        na.check_errors(sync=True)
        fill()
        torch.cuda.synchronize()
        if not (torch.equal(tab, persample) and torch.equal(zf, z_final) and torch.equal(W, Wf)):
            raise SystemExit("the noisy call and the disturbed call on the filled W disagree")
        res = timed([noisy, disturbed, drawn, fill], reps, warmup)
        for leg, (med, allms) in zip(LEGS, res):
            out[leg + "_ms"], out[leg + "_all"] = med, allms
        _lib.track_rollout_status(L, dev, "noise_time")
    na.check_errors(sync=True)
    print("RESULT " + json.dumps(out), flush=True)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "noise"))
    p.add_argument("--child", nargs=3, default=None, help=argparse.SUPPRESS)
    args = p.parse_args(argv)
    if args.child:
        return child(args.child[0], int(args.child[1]), int(args.child[2]), args.reps, args.warmup)
    rows = []
    for name, nt, n in SHAPES:
        env = dict(os.environ, NOCF_JIT="0")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--warmup", str(args.warmup),
                            "--child", name, str(nt), str(n)], env=env, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit(f"{name} failed with exit status {r.returncode}")
        rows.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))

    def cell(r, k):
        return "%8.3f [%.3f,%.3f]" % (r[k + "_ms"], min(r[k + "_all"]), max(r[k + "_all"]))
    lines = ["%-13s %5s %3s  %-42s %23s %23s %23s %23s %6s %6s %9s" % (
        "shape", "n", "nt", "noisy kernel", "(a) noisy ms [min,max]", "(b) disturbed ms", "(c) randn + (b) ms", "(d) fill ms", "a/b", "a/c",
        "W MB")]
    for r in rows:
        lines.append("%-13s %5d %3d  %-42s %23s %23s %23s %23s %6.3f %6.3f %9.2f" % (
            r["name"], r["n"], r["nt"], r["noisy_kernel"], cell(r, "noisy"), cell(r, "disturbed"), cell(r, "drawn"), cell(r, "fill"),
            r["noisy_ms"] / r["disturbed_ms"], r["noisy_ms"] / r["drawn_ms"], r["W_bytes"] / 1e6))
    text = "\n".join(lines)
    print(text)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "noise_time.txt"), "w") as f:
        f.write(text + "\n")
    with open(os.path.join(args.out, "noise_time.json"), "w") as f:
        json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
