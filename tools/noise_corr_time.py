#!/usr/bin/env python3
"""Time the rollout under time-correlated noise (nocf_rollout_noisy_corr_f32 / nocf_rollout_record_noisy_corr_f32: DESIGN.md section 3.18)
on the MI355X at n = 1024 on one shape per kernel family -- softcorridor (lane), singlequad (one-CU), swarm50 at nt = 80 (per-tile) --
against the white noisy calls in the same run.  Legs:
  (a) nocf_rollout_noisy_corr_f32                 (b) nocf_rollout_noisy_f32
  (c) nocf_rollout_record_noisy_corr_f32          (d) nocf_rollout_record_noisy_f32
  (e) nocf_noise_fill_corr_f32 into a W that is already allocated, then nocf_rollout_disturbed_f32 on it: what (a) replaces
tools/disturb_time.py's protocol: the C entry points, with the structs, the workspace, the tables and every output buffer made once outside
the HIP event pair; the legs alternate within a repetition; median of --reps after --warmup.  A ratio is the median of the per-repetition
ratios, with the smallest and the largest repetition's as its spread.  One child process per shape (NOCF_JIT=0: the shipped library).
--lib PATH runs the children on another build of the library (NOCF_LIB_PATH); one without the correlated entries is timed on legs (b) and
(d) alone -- the parent commit's white path beside this tree's, on one machine.

    python tools/noise_corr_time.py [--reps 7] [--warmup 2] [--out profiles/noise_corr] [--lib PATH --tag parent]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from disturb_time import load, timed                        # noqa: E402

SHAPES = [("softcorridor", 50, 1024), ("singlequad", 50, 1024), ("swarm50", 80, 1024)]
LEGS = ("corr", "white", "rec_corr", "rec_white", "fill_dist")
RATIOS = (("corr", "white"), ("rec_corr", "rec_white"), ("corr", "fill_dist"))


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
    sigma, rho, seed = 0.05 * float(meta["r"]), 0.9, 0x1234567887654321
    out = {"name": name, "nt": nt, "n": n, "d": d, "m": meta["m"]}
    with torch.no_grad(), torch.cuda.device(dev):
        phi_st, keep1, ws = net._c_struct(n)
        prob_st, keep2 = prob._c_struct(dev)
        L = _lib.lib_for(net.d, net.m, net.nTh, phi_st.r, prob_st.n_agents, fwd=prob_st.kind != _lib.PROB_QUADCOPTER)
        L, f_white = noise._entry_for(L, "nocf_rollout_noisy_f32", "noise_corr_time")
        f_rec_white = noise._entry(L, "nocf_rollout_record_noisy_f32")
        f_corr, f_rec_corr, f_fill = (noise._entry(L, k) for k in ("nocf_rollout_noisy_corr_f32", "nocf_rollout_record_noisy_corr_f32",
                                                                   "nocf_noise_fill_corr_f32"))
        f_dist = disturb._entry(L)
        have = f_corr is not None
        s0, s1, r = (t.to(dev) for t in noise.noise_corr_scales(sigma, rho, nt, d)) if have else (noise.noise_scale(sigma, nt, d).to(dev), None, None)
        persample = torch.empty(n, 7, dtype=torch.float32, device=dev)
        sums = torch.empty(8, dtype=torch.float32, device=dev)
        means = torch.empty(8, dtype=torch.float32, device=dev)
        z_final = torch.empty(n, d + 4, dtype=torch.float32, device=dev)
        s_all = torch.empty(nt * 4, n, d + 1, dtype=torch.float32, device=dev)
        nact = 0 if net.m > 128 else int(L.nocf_activation_record_floats(d, net.m, net.nTh, n, nt, _STEPPERS["rk4"]))
        act = torch.empty(nact, dtype=torch.float32, device=dev) if nact else None
        W = torch.empty(nt, n, d, dtype=torch.float32, device=dev)
        rec = C.c_int32(0)
        alph_c = (C.c_float * 6)(*[float(a) for a in alph[:6]])
        head = (C.byref(phi_st), C.byref(prob_st), _lib.ptr(x))
        mid = (n, 0.0, 1.0, nt, _STEPPERS["rk4"], alph_c)
        wsp = (_lib.ptr(ws), ws.numel() * ws.element_size(), _lib.stream_ptr(dev))
        ev = mid + (_lib.ptr(z_final), _lib.ptr(persample), _lib.ptr(sums), _lib.ptr(means), None, None) + wsp
        rc = mid + (_lib.ptr(z_final), _lib.ptr(persample), _lib.ptr(sums), _lib.ptr(s_all), _lib.ptr(act), C.byref(rec)) + wsp

        def corr():
            _lib.check(f_corr(*head, _lib.ptr(s0), _lib.ptr(s1), _lib.ptr(r), seed, 0, *ev), "nocf_rollout_noisy_corr_f32")

        def white():
            _lib.check(f_white(*head, _lib.ptr(s0), seed, 0, *ev), "nocf_rollout_noisy_f32")

        def rec_corr():
            _lib.check(f_rec_corr(*head, _lib.ptr(s0), _lib.ptr(s1), _lib.ptr(r), seed, 0, *rc), "nocf_rollout_record_noisy_corr_f32")

        def rec_white():
            _lib.check(f_rec_white(*head, _lib.ptr(s0), seed, 0, *rc), "nocf_rollout_record_noisy_f32")

        def fill_dist():
            _lib.check(f_fill(_lib.ptr(W), n, nt, d, _lib.ptr(s0), _lib.ptr(s1), _lib.ptr(r), seed, 0, _lib.stream_ptr(dev)), "nocf_noise_fill_corr_f32")
            _lib.check(f_dist(*head, _lib.ptr(W), *ev), "nocf_rollout_disturbed_f32")

        legs = {"corr": corr, "white": white, "rec_corr": rec_corr, "rec_white": rec_white, "fill_dist": fill_dist}
        if not have:
            legs = {k: legs[k] for k in ("white", "rec_white")}
        white()
        out["white_kernel"] = L.nocf_last_rollout_kernel().decode()
        _lib.track_rollout_status(L, dev, "noise_corr_time")
        na.check_errors(sync=True)
        if have:
            fill_dist()
            tab, zf = persample.clone(), z_final.clone()
            corr()
            out["corr_kernel"] = L.nocf_last_rollout_kernel().decode()
            _lib.track_rollout_status(L, dev, "noise_corr_time")
            na.check_errors(sync=True)
            if not (torch.equal(tab, persample) and torch.equal(zf, z_final)):
                raise SystemExit("the correlated call and the disturbed call on the filled W disagree")
        res = timed(list(legs.values()), reps, warmup)
        for leg, (med, allms) in zip(legs, res):
            out[leg + "_ms"], out[leg + "_all"] = med, allms
        _lib.track_rollout_status(L, dev, "noise_corr_time")
    na.check_errors(sync=True)
    print("RESULT " + json.dumps(out), flush=True)


def ratio(r, a, b):
    """(median, smallest, largest) of the per-repetition ratios a / b"""
    q = [x / y for x, y in zip(r[a + "_all"], r[b + "_all"])]
    return statistics.median(q), min(q), max(q)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "noise_corr"))
    p.add_argument("--lib", default=None, help="another build of the library to run the children on (NOCF_LIB_PATH)")
    p.add_argument("--tag", default=None, help="suffix of the output files (with --lib)")
    p.add_argument("--child", nargs=3, default=None, help=argparse.SUPPRESS)
    args = p.parse_args(argv)
    if args.child:
        return child(args.child[0], int(args.child[1]), int(args.child[2]), args.reps, args.warmup)
    rows = []
    for name, nt, n in SHAPES:
        env = dict(os.environ, NOCF_JIT="0")
        if args.lib:
            env["NOCF_LIB_PATH"] = os.path.abspath(args.lib)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--warmup", str(args.warmup),
                            "--child", name, str(nt), str(n)], env=env, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit(f"{name} failed with exit status {r.returncode}")
        rows.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))

    def cell(r, k):
        return "%8.3f [%.3f,%.3f]" % (r[k + "_ms"], min(r[k + "_all"]), max(r[k + "_all"])) if k + "_ms" in r else "-".rjust(23)

    def rcell(r, a, b):
        return "%6.3f [%.3f,%.3f]" % ratio(r, a, b) if a + "_ms" in r and b + "_ms" in r else "-".rjust(20)
    lines = ["%-13s %5s %3s  %-46s %23s %23s %23s %23s %23s  %20s %20s %20s" % (
        "shape", "n", "nt", "kernel", "(a) corr ms [min,max]", "(b) white ms", "(c) record corr ms", "(d) record white ms",
        "(e) fill + disturbed ms", "a/b [min,max]", "c/d [min,max]", "a/e [min,max]")]
    for r in rows:
        lines.append("%-13s %5d %3d  %-46s %23s %23s %23s %23s %23s  %20s %20s %20s" % (
            r["name"], r["n"], r["nt"], r.get("corr_kernel", r["white_kernel"]), cell(r, "corr"), cell(r, "white"), cell(r, "rec_corr"),
            cell(r, "rec_white"), cell(r, "fill_dist"), *[rcell(r, a, b) for a, b in RATIOS]))
    text = "\n".join(lines)
    print(text)
    os.makedirs(args.out, exist_ok=True)
    stem = "noise_corr_time" + ("_" + args.tag if args.tag else "")
    with open(os.path.join(args.out, stem + ".txt"), "w") as f:
        f.write(text + "\n")
    with open(os.path.join(args.out, stem + ".json"), "w") as f:
        json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
