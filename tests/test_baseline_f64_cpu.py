"""CPU: the double-precision baseline entry points (include/nocf.h: nocf_baseline_*_f64, nocf_baseline_max_nt) exist, check their
arguments on the host before anything is launched, and state the nt limits of both precisions; the Python layer dispatches on dtype
and refuses CPU tensors and mixed precisions.  (The library builds without a GPU; no compute call is made here.)"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import __graft_entry__ as entry
import neuraloc_amd as na
from neuraloc_amd import _lib, baseline as bl, baseline_quad as bq
import util_oracle as uo

HERE = os.path.dirname(os.path.abspath(__file__))
# the double limits the kernels must reach: the reference's baseline2D.py default nt = 50 for softcorridor, swap2, swap12 and swarm, and the
# four nt = 20 lines of log_deploy_results (softcorridor, swap2, swap12, swarm)
NT50 = ("softcorridor", "swap2", "swap12", "swarm")


@pytest.fixture(scope="module")
def L():
    entry.build()
    return _lib.lib()


def _struct(cls, kind, obstacle, n_agents):
    st = cls()
    st.kind, st.obstacle, st.n_agents, st.training = kind, obstacle, n_agents, 1
    st.r, st.alph_Q, st.alph_W, st.mass, st.grav = 0.5, 1.0, 1.0, 1.0, 9.81
    st.xtarget = 16
    return st


def _point(name, cls=_lib.NocfProb64):
    swarm = name.startswith("swarm")
    N = uo.N_AGENTS[name]
    return _struct(cls, _lib.PROB_SWARMTRAJ if swarm else _lib.PROB_CROSS2D, 0, N), (3 if swarm else 2) * N


def test_symbols_and_error_codes(L):
    for n in ("nocf_baseline_max_nt", "nocf_baseline_eval_f64", "nocf_baseline_adam_f64", "nocf_baseline_quad_eval_f64",
              "nocf_baseline_quad_lbfgs_f64", "nocf_baseline_quad_workspace_bytes_f64"):
        assert hasattr(L, n), n
    fake = C.c_void_p(16)
    quad = _struct(_lib.NocfProb64, _lib.PROB_QUADCOPTER, 0, 1)
    cross, _ = _point("softcorridor")
    ev, ad = L.nocf_baseline_eval_f64, L.nocf_baseline_adam_f64
    assert ev(C.byref(quad), 12, 1, 20, 100.0, fake, fake, fake, None, None, None, None) == -3          # NOCF_E_PROB
    assert ev(C.byref(cross), 4, 1, 20, 100.0, None, fake, fake, None, None, None, None) == -1          # NOCF_E_NULL
    assert ev(C.byref(cross), 4, 1, 0, 100.0, fake, fake, fake, None, None, None, None) == -2           # NOCF_E_SHAPE: nt
    assert ev(C.byref(cross), 4, 1, 257, 100.0, fake, fake, fake, None, None, None, None) == -2
    assert ev(C.byref(cross), 4, 0, 20, 100.0, fake, fake, fake, None, None, None, None) == -2          # B
    assert ev(C.byref(cross), 6, 1, 20, 100.0, fake, fake, fake, None, None, None, None) == -3          # d != 2 n_agents
    args = (0.1, 0.9, 0.999, 1e-8, 0, 0, fake, fake, fake, fake, fake, fake, None, None)                # niters = 0: nothing to launch
    assert ad(C.byref(quad), 12, 1, 20, 100.0, *args) == -3
    assert ad(C.byref(cross), 4, 1, 20, 100.0, *args) == 0
    assert ad(C.byref(cross), 4, 1, 20, 100.0, *(args[:4] + (-1,) + args[5:])) == -2                    # step0 < 0
    assert ad(C.byref(cross), 4, 1, 20, 100.0, *(args[:6] + (None,) + args[7:])) == -1
    qe, ql = L.nocf_baseline_quad_eval_f64, L.nocf_baseline_quad_lbfgs_f64
    assert qe(C.byref(cross), 4, 1, 20, 5000.0, fake, fake, fake, None, None, None, None) == -3
    assert qe(C.byref(quad), 24, 1, 20, 5000.0, fake, fake, fake, None, None, None, None) == -2         # single quadcopter only
    assert qe(C.byref(quad), 12, 1, 257, 5000.0, fake, fake, fake, None, None, None, None) == -2
    assert qe(C.byref(quad), 12, 1, 20, 5000.0, fake, None, fake, None, None, None, None) == -1
    la = (1.0, 0, 10, 1e-5, 1e-6, 100, fake, fake, fake, fake, fake, fake, fake)                        # max_iter = 0: nothing to launch
    need = L.nocf_baseline_quad_workspace_bytes_f64(1, 50, 100)
    assert ql(C.byref(quad), 12, 1, 50, 5000.0, *la, need, None) == 0
    assert ql(C.byref(quad), 12, 1, 50, 5000.0, *la, need - 1, None) == -4                              # NOCF_E_WORKSPACE
    assert ql(C.byref(quad), 12, 1, 50, 5000.0, *(la[:5] + (1025,) + la[6:]), need, None) == -2         # history_size
    assert ql(C.byref(cross), 4, 1, 50, 5000.0, *la, need, None) == -3


def test_quad_workspace_is_twice_the_fp32_figure(L):
    for B, nt, h in ((1, 50, 100), (1027, 20, 7), (3, 256, 1024)):
        assert L.nocf_baseline_quad_workspace_bytes_f64(B, nt, h) == 2 * L.nocf_baseline_quad_workspace_bytes(B, nt, h) > 0
    assert L.nocf_baseline_quad_workspace_bytes_f64(1, 257, 100) == 0
    assert L.nocf_baseline_quad_workspace_bytes_f64(0, 50, 100) == 0


@pytest.mark.parametrize("name", sorted(uo.BASE_ALPH))
def test_max_nt_reproduces_the_fp32_limits(L, name):
    """elem_bytes = 4: the limits tests/test_baseline_cpu.py::test_abi_nt_limits pins for the fp32 entry points"""
    st, d = _point(name, _lib.NocfProb)
    assert (L.nocf_baseline_max_nt(C.byref(st), d, 0, 4), L.nocf_baseline_max_nt(C.byref(st), d, 1, 4)) == uo.nt_limits(name)


@pytest.mark.parametrize("name", sorted(uo.BASE_ALPH))
def test_max_nt_in_double(L, name):
    """elem_bytes = 8: one limit for both entry points (the Adam moments are not in LDS), which the entry points enforce to the step; the
    reference's default nt = 50 fits for softcorridor, swap2, swap12 and swarm (d = 96), nt = 20 for every problem; the fixture's limits"""
    st32, d = _point(name, _lib.NocfProb)
    st, _ = _point(name)
    lim = L.nocf_baseline_max_nt(C.byref(st32), d, 0, 8)
    assert lim == L.nocf_baseline_max_nt(C.byref(st32), d, 1, 8)
    assert lim >= 20 and (name not in NT50 or lim >= 50)
    fake = C.c_void_p(16)
    args = (0.1, 0.9, 0.999, 1e-8, 0, 0, fake, fake, fake, fake, fake, fake, None, None)
    assert L.nocf_baseline_adam_f64(C.byref(st), d, 1, lim, 100.0, *args) == 0
    if lim < 256:
        assert L.nocf_baseline_adam_f64(C.byref(st), d, 1, lim + 1, 100.0, *args) == -2
        assert L.nocf_baseline_eval_f64(C.byref(st), d, 1, lim + 1, 100.0, fake, fake, fake, None, None, None, None) == -2
    # the bytes behind the limit: 3 nt d + d + 3 nt + 8 doubles and three partial sums per thread, within 160 KiB
    nth = uo.launch_shape(uo.N_AGENTS[name], lim)[0]
    assert (3 * lim * d + d + 3 * lim + 8 + 3 * nth) * 8 <= 160 * 1024
    meta = json.loads(str(np.load(os.path.join(HERE, "golden", "baseline_f64.npz"))["meta"]))
    if name in meta["limits"]:
        assert meta["limits"][name] == lim
    if name == "swarm":
        assert lim == 59
    if name == "swarm50":
        assert lim == 38                                     # (its fp32 Adam limit is 50)


def test_max_nt_refusals(L):
    quad = _struct(_lib.NocfProb, _lib.PROB_QUADCOPTER, 0, 1)
    cross, d = _point("softcorridor", _lib.NocfProb)
    assert L.nocf_baseline_max_nt(C.byref(quad), 12, 0, 8) == -3
    assert L.nocf_baseline_max_nt(C.byref(cross), d, 0, 2) == -2
    assert L.nocf_baseline_max_nt(None, d, 0, 8) == -1


def _prob(name):
    prob, _, _, xInit = na.initProb(name, 2, 2, var0=1.0, cvt=lambda t: t.double(), alph=[100.0, 1e4, 300.0, 0.0, 0.0, 0.0])
    return prob, xInit.reshape(-1)


def test_python_limit_helper(L):
    prob, _ = _prob("swarm50")
    assert (bl.max_nt(prob), bl.max_nt(prob, adam=True), bl.max_nt(prob, double=True), bl.max_nt(prob, True, True)) == (83, 50, 38, 38)


def test_cpu_float64_tensors_are_refused():
    prob, xInit = _prob("softcorridor")
    U = torch.zeros(20, 4, dtype=torch.float64)
    assert xInit.dtype == torch.float64
    for call in (lambda: bl.baseline_loss(xInit, U, prob, 100.0), lambda: bl.baseline_report(xInit, U, prob, 100.0),
                 lambda: bl.solve_baseline(xInit, prob, 20, niters=1), lambda: bl.solve_baseline(xInit, prob, 20, niters=1, U0=U)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    quad, xq = _prob("singlequad")
    Uq = torch.zeros(50, 4, dtype=torch.float64)
    for call in (lambda: bq.quad_baseline_loss(xq, Uq, quad, 5000.0), lambda: bq.quad_baseline_report(xq, Uq, quad, 5000.0),
                 lambda: bq.solve_baseline_quad(xq, quad, U0=Uq), lambda: bq.solve_baseline_quad(xq, quad)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_mixed_precisions_are_refused(monkeypatch):
    """the dtype of the first tensor decides; the others must match ("double-precision call" / "fp32 only").  The device check comes
    first in require_device_*, so it is taken out of the way here: nothing is launched, the dtype check raises before"""
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    prob, xInit = _prob("softcorridor")
    with pytest.raises(RuntimeError, match="double-precision call"):
        bl.baseline_loss(xInit, torch.zeros(20, 4), prob, 100.0)
    with pytest.raises(RuntimeError, match="fp32 only"):
        bl.baseline_loss(xInit.float(), torch.zeros(20, 4, dtype=torch.float64), prob, 100.0)
    with pytest.raises(RuntimeError, match="double-precision call"):
        bl.solve_baseline(xInit, prob, 20, niters=1, U0=torch.zeros(20, 4))
    quad, xq = _prob("singlequad")
    with pytest.raises(RuntimeError, match="double-precision call"):
        bq.quad_baseline_loss(xq, torch.zeros(50, 4), quad, 5000.0)
    with pytest.raises(RuntimeError, match="double-precision call"):
        bq.solve_baseline_quad(xq, quad, U0=torch.zeros(50, 4))
    with pytest.raises(RuntimeError, match="fp32 only"):
        bq.solve_baseline_quad(xq.float(), quad, U0=torch.zeros(50, 4, dtype=torch.float64))


def test_initial_guesses_follow_the_dtype():
    prob, xInit = _prob("softcorridor")
    g = torch.Generator().manual_seed(3)
    assert bl.initial_guess(xInit, prob, 20, g).dtype == torch.float64
    assert bl.initial_guess(xInit.float(), prob, 20, g).dtype == torch.float32
    a = bq.quad_initial_guess(50, generator=torch.Generator().manual_seed(5))
    b = bq.quad_initial_guess(50, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    assert a.dtype == torch.float32 and b.dtype == torch.float64 and torch.equal(a.double(), b)
    assert bq.quad_initial_guess(50, 3, torch.Generator().manual_seed(5), torch.float64).shape == (3, 50, 4)
