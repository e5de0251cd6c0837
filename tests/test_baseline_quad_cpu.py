"""CPU: the quadcopter baseline's restatement against its fixture, the fixture itself, argument and shape errors of the Python layer,
the C ABI's error codes (including one past each limit, refused before any launch) and the driver's flags."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import __graft_entry__ as entry
import neuraloc_amd as na
from neuraloc_amd import _lib
import util_quad as uq

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return uq.load_golden()


@pytest.fixture(scope="module")
def L():
    entry.build()
    return _lib.lib()


def quad(mass=1.0, grav=9.81, agents=1):
    return na.Quadcopter(torch.tensor(uq.XTARGET * agents), alph_Q=0.0, alph_W=0.0, mass=mass, grav=grav)


def test_fixture_is_small_and_complete(gold):
    assert os.path.getsize(uq.GOLDEN) < 2 * 1024 * 1024
    assert gold["ckpt/ctrls"].shape == (50, 4) and gold["ckpt/traj"].shape == (12, 51)
    assert gold["ckpt/loss"].shape == (1,) and gold["ckpt/L"].shape == (1,) and gold["ckpt/G"].shape == ()
    for nt in uq.NT_LIST:
        assert gold[f"obj/nt{nt}/U"].shape == (3, nt, 4) and gold[f"obj/nt{nt}/g64"].shape == (3, nt, 4)
        assert gold[f"obj/nt{nt}/z0"].shape == (3, 12) and gold[f"obj/nt{nt}/J64"].shape == (3,)
    assert gold["solve/z0"].shape == (4, 12) and gold["solve/U0"].shape == (4, 50, 4)
    for k in ("loss64", "n_iter64", "evals64"):
        assert gold["solve/" + k].shape == (4,)
    assert gold["lock/z0"].shape[0] >= 2 and gold["lock/U0"].shape[1:] == (50, 4)
    np.testing.assert_array_equal(gold["xInit"], np.array(uq.XINIT, dtype=np.float32))
    np.testing.assert_array_equal(gold["xtarget"], np.array(uq.XTARGET, dtype=np.float32))


def test_restatement_reproduces_the_checkpoint(gold):
    """the shipped controls re-evaluated from xInit give the shipped loss, L, G and trajectory"""
    rows, traj = uq.report(torch.tensor(uq.XINIT)[None], torch.from_numpy(gold["ckpt/ctrls"])[None], dtype=torch.float32)
    want = [float(gold["ckpt/loss"][0]), float(gold["ckpt/L"][0]), float(gold["ckpt/G"])]
    for got, w in zip(rows[0].tolist(), want):
        assert abs(got - w) <= 1e-6 * abs(w)
    assert float((traj[0] - torch.from_numpy(gold["ckpt/traj"])).abs().max()) <= 1e-6


@pytest.mark.parametrize("nt", uq.NT_LIST)
def test_restatement_reproduces_the_objective(gold, nt):
    z0, U = gold[f"obj/nt{nt}/z0"], gold[f"obj/nt{nt}/U"]
    J64, g64 = uq.objective(z0, U, grad=True)
    np.testing.assert_allclose(J64.numpy(), gold[f"obj/nt{nt}/J64"], rtol=1e-12)
    np.testing.assert_allclose(g64.numpy(), gold[f"obj/nt{nt}/g64"], rtol=1e-9, atol=1e-9 * np.abs(gold[f"obj/nt{nt}/g64"]).max())
    J32, g32 = uq.objective(z0, U, dtype=torch.float32, grad=True)
    assert uq.compare(J32, J64, gold[f"obj/nt{nt}/J32"], factor=8.0)[0]
    assert uq.compare(g32, g64, gold[f"obj/nt{nt}/g32"], factor=8.0)[0]


def test_comparator_rejects_a_wrong_objective(gold):
    """a restatement with the gradient of the previous step's state (an off-by-one adjoint) fails the rule"""
    z0, U = gold["obj/nt20/z0"], gold["obj/nt20/U"]
    J64, g64 = uq.objective(z0, U, grad=True)
    _, g32 = uq.objective(z0, U, dtype=torch.float32, grad=True)
    wrong = g64.clone()
    wrong[:, 1:] = g64[:, :-1]
    assert not uq.compare(wrong, g64, g32)[0]
    assert not uq.compare(J64 * (1 + 1e-4), J64, uq.objective(z0, U, dtype=torch.float32))[0]


def test_argument_errors():
    z0 = torch.tensor(uq.XINIT)
    U = torch.zeros(50, 4)
    with pytest.raises(TypeError):
        na.quad_baseline_loss(z0, U, object(), 5000.)
    with pytest.raises(TypeError):
        na.solve_baseline_quad(z0, na.Cross2D(torch.zeros(4)), nt=10)
    with pytest.raises(ValueError, match="single quadcopter"):
        na.quad_baseline_loss(torch.zeros(24), U, quad(agents=2), 5000.)
    with pytest.raises(ValueError):
        na.quad_baseline_loss(torch.zeros(11), U, quad(), 5000.)
    with pytest.raises(ValueError):
        na.quad_baseline_loss(z0, torch.zeros(50, 3), quad(), 5000.)
    with pytest.raises(ValueError):
        na.quad_baseline_loss(torch.zeros(3, 12), torch.zeros(2, 50, 4), quad(), 5000.)
    with pytest.raises(ValueError):
        na.quad_baseline_loss(z0, torch.zeros(257, 4), quad(), 5000.)
    with pytest.raises(ValueError, match="strong_wolfe"):
        na.solve_baseline_quad(z0, quad(), nt=10, line_search_fn=None)
    with pytest.raises(ValueError):
        na.solve_baseline_quad(z0, quad(), nt=10, history_size=0)
    with pytest.raises(ValueError):
        na.solve_baseline_quad(z0, quad(), nt=10, history_size=1025)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        na.quad_baseline_loss(z0, U, quad(), 5000.)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        na.solve_baseline_quad(z0, quad(), nt=10)
    # the point-agent baseline still refuses the quadcopter with a ValueError that names it
    with pytest.raises(ValueError, match="quadcopter"):
        na.baseline_loss(z0, torch.zeros(50, 12), quad(), 5000.)


def test_initial_guess_is_the_references_draw():
    g = torch.Generator().manual_seed(3)
    U = na.quad_initial_guess(50, None, g)
    g = torch.Generator().manual_seed(3)
    assert torch.equal(U, 1.e-2 * torch.randn(50, 4, generator=g))
    assert na.quad_initial_guess(7, 3, g).shape == (3, 7, 4)


def _call_eval(L, st, d=12, B=1, nt=50, z0=1, U=1, loss=1):
    p = C.c_void_p(0x1000)
    nz = lambda f: p if f else None
    return L.nocf_baseline_quad_eval_f32(C.byref(st) if st is not None else None, d, B, nt, 5000., nz(z0), nz(U), nz(loss),
                                         None, None, None, None)


def _call_lbfgs(L, st, d=12, B=1, nt=50, hist=100, max_iter=0, max_eval=10000, ws_bytes=None, ws=1):
    p = C.c_void_p(0x1000)
    if ws_bytes is None:
        ws_bytes = L.nocf_baseline_quad_workspace_bytes(max(B, 1), max(nt, 1), max(hist, 1))
    return L.nocf_baseline_quad_lbfgs_f32(C.byref(st), d, B, nt, 5000., 1., max_iter, max_eval, 1e-5, 1e-6, hist, p, p, p, p, p, p,
                                          p if ws else None, ws_bytes, None)


def test_abi_error_codes(L):
    """every refusal returns before a launch (the pointers are never dereferenced: max_iter = 0 or an error)"""
    st, keep = quad()._c_struct("cpu")
    assert _call_eval(L, None) == -1
    assert _call_eval(L, st, z0=0) == -1
    cs, keep2 = na.Cross2D(torch.zeros(4))._c_struct("cpu")
    assert _call_eval(L, cs, d=4) == -3
    assert _call_lbfgs(L, cs, d=4) == -3
    assert _call_eval(L, st, d=24) == -2
    st2, keep3 = quad(agents=2)._c_struct("cpu")
    assert _call_eval(L, st2, d=24) == -2
    assert _call_eval(L, st, nt=0) == -2
    assert _call_eval(L, st, B=0) == -2
    # the limits: the last accepted value passes the checks (max_iter = 0 returns before the launch), one past it is refused
    assert _call_lbfgs(L, st, nt=256) == 0
    assert _call_lbfgs(L, st, nt=257, ws_bytes=1 << 40) == -2
    assert _call_eval(L, st, nt=257) == -2
    assert _call_lbfgs(L, st, hist=1024) == 0
    assert _call_lbfgs(L, st, hist=1025, ws_bytes=1 << 40) == -2
    assert _call_lbfgs(L, st, hist=0, ws_bytes=1 << 40) == -2
    assert _call_lbfgs(L, st, max_eval=0) == -2
    assert _call_lbfgs(L, st, max_iter=-1) == -2
    assert _call_lbfgs(L, st, ws=0) == -1
    need = L.nocf_baseline_quad_workspace_bytes(1, 50, 100)
    assert need == 2 * 100 * 200 * 4
    assert _call_lbfgs(L, st, ws_bytes=need - 1) == -4
    assert L.nocf_baseline_quad_workspace_bytes(1, 257, 100) == 0
    assert L.nocf_baseline_quad_workspace_bytes(1, 50, 1025) == 0
    assert L.nocf_baseline_quad_workspace_bytes(0, 50, 100) == 0


def test_driver_flags():
    sys.path.insert(0, REPO)
    import baselineQuad
    a = baselineQuad.parse_args([])
    assert (a.data, a.nt, a.alph, a.niters, a.gpu, a.prec, a.save) == ("singlequad", 50, [5000.0, 0.0, 0.0], 600, 0, "single",
                                                                        "experiments/oc/baseline")
    assert (a.seed, a.nx, a.var0, a.max_iter) == (0, 1, 1.0, 16000)
    a = baselineQuad.parse_args(["--nx", "8", "--max-iter", "20", "--alph", "100,0,0", "--seed", "3"])
    assert (a.nx, a.max_iter, a.alph, a.seed) == (8, 20, [100.0, 0.0, 0.0], 3)
    with pytest.raises(SystemExit):
        baselineQuad.parse_args(["--data", "softcorridor"])
    with pytest.raises(SystemExit):
        baselineQuad.parse_args(["--nx", "0"])


def test_driver_refuses_double(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(REPO, "baselineQuad.py"), "--prec", "double", "--save", str(tmp_path)],
                       capture_output=True, text=True, cwd=REPO, timeout=120)
    assert r.returncode != 0 and "double" in r.stderr
    assert not list(tmp_path.iterdir())
