"""The split-role forward at the smallest batch that reaches each of its instantiations (neuraloc_amd/csrc/nocf_duo.hip: group geometry x
tiles per group x the one-tile modes), two steps of rk4, evaluation and training mode of the problem.  The serial sections of both roles form
their lane masks and wave-uniform tests where they use them (DU_HERE_V): every instantiation compiles them differently, so each is run here.

Per case: two runs are bit-identical, no exchange timed out, and the per-sample table agrees with the per-tile kernel (NOCF_DUO=0) under the
per-row tolerance and the fp64 adjudication of test_duo_gpu.py (its helpers, imported).  The change this file came with leaves every bit of the
forward's results as it was, so no case may adjudicate more rows than the kernels before it disagreed on: measured on that build at these
shapes, that is NO row in any case (at two steps nothing has been amplified yet) -- the number adjudicated is printed and must be 0."""
import pytest
import torch

from oracle import ocflow_oracle as orc
from conftest import load_golden
from util_hip import closed_form_normal, make_net, make_oracle, make_prob, synth_state_dict
import neuraloc_amd as na
from test_duo_gpu import DEV, _explained, _kernel, _table

pytestmark = pytest.mark.gpu
NT = 2

# (case, hidden width, rows, NOCF_DUO_G or None): rollout_duo_kernel<3, false, false, G, KBM, MODE>
CASES = [
    ("default geometry, two tiles per group, ragged last tile <8,32,0>", 512, 513, None),
    ("32 one-tile groups <8,32,1>", 512, 512, None),
    ("other one-tile launches of the default geometry <8,32,2>", 512, 17, "8"),
    ("fine geometry, two groups <16,32,0>", 512, 17, None),
    ("fine geometry, sixteen groups <16,32,0>", 512, 256, None),
    ("256-wide network, one tile per group <4,16,1>", 256, 17, None),
    ("256-wide network, two tiles per group <4,16,0>", 256, 1025, None),
]
ADJUDICATED_BEFORE = 0          # rows on which the split-role and the per-tile kernel disagreed before this change, every case (see above)


@pytest.fixture(scope="module")
def golden():
    return load_golden("swarm50")


@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("case,width,n,force_g", CASES, ids=[c[0].split(" <")[1][:-1] + f"-n{c[2]}" for c in CASES])
def test_every_instantiation_is_deterministic_and_matches_the_tile_kernel(case, width, n, force_g, training, golden, monkeypatch):
    g, m = golden, golden.meta
    for k in ("NOCF_DUO_G", "NOCF_DUO_MAP", "NOCF_DUO_FAST"):
        monkeypatch.delenv(k, raising=False)
    if force_g:
        monkeypatch.setenv("NOCF_DUO_G", force_g)
    if width == 512:
        sd = g.state_dict()
        net = make_net(g, DEV)
    else:
        sd = synth_state_dict(2, width, m["d"], seed=2)
        net = na.Phi(nTh=2, m=width, d=m["d"], alph=m["alph"])
        net.load_state_dict(sd)
        net = net.to(DEV).eval()
    prob = make_prob(g, DEV, training=training)
    x = (g.t("xInit") + m["var0"] * closed_form_normal(n, m["d"], 3)).contiguous()
    monkeypatch.setenv("NOCF_DUO", "1")
    duo = _table(x.to(DEV), net, prob, [0.0, 1.0], NT, "rk4", m["alph"])
    assert _kernel() == "rollout_duo_kernel"
    again = _table(x.to(DEV), net, prob, [0.0, 1.0], NT, "rk4", m["alph"])
    assert torch.equal(duo, again), f"{case}: not run-to-run deterministic"
    assert not torch.isnan(duo).any()
    na.check_errors(sync=True)
    monkeypatch.setenv("NOCF_DUO", "0")
    tile = _table(x.to(DEV), net, prob, [0.0, 1.0], NT, "rk4", m["alph"])
    assert _kernel().startswith("rollout_kernel")
    off = ((duo.double() - tile.double()).abs() > 1e-3 + 1e-3 * tile.double().abs()).any(dim=1)
    rows = torch.nonzero(off).flatten()
    print(f"[duo_streams] {case}, n = {n}, {'train' if training else 'eval'}: {len(rows)} row(s) adjudicated in fp64")
    assert len(rows) <= ADJUDICATED_BEFORE, f"{case}: rows {rows.tolist()} differ from the per-tile kernel; none did before"
    if len(rows):
        P64 = orc.PhiParams.from_state_dict(sd, dtype=torch.float64)
        S64 = make_oracle(g, training)[1].to(torch.float64)
        ok, _, _ = _explained(x[rows], duo[rows], tile[rows], P64, S64, NT, m["alph"])
        assert bool(ok.all()), f"{case}: rows {rows[~ok].tolist()} differ between the kernels without a reason in the fp64 oracle"
    keep = ~off
    for j in range(7):
        a, b = duo[keep, j].double().mean().item(), tile[keep, j].double().mean().item()
        assert abs(a - b) <= 1e-4 * abs(b) + 1e-6, f"{case} column {j}: mean {a} vs {b}"
    na.check_errors(sync=True)
