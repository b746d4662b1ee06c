"""The launch plan of sfx_block_mlp at C = 128 and 256 (csrc/mlp.hip plan_hs / tail_split): point counts around one
round of whole 128-point tiles -- `slots` workgroups, one per CU at C = 256, two at C = 128.  The plan picks whole
or hidden-split tiles per launch and splits the tail of the last round over the hidden chunks where the pieces fit
one round.  Every case meets the fp64 bar of tests/test_gpu_mlp.py (_check_fp64, restated here: relative L2 <=
max(2e-6, 2x torch's fp32 error), each row within 4x its fp32 error + 1e-6), returns the row exponents of
sfx_subm_rowexp, is bitwise reproducible, reports through sfx_block_mlp_last_plan a plan that follows tail_split's
rule and covers the rows, and computes the rows of its unsplit main part exactly as a call on those rows alone does.

Which kind is expected: on the 256 CUs the plan's constants were fitted on, the kind and split of every case are
asserted from the cost model's own prices (PLAN_256_CUS; one near tie, quarter_plus1 at C = 256, left out).  On any
device, where one round of whole tiles holds every point but at most one workgroup's worth (plus1, exact, minus5)
whole tiles are asserted (one round against two: 165 vs 178 us at C = 256, 78 vs 88 at C = 128, DESIGN section
20).  Whatever kind runs is held to tail_split's rule for that kind.  The whole-tile launch whose tail is more than
half a round (the plan runs that shape hidden-split at C = 256) has a forced case of its own.

The MLP acts on each row alone, so one input and one fp64 / fp32 reference per C (at the largest M) serve every
case through their leading rows."""
import functools

import pytest
import torch
import torch.nn.functional as F

from splatformer_amd import ptv3_ops as ops

pytestmark = pytest.mark.gpu

PTS = 128  # points per whole-tile workgroup
WHOLE, HS = 0, 1


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _slots(C):
    return _cus() if C == 256 else 2 * _cus()


# name -> M(slots); the largest is "half_plus"
CASES = {
    "plus1": lambda s: s * PTS + 1,                            # one tail workgroup: the widest split
    "quarter": lambda s: s * PTS + PTS * (s // 4),             # a tail that fits one split round exactly
    "quarter_plus1": lambda s: s * PTS + PTS * (s // 4) + 1,   # one workgroup more
    "half_plus": lambda s: s * PTS + PTS * (s // 2 + 1),       # more than half a round: whole tiles do not split it
    "exact": lambda s: s * PTS,                                # no tail
    "minus5": lambda s: s * PTS - 5,                           # one round only, ragged
}
WHOLE_FOR_SURE = ("plus1", "exact", "minus5")
# (kind, split) the cost model of csrc/mlp.hip picks on 256 CUs, from its constants (prices in us, whole vs hidden
# split).  C = 256: plus1 189.9 vs 203.4, quarter 209.9 vs 227.8, half_plus 310 vs 281.4 (three hidden-split rounds
# + a 2-workgroup tail beat two whole rounds), exact / minus5 165 vs 174; quarter_plus1 is a near tie (249.75 vs
# 252) and is held to the rule of whichever kind runs.  C = 128: plus1 91.1 vs 110.6, quarter 116.9 vs 128.2,
# quarter_plus1 115 vs 125, half_plus 140 vs 147.6, exact / minus5 77.5 vs 88.
PLAN_256_CUS = {
    256: {"plus1": (WHOLE, 8), "quarter": (WHOLE, 4), "quarter_plus1": None, "half_plus": (HS, 4),
          "exact": (WHOLE, 1), "minus5": (WHOLE, 1)},
    128: {"plus1": (WHOLE, 8), "quarter": (WHOLE, 2), "quarter_plus1": (WHOLE, 1), "half_plus": (WHOLE, 1),
          "exact": (WHOLE, 1), "minus5": (WHOLE, 1)},
}


def _mods(C):
    g = torch.Generator().manual_seed(11 * C)
    ln = torch.nn.LayerNorm(C)
    fc1, fc2 = torch.nn.Linear(C, 4 * C), torch.nn.Linear(4 * C, C)
    with torch.no_grad():
        ln.weight.copy_(torch.rand(C, generator=g) + 0.5)
        ln.bias.copy_(torch.randn(C, generator=g) * 0.1)
        for lin in (fc1, fc2):
            lin.weight.copy_(torch.randn(lin.weight.shape, generator=g) / lin.weight.shape[1] ** 0.5)
            lin.bias.copy_(torch.randn(lin.bias.shape, generator=g) * 0.1)
    return ln, fc1, fc2


@torch.no_grad()
def _ref(x, ln, fc1, fc2, dtype):
    x = x.to(dtype)
    h = F.layer_norm(x, (x.shape[1],), ln.weight.to(dtype), ln.bias.to(dtype), ln.eps)
    m = F.gelu(F.linear(h, fc1.weight.to(dtype), fc1.bias.to(dtype)))
    return x + F.linear(m, fc2.weight.to(dtype), fc2.bias.to(dtype))


@functools.lru_cache(maxsize=None)
def _problem(C):
    """(x, fp64 branch, fp32 branch, device modules, device x) at the largest M of CASES; never modified."""
    mmax = max(f(_slots(C)) for f in CASES.values())
    ln, fc1, fc2 = _mods(C)
    x = torch.randn(mmax, C, generator=torch.Generator().manual_seed(C)) * 2.0
    x[::3] *= 1e3   # rows of very different magnitudes (LayerNorm normalises them; the residual keeps them)
    x[1::5] *= 1e-3
    br = _ref(x, ln, fc1, fc2, torch.float64) - x.double()
    b32 = _ref(x, ln, fc1, fc2, torch.float32).double() - x.double()
    dev = torch.device("cuda:0")
    mods = [m.to(dev) for m in _mods(C)]
    return x, br, b32, mods, x.to(dev)


def _assert_fp64_bar(y, x, br, b32):
    """_check_fp64's bar of tests/test_gpu_mlp.py on the branch Y - X."""
    y = y.cpu().double()
    assert torch.isfinite(y).all()
    bh = y - x.double()
    rel = lambda a, b: float((a - b).norm() / b.norm().clamp_min(1e-30))
    assert rel(bh, br) <= max(2e-6, 2 * rel(b32, br)), (rel(bh, br), rel(b32, br))
    e_row = (bh - br).norm(dim=1) / br.norm(dim=1).clamp_min(1e-30)
    e32 = (b32 - br).norm(dim=1) / br.norm(dim=1).clamp_min(1e-30)
    assert bool((e_row <= 4 * e32 + 1e-6).all()), float((e_row - 4 * e32).max())


def _expected(kind, C, M):
    """The plan of a launch of `kind` tiles by tail_split's rule: after at least one whole round, the largest factor
    that divides the C / 16 hidden chunks and whose pieces fit -- whole tiles 8 / 4 / 2, one piece per CU;
    hidden-split tiles 4 / 3 / 2, a round of `slots` pieces."""
    slots = _slots(C)
    pts = PTS if kind == WHOLE else PTS // 2
    wgs = -(-M // pts)
    full, r = wgs // slots * slots, wgs % slots
    plan = {"kind": kind, "split": 1, "main_wgs": wgs, "tail_wgs": 0, "pts": pts}
    if full and r:
        for s in ((8, 4, 2) if kind == WHOLE else (4, 3, 2)):
            if (C // 16) % s == 0 and s * r <= (_cus() if kind == WHOLE else slots):
                plan.update(split=s, main_wgs=full, tail_wgs=r)
                break
    return plan


def _run(C, M, device):
    x, br, b32, mods, xd = _problem(C)
    e = torch.full((M,), -999, device=device, dtype=torch.int32)
    y = ops.block_mlp(xd[:M], *mods, rowexp=e)
    plan = ops.block_mlp_last_plan()
    print(f"C={C} M={M}: plan {plan}")
    _assert_fp64_bar(y, x[:M], br[:M], b32[:M])
    assert torch.equal(e.cpu(), ops.subm_rowexp(y).cpu())
    e2 = torch.full((M,), -999, device=device, dtype=torch.int32)
    y2 = ops.block_mlp(xd[:M], *mods, rowexp=e2)
    assert torch.equal(y, y2) and torch.equal(e, e2)
    return y, plan


def _check_plan_and_main_part(monkeypatch, device, C, M, y, plan):
    kind = plan["kind"]
    assert kind in (WHOLE, HS) and plan == _expected(kind, C, M), (plan, _expected(kind, C, M))
    main, tail, pts = plan["main_wgs"], plan["tail_wgs"], plan["pts"]
    if plan["split"] == 1:
        assert (main - 1) * pts < M <= main * pts and tail == 0
        return
    # row coverage: the main launch's whole rounds, then the tail's workgroups up to M
    assert main % _slots(C) == 0 and main * pts < M <= (main + tail) * pts
    # the unsplit main part equals a call of the same tile kind on its rows alone, bit for bit
    monkeypatch.setenv("SFX_MLP_HS", str(kind))
    _, _, _, mods, xd = _problem(C)
    ym = ops.block_mlp(xd[:main * pts], *mods)
    assert ops.block_mlp_last_plan() == {"kind": kind, "split": 1, "main_wgs": main, "tail_wgs": 0, "pts": pts}
    assert torch.equal(y[:main * pts], ym)


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("C", [128, 256])
def test_plan_and_tail_split(device, monkeypatch, C, case):
    for v in ("SFX_MLP_HS", "SFX_MLP_WAVES"):
        monkeypatch.delenv(v, raising=False)
    M = CASES[case](_slots(C))
    y, plan = _run(C, M, device)
    if case in WHOLE_FOR_SURE:
        assert plan["kind"] == WHOLE, plan
    if _cus() == 256:  # the MI355X the plan's constants were fitted on: the kind and split of every case
        want = PLAN_256_CUS[C][case]
        if want is not None:
            assert (plan["kind"], plan["split"]) == want, (plan, want)
    _check_plan_and_main_part(monkeypatch, device, C, M, y, plan)


def test_whole_tiles_tail_over_half_a_round_is_not_split(device, monkeypatch):
    """The half_plus shape at C = 256 under forced whole tiles (the plan runs it hidden-split): one whole round, then
    a round more than half full in the same unsplit launch."""
    monkeypatch.delenv("SFX_MLP_WAVES", raising=False)
    monkeypatch.setenv("SFX_MLP_HS", "0")
    M = CASES["half_plus"](_slots(256))
    y, plan = _run(256, M, device)
    assert plan == {"kind": WHOLE, "split": 1, "main_wgs": -(-M // PTS), "tail_wgs": 0, "pts": PTS}, plan
    _check_plan_and_main_part(monkeypatch, device, 256, M, y, plan)


@pytest.mark.parametrize("hs", [HS, WHOLE])
@pytest.mark.parametrize("C", [128, 256])
def test_forced_tile_kinds_still_run(device, monkeypatch, C, hs):
    """SFX_MLP_HS=1 / 0 force hidden-split / whole tiles whatever the plan would pick; both split their tails."""
    monkeypatch.delenv("SFX_MLP_WAVES", raising=False)
    monkeypatch.setenv("SFX_MLP_HS", str(hs))
    M = CASES["quarter"](_slots(C))
    y, plan = _run(C, M, device)
    assert plan["kind"] == hs and plan["split"] > 1, plan
    _check_plan_and_main_part(monkeypatch, device, C, M, y, plan)
