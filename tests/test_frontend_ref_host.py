"""The float64 reference and the bounds of tests/frontend_cases.py, checked on the CPU: that the bounds are not wrong (the same
statement in plain f32 stays inside them), not vacuous (ten nearly right statements leave them), and that every case has the
condition it was chosen for.  Prints, per case, the f32 statement's worst err / bound and, per mutant and case, the largest
share of elements over the bound among the gated tensors (the smaller of the two dtypes).  No GPU needed."""
import os
import re

import pytest
import torch

import attn_cases as A
import frontend_cases as FC
import gemm_cases as G

BF, F32 = FC.BF, FC.F32
ALL_CASES = ([("fused",) + c for c in FC.FUSED_CASES] + [("general",) + c for c in FC.GENERAL_CASES] + [("finite",) + FC.FINITE_CASE])
LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "small-object-detection-transformers_amd",
                   "libsodt_hip.so")


def _gated(su):
    if su["kind"] == "fused":
        return ("out", "dw", "db", "dgamma", "dbeta")
    if su["kind"] == "finite":
        return ("out", "de", "dgamma", "dbeta")
    return ("e", "out", "de", "dgamma", "dbeta", "dw", "db")


@pytest.mark.parametrize("key", ALL_CASES, ids=FC.case_id)
def test_f32_statement_sits_within_the_bound(key):
    su = FC.setup(key[0], key[1:])
    ratios = {}
    for dt in (F32, BF):
        dout, ref = FC.dout_and_reference(su, dt)
        bnd = FC.bounds_for(su, dt, FC.tightest_depth(su, dt))
        f32 = FC.reference(su["x4"], su["w"], su["b"], su["gamma"], su["beta"], su["ws"], su["shift"], dout, dtype=torch.float32,
                           e_given=su["e_given"])
        for name in _gated(su):
            got = f32[name]
            if name == "out" and dt == BF:
                got = got.to(BF)
            ratios[(name, dt)] = FC.worst(got, ref[name], bnd[name])
    print(f"\n{FC.case_id(key)}: f32 statement err / bound  " + "  ".join(
        f"{n}:{ratios[(n, F32)]:.3f}/{ratios[(n, BF)]:.3f}" for n in _gated(su)))
    assert max(ratios.values()) <= 1.0, ratios


def test_statement_without_a_mutant_is_the_reference():
    for key in (("fused",) + FC.STRIDE_CASE, ("general", 2, 32, 96, 8, 3), ("general", 1, 32, 32, 8, 7), ("finite",) + FC.FINITE_CASE):
        su = FC.setup(key[0], key[1:])
        dout, ref = FC.dout_and_reference(su, F32)
        st = FC.statement(su["x4"], su["w"], su["b"], su["gamma"], su["beta"], su["ws"], su["shift"], dout, None, e_given=su["e_given"])
        for name in _gated(su):
            err = float((st[name] - ref[name].reshape(st[name].shape)).abs().max())
            assert err <= 1e-11 * max(1.0, float(ref[name].abs().max())), (key, name, err)


@pytest.mark.parametrize("mutant", sorted(FC.MUTANTS), ids=lambda m: f"m{m}")
def test_mutated_reference_exceeds_the_bound(mutant):
    for key in FC.MUTANT_CASES[mutant]:
        su = FC.setup(key[0], key[1:])
        share = {}
        for dt in (F32, BF):
            dout, ref = FC.dout_and_reference(su, dt)
            depth = FC.tightest_depth(su, dt)
            if su["kind"] == "fused":                       # the loosest route of the case: the mutant must leave that bound too
                dd = max(FC.fused_bwd_route(dt, su["M"], wsf)["depth"] for wsf in (None, FC.WS_FLOATS))
                depth = dict(gamma=dd, de=3, embed=dd)
            bnd = FC.bounds_for(su, dt, depth)
            mu = FC.statement(su["x4"], su["w"], su["b"], su["gamma"], su["beta"], su["ws"], su["shift"], dout, mutant,
                              e_given=su["e_given"])
            share[dt] = {n: FC.share_over(mu[n], ref[n], bnd[n]) for n in _gated(su)}
        both = {n: min(share[F32][n], share[BF][n]) for n in _gated(su)}
        best = max(both, key=both.get)
        print(f"\nmutant {mutant} ({FC.MUTANTS[mutant]}) at {FC.case_id(key)}: {100 * both[best]:.1f} % of {best} over the bound")
        assert both[best] >= 0.01, (mutant, key, both)


def test_case_conditions_hold_in_the_reference():
    # nine mask regions wherever the grid has more than one window per axis
    for c in FC.GENERAL_CASES + [FC.FINITE_CASE]:
        B, H, W, ws, shift = c
        if shift == 0:
            continue
        g = A.Geo(B, H // 4, W // 4, FC.CE, FC.NH, ws, shift, "cpu")
        want = (3 if H // 4 > ws else 2) * (3 if W // 4 > ws else 2)     # (one window along an axis: its first band is empty)
        assert torch.unique(g.region).numel() == want, (c, torch.unique(g.region))
    assert any(c[1] // 4 > c[3] and c[4] > 0 for c in FC.GENERAL_CASES)
    # peaked softmax: the median over queries of the largest probability is at least 3 / N
    for c in FC.GENERAL_CASES:
        su = FC.setup("general", c)
        _, ref = FC.dout_and_reference(su, F32)
        g, pm = FC.probabilities(ref["e"], *c)
        med = float(torch.cat([P.max(-1).values.flatten() for P, _ in pm]).median())
        print(f"\n{FC.case_id(c)}: median largest probability {med:.3f}, uniform {1 / g.N:.3f}")
        assert med >= 3.0 / g.N, (c, med)
    # the finite-mask case: masked keys carry real mass
    su = FC.setup("finite", FC.FINITE_CASE)
    _, ref = FC.dout_and_reference(su, F32)
    g, pm = FC.probabilities(ref["e"], *FC.FINITE_CASE)
    mass = torch.cat([(P * m.double()).sum(-1).flatten() for P, m in pm])
    share = float((mass >= 0.1).double().mean())
    print(f"\nfinite mask: {100 * share:.1f} % of the (query, head, pair) rows carry masked mass >= 0.1; largest {float(mass.max()):.3f}")
    assert share >= 0.1


def test_route_table():
    """fused_bwd_route at the case shapes: the nblk > 64 switch, the 512 / 256 caps, the trips and the reduce grid."""
    r = FC.fused_bwd_route(F32, 64 * 64, FC.WS_FLOATS)
    assert (r["two_stage"], r["grid"], r["trips"]) == (False, 64, 1)
    r = FC.fused_bwd_route(F32, 64 * 65, FC.WS_FLOATS)
    assert (r["two_stage"], r["grid"], r["trips"], r["reduce_grid"]) == (True, 65, 1, (57, 3))
    assert not FC.fused_bwd_route(F32, 64 * 65, FC.WS_FLOATS - 1)["two_stage"]
    r = FC.fused_bwd_route(BF, 33075, FC.WS_FLOATS)
    assert (r["nblk"], r["grid"], r["trips"], r["reduce_grid"]) == (517, 512, 2, (57, 16))
    assert r["kernels"] == ["frontend_bwd_kernel<bf16, true>", "frontend_bwd_reduce_kernel"]
    r = FC.fused_bwd_route(BF, 33075, None)
    assert (r["grid"], r["trips"], r["kernels"]) == (256, 3, ["frontend_bwd_kernel<bf16, false>"])
    assert FC.FE_PART % 64 == 0


def test_route_names_exist_and_demangle():
    """Every kernel name of the route table is a kernel of the built library, and torch's demangler (the profiler's names)
    gives the same name as the mangled symbol."""
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} missing: run build() first")
    with open(LIB, "rb") as f:
        blob = f.read()
    mangled = sorted({m.decode() for m in re.findall(rb"_ZN12_GLOBAL__N_1\d+(?:frontend|patch_embed4|cross_attn_ln)_\w+", blob)})
    names = set()
    for m in mangled:
        want = G.canonical_kernel(m)
        assert "unreadable" not in want, (m, want)
        assert FC.canonical(torch._C._demangle(m)) == want, (m, torch._C._demangle(m))
        names.add(want)
    missing = sorted(set(FC.ALL_ROUTE_NAMES) - names)
    assert not missing, f"route table names no kernel of the library: {missing}; it has {sorted(names)}"
