"""The conditions tests/test_head_routes_gpu.py puts on its own float64 references, checked on the CPU (no GPU needed): for every
case and every gated tensor |T_A| > 0 and 0 < e_emul(T) <= 5e-2 (tests/head_cases.py), so that the bf16 gate 3 e_emul + 1e-5 is
neither vacuous nor loose; that the oracle's store hook changes nothing when it is absent or the identity; and that the case
table is the head headgraph.parse_head reads off the three head yamls."""
import importlib
import os

import pytest
import torch

import block_cases as BC
import head_cases as HC

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), HC.PKG, "libsodt_hip.so")
REF_CASES = list({(c.kind, c.head, c.row, c.B, c.H, c.W, c.dtype, c.training): c for c in HC.CASES}.values())


def _identity(t, name):
    return t


@pytest.mark.parametrize("case", [c for c in REF_CASES if c.dtype == HC.BF and (c.B, c.H) in ((2, 16), (2, 8), (2, 32))],
                         ids=lambda c: c.id)
def test_store_defaults_to_the_identity(case):
    """conv_bn_silu / c3 / spp / patch_merging without store= are the graphs they were before the hook: the same bits, forward and
    backward, as with an explicit identity store; the narrowing store gives other bits."""
    a, b, c = HC.run_reference(case, None), HC.run_reference(case, _identity), HC.run_reference(case, HC.narrow)
    assert set(a) == set(b) == set(c)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a["y" if case.kind == "merge" else "out"], c["y" if case.kind == "merge" else "out"])


def test_head_graph_store_defaults_to_the_identity():
    from oracle import ref_torch as R
    sd = HC.state_dict("base")
    feats = HC.walk_features("base")
    ns_a, ns_b, ns_c = {}, {}, {}
    with torch.no_grad():
        ra, ya = R.head_graph(sd, feats, HC.BASE_HEAD, True, ns_a)
        rb, yb = R.head_graph(sd, feats, HC.BASE_HEAD, True, ns_b, store=_identity)
        rc, yc = R.head(sd, feats, True, ns_c, store=_identity)
        rd, _ = R.head_graph(sd, feats, HC.BASE_HEAD, True, {}, store=HC.narrow)
    assert torch.equal(ra, rb) and torch.equal(ra, rc) and not torch.equal(ra, rd)
    assert all(torch.equal(p, q) for p, q in zip(ya, yb)) and all(torch.equal(p, q) for p, q in zip(ya, yc))
    assert set(ns_a) == set(ns_b) == set(ns_c) and all(torch.equal(ns_a[k], ns_b[k]) and torch.equal(ns_a[k], ns_c[k]) for k in ns_a)


def test_store_points_are_the_documented_ones():
    """the names the hook is called with, on every unit kind and on PatchMerging, training and eval"""
    seen = []

    def rec(t, name):
        seen.append(name)
        return t
    for c in HC.CASES:
        if c.dtype != HC.BF or c.prep or c.live:
            continue
        del seen[:]
        HC.run_reference(c, rec)
        if c.kind == "merge":
            assert seen == ["x", "z", "y"], (c.id, seen)
            continue
        pre = f"detect.{c.row}."
        u = HC.spec(c)
        convs = {"Conv": [""], "C3": ["cv1.", "m.0.cv1.", "m.0.cv2.", "cv2.", "cv3."], "SPP": ["cv1.", "cv2."]}[u.kind]
        want = [pre + "x"]
        for cv in convs:
            want += ([pre + cv + "z"] if c.training else []) + [pre + cv + "y"]
            if u.kind == "SPP" and cv == "cv1.":
                want += [f"{pre}m{k}.y" for k in (5, 9, 13)]
        assert seen == want, (c.id, seen)


@pytest.mark.parametrize("case", REF_CASES, ids=[c.id for c in REF_CASES])
def test_reference_conditions(case):
    ref = HC.reference(case)
    HC.check_reference(case, ref)
    sd = HC.state_dict(case.head)
    if case.kind == "merge":
        pre = f"{HC.E}pmerging{case.row}."
        want = {"y", "dX"} | {n[len(pre):] for n in sd if n.startswith(pre)}
        assert want == {"y", "dX", "reduction.weight", "norm.weight", "norm.bias"}
    elif case.training:
        pre = f"detect.{case.row}."
        want = {"out", "din"} | {n[len(pre):] for n in sd if n.startswith(pre)}
        assert sum(1 for n in want if n.endswith("running_var")) == {"Conv": 1, "C3": 5, "SPP": 2}[HC.spec(case).kind]
    else:
        want = {"out"}
    want |= {f"{k}[{s}]" for s, (fields, _) in HC.subsets(case).items() for k in fields if k in want}
    assert set(ref.A) == want and (case.dtype != HC.BF or set(ref.e_emul) == want)
    assert ("out[top]" in want) == HC.has_3x3(case) and ("dX[p10]" in want) == (case.kind == "merge")
    for k, v in ref.e_emul.items():
        print(f"EMUL {case.id} {k} e_emul {v:.3e} gate {HC.MARGIN * v + HC.FLOOR:.3e}")


@pytest.mark.parametrize("head", ["base", "conv3"])
def test_walk_reference_conditions(head):
    ref = HC.walk_reference(head, HC.BF)
    HC.check_reference(f"walk-{head}", ref, HC.BF)
    sd = HC.state_dict(head)
    det = f"detect.{len(HC.HEADS[head]) - 1}."
    want = {n for n in sd if n.startswith("detect.") and not n.startswith(det)}
    want |= {f"h{k}.out" for k, _ in HC.walk_units(head)} | {"df0", "df1", "df2"}
    assert HC.walk_upsampled(head) == [(3, 256), (7, 128)]
    for k, _ in HC.walk_upsampled(head):
        want |= {f"h{k}.din"} | {f"h{k}.din[p{a}{b}]" for a in (0, 1) for b in (0, 1)}
    assert set(ref.A) == want == set(ref.e_emul)
    assert ref.A["h3.din[p01]"].shape == (HC.B_WALK * 8 * 8, 256) and ref.A["h7.din[p11]"].shape == (HC.B_WALK * 16 * 16, 128)
    f32 = HC.walk_reference(head, HC.F32)
    assert set(f32.A) == want and not f32.e_emul


def test_subsets_cover_what_they_name():
    for c in HC.CASES:
        s = HC.subsets(c)
        n = c.B * c.H * c.W
        if c.kind == "merge":
            assert sorted(s) == ["p00", "p01", "p10", "p11"] and all(int(m.sum()) == n // 4 and f == ("dX",) for f, m in s.values())
            assert int(sum(m.long() for _, m in s.values()).min()) == 1 == int(sum(m.long() for _, m in s.values()).max())
        elif HC.has_3x3(c):
            assert sorted(s) == ["bottom", "left", "right", "top"]
            assert int(s["top"][1].sum()) == int(s["bottom"][1].sum()) == c.B * c.W and int(s["left"][1].sum()) == c.B * c.H
            assert bool(s["top"][1][: c.W].all()) and bool(s["right"][1][c.W - 1:: c.W].all())
        else:
            assert s == {}


def test_constants_are_block_cases():
    assert (HC.MARGIN, HC.FLOOR, HC.F32_GATE, HC.E_EMUL_MAX) == (BC.MARGIN, BC.FLOOR, BC.F32_GATE, BC.E_EMUL_MAX)
    assert HC.narrow is BC.narrow and HC.rel_l2 is BC.rel_l2


def test_case_matrix():
    ids = [c.id for c in HC.CASES]
    assert len(set(ids)) == len(ids) == 32
    have = {(c.kind, c.row, c.B, c.H, c.W, c.dtype, c.training, c.direct, c.merged, c.prep, c.live) for c in HC.CASES}
    BF, F32 = HC.BF, HC.F32
    for dt in (BF, F32):
        for row, B, H, W in ((0, 2, 8, 8), (4, 2, 16, 16), (4, 1, 16, 24)):
            assert any(k[:6] == ("conv", row, B, H, W, dt) and k[6] for k in have)
        for row, B, H, W in ((1, 2, 32, 32), (2, 2, 16, 16), (2, 1, 16, 24)):
            assert ("merge", row, B, H, W, dt, True, False, False, (), ()) in have
        for B, H, W in ((1, 16, 24), (2, 8, 8)):
            assert ("spp", 1, B, H, W, dt, True, False, False, (), ()) in have
        assert ("conv", 0, 2, 8, 8, dt, False, False, False, (), ()) in have and ("c3", 7, 2, 16, 16, dt, False, False, False, (), ()) in have
    for B, H, W in ((1, 24, 24), (2, 16, 24)):
        assert ("c3", 3, B, H, W, BF, True, False, False, (), ()) in have
    for B, H, W in ((2, 16, 16), (1, 16, 40)):
        assert ("c3", 7, B, H, W, BF, True, True, True, (), ()) in have
        assert ("c3", 7, B, H, W, BF, True, False, True, (), (("use_direct_conv3", False),)) in have
        assert ("c3", 7, B, H, W, BF, True, True, False, (("use_merged_c3_din", False),), ()) in have
        assert ("c3", 7, B, H, W, F32, True, False, False, (), ()) in have
    # the 3x3 Conv cases are the CONV3_HEAD row, the SPP cases the SPP_HEAD row
    assert all(HC.spec(c).ksize == 3 for c in HC.CASES if c.head == "conv3") and all(c.head == "spp" for c in HC.CASES if c.kind == "spp")
    assert HC.WALKS == (("base", BF), ("base", F32), ("conv3", BF), ("conv3", F32))


@pytest.mark.parametrize("head", sorted(HC.HEADS))
def test_case_table_is_the_parsed_head(head):
    """channels, levels and kernel sizes of UNITS against headgraph.parse_head on the head's yaml; the switches the cases name
    exist on the engine; the PatchMerging widths are the encoder's"""
    HG = importlib.import_module(HC.PKG + ".headgraph")
    from oracle import ref_torch as R
    model, sd = HC.build_model(head)
    hg = HG.parse_head(model)
    rows = [r for (h, r) in HC.UNITS if h == head]
    assert rows
    for r in rows:
        u, s = hg.by_row[r], HC.UNITS[(head, r)]
        assert (u.kind, u.c1, u.c2, u.ksize, u.level) == tuple(s), (head, r, u)
        pre = f"detect.{r}."
        w = sd[pre + ("conv.weight" if u.kind == "Conv" else "cv1.conv.weight")]
        assert w.shape[1] == s.c1 and w.shape[-1] == (s.ksize if u.kind == "Conv" else 1)
    assert [(u.k, u.kind) for u in hg.units] == HC.walk_units(head)
    if head != "spp":
        ups = [(u.k, u.parts[0].channels) for u in hg.units if u.parts[0].shr == 1]
        assert ups == HC.walk_upsampled(head)
        last = hg.by_row[hg.head_out[0]]
        assert HC.walk_grad(head).shape == (HC.B_WALK * (HC.S_MODEL // 4) ** 2, last.c2) and last.k == hg.units[-1].k
    assert all(c.row in hg.by_row for c in HC.CASES if c.head == head and c.kind != "merge")
    assert HC.MERGES == {1: R.STAGE_DIMS[0], 2: R.STAGE_DIMS[1]}
    src = open(os.path.join(os.path.dirname(LIB), "engine.py")).read()
    for c in HC.CASES:
        for k, _ in c.prep + c.live:
            assert f"self.{k} = True" in src, k


def test_watched_kernels_exist_in_the_library():
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} missing: run build() first")
    with open(LIB, "rb") as f:
        blob = f.read()
    from test_head_routes_gpu import SINGLE
    assert len(SINGLE) == 11
    for n in SINGLE + ("ln_fwd_half_kernel", "ln_bwd_half_kernel"):
        assert n.encode() in blob, n
