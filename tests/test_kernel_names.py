"""canonical_kernel (tests/gemm_cases.py) on the kernel names of the built library's code object: the mangled symbol and
whatever torch's demangler (the profiler's) makes of it must give the same instantiation name, and every attention
instantiation the route table of tests/attn_cases.py names must exist.  No GPU needed."""
import os
import re

import pytest
import torch

import attn_cases as A
import gemm_cases as G

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "small-object-detection-transformers_amd",
                   "libsodt_hip.so")


@pytest.fixture(scope="module")
def mangled():
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} missing: run build() first")
    with open(LIB, "rb") as f:
        blob = f.read()
    names = sorted({m.decode() for m in re.findall(rb"_ZN12_GLOBAL__N_1\d+(?:attn|gemm|tn3)_\w+", blob)})
    assert names, "no kernel symbols found in the library's code object"
    return names


def test_demangled_names_parse_like_mangled(mangled):
    seen = 0
    for m in mangled:
        want = G.canonical_kernel(m)
        assert "unreadable" not in want, (m, want)
        got = G.canonical_kernel(torch._C._demangle(m))
        assert got == want, f"{m}: torch's demangler gives {torch._C._demangle(m)!r} -> {got!r}, the mangled name {want!r}"
        seen += want.startswith("attn_")
    assert seen >= 40


def test_bf16_template_arguments(mangled):
    names = {G.canonical_kernel(m) for m in mangled}
    for n in ("attn_fwd_fast_kernel<bf16, 16, 4>", "attn_bwd_fast2_kernel<bf16, 16, 4, true, true>",
              "attn_bwd_kernel<bf16, 64, 1, false>", "attn_fwd_mt2_kernel<bf16, 64>", "attn_dq_finish_kernel<bf16>",
              "gemm_nt_kernel<bf16, -1>"):
        assert n in names, n


def test_route_table_names_exist(mangled):
    names = {G.canonical_kernel(m) for m in mangled}
    table = set(A.RC_ROUTE) | set(A.bwd_wm_route(A.BF)) | set(A.bwd_wm_route(A.F32))
    for dt in (A.BF, A.F32):
        for hd in (16, 32, 64):
            for ws in (8, 16, 32, 64):
                for shift in (0, ws // 2):
                    table.update(A.fwd_route(dt, hd, ws, shift) + A.bwd_route(dt, hd, ws, shift))
    missing = sorted(table - names)
    assert not missing, f"route table names no kernel of the library: {missing}"
