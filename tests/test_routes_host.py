"""csrc/routes.h against its Python mirror, without a GPU: tests/host/attn_routes_main.cpp includes only routes.h, is built with the
host compiler under AddressSanitizer and UBSan, and prints what attn_fwd_route / attn_bwd_route / attn_bwd_wm_route /
attn_bwd_rc_route and the three persistent-grid functions answer on dtype x head dim x window x shift (12 heads, B = 2,
H = W = 2 ws).  Every line must equal, as a string, the one tests/attn_cases.py - the table the GPU route tests pin through the
profiler - gives for the same point."""
import os
import shutil
import subprocess

import attn_cases as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "attn_routes_main.cpp")
HEADS, B = 12, 2


def _compiler():
    for c in (shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++"):
        if c and os.path.exists(c):
            return c
    raise AssertionError("a host C++ compiler (g++ or clang++) is required")


def _expected():
    lines = []
    for dt in (A.F32, A.BF):
        for hd in (16, 32, 64):
            for ws in (8, 16, 32, 64):
                for shift in (0, ws // 2):
                    nwin, nwb = B * 2 * 2, A.NW_BWD[(dt, hd)]
                    wm = hd == 16 and ws == 8                # what sodt_window_attn_bwd_wm takes (include/sodt_hip.h)
                    rc = wm and dt == A.BF                   # sodt_wmsa_block_bwd: bf16, C = 192, 12 heads, 8x8 windows
                    cols = [A.fwd_route(dt, hd, ws, shift), A.bwd_route(dt, hd, ws, shift),
                            A.bwd_wm_route(dt) if wm else None, A.RC_ROUTE if rc else None]
                    grids = (A.fwd_fast_grid(nwin), A.bwd_persistent_grid(nwin, HEADS // nwb, nwb), A.rc_grid(nwin))
                    lines.append(" | ".join(["%s %d %d %d" % (A._ty(dt), hd, ws, shift)] +
                                            [";".join(c) if c else "-" for c in cols] + ["%d %d %d" % grids]))
    return lines


def test_attention_routes_equal_their_python_mirror(tmp_path):
    exe = str(tmp_path / "attn_routes")
    r = subprocess.run([_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    got, want = r.stdout.splitlines(), _expected()
    assert len(got) == len(want) == 2 * 3 * 4 * 2
    for g, w in zip(got, want):
        assert g == w
