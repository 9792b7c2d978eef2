"""CPU-side checks: the C-ABI library loads and exports every symbol include/sodt_hip.h declares, the ctypes
records match the header, the Model boundary mirrors the reference's parameter names, and host logic."""
import copy
import ctypes
import importlib
import os
import pickle
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    src = open(os.path.join(ROOT, "include", "sodt_hip.h")).read()
    return sorted(set(re.findall(r"^(?:int|long|const char\*)\s+(sodt_\w+)\s*\(", src, flags=re.M)))


def test_library_exports_every_declared_symbol(pkg):
    L = pkg._lib
    lib = L.load()
    declared = header_symbols()
    assert len(declared) >= 24
    for name in declared:
        assert hasattr(lib, name), f"{name} is declared in include/sodt_hip.h but not exported by libsodt_hip.so"
    assert set(declared) == set(L.exported_symbols())        # (which side lacks what: test_signatures_equal_the_header_type_for_type)
    assert lib.sodt_version().startswith(b"sodt_hip")


HEADER = os.path.join(ROOT, "include", "sodt_hip.h")
SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "double": ctypes.c_double,
           "size_t": ctypes.c_size_t, "long long": ctypes.c_longlong, "unsigned long long": ctypes.c_ulonglong}
# the header's ten records and the ctypes classes of _lib.py that mirror them
STRUCTS = {"sodt_seg": "Seg", "sodt_aspec": "ASpec", "sodt_gemm_args": "GemmArgs", "sodt_gemm_tn_args": "GemmTnArgs",
           "sodt_linbwd_args": "LinBwdArgs", "sodt_conv3_geo": "Conv3Geo", "sodt_tta_pass": "TtaPass",
           "sodt_detect_args": "DetectArgs", "sodt_prep_desc": "PrepDesc", "sodt_step_ctl": "StepCtl"}


def _header_code():
    """include/sodt_hip.h without comments and preprocessor lines."""
    src = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    return re.sub(r"^[ \t]*#[^\n]*$", " ", src, flags=re.M)


def _c_type(decl, named):
    """'const float* rgb' -> ('float', 1): the base type and the pointer depth of a declaration, the name dropped."""
    tok = [t for t in re.findall(r"\w+|\*", decl) if t != "const"]
    if named:
        assert len(tok) >= 2 and re.fullmatch(r"[A-Za-z_]\w*", tok[-1]) and tok[-1] not in ("int", "long", "char", "void"), decl
        tok = tok[:-1]
    return " ".join(t for t in tok if t != "*"), tok.count("*")


def header_prototypes():
    """name -> ((return base, depth), [(parameter base, depth), ...]) of every sodt_* prototype of the header."""
    code = re.sub(r"typedef\s+struct\s*\{[^{}]*\}\s*\w+\s*;", " ", _header_code(), flags=re.S)
    protos = {}
    for stmt in code.split(";"):
        m = re.fullmatch(r"(.*?)\b(sodt_\w+)\s*\((.*)\)", stmt.strip(), flags=re.S)
        if not m:
            assert "(" not in stmt, f"a statement of the header with parentheses that is no sodt_* prototype: {stmt.strip()!r}"
            continue
        ret, name, params = m.groups()
        assert name not in protos, f"{name} is declared twice"
        params = [] if params.strip() == "void" else [_c_type(p, named=True) for p in params.split(",")]
        protos[name] = (_c_type(ret, named=False), params)
    return protos


def _matches(L, base, depth, ct):
    """Does the ctypes type ``ct`` bind a C parameter of type ``base`` with ``depth`` stars?"""
    if depth == 0 and base != "sodt_stream_t":
        return base in SCALARS and ct is SCALARS[base]
    if ct is ctypes.c_void_p:
        return True
    pointee = {"size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double}
    pointee.update({c: getattr(L, py) for c, py in STRUCTS.items()})
    return depth == 1 and base in pointee and ct is ctypes.POINTER(pointee[base])


def abi_findings(L):
    """Every disagreement between the header's prototypes and _lib.SIGNATURES / _lib.RESTYPES, one line each."""
    protos, out = header_prototypes(), []
    tn = lambda t: getattr(t, "__name__", repr(t))
    for name in sorted(set(protos) - set(L.SIGNATURES)):
        out.append(f"{name}: declared in include/sodt_hip.h, not in SIGNATURES")
    for name in sorted(set(L.SIGNATURES) - set(protos)):
        out.append(f"{name}: in SIGNATURES, not declared in include/sodt_hip.h")
    for name in sorted(set(L.RESTYPES) - set(L.SIGNATURES)):
        out.append(f"{name}: in RESTYPES, not in SIGNATURES")
    for name in sorted(set(protos) & set(L.SIGNATURES)):
        (rbase, rdepth), params = protos[name]
        bound, res = L.SIGNATURES[name], L.RESTYPES.get(name, ctypes.c_int)
        want = ctypes.c_char_p if (rbase, rdepth) == ("char", 1) else SCALARS.get(rbase) if rdepth == 0 else None
        if res is not want:
            out.append(f"{name}: returns {rbase}{'*' * rdepth} in the header, {tn(res)} in RESTYPES")
        if len(params) != len(bound):
            out.append(f"{name}: {len(params)} parameters in the header, {len(bound)} in SIGNATURES")
            continue
        for i, ((base, depth), ct) in enumerate(zip(params, bound)):
            if not _matches(L, base, depth, ct):
                out.append(f"{name}: argument {i} is {base}{'*' * depth} in the header, {tn(ct)} in SIGNATURES")
    return out


def test_signatures_equal_the_header_type_for_type(pkg):
    """include/sodt_hip.h is the contract: every prototype is bound in _lib.SIGNATURES (and nothing else is), with the header's
    return type and each parameter's type - scalars exactly, a pointer or the stream as c_void_p or as a POINTER to the
    header's pointee - and the loaded library exports every one of them with exactly these types set."""
    L = pkg._lib
    protos = header_prototypes()
    assert len(protos) == len(header_symbols()) >= 24           # the parser sees what the line-anchored pattern sees
    found = abi_findings(L)
    assert not found, "\n" + "\n".join(found)
    lib = L.load()
    assert L.exported_symbols() == list(L.SIGNATURES)
    for name, argtypes in L.SIGNATURES.items():
        fn = getattr(lib, name)                                  # AttributeError: not exported by libsodt_hip.so
        assert list(fn.argtypes) == list(argtypes) and fn.restype is L.RESTYPES.get(name, ctypes.c_int), name


def _layout_program(L):
    """A host program that prints sizeof of every record of the header and offsetof / sizeof of every field; the field names
    are those of the ctypes classes, so one the header does not have stops the compile."""
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "sodt_hip.h"',
             '#define FIELD(T, f) printf(#T "." #f " %zu %zu\\n", offsetof(T, f), sizeof(((T*)0)->f))',
             "int main(void) {"]
    for c, py in STRUCTS.items():
        lines.append(f'  printf("{c} %zu\\n", sizeof({c}));')
        lines += [f"  FIELD({c}, {f[0]});" for f in getattr(L, py)._fields_]
    return "\n".join(lines + ["  return 0;", "}", ""])


def test_every_ctypes_record_has_the_header_layout(pkg, tmp_path):
    """All ten records, field by field: the header compiled on the host against ctypes.sizeof / .offset / .size."""
    import subprocess
    from test_routes_host import _compiler
    L = pkg._lib
    declared = re.findall(r"typedef\s+struct\s*\{[^{}]*\}\s*(\w+)\s*;", _header_code(), flags=re.S)
    assert sorted(declared) == sorted(STRUCTS) and len(STRUCTS) == 10
    classes = [v for v in vars(L).values() if isinstance(v, type) and issubclass(v, ctypes.Structure) and v is not ctypes.Structure]
    assert sorted(c.__name__ for c in classes) == sorted(STRUCTS.values())
    src, exe = tmp_path / "layout.cpp", str(tmp_path / "layout")
    src.write_text(_layout_program(L))
    r = subprocess.run([_compiler(), "-std=c++17", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    got = {ln.split()[0]: tuple(int(v) for v in ln.split()[1:]) for ln in r.stdout.splitlines()}
    want = {}
    for c, py in STRUCTS.items():
        cls = getattr(L, py)
        want[c] = (ctypes.sizeof(cls),)
        for f in cls._fields_:
            want[f"{c}.{f[0]}"] = (getattr(cls, f[0]).offset, getattr(cls, f[0]).size)
    assert set(got) == set(want)
    bad = [f"{k}: header {got[k]}, ctypes {want[k]}" for k in want if got[k] != want[k]]
    assert not bad, "\n" + "\n".join(bad)
    # a field the header has and the class lacks leaves a gap or a short record: sizes and offsets above cover both, and
    # the counts close it
    for c, py in STRUCTS.items():
        body = re.search(r"typedef\s+struct\s*\{([^{}]*)\}\s*" + c + r"\s*;", _header_code(), flags=re.S).group(1)
        names = [re.search(r"(\w+)\s*(?:\[[^\]]*\])?\s*$", d).group(1) for s in body.split(";") if s.strip() for d in s.split(",")]
        assert names == [f[0] for f in getattr(L, py)._fields_], c


def test_frontend_wrappers_take_the_window_and_the_workspace_by_keyword_only(ops):
    """A call written for the former square wrappers, (..., B, S, 1) or (..., B, S, 1, ws), must not run with W = 1."""
    import inspect
    for fn, names in ((ops.frontend_fwd, ("ca_ws",)), (ops.frontend_bwd, ("ca_ws", "ws"))):
        par = inspect.signature(fn).parameters
        assert list(par)[-len(names) - 3:-len(names)] == ["B", "H", "W"]
        assert all(par[n].kind is inspect.Parameter.KEYWORD_ONLY for n in names)
    with pytest.raises(TypeError):
        ops.frontend_fwd(*[None] * 8, 1, 64, 64, 1)


def test_ctypes_record_layout(pkg):
    L = pkg._lib
    assert ctypes.sizeof(L.Seg) == 40 and ctypes.sizeof(L.ASpec) == 40 * 9 + 16
    assert ctypes.sizeof(L.PrepDesc) == 48
    assert L.GemmArgs.a.offset == 0 and L.GemmArgs.W.offset == ctypes.sizeof(L.ASpec)
    assert L.GemmTnArgs.x.offset == 16


def test_missing_library_fails_loudly(pkg, monkeypatch):
    L = pkg._lib
    monkeypatch.setattr(L, "_lib", None)
    monkeypatch.setattr(L, "LIB_PATH", "/nonexistent/libsodt_hip.so")
    with pytest.raises(ImportError):
        L.load()


@pytest.mark.parametrize("var", ["SODT_LIB_PATH", "SODT_HG_DBG", "SODT_WMSA_ONE_WAVE"])
def test_bench_refuses_diagnostic_environment(var):
    """a timed number must not come from an ablated kernel or a swapped library."""
    import subprocess
    import sys
    env = dict(os.environ, **{var: "1"})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "1"],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2, (r.returncode, r.stderr[-500:])
    assert var in r.stderr and "refusing" in r.stderr
    assert r.stdout.strip() == ""          # no JSON line


def test_library_reads_no_environment_switch():
    """The ablation paths of the fused kernel are compile-time macros of the tools/exp A/B build, not run-time switches."""
    csrc = os.path.join(ROOT, "small-object-detection-transformers_amd", "csrc")
    for f in os.listdir(csrc):
        assert "getenv" not in open(os.path.join(csrc, f)).read(), f


def test_version_reports_library_override(pkg, ops, monkeypatch):
    assert pkg._lib.overrides() == {} or "SODT_LIB_PATH" in os.environ
    monkeypatch.setenv("SODT_HG_DBG", "3")
    assert pkg._lib.overrides().get("SODT_HG_DBG") == "3"
    assert "SODT_HG_DBG=3" in ops.version()


@pytest.fixture(scope="module")
def M(pkg):
    return importlib.import_module("small-object-detection-transformers_amd.model")


def test_model_mirrors_reference_state_dict(M):
    from oracle import ref_torch as R
    for cfg in ("model.yaml", "SRyolo_MF.yaml"):
        m = M.Model(cfg, input_mode="RGB+IR", ch_steam=3, ch=128, nc=8)
        assert sum(p.numel() for p in m.parameters()) == 22007851
        sd = m.state_dict()
        assert len(sd) == 273
        spec = R.state_dict_spec(512, 8)
        for k, shape in spec.items():
            assert tuple(sd[k].shape) == tuple(shape), k
        extra = set(sd) - set(spec)
        assert all(("relative_position_index" in k or "attn_mask" in k or "num_batches_tracked" in k) for k in extra), extra
        det = m.detect[-1]
        assert det.nl == 1 and det.na == 3 and det.no == 13 and float(m.stride[0]) == 4.0
        assert torch.allclose(det.anchors.view(-1), torch.tensor([10, 13, 16, 30, 33, 23.]) / 4)
        assert m.yaml["nc"] == 8 and hasattr(m, "yaml_file")
        assert m.image_encoder.stage1[1].attn_mask.shape == (256, 64, 64)   # kept for checkpoint parity
        assert m.image_encoder.stage3[0].attn.relative_position_bias_table.shape == (3969, 12)
        bn = m.detect[0].bn
        assert bn.eps == 1e-3 and bn.momentum == 0.03


def test_model_has_no_cpu_path_and_is_copyable(M):
    m = M.Model("model.yaml", input_mode="RGB+IR", ch_steam=3, ch=128, nc=8)
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(x, x, "RGB+IR")
    with pytest.raises(RuntimeError):
        m.detect[0](x)                     # containers never compute in torch
    with pytest.raises(NotImplementedError):
        m(x, x, "RGB")
    m2 = copy.deepcopy(m)                  # ModelEMA
    assert m2._engine is None and len(m2.state_dict()) == 273
    m3 = pickle.loads(pickle.dumps(m))     # checkpoints pickle the module object
    assert torch.equal(m3.detect[8].m[0].bias, m.detect[8].m[0].bias)
    # sr=True builds the reference's DeepLab(4, c1, c2) parameter tree (model.py:109-117); its 82 tensors follow the detector's
    ms = M.Model("model.yaml", input_mode="RGB+IR", ch_steam=3, ch=128, nc=8, sr=True)
    keys = list(ms.state_dict())
    assert len(keys) == 273 + 82 and keys[273] == "model_up.sr_decoder.conv1.weight" and (ms.l1, ms.l2) == (4, 8)
    with pytest.raises(RuntimeError, match="inside the MI355X engine"):
        ms.model_up(x, x)
    with pytest.raises(NotImplementedError):
        M.Model("model.yaml", input_mode="RGB+IR", sr=True, factor=4)


def test_fuse_matches_reference_formula(M):
    m = M.Model("model.yaml", input_mode="RGB+IR", ch_steam=3, ch=128, nc=8)
    c = m.detect[3].m[0].cv2
    with torch.no_grad():
        c.bn.running_mean.uniform_(-0.5, 0.5); c.bn.running_var.uniform_(0.5, 2); c.bn.weight.uniform_(0.5, 1.5); c.bn.bias.uniform_(-1, 1)
    x = torch.randn(2, c.conv.in_channels, 6, 6)
    with torch.no_grad():
        z = torch.nn.functional.conv2d(x, c.conv.weight, None, padding=1)
        want = torch.nn.functional.batch_norm(z, c.bn.running_mean, c.bn.running_var, c.bn.weight, c.bn.bias, False, 0.0, 1e-3)
    m.fuse()
    assert not hasattr(c, "bn") and c.conv.bias is not None
    with torch.no_grad():
        got = torch.nn.functional.conv2d(x, c.conv.weight, c.conv.bias, padding=1)
    assert float((got - want).abs().max()) < 1e-4


def test_parse_model_rejects_out_of_scope_modules(M):
    cfg = dict(nc=8, depth_multiple=0.33, width_multiple=0.5, anchors=[[10, 13, 16, 30, 33, 23]],
               backbone=[[-1, 1, "MF", [3]]], head=[])
    with pytest.raises(NotImplementedError):
        M.Model(cfg, input_mode="RGB+IR")


def test_host_helpers(ops):
    assert ops.tn_splits(524288, 768, 192) == 85 and ops.tn_splits(100, 768, 192) == 1
    assert ops.tn_splits(32768, 3072, 768) == 10
    assert ops.tn_splits(524288, 192, 768, True) == 85 and ops.tn_splits(131072, 384, 384, True) == 64
    assert ops.tn_splits(512, 192, 768, True) == ops.tn_splits(512, 192, 768)      # short M keeps the f32-path rule
    s = ops.SegSpec(torch.zeros(4, 96), 32, 64)
    assert (s.ld, s.klen, s.coff) == (96, 32, 64)


def test_sr_direct_conv_bias_operand(pkg):
    """advisor r5: the direct 64 -> <= 8 convolution reads 8 bias floats; at cout == 8 there is no zero-padded copy (np_ == cout) and
    the parameter itself must be passed (a None there silently dropped the bias), at cout < 8 the padded copy, without a bias None."""
    import importlib
    import types
    sr = importlib.import_module("small-object-detection-transformers_amd.sr")
    b8, pad = torch.arange(8.0), torch.zeros(8)
    assert sr.SRBranch._bias8(types.SimpleNamespace(bias=b8, bias_pad=None)) is b8
    assert sr.SRBranch._bias8(types.SimpleNamespace(bias=torch.arange(4.0), bias_pad=pad)) is pad
    assert sr.SRBranch._bias8(types.SimpleNamespace(bias=None, bias_pad=None)) is None


def test_engine_names_the_input_sizes_it_refuses(M):
    """Window padding (round 6): the geometry helper must refuse, by name, the single-window stages whose rows 64-token tiles do not
    cover; it accepts 8 / 16 / 32-token windows and leaves larger grids to the padded path."""
    import importlib
    import types
    E = importlib.import_module("small-object-detection-transformers_amd.engine")
    tab = lambda ws: types.SimpleNamespace(relative_position_bias_table=torch.zeros((2 * ws - 1) ** 2, 12), window_size=(ws, ws))
    geo = E.Engine._block_geo
    assert geo(None, types.SimpleNamespace(window_size=32, shift_size=0, attn=tab(16)), 16, 16) == (16, 0)     # clamped to one window
    assert geo(None, types.SimpleNamespace(window_size=32, shift_size=0, attn=tab(32)), 40, 40) == (32, 0)     # padded by the caller
    with pytest.raises(NotImplementedError, match="ONE 20x20 window"):
        geo(None, types.SimpleNamespace(window_size=32, shift_size=0, attn=tab(20)), 20, 20)
