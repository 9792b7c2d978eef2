"""A/B of sodt_linear_bwd_sq (csrc/linbwd.hip) against the two launches it replaces, sodt_gemm_tn + sodt_gemm_nt with the
engine's arguments, at the stage-1 shape: M = 524288 (B = 8 @ 1024^2), N = K = 192, bf16, 256 slices, the engine's 64 MiB scratch.
HIP events on the launch stream, same process, same box; the arms alternate and the minimum / median of the rounds are printed.

  python tools/ab_linbwd.py [--parent-lib PATH] [--m 524288] [--rounds 5] [--iters 20] [--once plain|dgelu|pair_plain|pair_dgelu]

--parent-lib: a libsodt_hip.so built from the parent commit; the pair is then ALSO timed through that library (a second
              ctypes handle in the same process), which is the figure the per-launch gate compares against.
--once:       launch one arm a few times and exit (for a counter pass under rocprofv3 --pmc).
--check:      first compare the fused launch with the pair at this shape: dX bit for bit, dW / dbias by their largest difference
              relative to the largest element.
"""
import argparse, ctypes as C, importlib, os, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "small-object-detection-transformers_amd"
L = importlib.import_module(PKG + "._lib")
ops = importlib.import_module(PKG + ".ops")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--m", type=int, default=524288)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--once")
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    dev, dt, M, Cc = torch.device("cuda:0"), torch.bfloat16, a.m, 192
    g = torch.Generator(device="cpu").manual_seed(0)
    dY, X, aux = (torch.randn(M, Cc, generator=g).to(dt).to(dev) for _ in range(3))
    wT = torch.randn(Cc, Cc, generator=g).to(dt).to(dev)
    dX = torch.empty(M, Cc, device=dev, dtype=dt)
    dW = torch.zeros(Cc, Cc, device=dev)
    db = torch.zeros(Cc, device=dev)
    ops.set_tn_scratch(torch.empty(16 << 20, dtype=torch.float32, device=dev))       # the engine's scratch
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fused(dgelu):
        def f():
            assert ops.linear_bwd_sq(dY, X, wT, dX, dW, M, dbias=db, dgelu_aux=aux if dgelu else None)
        return f

    def pair(dgelu):
        def f():
            ops.gemm_tn(dY, [ops.SegSpec(X)], dW, M, Cc, Cc, dbias=db)
            ops.gemm_nt([ops.SegSpec(dY)], wT, dX, M, Cc, Cc, dgelu_aux=aux if dgelu else None)
        return f

    arms = {"plain": fused(False), "dgelu": fused(True), "pair_plain": pair(False), "pair_dgelu": pair(True)}
    if a.parent_lib:
        plib = C.CDLL(a.parent_lib)
        for n in ("sodt_gemm_tn", "sodt_gemm_nt"):
            getattr(plib, n).argtypes = L.SIGNATURES[n]
            getattr(plib, n).restype = C.c_int
        with ops.Recorder() as rec:                   # the very argument records the wrappers build, replayed through the parent
            pair(False)(); pair(True)()
        calls = [(getattr(plib, name), args) for (_, args, name, _) in rec.calls]

        def parent(lo):
            def f():
                for fn, args in calls[lo:lo + 2]:
                    assert fn(*args, st) == 0
            return f
        arms["parent_pair_plain"], arms["parent_pair_dgelu"] = parent(0), parent(2)
    if a.check:
        for k in ("plain", "dgelu"):
            out = {}
            for arm in (k, "pair_" + k):
                dX.zero_(); dW.zero_(); db.zero_()
                arms[arm](); torch.cuda.synchronize()
                out[arm] = (dX.clone(), dW.clone(), db.clone())
            (x1, w1, b1), (x2, w2, b2) = out[k], out["pair_" + k]
            print(f"check {k}: dX identical bits: {torch.equal(x1.view(torch.int16), x2.view(torch.int16))}; "
                  f"dW max |diff| / max |dW| = {float((w1 - w2).abs().max() / w2.abs().max()):.2e}; "
                  f"dbias {float((b1 - b2).abs().max() / b2.abs().max()):.2e}", flush=True)
        dW.zero_(); db.zero_()
    if a.once:
        for _ in range(3):
            arms[a.once]()
        torch.cuda.synchronize()
        return

    def timeit(fn):
        fn(); torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.iters):
            fn()
        e.record(); torch.cuda.synchronize()
        return s.elapsed_time(e) / a.iters

    res = {k: [] for k in arms}
    for _ in range(a.rounds):
        for k, fn in arms.items():
            res[k].append(timeit(fn))
    print(f"M={M} N=K=192 bf16, {a.rounds} rounds x {a.iters} launches, ms per launch (pair = gemm_tn + gemm_nt)")
    print("| arm | min | median | max |\n|---|---|---|---|")
    for k, v in res.items():
        print(f"| {k} | {min(v):.4f} | {statistics.median(v):.4f} | {max(v):.4f} |")
    npass = {"plain": 3, "dgelu": 4}
    for k in ("plain", "dgelu"):
        ref = "parent_pair_" + k if a.parent_lib else "pair_" + k
        t, tp = statistics.median(res[k]), statistics.median(res[ref])
        byt = M * npass[k] * Cc * 2 + (2 * ops.linear_bwd_sq_splits(M) + 2) * Cc * Cc * 4
        print(f"{k}: fused {t:.4f} ms ({byt / t / 1e6:.0f} GB/s of {byt / 1e6:.0f} MB) vs {ref} {tp:.4f} ms: saves {tp - t:+.4f} ms "
              f"(gate: >= 0.03)")


if __name__ == "__main__":
    main()
