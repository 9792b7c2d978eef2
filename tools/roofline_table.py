"""Per-kernel roofline table of one training step: every recorded launch of the forward and backward
plans is timed live with HIP events on the launch stream (3 repetitions), its ALGORITHMIC bytes and flops are derived from
its own arguments, and launches are grouped by (entry point, shape).  Bounds use the spec peaks of
/opt/skills/guides/MI355X_MICROARCH.md: 8 TB/s HBM, 2.5 PFLOP/s dense bf16.   frac = max(bytes / 8e12, flops / 2.5e15) / time.

  python tools/roofline_table.py [out.md]        (B=8 @1024^2 bf16 by default: env B, S)
"""
import collections, importlib, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
L = importlib.import_module(bench.PKG + "._lib")
HBM, MFMA = 8e12, 2.5e15
ES = 2          # bf16


def unwrap(a):
    return a._obj if hasattr(a, "_obj") else a


def val(a):
    a = unwrap(a)
    return a.value if hasattr(a, "value") else a


def cost(name, args):
    """(shape string, algorithmic bytes, flops) of one launch."""
    if name == "sodt_gemm_nt":
        g = unwrap(args[0])
        kin, seen = 0.0, set()
        for k in range(g.a.nseg):
            s = g.a.s[k]
            if g.a.spatial and s.p in seen:
                continue
            seen.add(s.p)
            kin += s.klen / ((s.mul * s.mul) if (g.a.spatial and s.shr) else 1)
        nout = 2 if g.flags & 4 else 1
        extra = (1 if g.flags & 2 else 0) + (1 if g.flags & 8 else 0)
        oes = 4 if g.flags & (64 | 128) else ES
        return (f"M={g.M} N={g.N} K={g.K} flags={g.flags}", g.M * (kin * ES + g.N * (nout * oes + extra * ES)) + g.N * g.K * ES,
                2.0 * g.M * g.N * g.K)
    if name == "sodt_gemm_tn":
        g = unwrap(args[0])
        kin, seen = 0.0, set()
        for k in range(g.x.nseg):
            s = g.x.s[k]
            if g.x.spatial and s.p in seen:
                continue
            seen.add(s.p)
            kin += s.klen
        return (f"M={g.M} N={g.N} K={g.K} dW", g.M * (kin + g.N) * ES + 2.0 * g.N * g.K * 4, 2.0 * g.M * g.N * g.K)
    if name == "sodt_linear_bwd_sq":
        g = unwrap(args[0])
        # dY, X in, dX out (+ aux in with SODT_EPI_DGELU): 3 or 4 passes; one partial dW tile per slice written and read, dW itself
        npass = 4 if g.flags & 8 else 3
        return (f"M={g.M} N={g.N} K={g.K} dX+dW{' dgelu' if g.flags & 8 else ''}",
                g.M * npass * g.N * ES + (2.0 * g.splits + 2) * g.N * g.K * 4 + g.N * g.K * ES, 4.0 * g.M * g.N * g.K)
    if name == "sodt_linear_bwd_wide":
        g = unwrap(args[0])
        # the single-pass model: dY (N wide) and X (K wide) in once, dX out; the second and third sibling's dY reads are priced as
        # L2 hits.  One partial dW tile per slice written and read, dW itself, the weight once
        return (f"M={g.M} N={g.N} K={g.K} dX+dW wide", g.M * (g.N + 2 * g.K) * ES + (2.0 * g.splits + 2) * g.N * g.K * 4 + g.N * g.K * ES,
                4.0 * g.M * g.N * g.K)
    if name == "sodt_mlp_bwd":
        M, splits = val(args[19]), val(args[21])
        hact = 1 if args[11] else 0
        # the single-pass model: xn2 and dY (192 wide) in once, dh (768 wide) out (+ GELU(h) where asked for); seven of the eight
        # siblings' reads are priced as L2 hits.  One partial tile per slice and weight written and read, both dW, both weight slabs
        # once; flops: h, dA, dW1, dW2
        return (f"M={M} C=192 hidden=768 dh+dW1+dW2", M * (2 * 192 + (1 + hact) * 768) * ES + 2 * (2.0 * splits + 2) * 768 * 192 * 4
                + 2 * 768 * 192 * ES, 8.0 * M * 768 * 192)
    if name in ("sodt_detect_fwd", "sodt_detect_bwd"):
        g = unwrap(args[0])
        M, N = g.B * g.HW, g.na * g.no
        if name == "sodt_detect_fwd":     # X in once, pred (f32, its own layout) out once, the weight
            return (f"M={M} N={N} K={g.K} Detect fwd", M * (g.K * ES + N * 4) + N * g.K * ES, 2.0 * M * N * g.K)
        # dpred (f32) and X in once; dX out unless SODT_DETECT_NO_DX; one [48][K] partial per slice written and read unless ..._NO_WGRAD
        dx, wg = 0 if g.flags & 2 else 1, 0 if g.flags & 1 else 1
        return (f"M={M} N={N} K={g.K} Detect bwd{'' if dx else ' no dX'}{'' if wg else ' no dW'}",
                M * (N * 4 + (1 + dx) * g.K * ES) + wg * 2.0 * g.splits * 48 * g.K * 4, 2.0 * (dx + wg) * M * N * g.K)
    if name == "sodt_wmsa_block_fwd":
        B, H, W, C = (val(args[i]) for i in (10, 11, 12, 13))
        T = B * H * W
        nrow = 8 if args[7] else 5       # x in; x_mid, xn2, xn1, ao out (+ q, k, v: the f32 parity kernel only)
        return (f"T={T} C={C} train", T * (nrow * C * ES + 12 * 4 + 16), 8.0 * T * C * C + 4.0 * T * 64 * C)
    if name == "sodt_wmsa_block_bwd":
        B, H, W, C = (val(args[i]) for i in (7, 8, 9, 10))
        T = B * H * W
        # xn1, dout in; dqkv (3 rows) out; + the 6 T C^2 flops of the recomputed QKV product on top of the five attention products
        return (f"T={T} C={C} ws=8 bwd+qkv recompute", T * (5 * C * ES + 12 * 4), 10.0 * T * 64 * C + 6.0 * T * C * C)
    if name in ("sodt_window_attn_fwd", "sodt_window_attn_bwd", "sodt_window_attn_bwd_wm"):
        o = {"sodt_window_attn_fwd": 4, "sodt_window_attn_bwd": 8, "sodt_window_attn_bwd_wm": 6}[name]
        B, H, W, C, heads, ws = (val(args[o + i]) for i in range(6))
        T, N = B * H * W, ws * ws
        if name == "sodt_window_attn_fwd":
            return (f"T={T} C={C} ws={ws} fwd", T * (4 * C * ES + heads * 4), 4.0 * T * N * C)
        return (f"T={T} C={C} ws={ws} bwd", T * (8 * C * ES + heads * 4), 10.0 * T * N * C)       # S, dP, dV, dK, dQ
    if name == "sodt_mlp_fwd":
        M, C = val(args[8]), val(args[9])
        # xn, resid in; out (+ GELU(h), 4C wide, in training) out; both weight matrices once
        return (f"M={M} C={C} {'train' if args[7] else 'inference'}", M * ((3 + (4 if args[7] else 0)) * C * ES) + 8.0 * C * C * ES, 16.0 * M * C * C)
    if name.startswith("sodt_conv3x3_c64n8_"):
        o = {"sodt_conv3x3_c64n8_fwd": 4, "sodt_conv3x3_c64n8_dgrad": 3, "sodt_conv3x3_c64n8_wgrad": 5}[name]
        B, H, W = (val(args[o + i]) for i in range(3))
        M = B * H * W           # one pass over the 64-channel tensor and one over the 8-column one; 8 (padded) output channels
        return (f"M={M} 64->8 3x3", M * (64 + 8) * ES, 2.0 * M * 576 * 8)
    if name == "sodt_conv3x3_c64_fwd":
        B, H, W, flags = (val(args[i]) for i in (6, 7, 8, 9))
        M = B * H * W
        nop = 2 + (1 if flags & (2 | 4096) else 0)
        return (f"M={M} 64->64 3x3 flags={flags}", M * 64 * ES * nop + 64 * 576 * ES, 2.0 * M * 64 * 576)
    if name == "sodt_conv3x3_c64_wgrad":
        B, H, W = (val(args[i]) for i in (5, 6, 7))
        M = B * H * W
        return (f"M={M} 64->64 3x3 dW", M * 128 * ES + 2.0 * 64 * 576 * 4, 2.0 * M * 64 * 576)
    if name == "sodt_col_stats":
        M, C = val(args[3]), val(args[4])
        return (f"M={M} C={C}", M * C * ES, 0.0)
    # BatchNorm+SiLU of the head's Conv units: z in, y out / dy, z in / dy, z in, dz out, plus the per-channel vectors
    # (mean, rstd, gamma, beta in f32; the two f64 sums)
    if name == "sodt_bn_silu_fwd":
        M, C = val(args[6]), val(args[7])
        return (f"M={M} C={C}", 2.0 * M * C * ES + 16 * C, 0.0)
    if name == "sodt_bn_silu_bwd_reduce":
        M, C = val(args[7]), val(args[8])
        return (f"M={M} C={C}", 2.0 * M * C * ES + 32 * C, 0.0)
    if name == "sodt_bn_silu_bwd_apply":
        M, C = val(args[10]), val(args[11])
        return (f"M={M} C={C}", 3.0 * M * C * ES + 40 * C, 0.0)
    if name == "sodt_layernorm_fwd":
        M, C = val(args[5]), val(args[6])
        return (f"M={M} C={C}", M * (2 * C * ES + 8), 0.0)
    if name == "sodt_layernorm_bwd":
        M, C = val(args[8]), val(args[9])
        nin = 3 if args[4] else 2
        return (f"M={M} C={C}", M * ((nin + 1) * C * ES + 8), 0.0)
    return ("", 0.0, 0.0)


def main():
    B, S = int(os.environ.get("B", 8)), int(os.environ.get("S", 1024))
    dev = torch.device("cuda:0")
    model = bench.build_model(S, dev, torch.bfloat16)
    x = torch.rand(B, 3, S, S, device=dev); ir = torch.rand(B, 3, S, S, device=dev)

    def step():
        pred, _ = model(x, ir, "RGB+IR"); pred[0].float().square().mean().backward()
        for p in model.parameters():
            p.grad = None
    for _ in range(3):
        step()
    eng = model._get_engine(); plan = eng.plans[(B, S, torch.bfloat16, True)]
    groups = collections.OrderedDict()
    total = 0.0
    tot_bytes = s1_bytes = s1_ms = 0.0
    for which, calls in (("fwd", plan.fwd_main), ("bwd", plan.bwd_main)):
        evs = {i: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for i in range(len(calls))}
        acc = collections.defaultdict(float)
        for rep in range(3):
            setattr(eng, "probes_" + which, evs)
            step(); torch.cuda.synchronize()
            setattr(eng, "probes_" + which, None)
            for i in range(len(calls)):
                acc[i] += evs[i][0].elapsed_time(evs[i][1]) / 3
        for i, (fn, args, name, tag) in enumerate(calls):
            shape, byt, fl = cost(name, args)
            g = groups.setdefault((name.replace("sodt_", ""), shape), [0, 0.0, 0.0, 0.0, set()])
            g[0] += 1; g[1] += acc[i]; g[2] += byt; g[3] += fl; g[4].add(tag.split(".")[0])
            total += acc[i]
            # the byte budget (VERDICT r5 task 3): algorithmic bytes of the whole step and of the stage-1 blocks
            tot_bytes += byt
            if tag.startswith("stage1."):
                s1_bytes += byt; s1_ms += acc[i]
    lines = [f"# Per-kernel roofline table, one training step, B={B} @{S}x{S} bf16 (tools/roofline_table.py)", "",
             f"Sum of the recorded launches: {total:.2f} ms per step (live launches - front end, Detect, optimizer, prep - are outside the "
             "recorded plans: ~1.5 ms).  HIP events on the launch stream, mean of 3 steps.  bytes / flops are ALGORITHMIC (each operand "
             "crosses HBM once); frac = max(bytes / 8 TB/s, flops / 2.5 PFLOP/s) / time.", "",
             "| entry point | shape | launches | ms/step | % | alg. MB / launch | GFLOP / launch | GB/s | TFLOP/s | bound | frac |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    cum = 0.0
    for (name, shape), (n, ms, byt, fl, tags) in sorted(groups.items(), key=lambda kv: -kv[1][1]):
        t = ms / n * 1e-3
        bb, fb = byt / n / HBM, fl / n / MFMA
        frac = max(bb, fb) / t if t > 0 and (byt or fl) else float("nan")
        cum += ms
        lines.append(f"| {name} | {shape} ({','.join(sorted(tags))}) | {n} | {ms:.3f} | {100 * ms / total:.1f} | {byt / n / 1e6:.0f} | {fl / n / 1e9:.1f} | "
                     f"{byt / n / t / 1e9 if t else 0:.0f} | {fl / n / t / 1e12 if t else 0:.0f} | {'mfma' if fb > bb else 'hbm'} | {frac:.3f} |")
        if cum >= 0.93 * total:
            break
    lines.append("")
    lines.append(f"The rows above cover {100 * cum / total:.0f} % of the recorded step time.")
    t1 = B * (S // 4) ** 2
    nblk = len(model.image_encoder.stage1)
    lines.append("")
    lines.append(f"**Byte budget** (tracked since round 6): {tot_bytes / 1e9:.1f} GB of algorithmic HBM traffic per step over the launches whose cost "
                 f"model is in this tool ({tot_bytes / 1e9 / B:.1f} GB per image) = {tot_bytes / 5e12 * 1e3:.1f} ms at the practical 5 TB/s against {total:.1f} ms "
                 f"measured ({tot_bytes / (total * 1e-3) / 1e9:.0f} GB/s average); stage 1: {s1_bytes / 1e9:.1f} GB in {s1_ms:.1f} ms = "
                 f"**{s1_bytes / nblk / (t1 * 192 * ES):.0f} passes over a [{t1}][192] bf16 tensor per block**, forward + backward.")
    out = "\n".join(lines)
    print(out)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(out + "\n")


main()
