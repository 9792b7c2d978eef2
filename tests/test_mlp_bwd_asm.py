"""Static checks on the gfx950 assembly of csrc/mlpbwd.hip (no GPU needed): the checker and the spill budget of
tests/test_asm_hazards.py applied to mlp_bwd_kernel, whose LDS reads are inline-asm loads retired by hand-counted waits while
LDS-DMA stages are in flight, plus the static properties the kernel was designed to: no scratch memory, at most 256 VGPRs (two
waves per SIMD at 512 threads), 152 KiB of dynamic LDS."""
import re

from test_asm_hazards import asm_of, check_async_loads, kernels_of


def test_no_instruction_touches_an_inflight_inline_asm_destination(tmp_path_factory):
    ks = kernels_of(asm_of("mlpbwd", tmp_path_factory), "mlp_bwd_kernel")
    assert len(ks) == 1, [n for n, _ in ks]
    name, body = ks[0]
    assert check_async_loads("mlpbwd.hip " + name, body) > 0


def test_spill_budget_and_register_count(tmp_path_factory):
    asm = asm_of("mlpbwd", tmp_path_factory)
    for pattern in ("mlp_bwd_kernel", "mlpbwd_reduce_kernel"):
        ks = kernels_of(asm, pattern)
        assert len(ks) == 1, pattern
        name, body = ks[0]
        n = len(re.findall(r"\bscratch_", body))
        assert n <= 0, f"mlpbwd.hip {name}: {n} scratch instructions (limit 0)"
        meta = asm[asm.index(".name:           " + name):]
        meta = meta[:meta.index(".wavefront_size")]
        stat = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|agpr_count|private_segment_fixed_size|vgpr_spill_count):\s+(\d+)", meta)}
        assert stat["private_segment_fixed_size"] == 0 and stat["vgpr_spill_count"] == 0, (name, stat)
        assert stat["vgpr_count"] + stat.get("agpr_count", 0) <= 256, (name, stat)


def test_the_stage_loop_waits_on_vector_memory_at_its_barrier_only(tmp_path_factory):
    """From the first LDS-DMA to the last (the prologue's stage 0, then the loop body, which hipcc may peel) every vmcnt wait is the
    hand-written one ahead of a stage barrier, where the stage in flight is the youngest entry of the queue.  Any other - a
    compiler wait on a store or a load it can see - would drain the stage just issued."""
    (name, body), = kernels_of(asm_of("mlpbwd", tmp_path_factory), "mlp_bwd_kernel")
    first = body.index("global_load_lds_dwordx4")
    last = body.rindex("global_load_lds_dwordx4")
    waits = [ln.strip() for ln in body[first:last].split("\n") if "vmcnt" in ln]
    assert waits and all(w == "s_waitcnt vmcnt(0) lgkmcnt(0)" for w in waits), waits
