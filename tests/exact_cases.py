"""What the bit-exact kernel tests (tests/test_sr_movement_gpu.py, tests/test_prep_utils_gpu.py) share: seeded inputs that carry the
rounding edge cases of an f32 -> bf16 conversion, and a comparison bit for bit."""
import torch

F32, BF16 = torch.float32, torch.bfloat16
IVIEW = {F32: torch.int32, BF16: torch.int16}


def gen(seed):
    return torch.Generator().manual_seed(seed)


def bits_equal(got, ref):
    """bit for bit, except that a NaN only has to be a NaN (its payload is the converter's choice)"""
    assert got.dtype == ref.dtype and got.shape == ref.shape
    ref = ref.to(got.device)
    nan = ref.isnan()
    return bool(torch.equal(got.isnan(), nan)) and bool(torch.equal(got.view(IVIEW[got.dtype])[~nan], ref.view(IVIEW[ref.dtype])[~nan]))


def specials():
    """bf16 ties both ways (1 + 2^-8 -> 1, 1 + 3 * 2^-8 -> 1 + 2^-6: to even, not up, not truncated), just above / below a tie, +-0,
    the largest finite bf16, floats that round up to inf, inf, NaN"""
    return torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), -(1.0 + 3 * 2.0 ** -8), 0.0, -0.0,
                         3.3895313892515355e38, 3.4e38, -3.4e38, float("inf"), -float("inf"), float("nan"),
                         1.0 + 2.0 ** -8 + 2.0 ** -20, 1.0 + 2.0 ** -8 - 2.0 ** -20], dtype=F32)


def values(n, seed):
    """n seeded f32 values with the special ones at seeded places (as many as fit)"""
    v = torch.randn(n, generator=gen(seed))
    sp = specials()
    k = min(sp.numel(), n)
    v[torch.randperm(n, generator=gen(seed + 1))[:k]] = sp.roll(seed)[:k]
    return v
