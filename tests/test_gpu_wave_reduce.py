"""The register-only wave reductions of csrc/wave_reduce.h (DPP row shifts and row broadcasts instead of six LDS
permutes) through the test entry nfft_dbg_wave_reduce (csrc/selftest.hip, _lib.wave_reduce): every wave of 64 lanes
against numpy, compared as bit patterns.

Reference: np.fmax.reduce / np.min per wave.  fmax ignores NaN operands, so a NaN comes out only when all 64 lanes hold
one.  One refinement: numpy's fmax leaves the sign of a zero result to the operand order, the hardware maximum orders
-0 < +0 whatever the order (as did the butterfly these helpers replace), so the expected bit pattern is the largest
non-NaN lane under that order -- it is checked to be np.fmax.reduce's value as well.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EDGE_LANES = (0, 15, 16, 31, 32, 47, 48, 63)  # first / last lane of every DPP row
QNAN = np.uint32(0x7FC00000)


def _f32_cases():
    rng = np.random.default_rng(20240611)
    rows = []
    # random values over many magnitudes, both signs
    rows.append((rng.standard_normal((200, 64)) * 10.0 ** rng.integers(-30, 30, (200, 1))).astype(np.float32))
    rows.append(-np.abs(rng.standard_normal((16, 64))).astype(np.float32))  # all negative: no help from a zero start
    # all lanes equal
    rows.append(np.repeat(np.array([[0.0], [-0.0], [1.5], [-2.25e-20], [3.4e38], [-3.4e38], [1e-45]], np.float32), 64, axis=1))
    # the extreme value in the first / last lane of every row of 16
    for lane in EDGE_LANES:
        r = (rng.random((2, 64)) - 0.5).astype(np.float32)
        r[0, lane] = 5.0
        r[1] -= 1.0
        r[1, lane] = -0.25  # the largest of an all-negative wave
        rows.append(r)
    # -0.0 against +0.0
    for lane in EDGE_LANES:
        r = np.full((2, 64), -0.0, np.float32)
        r[0, lane] = 0.0
        r[1] = -np.abs(rng.standard_normal(64)).astype(np.float32)
        r[1, lane] = -0.0
        rows.append(r)
    # denormals (bit patterns below 2^23), both signs, alone and next to normal numbers
    den = rng.integers(1, 1 << 23, (8, 64)).astype(np.uint32) | (rng.integers(0, 2, (8, 64)).astype(np.uint32) << 31)
    den[4:] |= np.uint32(0x80000000)  # four waves of negative denormals only
    rows.append(den.view(np.float32))
    mixed = den[:2].copy().view(np.float32)
    mixed[0, 7] = -1.0
    mixed[1, 40] = np.float32(1.1754944e-38)  # smallest normal
    rows.append(mixed)
    # the largest finite magnitudes
    big = (rng.standard_normal((4, 64)) * 1e30).astype(np.float32)
    big[0, 13] = 3.4e38
    big[1, 63] = np.finfo(np.float32).max
    big[2, :] = -3.4e38
    big[2, 32] = -3.3e38
    big[3, 0] = np.inf
    rows.append(big)
    # NaN lanes: one, several, all but one, all
    for lane in EDGE_LANES:
        r = rng.standard_normal((1, 64)).astype(np.float32)
        r.view(np.uint32)[0, lane] = QNAN
        rows.append(r)
    several = rng.standard_normal((4, 64)).astype(np.float32).view(np.uint32)
    several[0, ::2] = QNAN
    several[1, :48] = QNAN
    several[2, :] = QNAN
    several[2, 31] = np.float32(-7.0).view(np.uint32)  # the only number of the wave, negative
    several[3, :] = QNAN
    rows.append(several.view(np.float32))
    return np.ascontiguousarray(np.concatenate(rows, axis=0))


def _expected_max_bits(v):
    """Bit pattern of the largest non-NaN lane per wave with -0 < +0; NaN (the lanes' common pattern) if there is none."""
    bits = v.view(np.uint32).astype(np.int64)
    key = np.where(bits >> 31 == 1, 0xFFFFFFFF - bits, bits + 0x80000000)  # monotone in the float order, -0 below +0
    key = np.where(np.isnan(v), -1, key)
    pick = np.argmax(key, axis=1)
    return v.view(np.uint32)[np.arange(v.shape[0]), pick]


def test_wave_max_f32_matches_numpy_fmax_bit_for_bit():
    from torch_nfft_amd import _lib
    v = _f32_cases()
    assert 200 <= v.shape[0] <= 1000
    got = _lib.wave_reduce("max_f32", torch.from_numpy(v).cuda().reshape(-1)).cpu().numpy()
    want = _expected_max_bits(v)
    with np.errstate(invalid="ignore"):
        ref = np.fmax.reduce(v, axis=1)
    same_value = (want.view(np.float32) == ref) | (np.isnan(want.view(np.float32)) & np.isnan(ref))
    assert same_value.all()  # the expected pattern IS numpy's fmax (up to the sign of a zero)
    bad = np.nonzero(got.view(np.uint32) != want)[0]
    assert bad.size == 0, [(int(w), hex(int(got.view(np.uint32)[w])), hex(int(want[w]))) for w in bad[:8]]


def _i32_cases():
    rng = np.random.default_rng(77)
    lo, hi = np.iinfo(np.int32).min, np.iinfo(np.int32).max
    rows = [rng.integers(lo, hi, (200, 64), dtype=np.int64).astype(np.int32),
            rng.integers(-20, 200, (32, 64)).astype(np.int32),  # plane numbers, as the gather's producers reduce them
            np.repeat(np.array([[0], [-1], [7], [lo], [hi]], np.int32), 64, axis=1)]
    for lane in EDGE_LANES:
        r = rng.integers(-1000, 1000, (4, 64)).astype(np.int32)
        r[0, lane] = -5000
        r[1, lane] = lo
        r[2, :] = hi
        r[2, lane] = hi - 1
        r[3, :] = hi
        r[3, lane] = lo  # both extremes in one wave
        rows.append(r)
    return np.ascontiguousarray(np.concatenate(rows, axis=0))


def test_wave_min_i32_matches_numpy_min():
    from torch_nfft_amd import _lib
    v = _i32_cases()
    assert 200 <= v.shape[0] <= 1000
    got = _lib.wave_reduce("min_i32", torch.from_numpy(v).cuda().reshape(-1)).cpu().numpy()
    want = v.min(axis=1)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(int(w), int(got[w]), int(want[w])) for w in bad[:8]]
