"""fp64 reference, dyadic lattice and case table of the two-operand GEMM loader (``wgnn_linear_mix_fwd``, include/wgnn.h):

    a[m, k] = fmaf(c2[m], x2[m, k], c1[m] * x1[m, k]),   out = act(a . W^T + bias),   out_scaled[m, :] = row_scale[m] * out[m, :]

Shared by ``test_linear_mix_reference.py`` (CPU: the identity behind the cached feature sum, the lattice budget) and
``test_gpu_linear_mix.py`` (the kernel against this reference, bit for bit).  No kernel is launched here.

Lattice: x1, x2 integers in [-4, 4], c1, c2, row_scale in {0.5, 1, 2}, W in {-1, -0.5, 0.5, 1}, bias an integer in [-8, 8].  Then
a is a multiple of 1/2 with |a| <= 16, every term a * w a multiple of 1/4 (``UNIT``) with |term| <= 16, and the scaled output a
multiple of 1/8 (``UNIT_SCALED``): as long as sum|terms| / unit stays below 2^24 every partial sum in ANY order of summation is an
fp32 number, so fp32 arithmetic in the kernel's order, fp32 in any other order and fp64 agree bit for bit.
"""
import zlib

import numpy as np

UNIT, UNIT_SCALED = 0.25, 0.125
MIX_M = (1, 63, 64, 65, 129, 200)            # one row; around the 64-row tile; two 64-row / 128-row tiles with a ragged edge
MIX_K = (4, 16, 20, 400)                     # one float4; one 16-wide slab; a slab and a tail; the flagship's dense_dim
MIX_N = (1, 16, 127, 128, 129, 256)          # around the 128-column tile; two column tiles
MIX_TILES = (64, 128)
OUTPUTS = ("out", "scaled", "both")


def case_seed(*parts) -> int:
    return zlib.crc32(repr(parts).encode())


def lattice(M, K, N, seed):
    rng = np.random.default_rng(seed)
    half = np.array([0.5, 1.0, 2.0])
    return dict(x1=rng.integers(-4, 5, (M, K)).astype(np.float64), x2=rng.integers(-4, 5, (M, K)).astype(np.float64),
                c1=rng.choice(half, M), c2=rng.choice(half, M), row_scale=rng.choice(half, M),
                w=rng.choice(np.array([-1.0, -0.5, 0.5, 1.0]), (N, K)), bias=rng.integers(-8, 9, N).astype(np.float64))


def reference(x1, c1, x2, c2, w, bias=None, relu=False, row_scale=None):
    """fp64: {out, out_scaled | None, abs_sum (sum of |terms| per output element, the bias among them)}."""
    x1, x2, w = (np.asarray(t, dtype=np.float64) for t in (x1, x2, w))
    c1, c2 = np.asarray(c1, dtype=np.float64)[:, None], np.asarray(c2, dtype=np.float64)[:, None]
    out = (c2 * x2 + c1 * x1) @ w.T
    abs_sum = (np.abs(c2 * x2) + np.abs(c1 * x1)) @ np.abs(w).T
    if bias is not None:
        out, abs_sum = out + np.asarray(bias, dtype=np.float64), abs_sum + np.abs(np.asarray(bias, dtype=np.float64))
    if relu:
        out = np.maximum(out, 0.0)
    scaled = None if row_scale is None else np.asarray(row_scale, dtype=np.float64)[:, None] * out
    return dict(out=out, out_scaled=scaled, abs_sum=abs_sum)


def exact_cases():
    """(tile, M, K, N, bias, relu, outputs, ld): every (tile, M, K, N); the four switches walk through all their 24 combinations
    inside every (tile, M) block of 24 shapes (K x N), shifted from block to block so that every K and every N meets them all."""
    cases = []
    for ti, tile in enumerate(MIX_TILES):
        for mi, M in enumerate(MIX_M):
            for ki, K in enumerate(MIX_K):
                for ni, N in enumerate(MIX_N):
                    i = (ki * len(MIX_N) + ni + 5 * mi + 11 * ti) % 24
                    cases.append((tile, M, K, N, bool(i & 1), bool(i & 2), OUTPUTS[(i >> 2) % 3], bool(i // 12)))
    return cases


EXACT_CASES = exact_cases()


def same_bits(got32, want64) -> bool:
    want64 = np.asarray(want64, dtype=np.float64)
    want32 = want64.astype(np.float32)
    return got32.dtype == np.float32 and np.array_equal(want32.astype(np.float64), want64) and np.array_equal(got32, want32)
