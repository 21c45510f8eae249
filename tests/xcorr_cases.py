"""TEST HELPER: the fixed shapes of the correlation tests, each with the launch
variant it is meant to reach, as literals.

tests/test_gpu_parity.py runs every case and asserts that tmr_xcorr_plan
names the variant written here (a retuned threshold fails the case, saying
the table is stale, rather than quietly testing another kernel);
tests/test_abi_host.py scans tmr_xcorr_plan on the CPU and asserts that the
cases cover every MFMA variant the library can pick.

MFMA cases: (H, W, C, kmax, (band_rows, col_groups)).  band_rows 64 / 32 are
the kernel's 4 / 2 row quads per wave, col_groups its W / 64 accumulator
groups; with the precision (and the bf16 output plane, which every bf16 case
also runs) they name one instantiation of xcorr_mfma_kernel.
"""

# 3-term fp16 split (fp32 contract)
MFMA_3TERM = [
    (128, 128, 16, 31, (64, 2)),
    (70, 64, 24, 15, (64, 1)),
    (70, 128, 8, 31, (64, 2)),
    (192, 192, 8, 31, (32, 3)),
    (33, 64, 8, 15, (64, 1)),
    (128, 128, 8, 15, (64, 2)),
    (100, 192, 8, 21, (32, 3)),
    (77, 256, 8, 9, (32, 4)),
    (40, 256, 8, 29, (32, 4)),
    (70, 192, 4, 11, (64, 3)),  # the tallest template that keeps 64-row bands at 192 columns
]

# one bf16 / fp16 term (each case runs in both precisions; bf16 also with out_bf16)
MFMA_ONE_TERM = [
    (128, 128, 16, 31, (64, 2)),
    (70, 64, 24, 15, (64, 1)),
    (128, 128, 8, 15, (64, 2)),
    (100, 192, 8, 21, (32, 3)),
    (70, 192, 4, 19, (64, 3)),  # one plane: 64-row bands up to 19 rows
    (40, 192, 4, 31, (32, 3)),
    (40, 256, 4, 29, (32, 4)),
    (77, 256, 4, 9, (32, 4)),
]

# VALU kernels with a reduced band (staged rows past 150 KB of LDS):
# (H, W, max template (rows, cols), (kernel, band_rows)).  Template sides are
# clamped to the map (a template is never taller than H), so the 9- and 20-row
# maps reach their bands with 9- and 19-row templates; the 33-row maps hold
# the 27- and 31-row templates that take the band down to 1 and 4 rows.
VALU_REDUCED = [
    (40, 1024, (15, 15), ("rows15", 13)),
    (9, 1024, (27, 31), ("rows31", 19)),
    (33, 1024, (27, 31), ("rows31", 1)),
    (70, 512, (31, 31), ("rows31", 31)),
    (20, 1022, (31, 31), ("valu", 16)),
    (33, 1022, (31, 31), ("valu", 4)),
]


def mfma_variants_covered():
    """{(band_rows, col_groups, precision, out16)} over the fixed MFMA cases."""
    out = set()
    for _, _, _, _, (br, cg) in MFMA_3TERM:
        out.add((br, cg, "fp32", 0))
    for _, _, _, _, (br, cg) in MFMA_ONE_TERM:
        out |= {(br, cg, "bf16", 0), (br, cg, "bf16", 1), (br, cg, "f16", 0)}
    return out
