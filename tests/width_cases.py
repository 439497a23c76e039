"""
The row widths at which the kernels that sum in numpy's order take another branch: no GPU, nothing but arithmetic.

What those kernels branch on is the width alone: the tail n % 8, leaves shorter than 8, the first split at 129, trees whose
right spine is deeper than their left, ldq <= 156 (the re-rank's query tile in LDS or not), the 160 KiB of LDS that hold
the group kernel's eight queries (round_up(d, 4) <= 5112), the depth the walk is compiled for, and numpy's 8192-element
buffers.  WIDTHS is derived from those rules, not typed in; tests/test_hip_exact_widths.py asserts what comes out
(`test_width_list`) and walks five kernels over it, tests/test_hip_ivf.py the list scan of the IVF-Flat index.
"""

BUF = 8192                                   # numpy's reduction buffer (sq_pairwise.hpp: PW_BUFSIZE)


def _split(n):
    return n // 2 - (n // 2) % 8


def _depth(n):
    return 0 if n <= 128 else 1 + max(_depth(_split(n)), _depth(n - _split(n)))


def _depth_extremes():
    """For each depth of the split tree of one buffer: the smallest and the largest width that has it."""
    by_depth = {}
    for n in range(129, BUF + 1):
        by_depth.setdefault(_depth(n), []).append(n)
    return {dep: (min(ns), max(ns)) for dep, ns in sorted(by_depth.items())}


EXTREMES = _depth_extremes()
GROUP_LDS_EDGE = (160 * 1024 - 256) // (8 * 4)           # 5112: eight staged queries of round_up(d, 4) floats fill the LDS
WIDTHS = sorted(set(range(1, 18)) | set(range(120, 137))                                # tails, short leaves, the first split
                | {153, 156, 157, 160}                                                  # ldq <= 156
                | {255}                                                                 # a left leaf beside a right subtree
                | {w for pair in EXTREMES.values() for w in pair}
                | {GROUP_LDS_EDGE - 3, GROUP_LDS_EDGE, GROUP_LDS_EDGE + 1, GROUP_LDS_EDGE + 4, GROUP_LDS_EDGE + 5, 6000})
BEYOND = (BUF + 1, BUF + 7, BUF + 8, 2 * BUF + 5)        # numpy's buffers: 8193, 8199, 8200, 16389
N_INDEX = 33 * 32 - 7                                    # 1049 rows: the smallest shape tests/test_hip_scan_variants.py runs off the all-keys route
