"""Shared by test_temporal_plans.py (CPU) and test_gpu_temporal.py (MI355X): step_temporal<K, ROWS> at its ten depths
in its three row modes, on the wide shapes, loop-tail boards and thread-rank helpers of wide_cases.py.

    ROWS_WRAP   one rank that is its own N / S neighbour (STEP_WRAP_Y)
    ROWS_GHOST  a rank with y neighbours (thread ranks sharing the GPU), and every pass of a sub-tile superstep after
                the first
    ROWS_SEAM   the first pass of a sub-tile superstep (subtiles=2): rows < 0 and >= h are the other half's edge rows

The sub-tile geometry is mirrored here (the halves of HipEngine::setup_dual, the regions and the rows per segment of
HipEngine::sub_plan); test_gpu_temporal.py asserts the mirror against what the engine reports in stats()["tuning"].

Band heights of a sub-tile plan.  sub_plan cuts a half of hs rows (a region of hs + 2e rows when the pass also stores
e ghost rows each side) into ceil(rows / 2K) balanced bands, so every band is K .. 2K rows tall: K + 1 heights.  For
K >= 5 those reach every residue mod 6 and SEAM_HEIGHTS covers all six; for K <= 4 no sub-tile plan has more than
K + 1 distinct heights, and SEAM_HEIGHTS covers every one of them, K .. 2K, which is every residue such a plan can
have.  The half next to a short board's end (8K <= h < 16K: halves of 8K and h - 8K rows) is what gives the short
bands; one height per depth is >= 16K, where the halves are equal."""
import wide_cases as wc
from wide_cases import CONWAY

TEMPORAL_DEPTHS = [1, 2, 3, 4, 5, 6, 7, 8, 12, 16]
PINGPONG_DEPTHS = {"wrap": [6, 7, 12], "seam": [6, 7, 12], "ghost": [5, 6, 7, 12]}  # the two-triple steady loop
GENS_TOTAL = 2 * max(TEMPORAL_DEPTHS) + 1  # the sweeps' shared history: 2K + 1 generations for every K
TALL_DEPTHS = [5, 6, 7, 8, 12, 16]
SIZES = [1, 2, 3, 63, 64, 65, 127, 137, 200, 1000]
SIZE_CASES = [(N, K) for N in SIZES for K in TEMPORAL_DEPTHS if K <= N]

# ----- thread ranks -----
GHOST_TAIL_HEIGHTS = [2 * h for h in wc.TAIL_HEIGHTS]  # global rows: two strips of 41, 45, 49
MULTI = wc.Shape(96, 4096, 1, 2, 64)  # P = 2: strips of 48 x 4096
GRID = wc.Shape(96, 8192, 2, 4, 64)  # 2 x 2: tiles of 48 x 4096
GRID_DEPTHS = [5, 8, 12, 16]
MULTI_GENS_TOTAL = 4 * max(TEMPORAL_DEPTHS) + 3

# ----- sub-tiles -----
SEAM_WIDTHS = [3968, 8192, 192]
SEAM_HEIGHTS = {
    1: [9, 10, 16],
    2: [18, 19, 32],
    3: [27, 28, 49],
    4: [36, 37, 65],
    5: [45, 53, 81],
    6: [55, 65, 101],
    7: [63, 75, 113],
    8: [73, 87, 131],
    12: [109, 125, 221],
    16: [145, 165, 271],
}
SEAM2_WIDTH = 4096


def seam2_heights(K):
    """halo_depth = 2K: halves of 16K and 2K + 1 rows, and two halves of 16K + 2 and 16K + 3."""
    return [18 * K + 1, 32 * K + 5]


CROSS_SHAPES = [wc.S8000, wc.S3950]


def gens_of(K):
    return 2 * K + 1


def conway_after(H, W, gens, total):
    """The B3/S23 torus board after ``gens`` generations from wide_cases' start board (history over ``total``)."""
    return wc.history(H, W, CONWAY, "torus", total)[1][gens]


def cut(R, K):
    """The ``cut<R>=...`` entry of stats()["tuning"] for supersteps of R generations in passes of K."""
    assert R % K == 0
    return f"cut{R}=" + "+".join([f"temporal@{K}"] * (R // K))


# ----- the sub-tile mirror -----

def sub_halves(h, R):
    """``[(row0, rows)]`` of the two halves of a tile of h rows at halo depth R (HipEngine::setup_dual)."""
    h0 = max(8 * R, min(h - 8 * R, h // 2))
    return [(0, h0), (h0, h - h0)]


def sub_region(hs, nw, e):
    """The output region of a pass of a half of hs rows that also stores e ghost rows on each side."""
    return (-e, hs + e, 0, nw)


def sub_rows(gol, hs, W, K, e, resident_waves):
    """sub_plan's rows per segment: the shortest segments of at least 2K rows whose plan is one round of
    ``resident_waves`` waves."""
    nw = wc.nwords(W)
    return gol.native.balanced_rows_per_chunk([sub_region(hs, nw, e)], nw, hs, K, resident_waves, 2 * K, True)


# Resident waves of a sub-tile plan: blocks per CU x 4 waves x CUs.  At least one block on each of 256 CUs; the
# plans here have far fewer waves, so every count from there up gives the same rows (asserted in test_temporal_plans).
RESIDENT_MIN, RESIDENT_MAX = 4 * 256, 1 << 20


def sub_build(gol, hs, W, K, e=0):
    """``(rows per segment, waves, stats)`` of the plan of a half of hs rows x W columns at depth K."""
    rows = sub_rows(gol, hs, W, K, e, RESIDENT_MIN)
    waves, stats = wc.build(gol, hs, W, K, "torus", rows_per_wave=rows, region=sub_region(hs, wc.nwords(W), e))
    return rows, waves, stats


def sub_bands(gol, h, W, K, R, e=0):
    """The row bands of both halves' plans in tile rows, and per half ``(rows per segment, waves with padding)``."""
    bands, per_half = [], []
    for r0, hs in sub_halves(h, R):
        rows, waves, stats = sub_build(gol, hs, W, K, e)
        bands += [(r0 + b0, n) for b0, n in wc.bands_of(waves)]
        per_half.append((rows, stats["waves"]))
    return sorted(bands), per_half


def sub_entries(R, half, plans):
    """The ``sub<R>.<half>.<pass>=...`` entries of stats()["tuning"] in sub-tile mode for one half, from its plans'
    ``(rows per segment, waves)`` per pass (passes of one depth): consecutive passes with equal plans share an entry,
    ``<first>-<last>``."""
    out, j = [], 0
    while j < len(plans):
        j1 = j
        while j1 + 1 < len(plans) and plans[j1 + 1] == plans[j]:
            j1 += 1
        name = f"{j}" if j1 == j else f"{j}-{j1}"
        out.append(f"sub{R}.{half}.{name}={plans[j][0]}rows,{plans[j][1]}waves")
        j = j1 + 1
    return out
