"""Shapes at which a WAVE of the stage-1 kernels (csrc/conv_first_wave.hip) walks a run of several 8 x 16-pixel blocks.

The kernels are persistent per wave: wave k of a grid of `wgs` workgroups owns blocks [k run, (k + 1) run), run = ceil(blocks / (4 wgs)), row-major
inside an image, and carries the halo image (double-buffered in the forward passes, a single image in the Gram pass and the backward), the next
block's frame rows, the next block's dpooled and routing codes, the scalar block coordinates and its statistics / S1 / Gram accumulators from one
block to the next.  With the default grids (1024 workgroups for the statistics pass, 2048 for apply + pool, 512 for the Gram pass and the
backward) a run is longer than one block only above 4096 / 8192 / 2048 blocks; the HYB_S1_*_WGS switches, read once per process, shrink the grids
for the small rows (tests/stage1_run_worker.py runs them in a child process per environment).

A row: (Ci, Co, N, H, W), then what hyb_stage1_run answers in TRAINING mode for the passes (statistics, apply + pool, Gram, backward) per mode --
> 0 blocks per wave (wave-private kernel), < 0 minus the 8 x 32 tiles per workgroup (block-level kernel), 0 the pass does not run.  In eval mode
the statistics and Gram passes do not run and the other two answers are the same.  tests/test_stage1_run_cpu.py asserts every number from the
library's own query and, from the walk restated in Python, that the table holds what the GPU tests need (its docstring lists it)."""

PASSES = ("statistics", "apply", "gram", "backward")
MODES = ("fp32", "bf16", "bf16x3")

ENVS = {
    "default": {},
    # the workload's own run lengths (config 2: 128 frames of 224 x 224 walk runs of 7 in the apply pass, 25 in the Gram pass and the backward)
    "workload": {"HYB_S1_APPLY_WGS": "7", "HYB_S1_FWD_WGS": "7", "HYB_S1_GRAM_WGS": "2", "HYB_S1_BWD_WGS": "2"},
    # one workgroup per pass: four waves walk everything
    "single": {"HYB_S1_APPLY_WGS": "1", "HYB_S1_FWD_WGS": "1", "HYB_S1_GRAM_WGS": "1", "HYB_S1_BWD_WGS": "1"},
}

# env, (Ci, Co, N, H, W), forward only, {mode: (statistics, apply, gram, backward)}
TABLE = [
    # 13 x 7 = 91 blocks per image, 4186 in all: Gram and backward runs of 3, last run 1, workgroups 349..511 idle; N H W is no power of two
    ("default", (3, 32, 46, 56, 208), False, {"fp32": (2, 1, 0, -5), "bf16": (0, 1, 3, 3), "bf16x3": (2, 1, 0, 3)}),
    # 16471 blocks: apply runs of 3, last run 1, workgroups 1373..2047 idle.  Forward only; the reference is formed in slices of images
    ("default", (3, 32, 181, 56, 208), True, {"fp32": (5, 3, 0, -18), "bf16": (0, 3, 9, 9), "bf16x3": (5, 3, 0, 9)}),
    # 3 x 5 x 13 = 195 blocks under the shrunk grids: 28 waves x 7 (last run 6), 8 waves x 25 (last run 20)
    ("workload", (3, 32, 3, 40, 208), False, {"fp32": (7, 7, 0, -53), "bf16": (0, 7, 25, 25), "bf16x3": (7, 7, 0, 25)}),
    ("workload", (3, 64, 3, 40, 208), False, {"fp32": (7, 7, 0, -53), "bf16": (0, 7, 25, 25), "bf16x3": (7, 7, 0, 25)}),      # NT = 4
    ("workload", (1, 32, 3, 40, 208), False, {"fp32": (7, 7, 0, -53), "bf16": (0, 7, 25, 25), "bf16x3": (7, 7, 0, 25)}),      # the generic channel loop (CI == 0)
    ("workload", (4, 32, 3, 40, 208), False, {"fp32": (7, 7, 0, -53), "bf16": (0, 7, 25, 25), "bf16x3": (7, 7, 0, 25)}),
    ("workload", (3, 8, 3, 40, 208), False, {"fp32": (7, 7, 0, -53), "bf16": (0, 7, 25, 25), "bf16x3": (7, 7, 0, 25)}),       # 24 padded output channels
    ("workload", (3, 32, 2, 64, 256), False, {"fp32": (10, 10, 0, -64), "bf16": (0, 10, 32, 32), "bf16x3": (10, 10, 0, 32)}),   # 256 blocks, N H W = 2^15
    # ragged: W % 4 == 0, W % 16 != 0 and H % 8 != 0 -- the statistics pass's masked branch, no Gram pass, no codes, block-level backward;
    # the last block of a row and the whole last block row are edge blocks: all four orders of inside / edge blocks inside runs
    ("workload", (3, 32, 3, 36, 200), False, {"fp32": (7, 7, 0, -53), "bf16": (7, 7, 0, -53), "bf16x3": (7, 7, 0, -53)}),
    # W % 4 != 0: the block-level forward as well (105 tiles of 8 x 32 on 7 / 7 / 2 workgroups)
    ("workload", (3, 32, 3, 36, 202), False, {"fp32": (-15, -15, 0, -53), "bf16": (-15, -15, 0, -53), "bf16x3": (-15, -15, 0, -53)}),
    ("single", (3, 32, 3, 40, 208), False, {"fp32": (49, 49, 0, -105), "bf16": (0, 49, 49, 49), "bf16x3": (49, 49, 0, 49)}),
    ("single", (3, 32, 3, 36, 200), False, {"fp32": (49, 49, 0, -105), "bf16": (49, 49, 0, -105), "bf16x3": (49, 49, 0, -105)}),
]
ROW_IDS = ["%s_%dto%d_%dx%dx%d" % ((r[0],) + r[1]) for r in TABLE]

# the kernels' default grids (csrc/conv_first.hip, s1_grid_rule) and the switch that replaces each
DEFAULT_WGS = (1024, 2048, 512, 512)
WGS_SWITCH = ("HYB_S1_FWD_WGS", "HYB_S1_APPLY_WGS", "HYB_S1_GRAM_WGS", "HYB_S1_BWD_WGS")


def rows(env):
    return [r for r in TABLE if r[0] == env]


def geometry(shape):
    """-> blocks per row, block rows, blocks per image, blocks"""
    _, _, n, h, w = shape
    bx, by = -(-w // 16), -(-h // 8)
    return bx, by, bx * by, n * bx * by


def inside(shape, b):
    """block b (row-major inside an image) has no ragged edge"""
    _, _, _, h, w = shape
    bx, by, bpi, _ = geometry(shape)
    r = b % bpi
    return (r // bx) * 8 + 8 <= h and (r % bx) * 16 + 16 <= w
