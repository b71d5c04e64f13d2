"""Shapes at which a workgroup of the asynchronous conv3x3 kernels (csrc/conv_v2.hip) walks a run of several tiles WITHOUT statistics.

The kernels are persistent: a workgroup walks ceil(tiles / grid) consecutive tiles and carries the halo ping-pong, the weight-ring position, the
prefetch of the next tile and the `after_store` flag from one tile to the next.  Without statistics the grid is 256 (eight-wave variants) or
512 (four-wave variants) workgroups, so a run is longer than one tile only above that many tiles.  Every row below has, in that launch,
a run of at least 3 tiles, a shorter last run, runs that cross image boundaries and all four orders of consecutive full and edge tiles inside
runs -- tests/test_conv_run_cpu.py asserts each of these from the library's own queries and the geometry written here.  H and W are even: the
pooled epilogue takes the shapes too.  With statistics the grid is the same (hyb_conv_stats_rows = 512 for every row).

Shared by tests/test_conv_run_cpu.py and tests/test_gpu_exact.py; tests/test_gpu_infer.py (pooled epilogue) and tests/pool_ext_worker.py
(extremes epilogue) list the rows they take in their own STAGES tables."""

# Cin, Cout, N, H, W, hyb_conv3x3_fwd_variant, tile rows, tile columns, tiles, tiles per run, tiles of the last run
RUN_TABLE = [
    (32, 32, 130, 18, 100, 100, 16, 28, 1040, 3, 2),
    (96, 96, 130, 18, 100, 100, 16, 28, 1040, 3, 2),
    (32, 64, 257, 10, 58, 200, 8, 28, 1542, 4, 2),
    (32, 64, 107, 18, 112, 201, 4, 56, 1070, 3, 2),
    (64, 64, 257, 10, 58, 101, 8, 28, 1542, 4, 2),
    (64, 64, 107, 18, 112, 102, 4, 56, 1070, 3, 2),
    (64, 128, 257, 10, 58, 103, 8, 28, 1542, 4, 2),
    (64, 128, 107, 18, 112, 104, 4, 56, 1070, 3, 2),
    (128, 256, 129, 10, 58, 105, 8, 28, 774, 4, 2),
    (64, 256, 65, 18, 112, 106, 4, 56, 650, 3, 2),
    (32, 256, 129, 10, 58, 105, 8, 28, 774, 4, 2),        # one channel block: the weight prefetch of steps S + R - 1 >= 9 goes to the next tile
    (256, 128, 257, 10, 58, 103, 8, 28, 1542, 4, 2),      # eight channel blocks per tile
]
RUN_SHAPES = [r[:5] for r in RUN_TABLE]                   # (Cin, Cout, N, H, W)
RUN_IDS = ["%dto%d_%dx%dx%d" % s for s in RUN_SHAPES]
