"""The host-side work partitions of the training weight gradients, restated in Python, so that a CPU test can check that the scale
cases of test_gpu_training_scale.py still reach the regimes they were chosen for (several tiles per chunk, a ragged last chunk, the
2^24-float workspace cap) after a change to the partition or to the cases.

  wgrad2d_partition  sd_conv_wgrad_ndhwc_device, stardist_amd/csrc/train2d.hip:300-315 (8 x 32-pixel tiles, WG_TH / WG_TW :24)
  wgrad3_partition   wgrad3_launch, stardist_amd/csrc/train3d.hip:232-248 (128 columns per workgroup, WG3_COLS :36)
"""

WG_TH, WG_TW = 8, 32
WG3_COLS = 128
WS_CAP = 1 << 24                 # floats of partial sums, at most
TARGET_WGS = 2048                # workgroups the chunk count aims at
GRID_CAP = 65536 * 256           # threads of one element-wise launch (grid_for, train2d.hip:283, train3d.hip:227)


def _div_up(a, b):
    return -(-a // b)


def wgrad2d_partition(B, H, W, c_in, c_out, k):
    """dict(n_tiles, n_chunks, tiles_per_chunk, last_chunk_tiles, cap_binds) of the 2D weight gradient of a k x k layer"""
    tiles_y, tiles_x = _div_up(H, WG_TH), _div_up(W, WG_TW)
    n_tiles = B * tiles_y * tiles_x
    co_groups, ci_chunks = _div_up(c_out, 32), _div_up(c_in, 32)
    per_chunk = k * k * co_groups * 32 * ci_chunks * 32
    n_chunks = _div_up(TARGET_WGS, co_groups * ci_chunks)
    cap = WS_CAP // per_chunk
    cap_binds = n_chunks > cap and cap < n_tiles
    n_chunks = max(min(n_chunks, cap), 1)
    n_chunks = min(n_chunks, n_tiles)
    tpc = _div_up(n_tiles, n_chunks)
    n_chunks = _div_up(n_tiles, tpc)
    return dict(n_tiles=n_tiles, n_chunks=n_chunks, tiles_per_chunk=tpc, last_chunk_tiles=n_tiles - (n_chunks - 1) * tpc,
                cap_binds=cap_binds)


def wgrad3_partition(B, O3, c_in, c_out, k3):
    """dict(n_rows, n_chunks, rows_per_chunk, last_chunk_rows, cap_binds) of the 3D weight gradient: output extent O3 = (Do, Ho, Wo),
    kernel k3; the rows are the (b, zo, yo) of the output"""
    n_cols = k3[0] * k3[1] * k3[2] * c_in
    n_groups, co_groups = _div_up(n_cols, WG3_COLS), _div_up(c_out, 32)
    per_chunk = co_groups * 32 * n_groups * WG3_COLS
    n_rows = B * O3[0] * O3[1]
    n_chunks = _div_up(TARGET_WGS, co_groups * n_groups)
    cap = WS_CAP // per_chunk
    cap_binds = n_chunks > cap and cap < n_rows
    n_chunks = max(min(n_chunks, cap), 1)
    n_chunks = min(n_chunks, n_rows)
    rpc = _div_up(n_rows, n_chunks)
    n_chunks = _div_up(n_rows, rpc)
    return dict(n_rows=n_rows, n_chunks=n_chunks, rows_per_chunk=rpc, last_chunk_rows=n_rows - (n_chunks - 1) * rpc, cap_binds=cap_binds)
