"""CPU: the scale cases of test_gpu_training_scale.py still reach the regimes they were chosen for, on the host partition formulas of
the weight gradients restated in _train_partition.py: several tiles per 2D chunk with a ragged last chunk, the 2^24-float workspace
cap, ragged 3D row chunks, and more than 2^24 elements (a second grid-stride pass, with a ragged tail) for every adjoint, data-gradient
and loss-gradient case.  A change to the partition or to the cases that turns them back into single-iteration tests fails here."""
import numpy as np

import _train_partition as P
import test_gpu_training_scale as S


def _p2(case):
    B, H, W, c0, c1, co, up, k = case
    return P.wgrad2d_partition(B, H, W, c0 + c1, co, k)


def _p3(case):
    B, shape, ci, co, k3, s3, p3, O3 = S.wgrad3_geometry(case)
    return P.wgrad3_partition(B, O3, ci, co, k3)


def test_partition_mirror_examples():
    # worked examples: a 3x3 32 -> 32 layer's cap is 2^24 / (9 * 32 * 32) = 1820 chunks; the 3D_demo stem (7x7x7, 1 -> 32,
    # 2 x 48 x 96 x 96) runs 659 chunks of 14 rows, the last of 4
    p = P.wgrad2d_partition(8, 256, 256, 32, 32, 3)
    assert (p["n_tiles"], p["tiles_per_chunk"], p["n_chunks"], p["cap_binds"]) == (2048, 2, 1024, True)
    p = P.wgrad2d_partition(2, 128, 128, 32, 32, 3)
    assert (p["tiles_per_chunk"], p["n_chunks"], p["cap_binds"]) == (1, 128, False)
    p = P.wgrad3_partition(2, (48, 96, 96), 1, 32, (7, 7, 7))
    assert (p["n_chunks"], p["rows_per_chunk"], p["last_chunk_rows"]) == (659, 14, 4)
    p = P.wgrad3_partition(2, (48, 48, 48), 64, 64, (3, 3, 3))
    assert (p["rows_per_chunk"], p["last_chunk_rows"]) == (63, 9)


def test_2d_cases_reach_multi_tile_chunks():
    parts = [_p2(c) for c in S.WGRAD2D]
    assert any(p["tiles_per_chunk"] >= 2 and p["last_chunk_tiles"] < p["tiles_per_chunk"] for p in parts)
    assert any(p["tiles_per_chunk"] >= 8 for p in parts)
    assert any(p["cap_binds"] and p["tiles_per_chunk"] >= 2 for p in parts)
    # the edge shapes: W < 32, H < 8, extents that are not multiples of the tile
    assert any(c[2] < P.WG_TW for c in S.WGRAD2D) and any(c[1] < P.WG_TH for c in S.WGRAD2D)
    assert any(c[1] % P.WG_TH and c[2] % P.WG_TW for c in S.WGRAD2D)


def test_cap_binds_somewhere():
    assert any(_p2(c)["cap_binds"] for c in S.WGRAD2D) or any(_p3(c)["cap_binds"] for c in S.WGRAD3)


def test_3d_cases_reach_ragged_row_chunks():
    parts = [(c[0], _p3(c)) for c in S.WGRAD3]
    ragged = [(e, p) for e, p in parts if p["rows_per_chunk"] >= 2 and p["last_chunk_rows"] < p["rows_per_chunk"]]
    assert {e for e, _ in ragged} == {"conv3", "convg"}             # both 3D entry points
    assert any(p["rows_per_chunk"] > 8 and p["last_chunk_rows"] < p["rows_per_chunk"] for _, p in ragged)
    assert any(any(n % 2 for n in c[2]) for c in S.WGRAD3)           # odd extents


def _up_shape(shape, up, bits):
    return tuple(n >> ((up >> b) & 1) for n, b in zip(shape, bits))


def _past_grid(n):
    return n > P.GRID_CAP


def test_elementwise_cases_pass_the_grid_cap():
    counts = {}
    counts["relu"] = list(S.RELU_N)
    counts["maxpool2d"] = [int(np.prod(s)) for s, _ in S.MAXPOOL2D]
    counts["maxpool3d"] = [int(np.prod(s)) for s, _ in S.MAXPOOL3D]
    counts["upcat2d"] = [int(np.prod(_up_shape(s[1:], up, (1, 0)))) * s[0] * c0 + int(np.prod(s)) * c1 for s, c0, c1, up in S.UPCAT2D]
    counts["upcat3d"] = [int(np.prod(_up_shape(s[1:], up, (2, 1, 0)))) * s[0] * c0 + int(np.prod(s)) * c1 for s, c0, c1, up in S.UPCAT3D]
    # k_dgrad3: one element per input element of the strided convolution
    counts["dgrad3"] = [B * int(np.prod(shape)) * ci for B, shape, ci, co, k3, s3 in S.DGRAD3G]
    # the up-sampling / concatenation adjoints behind the two-source convolutions' data gradients
    counts["conv3x3 upcat"] = [B * (H >> up) * (W >> up) * c0 + B * H * W * c1 for B, H, W, c0, c1, co, up in S.DGRAD2D]
    counts["conv3x3x3 upcat"] = [B * int(np.prod(_up_shape(shape, up, (2, 1, 0)))) * c0 + B * int(np.prod(shape)) * c1
                                 for B, shape, c0, c1, co, up in S.DGRAD3]
    # k_loss_grad: n_pix * (n_rays + 1)
    counts["loss"] = [int(np.prod(bs)) * (R + 1) for R, bs, _, _, _ in S.LOSSES]
    for kind, ns in counts.items():
        assert ns and all(_past_grid(n) for n in ns), (kind, ns)
    for kind in ("relu", "maxpool2d", "maxpool3d", "upcat2d", "upcat3d"):
        assert all(n % 256 for n in counts[kind]), (kind, counts[kind])


def test_loss_cases():
    rays = {R for R, *_ in S.LOSSES}
    assert rays >= {96, 1, 33}
    assert all(int(np.prod(bs)) % 4096 for _, bs, _, _, _ in S.LOSSES)         # a ragged last partials block
    assert {m for *_, m in S.LOSSES} >= {"empty", "full", "mixed"}
    assert {d for _, _, d, _, _ in S.LOSSES} == {"mae", "mse"}
