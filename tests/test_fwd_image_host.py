"""The training forward's weight image, host side (no GPU): where the finishing launch puts each MLP weight (naruto_debug_fwd_image_map -- the
inverse of the staging routine, enumerated from its index expressions) and the register budgets of the two kernels that read the image.
tests/test_gpu_fwd_image.py holds the map against the staging code itself, byte for byte."""
import ctypes as C

import numpy as np

from naruto_amd import _lib

N_SDF_W0, N_SDF_W1, N_COL_W0, N_COL_W1 = 32 * 80, 16 * 32, 32 * 63, 3 * 32        # the optimiser's order


def _map(lib):
    img, nw = C.c_size_t(), C.c_uint32()
    total = lib.naruto_fwd_image_bytes(C.byref(img), C.byref(nw))
    slots = np.zeros(nw.value, np.uint32)
    zero = np.zeros(img.value, np.uint8)
    assert lib.naruto_debug_fwd_image_map(slots.ctypes.data, zero.ctypes.data) == 0
    return total, img.value, nw.value, slots, zero


def test_every_weight_has_its_own_bytes_and_the_rest_is_the_zero_padding(built_lib):
    total, img, nw, slots, zero = _map(built_lib)
    assert nw == N_SDF_W0 + N_SDF_W1 + N_COL_W0 + N_COL_W1 == 5184
    assert img % 16 == 0 and total >= img + 4 * nw            # | image | slot of every weight |
    off, stride = (slots & 0xFFFF).astype(np.int64), (slots >> 16).astype(np.int64)
    owner = np.full(img, -1, np.int64)
    for w in range(nw):
        # three bf16 pieces (hi, mid, lo) `stride` bytes apart for the matrix layers; one float for col_w1, whose layer runs on the vector ALU
        is_c1 = w >= nw - N_COL_W1
        assert (stride[w] == 0) == is_c1, w
        ranges = [(off[w], 4)] if is_c1 else [(off[w] + k * stride[w], 2) for k in range(3)]
        for b, n in ranges:
            assert 0 <= b and b + n <= img and b % n == 0, (w, b)
            assert (owner[b:b + n] == -1).all(), f"weight {w} shares bytes with weight {owner[b]}"
            owner[b:b + n] = w
    # the bytes no weight maps to are exactly those the staging fills with zero
    assert np.array_equal(owner == -1, zero == 1)
    # ... and those are what the layout says: output rows >= 16 of sdf layer 1 (2 K blocks x 32 lanes of the upper rows x 8 values) and the
    # sdf-net output row 0 (the sdf itself) in colour layer 0's geo block (32 units x 1 value), three 2-byte pieces each
    assert int((zero == 1).sum()) == 3 * 2 * (2 * 32 * 8 + 32)
    assert int((owner >= 0).sum()) == 6 * (N_SDF_W0 + N_SDF_W1 + N_COL_W0) + 4 * N_COL_W1 == img - int((zero == 1).sum())


def test_image_kernels_keep_the_register_budgets_of_the_kernels_they_stand_in_for(built_lib):
    """k_query_fwd_loss_img / k_query_fwd_loss_short_img run in place of k_query_fwd_loss<false,true> / k_query_fwd_loss_short<false> in the chained
    iterations: the same budgets (tests/test_host.py) -- no scratch, 256 registers per lane for two waves per SIMD, 140 / 128 spilled scalars."""
    res = _lib.kernel_resources()
    for name, sgpr in (("k_query_fwd_loss_img", 140), ("k_query_fwd_loss_short_img", 128)):
        assert name in res, sorted(res)[:8]
        r = res[name]
        assert r.get("vgpr_spill_count", 0) == 0 and r.get("private_segment_fixed_size", 0) == 0, (name, r)
        assert r["vgpr_count"] <= 256 and r["sgpr_spill_count"] <= sgpr, (name, r)
    # the image kernels hold the same LDS as the kernels they replace (two workgroups per CU at S = 128)
    assert res["k_query_fwd_loss_img"]["group_segment_fixed_size"] == res["k_query_fwd_loss<false,true>"]["group_segment_fixed_size"]
    assert res["k_query_fwd_loss_short_img"]["group_segment_fixed_size"] == res["k_query_fwd_loss_short<false>"]["group_segment_fixed_size"]
