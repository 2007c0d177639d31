"""k_hash_scatter_lds keeps its fixed-point image at LDS address 0: the hashed units' list visit (fix_add_corners8, naruto_field.hip) forms
the address of every ds_add_u64 from the corner's byte offset alone, without the image's symbol.  Dynamic LDS starts behind a kernel's
static LDS, so the contract is "no static LDS in this kernel" -- read here from the built code object's own metadata, the way
test_no_kernel_spills_to_scratch reads its figures; the launcher checks the same figure through hipFuncGetAttributes before the first launch."""


def test_scatter_image_sits_at_lds_offset_zero(built_lib):
    from naruto_amd import _lib
    res = _lib.kernel_resources()
    assert "k_hash_scatter_lds" in res, f"k_hash_scatter_lds not found in the code object (have: {sorted(res)[:8]} ...)"
    k = res["k_hash_scatter_lds"]
    assert "group_segment_fixed_size" in k, k
    assert k["group_segment_fixed_size"] == 0, f"k_hash_scatter_lds has {k['group_segment_fixed_size']} bytes of static LDS: its image would not start at LDS address 0"
