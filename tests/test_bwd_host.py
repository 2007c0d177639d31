"""The fp32 MLP backward's resources, read from the built code object's metadata (no GPU): k_query_bwd runs one wave per SIMD with its dW tiles
in accumulation registers, so what it may use is registers (no more than before its 16-wide tiles went to 16x16 blocks), no scratch, and the
LDS its launcher reserves."""


def test_query_bwd_resources(built_lib):
    from naruto_amd import _lib
    res = _lib.kernel_resources()
    lds_cu = 160 * 1024
    reserved = int(built_lib.naruto_debug_query_bwd_lds_bytes())
    assert 0 < reserved <= lds_cu, reserved
    for name in ("k_query_bwd", "k_query_bwd_timeline"):
        assert name in res, f"{name} not found in the code object"
        k = res[name]
        assert k["vgpr_count"] <= 416, (name, k)                    # unified total: architectural + accumulation registers
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("private_segment_fixed_size", 0) == 0, (name, k)
        # all of the kernel's LDS is the dynamic segment the launcher sizes and reserves: any static LDS would come on top of it
        assert k.get("group_segment_fixed_size", 0) + reserved <= lds_cu, (name, k, reserved)
        assert k.get("group_segment_fixed_size", 0) == 0, (name, k)
