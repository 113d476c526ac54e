"""CPU: every instance of the large-problem GEMM kernel (gemm_f16x3_p8s_kernel) without a private segment.  A wave holds 128 (96)
accumulators and the fragments of the eight-phase loop; what an instance derives from the lane id and hoists out of the tile loop goes
to scratch beside them, is stored once and re-loaded ~35 times per tile - and a build that spills still passes every numerical test.
Read from the built library's kernel descriptors (metadata only): 22 instances, private segment 0, at most 256 VGPRs (two waves per SIMD).

Before this check the 256-row instances of every epilogue but to_qkv's had private segments of 104-216 bytes (gemm_f16x3_p8s.hip,
epi_lean)."""
from test_attention_form_d import _gfx950_kernel_descriptors


def test_large_problem_gemm_instances_use_no_scratch():
    from covomix_amd import _lib
    kds = {k: v for k, v in _gfx950_kernel_descriptors(_lib.LIB_PATH).items() if "gemm_f16x3_p8s_kernel" in k}
    # <A2 = 0> x {generic, qkv, res, gelu_split, bias, res_tw, gelu_rs, qkv_rs} + <A2 = 1> x {generic, bias, bias_tw}, 192- and 256-row tiles
    assert len(kds) == 22, sorted(kds)
    for name, (group, private, vgprs) in sorted(kds.items()):
        print(f"FIGURE {name[:80]}: LDS {group}, private segment {private}, VGPRs allocated {vgprs}")
    for name, (group, private, vgprs) in sorted(kds.items()):
        assert private == 0, (name, private)
        assert vgprs <= 256, (name, vgprs)
