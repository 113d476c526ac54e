"""CPU: the to_qkv instances of the eight-phase GEMM kernels after their V^T stores went line-major and 16 bytes wide.  The exchange keeps
two row groups' packed halves in registers and the deferred-norm form re-reads its row factors per column group (8 x 4 of them held
through the epilogue went to scratch); a build that spilled would still pass every numerical test.  Read from the built library: no private segment in any to_qkv instance.

Before this change the 256-row qkv_rs instance had a private segment of 164 bytes (values derived from the lane id, hoisted out of the
tile loop and the K loop); the to_qkv instances now recompute them where they are used (gemm_f16x3_p8s.hip, LEAN)."""
from test_attention_form_d import _gfx950_kernel_descriptors

EPI_QKV, EPI_QKV_RS = 1, 8          # gemm_common.h


def test_to_qkv_instances_use_no_scratch():
    from covomix_amd import _lib
    kds = _gfx950_kernel_descriptors(_lib.LIB_PATH)
    large = {k: v for k, v in kds.items() if "gemm_f16x3_p8s_kernel" in k and any(f"Lb0ELi{e}ELi{mi}E" in k for e in (EPI_QKV, EPI_QKV_RS) for mi in (6, 8))}
    medium = {k: v for k, v in kds.items() if "gemm_f16x3_p8m_kernel" in k and f"ELi{EPI_QKV}E" in k}
    assert len(large) == 4, sorted(k for k in kds if "gemm_f16x3_p8s_kernel" in k)          # {qkv, qkv_rs} x {192-row, 256-row tiles}
    assert len(medium) >= 1, sorted(k for k in kds if "gemm_f16x3_p8m_kernel" in k)
    for name, (group, private, vgprs) in {**large, **medium}.items():
        print(f"FIGURE {name[:80]}: LDS {group}, private segment {private}, VGPRs allocated {vgprs}")
        assert private == 0, (name, private)
    for name, (group, private, vgprs) in large.items():
        assert vgprs <= 256, (name, vgprs)              # two waves per SIMD (one 512-thread block per CU)
