"""CPU: the shape tables of tests/test_gemm_medium_edges_gpu.py reach the split-K factors they name.  The medium-problem kernel's
split-K rule (splitk_factor_p8m in csrc/gemm_f16x3.hip) restated in gemm_guarded.py, against the tables, against the library's own
cvx_gemm_f16x3_workspace_floats and against the workspace ops.gemm passes: a shape that misses any of them runs unsplit without a word,
and the GPU test would check nothing of the reduction kernels."""
import gemm_guarded as gg
from gemm_guarded import splitk_factor_p8m
from test_gemm_medium_edges_gpu import MAP, NORM, SPLIT, UNSPLIT


def test_split_tables_reach_the_split_path():
    """The factor each table names is what the restated rule gives; the library's own workspace function asks for at least
    factor x M x N floats (so it splits at least that far), and that fits the workspace ops.gemm passes."""
    from covomix_amd import _lib
    lib = _lib.load()
    for M, N, K, K1, slices in SPLIT + NORM + MAP + UNSPLIT:
        assert splitk_factor_p8m(M, N, K, K1) == slices, (M, N, K, K1)
        assert M <= 2048 and K % 32 == 0 and K1 % 32 == 0 and N % 16 == 0
        if slices > 1:
            assert lib.cvx_gemm_f16x3_workspace_floats(M, N, K, K1) >= slices * M * N, (M, N, K, K1)
            assert slices * M * N <= gg.WORKSPACE_FLOATS
            assert K1 % (K // slices) == 0
    assert {s for *_, s in SPLIT} == {2, 4, 8} and any(K1 and s == 8 for _, _, _, K1, s in SPLIT)
    assert [N // 256 for _, N, *_ in NORM] == [1, 2, 3, 4] and 8 in {s for *_, s in NORM}
    # the rule's own edges: one K-tile short of a slice, one block too many, A | A2 off the slice boundary, N % 4
    assert splitk_factor_p8m(300, 80, 1024 - 32) == 1 and splitk_factor_p8m(300, 80, 512) == 2 and splitk_factor_p8m(300, 80, 480) == 1
    assert splitk_factor_p8m(300, 768, 1024) == 4 and splitk_factor_p8m(300, 512, 1024) == 8 and splitk_factor_p8m(1000, 1024, 4096) == 4
    assert splitk_factor_p8m(300, 256, 1024, 384) == 8 and splitk_factor_p8m(300, 256, 1024, 320) == 1 and splitk_factor_p8m(300, 256, 1024, 512) == 8
    for M, N, K, K1 in ((1000, 80, 1024, 0), (1000, 1024, 1024, 0), (1000, 1024, 4096, 0), (1000, 1024, 2048, 1024)):       # test_abi_and_host.py's
        assert lib.cvx_gemm_f16x3_workspace_floats(M, N, K, K1) >= splitk_factor_p8m(M, N, K, K1) * M * N
