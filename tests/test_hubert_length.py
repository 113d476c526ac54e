"""CPU: the route table of tests/test_hubert_length_gpu.py as data, against the library's own host arithmetic.  The frame counts
1024 / 1025 and 2048 / 2049 sit either side of the two thresholds at which the HuBERT encoder's GEMMs change launch form (tile rows
padded 8 -> 16 -> 24; callers pass a split-K workspace for M <= 2048 only); if the launch rule moves and leaves them on one side,
this file fails instead of the GPU file quietly testing one form twice.

What cvx_gemm_f16x3_workspace_floats reports is the larger of TWO rules - the plain pre-split branch's (splitk_factor) and, below
2048 rows, the interleaved medium-problem kernel's (splitk_factor_p8m, up to 8 slices) - because the caller sizes one scratch for
either operand layout; it does not know whether the caller passes a workspace at all.  So it equals 4 M N for fc2 wherever the plain
branch splits and 0 for qkv / fc1 everywhere, but reads 8 M N for pos and 2 M N for out / proj below 2048 rows (the interleaved
kernel's slices, which HuBERT's plain pairs never take), and 4 M N for pos at 2049 rows, where it is the CALLER's M <= 2048 rule that
keeps K whole.  Both rules are therefore restated and the library is held to their maximum exactly; the route table is checked
against the plain rule plus the callers' workspace rule."""
import hubert_oracle as ho
import pytest
from gemm_guarded import WORKSPACE_FLOATS, splitk_factor_p8m
from hubert_routes import ENCODER_GEMMS, LENGTHS, grid_m, n_samples, route, splitk_factor

# T -> {GEMM: (DMA ring stages, K slices)}: the table in tests/test_hubert_length_gpu.py's docstring
ROUTES = {
    1024: dict(proj=(4, 1), pos=(4, 4), qkv=(4, 1), out=(4, 1), fc1=(4, 1), fc2=(4, 4)),
    1025: dict(proj=(4, 1), pos=(4, 4), qkv=(2, 1), out=(4, 1), fc1=(2, 1), fc2=(2, 4)),
    2048: dict(proj=(4, 1), pos=(4, 4), qkv=(2, 1), out=(4, 1), fc1=(2, 1), fc2=(2, 4)),
    2049: dict(proj=(4, 1), pos=(4, 1), qkv=(2, 1), out=(4, 1), fc1=(2, 1), fc2=(4, 1)),
}


@pytest.fixture(scope="module")
def lib():
    from covomix_amd import _lib
    return _lib.load()


def test_lengths_give_the_frame_counts():
    for T in LENGTHS + (1, 2, 499, 4999):
        assert ho.frames_for(n_samples(T)) == T and ho.frames_for(n_samples(T) - 1) == T - 1 and ho.frames_for(n_samples(T) + 319) == T
    assert n_samples(4999) <= 1600000 < n_samples(5000)              # HubertFeatureReader's max_chunk is 4999 frames
    assert [grid_m(T) for T in LENGTHS] == [8, 16, 16, 24]


def test_workspace_sizes_of_the_encoder_shapes(lib):
    ws = lambda M, name: lib.cvx_gemm_f16x3_workspace_floats(M, *ENCODER_GEMMS[name], 0)
    for M in (1024, 1025, 2048):
        N, K = ENCODER_GEMMS["fc2"]
        assert ws(M, "fc2") == 4 * M * N                            # the plain branch's 4 slices (the interleaved rule agrees)
        assert ws(M, "qkv") == 0 and ws(M, "fc1") == 0              # more than 128 tiles, and more than 256 blocks at 2 slices
        assert splitk_factor(M, *ENCODER_GEMMS["pos"]) == 4 and splitk_factor(M, N, K) == 4
        for name in ("qkv", "out", "fc1", "proj"):
            assert splitk_factor(M, *ENCODER_GEMMS[name]) == 1, (M, name)
    assert ws(2048, "pos") == 4 * 2048 * 48 and ws(2048, "out") == 0 and ws(2048, "proj") == 0
    for M in (1024, 1025):                                          # the interleaved kernel's slices, not the plain branch's
        assert ws(M, "pos") == 8 * M * 48 and ws(M, "out") == 2 * M * 768 and ws(M, "proj") == 2 * M * 768
    # 2049 rows: more than 128 tiles, or no K slice of 512 columns - except pos (24 tiles, slices of 1536), which the library would
    # split and the callers' M <= 2048 rule does not
    for name, (N, K) in ENCODER_GEMMS.items():
        assert ws(2049, name) == (4 * 2049 * 48 if name == "pos" else 0), name
        assert route(2049, N, K)[1] == 1
    # the library's figure is exactly the larger of the two restated rules, at every length and shape
    for M in LENGTHS + (2047,):
        for name, (N, K) in ENCODER_GEMMS.items():
            f = max(splitk_factor(M, N, K), splitk_factor_p8m(M, N, K) if M < 2048 else 1)
            assert ws(M, name) == (f * M * N if f > 1 else 0), (M, name)
            assert splitk_factor(M, N, K) * M * N <= WORKSPACE_FLOATS                  # ... and fits what ops.gemm passes


def test_route_table():
    """The restated launch rule (hubert_routes.route: gemm_f16x3.hip:585-594 splitk_factor, :712-715 grid, :787-800 ring choice; the
    callers' workspace rule hubert.hip:376 / ops.py:292) gives the table's 4-stage / 2-stage and split-K columns."""
    for T, row in ROUTES.items():
        for name, (N, K) in ENCODER_GEMMS.items():
            assert route(T, N, K) == row[name], (T, name)
    # both thresholds are where the table says: one frame either way keeps the row
    for name, (N, K) in ENCODER_GEMMS.items():
        assert route(1, N, K) == route(1024, N, K) and route(1026, N, K) == route(1025, N, K) == route(2047, N, K) == route(2048, N, K)
        assert route(2049, N, K) == route(3072, N, K)
    # what the table is there for: forms that no shorter length launches
    assert ROUTES[1025]["fc2"] == (2, 4) and all(v[0] == 4 for v in ROUTES[1024].values())
    assert {n for n, v in ROUTES[2049].items() if v[0] == 2} == {"qkv", "fc1"} and all(v[1] == 1 for v in ROUTES[2049].values())
    # the kernel-level cases of the GPU file
    assert route(2049, 768, 3072) == (4, 1) and route(1025, 2304, 768) == (2, 1) and route(1025, 3072, 768) == (2, 1)
    assert route(1025, 48, 6144) == (4, 4) and route(2049, 48, 6144) == (4, 1)
    assert route(4096, 1024, 1024) == (4, 1) and route(4200, 1024, 1024) == (2, 1)     # single-term: the first shape past 256 blocks
