"""Shared by tests/test_hubert_length.py (CPU) and tests/test_hubert_length_gpu.py: the HuBERT encoder's GEMM shapes, waveform lengths
with an exact frame count, and the launch rule of the plain (non-interleaved) pre-split branch of gemm_f16x3_impl restated from
csrc/gemm_f16x3.hip, so that the GPU file's cases can say which kernel form they launch and the CPU file can hold the library to it."""

# (N, K) of the encoder GEMMs of a HuBERT-Base checkpoint, M = the frame count T
ENCODER_GEMMS = {"proj": (768, 512), "pos": (48, 6144), "qkv": (2304, 768), "out": (768, 768), "fc1": (3072, 768), "fc2": (768, 3072)}
LENGTHS = (1024, 1025, 2048, 2049)                       # frame counts either side of the two thresholds
SPLITK_MAX_GRID = 128                                    # gemm_f16x3.hip:582
DEEP_RING_MAX_BLOCKS = 256                               # gemm_f16x3.hip:795
CALLER_WORKSPACE_MAX_ROWS = 2048                         # hubert.hip:376 (lin) and ops.py:292 (gemm): a workspace only for M <= 2048


def n_samples(T):
    """A waveform length that yields exactly T frames: the conv stack has a receptive field of 400 samples and a hop of 320."""
    return 320 * (T - 1) + 400


def grid_m(M):
    """Tile rows of the launch, padded to a multiple of 8 for the XCD-aware block map (gemm_f16x3.hip:712-714)."""
    return -(-(-(-M // 128)) // 8) * 8


def splitk_factor(M, N, K):
    """splitk_factor of gemm_f16x3.hip:585-594 without an A2 operand: K slices of a plain pre-split product when the caller provides
    the scratch - at most 128 output tiles (padded tile rows counted), slices of whole 64-column steps and at least 512 columns."""
    tiles = -(-N // 128) * grid_m(M)
    if tiles > SPLITK_MAX_GRID or N % 4:
        return 1
    for cand in (4, 2):
        kp, odd = divmod(K, cand)
        if not odd and kp % 64 == 0 and kp >= 512:
            return cand
    return 1


def route(M, N, K, workspace=None):
    """(ring stages, K slices) of the dma kernel that gemm_f16x3_impl's plain pre-split branch launches (gemm_f16x3.hip:787-800):
    K splits only with a workspace (callers pass one for M <= 2048), and the 4-stage ring needs grid.x * ksplit <= 256."""
    if workspace is None:
        workspace = M <= CALLER_WORKSPACE_MAX_ROWS
    ksplit = splitk_factor(M, N, K) if workspace else 1
    blocks = grid_m(M) * -(-N // 128) * ksplit
    return (4 if blocks <= DEEP_RING_MAX_BLOCKS else 2), ksplit
