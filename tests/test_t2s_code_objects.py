"""The kernels of csrc/t2s_decode.hip in the built library, from their kernel descriptors alone.

The file's sampling kernels share one body (sample_step), its merge and back-track kernels one each.  The kernels of the default decode
chain and the stand-alone entries are REQUIRED to come out of that sharing as they went in: the table below holds their LDS bytes and
allocated VGPRs in the build of the commit BEFORE the bodies were folded (the instruction text was compared there, symbol by symbol:
profiles/r13_t2s_one_body.txt).  The kernels the fold may move (scoring, mixed pool, beam merge / back-track) are held to no scratch only."""
import re

from test_attention_form_d import _gfx950_kernel_descriptors

# every __global__ of the file: "<name>E..." (plain) or "<name>I..." (template) inside the anonymous namespace
KERNELS = ("gemv_kernel", "attn_kernel", "attn_owner_kernel", "geglu_kernel", "sample_kernel", "sample_per_kernel", "sample_mixed_kernel",
           "mixed_schedule_kernel", "logprob_rows_kernel", "sample_rows_kernel", "beam_select_kernel", "beam_shortlist_kernel",
           "beam_merge_kernel", "beam_backtrack_kernel", "beam_merge_queue_kernel", "beam_backtrack_queue_kernel")
SYMBOL = re.compile(r"_ZN12_GLOBAL__N_1\d+(" + "|".join(KERNELS) + r")([EI].*)")

# (LDS bytes, VGPRs allocated) in the parent's build.  gemv_kernel<MODE, BQ, 1, false>: one entry per BQ, the same for the five MODEs
GEMV = {1: (4112, 64), 2: (8224, 80), 4: (16448, 96), 8: (32896, 120)}
PARENT = {
    "attn_kernelENS_8AttnArgsE": (20496, 72),
    "attn_owner_kernelENS_8AttnArgsEPKi": (36880, 104),
    "geglu_kernelEPKfPflil": (0, 16),
    "sample_kernelILi0ELb0EEEvNS_10SampleArgsE": (4228, 72),                    # <FILT_TOP_K, LOGP = false>: every default launch
    "sample_kernelILi1ELb0EEEvNS_10SampleArgsE": (8324, 48),                    # <FILT_TOP_P, false>
    "sample_per_kernelILb0EEEvNS_10SampleArgsENS_7PerArgsE": (8324, 72),
    "sample_rows_kernelILi0ELb0EEEvNS_14SampleRowsArgsE": (4228, 40),
    "sample_rows_kernelILi0ELb1EEEvNS_14SampleRowsArgsE": (4228, 40),
    "sample_rows_kernelILi1ELb0EEEvNS_14SampleRowsArgsE": (8324, 40),
    "sample_rows_kernelILi1ELb1EEEvNS_14SampleRowsArgsE": (8324, 40),
    "mixed_schedule_kernelENS_10SampleArgsE": (272, 16),
    "beam_shortlist_kernelENS_8BeamArgsE": (8260, 40),
    "beam_select_kernelENS_14BeamSelectArgsE": (12612, 56),
}
PARENT.update({f"gemv_kernelILi{mode}ELi{bq}ELi1ELb0EEEvNS_8GemvArgsE": v for mode in range(5) for bq, v in GEMV.items()})


def test_t2s_kernels_use_no_scratch_and_the_default_chain_keeps_its_resources():
    from covomix_amd import _lib
    kds = {}
    for name, v in _gfx950_kernel_descriptors(_lib.LIB_PATH).items():
        m = SYMBOL.fullmatch(name)
        if m:
            kds[m.group(1) + m.group(2)] = v
    assert set(PARENT) <= set(kds), sorted(set(PARENT) - set(kds))
    missing = [k for k in KERNELS if not any(name.startswith(k + "E") or name.startswith(k + "I") for name in kds)]
    assert not missing, missing                      # (a renamed kernel must not drop out of the private-segment check unnoticed)
    for name, (group, private, vgprs) in sorted(kds.items()):
        print(f"FIGURE {name[:60]}: LDS {group}, private segment {private}, VGPRs allocated {vgprs}")
        assert private == 0, (name, private)
        if name in PARENT:
            assert (group, vgprs) == PARENT[name], (name, group, vgprs, PARENT[name])
