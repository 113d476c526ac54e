"""The launch rule of the split-precision attention with form D (256-query blocks, four waves with two query sets each): host
arithmetic only, no GPU.  D at and above 512 blocks of 256 queries (n_seq x H x ceil(max_T / 256)), the earlier rule below, and every
launch of the existing tables (oracle/attention_oracle.py) keeps the form it names."""
import pytest

import attention_oracle as ao
import covomix_amd.ops as ops


def earlier_rule(n_seq, max_T, rows, H):
    """forms A, B, C as the rule stood before form D: (name, queries per block, key groups, query waves)"""
    blocks = (n_seq * H + 7) // 8 * 8 * ((max_T + 127) // 128)
    if max_T >= 128 and rows < 2048:
        return ("C", 64, 4, 2) if blocks <= 128 else ("B", 128, 3, 4)
    return ("A", 128, 1, 4)


def blocks_256(n_seq, max_T, H):
    return n_seq * H * ((max_T + 255) // 256)


def test_form_d_at_and_above_512_blocks():
    for n_seq, T, H in ((16, 1000, 16), (16, 1008, 16), (8, 2000, 16), (32, 256, 16), (32, 300, 8), (64, 200, 8), (512, 1, 1), (2, 256 * 256, 1)):
        assert blocks_256(n_seq, T, H) >= 512
        assert ops.attention_form(n_seq, T, H) == ("D", 256, 1, 4), (n_seq, T, H)
        assert ops.attention_form(n_seq, T, H, single_term=True) == ("A1", 128, 1, 4), (n_seq, T, H)      # single-term: A1 measured faster
    assert ops.attention_form(H=16, ragged=[1000, 777, 650, 517] * 4) == ("D", 256, 1, 4)
    assert ops.attention_form(H=1, ragged=[128] + [1] * 511) == ("D", 256, 1, 4)          # few rows, many sequences: still D


def test_both_sides_of_the_threshold():
    assert blocks_256(73, 200, 7) == 511 and ops.attention_form(73, 200, 7) == ("A", 128, 1, 4)
    assert blocks_256(64, 200, 8) == 512 and ops.attention_form(64, 200, 8) == ("D", 256, 1, 4)
    assert blocks_256(511, 256, 1) == 511 and ops.attention_form(511, 256, 1)[0] == "A"
    assert blocks_256(511, 257, 1) == 1022 and ops.attention_form(511, 257, 1)[0] == "D"


def test_earlier_rule_below_512_blocks():
    n = 0
    for H in (1, 2, 3, 8, 16):
        for n_seq in (1, 2, 3, 4, 7, 8, 15, 16, 17, 31, 33, 64, 100):
            for T in (1, 31, 64, 127, 128, 129, 255, 256, 257, 300, 500, 512, 513, 1000, 1023, 1025, 2047, 2048, 2500, 5000):
                if blocks_256(n_seq, T, H) >= 512:
                    continue
                n += 1
                for single in (False, True):
                    name, qb, ks, nw = earlier_rule(n_seq, T, n_seq * T, H)
                    assert ops.attention_form(n_seq, T, H, single_term=single) == (name + "1" * single, qb, ks, nw), (n_seq, T, H)
    assert n > 500
    for lengths, H in (([700, 1, 5, 33, 400], 8), ([300, 1, 77], 2), ([900, 300, 900], 1), ([45, 83, 70], 1), ([2048] + [1] * 30, 1)):
        assert blocks_256(len(lengths), max(lengths), H) < 512
        assert ops.attention_form(H=H, ragged=lengths) == earlier_rule(len(lengths), max(lengths), sum(lengths), H)


def _form(shape, H, single=False):
    if isinstance(shape, list):
        return ops.attention_form(H=H, ragged=shape, single_term=single)[0]
    return ops.attention_form(shape[0], shape[1], H, single_term=single)[0]


def test_every_row_of_the_existing_tables_keeps_its_form():
    for row in ao.SHAPES:
        lengths = ao.lengths_of(row["shape"])
        assert blocks_256(len(lengths), max(lengths), row["H"]) < 512, row["id"]
        assert _form(row["shape"], row["H"], row["single"]) == row["form"], row["id"]
    for pair in ao.THRESHOLDS:
        for shape, H, form in pair:
            lengths = ao.lengths_of(shape)
            assert blocks_256(len(lengths), max(lengths), H) < 512, shape
            assert _form(shape, H) == form and _form(shape, H, True) == form + "1", shape
    for form, (shape, H) in ao.VARIANT_SHAPES.items():
        assert _form(shape, H) == form
    for form, Bt in ao.AGREEMENT["batches"].items():
        assert blocks_256(Bt, ao.AGREEMENT["T"], ao.AGREEMENT["H"]) < 512
        assert _form((Bt, ao.AGREEMENT["T"]), ao.AGREEMENT["H"]) == form


def test_forms_are_named():
    assert ops.ATTENTION_FORMS == ("A", "B", "C", "D", "A1", "B1", "C1")
    with pytest.raises(ValueError):
        ops.attention_form(0, 1000, 16)


def _gfx950_kernel_descriptors(path):
    """{kernel name: (group segment bytes, private segment bytes, VGPRs allocated)} of the gfx950 code objects inside a library: the
    offload bundles of its fat binary, each an ELF whose `<kernel>.kd` symbols point at 64-byte kernel descriptors."""
    import struct
    blob = open(path, "rb").read()
    magic, found, at = b"__CLANG_OFFLOAD_BUNDLE__", {}, 0
    while (at := blob.find(magic, at)) >= 0:
        n, = struct.unpack_from("<Q", blob, at + 24)
        pos = at + 32
        for _ in range(n):
            off, size, idlen = struct.unpack_from("<QQQ", blob, pos)
            ident = blob[pos + 24:pos + 24 + idlen].decode()
            pos += 24 + idlen
            if "gfx950" not in ident or size == 0:
                continue
            elf = blob[at + off:at + off + size]
            assert elf[:4] == b"\x7fELF"
            shoff, = struct.unpack_from("<Q", elf, 0x28)
            shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
            secs = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]
            for sec in secs:
                if sec[1] != 2:                                     # SHT_SYMTAB
                    continue
                strtab = secs[sec[6]]
                for j in range(sec[5] // 24):
                    name_off, _, _, shndx, value, _ = struct.unpack_from("<IBBHQQ", elf, sec[4] + 24 * j)
                    end = elf.index(b"\0", strtab[4] + name_off)
                    name = elf[strtab[4] + name_off:end].decode()
                    if not name.endswith(".kd"):
                        continue
                    home = secs[shndx]
                    kd = elf[home[4] + value - home[3]:][:64]
                    group, private = struct.unpack_from("<II", kd, 0)
                    rsrc1, = struct.unpack_from("<I", kd, 48)
                    found[name[:-3]] = (group, private, ((rsrc1 & 63) + 1) * 8)
        at += len(magic)
    return found


def test_form_d_code_objects_use_no_scratch():
    """The three-term form D kernel needs nearly the whole budget of two blocks per CU (256 registers); a build that spills would still
    pass every numerical test.  Read from the built library: no private segment in any attention_f16x3 kernel, 32 KiB of LDS and at
    most 256 registers in both form D kernels (two blocks per CU)."""
    from covomix_amd import _lib
    kds = {k: v for k, v in _gfx950_kernel_descriptors(_lib.LIB_PATH).items() if "attention_f16x3_kernel" in k}
    assert len(kds) == 7, sorted(kds)
    form_d = {k: v for k, v in kds.items() if "ILi3ELi4ELi1ELi2E" in k}
    assert len(form_d) == 1, sorted(kds)
    for name, (group, private, vgprs) in kds.items():
        print(f"FIGURE {name[:60]}: LDS {group}, private segment {private}, VGPRs allocated {vgprs}")
        assert private == 0, (name, private)
    for name, (group, private, vgprs) in form_d.items():
        assert group == 32768 and vgprs <= 256, (name, group, vgprs)
