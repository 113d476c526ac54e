"""GPU: the prompt mel of many wav prompts in one call (mel.mel_spectrogram_many / mel.extract_mel_many over
cvx_mel_spectrogram_many_f32) against the one-prompt path it must reproduce BIT FOR BIT (mel.mel_spectrogram / mel.extract_mel,
unchanged), the CPU oracle and the reference-held fixtures at the project's 5e-5 absolute on the log-mel (test_mel_gpu.py's bound;
it holds by the equality), and the packing kernel on its own against the numpy restatement in tests/mel_items.py (stored items
exact, resampled items within the resampler's 2e-6 of test_hubert_gpu.py).  Signals are test_mel_gpu.py's sine plus noise, seeded
per length."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import mel_items
import mel_oracle as mo

pytestmark = pytest.mark.gpu

LENGTHS = [161, 319, 320, 479, 480, 481, 159 * 160, 16123]
SENTINEL = -12345.0


def signal(n, rate=8000.0, seed=None):
    g = torch.Generator().manual_seed(n if seed is None else seed)
    t = torch.arange(n) / rate
    y = 0.4 * torch.sin(2 * np.pi * 440 * t) + 0.2 * torch.sin(2 * np.pi * 1333 * t + 1.0) + 0.05 * torch.randn(n, generator=g)
    return y.clamp(-1, 1)


def square(n):
    return (((torch.arange(n) // 7) % 2) * 2 - 1).float()                # full scale: pinned at +-1


@pytest.fixture(scope="module")
def batch():
    """The issue's eight lengths: signals, the one-prompt mels (computed once) and the mels of ONE ragged call."""
    from covomix_amd import mel
    wavs = [signal(n) for n in LENGTHS]
    one = [mel.mel_spectrogram(w.cuda()) for w in wavs]
    many = mel.mel_spectrogram_many([w.cuda() for w in wavs])
    return wavs, one, many


def test_every_item_is_bit_identical_to_the_one_prompt_call(batch):
    wavs, one, many = batch
    assert len(many) == len(LENGTHS)
    for n, a, b in zip(LENGTHS, one, many):
        assert b.is_cuda and b.shape == a.shape == (80, n // 160) and b.dtype == torch.float32
        assert torch.equal(a, b), f"length {n}: max abs diff {float((a - b).abs().max())}"


def test_every_item_against_the_cpu_oracle(batch):
    wavs, _one, many = batch
    for n, w, b in zip(LENGTHS, wavs, many):
        err = float((b.cpu() - mo.mel_spectrogram(w[None])[0]).abs().max())
        print("length", n, "max abs err vs oracle", err)
        assert err < 5e-5


def test_one_item_through_the_many_path(batch):
    from covomix_amd import mel
    wavs, one, _many = batch
    for i in (0, 6, 7):
        got = mel.mel_spectrogram_many([wavs[i].cuda()])
        assert len(got) == 1 and torch.equal(got[0], one[i])


def test_an_item_does_not_depend_on_its_neighbours_or_its_place(batch):
    from covomix_amd import mel
    wavs, one, _many = batch
    x, ref = wavs[7].cuda(), one[7]                                       # 16123 samples: its last slot is partly slack
    sq = [square(n).cuda() for n in (481, 3001, 161)]
    zero = [torch.zeros(n, device="cuda") for n in (481, 3001, 161)]
    for others in (sq, zero):
        for place in (0, 1, 3):                                           # first, in the middle, last
            items = list(others)
            items.insert(place, x)
            got = mel.mel_spectrogram_many(items)
            assert torch.equal(got[place], ref), (place, float((got[place] - ref).abs().max()))
    got = mel.mel_spectrogram_many([sq[0], x, zero[1]])
    assert torch.equal(got[1], ref)
    assert torch.equal(got[0], mel.mel_spectrogram(sq[0])) and torch.equal(got[2], mel.mel_spectrogram(zero[1]))


def test_nothing_stale_is_read(batch):
    """Workspace (the packed buffer lies in it) full of NaN before the call: the same finite output as from a zeroed one."""
    from covomix_amd import mel
    wavs, one, _many = batch
    items = [w.cuda() for w in wavs]
    mel.mel_spectrogram_many(items)                                       # (the workspace exists and is large enough from here on)
    ws = mel._WS[items[0].device]
    ws.zero_()
    clean = [m.clone() for m in mel.mel_spectrogram_many(items)]
    assert mel._WS[items[0].device] is ws
    ws[: ws.numel() // 4 * 4].view(torch.float32).fill_(float("nan"))
    dirty = mel.mel_spectrogram_many(items)
    assert mel._WS[items[0].device] is ws
    for a, b, c in zip(clean, dirty, one):
        assert bool(torch.isfinite(b).all()) and torch.equal(a, b) and torch.equal(b, c)


def test_more_rows_than_the_fp32_gemm_takes_in_64_row_tiles():
    """8135 rows (more than 63 tiles of 128) put the DFT GEMM of the ragged call on the 128-row LDS-DMA kernel while an item alone runs on 64-row tiles:
    the one size at which the call takes another kernel than the one-prompt path."""
    from covomix_amd import mel, ops
    lengths = [80000] * 16 + [16123]
    rows = sum(-(-(n + 320) // 160) for n in lengths)
    assert ops.gemm_f32_form(rows, 482, 480) == "T128_DMA" and ops.gemm_f32_form(80000 // 160, 482, 480) == "T64"
    long = signal(80000).cuda()
    items = [signal(80000, seed=100 + i).cuda() if i not in (0, 9) else long for i in range(16)] + [signal(16123).cuda()]
    got = mel.mel_spectrogram_many(items)
    ref = mel.mel_spectrogram(long)
    assert torch.equal(got[0], ref) and torch.equal(got[9], ref)
    assert torch.equal(got[16], mel.mel_spectrogram(items[16])) and torch.equal(got[5], mel.mel_spectrogram(items[5]))


def _upload_table(tab):
    return torch.from_numpy(tab.words).cuda()


def test_pack_kernel_against_the_numpy_restatement():
    from covomix_amd import _lib, mel, ops
    lib = _lib.load()
    sr = 8000
    rates = [8000, 16000, 8000, 44100, 4000, 8000, 16000]
    n_raw = [161, 2001, 481, 9000, 700, 16123, 641]
    raws = [signal(n, float(r)).numpy() * (1.5 if i == 5 else 1.0) for i, (n, r) in enumerate(zip(n_raw, rates))]     # item 5 clips
    other = tuple(dict.fromkeys(r for r in rates if r != sr))
    geom, taps = mel._banks_host(other, sr)
    bank = [other.index(r) if r != sr else -1 for r in rates]
    tab = mel.mel_item_table(n_raw, bank, geom)
    raw = np.zeros(tab.raw_floats, dtype=np.float32)
    for x, o in zip(raws, tab.raw_off):
        raw[int(o):int(o) + len(x)] = x
    raw_d, taps_d, items_d = torch.from_numpy(raw).cuda(), torch.from_numpy(taps).cuda(), _upload_table(tab)
    packed = torch.full((tab.packed_floats,), float("nan"), device="cuda")
    _lib.check(lib.cvx_mel_pack_f32(raw_d.data_ptr(), taps_d.data_ptr(), tab.words.ctypes.data, items_d.data_ptr(), tab.words.size, tab.n,
                                    packed.data_ptr(), ops._stream()), "cvx_mel_pack_f32")
    got = packed.cpu().numpy()
    want = mel_items.pack(raws, 480, 160, rates, sr)
    assert got.shape == want.shape and np.isfinite(got).all()
    bounds = [int(o) for o in tab.offsets] + [tab.packed_floats]
    for b in range(tab.n):
        g, w = got[bounds[b]:bounds[b + 1]], want[bounds[b]:bounds[b + 1]]
        n_pad = int(tab.samples[b]) + 2 * tab.pad
        assert (g[n_pad:] == 0).all(), f"item {b}: slack not zero"
        err = float(np.abs(g - w).max())
        print("item", b, "rate", rates[b], "max abs err", err)
        if rates[b] == sr:
            assert np.array_equal(g, w), f"stored item {b}"
        else:
            assert err < 2e-6, f"resampled item {b}"
    assert np.abs(got).max() == 1.0                                      # the clipped item reaches the clamp


def test_log_gather_kernel_against_the_one_prompt_kernel():
    from covomix_amd import _lib, mel, ops
    lib = _lib.load()
    tab = mel.mel_item_table([100, 500, 90, 321, 100, 4000], n_fft=320, hop=160)
    g = torch.Generator().manual_seed(3)
    proj = (torch.rand(tab.rows, 80, generator=g) * 2e-4 - 2e-5).cuda()                 # some below the 1e-5 floor, some negative
    out = torch.full((80 * tab.M + 4,), SENTINEL, device="cuda")
    items_d = _upload_table(tab)
    _lib.check(lib.cvx_mel_log_gather_f32(proj.data_ptr(), tab.words.ctypes.data, items_d.data_ptr(), tab.words.size, tab.n, 80,
                                          out.data_ptr(), ops._stream()), "cvx_mel_log_gather_f32")
    assert (out[80 * tab.M:] == SENTINEL).all()
    for b in range(tab.n):
        T, s = int(tab.frames[b]), int(tab.slot[b])
        got = out[80 * int(tab.cu[b]): 80 * (int(tab.cu[b]) + T)].view(80, T)
        if T == 0:
            continue
        rows = proj[s:s + T].contiguous()
        ref = torch.empty(80, T, device="cuda")
        _lib.check(lib.cvx_mel_log_transpose_f32(rows.data_ptr(), ref.data_ptr(), T, 80, ops._stream()), "cvx_mel_log_transpose_f32")
        assert torch.equal(got, ref)
        assert float((got.cpu() - torch.log(rows.cpu().clamp(min=1e-5)).T).abs().max()) < 1e-5


def test_files_of_mixed_rates_and_sample_types_in_one_call(tmp_path):
    from scipy.io.wavfile import write
    from covomix_amd import mel
    sig = lambda n, r: signal(n, float(r)).numpy()
    stereo = np.stack((sig(12001, 16000), 0.5 * sig(12001, 16000)[::-1]), axis=1)
    files = [("a.wav", 8000, (sig(8000, 8000) * 32767).astype(np.int16), None),
             ("b.wav", 16000, (stereo * 32767).astype(np.int16), None),                  # stereo, channel mean
             ("c.wav", 16000, (stereo * 32767).astype(np.int16), 1),                     # stereo, channel 1
             ("d.wav", 44100, (sig(22051, 44100) * (2 ** 31 - 1)).astype(np.int32), None),
             ("e.wav", 4000, sig(3000, 4000).astype(np.float32), None),
             ("f.wav", 8000, (sig(16123, 8000) * 32767).astype(np.int16), None)]
    paths, chans = [], []
    for name, rate, data, ch in files:
        write(str(tmp_path / name), rate, data)
        paths.append(str(tmp_path / name))
        chans.append(ch)
    got = mel.extract_mel_many(paths, channel_idx=chans)
    for p, ch, m in zip(paths, chans, got):
        ref = mel.extract_mel(p, channel_idx=ch)
        assert not m.is_cuda and m.shape == ref.shape and m.shape[1] > 0
        assert torch.equal(m, ref), (os.path.basename(p), float((m - ref).abs().max()))
    for ch in (None, 0):                                                  # one value for all entries
        got = mel.extract_mel_many(paths, channel_idx=ch)
        for p, m in zip(paths, got):
            assert torch.equal(m, mel.extract_mel(p, channel_idx=ch)), (os.path.basename(p), ch)
    arr = sig(5000, 8000)
    got = mel.extract_mel_many([arr, torch.from_numpy(arr), paths[0]])    # arrays at `sr` beside a file
    assert torch.equal(got[0], mel.extract_mel(arr)) and torch.equal(got[1], got[0]) and torch.equal(got[2], mel.extract_mel(paths[0]))


def test_reference_fixtures_as_one_two_item_call():
    """Row N3 pin at the reference's other geometry (16 kHz, n_fft = win = 1024, hop 256, fmax 8000)."""
    from conftest import GOLDEN
    from covomix_amd import mel
    g = np.load(os.path.join(GOLDEN, "mel_ref_16k.npz"))
    args = (int(g["n_fft"]), int(g["n_mels"]), int(g["sr"]), int(g["hop"]), int(g["win"]), float(g["fmin"]), float(g["fmax"]))
    wavs = [torch.from_numpy(g[f"wav{i}"].astype(np.float32) / 32768.0).cuda() for i in range(2)]
    got = mel.mel_spectrogram_many(wavs, *args)
    for i in range(2):
        ref = torch.from_numpy(g[f"mel{i}"])
        err = float((got[i].cpu() - ref).abs().max())
        print("mel fixture", i, "max abs err (ragged call)", err)
        assert got[i].shape == ref.shape and err < 5e-5
        assert torch.equal(got[i], mel.mel_spectrogram(wavs[i], *args))


def test_items_of_no_frames():
    from covomix_amd import mel
    lengths = [100, 500, 90, 321, 100]
    wavs = [signal(n).cuda() for n in lengths]
    kw = dict(n_fft=320, hop_size=160, win_size=320)
    got = mel.mel_spectrogram_many(wavs, **kw)
    for n, w, m in zip(lengths, wavs, got):
        if n in (100, 90):
            assert m.shape == (80, 0)
        else:
            assert m.shape == (80, (n + 160 - 320) // 160 + 1) and torch.equal(m, mel.mel_spectrogram(w, **kw))
    assert [m.shape for m in mel.mel_spectrogram_many([wavs[0], wavs[2]], **kw)] == [(80, 0), (80, 0)]       # nothing to launch at all
    assert [tuple(m.shape) for m in mel.extract_mel_many([w.cpu().numpy() for w in wavs], **kw)] == [tuple(m.shape) for m in got]


def test_a_list_cut_into_three_calls_gives_the_same_tensors():
    from covomix_amd import mel
    lengths = [4000, 161, 3000, 2500, 4100, 700, 3999]
    arrays = [signal(n).numpy() for n in lengths]
    budget = 9000                                                         # packed sizes 4320, 480, 3360, 2880, 4480, 1120, 4320
    groups = mel.split_batches(lengths, budget)
    assert groups == [[0, 1, 2], [3, 4, 5], [6]]
    whole = mel.extract_mel_many(arrays)
    cut = mel.extract_mel_many(arrays, max_batch_samples=budget)
    assert len(cut) == len(whole) == len(lengths)
    for n, a, b in zip(lengths, whole, cut):
        assert a.shape == (80, n // 160) and torch.equal(a, b)


def test_refusals_leave_the_output_untouched():
    from covomix_amd import _lib, mel, ops
    lib = _lib.load()
    wavs = [signal(n) for n in (481, 3001, 161)]
    tab = mel.mel_item_table([w.numel() for w in wavs])
    raw = torch.zeros(tab.raw_floats)
    for w, o in zip(wavs, tab.raw_off):
        raw[int(o):int(o) + w.numel()] = w
    raw = raw.cuda()
    dft, basis, _nb, _nbp = mel._constants(raw.device, 8000, 480, 480, 80, 0.0, 4000.0)
    need = int(lib.cvx_mel_workspace_bytes_many(tab.words.ctypes.data, tab.words.size, tab.n, 80))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = torch.full((80 * tab.M,), SENTINEL, device="cuda")
    good_dev = _upload_table(tab)

    def call(host, dev, ws_bytes):
        return lib.cvx_mel_spectrogram_many_f32(raw.data_ptr(), None, dft.data_ptr(), basis.data_ptr(), 80, host.ctypes.data, dev.data_ptr(),
                                                host.size, tab.n, out.data_ptr(), ws.data_ptr(), ws_bytes, ops._stream())
    for word in (3, 16 + 8 + 3, 16 + 8 * 2 + 5):                          # the hop, an item's slot, an item's cu
        bad_dev = good_dev.clone()
        bad_dev[word] += 1
        assert call(tab.words, bad_dev, need) == -22, f"device word {word}"
        bad_host = tab.words.copy()
        bad_host[word] += 1
        assert call(bad_host, good_dev, need) == -22, f"host word {word}"
    assert call(tab.words, good_dev, need - 1) == -22                     # a short workspace
    short = np.asarray([481, 160, 161], dtype=np.int64)                   # an item with n_b == pad: there is no table to call with
    assert lib.cvx_mel_items_words(480, 160, short.ctypes.data, None, None, 0, 3) == -1
    with pytest.raises(ValueError, match="item 1 "):
        mel.mel_spectrogram_many([signal(481).cuda(), signal(160).cuda(), signal(161).cuda()])
    with pytest.raises(_lib.CovomixHipError):
        mel.mel_spectrogram_many([signal(481).cuda(), signal(481)])       # a CPU tensor
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()), "a refused call wrote into the output"
    assert call(tab.words, good_dev, need) == 0                           # and the same call, untampered, runs
    for w, m in zip(wavs, mel._views(out, tab, 80)):
        assert torch.equal(m, mel.mel_spectrogram(w.cuda()))


def test_cli_pre_pass_gives_load_prompt_the_same_prompts(tmp_path, monkeypatch):
    from scipy.io.wavfile import write
    from covomix_amd import generation, mel
    monkeypatch.setattr(generation, "_HUBERT", None)
    monkeypatch.setattr(generation, "_PROMPT_MELS", {})
    d = str(tmp_path)
    names = [f"p{i}" for i in range(6)]
    for i, n in enumerate(names):
        rate = 16000 if i % 2 else 8000
        write(os.path.join(d, n + ".wav"), rate, (signal(rate + 777 * i, float(rate)).numpy() * 32767).astype(np.int16))
        np.save(os.path.join(d, n + ".hubert_code.npy"), np.arange(200) % 50)
    np.save(os.path.join(d, "p4.mel.npy"), np.full((80, 9), -3.0, dtype=np.float32))
    before = [generation._load_prompt(d, n) for n in names]
    calls = []
    real = mel.extract_mel_many
    monkeypatch.setattr(mel, "extract_mel_many", lambda paths: calls.append([os.path.basename(p) for p in paths]) or real(paths))
    assert generation.preextract_prompt_mels(d, names + names[:2], 4) == 5
    assert calls == [["p0.wav", "p1.wav", "p2.wav", "p3.wav"], ["p5.wav"]]                # p4 has its mel on disk: not extracted
    assert (d, "p4") not in generation._PROMPT_MELS and len(generation._PROMPT_MELS) == 5
    monkeypatch.setattr(mel, "extract_mel", None)                         # from here on a prompt that is re-extracted would raise
    for n, (tok0, mel0) in zip(names, before):
        tok1, mel1 = generation._load_prompt(d, n)
        assert torch.equal(tok0, tok1) and torch.equal(mel0, mel1), n
