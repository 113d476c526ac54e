#!/usr/bin/env python3
"""Dev: the prompt mel of N wav files - mel.extract_mel_many (one ragged call) against a loop of mel.extract_mel over the same files,
N = 1, 2, 4, 8, 16, 32, for (1) 10-s prompts at 8 kHz, (2) 10-s prompts at 16 kHz (resampled to 8 kHz on the GPU) and (3) a 3 - 10 s mix
at 8 kHz.  The files are int16 wavs written from a seed into a temporary directory.  One process; per N the two forms alternate (loop,
many, loop, many, ...) for ROUNDS (9) rounds after WARM (2) untimed ones; host wall time from the first file read to the last mel on the
host (file reading, uploads and the final copies included), device idle before and after.  Reported: the median over the rounds (and
min / max), ms per prompt, and the effective shader clock of each side's timed regions (ops.clock_stamps, median over the rounds).
Before anything is timed every file's mel from the ragged call is checked to be torch.equal to extract_mel's.
    ROUNDS=9 WARM=2 NS=1,2,4,8,16,32 OUT=profile.txt python tools/bench_mel.py"""
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from covomix_amd import mel, ops  # noqa: E402

ROUNDS, WARM = int(os.environ.get("ROUNDS", "9")), int(os.environ.get("WARM", "2"))
NS = [int(v) for v in os.environ.get("NS", "1,2,4,8,16,32").split(",")]
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def write_files(d, tag, rate, seconds):
    from scipy.io.wavfile import write
    paths = []
    for i, sec in enumerate(seconds):
        n = int(round(sec * rate))
        rng = np.random.default_rng(1000 * rate + i)
        t = np.arange(n) / rate
        y = 0.4 * np.sin(2 * np.pi * 440 * t) + 0.2 * np.sin(2 * np.pi * 1333 * t + 1.0) + 0.05 * rng.standard_normal(n)
        p = os.path.join(d, f"{tag}_{i:02d}.wav")
        write(p, rate, (np.clip(y, -1, 1) * 32767).astype(np.int16))
        paths.append(p)
    return paths


def timed(fn):
    torch.cuda.synchronize()
    c0 = ops.clock_stamps()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    clk = ops.clock_from_stamps(c0, ops.clock_stamps())
    return dt, clk.get("mhz", float("nan")), out


def cell(paths):
    loop = lambda: [mel.extract_mel(p) for p in paths]
    many = lambda: mel.extract_mel_many(paths)
    for _ in range(WARM):
        a, b = loop(), many()
    assert all(torch.equal(x, y) for x, y in zip(a, b)), "the ragged call differs from extract_mel"
    tl, tm, cl, cm = [], [], [], []
    for _ in range(ROUNDS):
        dt, mhz, _ = timed(loop)
        tl.append(dt * 1e3), cl.append(mhz)
        dt, mhz, _ = timed(many)
        tm.append(dt * 1e3), cm.append(mhz)
    return tl, tm, statistics.median(cl), statistics.median(cm)


def table(title, paths):
    say(title)
    say("      N    loop ms/prompt (min .. max)     clock    many ms/call (min .. max)       many ms/prompt   clock    many / loop")
    for n in NS:
        tl, tm, cl, cm = cell(paths[:n])
        ml, mm = statistics.median(tl), statistics.median(tm)
        say(f"      {n:<4d} {ml / n:7.3f} ({min(tl) / n:7.3f} .. {max(tl) / n:7.3f})   {cl:5.0f}    {mm:7.3f} ({min(tm):7.3f} .. {max(tm):7.3f})"
            f"     {mm / n:7.3f}          {cm:5.0f}    {mm / ml:6.3f}")
    say()


def main():
    assert torch.cuda.is_available(), "bench_mel.py measures on the GPU: there is nothing to time without one"
    nmax = max(NS)
    with tempfile.TemporaryDirectory() as d:
        mix = np.random.default_rng(0).uniform(3.0, 10.0, size=nmax)
        sets = [("(1) 10-s prompts, 8 kHz int16 files (500 frames each)", write_files(d, "a", 8000, [10.0] * nmax)),
                ("(2) 10-s prompts, 16 kHz int16 files: resampled to 8 kHz on the GPU (500 frames each)", write_files(d, "b", 16000, [10.0] * nmax)),
                (f"(3) lengths mixed 3 - 10 s, 8 kHz int16 files (numpy default_rng(0).uniform(3, 10), the first N of {nmax})",
                 write_files(d, "c", 8000, list(mix)))]
        say(f"device: {torch.cuda.get_device_name(0)}; {ROUNDS} timed rounds per cell after {WARM} untimed ones, loop and many alternating in one "
            f"process; host wall time, file reading and the final copies included; every mel of the ragged call torch.equal to extract_mel's")
        say()
        for title, paths in sets:
            table(title, paths)
    out = os.environ.get("OUT")
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
