"""Compare the kernels of two device-only assembly files (`hipcc <build.py's BASE_FLAGS> --cuda-device-only -S x.hip -o x.s`), parent first.

Per kernel symbol the instruction text is compared up to comments, directives and label numbers.  Kernels whose text differs are listed with
instruction count, VGPRs (.amdhsa_next_free_vgpr; the allocation granule is 8), LDS bytes and private segment of both sides.  Needs no GPU.

  python tools/kernel_text_diff.py parent.s change.s
"""
import re
import shutil
import subprocess
import sys

FIELDS = (("vgprs", "next_free_vgpr"), ("lds", "group_segment_fixed_size"), ("private", "private_segment_fixed_size"))


def kernels(path):
    text, res, cur, desc = {}, {}, None, {}
    for ln in open(path):
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            cur = m.group(1)
            text[cur] = []
            continue
        m = re.match(r"\s*\.amdhsa_kernel (\S+)", ln)
        if m:
            cur = None
            res[m.group(1)] = desc = {}
            continue
        m = re.match(r"\s*\.amdhsa_(\w+) (\d+)", ln)
        if m and not cur:
            desc[m.group(1)] = int(m.group(2))
        if cur is None:
            continue
        if ln.startswith(".Lfunc_end"):
            cur = None
            continue
        s = ln.split(";")[0].strip()
        if not s or (s.startswith(".") and not s.startswith(".LBB")):
            continue
        text[cur].append(re.sub(r"\.LBB\d+_\d+", ".LBB", s))
    return {k: (v, res[k]) for k, v in text.items() if k in res}


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return {n: re.sub(r"^void |\(anonymous namespace\)::|\(.*", "", o) for n, o in zip(names, out)}


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    names = demangle(sorted(set(a) | set(b)))
    same = [k for k in a if k in b and a[k][0] == b[k][0]]
    print(f"kernel symbols: parent {len(a)}, change {len(b)}; identical instruction text: {len(same)}")
    for k in sorted(set(a) ^ set(b)):
        print(("only in the parent: " if k in a else "only in the change: ") + names[k])
    print("identical:")
    for k in same:
        print("  " + names[k])
    print("moved (parent -> change):")
    for k in a:
        if k in b and k not in same:
            cols = [f"instructions {len(a[k][0])} -> {len(b[k][0])}"]
            cols += [f"{label} {a[k][1][field]} -> {b[k][1][field]}" for label, field in FIELDS]
            granule = "same granule" if -(-a[k][1]["next_free_vgpr"] // 8) == -(-b[k][1]["next_free_vgpr"] // 8) else "OTHER GRANULE"
            print(f"  {names[k]}: " + ", ".join(cols) + f" ({granule})")


if __name__ == "__main__":
    main()
