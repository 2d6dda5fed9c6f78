#!/usr/bin/env python3
"""Compare the gfx950 kernels of two hipcc object files, kernel by kernel: tools/isa_same.py A.o B.o

Both are disassembled with tools/isa_dump.sh and split at the function symbols; the trailing
"// address <symbol+off>" comments go (they change whenever a kernel moves in the code object). Prints
same / DIFF / gone (only in A) / new (only in B) per kernel; exits 1 on any DIFF or new."""
import os, re, shutil, subprocess, sys, tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
CXXFILT = shutil.which("c++filt")   # names stay mangled without it


def kernels(obj):
    with tempfile.NamedTemporaryFile(suffix=".s") as f:
        subprocess.run([os.path.join(HERE, "isa_dump.sh"), obj, f.name], check=True)
        text = open(f.name).read()
    out, name = {}, None
    for line in text.splitlines():
        head = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if head:
            name = head.group(1)
            out[name] = []
        elif name and line.strip():
            out[name].append(re.sub(r"\s*//.*$", "", line).strip())
    return out


def pretty(names):
    if not names or not CXXFILT:
        return {n: n for n in names}
    res = subprocess.run([CXXFILT] + names, capture_output=True, text=True, check=True).stdout.splitlines()
    return dict(zip(names, res))


a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
names = sorted(set(a) | set(b))
show = pretty(names)
count = {"same": 0, "DIFF": 0, "gone": 0, "new": 0}
for n in names:
    verdict = "gone" if n not in b else "new" if n not in a else "same" if a[n] == b[n] else "DIFF"
    count[verdict] += 1
    print(f"{verdict:4s}  {show[n]}")
print(", ".join(f"{v} {k}" for k, v in count.items()))
sys.exit(1 if count["DIFF"] or count["new"] else 0)
