#!/usr/bin/env python3
"""Do the kernels of two source trees compile to the same instructions?  Device-only compile of the named HIP units of both trees with the Makefile's flags,
llvm-objdump of the gfx950 code objects, one hash per kernel over its disassembly (addresses and encodings left out), and one line per kernel: same / CHANGED /
NEW / GONE.  tools/kernel_resources.sh compares register and LDS figures; this compares the code.

  python tools/kernel_code_compare.py <other tree> [unit ...]          (default units: rf_sums rf_denoise; the other tree is usually a checkout of the parent commit)
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
FLAGS = ("-std=c++20 -O3 -fPIC -ffp-contract=off -fno-fast-math -fvisibility=hidden --offload-arch=gfx950 -fhip-fp32-correctly-rounded-divide-sqrt "
         "-fno-gpu-flush-denormals-to-zero --offload-device-only").split()


def kernels(tree, unit, tmp):
    obj = os.path.join(tmp, unit + ".o")
    subprocess.check_call([ROCM + "/bin/hipcc"] + FLAGS + ["-I" + os.path.join(tree, "include"), "-c", os.path.join(tree, "rayfinder_amd", "csrc", unit + ".hip"), "-o", obj])
    subprocess.check_call([ROCM + "/lib/llvm/bin/clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + obj,
                           "--output=" + obj + ".co"])
    text = subprocess.run([ROCM + "/lib/llvm/bin/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", obj + ".co"], capture_output=True, text=True, check=True).stdout
    out, name = {}, None
    for line in text.splitlines():
        m = re.match(r"^\S* ?<(\S+)>:", line)
        if m:
            name = m.group(1)
            out[name] = []
        elif name:
            out[name].append(re.sub(r"//.*", "", line).strip())
    return {k: hashlib.sha1("\n".join(v).encode()).hexdigest()[:12] for k, v in out.items()}


def main():
    here = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    other = os.path.abspath(sys.argv[1])
    demangle = lambda n: subprocess.run(["c++filt", n], capture_output=True, text=True).stdout.strip().replace("rf::(anonymous namespace)::", "").split("(")[0]  # noqa: E731
    for unit in sys.argv[2:] or ["rf_sums", "rf_denoise"]:
        with tempfile.TemporaryDirectory() as a, tempfile.TemporaryDirectory() as b:
            theirs, ours = kernels(other, unit, a), kernels(here, unit, b)
        print(f"{unit}.hip: {len(theirs)} kernels in the other tree, {len(ours)} in this one")
        for k in sorted(set(theirs) | set(ours)):
            state = "same" if theirs.get(k) == ours.get(k) else "NEW" if k not in theirs else "GONE" if k not in ours else "CHANGED"
            print(f"  {state:8s}{demangle(k)}")


if __name__ == "__main__":
    main()
