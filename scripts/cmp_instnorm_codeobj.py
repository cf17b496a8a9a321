"""Device code of the InstanceNorm kernel family in two trees, kernel by kernel (a one-off for refactors of csrc/rx_instnorm.hip,
rx_head.hip, rx_se.hip and the headers they share; no GPU needed).

    python scripts/cmp_instnorm_codeobj.py --parent <checkout of the parent> [--out DIR]

Each file is compiled for gfx950 with the flags of csrc/build.py (device side only), the code object is disassembled, and for
every kernel the instruction stream and the resource numbers of the code-object metadata (VGPRs, SGPRs, scratch bytes, static LDS
bytes) are compared.  Kernels are matched by demangled name without the parameter list, after the renames in RENAMES, so a
parameter that changed its C++ type but not its layout still finds its partner.  Prints one line per kernel and a summary;
--out keeps the per-kernel listings of both trees for diffing by hand."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ap = argparse.ArgumentParser()
ap.add_argument("--parent", required=True)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--files", nargs="*", default=["rx_instnorm.hip", "rx_head.hip", "rx_se.hip"])
ap.add_argument("--out", default=None)
args = ap.parse_args()

CSRC = os.path.join("multi-task-3d-resencoder-unet_amd", "csrc")
sys.path.insert(0, os.path.join(args.root, CSRC))
import build as rxbuild  # noqa: E402

LLVM = os.path.join(os.path.dirname(os.path.dirname(rxbuild.HIPCC)), "llvm", "bin")
RENAMES = [("SeView", "ActView")]
META = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def key_of(demangled):
    """`void k<A, B<C>>(args)` -> `k<A, B<C>>`"""
    s = demangled[5:] if demangled.startswith("void ") else demangled
    depth = 0
    for i, ch in enumerate(s):
        depth += (ch == "<") - (ch == ">")
        if ch == "(" and depth == 0:
            s = s[:i]
            break
    for a, b in RENAMES:
        s = s.replace(a, b)
    return s


def listing(co, demangle):
    cmd = [os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr"] + (["-C"] if demangle else []) + [co]
    out, name = [], None
    for ln in subprocess.check_output(cmd, text=True).splitlines():
        m = re.match(r"^<(.*)>:$", ln)
        if m:
            name = m.group(1)
            out.append((name, []))
        elif name and ln.startswith("\t"):
            out[-1][1].append(re.sub(r"\s+", " ", ln.split("//")[0].strip()))
    return out


def kernels_of(tree, src, tmp):
    co = os.path.join(tmp, src + ".co")
    subprocess.check_call([rxbuild.HIPCC] + rxbuild.FLAGS + ["--cuda-device-only", "--no-gpu-bundle-output", "-c",
                                                            os.path.join(tree, CSRC, src), "-o", co])
    raw, nice = listing(co, False), listing(co, True)
    notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
    meta, cur = {}, None
    for ln in notes.splitlines():
        m = re.match(r"^\s+(?:- )?(\.\w+):\s+(\S+)$", ln)
        if not m:
            continue
        if ln.lstrip().startswith("- .agpr_count"):       # first key of a kernel's entry
            cur = {}
        if cur is not None and m.group(1) in META:
            cur[m.group(1)] = int(m.group(2))
        if cur is not None and m.group(1) == ".name":
            meta[m.group(2)] = cur
    res = {}
    for (mangled, code), (demangled, _) in zip(raw, nice):
        if mangled in meta:                               # device functions that were not inlined have no metadata entry
            res[key_of(demangled)] = (code, tuple(meta[mangled][k] for k in META))
    return res


same, differ, only = 0, [], []
with tempfile.TemporaryDirectory() as tmp:
    for src in args.files:
        os.makedirs(os.path.join(tmp, "a"), exist_ok=True)
        os.makedirs(os.path.join(tmp, "b"), exist_ok=True)
        a, b = kernels_of(args.parent, src, os.path.join(tmp, "a")), kernels_of(args.root, src, os.path.join(tmp, "b"))
        for k in sorted(set(a) | set(b)):
            if k not in a or k not in b:
                only.append((src, k, "parent" if k in a else "this tree"))
                continue
            ident = a[k][0] == b[k][0]
            tag = "same" if ident and a[k][1] == b[k][1] else "DIFFERS"
            print(f"{tag:8s}{src}: {k}  insns {len(a[k][0])}/{len(b[k][0])}  vgpr/sgpr/scratch/lds {a[k][1]} -> {b[k][1]}")
            if tag == "same":
                same += 1
            else:
                differ.append(k)
                if args.out:
                    os.makedirs(args.out, exist_ok=True)
                    stem = re.sub(r"\W+", "_", k)
                    for side, d in (("parent", a), ("new", b)):
                        with open(os.path.join(args.out, f"{stem}.{side}.s"), "w") as f:
                            f.write("\n".join(d[k][0]) + "\n")
for src, k, where in only:
    print(f"ONLY in {where}: {src}: {k}")
print(f"{same} kernels identical, {len(differ)} differ, {len(only)} unmatched")
