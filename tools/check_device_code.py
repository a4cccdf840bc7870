#!/usr/bin/env python3
"""Build-time guard on the gfx950 code objects inside rl_brain_trainer_amd/libkp1.so (called by __graft_entry__.build()).

Round 1 lost a GPU to a "Memory access fault ... on address (nil)" in kp1_step_kernel<double, APPROACH, false> while its reset path
still went through NON-INLINED device functions.  Every device function of the library is meant to be inlined
into its kernel; this script makes that a checked property instead of a convention:

  * no `s_swappc_b64` (device function call) anywhere in the device code;
  * every `s_setpc_b64` is a long-branch expansion (preceded by `s_getpc_b64` in the same kernel), not a return;
  * prints per-kernel scratch (private segment) sizes so a jump in spill volume is visible in the build log.

Exit status 1 on a violation.  `--digest` instead prints one line of SHA-256 digests per code object (see digest()), and
`--compare LIB_A LIB_B` names the kernels whose instruction text differs between two builds (see compare()).  Needs only llvm-objdump / llvm-readelf from /opt/rocm (no GPU).
"""
from __future__ import annotations

import difflib
import hashlib
import re
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

LLVM = Path("/opt/rocm/lib/llvm/bin")


def device_code_objects(lib: Path, work: Path) -> list[Path]:
    copy = work / lib.name
    shutil.copy(lib, copy)
    subprocess.run([str(LLVM / "llvm-objdump"), "--offloading", str(copy)], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, cwd=work)
    return sorted(p for p in work.iterdir() if "amdgcn" in p.name)


def check(lib: Path, verbose: bool = False) -> int:
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for co in device_code_objects(lib, Path(tmp)):
            dis = subprocess.run([str(LLVM / "llvm-objdump"), "-d", str(co)], check=True, capture_output=True, text=True).stdout
            kernel, getpc_seen = "?", False
            for line in dis.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:", line)
                if m:
                    kernel, getpc_seen = m.group(1), False
                    continue
                if "s_getpc_b64" in line:
                    getpc_seen = True
                if "s_swappc_b64" in line:
                    print(f"[check_device_code] device function CALL in {kernel}: {line.strip()}", file=sys.stderr)
                    bad += 1
                if "s_setpc_b64" in line and not getpc_seen:
                    print(f"[check_device_code] s_setpc_b64 without a preceding s_getpc_b64 (a function return?) in {kernel}", file=sys.stderr)
                    bad += 1
            if verbose:
                notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], check=True, capture_output=True, text=True).stdout
                names = re.findall(r"\.name:\s+(\S+)", notes)
                sizes = re.findall(r"\.private_segment_fixed_size:\s+(\d+)", notes)
                for n, s in zip(names, sizes):
                    if int(s) > 0:
                        print(f"[check_device_code] scratch {int(s):5d} B/lane  {n[:100]}")
    return bad


def digest(lib: Path) -> int:
    """Per code object: SHA-256 of its whole disassembly (without the line naming the file) and of its notes; equal for equal device code."""
    with tempfile.TemporaryDirectory() as tmp:
        for co in device_code_objects(lib, Path(tmp)):
            dis, notes = (subprocess.run([str(LLVM / t), f, str(co)], check=True, capture_output=True, text=True).stdout for t, f in (("llvm-objdump", "-d"), ("llvm-readelf", "--notes")))
            dis = "\n".join(line for line in dis.splitlines() if "file format" not in line)
            print(co.name, "disassembly", hashlib.sha256(dis.encode()).hexdigest(), "notes", hashlib.sha256(notes.encode()).hexdigest())
    return 0


def kernel_listings(dis: str) -> dict[str, list[str]]:
    """Instruction text per symbol of one `llvm-objdump -d` output: the address and everything from `//` on (the encoding) are dropped."""
    out: dict[str, list[str]] = {}
    cur = None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        text = re.sub(r"^\s*[0-9a-f]+:\s", "", line.split("//")[0]).strip()
        # `...` is objdump's mark for the zero padding up to the next symbol's alignment: it appears behind a kernel once another one follows
        # it in the code object, and is no instruction
        if cur is not None and text and text != "...":
            cur.append(text)
    return out


def compare_disassembly(dis_a: str, dis_b: str) -> tuple[list[tuple[str, int, int, int]], list[str], list[str], int]:
    """(differing kernels as (name, instructions in A, in B, differing lines), only in A, only in B, kernels in A or B).  Text equality only."""
    a, b = kernel_listings(dis_a), kernel_listings(dis_b)
    differ = []
    for name in sorted(a.keys() & b.keys()):
        if a[name] != b[name]:
            ops = difflib.SequenceMatcher(None, a[name], b[name], autojunk=False).get_opcodes()
            differ.append((name, len(a[name]), len(b[name]), sum(max(i2 - i1, j2 - j1) for tag, i1, i2, j1, j2 in ops if tag != "equal")))
    return differ, sorted(a.keys() - b.keys()), sorted(b.keys() - a.keys()), len(a.keys() | b.keys())


def compare(lib_a: Path, lib_b: Path) -> int:
    """Per code object and kernel symbol: which kernels of LIB_A and LIB_B differ in instruction text.  Exit status 1 when any does.
    Code objects are paired by the kernel symbols they share (a translation unit added to or removed from one build shifts the numbering);
    the kernels of a code object without a partner are listed as being in one build only."""
    n_bad = n_all = 0
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        dis_a, dis_b = ([(co.name, subprocess.run([str(LLVM / "llvm-objdump"), "-d", str(co)], check=True, capture_output=True, text=True).stdout)
                         for co in device_code_objects(lib, Path(tmp))] for lib, tmp in ((lib_a, ta), (lib_b, tb)))
        names_b = [set(kernel_listings(d)) for _, d in dis_b]
        free_b = set(range(len(dis_b)))
        for name_a, d_a in dis_a:
            shared = {j: len(set(kernel_listings(d_a)) & names_b[j]) for j in free_b}
            j = max(shared, key=shared.get, default=None)
            if j is None or shared[j] == 0:
                name, d_b = "-", ""
            else:
                free_b.discard(j)
                name, d_b = dis_b[j]
            if name != name_a:
                print(f"[check_device_code] {name_a} of A against {name} of B")
            differ, only_a, only_b, total = compare_disassembly(d_a, d_b)
            for kernel, na, nb, nd in differ:
                print(f"[check_device_code] {name_a}: differs  A {na:6d}  B {nb:6d} instructions, {nd:6d} lines differ  {kernel}")
            for side, names in (("A", only_a), ("B", only_b)):
                for kernel in names:
                    print(f"[check_device_code] {name_a}: only in {side}  {kernel}")
            n_bad += len(differ) + len(only_a) + len(only_b)
            n_all += total
        for j in sorted(free_b):
            for kernel in sorted(names_b[j]):
                print(f"[check_device_code] {dis_b[j][0]}: only in B  {kernel}")
            n_bad += len(names_b[j])
            n_all += len(names_b[j])
    print(f"[check_device_code] {n_bad} of {n_all} kernels differ")
    return 1 if n_bad else 0


def main() -> int:
    if "--compare" in sys.argv:
        libs = [Path(a) for a in sys.argv[1:] if not a.startswith("-")]
        if len(libs) != 2:
            print("usage: check_device_code.py --compare LIB_A LIB_B", file=sys.stderr)
            return 2
        return compare(*libs)
    lib = Path(next((a for a in sys.argv[1:] if not a.startswith("-")), Path(__file__).resolve().parent.parent / "rl_brain_trainer_amd" / "libkp1.so"))
    if "--digest" in sys.argv:
        return digest(lib)
    bad = check(lib, verbose="-v" in sys.argv)
    if bad:
        print(f"[check_device_code] {bad} violation(s) in {lib}", file=sys.stderr)
        return 1
    print(f"[check_device_code] {lib.name}: no device function calls")
    return 0


if __name__ == "__main__":
    sys.exit(main())
