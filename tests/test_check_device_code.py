"""tools/check_device_code.py --compare: the parsing and comparison of two disassembly texts (no build, no GPU, no library)."""
from __future__ import annotations

import importlib.util
from pathlib import Path

_spec = importlib.util.spec_from_file_location("check_device_code", Path(__file__).resolve().parent.parent / "tools" / "check_device_code.py")
cdc = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cdc)


def _dis(kernels: dict[str, list[str]], base: int = 0x1900, name: str = "a.co") -> str:
    """A text in the layout of `llvm-objdump -d` on an amdgcn code object: header lines, `<address> <symbol>:` lines, and per instruction
    a tab, the instruction, padding, `// <address>: <encoding words>`."""
    out = ["", f"{name}:\tfile format elf64-amdgpu", "", "Disassembly of section .text:", ""]
    addr = base
    for sym, insts in kernels.items():
        out.append(f"{addr:016x} <{sym}>:")
        for k, inst in enumerate(insts):
            out.append(f"\t{inst:<58} // {addr:012X}: {(0xBF800000 + 7 * addr + k) & 0xFFFFFFFF:08X}")
            addr += 4
        out.append("")
        addr = (addr + 0xFF) & ~0xFF
    return "\n".join(out)


K1 = ["s_load_dwordx2 s[0:1], s[4:5], 0x0", "s_waitcnt lgkmcnt(0)", "v_add_f32_e32 v2, v2, v3", "global_store_dword v4, v2, s[0:1]", "s_endpgm"]
K2 = ["v_lshlrev_b32_e32 v4, 2, v10", "s_cbranch_execz 10", "v_mov_b32_e32 v0, 0", "s_endpgm"]


def test_listing_drops_addresses_and_encodings():
    got = cdc.kernel_listings(_dis({"_Z2k1v": K1, "_Z2k2v": K2}))
    assert got == {"_Z2k1v": K1, "_Z2k2v": K2}


def test_equal_kernels():
    d = _dis({"_Z2k1v": K1, "_Z2k2v": K2})
    assert cdc.compare_disassembly(d, d) == ([], [], [], 2)


def test_addresses_encodings_and_file_name_are_ignored():
    a = _dis({"_Z2k1v": K1, "_Z2k2v": K2}, base=0x1900, name="parent.co")
    b = _dis({"_Z2k1v": K1, "_Z2k2v": K2}, base=0x7300, name="tree.co")
    assert a != b
    assert cdc.compare_disassembly(a, b) == ([], [], [], 2)


def test_one_kernel_differs_by_one_instruction():
    changed = list(K1)
    changed[2] = "v_add_f32_e32 v27, v0, v1"
    a, b = _dis({"_Z2k1v": K1, "_Z2k2v": K2}), _dis({"_Z2k1v": changed, "_Z2k2v": K2})
    assert cdc.compare_disassembly(a, b) == ([("_Z2k1v", 5, 5, 1)], [], [], 2)
    longer = K2[:2] + ["s_nop 0"] + K2[2:]
    assert cdc.compare_disassembly(a, _dis({"_Z2k1v": K1, "_Z2k2v": longer})) == ([("_Z2k2v", 4, 5, 1)], [], [], 2)


def test_kernel_missing_on_one_side():
    both, one = _dis({"_Z2k1v": K1, "_Z2k2v": K2}), _dis({"_Z2k1v": K1})
    assert cdc.compare_disassembly(both, one) == ([], ["_Z2k2v"], [], 2)
    assert cdc.compare_disassembly(one, both) == ([], [], ["_Z2k2v"], 2)
