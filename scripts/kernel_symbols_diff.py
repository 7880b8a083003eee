#!/usr/bin/env python3
"""Compare the gfx950 disassembly of kernel symbols between two builds' object files, and list a build's kernel resources.

    kernel_symbols_diff.py diff PARENT.o BUILD.o PATTERN [PATTERN ...]   every symbol of either object whose name holds a PATTERN
    kernel_symbols_diff.py resources BUILD.o PATTERN [PATTERN ...]       VGPRs, SGPRs, LDS, scratch and spills from the metadata note

The objects are what build.py leaves under rusty_sr_amd/build/ (<source>.o): the device code object is taken out of the .hip_fatbin
section.  Instructions are compared as text, without addresses and encodings; a symbol only one side has is reported.  Exit status 1
where a compared symbol differs."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def code_object(obj, tmp):
    fat = os.path.join(tmp, os.path.basename(obj) + ".fatbin")
    co = os.path.join(tmp, os.path.basename(obj) + ".co")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj, os.path.join(tmp, "unused.o")])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + fat, "--output=" + co])
    return co


def symbols(co):
    """name -> list of instruction lines"""
    text = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co], text=True)
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]* ?<(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            cur.append(re.sub(r"\s*//.*$", "", line).strip())
    return out


def resources(co):
    """name -> dict, from the AMDGPU metadata note"""
    text = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
    out, cur = {}, {}
    for line in text.splitlines():
        m = re.match(r"^\s*(?:- )?\.(\w+):\s*(.*)$", line)
        if not m:
            continue
        key, val = m.group(1), m.group(2).strip()
        if line.lstrip().startswith("- ") and key != "name" and "symbol" in cur:
            cur = {}
        cur[key] = val
        if key == "symbol":
            out[val.strip("'").removesuffix(".kd")] = cur
    return out


def wanted(names, patterns):
    return sorted(n for n in names if any(p in n for p in patterns))


def main(argv):
    if len(argv) < 3 or argv[0] not in ("diff", "resources"):
        print(__doc__)
        return 2
    with tempfile.TemporaryDirectory() as tmp:
        if argv[0] == "resources":
            res = resources(code_object(argv[1], tmp))
            for n in wanted(res, argv[2:]):
                r = res[n]
                print(f"{n} vgpr {r.get('vgpr_count')} agpr {r.get('agpr_count', 0)} sgpr {r.get('sgpr_count')} lds {r.get('group_segment_fixed_size')} "
                      f"scratch {r.get('private_segment_fixed_size')} vgpr_spill {r.get('vgpr_spill_count', 0)} sgpr_spill {r.get('sgpr_spill_count', 0)}")
            return 0
        os.makedirs(os.path.join(tmp, "a"))
        os.makedirs(os.path.join(tmp, "b"))
        a, b = symbols(code_object(argv[1], os.path.join(tmp, "a"))), symbols(code_object(argv[2], os.path.join(tmp, "b")))
        names = wanted(set(a) | set(b), argv[3:])
        differing = 0
        for n in names:
            if n not in a or n not in b:
                print(f"ONLY IN {'parent' if n in a else 'build'}: {n}")
                differing += 1
            elif a[n] != b[n]:
                first = next((i for i, (x, y) in enumerate(zip(a[n], b[n])) if x != y), min(len(a[n]), len(b[n])))
                print(f"DIFFERS: {n}: {len(a[n])} / {len(b[n])} instructions, first difference at {first}")
                differing += 1
            else:
                print(f"same ({len(a[n])} instructions): {n}")
        print(f"{len(names)} symbols compared, {differing} differ")
        return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
