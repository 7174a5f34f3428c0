#!/usr/bin/env python3
"""Compare the gfx950 code objects of two builds of libmsda_hip.so, symbol by symbol (no GPU needed).

    python tools/compare_code_objects.py OLD.so NEW.so

The device code objects are taken out of each library's offload bundles (`llvm-objdump --offloading`, as
tests/test_host_api.py does for its spill check) and disassembled with `llvm-objdump -d`; addresses, encodings,
branch-target comments and the padding behind a symbol's last instruction are dropped, and what is left is compared
symbol by symbol.  Prints the number of identical / different / missing / added symbols and, for every different one,
both sides' VGPR / SGPR / spill / scratch / LDS figures from the metadata notes and the instruction counts.
Exit status 0 only when no symbol is different or missing: a refactor of device code that claims "same machine code"
is checked with one command.  Limitation: the padding is recognised by name (trailing s_nop / s_code_end lines), so two
symbols that differ ONLY in such trailing instructions compare equal.
"""
import argparse
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("MSDA_LLVM_BIN", "/opt/rocm/lib/llvm/bin")
NOTE_KEYS = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
             "group_segment_fixed_size")
PADDING = ("s_nop", "s_code_end")


def code_objects(lib, workdir):
    """The gfx950 code objects of `lib`, unbundled into `workdir`."""
    copy = os.path.join(workdir, "lib.so")
    shutil.copy(lib, copy)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", copy], cwd=workdir, check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)  # one file per bundle next to the copy
    objs = sorted(glob.glob(copy + ".*gfx950"))
    if not objs:
        sys.exit(f"{lib}: no gfx950 code object found")
    return objs


def disassembly(obj):
    """symbol -> list of instructions (mnemonic + operands, nothing position-dependent)."""
    text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", obj], capture_output=True,
                          text=True, check=True).stdout
    syms, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-fA-F]+ <(.+)>:\s*$", line)
        if m:
            cur = syms.setdefault(m.group(1), [])
            continue
        if cur is None or not line.strip() or line.startswith("Disassembly"):
            continue
        ins = " ".join(line.split("//", 1)[0].split())  # (the comment holds the address, the encoding and branch targets)
        if ins:
            cur.append(ins)
    for body in syms.values():
        while body and body[-1].split()[0] in PADDING:
            body.pop()
    return syms


def notes(obj):
    """kernel symbol -> {note key: value} from the code object's metadata."""
    text = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", obj], capture_output=True, text=True,
                          check=True).stdout
    fields = [(len(m.group(1)), m.group(1).endswith("- "), m.group(2), m.group(3))
              for m in (re.match(r"^(\s*(?:- )?)\.(\w+):\s*(.*)$", ln) for ln in text.splitlines()) if m]
    cols = [c for c, _, k, _ in fields if k == "vgpr_count"]
    out, cur = {}, None
    for col, first, key, val in fields:
        if not cols or col != cols[0]:
            continue  # (an argument's fields: deeper)
        if first:
            cur = {}
        if cur is None:
            continue
        if key == "name":
            out[val.strip("'\"")] = cur
        elif key in NOTE_KEYS:
            cur[key] = val
    return out


def load(lib):
    with tempfile.TemporaryDirectory() as tmp:
        code, meta = {}, {}
        for obj in code_objects(lib, tmp):
            for name, body in disassembly(obj).items():
                code.setdefault(name, []).append(body)  # (a symbol emitted by several translation units: every copy)
            meta.update(notes(obj))
    for bodies in code.values():
        bodies.sort()
    return code, meta


def figures(meta, code, name):
    m = meta.get(name, {})
    return ("vgpr {} sgpr {} vgpr-spill {} sgpr-spill {} scratch {} lds {} instructions {}".format(
        m.get("vgpr_count", "-"), m.get("sgpr_count", "-"), m.get("vgpr_spill_count", "-"), m.get("sgpr_spill_count", "-"),
        m.get("private_segment_fixed_size", "-"), m.get("group_segment_fixed_size", "-"),
        "+".join(str(len(b)) for b in code[name])))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--names", action="store_true", help="also list the missing and added symbols by name")
    args = ap.parse_args()
    old_code, old_meta = load(args.old)
    new_code, new_meta = load(args.new)
    missing = sorted(set(old_code) - set(new_code))
    added = sorted(set(new_code) - set(old_code))
    common = sorted(set(old_code) & set(new_code))
    different = [n for n in common if old_code[n] != new_code[n]]
    print(f"symbols: {len(common) - len(different)} identical, {len(different)} different, {len(missing)} missing, "
          f"{len(added)} added")
    for n in different:
        print(f"DIFFERENT {n}")
        print(f"    old: {figures(old_meta, old_code, n)}")
        print(f"    new: {figures(new_meta, new_code, n)}")
    if args.names or len(missing) + len(added) <= 20:
        for n in missing:
            print(f"MISSING {n}")
        for n in added:
            print(f"ADDED {n}")
    return 1 if different or missing else 0


if __name__ == "__main__":
    sys.exit(main())
