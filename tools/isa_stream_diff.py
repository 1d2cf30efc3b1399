#!/usr/bin/env python3
"""Are the kernels of two gfx950 assembly listings the same instruction streams?  (no GPU needed)

For a refactor that must not change what the device executes: compile the file before and after (hipcc -S --cuda-device-only, or
tools/wino_isa_counts.compile_asm) and compare kernel by kernel.  Of every kernel only its instructions are kept: comments,
directives and labels are dropped, and the function-local block labels .LBB<n>_<m> become .LBB_<m>, since the function index <n>
shifts as soon as a kernel is added to or removed from the file.  The register and memory figures of the kernel metadata (VGPRs,
SGPRs, spills, scratch, static LDS) are compared as well.

usage: isa_stream_diff.py OLD.s NEW.s [NEW2.s ...] [--rename OLD_SYMBOL=NEW_SYMBOL ...]
  Several NEW files: the kernels of OLD were split over them.  --rename: a symbol that is meant to differ (a kernel's mangled name, a
  table that became static); applied to OLD's text as a plain substring replacement, longest first.
Prints one line per kernel -- its instruction count and "equal", or the first differing line -- and exits non-zero on any difference,
a kernel missing on either side included.
"""
import argparse
import re
import sys

META_KEYS = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")


def streams(asm):
    """kernel name -> list of its instruction lines, normalised"""
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    out, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^([A-Za-z_$][\w$.]*):", line)
        if m and m.group(1) in names:
            cur = out[m.group(1)] = []
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        s = line.split(";", 1)[0].strip()
        if not s or s.startswith(".") or s.endswith(":"):          # directive or label (a .LBB operand never starts a line)
            continue
        cur.append(re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", " ".join(s.split())))
    return out


def metadata(asm):
    """kernel name -> the META_KEYS of its entry in amdhsa.kernels (an entry starts at '  - .key:'; its .name comes after some of them)"""
    meta = {}
    for entry in re.split(r"^  - (?=\.)", asm[asm.find("amdhsa.kernels:"):], flags=re.M)[1:]:
        name = re.search(r"^\s*\.name:\s+(\S+)", entry, re.M)
        if name:
            meta[name.group(1)] = {k: int(v) for k, v in re.findall(r"^\s*\.(\w+):\s+(\d+)\s*$", entry, re.M) if k in META_KEYS}
    return meta


def compare(old_asm, new_asms, renames=()):
    """-> [(kernel, instruction count, None or a description of the first difference)], every kernel of either side"""
    for a, b in sorted(renames, key=lambda r: -len(r[0])):
        old_asm = old_asm.replace(a, b)
    old_s, old_m = streams(old_asm), metadata(old_asm)
    new_s, new_m = {}, {}
    for asm in new_asms:
        new_s.update(streams(asm))
        new_m.update(metadata(asm))
    rows = []
    for k in sorted(set(old_s) | set(new_s)):
        a, b = old_s.get(k), new_s.get(k)
        if a is None or b is None:
            rows.append((k, len(a if b is None else b), "only in the %s listing" % ("old" if b is None else "new")))
            continue
        diff = None
        for i, (x, y) in enumerate(zip(a, b)):
            if x != y:
                diff = "instruction %d: '%s' became '%s'" % (i, x, y)
                break
        if diff is None and len(a) != len(b):
            diff = "%d instructions became %d (equal up to the shorter end)" % (len(a), len(b))
        if diff is None and old_m.get(k) != new_m.get(k):
            diff = "metadata %s became %s" % (old_m.get(k), new_m.get(k))
        rows.append((k, len(b), diff))
    return rows


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("old")
    ap.add_argument("new", nargs="+")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    args = ap.parse_args()
    rows = compare(open(args.old).read(), [open(f).read() for f in args.new], [tuple(r.split("=", 1)) for r in args.rename])
    for k, n, diff in rows:
        print("%-110s %5d  %s" % (k, n, diff or "equal"))
    bad = sum(1 for r in rows if r[2])
    print("%d kernels, %d differ" % (len(rows), bad))
    sys.exit(1 if bad or not rows else 0)
