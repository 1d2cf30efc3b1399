#!/usr/bin/env python3
"""Instruction counts of the compiled Winograd layer kernels, per basic block and per region (no GPU needed).

Compiles csrc/conv_wino.hip (the product's conv_wino_kernel) or, with --dev, csrc/conv_wino_dev.hip (the dev library's earlier forms,
conv_wino_earlier_kernel) to gfx950 assembly with the build recipe's flags and prints, for every instantiation:
  * the kernel metadata (VGPRs, SGPR spills, scratch bytes);
  * per basic block: loop depth and instructions per class (MFMA, VALU, SALU, LDS, DMA, VMEM, branch, wait / barrier / nop);
  * per chunk body -- every depth-2 loop, and every piece of the depth-1 code between two s_barrier that holds MFMAs (a peeled chunk;
    its piece runs on to the next barrier in layout order) -- the same sums and the number of separate VALU runs between its first
    and last MFMA in layout order (a run = VALU instructions with no MFMA between them; the rule of the chunk loop is ONE);
  * the rest of the item loop (the depth-1 pieces without MFMAs): the sums of the item's prologue and epilogue.
A block that a wave-uniform branch skips is still counted: the sums are those of a steady-state chunk / of an item that takes every path,
so an epilogue specialised by branches counts once per variant (--blocks shows the blocks).

usage: wino_isa_counts.py [--dev] [--source FILE.hip] [--blocks] [--asm FILE] [extra hipcc flags, e.g. -fno-slp-vectorize]
  --dev: the dev library's flags and, unless --source says otherwise, conv_wino_dev.hip; --source: a file under csrc/
"""
import collections
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

CLASSES = ("mfma", "valu", "salu", "lds", "dma", "vmem", "branch", "wait")


def compile_asm(dev=False, extra=(), source=None):
    """dev: the dev library's flags.  source: a file under csrc/ (default: conv_wino.hip, the product kernel; with dev, conv_wino_dev.hip, the
    earlier forms -- conv_wino.hip itself is part of both libraries, so it can be asked for with dev=True as well)."""
    from hierarchicalprobabilistic3dhuman_amd import build as B
    source = source or ("conv_wino_dev.hip" if dev else "conv_wino.hip")
    flags = B.FLAGS + (["-DHPS_DEV_BUILD"] if dev else []) + B.FILE_FLAGS.get(source, []) + list(extra)
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "conv_wino.s")
        cmd = [B._hipcc()] + flags + ["-I", B.INCLUDE, "-I", B.CSRC, "-S", "--cuda-device-only", os.path.join(B.CSRC, source), "-o", out]
        subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        with open(out) as f:
            return f.read()


def classify(op):
    if op.startswith("v_mfma") or op.startswith("v_smfma"):
        return "mfma"
    if op.startswith("s_cbranch") or op in ("s_branch", "s_endpgm", "s_setpc_b64"):
        return "branch"
    if op in ("s_waitcnt", "s_barrier", "s_nop", "s_sleep", "s_setprio") or op.startswith("s_waitcnt"):
        return "wait"
    if op.startswith("global_load_lds"):
        return "dma"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("s_"):
        return "salu"
    return None


def kernels(asm):
    """name -> list of blocks; a block = [label, depth, [(class, opcode)], label of its innermost loop's header]."""
    out = collections.OrderedDict()
    cur = None
    for line in asm.splitlines():
        m = re.match(r"^(_Z\w*conv_wino_(?:earlier_)?kernel\w*):", line)
        if m:
            cur = out[m.group(1)] = [["entry", 0, [], "entry"]]
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        m = re.match(r"^(\.LBB\d+_\d+):(.*)$", line) or re.match(r"^; %bb\.(\d+):(.*)$", line)
        if m:
            d = re.search(r"Depth[= ](\d+)", m.group(2))
            h = re.search(r"Header=(BB\d+_\d+)", m.group(2))
            cur.append([m.group(1), int(d.group(1)) if d else 0, [], ".L" + h.group(1) if h else m.group(1)])
            continue
        d = re.match(r"^\s*;\s+(?:Child|=>)", line)
        if d:                                                  # loop-header comment lines after a label carry its own depth
            dd = re.search(r"=>\s*This (?:Inner )?Loop Header: Depth=(\d+)", line)
            if dd:
                cur[-1][1] = int(dd.group(1))
            continue
        s = line.strip()
        if not s or s.startswith((";", ".", "//")):
            continue
        op = s.split()[0]
        c = classify(op)
        if c:
            cur[-1][2].append((c, op))
    return out


def metadata(asm):
    meta, name = {}, None
    for line in asm.splitlines():
        m = re.match(r"^\s+\.name:\s+(\S+)", line)
        if m:
            name = m.group(1)
            meta.setdefault(name, {})
            continue
        m = re.match(r"^\s+\.(vgpr_count|sgpr_count|sgpr_spill_count|vgpr_spill_count|private_segment_fixed_size):\s+(\d+)", line)
        if m and name:
            meta[name][m.group(1)] = int(m.group(2))
    return meta


def summary(ins):
    cnt = collections.Counter(c for c, _, _ in ins)
    idx = [k for k, (c, _, _) in enumerate(ins) if c == "mfma"]
    runs, prev = 0, None
    if idx:
        for c, _, _ in ins[idx[0]:idx[-1] + 1]:
            if c == "valu" and prev != "valu":
                runs += 1
            if c in ("valu", "mfma"):
                prev = c
    ops = collections.Counter(op for c, op, _ in ins if c == "valu")
    return cnt, runs, ops


def report(asm, show_blocks=False):
    meta = metadata(asm)
    for name, blocks in kernels(asm).items():
        print("== %s" % name)
        print("   metadata: %s" % ", ".join("%s=%d" % kv for kv in sorted(meta.get(name, {}).items())))
        if show_blocks:
            for label, depth, ins, _ in blocks:
                cnt = collections.Counter(c for c, _ in ins)
                if ins:
                    print("   %-12s depth %d  %s" % (label, depth, "  ".join("%s %3d" % (c, cnt[c]) for c in CLASSES if cnt[c])))
        # chunk bodies: every depth-2 loop (by its header), and the pieces of the depth-1 stream between two s_barrier that hold MFMAs
        loops, pieces, cur = collections.OrderedDict(), [], []
        for label, depth, ins, header in blocks:
            if depth >= 2:
                loops.setdefault(header, []).extend((c, op, depth) for c, op in ins)
            elif depth == 1:
                for c, op in ins:
                    cur.append((c, op, depth))
                    if op == "s_barrier":
                        pieces.append(cur)
                        cur = []
        pieces.append(cur)
        item = []
        for title, body in [("chunk loop %s" % h, b) for h, b in loops.items()] + [("peeled chunk (depth 1)", p) for p in pieces]:
            if any(c == "mfma" for c, _, _ in body):
                cnt, runs, ops = summary(body)
                print("   %-40s %s" % (title, "  ".join("%s %4d" % (c, cnt[c]) for c in CLASSES)))
                print("   %-40s VALU runs between its first and last MFMA: %d; VALU by opcode: %s"
                      % ("", runs, ", ".join("%s %d" % kv for kv in ops.most_common(6))))
            else:
                item += body
        cnt, _, ops = summary(item)
        print("   %-40s %s" % ("item code between the chunks (depth 1)", "  ".join("%s %4d" % (c, cnt[c]) for c in CLASSES)))
        print("   %-40s VALU by opcode: %s" % ("", ", ".join("%s %d" % kv for kv in ops.most_common(8))))


if __name__ == "__main__":
    args = sys.argv[1:]
    dev = "--dev" in args
    show = "--blocks" in args
    src = source = None
    if "--asm" in args:
        src = args[args.index("--asm") + 1]
        args.remove(src)
    if "--source" in args:
        source = args[args.index("--source") + 1]
        args.remove(source)
    extra = [a for a in args if a not in ("--dev", "--blocks", "--asm", "--source")]
    text = open(src).read() if src else compile_asm(dev, extra, source)
    report(text, show)
