#!/usr/bin/env python3
"""SGPRs parked in VGPR lanes: the v_readlane_b32 / v_writelane_b32 of every kernel of an ISA file.

  python tools/lane_moves.py obj/sdirt_psf-hip-amdgcn-amd-amdhsa-gfx950.s [other.s] [--kernel PATTERN] [--blocks]

When a kernel needs more SGPRs than its occupancy allows, the register allocator spills them into lanes of a
VGPR: a v_writelane_b32 where the value is parked, a v_readlane_b32 (and an s_nop before the scalar unit may use
it) where it comes back.  Both are vector instructions that compute nothing; inside a sample loop they are paid
per ray.  For each kernel (those whose mangled name contains PATTERN) this prints

  the static number of both mnemonics,
  those in blocks the compiler annotates as part of a loop (`in Loop:` / `Loop Header:`), with the deepest level,
  the register totals of the kernel's resource comment (SGPRs, VGPRs, scratch, occupancy),

and with --blocks every block that holds one, with its loop header and depth.  Given a second ISA file (the same
translation unit from another build) the two are printed side by side.  A report, not a gate.
"""
import argparse
import re
import sys
from collections import OrderedDict

LABEL = re.compile(r"^\.(LBB\d+_\d+):")
FALL = re.compile(r"^\s*; %bb\.(\d+):")
IN_LOOP = re.compile(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)")
HEADER = re.compile(r"This (?:Inner )?Loop Header: Depth=(\d+)")
TOTALS = OrderedDict((("sgpr", r";\s*TotalNumSgprs:\s*(\d+)"), ("vgpr", r";\s*NumVgprs:\s*(\d+)"),
                      ("scratch", r";\s*ScratchSize:\s*(\d+)"), ("occ", r";\s*Occupancy:\s*(\d+)")))


def kernels(lines):
    """-> OrderedDict name -> (body lines, resource comment lines)"""
    out = OrderedDict()
    starts = [i for i, l in enumerate(lines) if re.match(r"^_Z\S+:\s*; @", l) or re.match(r"^[A-Za-z_]\w*:\s*; @", l)]
    for n, i in enumerate(starts):
        end = starts[n + 1] if n + 1 < len(starts) else len(lines)
        name = lines[i].split(":")[0]
        stop = next((j for j in range(i, end) if lines[j].strip().startswith("s_endpgm")), None)
        if stop is None:
            continue                      # a device function, not a kernel
        # the last s_endpgm of the kernel: the resource comment follows .Lfunc_end
        fe = next((j for j in range(stop, end) if lines[j].startswith(".Lfunc_end")), end)
        out[name] = (lines[i:fe], lines[fe:end])
    return out


def blocks(body):
    """-> list of [block label, loop header or None, depth, readlanes, writelanes]"""
    out = [["entry", None, 0, 0, 0]]
    i = 0
    while i < len(body):
        l = body[i]
        m = LABEL.match(l) or FALL.match(l)
        if m:
            label = m.group(1) if l.startswith(".") else "bb." + m.group(1)
            note = l
            while i + 1 < len(body) and re.match(r"^\s+;\s", body[i + 1]) and "Loop" in body[i + 1]:
                i += 1
                note += body[i]
            h, inl = HEADER.search(note), IN_LOOP.search(note)
            if h:
                out.append([label, label[1:] if label.startswith("L") else label, int(h.group(1)), 0, 0])
            elif inl:
                out.append([label, inl.group(1), int(inl.group(2)), 0, 0])
            else:
                out.append([label, None, 0, 0, 0])
        else:
            t = l.strip()
            if t.startswith("v_readlane_b32"):
                out[-1][3] += 1
            elif t.startswith("v_writelane_b32"):
                out[-1][4] += 1
        i += 1
    return out


def report(path, pattern):
    lines = open(path).read().splitlines()
    rows = OrderedDict()
    for name, (body, tail) in kernels(lines).items():
        if pattern and pattern not in name:
            continue
        bl = blocks(body)
        tot = {}
        for key, rx in TOTALS.items():
            m = next((re.search(rx, l) for l in tail if re.search(rx, l)), None)
            tot[key] = int(m.group(1)) if m else -1
        # keyed without the parameter list: an instantiation keeps its row when the kernel's signature changes
        rows[short(name, 1 << 20)] = dict(rd=sum(b[3] for b in bl), wr=sum(b[4] for b in bl),
                          rd_loop=sum(b[3] for b in bl if b[2] > 0), wr_loop=sum(b[4] for b in bl if b[2] > 0),
                          deep=max([b[2] for b in bl if b[3] + b[4] > 0] + [0]), blocks=[b for b in bl if b[3] + b[4] > 0],
                          **tot)
    return rows


def cell(r):
    if r is None:
        return f"{'-':>40}"
    return (f"{r['rd']:>5}{r['wr']:>5} |{r['rd_loop']:>5}{r['wr_loop']:>5}{r['deep']:>4} |"
            f"{r['sgpr']:>4}{r['vgpr']:>5}{r['scratch']:>5}{r['occ']:>3}")


def short(name, width):
    # the template arguments are what tells instantiations apart: drop the parameter list
    m = re.match(r"^(_Z\d+\w+?I.*?E)Ev", name)
    s = m.group(1) if m else name
    return s if len(s) <= width else s[:width - 1] + "~"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("asm")
    ap.add_argument("other", nargs="?", help="the same translation unit from another build, printed beside the first")
    ap.add_argument("--kernel", default="", help="only kernels whose mangled name contains this")
    ap.add_argument("--blocks", action="store_true", help="list every block that holds a lane move")
    args = ap.parse_args()
    a = report(args.asm, args.kernel)
    b = report(args.other, args.kernel) if args.other else None
    head = f"{'rdln':>5}{'wrln':>5} |{'rd':>5}{'wr':>5}{'dep':>4} |{'sgpr':>4}{'vgpr':>5}{'scr':>5}{'oc':>3}"
    sub = f"{'static':>10} |{'in loops':>14} |{'registers':>17}"
    w = 58
    print(f"{'':<{w}}{sub}" + (f"   {sub}" if b is not None else ""))
    print(f"{'kernel':<{w}}{head}" + (f"   {head}" if b is not None else ""))
    names = list(a) + [n for n in (b or {}) if n not in a]
    for n in names:
        ra, rb = a.get(n), (b.get(n) if b is not None else None)
        if not args.kernel and not any(r and (r["rd"] or r["wr"]) for r in (ra, rb)):
            continue
        print(f"{short(n, w - 1):<{w}}{cell(ra)}" + (f"   {cell(rb)}" if b is not None else ""))
        if args.blocks:
            for tag, r in (("", ra), ("other ", rb)):
                for lab, hdr, dep, rd, wr in (r["blocks"] if r else []):
                    where = f"in loop {hdr} depth {dep}" if dep else "outside every loop"
                    print(f"    {tag}{lab:<14}{rd:>4} readlane{wr:>4} writelane   {where}")
    ta = (sum(r["rd"] for r in a.values()), sum(r["wr"] for r in a.values()),
          sum(r["rd_loop"] for r in a.values()), sum(r["wr_loop"] for r in a.values()))
    line = f"total of {len(a)} kernels: {ta[0]} readlane, {ta[1]} writelane, of them in loops {ta[2]} + {ta[3]}"
    if b is not None:
        tb = (sum(r["rd"] for r in b.values()), sum(r["wr"] for r in b.values()),
              sum(r["rd_loop"] for r in b.values()), sum(r["wr_loop"] for r in b.values()))
        line += f"   |   other: {tb[0]} readlane, {tb[1]} writelane, in loops {tb[2]} + {tb[3]}"
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
