#!/usr/bin/env python3
"""Instruction-class histogram of one kernel's gfx950 ISA, loop by loop.

  make -C sdirt_amd/csrc        (leaves the device ISA of every translation unit in csrc/obj/)
  python tools/isa_hist.py sdirt_amd/csrc/obj/sdirt_psf-hip-amdgcn-amd-amdhsa-gfx950.s \
         'k_psf_lrILb1ELb0EN5sdirt4LeanELb1' [--json out.json]

Reads the compiler's `.s` (hipcc -S --cuda-device-only), cuts out the kernel whose mangled name
contains the pattern, assigns every instruction to its innermost loop using LLVM's own block
comments ("=>This Loop Header: Depth=N" / "in Loop: Header=BBx_y Depth=N") and counts classes:

  valu        vector ALU, VGPR / inline-constant / literal operands only
  valu_s      vector ALU that reads or writes the scalar file: an SGPR or vcc SOURCE operand,
              v_cmp (writes vcc / an SGPR pair), v_cndmask with an SGPR-pair mask, plus v_med3_*
  cndmask_vcc v_cndmask_b32 with the implicit vcc mask (VOP2)
  valu_trans  v_rcp/v_rsq/v_sqrt/v_sin/v_cos/v_exp/v_log
  valu_f64    fp64 vector ops
  lane        v_readlane / v_writelane / v_readfirstlane (SGPR spill traffic and uniform moves)
  salu, smem (s_load), s_nop, s_waitcnt, branch, vmem, lds

`simd_cyc` prices one pass through the block with the per-SIMD costs MEASURED on gfx950 at 8 waves
per SIMD by tools/form_bench.hip (profiles/r02/form_bench.txt): valu 2.25, valu_s / valu_f64 / lane 4.2,
cndmask_vcc 2.25, valu_trans 8.2, salu / branch / smem / s_waitcnt 2.3, s_nop 1, vmem / lds 2.3 -- an UPPER
estimate of SIMD issue time (in the product the half- and quarter-rate forms hide behind the other
waves: 2.24 cycles per instruction of any kind), not a latency.  The Newton loops are
the innermost loops of the surface loop; their rows are what VERDICT r01 item 3 asks to be tracked.

  python tools/isa_hist.py <asm> <pattern> --path sphere|asphere6 [--trips 2] [--flags 0x..] [--show]

counts what ONE surface visit executes in the last (largest) surface loop of the kernel, outside its trip loops: the
way docs/KERNEL_NOTES.md counts "executed per ray", done by the tool.  The scalar registers are followed from the
visit's prefetch (the s_load_dwordx8 / x4 / dword of surf_issue) once round the loop to the same instruction, with
the flags word and the trip word that the prefetch delivers set to the given surface's, every other register unknown
(known bits are tracked, so the byte of a trip word whose four bytes are equal survives the shift by 8 * (k & 3)).
A branch whose condition is known is followed; one whose condition is not (a lane mask, the loop's own exit, the
"any trip open" test) is walked both ways, paths that leave the loop are dropped, and the shortest and the longest
path are printed.  `exec` counts as non-zero.  --all-valid takes the branches of zero_outside_wave (sdirt_device.hpp:
`s_cbranch_scc1 .Lwave_inside_N` over a v_cndmask) instead of walking both sides: the visit of a wave whose 64 rays
all pass their validity tests.
"""
import argparse
import json
import re
from collections import OrderedDict, defaultdict

# zero_outside_wave (sdirt_device.hpp): `s_cbranch_scc1 .Lwave_inside_N` over a v_cndmask when the wave's lanes all pass
WAVE_LABEL = re.compile(r"^(\.Lwave_inside_\d+):")
ALL_VALID = False                    # --all-valid: --path takes those branches (a wave whose 64 rays are all valid)
TRANS = re.compile(r"^v_(rcp|rsq|sqrt|sin|cos|exp|log)_(f32|f16|legacy)")
F64 = re.compile(r"^v_\w+_f64|^v_cvt_f64|^v_cvt_\w+_f64")


COST = dict(valu=2.25, valu_s=4.2, cndmask_vcc=2.25, valu_trans=8.2, valu_f64=4.2, lane=4.2, salu=2.3,
            smem=2.3, s_nop=1.0, s_waitcnt=2.3, branch=2.3, vmem=2.3, lds=2.3, barrier=2.3, other=2.3)
SREG = re.compile(r"(?<![\w.])(s\d+|s\[\d+:\d+\]|vcc|exec)\b")


def classify(op, text=""):
    c = classify_op(op)
    if c != "valu":
        return c
    args = text.split(None, 1)[1] if " " in text.strip() else ""
    args = args.split(";")[0]
    if op.startswith("v_cndmask"):
        return "valu_s" if SREG.search(args) else "cndmask_vcc"
    if op.startswith("v_cmp") or op.startswith("v_med3") or op.startswith("v_div_scale") or op.startswith("v_div_fmas"):
        return "valu_s"
    return "valu_s" if SREG.search(args) else "valu"


def classify_op(op):
    if op.startswith("v_readlane") or op.startswith("v_writelane") or op.startswith("v_readfirstlane"):
        return "lane"
    if op.startswith("v_"):
        if TRANS.match(op):
            return "valu_trans"
        if F64.match(op):
            return "valu_f64"
        return "valu"
    if op.startswith("s_load") or op.startswith("s_buffer_load"):
        return "smem"
    if op == "s_nop":
        return "s_nop"
    if op.startswith("s_waitcnt"):
        return "s_waitcnt"
    if op.startswith("s_cbranch") or op.startswith("s_branch") or op in ("s_endpgm", "s_setpc_b64"):
        return "branch"
    if op.startswith("s_barrier"):
        return "barrier"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("global_") or op.startswith("buffer_") or op.startswith("flat_") or op.startswith("scratch_"):
        return "vmem"
    if op.startswith("ds_"):
        return "lds"
    return "other"


def kernel_body(lines, pattern):
    start = None
    for i, l in enumerate(lines):
        if l.startswith("_Z") and pattern in l and l.rstrip().split(":")[0].endswith(l.split(":")[0]):
            if re.match(r"^_Z\S+:", l):
                start = i
                break
    if start is None:
        raise SystemExit(f"no kernel matching {pattern!r}")
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith("s_endpgm"))
    return lines[start:end + 1]


def program(body):
    """-> (items, parents): items = [("label", name) | ("ins", text, innermost loop key, depth)] in file order;
    parents[loop key] = the loops around it.  loop key = header label without ".L", or "straight"."""
    items, parents, pending = [], {}, []
    cur, last_label = ("straight", 0), None
    hdr = re.compile(r"^(\.LBB\d+_\d+):")
    for l in body:
        m = WAVE_LABEL.match(l)
        if m:                        # a label inside an inline-asm statement: a branch target, not a block of the compiler's
            items.append(("label", m.group(1)[2:]))
            continue
        m = hdr.match(l)
        if m:
            label = last_label = m.group(1)[2:]
            items.append(("label", label))
            pending = re.findall(r"Parent Loop (BB\d+_\d+)", l)
            d = re.search(r"Loop Header: Depth=(\d+)", l)
            i = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", l)
            if d:
                cur = (label, int(d.group(1)))
                parents[label] = pending
            elif i:
                cur = (i.group(1), int(i.group(2)))
            elif "Parent Loop" not in l:
                cur = ("straight", 0)
            continue
        t = l.strip()
        if t.startswith(";") and "Parent Loop" in l:
            pending = pending + re.findall(r"Parent Loop (BB\d+_\d+)", l)
            continue
        if t.startswith(";") and "Loop Header: Depth=" in l and last_label:       # header of a loop nested in others:
            d = re.search(r"Loop Header: Depth=(\d+)", l)          # the label line names the parents
            cur = (last_label, int(d.group(1)))
            parents[last_label] = pending
            continue
        if t.startswith(";") and "in Loop: Header=" in l:          # "; %bb.N:  ; in Loop: Header=...", or the line
                                                                   # under a label that carries the block's IR name
            i = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", l)
            cur = (i.group(1), int(i.group(2)))
            continue
        if t.startswith("; %bb.") and "in Loop" not in t:
            cur = ("straight", 0)
            continue
        if not t or t.startswith(";") or t.startswith(".") or t.endswith(":"):
            continue
        items.append(("ins", t, cur[0], cur[1]))
    return items, parents


def histogram(body):
    """-> OrderedDict loop_key -> {depth, classes...}; loop_key = header label or 'straight'."""
    loops = OrderedDict()
    for it in program(body)[0]:
        if it[0] != "ins":
            continue
        rec = loops.setdefault(it[2], defaultdict(int))
        rec["depth"] = it[3]
        rec[classify(it[1].split()[0], it[1])] += 1
    return loops


# ---- --path: what one surface visit executes -------------------------------------------------------------------
# The flags word of a surface as sdirt_trace.hip's make_dev_surface builds it (kind | refract | k > -1 | c > 0 |
# 1 + k == 1 | degree << 8, and in bits 12-19 the visit word the kernels dispatch on: sdirt_device.hpp, visit_bits);
# kernels that know nothing of the bits from 12 on mask them away, so one word serves every build.
M32 = 0xffffffff
VISIT = dict(sphere=0x3d | (1 << 13) | (1 << 17), asphere6=0x61e | (1 << 15) | (1 << 16) | (3 << 20))
FULL, NONE = lambda v: (M32, v & M32), (0, 0)
NO_SCC = ("s_mov", "s_movk", "s_cselect", "s_sext", "s_mul", "s_brev", "s_ff1", "s_flbit", "s_cmov", "s_load",
          "s_waitcnt", "s_nop", "s_setprio", "s_barrier", "s_getpc", "s_bitset", "s_sleep", "s_buffer_load")


class Unknown(Exception):
    pass


class State:
    """32-bit scalar registers as (known-bit mask, value); `eq_exec`: 64-bit registers known to hold exec."""

    def __init__(self):
        self.r, self.scc, self.eq_exec = {}, None, set()

    def copy(self):
        s = State()
        s.r, s.scc, s.eq_exec = dict(self.r), self.scc, set(self.eq_exec)
        return s


def _regs(tok):
    """register token -> list of 32-bit register names, or None for a non-register"""
    tok = tok.strip()
    if tok in ("vcc", "exec"):
        return [tok + "_lo", tok + "_hi"]
    if tok in ("vcc_lo", "vcc_hi", "exec_lo", "exec_hi", "m0"):
        return [tok]
    m = re.fullmatch(r"s(\d+)", tok)
    if m:
        return [tok]
    m = re.fullmatch(r"s\[(\d+):(\d+)\]", tok)
    if m:
        return [f"s{i}" for i in range(int(m.group(1)), int(m.group(2)) + 1)]
    return None


def _get32(st, tok):
    tok = tok.strip()
    rg = _regs(tok)
    if rg:
        return st.r.get(rg[0], NONE)
    try:
        return FULL(int(tok, 0))
    except ValueError:
        pass
    try:
        import struct
        return FULL(struct.unpack("<I", struct.pack("<f", float(tok)))[0])
    except ValueError:
        return NONE


def _get64(st, tok):
    """-> ("exec",) | (mask64, val64)"""
    tok = tok.strip()
    rg = _regs(tok)
    if rg and len(rg) == 2:
        if tok == "exec" or rg[0] in st.eq_exec:
            return ("exec",)
        lo, hi = st.r.get(rg[0], NONE), st.r.get(rg[1], NONE)
        return (lo[0] | hi[0] << 32, lo[1] | hi[1] << 32)
    v = int(tok, 0)
    return ((1 << 64) - 1, v & ((1 << 64) - 1))


def _set(st, tok, val, wide=False):
    rg = _regs(tok) or []
    for x in rg:
        st.eq_exec.discard(x)
    if wide and len(rg) == 2:
        if val == ("exec",):
            st.r[rg[0]] = st.r[rg[1]] = NONE
            st.eq_exec.add(rg[0])
            return
        st.r[rg[0]] = (val[0] & M32, val[1] & M32)
        st.r[rg[1]] = (val[0] >> 32, val[1] >> 32)
        return
    for i, x in enumerate(rg):
        st.r[x] = val if i == 0 and len(rg) == 1 else NONE


def _full(a):
    return a[0] == M32


def _signed(v):
    return v - (1 << 32) if v & 0x80000000 else v


def _shift(a, b, f):
    """a shifted by the low five bits of b, b partly known: the bits on which every possible amount agrees"""
    cands = [n for n in range(32) if (n & b[0] & 31) == (b[1] & 31)]
    outs = [f(a, n) for n in cands]
    m, v = outs[0]
    for om, ov in outs[1:]:
        m &= om & ~(v ^ ov)
    return (m & M32, v & m & M32)


def step_scalar(st, op, args):
    """One scalar (or SGPR-writing vector) instruction on the state.  Returns nothing; unknown results are unknown."""
    a = [x.strip() for x in args.split(",")] if args else []
    base = op.rsplit("_", 1)[0] if re.search(r"_(b32|b64|u32|i32|u64|i8|i16)$", op) else op
    writes_scc = not op.startswith(NO_SCC)
    scc = None
    try:
        if op.startswith("v_"):                        # a compare, v_readfirstlane: an unknown value in its SGPRs
            if a and _regs(a[0]):
                for q in _regs(a[0]):
                    st.eq_exec.discard(q)
                    st.r[q] = NONE
            return
        if op in ("s_mov_b32", "s_movk_i32"):
            _set(st, a[0], _get32(st, a[1]))
        elif op == "s_mov_b64":
            _set(st, a[0], _get64(st, a[1]), True)
        elif op in ("s_and_b32", "s_or_b32", "s_andn2_b32", "s_xor_b32", "s_orn2_b32"):
            (xm, xv), (ym, yv) = _get32(st, a[1]), _get32(st, a[2])
            if "n2" in op:
                yv = ~yv & ym & M32
            if op.startswith("s_and"):
                m = (xm & ym) | (xm & ~xv) | (ym & ~yv)
                v = xv & yv
            elif op.startswith("s_or"):
                m = (xm & ym) | (xm & xv) | (ym & yv)
                v = (xv | yv)
            else:
                m, v = xm & ym, xv ^ yv
            m &= M32
            _set(st, a[0], (m, v & m))
            scc = (v & m) != 0 if m == M32 or (v & m) else None
        elif op in ("s_and_b64", "s_or_b64", "s_andn2_b64", "s_xor_b64", "s_orn2_b64"):
            x, y = _get64(st, a[1]), _get64(st, a[2])
            full = (1 << 64) - 1
            res = None
            if op == "s_andn2_b64" and x == ("exec",) and y != ("exec",) and y[0] == full:
                res = (full, 0) if y[1] == full else ("exec",) if y[1] == 0 else None
            elif op == "s_and_b64" and ("exec",) in (x, y):
                o = y if x == ("exec",) else x
                if o == ("exec",) or (o[0] == full and o[1] == full):
                    res = ("exec",)
                elif o[0] == full and o[1] == 0:
                    res = (full, 0)
            elif op == "s_or_b64" and ("exec",) in (x, y):
                o = y if x == ("exec",) else x
                if o == ("exec",) or (o[0] == full and o[1] == 0):
                    res = ("exec",)
            elif x != ("exec",) and y != ("exec",) and x[0] == full and y[0] == full:
                yy = ~y[1] & full if "n2" in op else y[1]
                res = (full, x[1] & yy if op.startswith("s_and") else x[1] | yy if op.startswith("s_or") else x[1] ^ yy)
            if res is None:
                _set(st, a[0], NONE)
                for x in _regs(a[0]):
                    st.r[x] = NONE
            else:
                _set(st, a[0], res, True)
                scc = True if res == ("exec",) else res[1] != 0
        elif op in ("s_add_i32", "s_add_u32", "s_sub_i32", "s_sub_u32", "s_addk_i32", "s_mul_i32", "s_min_i32",
                    "s_max_i32", "s_min_u32", "s_max_u32"):
            x, y = (_get32(st, a[0]), _get32(st, a[1])) if op == "s_addk_i32" else (_get32(st, a[1]), _get32(st, a[2]))
            if _full(x) and _full(y):
                if "add" in op:
                    t = x[1] + y[1]
                    scc = t > M32 if op.endswith("u32") else not (-(1 << 31) <= _signed(x[1]) + _signed(y[1]) < (1 << 31))
                elif "sub" in op:
                    t = x[1] - y[1]
                    scc = t < 0 if op.endswith("u32") else not (-(1 << 31) <= _signed(x[1]) - _signed(y[1]) < (1 << 31))
                elif "mul" in op:
                    t = x[1] * y[1]
                else:
                    sx, sy = (_signed(x[1]), _signed(y[1])) if op.endswith("i32") else (x[1], y[1])
                    t = min(sx, sy) if "min" in op else max(sx, sy)
                    scc = t == sx
                _set(st, a[0], FULL(t))
            else:
                _set(st, a[0], NONE)
        elif op in ("s_lshl_b32", "s_lshr_b32", "s_ashr_i32"):
            x, y = _get32(st, a[1]), _get32(st, a[2])
            if op == "s_lshl_b32":
                f = lambda q, n: (((q[0] << n) | ((1 << n) - 1)) & M32, (q[1] << n) & M32)
            elif op == "s_lshr_b32":
                f = lambda q, n: ((q[0] >> n) | (M32 & ~(M32 >> n)), q[1] >> n)
            else:
                def f(q, n):
                    top = (M32 & ~(M32 >> n))
                    if q[0] & 0x80000000:
                        return ((q[0] >> n) | top, (q[1] >> n) | (top if q[1] & 0x80000000 else 0))
                    return ((q[0] >> n) & ~top & M32, q[1] >> n)
            r = _shift(x, y, f)
            _set(st, a[0], r)
            scc = (r[1] != 0) if _full(r) or r[1] else None
        elif op in ("s_bfe_u32", "s_bfe_i32"):
            x, y = _get32(st, a[1]), _get32(st, a[2])
            if not _full(y):
                raise Unknown
            off, wid = y[1] & 31, (y[1] >> 16) & 0x7f
            fm = ((1 << wid) - 1)
            m, v = ((x[0] >> off) & fm) | (M32 & ~fm), (x[1] >> off) & fm
            if op == "s_bfe_i32" and wid:
                if (x[0] >> off) >> (wid - 1) & 1:
                    v |= (M32 & ~fm) if v >> (wid - 1) & 1 else 0
                else:
                    m &= fm >> 1
            _set(st, a[0], (m & M32, v & m & M32))
            scc = (v & m) != 0 if (m & M32) == M32 or (v & m) else None
        elif op in ("s_sext_i32_i8", "s_sext_i32_i16"):
            w = 8 if op.endswith("i8") else 16
            x = _get32(st, a[1])
            fm = (1 << w) - 1
            if x[0] >> (w - 1) & 1:
                _set(st, a[0], ((x[0] & fm) | (M32 & ~fm), (x[1] & fm) | ((M32 & ~fm) if x[1] >> (w - 1) & 1 else 0)))
            else:
                _set(st, a[0], (x[0] & (fm >> 1), x[1] & (fm >> 1)))
        elif op == "s_abs_i32":
            x = _get32(st, a[1])
            if not _full(x):
                raise Unknown
            _set(st, a[0], FULL(abs(_signed(x[1]))))
            scc = x[1] != 0
        elif op in ("s_bitcmp0_b32", "s_bitcmp1_b32"):
            x, y = _get32(st, a[0]), _get32(st, a[1])
            if _full(y) and x[0] >> (y[1] & 31) & 1:
                scc = ((x[1] >> (y[1] & 31)) & 1) == (1 if op == "s_bitcmp1_b32" else 0)
        elif op.startswith("s_cmp_") or op.startswith("s_cmpk_"):
            kind, ty = op.split("_")[2], op.split("_")[3]
            if ty == "u64":
                x, y = _get64(st, a[0]), _get64(st, a[1])
                if ("exec",) in (x, y):
                    if x == y:
                        eq = True
                    else:
                        o = y if x == ("exec",) else x
                        eq = False if o[0] == (1 << 64) - 1 and o[1] == 0 else None
                else:
                    diff = x[0] & y[0] & (x[1] ^ y[1])
                    eq = False if diff else True if x[0] == y[0] == (1 << 64) - 1 else None
                scc = None if eq is None else eq if kind == "eq" else not eq
            else:
                x, y = _get32(st, a[0]), _get32(st, a[1])
                if kind in ("eq", "lg"):
                    diff = x[0] & y[0] & (x[1] ^ y[1])
                    eq = False if diff else True if _full(x) and _full(y) else None
                    scc = None if eq is None else eq if kind == "eq" else not eq
                elif _full(x) and _full(y):
                    p, q = (_signed(x[1]), _signed(y[1])) if ty == "i32" else (x[1], y[1])
                    scc = dict(lt=p < q, le=p <= q, gt=p > q, ge=p >= q)[kind]
                elif ty == "u32" and _full(y) and kind in ("lt", "gt", "le", "ge"):
                    # a bound decides it when the unknown bits cannot reach across
                    lo, hi = x[1], x[1] | (~x[0] & M32)
                    q = y[1]
                    for c, fn in (("lt", lambda p: p < q), ("le", lambda p: p <= q), ("gt", lambda p: p > q), ("ge", lambda p: p >= q)):
                        if kind == c and fn(lo) == fn(hi):
                            scc = fn(lo)
        elif op in ("s_cselect_b32", "s_cselect_b64"):
            wide = op.endswith("b64")
            x, y = (_get64 if wide else _get32)(st, a[1]), (_get64 if wide else _get32)(st, a[2])
            if st.scc is not None:
                _set(st, a[0], x if st.scc else y, wide)
            elif x == y and (x == ("exec",) or x[0] == ((1 << 64) - 1 if wide else M32)):
                _set(st, a[0], x, wide)
            else:
                _set(st, a[0], NONE)
                for q in _regs(a[0]):
                    st.r[q] = NONE
        elif op == "s_addc_u32":
            _set(st, a[0], NONE)
        else:
            raise Unknown
    except (Unknown, IndexError, ValueError):
        if a and _regs(a[0]) and not (op.startswith("s_cmp") or op.startswith("s_bitcmp") or op.startswith("s_waitcnt")):
            _set(st, a[0], NONE)
            for q in _regs(a[0]):
                st.r[q] = NONE
        if op.endswith("saveexec_b64"):
            pass
        scc = None
    if writes_scc:
        st.scc = scc


def visit_path(body, flags, trips, show=False, loop=None):
    items, parents = program(body)
    where = {it[1]: i for i, it in enumerate(items) if it[0] == "label"}
    # the surface loop: the loop with the most instructions among those that hold child loops and a prefetch
    inside = lambda key, L: key == L or L in parents.get(key, [])
    size = defaultdict(int)
    kids = defaultdict(set)
    for key, ps in parents.items():
        for p in ps:
            kids[p].add(key)
    for it in items:
        if it[0] == "ins":
            size[it[2]] += 1
    cands = [k for k in kids if any(it[0] == "ins" and it[2] == k and it[1].startswith("s_load_dwordx8") for it in items)
             and parents.get(k)]
    if loop is None:
        loop = max(cands, key=lambda k: (size[k], list(where).index(k) if k in where else 0))
        loop = [k for k in cands if size[k] == size[loop]][-1]
    start = next(i for i, it in enumerate(items) if it[0] == "ins" and it[2] == loop and it[1].startswith("s_load_dwordx8"))
    tw = (trips & 0xff) * 0x01010101
    # lap 1, uncounted: from the prefetch round to the prefetch with nothing known but what it delivers; what every
    # such path agrees on (the delivered words, now the CURRENT surface's) is the state lap 2 starts from
    laps = walk(items, where, inside, loop, start, State(), flags, tw, False)
    if not laps:
        raise SystemExit("--path: no path comes back to the prefetch")
    st0 = laps[0][2]
    for _, _, st in laps[1:]:
        st0.r = {k: v for k, v in st0.r.items() if st.r.get(k) == v}
        st0.eq_exec &= st.eq_exec
    st0.scc = None
    done = walk(items, where, inside, loop, start, st0, flags, tw, show)
    if not done:
        raise SystemExit("--path: no path comes back to the prefetch")
    return loop, done


def walk(items, where, inside, loop, start, st_in, flags, tw, show):
    done, todo = [], [(start, st_in.copy(), defaultdict(int), [], True)]
    forks = 0
    while todo:
        pc, st, cnt, trace, first = todo.pop()
        hops = 0
        while True:
            it = items[pc]
            if it[0] == "label":
                pc += 1
                continue
            text, key = it[1], it[2]
            if not inside(key, loop):
                break                                   # left the loop: not a visit
            if pc == start and not first:
                done.append((cnt, trace, st))
                break
            first = False
            hops += 1
            if hops > 20000:
                raise SystemExit("--path: a path does not come back to the prefetch")
            op = text.split()[0]
            args = text.split(None, 1)[1].split(";")[0] if " " in text else ""
            if key == loop:
                cnt[classify(op, text)] += 1
                if show:
                    trace = trace + [text]
            if op.startswith("s_load_dwordx8"):
                dst = _regs(args.split(",")[0])
                _set(st, args.split(",")[0], NONE)
                for q in dst:
                    st.r[q] = NONE
                if args.split(",")[-1].strip() in ("0x0", "0"):
                    st.r[dst[0]] = FULL(flags)
                pc += 1
                continue
            if op == "s_load_dword":
                _set(st, args.split(",")[0], FULL(tw))
                pc += 1
                continue
            if op in ("s_branch",):
                pc = where[args.strip()[2:]]
                continue
            if op.startswith("s_cbranch"):
                tgt = where[args.strip()[2:]]
                cond = op.split("_")[2]
                if ALL_VALID and args.strip().startswith(".Lwave_inside_"):
                    take = True
                elif cond in ("scc0", "scc1"):
                    take = None if st.scc is None else st.scc == (cond == "scc1")
                elif cond in ("vccz", "vccnz"):
                    v = _get64(st, "vcc")
                    nz = True if v == ("exec",) else (v[1] != 0 if v[0] == (1 << 64) - 1 or v[1] else None)
                    take = None if nz is None else nz == (cond == "vccnz")
                else:
                    take = cond == "execnz"
                if take is None:
                    forks += 1
                    if forks > 4096:
                        raise SystemExit("--path: too many branches on unknown conditions")
                    todo.append((tgt, st.copy(), defaultdict(int, cnt), trace, False))
                    pc += 1
                else:
                    pc = tgt if take else pc + 1
                continue
            if op.startswith("s_") or op.startswith("v_"):
                step_scalar(st, op, args)
            pc += 1
    return done


def print_path(args, body):
    flags = int(args.flags, 0) if args.flags else VISIT[args.path]
    loop, done = visit_path(body, flags, args.trips, args.show, args.loop)
    sc = lambda c: c["salu"] + c["branch"]
    done.sort(key=lambda d: sc(d[0]))
    cols = ["salu", "branch", "smem", "s_nop", "s_waitcnt", "valu", "valu_s", "cndmask_vcc", "valu_trans", "valu_f64", "lane"]
    print(f"visit path {args.path} (flags {flags:#x}, {args.trips} trips) in surface loop {loop}, outside the trip loops: "
          f"{len(done)} path(s)")
    for name, (c, trace, _) in (("shortest", done[0]), ("longest", done[-1])):
        print(f"  {name:<9} scalar+branch {sc(c):>4}   " + "  ".join(f"{k} {c[k]}" for k in cols))
    if args.show:
        for t in done[-1][1]:
            if t.startswith("s_") and not t.startswith(("s_nop", "s_waitcnt")):
                print("      " + t)
    return dict(loop=loop, flags=flags, trips=args.trips, shortest=dict(done[0][0]), longest=dict(done[-1][0]),
                scalar_branch=[sc(done[0][0]), sc(done[-1][0])])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--path", choices=sorted(VISIT), help="count one visit of this surface class instead of the histogram")
    ap.add_argument("--trips", type=int, default=2, help="--path: the visit's entry of the trip table, 0 to 4: a fixed table and the plain loop (what a trip of the "
                    "periodic or of an adaptive loop leaves of the count is not known here, and the walk gives up)")
    ap.add_argument("--flags", help="--path: the surface's flags word, if not the class's usual one")
    ap.add_argument("--loop", help="--path: the surface loop's header (BBn_m) if not the kernel's last one")
    ap.add_argument("--show", action="store_true", help="--path: list the scalar instructions of the longest path")
    ap.add_argument("--all-valid", action="store_true", help="--path: every lane of the wave passes its validity tests: the "
                    "branches over the selects that are then the identity are taken (without it they fork)")
    ap.add_argument("asm")
    ap.add_argument("pattern")
    ap.add_argument("--json")
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    global ALL_VALID
    ALL_VALID = args.all_valid
    body = kernel_body(open(args.asm).read().splitlines(), args.pattern)
    if args.path:
        out = print_path(args, body)
        if args.json:
            with open(args.json, "w") as f:
                json.dump(out, f, indent=1)
        return
    loops = histogram(body)
    cols = ["valu", "valu_s", "cndmask_vcc", "valu_trans", "valu_f64", "lane", "salu", "smem", "s_nop",
            "s_waitcnt", "branch", "vmem", "lds"]
    total = defaultdict(int)
    print(f"{'loop':<10}{'depth':>6}" + "".join(f"{c[:9]:>10}" for c in cols) + f"{'simd_cyc':>10}")
    out = {"kernel_pattern": args.pattern, "label": args.label, "cost_per_instr": COST, "loops": {}}
    for k, rec in loops.items():
        cyc = round(sum(COST[c] * rec[c] for c in cols), 1)
        print(f"{k:<10}{rec['depth']:>6}" + "".join(f"{rec[c]:>10}" for c in cols) + f"{cyc:>10}")
        out["loops"][k] = dict(depth=rec["depth"], simd_cycles=cyc, **{c: rec[c] for c in cols})
        for c in cols:
            total[c] += rec[c]
    print(f"{'TOTAL':<10}{'':>6}" + "".join(f"{total[c]:>10}" for c in cols))
    out["total_static"] = dict(total)
    for l in body:
        m = re.search(r"; (NumSgprs|NumVgprs|ScratchSize|Occupancy|SGPRBlocks|LDSByteSize): (\d+)", l)
        if m:
            out[m.group(1)] = int(m.group(2))
    spills = sum(1 for l in body if "SGPR spill to VGPR lane" in l)
    out["sgpr_spill_vgprs"] = spills
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
